// mskf_internal.h — private definitions of the C-ABI handles (mskf_ctx / mskf_stream) and what its files share: mskf_capi_ctx.cpp (contexts,
// marks, waits, staging copies, timing, streams), _fe.cpp (settings, push, track, device frame), _kf.cpp (describe, match, verify), _ekf.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../../include/mskf_hip.h"
#include "../hip/fe_device.h"
#include "../hip/fe_book.h"
#include "../hip/fe_equalize.h"
#include "../hip/fe_pixfmt.h"
#include "../hip/fe_mask.h"
#include "../hip/fe_patch.h"
#include "../hip/fe_fb.h"
#include "../hip/fe_cam_models.h"
#include "../hip/fe_deep.h"
#include "../hip/fe_brief.h"
#include "../hip/fe_match.h"
#include "../hip/fe_verify.h"
#include "../hip/ekf_device.h"
#include "host_math.h"

struct Pyr3Job { const uint8_t *src; uint8_t *d1, *d2, *d3; int w0, h0; };      // one image: level 0 in, levels 1..3 out (fe_kernels.hip)

extern "C" {
void fe_launch_pyr_down3(const Pyr3Job *jobs_dev, int n_jobs, int max_w0, int max_h0, hipStream_t st);
// Host wait for everything queued on the context's stream.  MSKF_WAIT=block (default when the process runs
// more waiting host threads than it has cores to spin on) parks the thread on an interrupt-driven event instead of
// spinning in hipStreamSynchronize, leaving the core to the other groups' host phases.
int mskf_wait(mskf_ctx *c);
void fe_launch_detect(const FeStreamDev *streams_dev, int n_streams, int max_w, int max_h, unsigned int gen, hipStream_t st);
void fe_launch_track(const FeStreamDev *streams_dev, int n_streams, int max_pts, hipStream_t st);
// extended camera models (fe_cam_models.h): cams_dev[i] goes with streams_dev[i]; the extended instantiation of the track kernel
void fe_launch_track_ext(const FeStreamDev *streams_dev, const FeCamExtDev *cams_dev, int n_streams, int max_pts, hipStream_t st);
// deeper LK pyramids (fe_deep.h): the levels 4 and up of the deep streams' images behind fe_launch_pyr_down3; the deep instantiations of
// the track kernel and of the forward-backward gate, deep_dev[i] beside streams_dev[i]
void fe_launch_pyr_down_deep(const DeepPyrJob *jobs_dev, int n_jobs, hipStream_t st);
void fe_launch_track_deep(const FeStreamDev *streams_dev, const FeCamExtDev *cams_dev, const FeDeepDev *deep_dev, int n_streams, int max_pts, hipStream_t st);
void fe_launch_fb_points_deep(const FeStreamDev *streams_dev, const FeFbDev *fb_dev, const FeDeepDev *deep_dev, int n_streams, int max_pts, hipStream_t st);
// image masks (fe_mask.h): masks_dev[i] goes with streams_dev[i]
void fe_launch_detect_masked(const FeStreamDev *streams_dev, const FeMaskDev *masks_dev, int n_streams, int max_w, int max_h, unsigned int gen, hipStream_t st);
void fe_launch_mask_points(const FeStreamDev *streams_dev, const FeMaskDev *masks_dev, int n_streams, int max_pts, hipStream_t st);
// patch check (fe_patch.h): patch_dev[i] goes with streams_dev[i]
void fe_launch_patch_points(const FeStreamDev *streams_dev, const FePatchDev *patch_dev, int n_streams, int max_pts, hipStream_t st);
// forward-backward check (fe_fb.h): fb_dev[i] goes with streams_dev[i]; the grid of fe_launch_track
void fe_launch_fb_points(const FeStreamDev *streams_dev, const FeFbDev *fb_dev, int n_streams, int max_pts, hipStream_t st);
// descriptors (fe_brief.h): jobs of any size and count in one launch; max_pts = the largest count
void fe_launch_describe(const FeDescribeDev *jobs_dev, int n_jobs, int max_pts, hipStream_t st);
// descriptor matching (fe_match.h): jobs of any size and count in one launch, cross-checked or not; max_nq / max_nt = the largest counts
void fe_launch_match(const FeMatchDev *jobs_dev, int n_jobs, int max_nq, int max_nt, hipStream_t st);
// geometric verification (fe_verify.h): jobs of any n and K in one launch; max_K = the largest hypothesis count
void fe_launch_verify(const FeVerifyDev *jobs_dev, int n_jobs, int max_K, hipStream_t st);
extern "C" int fe_mark_slots_used(const struct mskf_ctx *ctx);               // internal, for the tests: not in include/mskf_hip.h
extern "C" size_t fe_verify_arena_bytes(const struct mskf_ctx *ctx);      // internal, for the tests: not in include/mskf_hip.h
extern "C" int fe_stream_desc(const struct mskf_stream *s, FeStreamDev *out);   // internal, for the tests: not in include/mskf_hip.h
void fe_launch_book(const FeBookDev *books_dev, int n_streams, int which, size_t scratch_bytes, hipStream_t st);
void fe_launch_equalize(const EqJob *jobs_dev, int n_jobs, int max_units, int any_global, int max_regions, int splits, hipStream_t st);
void fe_launch_px_convert(const PxJob *jobs_dev, int n_jobs, int max_w, int max_h, hipStream_t st);
}

void mskf_set_error(const std::string &s);

#define MSKF_HIPCHK(expr)                                                                            \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess) {                                                                      \
            mskf_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                       \
            return MSKF_ERR_HIP;                                                                     \
        }                                                                                            \
    } while (0)

static inline size_t round_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }      // a: a power of two

template <typename T>
struct PinnedDev {  // a pinned host array with a device twin
    T *h = nullptr, *d = nullptr;
    size_t cap = 0;
    std::vector<std::pair<T *, T *>> retired;      // outgrown buffers, freed with the owner
    // Optional reuse fence, for an arena whose host side no pending batch protects (pred_arena): recorded behind the copy
    // that reads h, synchronised by the next writer before it writes h.
    hipEvent_t fence = nullptr;
    bool fence_pending = false;
    // Growth NEVER frees: hipFree / hipHostFree wait for every stream of the device, and a context that outgrew a staging
    // buffer in the middle of a run stood still until all the other groups' queues were idle (0.3 s in the round-3 bench).
    // The outgrown pair is retired and freed by release(); with doubling that is at most as much again as the final size.
    // Growth therefore needs no stream synchronisation either: work in flight keeps reading and writing the retired pair,
    // and nothing in flight knows the new one.  (What keeps the host from overwriting h under an in-flight reader is the
    // fence or the pending batch that owns the arena, not growth.)
    int ensure(size_t n) {
        if (n <= cap) return MSKF_OK;
        if (h || d) retired.push_back({h, d});
        h = d = nullptr; cap = 0;
        size_t c = n < 16 ? 16 : 2 * n;
        MSKF_HIPCHK(hipHostMalloc((void **)&h, c * sizeof(T), hipHostMallocDefault));
        MSKF_HIPCHK(hipMalloc((void **)&d, c * sizeof(T)));
        cap = c;
        return MSKF_OK;
    }
    int fence_wait() {            // before writing h
        if (!fence_pending) return MSKF_OK;
        MSKF_HIPCHK(hipEventSynchronize(fence));
        fence_pending = false;
        return MSKF_OK;
    }
    int fence_record(hipStream_t st) {   // behind the copy that reads h
        if (!fence) MSKF_HIPCHK(hipEventCreateWithFlags(&fence, hipEventDisableTiming));
        MSKF_HIPCHK(hipEventRecord(fence, st));
        fence_pending = true;
        return MSKF_OK;
    }
    void release() {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        for (auto &r : retired) { if (r.first) (void)hipHostFree(r.first); if (r.second) (void)hipFree(r.second); }
        retired.clear();
        h = d = nullptr; cap = 0;
        if (fence) (void)hipEventDestroy(fence);
        fence = nullptr; fence_pending = false;
    }
};

// A batch between its _begin and its _end (one of each kind per context).  Each kind keeps its own fields around it.
//   mskf_batch_arm:    record the completion mark behind everything the _begin enqueued, then set `active`.
//   mskf_batch_finish: make the context's device current and wait for the mark; `active` is cleared only once the wait
//                      succeeded.  A failed _end (timeout, stream error) leaves the batch pending, since its kernels may still be
//                      using the arenas it owns: _end may be called again, a _begin that needs those arenas is refused,
//                      mskf_ctx_destroy drains the stream.
//                      Timing is collected by the caller (the LK units are known only from the unpacked results).
// A _begin that fails after it has enqueued anything (copy, memset, stream-ordered allocation, launch) synchronises the
// context's stream before it returns the error (DrainOnError): no staged work outlives it, and nothing is left pending.
struct PendingBatch {
    bool active = false;
    hipEvent_t done = nullptr;        // completion-mark slot (mskf_wait_event)
};
int mskf_batch_arm(mskf_ctx *c, PendingBatch &b);
int mskf_batch_finish(mskf_ctx *c, PendingBatch &b);

// A batch that stages through arenas of its own: one job array, one input block and one result block, empty until the first
// call that launches, written by its _begin and read by its _end only (mskf_enqueue_staged below).
template <typename Job, typename In, typename Out>
struct StagedBatch : PendingBatch {
    PinnedDev<Job> jobs;
    PinnedDev<In> in;
    PinnedDev<Out> out;
    int n = 0;
    void release() { jobs.release(); in.release(); out.release(); }      // (the mark's event goes with the other kinds': mskf_ctx_destroy)
};

// Which pending batch owns which arenas of the context (mskf_ctx::pending lists the records):
//   pend_trk, pend_frame   the front-end arenas: desc, what the track pass stages beside it (mask_desc .. deep_desc), jobs, deep_jobs, cell_arena, trk_in / trk_out, book_desc / book_out;
//   pend_upd               ekf_desc, upd_in, upd_out (a feature update or a direct update: one record for both kinds);
//   pend_ro                pred_arena, whose host side its kernel reads and writes (position variances or odometry covariance: one record);
//   pend_dsc, pend_mch,    the jobs / in / out arenas inside the record itself (StagedBatch), which nothing else touches: only a call
//   pend_vfy               of the same kind refuses for it.  A match or verify batch reads no image and no stream, so pushes, frames,
//                          describe batches and updates may run between its _begin and its _end.
// Every _begin and every batch call that writes an arena refuses while the owner is pending: MSKF_ERR_INVALID, and the
// error message names the pending batch.  What each step of such a call may touch:
//   plan    (plan_push, plan_update, a _begin's own checks): reads the context and the streams, makes no HIP call; every
//           refusal comes from here, so a refused call has changed no stream and no context and has enqueued nothing;
//   grow    the arenas' ensure() (a push first waits for the previous push's mark): allocation only;
//   commit  the streams' and the context's own fields (push generation, cell slices, level-0 planes, has_curr);
//   enqueue the arenas, copies and launches, under a DrainOnError; last the mark (mskf_batch_arm), and only behind it what a
//           finished frame rotates (parity, pyramid roles).
enum MskfArenas { MSKF_ARENAS_FE, MSKF_ARENAS_UPDATE, MSKF_ARENAS_PRED };
int mskf_refuse_if_owned(const mskf_ctx *c, MskfArenas which);

// Set `armed` once a _begin has enqueued work; a return while it is still set synchronises the context's stream.
struct DrainOnError {
    hipStream_t st;
    bool armed = false;
    ~DrainOnError() { if (armed) (void)hipStreamSynchronize(st); }     // (its result is ignored: the original error is returned)
};

// What mskf_ekf_update_batch_begin decided about one stream of a batch before it touched anything (plan_update,
// mskf_capi_ekf.cpp); mskf_ekf_update_batch_end finds the stream's results through the output offsets.
struct EkfUpdatePlan {
    int route, na_max;                                // EkfStreamDev::route, ::na_max
    int m_total, n_tri;
    int cnt[3];                                       // features per work list of the feature kernel: [0] wave, [1] small, [2] big class
    int grow_rows;                                    // > 0: the stack does not fit Hs, which grows to this many rows before the batch runs
    size_t clones, feats, obs_clone, obs_z, tri;      // byte offsets of the stream's inputs in upd_in
    size_t o_dx, o_gamma, o_pos, o_rows, o_status;    // ... and of its results in upd_out
};

struct TimingSlot { hipEvent_t a, b; int kind; long long units; };

struct mskf_ctx {
    bool timing = false;
    bool t_gate = true;                          // mskf_ctx_timing_gate: launches begun (and host seconds spent) while it is off are not accounted
    int timing_period = 1;                       // every n-th launch of a kind is timed (mskf_ctx_set_timing)
    long long t_all[MSKF_K_COUNT] = {0};         // launches of a kind since the last reset, timed or not
    double host_s[4] = {0, 0, 0, 0};   // host seconds inside the batched entry points: [0] update pack, [1] update unpack, [2] track pack, [3] track unpack
    std::vector<TimingSlot> t_pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> t_pool;
    double t_ms[MSKF_K_COUNT] = {0};
    long long t_launches[MSKF_K_COUNT] = {0}, t_units[MSKF_K_COUNT] = {0};
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = true;          // false: created by mskf_ctx_create_shared on another context's stream
    PinnedDev<FeStreamDev> desc[3];   // 0: push/detect, 1: track (first track call of a device frame), 2: second track call of a device frame
    // What the track pass stages (plan_track_pass, mskf_capi_fe.cpp): the streams' opt-in settings, element for element beside the
    // descriptors the pass runs over (one array serves both passes of a device frame); each is empty until a stream has the setting.
    PinnedDev<FeMaskDev> mask_desc[2];   // image masks: [0] beside desc[0], the push's (cam0 only, the detector), [1] the track pass's
    PinnedDev<FePatchDev> patch_desc;    // patch checks
    PinnedDev<FeFbDev> fb_desc;          // forward-backward checks
    PinnedDev<FeCamExtDev> cam_desc;     // camera models: staged when a stream has an extended model, or the pass is deep
    PinnedDev<FeDeepDev> deep_desc;      // deeper pyramid levels
    PinnedDev<DeepPyrJob> deep_jobs;     // the deep streams' images of a push (a front-end arena like jobs; empty likewise)
    PinnedDev<FeBookDev> book_desc;   // bookkeeping descriptors of a device frame batch
    PinnedDev<char> book_out;         // what a device frame batch returns: per stream 16 ints + the published grid
    PinnedDev<char> grid_in;          // staging of mskf_fe_set_grid (synchronous: no batch owns it)
    struct PendingFrame : PendingBatch {
        int n = 0; mskf_stream *const *streams = nullptr; struct mskf_fe_frame_args *args = nullptr;
        std::vector<size_t> out_off; int ts1 = -1, ts2 = -1;
    } pend_frame;
    hipEvent_t wait_ev = nullptr;     // mark of mskf_wait
    bool wait_block = false;
    volatile unsigned int *flag_h = nullptr;   // pinned host words the mark kernels write (spinning mode), one per mark slot
    static constexpr int kMarkSlots = 16;      // completion-mark slots: every kind of pending batch and wait_ev claims one at its first use (counted below, beside `pending`)
    unsigned int flag_seq[kMarkSlots] = {0};
    hipEvent_t *flag_slot[kMarkSlots] = {nullptr};
    PinnedDev<char> cell_arena;       // per-cell maximum keys of every stream of the last push batch (one D2H copy)
    PinnedDev<char> trk_in, trk_out;  // input points / results of every stream of a track batch (one copy each way)
    unsigned long long push_gen = 0;
    hipEvent_t cell_ev = nullptr;     // recorded behind the D2H copy of the per-cell maxima of the last push
    bool cell_mark_recorded = false;  // a push has recorded cell_ev: the next push waits for it before it reuses the staging
    bool cell_keys_dirty = true;      // the key array holds bytes no generation tag explains (fresh allocation): clear before use
    PinnedDev<Pyr3Job> jobs;
    PinnedDev<EqJob> eq_jobs;         // the equalising streams' images of a push (a front-end arena like jobs; empty until a stream turns it on)
    PinnedDev<PxJob> px_jobs;         // the converting streams' images of a push (mskf_fe_set_input_format; empty until a stream turns it on)
    PinnedDev<EkfStreamDev> ekf_desc;
    PinnedDev<char> upd_in, upd_out;     // inputs / results of every stream of an update batch (one copy each way)
    PinnedDev<char> pred_arena;          // descriptors + Phi/Q or IMU steps + J of a prediction, clone removal, read-out (fenced)
    std::vector<mskf_stream *> streams;
    // batches between their *_begin and *_end call (PendingBatch)
    struct PendingTrack : PendingBatch {
        int n = 0; const mskf_fe_track_args *args = nullptr;
        std::vector<size_t> in_off, out_off; int ts = -1;      // per stream, written by _begin's planning step; storage reused from call to call
    } pend_trk;
    struct PendingUpdate : PendingBatch {
        bool launched = false; int n = 0; mskf_stream *const *streams = nullptr; mskf_ekf_update_args *args = nullptr;
        std::vector<EkfUpdatePlan> plan;       // per stream, written by _begin's planning step; storage reused from call to call
        // the same slot holds a pending DIRECT update (mskf_ekf_update_direct_batch_begin): the two kinds share the arenas
        bool direct = false; struct mskf_ekf_direct_args *dargs = nullptr;
        std::vector<size_t> d_out;             // direct: byte offset of each stream's results in upd_out
    } pend_upd;
    // descriptors (mskf_fe_describe_batch_*; fe_brief.h): in = the points, out = desc + valid of every stream
    struct PendingDescribe : StagedBatch<FeDescribeDev, char, char> {
        struct mskf_fe_describe_args *args = nullptr;
        std::vector<size_t> out_off;           // per stream: byte offset of its results in out
    } pend_dsc;
    // descriptor matching (mskf_fe_match_batch_*; fe_match.h): in = every distinct descriptor set and validity array, out = the matches of every job
    struct PendingMatch : StagedBatch<FeMatchDev, char, char> {
        struct mskf_fe_match_args *args = nullptr;
        std::vector<size_t> out_off;           // per job: byte offset of its matches in out
    } pend_mch;
    // geometric verification (mskf_fe_verify_batch_*; fe_verify.h): in = the staged usable pairs of every job, out = FV_MAX_BLOCKS keys per job
    struct PendingVerify : StagedBatch<FeVerifyDev, double, unsigned long long> {
        struct mskf_fe_verify_args *args = nullptr;
        std::vector<size_t> in_off;            // per job: where its staged pairs start in `in`, in doubles
        std::vector<std::vector<int>> orig;    // per job: the original index of every staged pair
    } pend_vfy;
    // a read-out of `rec` doubles per stream: 3 = position variances, 48 = odometry covariance (mskf_odom_cov)
    struct PendingReadOut : PendingBatch { int n = 0, rec = 0; double *out = nullptr; size_t desc_bytes = 0; } pend_ro;
    // Every kind of pending batch, once: mskf_ctx_destroy and mskf_ctx_set_wait_mode walk this list, so a new kind is added here
    // and nowhere else (mskf_refuse_if_owned names the owners it knows in messages of their own).
    static constexpr int kPendingKinds = 7;
    PendingBatch *const pending[kPendingKinds] = {&pend_trk, &pend_frame, &pend_upd, &pend_ro, &pend_dsc, &pend_mch, &pend_vfy};
    static_assert(kPendingKinds + 2 <= kMarkSlots, "every kind of pending batch, wait_ev and cell_ev claim a completion-mark slot each");
};
// Completion marks.  mskf_wait_event(c, slot, true) marks the point the context's stream has reached, (.., false) waits
// for that mark.  Spinning mode (default): the mark is a sequence number written into pinned host memory by a stream
// write-value command (or a one-thread kernel), the wait spins on that word in user space (no HIP call inside the wait: hipEventSynchronize / hipStreamSynchronize
// spinning in several threads at once slows every other thread's launches down, measured -25 %).  MSKF_WAIT=block: a
// blocking-sync HIP event, the thread is parked.  `slot` identifies the mark (one per kind of pending batch).
// Staging copies between the library's own pinned host arenas and device memory, enqueued on the context's stream as ONE kernel
// launch for up to MSKF_COPY_SEGS segments (fe_kernels.hip: why not hipMemcpyAsync).  Both ends must be addressable from a
// kernel: device memory or hipHostMalloc'ed memory.  Every copy from or into an arena of the library goes this way;
// hipMemcpy* in the C ABI copies only memory the caller owns (image pushes, mskf_ekf_reset / set_cov / get_cov,
// mskf_ekf_debug_read, mskf_fe_get_level) and the chi-square table of mskf_ekf_stream_init.
struct MskfCopy { void *dst; const void *src; size_t bytes; };
int mskf_copy_async(mskf_ctx *c, const MskfCopy *segs, int n);
int mskf_wait_event(mskf_ctx *c, hipEvent_t *ev_slot, bool record);

// The enqueue step of a batch whose _begin has planned, grown and packed: the input copies, launch() (the kernels, on c->stream),
// the result copy, and last the mark.  The order is the protocol: nothing is pending before everything is enqueued, and a failure
// on the way drains the stream.  What the _end reads of the record (n, args, offsets) the _begin writes before it calls this.
template <typename Launch>
int mskf_enqueue_staged(mskf_ctx *c, PendingBatch &b, const MskfCopy *in, int n_in, Launch launch, const MskfCopy &out) {
    DrainOnError drain{c->stream, true};
    int rc;
    if ((rc = mskf_copy_async(c, in, n_in)) != MSKF_OK) return rc;
    launch();
    if ((rc = mskf_copy_async(c, &out, 1)) != MSKF_OK) return rc;
    MSKF_HIPCHK(hipGetLastError());
    if ((rc = mskf_batch_arm(c, b)) != MSKF_OK) return rc;
    drain.armed = false;
    return MSKF_OK;
}

struct mskf_stream {
    mskf_ctx *ctx = nullptr;
    mskf_ctx *ctx_ekf = nullptr;      // context the mskf_ekf_* calls run on (== ctx unless re-attached)
    mskf_ctx *home_ctx = nullptr;     // the context the stream was created on (its bookkeeping list); ctx / ctx_ekf may move (mskf_stream_rebind)
    mskf_calib calib;
    mskf_fe_cfg fe;
    mskf_ekf_cfg ekf;
    // ---- front-end
    int w = 0, h = 0;
    int lw[MSKF_LEVELS], lh[MSKF_LEVELS];
    size_t lvl_off[MSKF_LEVELS];
    size_t pyr_bytes = 0;
    uint8_t *pyr[3] = {nullptr, nullptr, nullptr};
    const uint8_t *lvl0[3] = {nullptr, nullptr, nullptr};   // level 0 of each pyramid: own buffer or a borrowed device image
    int i_prev0 = 0, i_curr0 = 1, i_curr1 = 2;
    bool has_curr = false;
    bool held[3] = {false, false, false};   // pyr[i] (or lvl0[i]) holds an image a push has enqueued (mskf_fe_describe refuses a role without one)
    int pt_cap = 0;
    size_t cell_off = 0;              // slice of ctx->cell_arena
    unsigned long long push_gen = 0;
    CamDev cam0, cam1;
    double R01[9], E[9], epi_thresh = 0;
    int det_cw = 0, det_ch = 0;
    int det_floor = 0;                // mskf_fe_set_detect_floor
    double time_stamp = 0;
    // ---- opt-in equalisation of pushed level-0 images (mskf_fe_set_equalize; fe_equalize.h)
    struct Equalize {
        mskf_fe_equalize cfg{0, 8, 8, 0, 40.0};
        EqGeom geom{};                             // mode 2
        int clip = 0, strip_rows = 0, n_strips = 0;
        char *mem = nullptr;                       // one allocation: the LUTs of both cameras, then (mode 1) their partial histograms
        uint8_t *lut[2] = {nullptr, nullptr};
        int *part[2] = {nullptr, nullptr};
    } eq;
    // ---- opt-in input pixel format (mskf_fe_set_input_format; fe_pixfmt.h)
    struct PixFmt {
        mskf_fe_input_format cfg{0, 0};
        int bpp = 1;
        uint8_t *raw = nullptr;                    // raw staging of host pushes: both cameras, w * h * bpp bytes each (null on GRAY8)
    } px;
    // ---- opt-in image masks (mskf_fe_set_mask; fe_mask.h): the eroded bit planes, on the device and (for mskf_fe_get_mask) on the host
    struct Mask {
        uint32_t *dev[2] = {nullptr, nullptr};     // cam0, cam1; null = not masked
        std::vector<uint32_t> host[2];
        int margin = 0;
        bool any() const { return dev[0] || dev[1]; }
    } mask;
    // ---- opt-in patch check (mskf_fe_set_patch_check; fe_patch.h): the setting is all there is
    mskf_fe_patch_check patch{0, 4, 0.8f, 0.8f};
    // ---- opt-in forward-backward check (mskf_fe_set_fb_check; fe_fb.h): likewise
    mskf_fe_fb_check fb{0, 1.0f, 1.0f};
    // ---- opt-in camera models (mskf_fe_set_camera_model; fe_cam_models.h): per camera the model and all eight coefficients as set
    // (a base model's first four are also CamDev::D).  A stream never set holds what mskf_calib gave it.
    struct CamExt {
        int model[2] = {0, 0};
        double coef[2][FCM_COEFFS] = {{0}, {0}};
        bool any() const { return model[0] >= FCM_RADTAN8 || model[1] >= FCM_RADTAN8; }
    } cam_ext;
    // ---- opt-in deeper LK pyramids (mskf_fe_set_lk_levels; fe_deep.h): the levels 4 .. levels - 1 of the three pyramids in an arena of
    // its own, pyramid i's planes at mem + i * plane_bytes (the roles rotate with i_prev0 / i_curr0 as the levels 0 .. 3 do)
    struct Deep {
        int levels = FD_BASE_LEVELS;
        uint8_t *mem = nullptr;
        int w[FD_EXTRA] = {0, 0, 0, 0}, h[FD_EXTRA] = {0, 0, 0, 0};
        size_t off[FD_EXTRA] = {0, 0, 0, 0};       // of level 4 + k inside a pyramid's planes
        size_t plane_bytes = 0;
        bool any() const { return levels > FD_BASE_LEVELS; }
        uint8_t *level(int pyr_idx, int l) const { return mem + (size_t)pyr_idx * plane_bytes + off[l - FD_BASE_LEVELS]; }
    } deep;
    // ---- device-side bookkeeping (fe_book.h): grids, candidate lists and track results of the stream, one allocation
    struct Book {
        char *mem = nullptr;
        FeBookDev dev{};                           // what is constant for the stream's life, filled once by book_alloc (dev.cap == 0: books on the
                                                   // host); a frame copies it and sets gen, R_p_c, prev / curr, cell_keys and the x_* pointers
        FeGridArr grid[3];                         // [parity], [parity ^ 1]: previous / current grid; [2]: this frame's survivors (== dev.tracked)
        int parity = 0;                            // grid[parity] holds the published grid of the last frame
        int n_prev = 0, n_cand_last = -1;          // host copies of the counts (launch sizing)
        bool grid_set = false;
    } book;
    // ---- EKF
    EkfStreamState ekf_state;
    void *ekf_extra = nullptr;
};

// timing helpers: t_begin records the start event and returns a slot index (or -1), t_end records the stop event
int mskf_t_begin(mskf_ctx *c, int kind);
void mskf_t_end(mskf_ctx *c, int slot, long long units);
void mskf_t_collect(mskf_ctx *c);   // call after the stream has been synchronised
void mskf_t_set_units(mskf_ctx *c, int slot, int kind, long long units);   // units of a slot begun earlier (bounds- and kind-checked)
// the pyramid (index into pyr / lvl0 / held) that plays a role: 0 prev cam0, 1 curr cam0, 2 curr cam1
static inline int pyr_of_role(const mskf_stream *s, int role) { return role == 0 ? s->i_prev0 : (role == 1 ? s->i_curr0 : s->i_curr1); }
// level 0 of a pyramid: the borrowed device image if there is one, else the stream's own plane
static inline const uint8_t *level0(const mskf_stream *s, int idx) { return s->lvl0[idx] ? s->lvl0[idx] : s->pyr[idx] + s->lvl_off[0]; }
void fill_pyr(const mskf_stream *s, int idx, PyrDev &p);
int mskf_ekf_stream_init(mskf_stream *s);
void mskf_ekf_stream_free(mskf_stream *s);
