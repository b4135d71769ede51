// mskf_capi_ctx.cpp — C-ABI: contexts, completion marks and waits, staging copies, timing, streams and points (include/mskf_hip.h).
#include <sys/prctl.h>
#include <time.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <atomic>
#include <type_traits>
#include <vector>
#include "mskf_internal.h"

static thread_local std::string g_last_error;
void mskf_set_error(const std::string &s) { g_last_error = s; }

extern "C" const char *mskf_last_error(void) { return g_last_error.c_str(); }
extern "C" int mskf_abi_version(void) { return 4; }   // 4: round 4 (2-point RANSAC inside the device frame: mskf_fe_frame_args.R_p_c / ransac_draws, mskf_fe_set_grid's draw counter)

extern "C" int mskf_ctx_create(int device, mskf_ctx **out) { return mskf_ctx_create_prio(device, 0, out); }

extern "C" int mskf_ctx_create_prio(int device, int high_priority, mskf_ctx **out) {
    if (!out) return MSKF_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        mskf_set_error("no HIP device visible (this library has no CPU fallback)");
        return MSKF_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) { mskf_set_error("device index out of range"); return MSKF_ERR_INVALID; }
    MSKF_HIPCHK(hipSetDevice(device));
    mskf_ctx *c = new mskf_ctx();
    c->device = device;
    hipError_t e;
    if (high_priority) {
        int lo = 0, hi = 0;   // numerically lower = more urgent
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi);
    } else {
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    }
    if (e != hipSuccess) { delete c; mskf_set_error(hipGetErrorString(e)); return MSKF_ERR_HIP; }
    { const char *w = std::getenv("MSKF_WAIT"); c->wait_block = w && std::strcmp(w, "block") == 0; }
    *out = c;
    return MSKF_OK;
}

extern "C" int mskf_ctx_create_shared(mskf_ctx *parent, mskf_ctx **out) {
    if (!parent || !out) return MSKF_ERR_INVALID;
    mskf_ctx *c = new mskf_ctx();
    c->device = parent->device;
    c->stream = parent->stream;
    c->owns_stream = false;
    c->wait_block = parent->wait_block;
    *out = c;
    return MSKF_OK;
}

extern "C" void mskf_ctx_destroy(mskf_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    mskf_t_collect(c);
    for (auto &e : c->t_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (int i = 0; i < 3; ++i) c->desc[i].release();
    for (int i = 0; i < 2; ++i) c->mask_desc[i].release();
    c->patch_desc.release();
    c->fb_desc.release();
    c->cam_desc.release();
    c->deep_desc.release(); c->deep_jobs.release();
    c->cell_arena.release(); c->trk_in.release(); c->trk_out.release(); c->upd_in.release(); c->upd_out.release();
    c->jobs.release(); c->eq_jobs.release(); c->px_jobs.release();
    c->book_desc.release(); c->book_out.release(); c->grid_in.release();
    c->pend_dsc.release(); c->pend_mch.release(); c->pend_vfy.release();
    c->ekf_desc.release();
    c->pred_arena.release();
    if (c->wait_ev) (void)hipEventDestroy(c->wait_ev);
    if (c->flag_h) (void)hipHostFree((void *)c->flag_h);
    if (c->cell_ev) (void)hipEventDestroy(c->cell_ev);
    for (PendingBatch *b : c->pending) if (b->done) (void)hipEventDestroy(b->done);
    if (c->owns_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" void fe_launch_mark(volatile unsigned int *flag, unsigned int seq, hipStream_t st);
extern "C" size_t fe_book_lds_budget(void);

extern "C" void fe_launch_copy(void *const *dst, const void *const *src, const size_t *bytes, int n_segs, hipStream_t st);
int mskf_copy_async(mskf_ctx *c, const MskfCopy *segs, int n) {
    for (int i0 = 0; i0 < n; i0 += MSKF_COPY_SEGS) {
        void *dst[MSKF_COPY_SEGS]; const void *src[MSKF_COPY_SEGS]; size_t bytes[MSKF_COPY_SEGS];
        int m = 0;
        for (int i = i0; i < n && i < i0 + MSKF_COPY_SEGS; ++i) {
            if (!segs[i].bytes) continue;
            if (((uintptr_t)segs[i].dst | (uintptr_t)segs[i].src) & 15) { mskf_set_error("staging copy with an unaligned end"); return MSKF_ERR_INVALID; }
            dst[m] = segs[i].dst; src[m] = segs[i].src; bytes[m] = segs[i].bytes; ++m;
        }
        if (m) fe_launch_copy(dst, src, bytes, m, c->stream);
    }
    MSKF_HIPCHK(hipGetLastError());
    return MSKF_OK;
}

int mskf_wait_event(mskf_ctx *c, hipEvent_t *ev_slot, bool record) {
    if (c->wait_block) {
        if (!*ev_slot) MSKF_HIPCHK(hipEventCreateWithFlags(ev_slot, hipEventDisableTiming | hipEventBlockingSync));
        if (record) { MSKF_HIPCHK(hipEventRecord(*ev_slot, c->stream)); return MSKF_OK; }
        MSKF_HIPCHK(hipEventSynchronize(*ev_slot));
        return MSKF_OK;
    }
    if (!c->flag_h) {
        unsigned int *p = nullptr;
        MSKF_HIPCHK(hipHostMalloc((void **)&p, mskf_ctx::kMarkSlots * 64, hipHostMallocCoherent | hipHostMallocMapped));      // one cache line per slot
        std::memset(p, 0, mskf_ctx::kMarkSlots * 64);
        c->flag_h = p;
    }
    int k = 0;
    while (k < mskf_ctx::kMarkSlots && c->flag_slot[k] && c->flag_slot[k] != ev_slot) ++k;
    if (k == mskf_ctx::kMarkSlots) { mskf_set_error("too many completion marks"); return MSKF_ERR_INVALID; }
    if (record) c->flag_slot[k] = ev_slot;       // a slot is claimed when its first mark is recorded; waiting only reads the context
    else if (c->flag_slot[k] != ev_slot) { mskf_set_error("waiting for a completion mark that was never recorded"); return MSKF_ERR_INVALID; }
    volatile unsigned int *w = c->flag_h + 16 * k;
    if (record) {
        // the mark is a stream write-value command (no dispatch: a one-thread kernel waits 37 us for a CU slot on a busy
        // device, profiles/r02_kernel_stats.csv of the kernel-mark build); a runtime that refuses the command on pinned host
        // memory falls back to the one-thread kernel k_mark
        static std::atomic<bool> use_write{true};   // (contexts are driven from several host threads)
        ++c->flag_seq[k];
        if (use_write.load(std::memory_order_relaxed)) {
            if (hipStreamWriteValue32(c->stream, (void *)w, c->flag_seq[k], 0) == hipSuccess) return MSKF_OK;
            (void)hipGetLastError();
            use_write.store(false, std::memory_order_relaxed);
        }
        fe_launch_mark(w, c->flag_seq[k], c->stream);
        MSKF_HIPCHK(hipGetLastError());
        return MSKF_OK;
    }
    const unsigned int want = c->flag_seq[k];
    // a mark that never arrives (device fault, lost queue) must not hang the caller for ever: after MSKF_WAIT_TIMEOUT_S
    // seconds (default 120) the stream is asked for its error state and the wait fails
    static const double limit_s = [] { const char *e = std::getenv("MSKF_WAIT_TIMEOUT_S"); const double v = e ? std::atof(e) : 120.0; return v > 0 ? v : 120.0; }();
    // MSKF_WAIT=nap[:us]: the same mark, polled between short sleeps (default 40 us) instead of spun on: a wait of some
    // milliseconds then costs the core a few per cent of its time and the waiter at most one sleep of latency, which leaves a
    // host that runs under a CPU quota its cores for the other groups' host phases
    static const long nap_ns = [] {
        const char *e = std::getenv("MSKF_WAIT");
        if (!e || std::strncmp(e, "nap", 3) != 0) return 0L;
        const long us = e[3] == ':' ? std::atol(e + 4) : 40L;
        return 1000L * (us > 0 ? us : 40L);
    }();
    if (nap_ns) {
        static thread_local bool slack_set = false;
        if (!slack_set) { (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL); slack_set = true; }     // (the default slack of 50 us would double every sleep)
    }
    unsigned long long spins = 0, naps = 0;
    bool timing = false;
    std::chrono::steady_clock::time_point t0;
    while ((int)(__atomic_load_n((const unsigned int *)w, __ATOMIC_ACQUIRE) - want) < 0) {
        bool check;
        if (nap_ns && spins >= 64) { const struct timespec ts = {0, nap_ns}; (void)nanosleep(&ts, nullptr); check = (++naps & 0xFFULL) == 0; }
        else { __builtin_ia32_pause(); check = (++spins & 0xFFFFFULL) == 0; }
        if (check) {                                             // about every 10 ms
            const auto now = std::chrono::steady_clock::now();
            if (!timing) { t0 = now; timing = true; }
            else if (std::chrono::duration<double>(now - t0).count() > limit_s) {
                const hipError_t e = hipStreamQuery(c->stream);
                mskf_set_error(e != hipSuccess && e != hipErrorNotReady ? hipGetErrorString(e) : "completion mark not written within the wait limit");
                std::fprintf(stderr, "mskf_wait_event: ctx %p slot %d mark %u wanted %u, stream query %d\n", (void *)c, k, *w, want, (int)e);
                return MSKF_ERR_HIP;
            }
        }
    }
    return MSKF_OK;
}

int mskf_batch_arm(mskf_ctx *c, PendingBatch &b) {
    const int rc = mskf_wait_event(c, &b.done, true);
    if (rc == MSKF_OK) b.active = true;
    return rc;
}
int mskf_batch_finish(mskf_ctx *c, PendingBatch &b) {
    MSKF_HIPCHK(hipSetDevice(c->device));
    const int rc = mskf_wait_event(c, &b.done, false);
    if (rc == MSKF_OK) b.active = false;
    return rc;
}

int mskf_refuse_if_owned(const mskf_ctx *c, MskfArenas which) {
    const char *owner = nullptr;
    switch (which) {
        case MSKF_ARENAS_FE:
            if (c->pend_trk.active) owner = "a track batch of this context is still pending (call mskf_fe_track_batch_end)";
            else if (c->pend_frame.active) owner = "a device frame of this context is still pending (call mskf_fe_frame_batch_end)";
            break;
        case MSKF_ARENAS_UPDATE:
            if (c->pend_upd.active)
                owner = c->pend_upd.direct ? "a direct update batch of this context is still pending (call mskf_ekf_update_direct_batch_end)"
                                           : "an update batch of this context is still pending (call mskf_ekf_update_batch_end)";
            break;
        case MSKF_ARENAS_PRED:
            if (c->pend_ro.active)
                owner = c->pend_ro.rec == 3 ? "a position-variance read-out of this context is still pending (call mskf_ekf_get_pos_var_batch_end)"
                                            : "an odometry-covariance read-out of this context is still pending (call mskf_ekf_get_odom_cov_batch_end)";
            break;
    }
    if (!owner) return MSKF_OK;
    mskf_set_error(owner);
    return MSKF_ERR_INVALID;
}

int mskf_wait(mskf_ctx *c) {
    int rc = mskf_wait_event(c, &c->wait_ev, true);
    if (rc != MSKF_OK) return rc;
    return mskf_wait_event(c, &c->wait_ev, false);
}

extern "C" int mskf_ctx_sync(mskf_ctx *c) {
    if (!c) return MSKF_ERR_INVALID;
    { const int rc = mskf_wait(c); if (rc != MSKF_OK) return rc; }
    mskf_t_collect(c);
    return MSKF_OK;
}

int mskf_t_begin(mskf_ctx *c, int kind) {
    if (!c->timing || !c->t_gate) return -1;
    if ((c->t_all[kind]++ % c->timing_period) != 0) return -1;      // sampled: the events themselves cost device and host time
    TimingSlot t;
    if (!c->t_pool.empty()) { t.a = c->t_pool.back().first; t.b = c->t_pool.back().second; c->t_pool.pop_back(); }
    else {
        if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess) return -1;
    }
    t.kind = kind; t.units = 0;
    (void)hipEventRecord(t.a, c->stream);
    c->t_pending.push_back(t);
    return (int)c->t_pending.size() - 1;
}
void mskf_t_end(mskf_ctx *c, int slot, long long units) {
    if (slot < 0) return;
    (void)hipEventRecord(c->t_pending[slot].b, c->stream);
    c->t_pending[slot].units = units;
}
// Units of a slot that was begun earlier: the slot index is only valid until the next mskf_t_collect (any synchronising
// call of the context collects), so it is checked against the pending list and the kind it was begun with.
void mskf_t_set_units(mskf_ctx *c, int slot, int kind, long long units) {
    if (slot < 0 || (size_t)slot >= c->t_pending.size() || c->t_pending[slot].kind != kind) return;
    c->t_pending[slot].units = units;
}
void mskf_t_collect(mskf_ctx *c) {
    for (auto &t : c->t_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
            c->t_ms[t.kind] += ms; c->t_launches[t.kind] += 1; c->t_units[t.kind] += t.units;
        }
        c->t_pool.push_back({t.a, t.b});
    }
    c->t_pending.clear();
}

extern "C" int mskf_ctx_set_timing(mskf_ctx *c, int enable) {
    if (!c) return MSKF_ERR_INVALID;
    MSKF_HIPCHK(hipSetDevice(c->device));
    MSKF_HIPCHK(hipStreamSynchronize(c->stream));
    mskf_t_collect(c);
    c->timing = enable != 0;
    c->timing_period = enable > 1 ? enable : 1;
    return MSKF_OK;
}

extern "C" int mskf_ctx_set_wait_mode(mskf_ctx *c, int block) {
    if (!c) return MSKF_ERR_INVALID;
    // (a mark recorded in one mode cannot be awaited in the other)
    for (const PendingBatch *b : c->pending) if (b->active) { mskf_set_error("a batch of this context is pending"); return MSKF_ERR_INVALID; }
    c->wait_block = block != 0;
    return MSKF_OK;
}

extern "C" int mskf_ctx_timing_gate(mskf_ctx *c, int on) {
    if (!c) return MSKF_ERR_INVALID;
    c->t_gate = on != 0;          // no synchronisation: launches already begun keep the state they were begun with
    return MSKF_OK;
}

extern "C" int mskf_ctx_get_timing(mskf_ctx *c, double *ms, long long *launches, long long *units, int reset) {
    if (!c || !ms || !launches || !units) return MSKF_ERR_INVALID;
    MSKF_HIPCHK(hipSetDevice(c->device));
    MSKF_HIPCHK(hipStreamSynchronize(c->stream));
    mskf_t_collect(c);
    for (int k = 0; k < MSKF_K_COUNT; ++k) {
        // sampled timing: the sums are scaled from the timed launches to all launches of the kind
        const double sc = c->t_launches[k] > 0 ? (double)c->t_all[k] / (double)c->t_launches[k] : 0.0;
        ms[k] = c->t_ms[k] * sc; launches[k] = c->t_launches[k] > 0 ? c->t_all[k] : 0; units[k] = (long long)((double)c->t_units[k] * sc);
        if (reset) { c->t_ms[k] = 0; c->t_launches[k] = 0; c->t_units[k] = 0; c->t_all[k] = 0; }
    }
    return MSKF_OK;
}

extern "C" void *mskf_ctx_hip_stream(mskf_ctx *c) { return c ? (void *)c->stream : nullptr; }

extern "C" int mskf_ctx_get_host_time(mskf_ctx *c, double out[4], int reset) {
    if (!c || !out) return MSKF_ERR_INVALID;
    for (int k = 0; k < 4; ++k) { out[k] = c->host_s[k]; if (reset) c->host_s[k] = 0; }
    return MSKF_OK;
}

// The stream's book allocation: ONE sequence of take()s, run on a null base to obtain the size and on the allocation to
// set the pointers (every region rounded up to 256 bytes).  D holds the capacities on entry.
static size_t book_carve(char *base, FeBookDev &D, FeGridArr grid[3]) {
    size_t off = 0;
    auto take = [&](auto *&p, size_t count) {
        p = (std::remove_reference_t<decltype(p)>)((uintptr_t)base + off);
        off += round_up(sizeof(*p) * count, 256);
    };
    const size_t cap = (size_t)D.cap, cand_cap = (size_t)D.cand_cap, det_cap = (size_t)D.det_cap;
    take(D.st, 1);
    for (int g = 0; g < 3; ++g) {
        FeGridArr &G = grid[g];
        take(G.id, cap); take(G.lifetime, cap); take(G.code, cap); take(G.response, cap);
        take(G.cam0, cap); take(G.cam1, cap); take(G.und0, cap); take(G.und1, cap);
    }
    D.tracked = grid[2];
    take(D.det_pt, det_cap); take(D.det_score, det_cap);
    take(D.cand_pt, cand_cap); take(D.cand_index, cand_cap); take(D.cand_score, cand_cap);
    take(D.cand_off, (size_t)D.n_cells + 1); take(D.cand_cnt, (size_t)D.n_cells + 1); take(D.cell_count, (size_t)D.n_codes + 1);
    take(D.t_out0, cap); take(D.t_out1, cap); take(D.t_und0, cap); take(D.t_und1, cap); take(D.t_status, cap);
    take(D.c_out0, cand_cap); take(D.c_out1, cand_cap); take(D.c_und0, cand_cap); take(D.c_und1, cand_cap); take(D.c_status, cand_cap);
    take(D.rs_pair, 4 * cap); take(D.rs_pt, 4 * cap); take(D.rs_scalar, 48);       // fe_book.h: the scratch of the 2-point RANSAC
    return off;
}

// Device-side books of a stream (fe_book.h): the three feature lists, detection / candidate lists and the results of the two
// track calls, in ONE allocation, and the descriptor of everything about them that never changes (Book::dev).  Streams whose
// grid_min / grid_max exceed the short-list bound of the kernels keep their books on the host (dev.cap stays 0).
static int book_alloc(mskf_stream *s) {
    mskf_stream::Book &K = s->book;
    const mskf_fe_cfg &fe = s->fe;
    if (fe.grid_min_feature_num > FB_MAXK || fe.grid_max_feature_num > FB_MAXK || fe.grid_min_feature_num < 0 ||
        fe.grid_max_feature_num < fe.grid_min_feature_num) return MSKF_OK;
    FeBookDev D{};
    D.grid_row = fe.grid_row; D.grid_col = fe.grid_col; D.grid_min = fe.grid_min_feature_num; D.grid_max = fe.grid_max_feature_num;
    D.grid_h = s->h / fe.grid_row; D.grid_w = s->w / fe.grid_col;                 // image_processor.cpp:250-251
    if (D.grid_h <= 0 || D.grid_w <= 0) return MSKF_OK;
    D.n_cells = fe.grid_row * fe.grid_col;
    D.n_codes = std::max(((s->h - 1) / D.grid_h) * fe.grid_col + (s->w - 1) / D.grid_w + 1, D.n_cells);   // Q7: partial rows / columns
    D.cap = D.n_codes * std::max(fe.grid_max_feature_num, 1) + 8;
    D.cand_cap = D.n_cells * std::max(fe.grid_max_feature_num, 1) + 8;
    D.det_cap = fe.det_rows * fe.det_cols;
    // the bookkeeping kernel keeps its lists in LDS: a configuration whose lists do not fit the budget the kernel can get
    // (a very fine detector grid) keeps its books on the host
    if (4 * fe_book_scratch_ints(D.cap, D.cand_cap, D.det_cap, D.n_codes, D.det_cap) > fe_book_lds_budget()) return MSKF_OK;
    D.det_rows = fe.det_rows; D.det_cols = fe.det_cols; D.det_cw = s->det_cw; D.det_ch = s->det_ch;
    D.thr_score = fe.fast_threshold * 256;
    D.q4 = (fe.compat_flags & MSKF_COMPAT_Q4_RESPONSE_INDEX) ? 1 : 0;
    // twoPointRansac between the tracks (:482-500; commented out in the reference, Q5): iterations as :920-921
    D.ransac = (fe.compat_flags & MSKF_COMPAT_Q5_NO_RANSAC) ? 0 : 1;
    D.ransac_iters = static_cast<int>(std::ceil(std::log(1 - 0.99) / std::log(1 - 0.7 * 0.7)));
    D.ransac_thr = fe.ransac_threshold;
    D.ransac_npu[0] = 2.0 / (s->cam0.K[0] + s->cam0.K[1]); D.ransac_npu[1] = 2.0 / (s->cam1.K[0] + s->cam1.K[1]);
    const size_t bytes = book_carve(nullptr, D, K.grid);
    MSKF_HIPCHK(hipMalloc((void **)&K.mem, bytes));
    MSKF_HIPCHK(hipMemsetAsync(K.mem, 0, bytes, s->ctx->stream));
    MSKF_HIPCHK(hipStreamSynchronize(s->ctx->stream));
    book_carve(K.mem, D, K.grid);
    K.dev = D;
    return MSKF_OK;
}

extern "C" int mskf_stream_create(mskf_ctx *ctx, const mskf_calib *calib, const mskf_fe_cfg *fe, const mskf_ekf_cfg *ekf,
                                  mskf_stream **out) {
    if (!ctx || !calib || !fe || !ekf || !out) return MSKF_ERR_INVALID;
    for (int m : {calib->cam0_model, calib->cam1_model})
        if (m != MSKF_MODEL_RADTAN && m != MSKF_MODEL_EQUIDISTANT) {
            mskf_set_error("unknown distortion model (radtan and equidistant are implemented)");
            return MSKF_ERR_UNSUPPORTED;
        }
    if (calib->width < 64 || calib->height < 64 || fe->det_rows <= 0 || fe->det_cols <= 0 || fe->grid_row <= 0 || fe->grid_col <= 0)
        return MSKF_ERR_INVALID;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    mskf_stream *s = new mskf_stream();
    s->ctx = ctx;
    s->ctx_ekf = ctx;
    s->home_ctx = ctx;
    s->calib = *calib; s->fe = *fe; s->ekf = *ekf;
    s->w = calib->width; s->h = calib->height;
    size_t off = 0;
    int w = s->w, h = s->h;
    for (int l = 0; l < MSKF_LEVELS; ++l) {
        s->lw[l] = w; s->lh[l] = h; s->lvl_off[l] = off;
        off += round_up((size_t)w * h, 256);
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    s->pyr_bytes = off;
    int rc = MSKF_OK;
    for (int i = 0; i < 3 && rc == MSKF_OK; ++i) {
        hipError_t e = hipMalloc((void **)&s->pyr[i], s->pyr_bytes);
        if (e != hipSuccess) { mskf_set_error(hipGetErrorString(e)); rc = MSKF_ERR_HIP; }
    }
    // point capacity: every live grid slot plus every detector cell
    const int det_cells = fe->det_rows * fe->det_cols;
    s->pt_cap = (fe->grid_row + 1) * (fe->grid_col + 1) * (fe->grid_max_feature_num + 1) + det_cells + 64;
    if (rc == MSKF_OK) rc = mskf_ekf_stream_init(s);
    if (rc != MSKF_OK) { mskf_stream_destroy(s); return rc; }

    for (int i = 0; i < 4; ++i) {
        s->cam0.K[i] = calib->cam0_intrinsics[i]; s->cam0.D[i] = calib->cam0_distortion[i];
        s->cam0.model = calib->cam0_model; s->cam1.model = calib->cam1_model;
        s->cam1.K[i] = calib->cam1_intrinsics[i]; s->cam1.D[i] = calib->cam1_distortion[i];
        s->cam_ext.coef[0][i] = calib->cam0_distortion[i]; s->cam_ext.coef[1][i] = calib->cam1_distortion[i];
    }
    s->cam_ext.model[0] = calib->cam0_model; s->cam_ext.model[1] = calib->cam1_model;      // (mskf_fe_set_camera_model may change it)
    // image_processor.cpp:63-72 (loadParameters) and :544,:587-591 (stereoMatch)
    using namespace hm;
    Rigid m4_cam0_imu = Rigid::from_rowmajor16(calib->T_cam0_imu);
    Mat3 R_cam0_imu = m4_cam0_imu.R.transpose();
    Vec3 t_cam0_imu = -(R_cam0_imu * m4_cam0_imu.t);
    Rigid m4_cam1_cam0 = Rigid::from_rowmajor16(calib->T_cam1_cam0);
    Rigid T_cam1_imu = m4_cam1_cam0 * m4_cam0_imu;
    Mat3 R_cam1_imu = T_cam1_imu.R.transpose();
    Vec3 t_cam1_imu = -(R_cam1_imu * T_cam1_imu.t);
    Mat3 R_cam0_cam1 = R_cam1_imu.transpose() * R_cam0_imu;
    Vec3 t_cam0_cam1 = R_cam1_imu.transpose() * (t_cam0_imu - t_cam1_imu);
    Mat3 E = skew(t_cam0_cam1) * R_cam0_cam1;
    std::memcpy(s->R01, R_cam0_cam1.m, sizeof(s->R01));
    std::memcpy(s->E, E.m, sizeof(s->E));
    const double norm_pixel_unit = 4.0 / (s->cam0.K[0] + s->cam0.K[1] + s->cam1.K[0] + s->cam1.K[1]);
    s->epi_thresh = fe->stereo_threshold * norm_pixel_unit;
    s->det_ch = (s->h + fe->det_rows - 1) / fe->det_rows;
    s->det_cw = (s->w + fe->det_cols - 1) / fe->det_cols;
    rc = book_alloc(s);
    if (rc != MSKF_OK) { mskf_stream_destroy(s); return rc; }
    ctx->streams.push_back(s);
    *out = s;
    return MSKF_OK;
}

extern "C" mskf_ctx *mskf_stream_ctx(mskf_stream *s) { return s ? s->ctx : nullptr; }
extern "C" mskf_ctx *mskf_stream_ekf_ctx(mskf_stream *s) { return s ? s->ctx_ekf : nullptr; }
extern "C" int mskf_stream_set_ekf_ctx(mskf_stream *s, mskf_ctx *c) {
    if (!s || !c || c->device != s->ctx->device) return MSKF_ERR_INVALID;
    MSKF_HIPCHK(hipSetDevice(c->device));
    MSKF_HIPCHK(hipStreamSynchronize(s->ctx_ekf->stream));
    MSKF_HIPCHK(hipStreamSynchronize(c->stream));
    s->ctx_ekf = c;
    return MSKF_OK;
}

extern "C" int mskf_stream_rebind(mskf_stream *s, mskf_ctx *fe_ctx, mskf_ctx *ekf_ctx) {
    if (!s) return MSKF_ERR_INVALID;
    if ((fe_ctx && fe_ctx->device != s->home_ctx->device) || (ekf_ctx && ekf_ctx->device != s->home_ctx->device)) return MSKF_ERR_INVALID;
    if (fe_ctx) s->ctx = fe_ctx;
    if (ekf_ctx) s->ctx_ekf = ekf_ctx;
    return MSKF_OK;
}

struct mskf_point { hipEvent_t ev = nullptr; };
extern "C" int mskf_ctx_record_point(mskf_ctx *ctx, mskf_point **point) {
    if (!ctx || !point) return MSKF_ERR_INVALID;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    if (!*point) { *point = new mskf_point(); MSKF_HIPCHK(hipEventCreateWithFlags(&(*point)->ev, hipEventDisableTiming)); }
    MSKF_HIPCHK(hipEventRecord((*point)->ev, ctx->stream));
    return MSKF_OK;
}
extern "C" int mskf_ctx_wait_point(mskf_ctx *ctx, mskf_point *point) {
    if (!ctx || !point || !point->ev) return MSKF_ERR_INVALID;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    MSKF_HIPCHK(hipStreamWaitEvent(ctx->stream, point->ev, 0));
    return MSKF_OK;
}
extern "C" void mskf_point_destroy(mskf_point *point) {
    if (!point) return;
    if (point->ev) (void)hipEventDestroy(point->ev);
    delete point;
}

extern "C" void mskf_stream_destroy(mskf_stream *s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    if (s->ctx_ekf && s->ctx_ekf != s->ctx) (void)hipStreamSynchronize(s->ctx_ekf->stream);
    for (int i = 0; i < 3; ++i) if (s->pyr[i]) (void)hipFree(s->pyr[i]);
    if (s->book.mem) (void)hipFree(s->book.mem);
    if (s->eq.mem) (void)hipFree(s->eq.mem);
    if (s->px.raw) (void)hipFree(s->px.raw);
    if (s->deep.mem) (void)hipFree(s->deep.mem);
    for (int c = 0; c < 2; ++c) if (s->mask.dev[c]) (void)hipFree(s->mask.dev[c]);
    mskf_ekf_stream_free(s);
    auto &v = s->home_ctx->streams;
    for (size_t i = 0; i < v.size(); ++i) if (v[i] == s) { v.erase(v.begin() + i); break; }
    delete s;
}

// Completion-mark slots claimed so far (spinning mode).  NOT part of the C ABI (declared in mskf_internal.h only, like the
// fe_launch_* functions): tests/test_gpu_verify.py reads it.
extern "C" int fe_mark_slots_used(const mskf_ctx *ctx) {
    int k = 0;
    while (k < mskf_ctx::kMarkSlots && ctx->flag_slot[k]) ++k;
    return k;
}
