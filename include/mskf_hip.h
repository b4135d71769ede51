/* mskf_hip.h — C ABI of the MI355X (gfx950) hot path: stereo KLT front-end + MSCKF measurement update.
 *
 * This is the drop-in boundary: the host-side C++ mirror of the reference classes
 * (msckf_stereo_c_amd/csrc/host/: cg::ImageProcessor, cg::MsckfVio, cg::System) calls ONLY these
 * entry points; a maintainer of the reference would bind the same symbols from
 * msckf_core/src/image_processor.cpp and msckf_core/src/msckf_vio.cpp.
 *
 * Conventions: plain pointers and sizes, no C++ / torch types; every function returns MSKF_OK (0)
 * or a negative mskf_status and never throws; the caller owns all host buffers; device buffers are
 * owned by the handles; calls on one mskf_ctx are serialised by the caller, different contexts may be
 * driven from different host threads.  One mskf_ctx = one HIP stream on one GPU plus the batch
 * staging buffers; one mskf_stream = one VIO stream (one ImageProcessor + one MsckfVio state).
 * The *_batch entry points process one frame of many VIO streams per kernel launch; the single
 * stream entry points are batches of one.
 *
 * There is no CPU fallback: every compute entry point fails with MSKF_ERR_NO_DEVICE / MSKF_ERR_HIP
 * when no gfx950 device or code object is available.
 */
#ifndef MSKF_HIP_H
#define MSKF_HIP_H

#include "mskf_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mskf_status {
    MSKF_OK = 0,
    MSKF_ERR_INVALID = -1,      /* bad argument */
    MSKF_ERR_HIP = -2,          /* a HIP runtime call failed (mskf_last_error() has the text) */
    MSKF_ERR_UNSUPPORTED = -3,  /* e.g. an unknown distortion model */
    MSKF_ERR_CAPACITY = -4,     /* more points / clones / rows than the stream was created for */
    MSKF_ERR_NO_DEVICE = -5
} mskf_status;

typedef struct mskf_ctx mskf_ctx;
typedef struct mskf_stream mskf_stream;

const char *mskf_last_error(void);
int mskf_abi_version(void);   /* 2: update args carry diag_out, mskf_ekf_cfg.compression_mode, *_begin / *_end entry points; 3 (round 3): update args carry
                                 pos_var_out, mskf_fe_frame_batch_* (whole front-end frames on the device), mskf_ctx_timing_gate, mskf_ctx_set_wait_mode;
                                 4 (round 4): the 2-point RANSAC inside the device frame (mskf_fe_frame_args.R_p_c / ransac_draws, mskf_fe_set_grid's draw counter);
                                 added under 4, symbols only, no struct changed: mskf_ekf_get_odom_cov, _batch, _batch_begin, _batch_end;
                                 mskf_fe_set_equalize, mskf_fe_get_equalize; mskf_fe_set_input_format, mskf_fe_get_input_format;
                                 mskf_ekf_update_direct, _batch, _batch_begin, _batch_end (with their own mskf_ekf_direct_args);
                                 mskf_fe_set_mask, mskf_fe_get_mask (with their own mskf_fe_mask) and the timing kind MSKF_K_FE_MASK, which is the
                                 slot MSKF_K_PT_GEOM left empty (MSKF_K_COUNT is unchanged);
                                 mskf_fe_describe, _batch, _batch_begin, _batch_end (with their own mskf_fe_describe_args), mskf_fe_descriptor_pattern;
                                 mskf_fe_match, _batch, _batch_begin, _batch_end (with their own mskf_fe_match_args and mskf_match);
                                 mskf_fe_verify, _batch, _batch_begin, _batch_end (with their own mskf_fe_verify_args);
                                 mskf_fe_set_patch_check, mskf_fe_get_patch_check (with their own mskf_fe_patch_check) and the alias MSKF_K_FE_PATCH of
                                 the timing slot the mask gate borrowed;
                                 mskf_fe_set_fb_check, mskf_fe_get_fb_check (with their own mskf_fe_fb_check) and the alias MSKF_K_FE_FB of the same slot;
                                 mskf_fe_set_lk_levels, mskf_fe_get_lk_levels and the alias MSKF_K_PYR_DEEP of the same slot */

int mskf_ctx_create(int device, mskf_ctx **out);
/* Same, with the context's HIP stream created at the device's most urgent priority when high_priority != 0.
 * The batch runner puts the filter stage of a pipelined group (the serial dependency chain of the step) on such a
 * context so that its short kernels are dispatched ahead of the front-end's wide ones. */
int mskf_ctx_create_prio(int device, int high_priority, mskf_ctx **out);
/* A second context (own staging arenas, events, timing) whose work is enqueued on `parent`'s HIP stream: two host threads
 * (e.g. the front-end and the filter of one group of streams) can then feed one hardware queue.  `parent` must outlive it. */
int mskf_ctx_create_shared(mskf_ctx *parent, mskf_ctx **out);
void mskf_ctx_destroy(mskf_ctx *ctx);
int mskf_ctx_sync(mskf_ctx *ctx);
/* How the *_end calls of this context wait for the device: 0 = spin on a completion mark in pinned host memory (lowest
 * latency, occupies a core), 1 = park the thread on a blocking HIP event.  Default: MSKF_WAIT=block in the environment
 * selects 1, else 0.  A stage that waits once per frame for a long chain of kernels (the device front-end frame) loses
 * nothing by parking and leaves its core to the threads that have host work. */
int mskf_ctx_set_wait_mode(mskf_ctx *ctx, int block);
/* the HIP stream of this context as a void* (hipStream_t), for event timing by the caller */
void *mskf_ctx_hip_stream(mskf_ctx *ctx);

/* Optional per-kernel timing with HIP events recorded on the context's own stream (bench / roofline).
 * `units` are the algorithmic work units of a launch (LK: point tracks, temporal + stereo of one track call in one launch — MSKF_K_PT_GEOM
 * is kept for ABI stability, counts no geometry since that moved into that launch, and carries the point gates behind a track launch instead (MSKF_K_FE_MASK, MSKF_K_FE_PATCH, MSKF_K_FE_FB) and the deep pyramid launch (MSKF_K_PYR_DEEP); pyramid: output pixels;
 * EKF feature / GEMM / Cholesky / TRSM kernels: algorithmic FP64 flops; others: streams).  Disabled by default.
 * `enable` = n > 1 times every n-th launch of each kind only and scales the sums to all launches: two event records per launch cost
 * 7 % of the throughput at the C2 bench shape and 36 % at C5 (one stream per launch), measured.  MSKF_K_EKF_AUGMENT is kept for ABI
 * stability and counts no augmentation: that runs inside k_ekf_propagate (MSKF_K_EKF_PROPAGATE), also for mskf_ekf_augment.  The slot
 * counts the launches of k_ekf_direct_update instead (mskf_ekf_update_direct*; units: streams with rows), which nothing but those calls makes. */
enum {
    MSKF_K_PYR = 0, MSKF_K_DETECT, MSKF_K_LK, MSKF_K_EKF_PROPAGATE, MSKF_K_EKF_AUGMENT, MSKF_K_EKF_FEATURES,
    MSKF_K_EKF_TSQR /* k_ekf_tsqr; rounds 1-3: the stacking-decision kernel, which no longer exists */, MSKF_K_EKF_GEMM, MSKF_K_EKF_CHOL, MSKF_K_EKF_TRSM, MSKF_K_EKF_SMALL, MSKF_K_EKF_REMOVE, MSKF_K_PT_GEOM, MSKF_K_FE_BOOK, MSKF_K_COUNT,
    /* k_mask_points, the point gate of the image masks (mskf_fe_set_mask), launched behind a track launch only when a stream of that batch
       has a mask; units: streams.  It takes the slot of MSKF_K_PT_GEOM, which nothing else fills (see above), so MSKF_K_COUNT and the
       arrays of mskf_ctx_get_timing keep their size. */
    MSKF_K_FE_MASK = MSKF_K_PT_GEOM,
    /* k_patch_points, the point gate of the patch check (mskf_fe_set_patch_check), launched behind a track launch only when a stream of
       that batch checks; units: streams.  The same slot: it counts the point gates behind a track launch, of either kind, and with both
       features off its counts are exactly as before. */
    MSKF_K_FE_PATCH = MSKF_K_PT_GEOM,
    /* k_fb_points, the point gate of the forward-backward check (mskf_fe_set_fb_check), launched behind a track launch only when a
       stream of that batch checks; units: streams.  The same slot again: with the three features off its counts are exactly as before. */
    MSKF_K_FE_FB = MSKF_K_PT_GEOM,
    /* k_pyr_down_deep, the pyramid levels 4 and up of the streams that track over more than four levels (mskf_fe_set_lk_levels), launched
       behind the pyramid launch of a push only when a stream of that batch is deep; units: output pixels.  The same slot once more (so
       that MSKF_K_PYR keeps meaning k_pyr_down3): with the four features off its counts are exactly as before. */
    MSKF_K_PYR_DEEP = MSKF_K_PT_GEOM
};
int mskf_ctx_set_timing(mskf_ctx *ctx, int enable);
/* Accounting gate (default on): while it is off, launches are not timed and host seconds not accumulated.  Unlike
 * mskf_ctx_set_timing it does not synchronise, so the thread that drives the context can open and close a measurement
 * window in the middle of a running pipeline; launches already begun keep the state they were begun with. */
int mskf_ctx_timing_gate(mskf_ctx *ctx, int on);
/* host seconds spent inside the batched entry points of this context, outside the device waits: [0] mskf_ekf_update_batch
 * packing, [1] its unpacking, [2] mskf_fe_track_batch packing, [3] its unpacking */
int mskf_ctx_get_host_time(mskf_ctx *ctx, double out[4], int reset);
/* arrays of MSKF_K_COUNT entries: accumulated milliseconds, launches and units since the last reset */
int mskf_ctx_get_timing(mskf_ctx *ctx, double *ms, long long *launches, long long *units, int reset);

int mskf_stream_create(mskf_ctx *ctx, const mskf_calib *calib, const mskf_fe_cfg *fe, const mskf_ekf_cfg *ekf,
                       mskf_stream **out);
void mskf_stream_destroy(mskf_stream *s);
mskf_ctx *mskf_stream_ctx(mskf_stream *s);
/* Run the EKF half of a stream (all mskf_ekf_* calls) on another context of the same GPU, so a front-end
 * thread and a filter thread can drive one VIO stream concurrently (they share no device buffers). */
int mskf_stream_set_ekf_ctx(mskf_stream *s, mskf_ctx *ekf_ctx);
mskf_ctx *mskf_stream_ekf_ctx(mskf_stream *s);
/* Move a stream's front-end half and / or its filter half to other contexts of the same GPU (NULL = stays where it is) WITHOUT
 * synchronising anything: for a scheduler that hands whole batches of streams to whichever worker (context + host thread) is
 * free.  The caller guarantees that the half being moved has no work in flight that the new context's queue is not ordered
 * behind: it has waited for the half's last batch (every *_end call does), or it chains the queues with
 * mskf_ctx_record_point / mskf_ctx_wait_point. */
int mskf_stream_rebind(mskf_stream *s, mskf_ctx *fe_ctx, mskf_ctx *ekf_ctx);
/* Device-side ordering between two contexts' queues: record a point in `ctx`'s stream (the handle is created on first use
 * and reused), make another context's stream wait for it.  No host wait on either side. */
typedef struct mskf_point mskf_point;
int mskf_ctx_record_point(mskf_ctx *ctx, mskf_point **point);
int mskf_ctx_wait_point(mskf_ctx *ctx, mskf_point *point);
void mskf_point_destroy(mskf_point *point);

/* ------------------------------------------------------------------ front-end
 * Replaces, inside cg::ImageProcessor::stereoCallback (image_processor.cpp:139-203):
 *   createImagePyramids()              :213-245  -> mskf_fe_push_stereo*   (pyramids of cam0/cam1 in HBM)
 *   detector_.detect_features()        :259,:657 -> mskf_fe_push_stereo*   (per-cell maxima) + mskf_fe_get_cell_maxima
 *   predictFeatureTracking + optical_flow_multi_level + stereoMatch  :389-463 -> mskf_fe_track (do_temporal = 1)
 *   stereoMatch of new candidates      :268,:688 -> mskf_fe_track (do_temporal = 0)
 *   std::swap(prev pyramid, curr pyramid) :194   -> mskf_fe_swap
 */

/* Upload one stereo pair (host memory, row pitch in bytes), build the 4-level pyramids of both
 * cameras and the detector's per-cell maxima of cam0 level 0.  Asynchronous on the context stream.
 * The image pointers of every push mean raw bytes in the stream's input format (mskf_fe_set_input_format; 8-bit grey by
 * default): pitch >= width * bytes per pixel here, and "dense" means pitch == width * bytes per pixel everywhere else. */
int mskf_fe_push_stereo(mskf_stream *s, const uint8_t *cam0, const uint8_t *cam1, int width, int height, int pitch,
                        double time_stamp);
/* Same with the images already resident in device memory (dense, pitch == width). */
int mskf_fe_push_stereo_device(mskf_stream *s, const uint8_t *d_cam0, const uint8_t *d_cam1, int width, int height,
                               double time_stamp);
/* on_device: 0 = host images (copied in), 1 = device images (copied D2D), 2 = device images BORROWED: read in
 * place, the caller keeps each pair valid and unchanged until the second-next push of that stream.
 * (3 is internal to mskf_fe_push_stereo: level 0 already copied into the stream's own planes.) */
int mskf_fe_push_stereo_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, const uint8_t *const *cam0,
                              const uint8_t *const *cam1, int on_device);

/* Detector floor of a stream, in score units (1/256 of the response): from the next push on only per-cell maxima ABOVE the
 * floor are recorded (default 0: every cell with a positive score).  A caller that only ever asks for the candidates above
 * its detector threshold (image_processor.cpp:132: fast_threshold) sets the floor to that threshold: the comparison is made
 * exactly, before the integer square root of the Shi-Tomasi score, which most pixels then never need. */
int mskf_fe_set_detect_floor(mskf_stream *s, int min_score);
/* All det_rows*det_cols per-cell maxima of the last pushed cam0 image (score 0 = no corner above the floor). Synchronises. */
int mskf_fe_get_cell_maxima(mskf_stream *s, mskf_corner *out, int capacity, int *n_out);
/* Same, restricted to the cells whose maximum score exceeds min_score (the detector threshold of
 * image_processor.cpp:132, in 1/256 units), in cell order; out[k].cell identifies the cell.  This is what
 * detect_features() needs — converting and copying the ~1400 sub-threshold cells of a 752x480 frame was a
 * measurable share of the host time per frame.  min_score must not be below the stream's detector floor. */
int mskf_fe_get_cell_candidates(mskf_stream *s, int min_score, mskf_corner *out, int capacity, int *n_out);

typedef struct mskf_fe_track_args {
    int32_t n;                    /* number of points */
    int32_t do_temporal;          /* 1: prev cam0 -> curr cam0 LK, then stereo; 0: stereo only */
    const mskf_point2f *in_pts;   /* prev cam0 points (temporal) or curr cam0 points (stereo only) */
    double Hpred[9];              /* K R_p_c K^-1 (image_processor.cpp:335-340); identity-like under Q2 */
    mskf_point2f *out0, *out1;    /* tracked cam0 / matched cam1 pixels */
    mskf_point2f *und0, *und1;    /* undistorted normalised coordinates of out0 / out1 */
    uint8_t *status;              /* bit0 temporal ok, bit1 stereo inlier */
} mskf_fe_track_args;

int mskf_fe_track(mskf_stream *s, const mskf_fe_track_args *args);
int mskf_fe_track_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, const mskf_fe_track_args *args);
/* The same in two halves, so that a host thread can prepare another batch (on another context, possibly sharing this
 * one's HIP stream: mskf_ctx_create_shared) while the device works: _begin validates, stages and enqueues everything and
 * returns; _end waits and copies the results into the args passed to _begin (they and their arrays must still be valid).
 * One pending batch per context.  The same holds for every _begin / _end pair of this header:
 *   - while a batch is pending, calls that need the staging buffers it owns fail with MSKF_ERR_INVALID, and mskf_last_error
 *     names the pending batch: a track or device-frame batch blocks the front-end calls (push, track, frame), an update
 *     batch blocks the next update, a read-out (position variances or odometry covariance) blocks every prediction,
 *     augmentation, clone removal and any other read-out;
 *   - a failed _end (the wait timed out or the stream reported an error) leaves the batch pending: its kernels may still
 *     be running.  _end may be called again; mskf_ctx_destroy drains the stream as always;
 *   - a failed _begin leaves nothing pending and nothing running: if it had enqueued work, it synchronises the context's
 *     stream before it returns the error. */
int mskf_fe_track_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, const mskf_fe_track_args *args);
int mskf_fe_track_batch_end(mskf_ctx *ctx);

/* curr cam0 pyramid becomes the prev pyramid (image_processor.cpp:194) */
int mskf_fe_swap(mskf_stream *s);

/* ---- a whole front-end frame on the device
 * Replaces, for every frame after the first, ALL of cg::ImageProcessor::stereoCallback between the image copy and
 * publish() (image_processor.cpp:148-200): createImagePyramids, trackFeatures (:352-532), addNewFeatures (:622-756),
 * pruneGridFeatures (:758-768) and the state rotation (:192-200).  The live grid stays in device memory from frame to
 * frame; one call enqueues pyramids + detector, the temporal and stereo track of the previous features, the bookkeeping
 * between (survivors, occupancy, detections, per-cell sieve, candidates), the candidates' stereo track and the bookkeeping
 * after it (vacancy fill, ids, pruning), and returns the published grid: ids, lifetimes, pixels and the undistorted
 * points publish() writes into the message (:1137-1182).  One host wait per frame instead of two, no points travel to
 * the device.  With MSKF_COMPAT_Q5_NO_RANSAC cleared the 2-point RANSAC of :482-500 / :911-1135 runs inside the call too,
 * between the track of the previous features and the bookkeeping (its draws come from a counter the stream keeps on the
 * device).  Limits: grid_min / grid_max_feature_num <= 16 and bookkeeping lists that fit the kernel's LDS
 * (mskf_fe_grid_capacity returns 0 otherwise); the caller keeps such streams, and the first frame of every stream, on the
 * mskf_fe_track path and hands the grid over with mskf_fe_set_grid. */
typedef struct mskf_fe_frame_args {
    double Hpred[9];              /* in: K R_p_c K^-1 of this frame (image_processor.cpp:335-340) */
    int32_t capacity;             /* in: entries each output array holds, >= mskf_fe_grid_capacity(stream) */
    int32_t n;                    /* out: features of the published grid, in flatten order (ascending grid code) */
    uint64_t *id;                 /* out */
    int32_t *lifetime;            /* out */
    mskf_point2f *cam0, *cam1;    /* out: pixels */
    mskf_point2f *und0, *und1;    /* out: undistorted normalised coordinates */
    int32_t before_tracking, after_tracking, after_matching, after_ransac;   /* out: TrackingInfo (:514-530) */
    int32_t n_candidates, n_new;  /* out: candidates stereo-matched for the vacancies, features created */
    uint64_t next_feature_id;     /* out: the stream's id counter after this frame */
    double R_p_c[2][9];           /* in: rotation previous -> current frame of cam0 and of cam1 (integrateImuData, :850-889); read by the
                                   *     2-point RANSAC only (MSKF_COMPAT_Q5_NO_RANSAC cleared) */
    uint64_t ransac_draws;        /* out: numbers the stream's RANSAC generator has drawn so far (a host-side frame continues from it) */
} mskf_fe_frame_args;
/* entries a published grid can have: (grid codes) x grid_max_feature_num; 0 = this stream keeps its books on the host */
int mskf_fe_grid_capacity(mskf_stream *s);
/* Hand the device the grid a host-side frame has published (the first frame of a stream), with the id counter, the
 * tracking counters that survive frames without features (:383) and the draw counter of the RANSAC generator.  Synchronous. */
int mskf_fe_set_grid(mskf_stream *s, int n, const uint64_t *id, const int32_t *lifetime, const mskf_point2f *cam0, const mskf_point2f *cam1,
                     const mskf_point2f *und0, const mskf_point2f *und1, uint64_t next_feature_id, const int32_t tracking_counters[3],
                     uint64_t ransac_draws);
/* streams / args must stay valid until _end; the pyramid swap of :194 is part of the call */
int mskf_fe_frame_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, const uint8_t *const *cam0, const uint8_t *const *cam1,
                              int on_device, mskf_fe_frame_args *args);
int mskf_fe_frame_batch_end(mskf_ctx *ctx);

/* ---- opt-in equalisation of the pushed images
 * Off by default.  With mode 1 (global histogram equalisation) or 2 (CLAHE) every push of the stream equalises level 0 of
 * both cameras on the device before the pyramid and the detector read it (DESIGN.md §3 has the arithmetic, which restates
 * OpenCV's equalizeHist and 8-bit CLAHE::apply): at most three more launches per push call, for all equalising streams of the
 * call together; streams with mode 0 take no part and see no change.  The result is written into the stream's own level-0
 * plane, whatever the push delivered: host images and device images (on_device 1) are equalised from where the push put or
 * found them, a BORROWED device image (on_device 2) is read once during the push and not needed afterwards (the caller may
 * overwrite it as soon as the push's work is done; the stream never writes it).  The pyramid, the detector, both track calls,
 * the device frame and mskf_fe_get_level all read the equalised plane.
 * The three launches are not timed by the per-kernel timing (there is no MSKF_K_* kind for them).
 * mskf_fe_set_equalize validates before it touches anything: MSKF_ERR_INVALID for an unknown mode, tiles_x / tiles_y < 1 or
 * more tiles than pixels in a dimension, a negative or non-finite clip_limit (0 = no clip), and while a track or device-frame
 * batch of the stream's context is pending (mskf_last_error names it).  It allocates the stream's LUT and histogram scratch
 * (call it outside a run: replacing an earlier setting synchronises the device) and takes effect with the next push.
 * The scratch is 2 x 256 x tiles_x x tiles_y bytes per stream and the histogram launch has one workgroup per tile: tile counts
 * far beyond the usual 8 x 8 are accepted up to one tile per pixel, but cost memory and launches in proportion. */
typedef struct mskf_fe_equalize {
    int32_t mode;                 /* 0 off, 1 global, 2 CLAHE */
    int32_t tiles_x, tiles_y, _pad;
    double clip_limit;
} mskf_fe_equalize;
int mskf_fe_set_equalize(mskf_stream *s, const mskf_fe_equalize *cfg);
int mskf_fe_get_equalize(mskf_stream *s, mskf_fe_equalize *out);

/* ---- opt-in input pixel formats: 16-bit grey, interleaved colour and 8-bit Bayer images, converted on the device
 * MSKF_PIX_GRAY8 by default, and then nothing new runs.  With another format every push of the stream takes raw bytes in that
 * format through the same pointers (const uint8_t *, rows dense or `pitch` bytes apart as the entry point says) and converts
 * them to the 8-bit grey level 0 of both cameras on the device before anything else reads it (DESIGN.md §3 has the integer
 * arithmetic): one more launch per push call, for all converting streams of the call together; streams on GRAY8 take no
 * part and see no change; streams of different formats mix freely in a batch.  From level 0 on everything is as if the caller
 * had pushed the converted 8-bit image: the equalisation, if on, runs on the converted plane, in place.
 *   GRAY16: little-endian unsigned 16-bit, g = min(v >> shift, 255) (12-bit data: shift 4, 10-bit: 2, full 16-bit: 8); image
 *           pointers and pitch must be 2-byte aligned (a push that is not is refused and changes nothing);
 *   RGB8 / BGR8 / RGBA8 / BGRA8: interleaved, the fourth byte is ignored; Y = (9798 R + 19235 G + 3735 B + 16384) >> 15;
 *   BAYER_*8: 8-bit mosaic, bilinear demosaic with REFLECT_101 borders, then the same luma.  The name spells the 2 x 2 tile at
 *           the image's top-left corner in reading order (row 0: x = 0, 1; row 1: x = 0, 1).  This is NOT OpenCV's naming.
 * The result is written into the stream's own level-0 plane, whatever the push delivered: host images (on_device 0) are
 * copied into the stream's raw staging and converted from there; device images (on_device 1 and 2) are converted from where
 * the caller has them.  Nothing stays borrowed: a borrowed image (on_device 2) is read once during the push and never
 * written, and the caller may overwrite it as soon as the push's work is done (mskf_ctx_sync).
 * The launch is not timed by the per-kernel timing (there is no MSKF_K_* kind for it).
 * mskf_fe_set_input_format validates before it touches anything: MSKF_ERR_INVALID for an unknown format, a shift outside
 * 0 .. 8, a shift other than 0 with a format other than GRAY16, and while a track or device-frame batch of the stream's
 * context is pending (mskf_last_error names it).  For a format other than GRAY8 it allocates the stream's raw staging
 * (2 x width x height x bytes per pixel of device memory, for host pushes); setting GRAY8 again releases it and the stream is
 * exactly as before.  Call it outside a run (replacing an earlier setting synchronises the device); it takes effect with
 * the next push. */
enum {
    MSKF_PIX_GRAY8 = 0, MSKF_PIX_GRAY16 = 1, MSKF_PIX_RGB8 = 2, MSKF_PIX_BGR8 = 3, MSKF_PIX_RGBA8 = 4, MSKF_PIX_BGRA8 = 5,
    MSKF_PIX_BAYER_RGGB8 = 6, MSKF_PIX_BAYER_GRBG8 = 7, MSKF_PIX_BAYER_GBRG8 = 8, MSKF_PIX_BAYER_BGGR8 = 9
};
typedef struct mskf_fe_input_format { int32_t format; int32_t shift; } mskf_fe_input_format;
int mskf_fe_set_input_format(mskf_stream *s, const mskf_fe_input_format *cfg);
int mskf_fe_get_input_format(mskf_stream *s, mskf_fe_input_format *out);

/* ---- opt-in per-camera image masks: which pixels are scene
 * Off by default, and then nothing new runs or is allocated.  A stream may hold one mask per camera (cam0, cam1, each optional)
 * of the stream's level-0 size: an 8-bit plane with a pitch in which a pixel != 0 is USABLE and 0 is masked out (the opposite of
 * some other stacks' convention).  `margin` (0 .. 64) erodes the usable set when the mask is set, on the host: a pixel stays
 * usable iff every pixel of the image within Chebyshev distance `margin` is non-zero; pixels outside the image count as usable.
 * A detector score at x reads the pixels x - 5 .. x + 4 in both directions, so a mask (or its margin) should reach at least
 * 5 pixels beyond a hard edge.  DESIGN.md §3 has the contract:
 *   detector (cam0 mask): a masked-out pixel is never recorded as a cell maximum; everything else (scores, the floor, ties, the
 *           keys) is unchanged: the per-cell reduction runs over the score map with the masked pixels' scores set to 0.  One
 *           launch as before, of another instantiation of the kernel, for every push call that has a stream with a cam0 mask;
 *   point gate: one more launch (MSKF_K_FE_MASK) behind every track launch of a batch that has a masked stream: both track
 *           launches of a device frame, and mskf_fe_track*.  The pixel of a point is ((int)(x + 0.5f), (int)(y + 0.5f)).  A point
 *           with status bit 0 whose cam0 pixel (out0) is masked out is lost as a track loses one: status 0, out1 = und0 = und1 = 0,
 *           out0 kept; otherwise a point with bit 1 whose cam1 pixel (out1) is masked out loses bit 1 and nothing else (as behind
 *           the epipolar gate).  The bookkeeping drops what the status bits say, so the TrackingInfo counts of a device frame
 *           count mask losses as tracking (cam0) and matching (cam1) losses.
 * A new mask applies to the detector from the stream's next push and to the gate from its next track or frame call.
 * mskf_fe_set_mask validates before it touches anything: MSKF_ERR_INVALID for a null cfg, with a plane given a size other than the
 * stream's, a pitch below the width or a margin outside 0 .. 64, and while a track or device-frame batch of the stream's context is
 * pending (mskf_last_error names it); the previous mask then stays in force.  Both planes null = off: the stream's planes are
 * released and it is exactly as before.  The planes are read during the call (caller memory, a blocking copy); a replaced plane is
 * released after the context's stream has been synchronised: call it outside a run. */
typedef struct mskf_fe_mask {
    const uint8_t *cam0, *cam1;   /* NULL: that camera is not masked */
    int32_t width, height, pitch; /* of both planes; pitch in bytes */
    int32_t margin;               /* 0 .. 64 */
} mskf_fe_mask;
int mskf_fe_set_mask(mskf_stream *s, const mskf_fe_mask *cfg);
/* The mask of camera `cam` (0 / 1) as the stream holds it, eroded, one byte per pixel (0 masked out, 255 usable), dense;
 * *w = *h = 0 when that camera has none (nothing is written to out, which may then be NULL).  No device call. */
int mskf_fe_get_mask(mskf_stream *s, int cam, uint8_t *out, int capacity, int *w, int *h, int *margin);

/* ---- opt-in ZNCC patch check of temporal tracks and stereo matches: is it still the same piece of scene?
 * Off by default, and then nothing new runs or is allocated.  One more launch (k_patch_points, MSKF_K_FE_PATCH) behind every track
 * launch of a batch that has a checking stream: both track launches of a device frame, and mskf_fe_track*; behind the mask gate where
 * both are on (the two only remove points, so the result does not depend on the order).  It is a pure function of the track's
 * outputs and the level-0 images, a pixel rule and a threshold ("Patch check", has the arithmetic, which is exact):
 * a (2 half + 1)^2 patch of bilinear samples (fractions in 32nds, replicated border) around a point in each of two images, and
 * their zero-mean normalised cross-correlation against a threshold.
 *   temporal (mode bit 1; track calls with do_temporal = 1, points with status bit 0): in_pts[pt] in the previous cam0 image against
 *           out0[pt] in the current one.  A failing point is lost as a track loses one: status 0, out1 = und0 = und1 = 0, out0 kept.
 *   stereo  (mode bit 2; points with status bit 1 of any track call): out0[pt] in the current cam0 image against out1[pt] in the
 *           current cam1 image.  A failing point loses bit 1 and nothing else (as behind the epipolar gate).
 * The temporal comparison runs first; a point lost there is not compared again.  Two flat patches pass (nothing to judge), a flat one
 * against a textured one fails.  ZNCC ignores gain and offset.  The bookkeeping drops what the status bits say, so the TrackingInfo
 * counts of a device frame count these losses as tracking and matching losses.  The temporal comparison is frame to frame: it sees
 * jumps and occlusions, not slow drift (that would need a stored template per feature).
 * mskf_fe_set_patch_check validates before it touches anything: MSKF_ERR_INVALID for a null cfg, an unknown mode bit, `half` outside
 * 2 .. 7 with mode != 0, a threshold outside [0, 1] or not finite, and while a track or device-frame batch of the stream's context is
 * pending (mskf_last_error names it); the previous setting then stays in force.  mode = 0 = off.  A new setting applies from the
 * stream's next track or frame call.  No device call. */
enum { MSKF_PATCH_TEMPORAL = 1, MSKF_PATCH_STEREO = 2 };
typedef struct mskf_fe_patch_check {
    int32_t mode, half;                        /* mode: MSKF_PATCH_* bits, 0 = off; half: 2 .. 7 */
    float min_zncc_temporal, min_zncc_stereo;  /* in [0, 1] */
} mskf_fe_patch_check;
int mskf_fe_set_patch_check(mskf_stream *s, const mskf_fe_patch_check *cfg);
int mskf_fe_get_patch_check(mskf_stream *s, mskf_fe_patch_check *out);      /* a stream never set: {0, 4, 0.8, 0.8} */

/* ---- opt-in forward-backward check of temporal tracks and stereo matches: does LK, run backwards, return to where it started?
 * Off by default, and then nothing new runs or is allocated.  One more launch (k_fb_points, MSKF_K_FE_FB) behind every track launch
 * of a batch that has a checking stream: both track launches of a device frame, and mskf_fe_track*; behind the mask gate and the
 * patch gate, whose survivors it sees (it is the most expensive gate).  It is a pure function of the track's outputs and the resident
 * pyramids ("Forward-backward check"): the backward track is the forward track's own code over all pyramid levels with
 * the pyramids' roles swapped, started at the KNOWN ORIGIN (not at the tracked point: the lenient variant), and its result is
 * compared with that origin: passes iff the backward track succeeded and dx * dx + dy * dy <= max_error * max_error (float32, each
 * operation rounded; a NaN fails; threshold 0 passes only an exact return).
 *   temporal (mode bit 1; track calls with do_temporal = 1, points with status bit 0): template at out0[pt] in the current cam0
 *           image, searched in the previous one from in_pts[pt], compared with in_pts[pt].  A failing point is lost as a track loses
 *           one: status 0, out1 = und0 = und1 = 0, out0 kept.
 *   stereo  (mode bit 2; points with status bit 1 of any track call): template at out1[pt] in the current cam1 image, searched in
 *           the current cam0 image from out0[pt], compared with out0[pt].  A failing point loses bit 1 and nothing else.
 * The temporal half runs first; a point lost there is not tracked back again.  What it cannot see: a stereo match on the next
 * period of a repetitive texture is consistent in both directions (that stays with the patch check and the epipolar gate).  The
 * defaults are starting values nobody has tuned.
 * mskf_fe_set_fb_check validates before it touches anything: MSKF_ERR_INVALID for a null cfg, an unknown mode bit, a threshold that is
 * not finite or lies outside [0, 64], and while a track or device-frame batch of the stream's context is pending (mskf_last_error
 * names it); the previous setting then stays in force.  mode = 0 = off.  A new setting applies from the stream's next track or frame
 * call.  No device call. */
enum { MSKF_FB_TEMPORAL = 1, MSKF_FB_STEREO = 2 };
typedef struct mskf_fe_fb_check {
    int32_t mode;                                /* MSKF_FB_* bits, 0 = off */
    float max_error_temporal, max_error_stereo;  /* level-0 pixels, finite, 0 .. 64 */
} mskf_fe_fb_check;
int mskf_fe_set_fb_check(mskf_stream *s, const mskf_fe_fb_check *cfg);
int mskf_fe_get_fb_check(mskf_stream *s, mskf_fe_fb_check *out);      /* a stream never set: {0, 1.0f, 1.0f} */

/* ---- opt-in camera models beyond the two of mskf_calib: OpenCV's rational radtan, Kalibr's fov distortion, the double-sphere camera.
 * Off by default, and then nothing new runs or is allocated.  The intrinsics fx fy cx cy stay those of mskf_calib; each camera of
 * a stream takes a model of its own ("Extended camera models", has the formulas and their operation order):
 *   MSKF_MODEL_RADTAN8  k1 k2 p1 p2 k3 k4 k5 k6, OpenCV's order (cv::projectPoints / cv::undistortPoints, five fixed-point steps).  A
 *                       five-coefficient calibration is k4 = k5 = k6 = 0; with k3 .. k6 = 0 it gives the bits of MSKF_MODEL_RADTAN.
 *   MSKF_MODEL_FOV      w (radians, 0 < w < pi): rd = atan(2 ru tan(w / 2)) / w.  A pixel with rd w >= pi/2 is outside the domain.
 *   MSKF_MODEL_DS       xi, alpha (-1 < xi <= 1, 0 <= alpha <= 1), Usenko et al. 2018, rays on the z = 1 plane.  Outside the domain:
 *                       the paper's projection condition fails or the denominator is not positive; alpha > 0.5 and
 *                       r2 > 1 / (2 alpha - 1); an un-projected ray with z <= 0 (fields of view that reach 90 degrees off axis).
 *   MSKF_MODEL_RADTAN / MSKF_MODEL_EQUIDISTANT with four coefficients are accepted too and put the camera back on the base path.
 * A point outside the domain (the base models never refuse one): where the stereo guess cannot be formed the point takes no stereo
 * trip (out1 = 0, status bit 1 clear); a point whose und0 or und1 cannot be computed loses status bit 1 as behind the epipolar gate,
 * and the coordinates that could not be computed are 0.  Status bit 0, out0 and the temporal result are untouched.
 * A track or device-frame batch in which a stream has an extended model on either camera launches the extended instantiation of the
 * track kernel (k_track4_ext, timed as MSKF_K_LK) in place of k_track4, for both track launches of a device frame and for
 * mskf_fe_track*; base-model streams of such a batch get the bits they get from k_track4.  The gates run behind it as before.
 * mskf_fe_set_camera_model validates before it touches anything: MSKF_ERR_INVALID for a null pointer, cam not 0 or 1, an unknown
 * model, a coefficient that is not finite (all eight are looked at; those past the model's own are kept and ignored), w outside
 * (0, pi), xi or alpha outside their ranges, and while a track or device-frame batch of the stream's context is pending
 * (mskf_last_error names the reason); the previous setting then stays in force.  A new setting applies from the stream's next track
 * or frame call.  No device call: the coefficients travel with the staged descriptors. */
enum { MSKF_MODEL_RADTAN8 = 2, MSKF_MODEL_FOV = 3, MSKF_MODEL_DS = 4 };      /* continue MSKF_MODEL_* */
typedef struct mskf_fe_camera_model { int32_t cam, model; double coeffs[8]; } mskf_fe_camera_model;
int mskf_fe_set_camera_model(mskf_stream *s, const mskf_fe_camera_model *cfg);
int mskf_fe_get_camera_model(mskf_stream *s, int cam, mskf_fe_camera_model *out);      /* a stream never set: what mskf_calib gave it */

/* ---- opt-in deeper LK pyramids: a stream may run every pyramidal LK over L = 5 .. 8 levels instead of 4, which widens the capture range
 * of the temporal track, of both stereo matches and of the backward tracks of the forward-backward check ("Deeper LK
 * pyramids").  4 is the default, and then nothing new runs or is allocated.  Deeper is not better: top levels without structure send the
 * guess astray, so the depth is a per-stream choice (README has measured counts).
 *   pyramid   level l (4 <= l < L) is pyr_down of level l - 1, ((w + 1) / 2, (h + 1) / 2), the function that makes the levels 1 .. 3; the
 *             three pyramids' extra planes live in an arena of the stream's own (3 x sum of w_l h_l bytes, rounded up per level), allocated
 *             by this call, freed with the stream, rotated by mskf_fe_swap and by the device frame as the levels 0 .. 3 are;
 *   LK        the arithmetic of the four-level track with 4 replaced by L: sc = 2^-l, the guess scaled once at level L - 1 and doubled per
 *             level, status 0 set by level 0 only, a level that fails its bounds or minEig test passes the guess on unchanged;
 *   launches  one more launch (k_pyr_down_deep, MSKF_K_PYR_DEEP) behind the pyramid launch of a push with a deep stream; a track or
 *             device-frame batch with a deep stream launches k_track4_deep (timed as MSKF_K_LK) in place of k_track4 / k_track4_ext, and
 *             k_fb_points_deep in place of k_fb_points; the other streams of such a batch get the bits they always got.
 * mskf_fe_set_lk_levels validates before it touches anything: MSKF_ERR_INVALID for levels outside 4 .. 8, for an L whose level L - 1 has a
 * side below 15 pixels at the stream's calibrated size (752 x 480 allows up to 6, 3840 x 2160 allows 8; mskf_last_error names the largest L
 * the size allows), after the stream's first push, and while a track or device-frame batch of the stream's context is pending. */
int mskf_fe_set_lk_levels(mskf_stream *s, int levels);
int mskf_fe_get_lk_levels(mskf_stream *s, int *levels);      /* a stream never set: 4 */

/* download pyramid level `level` (0..3; up to L - 1 for a stream with mskf_fe_set_lk_levels(L)) of image role 0: prev cam0, 1: curr cam0, 2: curr cam1 (parity tests) */
int mskf_fe_get_level(mskf_stream *s, int role, int level, uint8_t *out, int capacity, int *w, int *h);

/* ---- opt-in 256-bit binary descriptors of points of a resident level-0 image ("Descriptors")
 * Nothing runs or is allocated for a context that never calls these.  A descriptor is upright, single-scale BRIEF: 256 tests
 * (ax, ay, bx, by), offsets within -12 .. 12 (mskf_fe_descriptor_pattern), over 5 x 5 box sums S of the image with a replicated
 * border; for a point (x, y) in level-0 pixels the centre is ((int)(x + 0.5f), (int)(y + 0.5f)), the point is valid iff
 * 0 <= x + 0.5f < width and 0 <= y + 0.5f < height in float32 (false for NaN), and bit t, in byte t >> 3 at bit t & 7, is
 * S(c + a_t) < S(c + b_t), strictly.  An invalid point gets 32 zero bytes and valid 0, a valid one valid 1.  Descriptors are
 * compared by Hamming distance.
 * The image is the stream's level 0 of `role` as mskf_fe_get_level returns it (equalised or converted where those options are on;
 * a mask does not enter); a borrowed device image (on_device 2) is read in place, under the duty to keep it valid that the push
 * states.  Points and results travel through arenas of the call's own: one copy in, one launch (k_fe_describe, one wavefront per
 * point; not timed, there is no MSKF_K_* kind for it) and one copy out for the whole batch.
 * Everything is validated before anything is touched.  MSKF_ERR_INVALID, mskf_last_error naming the reason: a null argument, role
 * outside 0 .. 2, a role whose image the stream does not hold yet (nothing pushed, or no previous image), n < 0, null pts, desc or
 * valid with n > 0, a stream of another context, and while a track, device-frame or describe batch of the context is pending.
 * Pushes and frames enqueued after _begin run behind it on the context's stream: the image pointers are resolved at _begin.  A
 * batch whose every n is 0 is MSKF_OK and leaves nothing pending.  The args and their arrays stay valid until _end. */
typedef struct mskf_fe_describe_args {
    int32_t role;              /* image, as mskf_fe_get_level: 0 prev cam0, 1 curr cam0, 2 curr cam1 */
    int32_t n;                 /* points, >= 0 */
    const mskf_point2f *pts;   /* in: level-0 pixels */
    uint8_t *desc;             /* out: 32 n bytes */
    uint8_t *valid;            /* out: n bytes */
} mskf_fe_describe_args;
int mskf_fe_describe(mskf_stream *s, mskf_fe_describe_args *args);          /* batch of one; synchronises */
int mskf_fe_describe_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_fe_describe_args *args);
int mskf_fe_describe_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_fe_describe_args *args);
int mskf_fe_describe_batch_end(mskf_ctx *ctx);
/* ax, ay, bx, by of test 0, 1, .. 255; no device call */
void mskf_fe_descriptor_pattern(int8_t out[1024]);

/* ---- opt-in brute-force Hamming matcher of those descriptors ("Descriptor matching")
 * Nothing runs or is allocated for a context that never calls these.  A job matches nq query descriptors against nt train
 * descriptors (32 bytes each, 0 .. 65535 of either); query_valid / train_valid are what describe returns (one byte each, != 0 =
 * valid; NULL = all valid).  The distance is the popcount of the XOR, 0 .. 256.  For a valid query, nearest is the valid train of
 * the smallest (distance, index): among equal distances the lowest index wins; dist is that distance and second the smallest
 * distance to a valid train other than nearest (it may equal dist).  Without a valid train, or for an invalid query, nearest = -1
 * and dist = second = 0xFFFF; with exactly one valid train second = 0xFFFF.  idx = nearest iff nearest >= 0, dist <= max_distance,
 * the ratio test holds (ratio == 0: off; second == 0xFFFF: passes; else (float)dist < ratio * (float)second in float32) and, with
 * cross_check != 0, the valid query of the smallest (distance, index) to train `nearest` is this one; otherwise idx = -1.  nearest,
 * dist and second are always the raw values.  n_matches counts the queries with idx >= 0.
 * The calls take a context, not streams: matching reads no image.  Sets and results travel through arenas of the call's own: one
 * copy in, ONE launch (k_fe_match, cross-checked or not; not timed, there is no MSKF_K_* kind for it) and one copy out for the whole
 * batch.  A descriptor set or validity array that several jobs of a batch name by the same (pointer, count) is copied once: a
 * query against K keyframes is K jobs with one query pointer.  The host arrays need no alignment.
 * Everything is validated before anything is touched.  MSKF_ERR_INVALID, mskf_last_error naming the reason: a null ctx or args,
 * n <= 0, nq or nt negative or above 65535, null query with nq > 0, null train with nt > 0, null matches with nq > 0, max_distance
 * outside 0 .. 256, a ratio that is NaN, negative or above 1, and while a match batch of the context is pending (nothing else
 * refuses for it, and it refuses for nothing else).  A batch whose every nq is 0 is MSKF_OK, sets every n_matches to 0 and leaves
 * nothing pending.  The args and their arrays stay valid until _end, which fills matches and n_matches. */
typedef struct mskf_fe_match_args {
    int32_t nq, nt;
    const uint8_t *query, *query_valid;   /* 32 nq bytes; nq bytes or NULL */
    const uint8_t *train, *train_valid;   /* 32 nt bytes; nt bytes or NULL */
    int32_t max_distance;                 /* 0 .. 256 */
    float   ratio;                        /* 0 = off, else (0, 1] */
    int32_t cross_check;
    mskf_match *matches;                  /* out: nq */
    int32_t n_matches;                    /* out */
} mskf_fe_match_args;
int mskf_fe_match(mskf_ctx *ctx, mskf_fe_match_args *args);            /* batch of one; synchronises */
int mskf_fe_match_batch(mskf_ctx *ctx, int n, mskf_fe_match_args *args);
int mskf_fe_match_batch_begin(mskf_ctx *ctx, int n, mskf_fe_match_args *args);
int mskf_fe_match_batch_end(mskf_ctx *ctx);

/* ---- opt-in stereo RANSAC pose check of matched pairs ("Geometric verification")
 * Nothing runs or is allocated for a context that never calls these.  A job takes n pairs (0 .. 4096) of stereo observations, each
 * the four undistorted normalised coordinates (x0, y0, x1, y1) of a feature (what the published feature message carries as u0, v0, u1,
 * v1): query_obs of the frame asked about, train_obs of the keyframe, and says whether the pairs agree on one rigid motion
 * p_k = R p_q + t (query cam0 -> keyframe cam0).  Both sides are triangulated with T_cam1_cam0 (p_c1 = R10 p_c0 + t10); a pair is
 * usable iff its usable byte is != 0 (NULL = all) and both depths are finite and in [min_depth, max_depth].  Hypothesis h = 0 ..
 * n_hypotheses - 1 (1 .. 1024) is fitted to three distinct usable pairs drawn as a function of (seed, h, n_usable) alone; a pair is
 * an inlier of (R, t) iff the query point lands in front of both keyframe cameras (z >= min_depth) and the sum of the four squared
 * differences between its projections and the keyframe's observation is < max_error^2 (strictly; normalised units).  The hypothesis
 * with the most inliers wins, the lowest h among equal counts; its pose is refined by five Gauss-Newton steps on its inlier set.
 * Out: n_usable, n_inliers, best (the winning h, or -1), inlier (n bytes at the ORIGINAL indices, may be NULL), R (row-major), t,
 * info = J^T J of the four residuals per inlier (6 x 6 row-major, order [theta, t], left perturbation; a covariance is sigma^2
 * info^-1 with sigma the caller's observation noise in normalised units), rms of the residuals, and status: 0 ok; 1 no hypothesis
 * (fewer than 3 usable pairs, or every sampled triangle degenerate): best = -1, n_inliers = 0, identity pose, zero info; 2 the
 * refinement failed: R, t are the three-pair fit, info is zero.
 * The calls take a context, not streams: no image is read.  The host triangulates and compacts the usable pairs in _begin; they and
 * the results travel through arenas of the call's own: one copy in, ONE launch (k_fe_verify; not timed) and one copy out (a 64-bit
 * key per 64 hypotheses) for the whole batch; _end re-forms the winner, marks its inliers and refines it on the host.
 * Everything is validated before anything is touched.  MSKF_ERR_INVALID, mskf_last_error naming the reason: a null ctx or args, a
 * batch of n_jobs <= 0, n negative or above 4096, null query_obs or train_obs with n > 0, n_hypotheses outside 1 .. 1024, max_error
 * not > 0 or not finite, depths that are not 0 < min_depth < max_depth < infinity, a T_cam1_cam0 that is not finite, and while a
 * verify batch of the context is pending (nothing else refuses for it, and it refuses for nothing else).  A batch whose every n is
 * 0 is MSKF_OK, fills every job's outputs (status 1) and leaves nothing pending.  The args and their arrays stay valid until _end. */
typedef struct mskf_fe_verify_args {
    int32_t n, n_hypotheses;
    const double *query_obs, *train_obs;  /* 4 n doubles each */
    const uint8_t *usable;                /* n bytes or NULL */
    double T_cam1_cam0[16];
    uint64_t seed;
    double max_error, min_depth, max_depth;
    uint8_t *inlier;                      /* out: n bytes, or NULL */
    int32_t n_usable, n_inliers, best, status;      /* out */
    double R[9], t[3], info[36], rms;     /* out */
} mskf_fe_verify_args;
int mskf_fe_verify(mskf_ctx *ctx, mskf_fe_verify_args *args);            /* batch of one; synchronises */
int mskf_fe_verify_batch(mskf_ctx *ctx, int n_jobs, mskf_fe_verify_args *args);
int mskf_fe_verify_batch_begin(mskf_ctx *ctx, int n_jobs, mskf_fe_verify_args *args);
int mskf_fe_verify_batch_end(mskf_ctx *ctx);

/* ------------------------------------------------------------------ EKF (covariance resident in HBM)
 * Replaces, inside cg::MsckfVio (msckf_vio.cpp):
 *   state_cov part of processModel     :458-469  -> mskf_ekf_propagate
 *   state_cov part of stateAugmentation :564-582 -> mskf_ekf_augment
 *   Feature::initializePosition        feature.hpp:289-450 -> inside mskf_ekf_update (needs_init)
 *   featureJacobian / measurementJacobian / gatingTest / stacking / measurementUpdate
 *                                      :610-935, :986-1017, :1124-1159 -> mskf_ekf_update
 *   clone row/column deletion          :1161-1181 -> mskf_ekf_remove_clone
 *   covariance reset                   :102-112, :1222-1232 -> mskf_ekf_reset
 */
typedef struct mskf_clone_state {   /* CAMState, common/cam_state.h:25-55 */
    double q[4], p[3], q_null[4], p_null[3];
} mskf_clone_state;

typedef struct mskf_ekf_feature {   /* one feature of an update */
    int32_t obs_start, n_obs;       /* range in the observation arrays */
    int32_t needs_init;             /* 1: triangulate from ALL its observations listed in init_* first */
    int32_t init_start, n_init;     /* observation range used for triangulation (all of the feature's obs) */
    int32_t _pad;
    double position[3];             /* in: world position if !needs_init; out: triangulated position */
} mskf_ekf_feature;

typedef struct mskf_ekf_update_args {
    int32_t n_clones;
    int32_t n_feat;
    int32_t n_obs;
    int32_t dof_offset;             /* gating dof = n_obs_j + dof_offset: -1 lost features, 0 pruning (Q12) */
    int32_t apply_row_cap;          /* 1: stop stacking once rows > max_stack_rows (removeLostFeatures only, Q13) */
    int32_t _pad;
    double gravity[3];
    const mskf_clone_state *clones; /* n_clones, in state order */
    mskf_ekf_feature *features;     /* in/out: position, and status in `feat_status` */
    const int32_t *obs_clone;       /* n_obs: clone index of each observation */
    const double *obs_z;            /* n_obs x 4: u0 v0 u1 v1 */
    double *delta_x;                /* out: 21 + 6 n_clones */
    uint8_t *feat_status;           /* out per feature: bit0 triangulation valid, bit1 gating passed (stacked) */
    double *gamma;                  /* out per feature (may be NULL): Mahalanobis gate value */
    int32_t *rows_out;              /* out: number of stacked rows (0 => no update applied) */
    int32_t *diag_out;              /* out, optional (may be NULL), 2 ints: [0] how the stack was compressed: 0 Gram + Cholesky,
                                       1 Householder TSQR, 2 not at all (rows <= active columns, msckf_vio.cpp:818-821);
                                       [1] pivots of the Gram factor below 100 lambda (-1: not computed) */
    double *pos_var_out;            /* out, optional (may be NULL), 3 doubles: P(12,12), P(13,13), P(14,14) AFTER this update, i.e.
                                       what onlineReset tests (msckf_vio.cpp:1194-1196) — they come back with the update's
                                       results, so a caller that updates every frame never needs mskf_ekf_get_pos_var and its
                                       extra wait (clone removal does not touch these entries).  -1 when no stream of the batch
                                       had features (nothing was launched).  ABI v3 */
} mskf_ekf_update_args;

/* What processModel (msckf_vio.cpp:409-469) needs to propagate the covariance over one IMU sample.
 * The host integrates the 16-dim nominal state (predictNewState, :482-531) and hands over these
 * quantities; F, Phi (3rd-order expm + observability fix-up) and Q are formed on the device. */
typedef struct mskf_imu_step {
    double dt;
    double gyro[3], acc[3];   /* bias-corrected measurements (:412-413) */
    double R_t[9];            /* R(q)^T before the step (:422-423) */
    double Phi00[9];          /* R(q_new) R(q_null)^T (:443) */
    double u[3], s[3];        /* u = R(q_null) g, s = u / (u.u) (:445-446) */
    double w1[3], w2[3];      /* [v_null - v_new]x g (:450), [dt v_null + p_null - p_new]x g (:454) */
} mskf_imu_step;

int mskf_ekf_reset(mskf_stream *s, const double *P0 /* 21x21 row-major */);
int mskf_ekf_propagate_imu(mskf_stream *s, int n_steps, const mskf_imu_step *steps);
/* One fused launch for many streams: IMU propagation over n_steps[i] samples followed (J[i] != NULL) by the
 * state augmentation.  mskf_ekf_propagate_imu, mskf_ekf_propagate and mskf_ekf_augment are batches of one of it, so
 * mskf_ekf_propagate_imu followed by mskf_ekf_augment gives the same bits. */
int mskf_ekf_predict_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, const int32_t *n_steps,
                           const mskf_imu_step *const *steps, const double *const *J);
/* position variances P(12,12), P(13,13), P(14,14) for onlineReset (msckf_vio.cpp:1194-1196). Synchronises. */
int mskf_ekf_get_pos_var(mskf_stream *s, double out[3]);
int mskf_ekf_get_pos_var_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, double *out /* 3n */);
int mskf_ekf_get_pos_var_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, double *out /* 3n, filled by _end */);
int mskf_ekf_get_pos_var_batch_end(mskf_ctx *ctx);
/* Covariance half of MsckfVio::publish (msckf_vio.cpp:1262-1293): the 6x6 body-frame pose covariance H P_imu_pose H^T, the 3x3
 * body-frame velocity covariance and, unrotated, the three position variances of mskf_ekf_get_pos_var, 48 doubles per stream.
 * One small kernel for the whole batch on the context's stream, behind whatever the streams' filter halves enqueued before
 * it (no synchronisation needed after an update or a clone removal); it reads its descriptors from pinned host memory and
 * writes the records straight into it: no staging copy.  Same _begin / _end protocol as the position variances, and the two
 * kinds of read-out share one pending slot per context: while either is pending, the other's _begin and _end refuse too. */
int mskf_ekf_get_odom_cov(mskf_stream *s, mskf_odom_cov *out);                                   /* batch of one; synchronises */
int mskf_ekf_get_odom_cov_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_odom_cov *out /* n */);
int mskf_ekf_get_odom_cov_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_odom_cov *out /* n, filled by _end */);
int mskf_ekf_get_odom_cov_batch_end(mskf_ctx *ctx);
int mskf_ekf_propagate(mskf_stream *s, int n_steps, const double *Phi /* n x 21x21 */, const double *Q /* n x 21x21 */);
int mskf_ekf_augment(mskf_stream *s, const double *J /* 6x21 */);
int mskf_ekf_update(mskf_stream *s, mskf_ekf_update_args *args);
int mskf_ekf_update_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_ekf_update_args *args);
/* begin / end halves as for mskf_fe_track_batch; `streams` and `args` must stay valid until _end */
int mskf_ekf_update_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_ekf_update_args *args);
int mskf_ekf_update_batch_end(mskf_ctx *ctx);
/* ---- opt-in direct measurement update: a few caller-supplied rows on the IMU block
 * A Kalman update of the resident covariance with a measurement that is not a feature track: r = H x~ + noise of covariance R,
 * H acting on the 21 IMU error states only (0..2 attitude, 3..5 gyro bias, 6..8 velocity, 9..11 acc bias, 12..14 position,
 * 15..20 extrinsics), 1 .. 6 rows.  A world-frame velocity or position fix is a selector H on columns 6..8 / 12..14 with
 * r = z - state; a zero-velocity update is the former with z = 0.  The arithmetic is measurementUpdate's (msckf_vio.cpp:831-904)
 * with R in place of observation_noise * I, every sum in a fixed order: S = H P H^T + R is factored by Cholesky,
 * gamma = r^T S^-1 r, and when gate > 0 the update is applied only if gamma <= gate (mskf_chi2_table.h has the values);
 * delta_x = K r is returned for the caller to apply to its state (all 21 + 6 n_clones entries: the clones are corrected through
 * their correlation), P <- sym((I - K H) P) in place, one launch for the batch and one more read and write of P.
 * status: 1 applied; 0 gated out; 2 S not positive definite (an indefinite P).  Unless 1, P is untouched and delta_x is zero;
 * gamma is 0 with status 2.  A stream with m = 0 takes no part: status 0, delta_x zero, gamma 0, pos_var_out -1.
 * A direct update is a kind of update batch: it stages through the update's arenas and shares its pending slot, so while
 * either kind is pending the _begin and the _end of the other refuse (MSKF_ERR_INVALID, mskf_last_error names the pending
 * call); it also refuses while a read-out is pending.  MSKF_ERR_INVALID, with nothing grown, enqueued or written, for m outside
 * 0..6, null H / r / R / delta_x with m > 0, a non-finite value in H, r or R, a NaN gate, R not exactly symmetric or with
 * a diagonal entry <= 0, and a stream that appears twice with rows in one batch (the update is in place). */
typedef struct mskf_ekf_direct_args {
    int32_t m;                      /* rows, 0 .. 6 (0: the stream takes no part) */
    int32_t status;                 /* out */
    const double *H;                /* m x 21, row-major */
    const double *r;                /* m: residual, measurement minus prediction */
    const double *R;                /* m x m, row-major, symmetric, positive diagonal */
    double gate;                    /* > 0: Mahalanobis gate; <= 0: none */
    double *delta_x;                /* out: 21 + 6 n_clones */
    double gamma;                   /* out */
    double *pos_var_out;            /* out, optional (may be NULL), 3 doubles: P(12,12), P(13,13), P(14,14) after the call */
} mskf_ekf_direct_args;
int mskf_ekf_update_direct(mskf_stream *s, mskf_ekf_direct_args *args);                          /* batch of one; synchronises */
int mskf_ekf_update_direct_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_ekf_direct_args *args);
/* `streams` and `args` (and what args point to) must stay valid until _end */
int mskf_ekf_update_direct_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_ekf_direct_args *args);
int mskf_ekf_update_direct_batch_end(mskf_ctx *ctx);
int mskf_ekf_remove_clone(mskf_stream *s, int clone_index);
/* Remove up to two clones per stream in one launch: idx[2*i], idx[2*i+1] are clone indices in the CURRENT
 * state order (distinct; -1 = none).  Equivalent to mskf_ekf_remove_clone calls (msckf_vio.cpp:1161-1181). */
int mskf_ekf_remove_clones_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, const int32_t *idx);
/* Diagnostics for tests: raw work buffers of the stream's last update (0 Hs, 1 rowmask, 2 S, 3 T, 4 W, 5 act);
 * 6 is the current covariance plane itself, all ld x ld doubles, of which only [0,d) x [0,d) is live. */
int mskf_ekf_debug_read(mskf_stream *s, int which, void *out, size_t capacity, int *ld_out);
/* Change mskf_ekf_cfg.compression_mode of a live stream (0 auto, 1 Gram + Cholesky only, 2 Householder TSQR always, 3 the rule
 * of msckf_vio.cpp:795-821 as written); takes effect with the stream's next update.  Not while an update of the stream is pending. */
int mskf_ekf_set_compression_mode(mskf_stream *s, int mode);
int mskf_ekf_get_dim(mskf_stream *s, int *d);
int mskf_ekf_get_cov(mskf_stream *s, double *P, int capacity /* doubles */);
int mskf_ekf_set_cov(mskf_stream *s, const double *P, int d);

#ifdef __cplusplus
}
#endif
#endif /* MSKF_HIP_H */
