// mskf_capi_ekf.cpp — C-ABI: EKF entry points (include/mskf_hip.h).  The covariance lives in HBM;
// the host passes small per-frame descriptors (Phi/Q sequence, J, clone states, observation lists).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include "../../../include/mskf_chi2_table.h"
#include "mskf_internal.h"

namespace {
constexpr int kMaxRows = 65536;     // stacked-Jacobian row capacity per stream and update

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Zero-filled device buffer.  The fill is enqueued on the stream the buffer is going to be used on: the context
// streams are hipStreamNonBlocking, so a hipMemset on the null stream is not ordered against their kernels (it is
// asynchronous for device memory) and could land on top of data a kernel had already written.
int dev_alloc(double **p, size_t n, hipStream_t st) {
    MSKF_HIPCHK(hipMalloc((void **)p, n * sizeof(double)));
    MSKF_HIPCHK(hipMemsetAsync(*p, 0, n * sizeof(double), st));
    return MSKF_OK;
}
}  // namespace

struct EkfExtra {  // lives behind EkfStreamState via the stream (kept out of the device header)
    EkfStreamDev desc_static;         // constant part of the stream's descriptors (base_desc)
    bool desc_valid = false;
    double *P_alt = nullptr;          // ping-pong target of clone removal
    std::vector<double *> retired_hs; // stacked-Jacobian blocks from hipMalloc that were outgrown: freed with the stream (hipFree inside a run waits for the whole device)
};
static EkfExtra *extra_of(mskf_stream *s) { return (EkfExtra *)s->ekf_extra; }

int mskf_ekf_stream_init(mskf_stream *s) {
    EkfStreamState &E = s->ekf_state;
    E.max_clones = s->ekf.max_cam_state_size;
    if (E.max_clones < 4 || E.max_clones > MAX_CLONES_DEV) {
        mskf_set_error("max_cam_state_size must be in [4, " + std::to_string(MAX_CLONES_DEV) + "]");
        return MSKF_ERR_UNSUPPORTED;
    }
    if (s->ekf.compression_mode < 0 || s->ekf.compression_mode > 3) {
        // (the field took the place of padding in ABI v1: a caller that never initialised it must hear about it)
        mskf_set_error("mskf_ekf_cfg.compression_mode must be 0 (auto), 1 (Gram only), 2 (Householder TSQR always) or 3 (the reference's rule)");
        return MSKF_ERR_INVALID;
    }
    E.ld = (int)align_up((size_t)(EKF_IMU_DIM + 6 * E.max_clones), 8);
    E.d = EKF_IMU_DIM;
    E.nmax = 4 * E.max_clones;
    int rc;
    const size_t pl = (size_t)E.ld * E.ld;
    hipStream_t st = s->ctx->stream;     // the fills are drained below: the stream may be re-attached to another context later
    // one allocation and one fill for the stream's fixed-size filter buffers (eight of each per stream showed up as
    // thousands of fill kernels in the profile of a 1536-stream run)
    EkfExtra *X = new EkfExtra();
    s->ekf_extra = X;
    {
        auto pad = [](size_t n) { return (n + 31) / 32 * 32; };      // 256-byte aligned sub-buffers
        const size_t n_gate = pad((size_t)EKF_SLOTS * E.nmax * E.nmax), n_act = pad((size_t)E.ld), n_chi = pad(128), n_pl = pad(pl);
        if ((rc = dev_alloc(&E.pool, 5 * n_pl + n_act + n_gate + n_chi, st)) != MSKF_OK) return rc;
        double *q = E.pool;
        E.P = q; q += n_pl; E.T = q; q += n_pl; E.S = q; q += n_pl; E.W = q; q += n_pl; X->P_alt = q; q += n_pl;
        E.act = (int *)q; q += n_act;           // ld ints fit
        E.gate_S = q; q += n_gate;
        E.chi2 = q;
    }
    {
        // stacked Jacobian + row masks: the APPLIED lost-feature stack is capped at max_stack_rows + one block and the pruning
        // stack is five rows per feature the map can hold (every live grid slot), which is what this first block is sized for.
        // The rows are laid out BEFORE the cap, though (every lost feature's block has its place): a frame that loses most of
        // its features at once (a blackout) needs more and grows the buffer, stream-ordered (mskf_ekf_update_batch_begin)
        const int live = s->fe.grid_row * s->fe.grid_col * std::max(s->fe.grid_max_feature_num, 1) + 64;
        const int cap = std::min(kMaxRows, std::max(std::max(2048, s->ekf.max_stack_rows + 4 * E.max_clones + 64), 5 * live));
        if ((rc = dev_alloc(&E.Hs, (size_t)cap * E.ld + (size_t)cap, st)) != MSKF_OK) return rc;
        E.rs = E.Hs + (size_t)cap * E.ld;
        E.max_rows = cap;
    }
    MSKF_HIPCHK(hipStreamSynchronize(st));
    double tab[100];
    tab[0] = 0.0;
    for (int i = 1; i < 100; ++i) tab[i] = s->ekf.chi2_mode == 1 ? mskf_chi2_ppf95[i - 1] : mskf_chi2_ppf05[i - 1];  // msckf_vio.cpp:181-185
    MSKF_HIPCHK(hipMemcpy(E.chi2, tab, sizeof(tab), hipMemcpyHostToDevice));
    return MSKF_OK;
}

void mskf_ekf_stream_free(mskf_stream *s) {
    EkfStreamState &E = s->ekf_state;
    if (E.pool) (void)hipFree(E.pool);          // P, T, S, W, P_alt, act, gate_S, chi2
    if (E.Hs) { if (E.hs_async) (void)hipFreeAsync(E.Hs, s->ctx_ekf->stream); else (void)hipFree(E.Hs); }      // Hs + rowmask
    if (EkfExtra *X = extra_of(s)) {
        for (double *p : X->retired_hs) (void)hipFree(p);
        delete X;
        s->ekf_extra = nullptr;
    }
}

// The per-stream part of a descriptor that never changes (noise levels, extrinsics, buffer pointers that are only
// replaced together with `desc_valid = false`) is built once and copied; d and the ping-pong P are patched in.
static void base_desc(const mskf_stream *s, EkfStreamDev &D) {
    const EkfStreamState &E = s->ekf_state;
    EkfExtra *X = extra_of(const_cast<mskf_stream *>(s));
    if (!X->desc_valid) {
        EkfStreamDev &T = X->desc_static;
        std::memset(&T, 0, sizeof(T));
        T.ld = E.ld;
        T.sigma2 = s->ekf.noise_feature * s->ekf.noise_feature;   // msckf_vio.cpp:74,81
        T.max_stack_rows = s->ekf.max_stack_rows;
        T.qr_mode = s->ekf.compression_mode;
        T.chi2 = E.chi2;
        T.remove_index = T.remove_index2 = -1;
        // continuous_noise_cov diagonal blocks: gyro, gyro bias, acc, acc bias (msckf_vio.cpp:70-80, 174-178)
        T.qc[0] = s->ekf.noise_gyro * s->ekf.noise_gyro;
        T.qc[1] = s->ekf.noise_gyro_bias * s->ekf.noise_gyro_bias;
        T.qc[2] = s->ekf.noise_acc * s->ekf.noise_acc;
        T.qc[3] = s->ekf.noise_acc_bias * s->ekf.noise_acc_bias;
        T.T = E.T; T.S = E.S; T.W = E.W; T.act = E.act; T.gate_S = E.gate_S; T.nmax = E.nmax;
        hm::Rigid T01 = hm::Rigid::from_rowmajor16(s->calib.T_cam1_cam0);   // CAMState::T_cam0_cam1, msckf_vio.cpp:121-122
        std::memcpy(T.R_c0_c1, T01.R.m, sizeof(T.R_c0_c1));
        for (int i = 0; i < 3; ++i) T.t_c0_c1[i] = T01.t[i];
        hm::Rigid Tib = hm::Rigid::from_rowmajor16(s->calib.T_imu_body).inverse();    // IMUState::T_imu_body, msckf_vio.cpp:124-125
        std::memcpy(T.R_imu_body, Tib.R.m, sizeof(T.R_imu_body));
        X->desc_valid = true;
    }
    D = X->desc_static;
    D.P = E.P; D.d = E.d;
    D.Hs = E.Hs; D.rowmask = (unsigned long long *)E.rs;
}

extern "C" int mskf_ekf_reset(mskf_stream *s, const double *P0) {
    if (!s || !P0) return MSKF_ERR_INVALID;
    EkfStreamState &E = s->ekf_state;
    MSKF_HIPCHK(hipSetDevice(s->ctx_ekf->device));
    hipStream_t st = s->ctx_ekf->stream;       // everything on the stream's own queue: the null stream is not ordered against it
    MSKF_HIPCHK(hipMemsetAsync(E.P, 0, sizeof(double) * (size_t)E.ld * E.ld, st));
    MSKF_HIPCHK(hipMemcpy2DAsync(E.P, sizeof(double) * E.ld, P0, sizeof(double) * EKF_IMU_DIM, sizeof(double) * EKF_IMU_DIM, EKF_IMU_DIM,
                                 hipMemcpyHostToDevice, st));
    MSKF_HIPCHK(hipStreamSynchronize(st));
    E.d = EKF_IMU_DIM;
    return MSKF_OK;
}

extern "C" int mskf_ekf_set_cov(mskf_stream *s, const double *P, int d) {
    if (!s || !P) return MSKF_ERR_INVALID;
    EkfStreamState &E = s->ekf_state;
    if (d < EKF_IMU_DIM || (d - EKF_IMU_DIM) % 6 || d > EKF_IMU_DIM + 6 * E.max_clones) return MSKF_ERR_CAPACITY;
    MSKF_HIPCHK(hipSetDevice(s->ctx_ekf->device));
    hipStream_t st = s->ctx_ekf->stream;
    MSKF_HIPCHK(hipMemsetAsync(E.P, 0, sizeof(double) * (size_t)E.ld * E.ld, st));
    MSKF_HIPCHK(hipMemcpy2DAsync(E.P, sizeof(double) * E.ld, P, sizeof(double) * d, sizeof(double) * d, d, hipMemcpyHostToDevice, st));
    MSKF_HIPCHK(hipStreamSynchronize(st));
    E.d = d;
    return MSKF_OK;
}

extern "C" int mskf_ekf_set_compression_mode(mskf_stream *s, int mode) {
    if (!s) return MSKF_ERR_INVALID;
    if (mode < 0 || mode > 3) { mskf_set_error("compression_mode must be 0 (auto), 1 (Gram only), 2 (Householder TSQR always) or 3 (the reference's rule)"); return MSKF_ERR_INVALID; }
    if (s->ctx_ekf->pend_upd.active) { mskf_set_error("an update batch of the stream's context is pending"); return MSKF_ERR_INVALID; }
    s->ekf.compression_mode = mode;
    extra_of(s)->desc_valid = false;          // the cached descriptor carries the mode
    return MSKF_OK;
}

extern "C" int mskf_ekf_get_dim(mskf_stream *s, int *d) {
    if (!s || !d) return MSKF_ERR_INVALID;
    *d = s->ekf_state.d;
    return MSKF_OK;
}

extern "C" int mskf_ekf_get_cov(mskf_stream *s, double *P, int capacity) {
    if (!s || !P) return MSKF_ERR_INVALID;
    EkfStreamState &E = s->ekf_state;
    if (capacity < E.d * E.d) return MSKF_ERR_CAPACITY;
    MSKF_HIPCHK(hipSetDevice(s->ctx_ekf->device));
    MSKF_HIPCHK(hipStreamSynchronize(s->ctx_ekf->stream));
    MSKF_HIPCHK(hipMemcpy2D(P, sizeof(double) * E.d, E.P, sizeof(double) * E.ld, sizeof(double) * E.d, E.d, hipMemcpyDeviceToHost));
    return MSKF_OK;
}

// The one prediction routine.  Per stream n_steps[i] IMU steps (Phi_k, Q_k formed inside k_ekf_propagate) or, with Phi / Q
// given, n_steps[i] pairs (Phi_k, Q_k) formed by the caller; then the state augmentation with J[i] where it is not NULL.
// One staging copy through pred_arena and one launch for the whole batch; the single-stream calls are batches of one.
static int predict(mskf_ctx *ctx, int n, mskf_stream *const *streams, const int32_t *n_steps, const mskf_imu_step *const *steps,
                   const double *const *Phi, const double *const *Q, const double *const *J) {
    int rc = mskf_refuse_if_owned(ctx, MSKF_ARENAS_PRED);
    if (rc != MSKF_OK) return rc;
    const size_t nn = EKF_IMU_DIM * EKF_IMU_DIM, j_bytes = align_up(sizeof(double) * 6 * EKF_IMU_DIM, 64);
    auto seq_bytes = [&](int i) { return align_up((Phi ? sizeof(double) * 2 * nn : sizeof(mskf_imu_step)) * (size_t)n_steps[i], 64); };
    size_t bytes = align_up(sizeof(EkfStreamDev) * (size_t)n, 64);
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const mskf_stream *s = streams[i];
        if (!s || s->ctx_ekf != ctx || n_steps[i] < 0 || (n_steps[i] && (Phi ? !Phi[i] || !Q[i] : !steps[i]))) return MSKF_ERR_INVALID;
        if (J[i] && s->ekf_state.d + 6 > EKF_IMU_DIM + 6 * s->ekf_state.max_clones) { mskf_set_error("clone capacity exceeded"); return MSKF_ERR_CAPACITY; }
        bytes += seq_bytes(i) + (J[i] ? j_bytes : 0);
        any |= n_steps[i] > 0 || J[i];
    }
    if (!any) return MSKF_OK;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if ((rc = ctx->pred_arena.fence_wait()) != MSKF_OK || (rc = ctx->pred_arena.ensure(bytes)) != MSKF_OK) return rc;
    char *h = ctx->pred_arena.h, *dv = ctx->pred_arena.d;
    EkfStreamDev *D = (EkfStreamDev *)h;
    size_t off = align_up(sizeof(EkfStreamDev) * (size_t)n, 64);
    for (int i = 0; i < n; ++i) {
        base_desc(streams[i], D[i]);
        D[i].n_steps = n_steps[i];
        if (n_steps[i] > 0 && Phi) {
            double *pq = (double *)(h + off);
            for (int k = 0; k < n_steps[i]; ++k) {
                std::memcpy(pq + (size_t)k * 2 * nn, Phi[i] + (size_t)k * nn, sizeof(double) * nn);
                std::memcpy(pq + (size_t)k * 2 * nn + nn, Q[i] + (size_t)k * nn, sizeof(double) * nn);
            }
            D[i].PhiQ = (const double *)(dv + off);
        } else if (n_steps[i] > 0) {
            std::memcpy(h + off, steps[i], sizeof(mskf_imu_step) * (size_t)n_steps[i]);
            D[i].imu_steps = (const mskf_imu_step *)(dv + off);
        }
        off += seq_bytes(i);
        if (J[i]) {
            std::memcpy(h + off, J[i], sizeof(double) * 6 * EKF_IMU_DIM);
            D[i].J = (const double *)(dv + off);
            off += j_bytes;
        }
    }
    DrainOnError drain{st, true};
    { const MskfCopy cp = {dv, h, off}; if ((rc = mskf_copy_async(ctx, &cp, 1)) != MSKF_OK) return rc; }
    if ((rc = ctx->pred_arena.fence_record(st)) != MSKF_OK) return rc;
    {
        const int ts = mskf_t_begin(ctx, MSKF_K_EKF_PROPAGATE);
        ekf_launch_propagate((const EkfStreamDev *)dv, n, st);
        mskf_t_end(ctx, ts, n);
    }
    MSKF_HIPCHK(hipGetLastError());
    drain.armed = false;
    for (int i = 0; i < n; ++i) if (J[i]) streams[i]->ekf_state.d += 6;
    return MSKF_OK;
}

extern "C" int mskf_ekf_predict_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, const int32_t *n_steps,
                                      const mskf_imu_step *const *steps, const double *const *J) {
    if (!ctx || n <= 0 || !streams || !n_steps || !steps || !J) return MSKF_ERR_INVALID;
    return predict(ctx, n, streams, n_steps, steps, nullptr, nullptr, J);
}

extern "C" int mskf_ekf_propagate(mskf_stream *s, int n_steps, const double *Phi, const double *Q) {
    if (!s) return MSKF_ERR_INVALID;
    mskf_stream *ss[1] = {s};
    const int32_t ns[1] = {n_steps};
    const double *phi[1] = {Phi}, *q[1] = {Q}, *j[1] = {nullptr};
    return predict(s->ctx_ekf, 1, ss, ns, nullptr, phi, q, j);
}

extern "C" int mskf_ekf_propagate_imu(mskf_stream *s, int n_steps, const mskf_imu_step *steps) {
    if (!s) return MSKF_ERR_INVALID;
    mskf_stream *ss[1] = {s};
    const int32_t ns[1] = {n_steps};
    const mskf_imu_step *st[1] = {steps};
    const double *j[1] = {nullptr};
    return predict(s->ctx_ekf, 1, ss, ns, st, nullptr, nullptr, j);
}

extern "C" int mskf_ekf_augment(mskf_stream *s, const double *J) {
    if (!s || !J) return MSKF_ERR_INVALID;
    mskf_stream *ss[1] = {s};
    const int32_t ns[1] = {0};
    const mskf_imu_step *st[1] = {nullptr};
    const double *j[1] = {J};
    return predict(s->ctx_ekf, 1, ss, ns, st, nullptr, nullptr, j);
}

// ---- read-outs: position variances (3 doubles per stream) and the published odometry covariance (48: mskf_odom_cov).
// One routine and one pending slot (mskf_ctx::pend_ro) for both kinds: the kernel reads its descriptors from the pinned
// side of pred_arena and writes its `rec` doubles per stream straight into it, behind them; _end waits and copies out.
static int readout_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, double *out, int rec) {
    if (!ctx || n <= 0 || !streams || !out) return MSKF_ERR_INVALID;
    for (int i = 0; i < n; ++i) if (!streams[i] || streams[i]->ctx_ekf != ctx) return MSKF_ERR_INVALID;
    int rc = mskf_refuse_if_owned(ctx, MSKF_ARENAS_PRED);
    if (rc != MSKF_OK) return rc;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t desc_bytes = align_up(sizeof(EkfStreamDev) * (size_t)n, 64);
    const size_t bytes = desc_bytes + sizeof(double) * (size_t)rec * (size_t)n;
    if ((rc = ctx->pred_arena.fence_wait()) != MSKF_OK || (rc = ctx->pred_arena.ensure(bytes)) != MSKF_OK) return rc;
    EkfStreamDev *D = (EkfStreamDev *)ctx->pred_arena.h;
    for (int i = 0; i < n; ++i) base_desc(streams[i], D[i]);
    // (no staging copies: the kernel reads its descriptors from the pinned arena and writes the rec * n doubles straight into it)
    DrainOnError drain{st, true};
    double *res = (double *)(ctx->pred_arena.h + desc_bytes);
    if (rec == 3) ekf_launch_posvar((const EkfStreamDev *)ctx->pred_arena.h, n, res, st);
    else ekf_launch_odom_cov((const EkfStreamDev *)ctx->pred_arena.h, n, res, st);
    mskf_ctx::PendingReadOut &V = ctx->pend_ro;
    V.n = n; V.rec = rec; V.out = out; V.desc_bytes = desc_bytes;
    if ((rc = mskf_batch_arm(ctx, V)) != MSKF_OK) return rc;
    drain.armed = false;
    return MSKF_OK;
}

static int readout_end(mskf_ctx *ctx, int rec) {
    if (!ctx) return MSKF_ERR_INVALID;
    mskf_ctx::PendingReadOut &V = ctx->pend_ro;
    if (!V.active) return MSKF_OK;
    if (V.rec != rec) return mskf_refuse_if_owned(ctx, MSKF_ARENAS_PRED);      // the other kind is pending: names it and its _end
    const int rc = mskf_batch_finish(ctx, V);
    if (rc != MSKF_OK) return rc;
    mskf_t_collect(ctx);
    std::memcpy(V.out, ctx->pred_arena.h + V.desc_bytes, sizeof(double) * (size_t)V.rec * (size_t)V.n);
    return MSKF_OK;
}

extern "C" int mskf_ekf_get_pos_var_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, double *out) {
    const int rc = mskf_ekf_get_pos_var_batch_begin(ctx, n, streams, out);
    return rc != MSKF_OK ? rc : mskf_ekf_get_pos_var_batch_end(ctx);
}

extern "C" int mskf_ekf_get_pos_var_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, double *out) {
    return readout_begin(ctx, n, streams, out, 3);
}

extern "C" int mskf_ekf_get_pos_var_batch_end(mskf_ctx *ctx) { return readout_end(ctx, 3); }

extern "C" int mskf_ekf_get_pos_var(mskf_stream *s, double out[3]) {
    if (!s || !out) return MSKF_ERR_INVALID;
    mskf_stream *ss[1] = {s};
    return mskf_ekf_get_pos_var_batch(s->ctx_ekf, 1, ss, out);
}

static_assert(sizeof(mskf_odom_cov) == 48 * sizeof(double), "k_ekf_odom_cov writes 48 doubles per stream");

extern "C" int mskf_ekf_get_odom_cov_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_odom_cov *out) {
    return readout_begin(ctx, n, streams, (double *)out, 48);
}

extern "C" int mskf_ekf_get_odom_cov_batch_end(mskf_ctx *ctx) { return readout_end(ctx, 48); }

extern "C" int mskf_ekf_get_odom_cov_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_odom_cov *out) {
    const int rc = mskf_ekf_get_odom_cov_batch_begin(ctx, n, streams, out);
    return rc != MSKF_OK ? rc : mskf_ekf_get_odom_cov_batch_end(ctx);
}

extern "C" int mskf_ekf_get_odom_cov(mskf_stream *s, mskf_odom_cov *out) {
    if (!s || !out) return MSKF_ERR_INVALID;
    mskf_stream *ss[1] = {s};
    return mskf_ekf_get_odom_cov_batch(s->ctx_ekf, 1, ss, out);
}

extern "C" int mskf_ekf_remove_clones_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, const int32_t *idx) {
    if (!ctx || n <= 0 || !streams || !idx) return MSKF_ERR_INVALID;
    int rc = mskf_refuse_if_owned(ctx, MSKF_ARENAS_PRED);
    if (rc != MSKF_OK) return rc;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t bytes = sizeof(EkfStreamDev) * (size_t)n;
    if ((rc = ctx->pred_arena.fence_wait()) != MSKF_OK || (rc = ctx->pred_arena.ensure(bytes)) != MSKF_OK) return rc;
    EkfStreamDev *D = (EkfStreamDev *)ctx->pred_arena.h;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        mskf_stream *s = streams[i];
        if (!s || s->ctx_ekf != ctx) return MSKF_ERR_INVALID;
        EkfStreamState &E = s->ekf_state;
        EkfExtra *X = extra_of(s);
        const int nc = (E.d - EKF_IMU_DIM) / 6;
        int a = idx[2 * i], b = idx[2 * i + 1];
        if (a < 0 && b >= 0) std::swap(a, b);
        if (b >= 0 && b < a) std::swap(a, b);
        if (a >= nc || b >= nc || (a >= 0 && a == b)) return MSKF_ERR_INVALID;
        base_desc(s, D[i]);
        D[i].remove_index = a; D[i].remove_index2 = b; D[i].P_dst = X->P_alt;
        any |= a >= 0;
    }
    if (!any) return MSKF_OK;
    DrainOnError drain{st, true};
    { const MskfCopy cp = {ctx->pred_arena.d, ctx->pred_arena.h, bytes}; if ((rc = mskf_copy_async(ctx, &cp, 1)) != MSKF_OK) return rc; }
    if ((rc = ctx->pred_arena.fence_record(st)) != MSKF_OK) return rc;
    {
        const int ts = mskf_t_begin(ctx, MSKF_K_EKF_REMOVE);
        ekf_launch_remove_clone((const EkfStreamDev *)ctx->pred_arena.d, n, st);
        mskf_t_end(ctx, ts, n);
    }
    MSKF_HIPCHK(hipGetLastError());
    drain.armed = false;
    for (int i = 0; i < n; ++i) {
        const EkfStreamDev &Di = D[i];
        if (Di.remove_index < 0) continue;
        EkfStreamState &E = streams[i]->ekf_state;
        std::swap(E.P, extra_of(streams[i])->P_alt);
        E.d -= Di.remove_index2 >= 0 ? 12 : 6;
    }
    return MSKF_OK;
}

extern "C" int mskf_ekf_remove_clone(mskf_stream *s, int clone_index) {
    if (!s) return MSKF_ERR_INVALID;
    const int nc = (s->ekf_state.d - EKF_IMU_DIM) / 6;
    if (clone_index < 0 || clone_index >= nc) return MSKF_ERR_INVALID;
    mskf_stream *ss[1] = {s};
    const int32_t idx[2] = {clone_index, -1};
    return mskf_ekf_remove_clones_batch(s->ctx_ekf, 1, ss, idx);
}

extern "C" int mskf_ekf_update_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_ekf_update_args *args) {
    const int rc = mskf_ekf_update_batch_begin(ctx, n, streams, args);
    return rc != MSKF_OK ? rc : mskf_ekf_update_batch_end(ctx);
}

// ---------------------------------------------------------------------------------------------- measurement update
// mskf_ekf_update_batch_begin in four steps: plan_update looks at the whole batch and decides everything, touching nothing;
// grow_stacks, pack_update and enqueue_update then carry the plan out.
// What the batch as a whole needs (the per-stream part is EkfUpdatePlan, mskf_internal.h)
struct UpdateBatchPlan {
    bool any_pairs, any_small, any_general;
    bool any_householder, any_gram;      // among the general-route streams: compressed by k_ekf_tsqr / by the Gram factorisation
    bool any_pv_nofeat;                  // a stream without features wants its position variances
    int max_feat, max_d, min_d, max_clones_cfg;   // min_d: over the streams with features (those the dense kernels work on)
    int max_frows, max_frows_small;      // block rows (4 n_obs) of the largest feature / of the largest one in the small class's list
    int max_feat_pairs, max_tri;         // over the pair-route streams
    int n_work[3];                       // entries of the three work lists of the feature kernel
    size_t work_off, in_bytes, out_bytes;
    double fl_feat, fl_qr, fl_upd;       // algorithmic FP64 flops of this launch
};
// flops of a stream's Kalman update per d^3: downdate 4, a factorisation 1/3, T, S and the solve 2 each
constexpr double kUpdFlopsPerD3 = 4.0 + 1.0 / 3.0 + 2.0 + 2.0 + 2.0;

// Which kernels handle a stream is decided per STREAM, from that stream's features alone (EkfStreamDev::route): the same
// stream takes the same route, and therefore runs the same arithmetic, whatever else is in the batch.
//   pairs : every feature has exactly two Jacobian observations, all of the same ordered clone pair (the pruning update)
//   wave  : every feature has <= FEAT_WAVE_CLONES Jacobian observations and a triangulation over <= TRI_SMALL_CLONES clones:
//           list [0] of the feature kernel, one wavefront per feature; otherwise a feature is in list [1]
//           (<= FEAT_SMALL_CLONES observations and triangulation clones) or [2]
//   small : the stream touches at most SU_MAX_NA / 6 clones: whole update in k_ekf_small_update
static int plan_stream(const mskf_ctx *ctx, const mskf_stream *s, const mskf_ekf_update_args &a, EkfUpdatePlan &L, UpdateBatchPlan &B) {
    if (!s || s->ctx_ekf != ctx) return MSKF_ERR_INVALID;
    const EkfStreamState &E = s->ekf_state;
    if (a.n_clones * 6 + EKF_IMU_DIM != E.d) { mskf_set_error("n_clones does not match the covariance dimension"); return MSKF_ERR_INVALID; }
    if (a.n_feat < 0 || a.n_obs < 0) return MSKF_ERR_INVALID;
    if (a.n_feat && (!a.clones || !a.features || !a.obs_clone || !a.obs_z || !a.delta_x || !a.feat_status || !a.rows_out)) return MSKF_ERR_INVALID;
    L = EkfUpdatePlan{};
    unsigned long long clone_mask = 0ULL;          // clones any Jacobian block of this stream touches: bounds the active columns
    bool pairs = a.n_feat > 0, wave = a.n_feat > 0;
    int pair_a = -1, pair_b = -1, frows_cls[3] = {0, 0, 0};
    for (int j = 0; j < a.n_feat; ++j) {
        const mskf_ekf_feature &f = a.features[j];
        L.n_tri += f.needs_init ? 1 : 0;
        if (f.n_obs < 2 || f.n_obs > E.max_clones || f.obs_start < 0 || f.obs_start + f.n_obs > a.n_obs) return MSKF_ERR_INVALID;
        if (f.needs_init && (f.n_init < 1 || f.n_init > E.max_clones || f.init_start < 0 || f.init_start + f.n_init > a.n_obs)) return MSKF_ERR_INVALID;
        if (f.n_obs != 2) pairs = false;
        else if (pairs) {
            // the pair kernel keeps the two clones' blocks in the order (lower, higher) and shares their covariance
            // block among the features: both observations distinct, ascending, and the same pair for every feature
            const int c0 = a.obs_clone[f.obs_start], c1 = a.obs_clone[f.obs_start + 1];
            if (j == 0) { pair_a = c0; pair_b = c1; }
            if (!(c0 < c1) || c0 != pair_a || c1 != pair_b) pairs = false;
        }
        if (f.n_obs > FEAT_WAVE_CLONES || (f.needs_init && f.n_init > TRI_SMALL_CLONES)) wave = false;
        L.m_total += 4 * f.n_obs - 3;
        B.max_frows = std::max(B.max_frows, 4 * f.n_obs);
        const int cls = std::max(f.n_obs, f.needs_init ? f.n_init : 0) <= FEAT_SMALL_CLONES ? 1 : 2;
        frows_cls[cls] = std::max(frows_cls[cls], 4 * f.n_obs);
        ++L.cnt[cls];
        for (int o = 0; o < f.n_obs; ++o) {
            const int c = a.obs_clone[f.obs_start + o];
            if (c < 0 || c >= a.n_clones) return MSKF_ERR_INVALID;
            clone_mask |= 1ULL << c;
        }
        const double nj = 4.0 * f.n_obs - 3.0, M = f.n_obs, dd = E.d;
        B.fl_feat += 2.0 * nj * (4.0 * M) * (6.0 * M) + 2.0 * nj * dd * dd + 2.0 * nj * nj * dd;
    }
    if (L.m_total > kMaxRows) { mskf_set_error("stacked Jacobian exceeds the row capacity"); return MSKF_ERR_CAPACITY; }
    L.clones = B.in_bytes;
    L.feats = align_up(L.clones + sizeof(mskf_clone_state) * (size_t)a.n_clones, 16);
    L.obs_clone = align_up(L.feats + sizeof(EkfFeatDev) * (size_t)a.n_feat, 16);
    L.obs_z = align_up(L.obs_clone + sizeof(int) * (size_t)a.n_obs, 16);
    L.tri = align_up(L.obs_z + sizeof(double) * 4 * (size_t)a.n_obs, 16);
    B.in_bytes = align_up(L.tri + sizeof(int) * (size_t)L.n_tri, 64);
    L.o_dx = B.out_bytes;
    L.o_gamma = align_up(L.o_dx + sizeof(double) * (size_t)E.ld, 16);
    L.o_pos = align_up(L.o_gamma + sizeof(double) * (size_t)a.n_feat, 16);
    L.o_rows = align_up(L.o_pos + sizeof(double) * 3 * (size_t)a.n_feat, 16);
    static_assert(EKF_ROWS_COUNT * sizeof(int) <= 32, "rows_out fits its 32 bytes");
    L.o_status = L.o_rows + 32 + 32;           // rows_out (EKF_ROWS_COUNT ints, padded to 32 bytes) + 3 position variances
    B.out_bytes = align_up(L.o_status + (size_t)a.n_feat, 64);
    B.any_pv_nofeat |= a.pos_var_out != nullptr && a.n_feat == 0;
    // (the first block is sized for what a stream of this configuration can stack, mskf_ekf_stream_init: growth is rare)
    if (L.m_total > E.max_rows) L.grow_rows = std::min(kMaxRows, std::max(2048, L.m_total + L.m_total / 2));
    if (a.n_feat > 0) {
        const double dd = E.d, mm = L.m_total;
        if (L.m_total > E.d) B.fl_qr += 2.0 * mm * dd * dd - (2.0 / 3.0) * dd * dd * dd;
        B.fl_upd += kUpdFlopsPerD3 * dd * dd * dd;
        if (pairs) wave = false;
        L.na_max = 6 * __builtin_popcountll(clone_mask);
        const bool small = L.na_max <= SU_MAX_NA;
        L.route = (pairs ? EKF_ROUTE_PAIRS : 0) | (wave ? EKF_ROUTE_WAVE : 0) | (small ? EKF_ROUTE_SMALL : 0);
        B.any_pairs |= pairs; B.any_small |= small; B.any_general |= !small;
        if (!small) { const bool hh = ekf_mode_householder(s->ekf.compression_mode); B.any_householder |= hh; B.any_gram |= !hh; }
        if (pairs) { B.max_feat_pairs = std::max(B.max_feat_pairs, a.n_feat); B.max_tri = std::max(B.max_tri, L.n_tri); }
        if (pairs || wave) {
            // the whole stream is list [0] (wave) or handled by the pair kernels: none of its features in [1] / [2]
            L.cnt[0] = pairs ? 0 : L.cnt[1] + L.cnt[2];
            L.cnt[1] = L.cnt[2] = 0;
        } else B.max_frows_small = std::max(B.max_frows_small, frows_cls[1]);
    }
    B.max_clones_cfg = std::max(B.max_clones_cfg, E.max_clones);
    B.max_feat = std::max(B.max_feat, a.n_feat);
    B.max_d = std::max(B.max_d, E.d);
    if (a.n_feat > 0) B.min_d = B.min_d ? std::min(B.min_d, E.d) : E.d;
    return MSKF_OK;
}

// Validates every stream and feature of the batch and fills plan[0..n) and B.  No HIP call, and nothing but the plan is
// written: a batch that is refused for its last stream has not touched the first.
static int plan_update(const mskf_ctx *ctx, int n, mskf_stream *const *streams, const mskf_ekf_update_args *args, EkfUpdatePlan *plan, UpdateBatchPlan &B) {
    B = UpdateBatchPlan{};
    for (int i = 0; i < n; ++i) {
        const int rc = plan_stream(ctx, streams[i], args[i], plan[i], B);
        if (rc != MSKF_OK) return rc;
    }
    // work lists: stream << 16 | slot << 8 | n_slots per feature group in flight
    if (n > 0xffff) { mskf_set_error("too many streams in one update batch"); return MSKF_ERR_CAPACITY; }
    for (int c = 0; c < 3; ++c) for (int i = 0; i < n; ++i) B.n_work[c] += std::min(plan[i].cnt[c], EKF_SLOTS);
    B.work_off = B.in_bytes;
    B.in_bytes = align_up(B.in_bytes + sizeof(int) * (size_t)(B.n_work[0] + B.n_work[1] + B.n_work[2]), 64);
    return MSKF_OK;
}

// Growth of the stacked-Jacobian buffer of the streams the plan marked, STREAM-ORDERED: hipFree / hipMalloc synchronise the
// whole device, and a group that grows a buffer in the middle of a run then waits until every other group's queue is idle
// (measured in the round-3 bench: the two groups that met their largest pruning update inside the timed window stood still
// for 0.3 s each).
// The new block is allocated FIRST: if that fails the call fails with the stream's buffers as they were (a later, smaller
// update still finds a valid Hs of max_rows rows).  The old block goes back to the pool it came from: a stream-ordered free
// for a stream-ordered block, retirement until the stream is destroyed for the first one (hipMalloc'ed at stream creation;
// hipFreeAsync does not take such a pointer without a device-wide wait).
static int grow_stacks(int n, mskf_stream *const *streams, const EkfUpdatePlan *plan, hipStream_t st) {
    for (int i = 0; i < n; ++i) {
        EkfStreamState &E = streams[i]->ekf_state;
        const int cap = plan[i].grow_rows;
        if (cap <= E.max_rows) continue;
        const size_t bytes = ((size_t)cap * E.ld + (size_t)cap) * sizeof(double);
        double *grown = nullptr;
        MSKF_HIPCHK(hipMallocAsync((void **)&grown, bytes, st));
        if (hipMemsetAsync(grown, 0, bytes, st) != hipSuccess) { (void)hipFreeAsync(grown, st); mskf_set_error("hipMemsetAsync of the grown stacked-Jacobian buffer failed"); return MSKF_ERR_HIP; }
        if (E.Hs) { if (E.hs_async) (void)hipFreeAsync(E.Hs, st); else extra_of(streams[i])->retired_hs.push_back(E.Hs); }      // (rs lives behind Hs in the same allocation)
        E.Hs = grown;
        E.rs = E.Hs + (size_t)cap * E.ld;
        E.max_rows = cap;
        E.hs_async = true;
    }
    return MSKF_OK;
}

// The batch's inputs into upd_in (per stream: clone states, features, observations, triangulation list; then the three
// work lists) and its descriptors into ekf_desc, host side.
static void pack_update(mskf_ctx *ctx, int n, mskf_stream *const *streams, const mskf_ekf_update_args *args, const EkfUpdatePlan *plan, const UpdateBatchPlan &B) {
    char *hin = ctx->upd_in.h, *din = ctx->upd_in.d, *dout = ctx->upd_out.d;
    int *w = (int *)(hin + B.work_off);
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < n; ++i) {
            const int ns = std::min(plan[i].cnt[c], EKF_SLOTS);
            for (int k = 0; k < ns; ++k) *w++ = (i << 16) | (k << 8) | ns;
        }
    for (int i = 0; i < n; ++i) {
        const mskf_ekf_update_args &a = args[i];
        const EkfUpdatePlan &L = plan[i];
        if (a.n_clones) std::memcpy(hin + L.clones, a.clones, sizeof(mskf_clone_state) * (size_t)a.n_clones);
        EkfFeatDev *fd = (EkfFeatDev *)(hin + L.feats);
        int *tri = (int *)(hin + L.tri);
        int n_tri_w = 0, row = 0;
        for (int j = 0; j < a.n_feat; ++j) {
            const mskf_ekf_feature &f = a.features[j];
            fd[j].obs_start = f.obs_start; fd[j].n_obs = f.n_obs;
            fd[j].needs_init = f.needs_init; fd[j].init_start = f.init_start; fd[j].n_init = f.n_init;
            fd[j].row_off = row;
            fd[j].position[0] = f.position[0]; fd[j].position[1] = f.position[1]; fd[j].position[2] = f.position[2];
            fd[j].colmask = 0ULL;
            row += 4 * f.n_obs - 3;
            if (f.needs_init) tri[n_tri_w++] = j;
        }
        if (a.n_obs) {
            std::memcpy(hin + L.obs_clone, a.obs_clone, sizeof(int) * (size_t)a.n_obs);
            std::memcpy(hin + L.obs_z, a.obs_z, sizeof(double) * 4 * (size_t)a.n_obs);
        }
        EkfStreamDev &D = ctx->ekf_desc.h[i];
        base_desc(streams[i], D);
        D.n_clones = a.n_clones; D.n_feat = a.n_feat; D.n_obs = a.n_obs;
        D.route = L.route; D.na_max = L.na_max;
        D.dof_offset = a.dof_offset; D.apply_row_cap = a.apply_row_cap;
        D.m_total = L.m_total;
        for (int k = 0; k < 3; ++k) D.gravity[k] = a.gravity[k];
        D.clones = (const mskf_clone_state *)(din + L.clones);
        D.feats = (EkfFeatDev *)(din + L.feats);
        D.obs_clone = (const int *)(din + L.obs_clone);
        D.obs_z = (const double *)(din + L.obs_z);
        D.tri_idx = (const int *)(din + L.tri);
        D.n_tri = L.n_tri;
        D.delta_x = (double *)(dout + L.o_dx);
        D.gamma = (double *)(dout + L.o_gamma);
        D.pos_out = (double *)(dout + L.o_pos);
        D.rows_out = (int *)(dout + L.o_rows);
        D.pos_var_out = a.pos_var_out ? (double *)(dout + L.o_rows + 32) : nullptr;
        D.feat_status = (uint8_t *)(dout + L.o_status);
    }
}

// One timed launch (mskf_t_begin / mskf_t_end around it)
#define EKF_TIMED(kind, units, launch) do { const int ts_ = mskf_t_begin(ctx, kind); launch; mskf_t_end(ctx, ts_, (long long)(units)); } while (0)

// Staging copy in, the launch chain, result copy out.  A launch set is enqueued when some stream of the batch needs it; the
// streams of the other routes leave those kernels at once.
static int enqueue_update(mskf_ctx *ctx, int n, const UpdateBatchPlan &B) {
    hipStream_t st = ctx->stream;
    const EkfStreamDev *D = ctx->ekf_desc.d;
    const MskfCopy in[2] = {{ctx->upd_in.d, ctx->upd_in.h, B.in_bytes}, {ctx->ekf_desc.d, ctx->ekf_desc.h, sizeof(EkfStreamDev) * (size_t)n}};
    const int rc = mskf_copy_async(ctx, in, 2);
    if (rc != MSKF_OK) return rc;
    const int ts = mskf_t_begin(ctx, MSKF_K_EKF_FEATURES);
    if (B.any_pairs) ekf_launch_pair_features(D, n, B.max_feat_pairs, B.max_tri, st);      // the pruning update
    if (B.n_work[0] + B.n_work[1] + B.n_work[2] > 0) {
        const int *w0 = (const int *)(ctx->upd_in.d + B.work_off);
        ekf_launch_features(D, w0, B.n_work[0], w0 + B.n_work[0], B.n_work[1], w0 + B.n_work[0] + B.n_work[1], B.n_work[2], B.max_frows,
                            B.max_frows_small, B.max_clones_cfg, st);
    }
    mskf_t_end(ctx, ts, (long long)B.fl_feat);
    // (which blocks are stacked - the 1500-row cap of :1002-1010 - is worked out by the first dense kernel of each route
    //  itself: ekf_cap.h; rounds 1-3 ran it as a launch of its own here)
    const double d3 = B.fl_upd / kUpdFlopsPerD3;     // sum of d^3 over the launch
    const int max_d = B.max_d, min_d = B.min_d ? B.min_d : B.max_d;
    // streams that stack blocks of at most four clones (the pruning update: the two clones being removed):
    // compression, gain and Y in one launch (k_ekf_small_update); the other streams leave it at once
    if (B.any_small) EKF_TIMED(MSKF_K_EKF_SMALL, B.any_general ? 0 : B.fl_qr + B.fl_upd, ekf_launch_small_update(D, n, max_d, st));
    if (B.any_general) {
        // QR compression as Gram + semidefinite Cholesky (Householder TSQR inside the factorisation kernel for the
        // streams that need it), then the Kalman update (ekf_linalg.hip); small-route streams leave these at once
        // (GRAM is also the first dense kernel of the general route: its tiles work out the stacking decision for every stream)
        if (B.any_gram) EKF_TIMED(MSKF_K_EKF_GEMM, B.fl_qr, ekf_launch_gemm(D, n, GM_GRAM, max_d + 1, st));
        // Householder TSQR of the streams in compression_mode 2 / 3 (a kernel without LDS of its own: ekf_linalg.hip); with no
        // Gram launch before it, it is the first dense kernel and makes the stacking decision itself
        if (B.any_householder) EKF_TIMED(MSKF_K_EKF_TSQR, B.fl_qr, ekf_launch_tsqr(D, n, min_d, max_d, B.any_gram ? 0 : 1, st));
        if (B.any_gram) EKF_TIMED(MSKF_K_EKF_CHOL, d3 / 3.0, ekf_launch_chol(D, n, 0, min_d, max_d, st));
        EKF_TIMED(MSKF_K_EKF_GEMM, 2.0 * d3, ekf_launch_gemm(D, n, GM_T, max_d, st));
        EKF_TIMED(MSKF_K_EKF_GEMM, 2.0 * d3, ekf_launch_gemm(D, n, GM_S2, max_d, st));
        EKF_TIMED(MSKF_K_EKF_CHOL, d3 / 3.0, ekf_launch_chol(D, n, 1, min_d, max_d, st));
        EKF_TIMED(MSKF_K_EKF_TRSM, 2.0 * d3, ekf_launch_trsm(D, n, max_d, st));
    }
    // P <- P - Y^T Y and delta_x = Y^T w for every stream, whichever route produced Y
    EKF_TIMED(MSKF_K_EKF_GEMM, B.any_general ? 4.0 * d3 : 0, ekf_launch_gemm(D, n, GM_PUPD, max_d, st));
    if (B.any_pv_nofeat) ekf_launch_posvar_upd(D, n, st);       // (streams with features get theirs from the downdate's epilogue)
    MSKF_HIPCHK(hipGetLastError());
    const MskfCopy out = {ctx->upd_out.h, ctx->upd_out.d, B.out_bytes};
    return mskf_copy_async(ctx, &out, 1);
}
#undef EKF_TIMED

extern "C" int mskf_ekf_update_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_ekf_update_args *args) {
    if (!ctx || n <= 0 || !streams || !args) return MSKF_ERR_INVALID;
    int rc = mskf_refuse_if_owned(ctx, MSKF_ARENAS_UPDATE);
    if (rc != MSKF_OK) return rc;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    const auto t_h0 = std::chrono::steady_clock::now();
    mskf_ctx::PendingUpdate &U = ctx->pend_upd;
    U.plan.resize((size_t)n);
    UpdateBatchPlan B;
    if ((rc = plan_update(ctx, n, streams, args, U.plan.data(), B)) != MSKF_OK) return rc;
    if ((rc = ctx->ekf_desc.ensure(n)) != MSKF_OK || (rc = ctx->upd_in.ensure(B.in_bytes)) != MSKF_OK || (rc = ctx->upd_out.ensure(B.out_bytes)) != MSKF_OK) return rc;
    // the batch is accepted: from here on work is enqueued, and a failure drains the stream before it is reported
    DrainOnError drain{ctx->stream, true};
    if ((rc = grow_stacks(n, streams, U.plan.data(), ctx->stream)) != MSKF_OK) return rc;
    pack_update(ctx, n, streams, args, U.plan.data(), B);
    U.launched = B.max_feat > 0; U.n = n; U.streams = streams; U.args = args; U.direct = false;
    if (!U.launched) U.active = true;            // nothing launched, no mark: _end only fills the outputs
    else if ((rc = enqueue_update(ctx, n, B)) != MSKF_OK || (rc = mskf_batch_arm(ctx, U)) != MSKF_OK) return rc;
    drain.armed = false;
    if (ctx->t_gate) ctx->host_s[0] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_h0).count();
    return MSKF_OK;
}

// Wait for the batch started by mskf_ekf_update_batch_begin and copy delta_x, gate results, positions and the stacked
// row counts into the args given there.  No-op when nothing is pending.
extern "C" int mskf_ekf_update_batch_end(mskf_ctx *ctx) {
    if (!ctx) return MSKF_ERR_INVALID;
    mskf_ctx::PendingUpdate &U = ctx->pend_upd;
    if (!U.active) return MSKF_OK;
    if (U.direct) return mskf_refuse_if_owned(ctx, MSKF_ARENAS_UPDATE);        // the other kind is pending: names it and its _end
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    if (!U.launched) U.active = false;
    else {
        const int rc = mskf_batch_finish(ctx, U);
        if (rc != MSKF_OK) return rc;
        mskf_t_collect(ctx);
    }
    const auto t_h1 = std::chrono::steady_clock::now();
    const int n = U.n;
    mskf_stream *const *streams = U.streams;
    mskf_ekf_update_args *args = U.args;
    const char *hout = ctx->upd_out.h;
    for (int i = 0; i < n; ++i) {
        mskf_ekf_update_args &a = args[i];
        EkfStreamState &E = streams[i]->ekf_state;
        const EkfUpdatePlan &L = U.plan[i];
        const int d = E.d;
        if (a.pos_var_out) {
            if (U.launched) std::memcpy(a.pos_var_out, hout + L.o_rows + 32, sizeof(double) * 3);
            else a.pos_var_out[0] = a.pos_var_out[1] = a.pos_var_out[2] = -1.0;       // nothing ran: no value (variances are never negative)
        }
        if (!a.n_feat) {
            if (a.delta_x) std::memset(a.delta_x, 0, sizeof(double) * (size_t)d);
            if (a.rows_out) *a.rows_out = 0;
            if (a.diag_out) { a.diag_out[0] = 0; a.diag_out[1] = -1; }
            continue;
        }
        std::memcpy(a.delta_x, hout + L.o_dx, sizeof(double) * (size_t)d);
        if (a.gamma) std::memcpy(a.gamma, hout + L.o_gamma, sizeof(double) * (size_t)a.n_feat);
        *a.rows_out = ((const int *)(hout + L.o_rows))[EKF_ROWS_STACKED];
        if (a.diag_out) ekf_diag_decode(((const int *)(hout + L.o_rows))[EKF_ROWS_DIAG], &a.diag_out[0], &a.diag_out[1]);
        std::memcpy(a.feat_status, hout + L.o_status, (size_t)a.n_feat);
        const double *po = (const double *)(hout + L.o_pos);
        for (int j = 0; j < a.n_feat; ++j)
            for (int k = 0; k < 3; ++k) a.features[j].position[k] = po[3 * j + k];
    }
    if (ctx->t_gate) ctx->host_s[1] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_h1).count();
    return MSKF_OK;
}

// ------------------------------------------------------------------------------------------ direct measurement update
// mskf_ekf_update_direct_batch_begin: plan (validate everything, lay out the arenas; no HIP call), grow, stage, enqueue:
// one copy in (descriptors + H, r, R of every stream, all in upd_in), k_ekf_direct_update, one copy out.
static bool finite_all(const double *v, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

static int plan_direct(const mskf_ctx *ctx, int n, mskf_stream *const *streams, const mskf_ekf_direct_args *args, std::vector<size_t> &in_off,
                       std::vector<size_t> &out_off, size_t &in_bytes, size_t &out_bytes, int &n_rows) {
    in_bytes = align_up(sizeof(EkfDirectDev) * (size_t)n, 64);
    out_bytes = 0; n_rows = 0;
    for (int i = 0; i < n; ++i) {
        const mskf_stream *s = streams[i];
        const mskf_ekf_direct_args &a = args[i];
        if (!s || s->ctx_ekf != ctx) return MSKF_ERR_INVALID;
        const int m = a.m;
        if (m < 0 || m > MSKF_DIRECT_MAX_ROWS) { mskf_set_error("mskf_ekf_direct_args.m must be in [0, " + std::to_string(MSKF_DIRECT_MAX_ROWS) + "]"); return MSKF_ERR_INVALID; }
        // (the update is in place: two entries with rows for one stream would be two workgroups writing one P)
        if (m > 0) for (int k = 0; k < i; ++k) if (streams[k] == s && args[k].m > 0) { mskf_set_error("a stream appears twice with rows in one direct update batch"); return MSKF_ERR_INVALID; }
        if (m > 0) {
            if (!a.H || !a.r || !a.R || !a.delta_x) { mskf_set_error("a direct update with rows needs H, r, R and delta_x"); return MSKF_ERR_INVALID; }
            if (!finite_all(a.H, m * EKF_IMU_DIM) || !finite_all(a.r, m) || !finite_all(a.R, m * m) || std::isnan(a.gate)) {
                mskf_set_error("a direct update takes finite H, r and R (and a gate that is a number)");
                return MSKF_ERR_INVALID;
            }
            for (int p = 0; p < m; ++p) {
                if (!(a.R[p * m + p] > 0.0)) { mskf_set_error("R of a direct update needs a positive diagonal"); return MSKF_ERR_INVALID; }
                for (int q = 0; q < p; ++q)
                    if (a.R[p * m + q] != a.R[q * m + p]) { mskf_set_error("R of a direct update must be symmetric"); return MSKF_ERR_INVALID; }
            }
        }
        in_off[i] = in_bytes;
        in_bytes = align_up(in_bytes + sizeof(double) * (size_t)(m * EKF_IMU_DIM + m + m * m), 64);
        out_off[i] = out_bytes;           // delta_x (ld), gamma, 3 position variances, status
        out_bytes = align_up(out_bytes + sizeof(double) * (size_t)(s->ekf_state.ld + 4) + sizeof(int), 64);
        n_rows += m > 0;
    }
    return MSKF_OK;
}

extern "C" int mskf_ekf_update_direct_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_ekf_direct_args *args) {
    if (!ctx || n <= 0 || !streams || !args) return MSKF_ERR_INVALID;
    int rc = mskf_refuse_if_owned(ctx, MSKF_ARENAS_UPDATE);
    if (rc != MSKF_OK || (rc = mskf_refuse_if_owned(ctx, MSKF_ARENAS_PRED)) != MSKF_OK) return rc;
    mskf_ctx::PendingUpdate &U = ctx->pend_upd;
    std::vector<size_t> in_off((size_t)n), out_off((size_t)n);
    size_t in_bytes, out_bytes;
    int n_rows;
    if ((rc = plan_direct(ctx, n, streams, args, in_off, out_off, in_bytes, out_bytes, n_rows)) != MSKF_OK) return rc;
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    if ((rc = ctx->upd_in.ensure(in_bytes)) != MSKF_OK || (rc = ctx->upd_out.ensure(out_bytes)) != MSKF_OK) return rc;
    // the batch is accepted
    char *hin = ctx->upd_in.h, *din = ctx->upd_in.d, *dout = ctx->upd_out.d;
    EkfDirectDev *D = (EkfDirectDev *)hin;
    for (int i = 0; i < n; ++i) {
        const mskf_ekf_direct_args &a = args[i];
        const EkfStreamState &E = streams[i]->ekf_state;
        const int m = a.m;
        double *in = (double *)(hin + in_off[i]);
        const double *din_i = (const double *)(din + in_off[i]);
        double *o = (double *)(dout + out_off[i]);
        if (m > 0) {
            std::memcpy(in, a.H, sizeof(double) * (size_t)(m * EKF_IMU_DIM));
            std::memcpy(in + m * EKF_IMU_DIM, a.r, sizeof(double) * (size_t)m);
            std::memcpy(in + m * EKF_IMU_DIM + m, a.R, sizeof(double) * (size_t)(m * m));
        }
        EkfDirectDev &d = D[i];
        d.P = E.P; d.d = E.d; d.ld = E.ld; d.m = m;
        d.H = din_i; d.r = din_i + m * EKF_IMU_DIM; d.R = din_i + m * EKF_IMU_DIM + m;
        d.gate = a.gate;
        d.delta_x = o; d.gamma = o + E.ld; d.pos_var_out = a.pos_var_out ? o + E.ld + 1 : nullptr;
        d.status = (int *)(o + E.ld + 4);
    }
    // the slot's fields describe a direct batch only once it is pending: `direct` is set together with `active`
    U.launched = n_rows > 0; U.n = n; U.streams = streams; U.args = nullptr; U.dargs = args;
    U.d_out.swap(out_off);
    if (!U.launched) { U.direct = true; U.active = true; return MSKF_OK; }      // nothing launched, no mark: _end only fills the outputs
    DrainOnError drain{ctx->stream, true};
    { const MskfCopy cp = {din, hin, in_bytes}; if ((rc = mskf_copy_async(ctx, &cp, 1)) != MSKF_OK) return rc; }
    {
        const int ts = mskf_t_begin(ctx, MSKF_K_EKF_AUGMENT);     // (the slot the direct update is accounted in: mskf_hip.h)
        ekf_launch_direct_update((const EkfDirectDev *)din, n, ctx->stream);
        mskf_t_end(ctx, ts, n_rows);
    }
    MSKF_HIPCHK(hipGetLastError());
    { const MskfCopy cp = {ctx->upd_out.h, dout, out_bytes}; if ((rc = mskf_copy_async(ctx, &cp, 1)) != MSKF_OK) return rc; }
    if ((rc = mskf_batch_arm(ctx, U)) != MSKF_OK) return rc;
    U.direct = true;
    drain.armed = false;
    return MSKF_OK;
}

extern "C" int mskf_ekf_update_direct_batch_end(mskf_ctx *ctx) {
    if (!ctx) return MSKF_ERR_INVALID;
    mskf_ctx::PendingUpdate &U = ctx->pend_upd;
    if (!U.active) return MSKF_OK;
    if (!U.direct) return mskf_refuse_if_owned(ctx, MSKF_ARENAS_UPDATE);       // the other kind is pending: names it and its _end
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    if (!U.launched) U.active = false;
    else {
        const int rc = mskf_batch_finish(ctx, U);
        if (rc != MSKF_OK) return rc;
        mskf_t_collect(ctx);
    }
    const char *hout = ctx->upd_out.h;
    for (int i = 0; i < U.n; ++i) {
        mskf_ekf_direct_args &a = U.dargs[i];
        const EkfStreamState &E = U.streams[i]->ekf_state;
        if (a.m <= 0) {
            a.status = 0; a.gamma = 0.0;
            if (a.delta_x) std::memset(a.delta_x, 0, sizeof(double) * (size_t)E.d);
            if (a.pos_var_out) a.pos_var_out[0] = a.pos_var_out[1] = a.pos_var_out[2] = -1.0;      // nothing ran for it: no value
            continue;
        }
        const double *o = (const double *)(hout + U.d_out[i]);
        std::memcpy(a.delta_x, o, sizeof(double) * (size_t)E.d);
        a.gamma = o[E.ld];
        if (a.pos_var_out) std::memcpy(a.pos_var_out, o + E.ld + 1, sizeof(double) * 3);
        a.status = *(const int *)(o + E.ld + 4);
    }
    U.direct = false;
    return MSKF_OK;
}

extern "C" int mskf_ekf_update_direct_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_ekf_direct_args *args) {
    const int rc = mskf_ekf_update_direct_batch_begin(ctx, n, streams, args);
    return rc != MSKF_OK ? rc : mskf_ekf_update_direct_batch_end(ctx);
}

extern "C" int mskf_ekf_update_direct(mskf_stream *s, mskf_ekf_direct_args *args) {
    if (!s || !args) return MSKF_ERR_INVALID;
    mskf_stream *ss[1] = {s};
    return mskf_ekf_update_direct_batch(s->ctx_ekf, 1, ss, args);
}

// Test / diagnostic access to the work buffers of the last update of a stream (not used by the product path):
// which = 0 Hs (max_rows x ld), 1 rowmask (max_rows, 8-byte), 2 S (ld x ld), 3 T (ld x ld), 4 W (ld x ld), 5 act (ld ints),
// 6 the current covariance plane P, all ld x ld doubles (only [0,d) x [0,d) is live; the rest is what earlier calls left).
// Copies min(capacity, size) bytes; *ld_out = row stride in doubles.
extern "C" int mskf_ekf_debug_read(mskf_stream *s, int which, void *out, size_t capacity, int *ld_out) {
    if (!s || !out) return MSKF_ERR_INVALID;
    EkfStreamState &E = s->ekf_state;
    MSKF_HIPCHK(hipSetDevice(s->ctx_ekf->device));
    MSKF_HIPCHK(hipStreamSynchronize(s->ctx_ekf->stream));
    const void *src = nullptr;
    size_t bytes = 0;
    const size_t pl = sizeof(double) * (size_t)E.ld * E.ld;
    switch (which) {
        case 0: src = E.Hs; bytes = sizeof(double) * (size_t)E.max_rows * E.ld; break;
        case 1: src = E.rs; bytes = sizeof(double) * (size_t)E.max_rows; break;
        case 2: src = E.S; bytes = pl; break;
        case 3: src = E.T; bytes = pl; break;
        case 4: src = E.W; bytes = pl; break;
        case 5: src = E.act; bytes = sizeof(int) * (size_t)E.ld; break;
        case 6: src = E.P; bytes = pl; break;
        default: return MSKF_ERR_INVALID;
    }
    if (!src) return MSKF_ERR_INVALID;
    if (ld_out) *ld_out = E.ld;
    MSKF_HIPCHK(hipMemcpy(out, src, std::min(bytes, capacity), hipMemcpyDeviceToHost));
    return MSKF_OK;
}

extern "C" int mskf_ekf_update(mskf_stream *s, mskf_ekf_update_args *args) {
    if (!s || !args) return MSKF_ERR_INVALID;
    mskf_stream *ss[1] = {s};
    return mskf_ekf_update_batch(s->ctx_ekf, 1, ss, args);
}
