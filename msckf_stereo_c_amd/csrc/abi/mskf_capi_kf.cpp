// mskf_capi_kf.cpp — C-ABI: the keyframe calls of the front end: descriptors, matching, geometric verification (include/mskf_hip.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>
#include "mskf_internal.h"

// ------------------------------------------------------------------------------------------ descriptors (fe_brief.h)
extern "C" void mskf_fe_descriptor_pattern(int8_t out[4 * FB_TESTS]) {
    static constexpr FbPattern pat = fb_make_pattern();
    if (out) std::memcpy(out, pat.t, sizeof(pat.t));
}

// every refusal of these calls: MSKF_ERR_INVALID, the message begins with the kind ("describe: ", "match: ", "verify: ")
static int refuse(const char *kind, const char *why) { mskf_set_error(std::string(kind) + why); return MSKF_ERR_INVALID; }

// One stream's block of a describe batch: np points in `in`, FB_BYTES * np descriptor bytes and np validity bytes in `out`.
static inline size_t describe_in_bytes(size_t np) { return round_up(sizeof(mskf_point2f) * np, 64); }
static inline size_t describe_out_bytes(size_t np) { return round_up((FB_BYTES + 1) * np, 64); }

extern "C" int mskf_fe_describe_batch_begin(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_fe_describe_args *args) {
    // ---- plan: every refusal comes from here, before anything is touched
    if (!ctx || !streams || !args) return refuse("describe: ", "null argument");
    if (n <= 0) return refuse("describe: ", "a batch has at least one stream");
    if (const int rc = mskf_refuse_if_owned(ctx, MSKF_ARENAS_FE)) return rc;
    if (ctx->pend_dsc.active) return refuse("describe: ", "a describe batch of this context is still pending (call mskf_fe_describe_batch_end)");
    size_t in_bytes = 0, out_bytes = 0;
    int max_pts = 0;
    for (int i = 0; i < n; ++i) {
        const mskf_stream *s = streams[i];
        const mskf_fe_describe_args &a = args[i];
        if (!s) return refuse("describe: ", "null stream");
        if (s->ctx != ctx) return refuse("describe: ", "a stream of another context");
        if (a.role < 0 || a.role > 2) return refuse("describe: ", "role must be 0 (prev cam0), 1 (curr cam0) or 2 (curr cam1)");
        if (a.n < 0) return refuse("describe: ", "negative point count");
        if (a.n > 0 && (!a.pts || !a.desc || !a.valid)) return refuse("describe: ", "null pts, desc or valid with n > 0");
        if (!s->held[pyr_of_role(s, a.role)]) return refuse("describe: ", a.role == 0 ? "the stream holds no previous image yet" : "no stereo pair pushed yet");
        in_bytes += describe_in_bytes((size_t)a.n);
        out_bytes += describe_out_bytes((size_t)a.n);
        max_pts = std::max(max_pts, a.n);
    }
    if (max_pts <= 0) return MSKF_OK;      // nothing to describe: no batch pending, _end is a no-op
    // ---- grow
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    int rc;
    mskf_ctx::PendingDescribe &D = ctx->pend_dsc;              // (no batch is pending: nobody reads it)
    if ((rc = D.jobs.ensure(n)) != MSKF_OK || (rc = D.in.ensure(in_bytes)) != MSKF_OK || (rc = D.out.ensure(out_bytes)) != MSKF_OK) return rc;
    D.n = n; D.args = args; D.out_off.resize(n);
    size_t in_off = 0, o_off = 0;
    for (int i = 0; i < n; ++i) {
        const mskf_stream *s = streams[i];
        const mskf_fe_describe_args &a = args[i];
        const size_t np = (size_t)a.n;
        FeDescribeDev &j = D.jobs.h[i];
        j.img = level0(s, pyr_of_role(s, a.role));
        j.w = s->w; j.h = s->h; j.pitch = s->w;
        if (np) std::memcpy(D.in.h + in_off, a.pts, sizeof(mskf_point2f) * np);
        j.pts = (const float *)(D.in.d + in_off);
        j.n = a.n; j.pad_ = 0;
        j.desc = (uint8_t *)(D.out.d + o_off);
        j.valid = j.desc + FB_BYTES * np;
        D.out_off[i] = o_off;
        in_off += describe_in_bytes(np); o_off += describe_out_bytes(np);
    }
    // ---- enqueue: one copy in, one launch (untimed: there is no MSKF_K_* kind for it), one copy out
    const MskfCopy cp[2] = {{D.in.d, D.in.h, in_bytes}, {D.jobs.d, D.jobs.h, sizeof(FeDescribeDev) * (size_t)n}};
    return mskf_enqueue_staged(ctx, D, cp, 2, [&] { fe_launch_describe(D.jobs.d, n, max_pts, ctx->stream); }, MskfCopy{D.out.h, D.out.d, out_bytes});
}

// Wait for the batch started by mskf_fe_describe_batch_begin and copy its results into the args given there.  No-op when nothing
// is pending.
extern "C" int mskf_fe_describe_batch_end(mskf_ctx *ctx) {
    if (!ctx) return MSKF_ERR_INVALID;
    mskf_ctx::PendingDescribe &D = ctx->pend_dsc;
    if (!D.active) return MSKF_OK;
    if (const int rc = mskf_batch_finish(ctx, D)) return rc;
    for (int i = 0; i < D.n; ++i) {
        const mskf_fe_describe_args &a = D.args[i];
        const size_t np = (size_t)a.n;
        if (!np) continue;
        const char *src = D.out.h + D.out_off[i];
        std::memcpy(a.desc, src, FB_BYTES * np);
        std::memcpy(a.valid, src + FB_BYTES * np, np);
    }
    return MSKF_OK;
}

extern "C" int mskf_fe_describe_batch(mskf_ctx *ctx, int n, mskf_stream *const *streams, mskf_fe_describe_args *args) {
    const int rc = mskf_fe_describe_batch_begin(ctx, n, streams, args);
    return rc != MSKF_OK ? rc : mskf_fe_describe_batch_end(ctx);
}

extern "C" int mskf_fe_describe(mskf_stream *s, mskf_fe_describe_args *args) {
    if (!s || !args) return refuse("describe: ", "null argument");
    mskf_stream *ss[1] = {s};
    return mskf_fe_describe_batch(s->ctx, 1, ss, args);
}

// ------------------------------------------------------------------------------------------ descriptor matching (fe_match.h)
// The distinct host arrays of a match batch, by (pointer, bytes), and where the one copy of each lies in `in`.
struct MatchSets {
    std::map<std::pair<const uint8_t *, size_t>, size_t> off;
    size_t bytes = 0;
    size_t place(const uint8_t *p, size_t n) {
        const auto it = off.find({p, n});
        if (it != off.end()) return it->second;
        const size_t o = bytes;
        off[{p, n}] = o;
        bytes += round_up(n, 64);
        return o;
    }
};

extern "C" int mskf_fe_match_batch_begin(mskf_ctx *ctx, int n, mskf_fe_match_args *args) {
    // ---- plan: every refusal comes from here, before anything is touched
    if (!ctx || !args) return refuse("match: ", "null argument");
    if (n <= 0) return refuse("match: ", "a batch has at least one job");
    if (ctx->pend_mch.active) return refuse("match: ", "a match batch of this context is still pending (call mskf_fe_match_batch_end)");
    int max_nq = 0, max_nt = 0;
    for (int i = 0; i < n; ++i) {
        const mskf_fe_match_args &a = args[i];
        if (a.nq < 0 || a.nt < 0) return refuse("match: ", "negative descriptor count");
        if (a.nq > FM_MAX_N || a.nt > FM_MAX_N) return refuse("match: ", "more than 65535 descriptors in a set");
        if (a.nq > 0 && !a.query) return refuse("match: ", "null query with nq > 0");
        if (a.nt > 0 && !a.train) return refuse("match: ", "null train with nt > 0");
        if (a.nq > 0 && !a.matches) return refuse("match: ", "null matches with nq > 0");
        if (a.max_distance < 0 || a.max_distance > FM_MAX_DISTANCE) return refuse("match: ", "max_distance must be 0 .. 256");
        if (!(a.ratio >= 0.f && a.ratio <= 1.f)) return refuse("match: ", "ratio must be 0 (off) or in (0, 1]");
        max_nq = std::max(max_nq, a.nq);
        max_nt = std::max(max_nt, a.nt);
    }
    if (max_nq <= 0) {                     // nothing to match: no batch pending, _end is a no-op
        for (int i = 0; i < n; ++i) args[i].n_matches = 0;
        return MSKF_OK;
    }
    MatchSets sets;
    mskf_ctx::PendingMatch &M = ctx->pend_mch;                 // (no batch is pending: nobody reads it)
    M.n = n; M.args = args; M.out_off.resize(n);
    size_t out_bytes = 0;
    struct Placed { size_t q, qv, t, tv; };
    std::vector<Placed> placed(n);
    for (int i = 0; i < n; ++i) {
        const mskf_fe_match_args &a = args[i];
        M.out_off[i] = out_bytes;
        if (a.nq <= 0) continue;
        placed[i].q = sets.place(a.query, (size_t)FM_BYTES * a.nq);
        placed[i].qv = a.query_valid ? sets.place(a.query_valid, (size_t)a.nq) : 0;
        placed[i].t = a.nt > 0 ? sets.place(a.train, (size_t)FM_BYTES * a.nt) : 0;
        placed[i].tv = a.nt > 0 && a.train_valid ? sets.place(a.train_valid, (size_t)a.nt) : 0;
        out_bytes += round_up(sizeof(mskf_match) * (size_t)a.nq, 64);
    }
    // ---- grow
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    int rc;
    if ((rc = M.jobs.ensure(n)) != MSKF_OK || (rc = M.in.ensure(sets.bytes)) != MSKF_OK || (rc = M.out.ensure(out_bytes)) != MSKF_OK) return rc;
    for (const auto &s : sets.off) std::memcpy(M.in.h + s.second, s.first.first, s.first.second);      // each distinct array once
    for (int i = 0; i < n; ++i) {
        const mskf_fe_match_args &a = args[i];
        FeMatchDev &j = M.jobs.h[i];
        std::memset(&j, 0, sizeof(j));
        if (a.nq <= 0) continue;           // (nq = 0: the launch skips it)
        const uint8_t *base = (const uint8_t *)M.in.d;
        j.query = base + placed[i].q;
        j.query_valid = a.query_valid ? base + placed[i].qv : nullptr;
        j.train = a.nt > 0 ? base + placed[i].t : nullptr;
        j.train_valid = a.nt > 0 && a.train_valid ? base + placed[i].tv : nullptr;
        j.nq = a.nq; j.nt = a.nt;
        j.max_distance = a.max_distance; j.ratio = a.ratio; j.cross_check = a.cross_check != 0;
        j.matches = (mskf_match *)(M.out.d + M.out_off[i]);
    }
    // ---- enqueue: one copy in, one launch (untimed: there is no MSKF_K_* kind for it), one copy out
    const MskfCopy cp[2] = {{M.in.d, M.in.h, sets.bytes}, {M.jobs.d, M.jobs.h, sizeof(FeMatchDev) * (size_t)n}};
    return mskf_enqueue_staged(ctx, M, cp, 2, [&] { fe_launch_match(M.jobs.d, n, max_nq, max_nt, ctx->stream); }, MskfCopy{M.out.h, M.out.d, out_bytes});
}

// Wait for the batch started by mskf_fe_match_batch_begin and copy its results into the args given there.  No-op when nothing
// is pending.
extern "C" int mskf_fe_match_batch_end(mskf_ctx *ctx) {
    if (!ctx) return MSKF_ERR_INVALID;
    mskf_ctx::PendingMatch &M = ctx->pend_mch;
    if (!M.active) return MSKF_OK;
    if (const int rc = mskf_batch_finish(ctx, M)) return rc;
    for (int i = 0; i < M.n; ++i) {
        mskf_fe_match_args &a = M.args[i];
        const mskf_match *src = (const mskf_match *)(M.out.h + M.out_off[i]);
        if (a.nq > 0) std::memcpy(a.matches, src, sizeof(mskf_match) * (size_t)a.nq);
        a.n_matches = a.nq > 0 ? fm_count_matches(src, a.nq) : 0;
    }
    return MSKF_OK;
}

extern "C" int mskf_fe_match_batch(mskf_ctx *ctx, int n, mskf_fe_match_args *args) {
    const int rc = mskf_fe_match_batch_begin(ctx, n, args);
    return rc != MSKF_OK ? rc : mskf_fe_match_batch_end(ctx);
}

extern "C" int mskf_fe_match(mskf_ctx *ctx, mskf_fe_match_args *args) { return mskf_fe_match_batch(ctx, 1, args); }

// ------------------------------------------------------------------------------------------ geometric verification (fe_verify.h)
// the job record of args a over `pairs` (host or device side) with n_usable staged pairs
static FeVerifyDev verify_job(const mskf_fe_verify_args &a, const double *pairs, int n_usable, unsigned long long *keys) {
    FeVerifyDev j;
    std::memset(&j, 0, sizeof(j));
    j.pairs = pairs; j.keys = keys;
    j.cam = fv_cam(a.T_cam1_cam0);
    j.seed = a.seed;
    j.max_error2 = a.max_error * a.max_error; j.min_depth = a.min_depth;
    j.n = n_usable; j.K = a.n_hypotheses;
    return j;
}

static void verify_write(mskf_fe_verify_args &a, const FvResult &r) {
    a.n_usable = r.n_usable; a.n_inliers = r.n_inliers; a.best = r.best; a.status = r.status;
    std::memcpy(a.R, r.R, sizeof(a.R)); std::memcpy(a.t, r.t, sizeof(a.t)); std::memcpy(a.info, r.info, sizeof(a.info));
    a.rms = r.rms;
}

// Bytes of the verify arenas of a context (device side): 0 until the first verify call that launches.  NOT part of the C ABI
// (declared in mskf_internal.h only, like the fe_launch_* functions): tests/test_gpu_verify.py reads it.
extern "C" size_t fe_verify_arena_bytes(const mskf_ctx *ctx) {
    const mskf_ctx::PendingVerify &V = ctx->pend_vfy;
    return V.jobs.cap * sizeof(FeVerifyDev) + V.in.cap * sizeof(double) + V.out.cap * sizeof(unsigned long long);
}

extern "C" int mskf_fe_verify_batch_begin(mskf_ctx *ctx, int n, mskf_fe_verify_args *args) {
    // ---- plan: every refusal comes from here, before anything is touched
    if (!ctx || !args) return refuse("verify: ", "null argument");
    if (n <= 0) return refuse("verify: ", "a batch has at least one job");
    if (ctx->pend_vfy.active) return refuse("verify: ", "a verify batch of this context is still pending (call mskf_fe_verify_batch_end)");
    int max_K = 0;
    for (int i = 0; i < n; ++i) {
        const mskf_fe_verify_args &a = args[i];
        if (a.n < 0) return refuse("verify: ", "negative pair count");
        if (a.n > FV_MAX_N) return refuse("verify: ", "more than 4096 pairs in a job");
        if (a.n > 0 && !a.query_obs) return refuse("verify: ", "null query_obs with n > 0");
        if (a.n > 0 && !a.train_obs) return refuse("verify: ", "null train_obs with n > 0");
        if (a.n_hypotheses < 1 || a.n_hypotheses > FV_MAX_K) return refuse("verify: ", "n_hypotheses must be 1 .. 1024");
        if (!(a.max_error > 0.0) || !std::isfinite(a.max_error)) return refuse("verify: ", "max_error must be > 0 and finite");
        if (!(a.min_depth > 0.0) || !(a.min_depth < a.max_depth) || !std::isfinite(a.max_depth)) return refuse("verify: ", "depths must be 0 < min_depth < max_depth, finite");
        for (int k = 0; k < 12; ++k) if (!std::isfinite(a.T_cam1_cam0[k])) return refuse("verify: ", "T_cam1_cam0 is not finite");
        max_K = std::max(max_K, a.n_hypotheses);
    }
    // ---- stage (host memory of the call's own): triangulate, compact the usable pairs in order, keep the map back
    mskf_ctx::PendingVerify &V = ctx->pend_vfy;                // (no batch is pending: nobody reads it)
    V.in_off.assign(n, 0); V.orig.assign(n, {});
    std::vector<std::vector<double>> staged(n);
    size_t in_doubles = 0;
    int max_usable = 0;
    for (int i = 0; i < n; ++i) {
        const mskf_fe_verify_args &a = args[i];
        V.in_off[i] = in_doubles;
        const int nu = fv_stage_host(fv_cam(a.T_cam1_cam0), a.n, a.query_obs, a.train_obs, a.usable, a.min_depth, a.max_depth, staged[i], V.orig[i]);
        in_doubles += (size_t)FV_PAIR * nu;
        max_usable = std::max(max_usable, nu);
    }
    if (max_usable < 3) {                  // no job can form a hypothesis: no launch, no batch pending, _end is a no-op
        for (int i = 0; i < n; ++i) {
            const FeVerifyDev j = verify_job(args[i], staged[i].data(), (int)V.orig[i].size(), nullptr);
            verify_write(args[i], fv_finish_host(j, V.orig[i].data(), args[i].n, FV_KEY_NONE, args[i].inlier));
        }
        return MSKF_OK;
    }
    // ---- grow
    MSKF_HIPCHK(hipSetDevice(ctx->device));
    int rc;
    const size_t n_keys = (size_t)FV_MAX_BLOCKS * n;
    if ((rc = V.jobs.ensure(n)) != MSKF_OK || (rc = V.in.ensure(in_doubles)) != MSKF_OK || (rc = V.out.ensure(n_keys)) != MSKF_OK) return rc;
    V.n = n; V.args = args;
    for (int i = 0; i < n; ++i) {
        if (!staged[i].empty()) std::memcpy(V.in.h + V.in_off[i], staged[i].data(), sizeof(double) * staged[i].size());
        V.jobs.h[i] = verify_job(args[i], V.in.d + V.in_off[i], (int)V.orig[i].size(), V.out.d + (size_t)FV_MAX_BLOCKS * i);
    }
    // ---- enqueue: one copy in, one launch (untimed: there is no MSKF_K_* kind for it), one copy out
    const MskfCopy cp[2] = {{V.in.d, V.in.h, sizeof(double) * in_doubles}, {V.jobs.d, V.jobs.h, sizeof(FeVerifyDev) * (size_t)n}};
    return mskf_enqueue_staged(ctx, V, cp, 2, [&] { fe_launch_verify(V.jobs.d, n, max_K, ctx->stream); }, MskfCopy{V.out.h, V.out.d, sizeof(unsigned long long) * n_keys});
}

// Wait for the batch started by mskf_fe_verify_batch_begin; merge every job's block keys, re-form the winner, mark its inliers
// and refine it (all with fe_verify.h, on the staged pairs still in the host side of `in`).  No-op when nothing is pending.
extern "C" int mskf_fe_verify_batch_end(mskf_ctx *ctx) {
    if (!ctx) return MSKF_ERR_INVALID;
    mskf_ctx::PendingVerify &V = ctx->pend_vfy;
    if (!V.active) return MSKF_OK;
    if (const int rc = mskf_batch_finish(ctx, V)) return rc;
    for (int i = 0; i < V.n; ++i) {
        mskf_fe_verify_args &a = V.args[i];
        const FeVerifyDev j = verify_job(a, V.in.h + V.in_off[i], (int)V.orig[i].size(), nullptr);
        unsigned long long key = FV_KEY_NONE;
        const int blocks = (a.n_hypotheses + FV_HYP_BLOCK - 1) / FV_HYP_BLOCK;
        for (int b = 0; b < blocks; ++b) key = fv_merge(key, V.out.h[(size_t)FV_MAX_BLOCKS * i + b]);
        verify_write(a, fv_finish_host(j, V.orig[i].data(), a.n, key, a.inlier));
    }
    return MSKF_OK;
}

extern "C" int mskf_fe_verify_batch(mskf_ctx *ctx, int n, mskf_fe_verify_args *args) {
    const int rc = mskf_fe_verify_batch_begin(ctx, n, args);
    return rc != MSKF_OK ? rc : mskf_fe_verify_batch_end(ctx);
}

extern "C" int mskf_fe_verify(mskf_ctx *ctx, mskf_fe_verify_args *args) { return mskf_fe_verify_batch(ctx, 1, args); }
