// csrc/hip/fe_verify.h (the header k_fe_verify and the C ABI run) compiled for the host: a small shared library for
// tests/test_verify_reference.py, which compares it with the Python restatement (tests/verify_reference.py).
#include <cstddef>
#include <cstring>
#include <vector>
#include "include/mskf_hip.h"
#include "msckf_stereo_c_amd/csrc/hip/fe_verify.h"

extern "C" {
// FV_MAX_N, FV_MAX_K, FV_TILE, FV_PAIR, FV_HYP_BLOCK, FV_REFINE_ITERS; FV_MIN_SIN2
int fv_constants(int out[6], double *min_sin2) {
    out[0] = FV_MAX_N; out[1] = FV_MAX_K; out[2] = FV_TILE; out[3] = FV_PAIR; out[4] = FV_HYP_BLOCK; out[5] = FV_REFINE_ITERS;
    *min_sin2 = FV_MIN_SIN2;
    return 6;
}

// the usable pairs of a job: returns their count, pairs takes 7 doubles and orig one int per usable pair (capacity n each)
int fv_stage(const double T[16], int n, const double *query_obs, const double *train_obs, const uint8_t *usable, double min_depth, double max_depth, double *pairs, int *orig) {
    std::vector<double> p;
    std::vector<int> o;
    const int m = fv_stage_host(fv_cam(T), n, query_obs, train_obs, usable, min_depth, max_depth, p, o);
    if (m) { std::memcpy(pairs, p.data(), sizeof(double) * p.size()); std::memcpy(orig, o.data(), sizeof(int) * o.size()); }
    return m;
}

void fv_draws(uint64_t seed, int h0, int h1, int n, uint32_t *out) {
    for (int h = h0; h < h1; ++h) fv_draw(seed, (uint32_t)h, (uint32_t)n, out + 3 * (h - h0));
}

int fv_fit(const double pq[9], const double pk[9], double R[9], double t[3]) {
    double a[3][3], b[3][3];
    std::memcpy(a, pq, sizeof(a)); std::memcpy(b, pk, sizeof(b));
    return fv_fit3(a, b, R, t) ? 1 : 0;
}

static FeVerifyDev job_of(const double T[16], const double *pairs, int n, int K, uint64_t seed, double max_error2, double min_depth) {
    FeVerifyDev J;
    std::memset(&J, 0, sizeof(J));
    J.pairs = pairs; J.cam = fv_cam(T); J.seed = seed; J.max_error2 = max_error2; J.min_depth = min_depth; J.n = n; J.K = K;
    return J;
}

// hypothesis h over the staged pairs: 1 and (R, t), or 0: void
int fv_hyp(const double T[16], const double *pairs, int n, uint64_t seed, int h, double R[9], double t[3]) {
    return n >= 3 && fv_hypothesis(fv_cam(T), pairs, (uint32_t)n, seed, (uint32_t)h, R, t) ? 1 : 0;
}

// valid[i], e2[i] of every staged pair under (R, t); returns the count of inliers (error2 < max_error2, in front)
int fv_errors(const double T[16], const double R[9], const double t[3], const double *pairs, int n, double min_depth, double max_error2, uint8_t *valid, double *e2,
              uint8_t *inlier) {
    const FvCam c = fv_cam(T);
    int count = 0;
    for (int i = 0; i < n; ++i) {
        const double *p = pairs + (size_t)FV_PAIR * i;
        double e = 0.0;
        valid[i] = fv_error2(c, R, t, p, p + 3, min_depth, &e) ? 1 : 0;
        e2[i] = e;
        inlier[i] = fv_inlier(c, R, t, p, min_depth, max_error2) ? 1 : 0;
        count += inlier[i];
    }
    return count;
}

// the key of every hypothesis 0 .. K - 1 alone, the pair list cut at `split`
void fv_keys(const double T[16], const double *pairs, int n, int K, uint64_t seed, double max_error2, double min_depth, int split, unsigned long long *keys) {
    const FeVerifyDev J = job_of(T, pairs, n, K, seed, max_error2, min_depth);
    for (int h = 0; h < K; ++h) keys[h] = fv_score_host(J, h, h + 1, split);
}

// The merged key of the job: hypotheses 0 .. hsplit - 1 and hsplit .. K - 1 scored apart, each with the pair list cut at `split`.
unsigned long long fv_score(const double T[16], const double *pairs, int n, int K, uint64_t seed, double max_error2, double min_depth, int split, int hsplit) {
    const FeVerifyDev J = job_of(T, pairs, n, K, seed, max_error2, min_depth);
    if (hsplit < 0) hsplit = 0;
    if (hsplit > K) hsplit = K;
    return fv_merge(fv_score_host(J, 0, hsplit, split), fv_score_host(J, hsplit, K, split));
}

// the number of pair splits first .. last at which the job's merged key differs from `want`
int fv_bad_pair_splits(const double T[16], const double *pairs, int n, int K, uint64_t seed, double max_error2, double min_depth, int first, int last, unsigned long long want) {
    const FeVerifyDev J = job_of(T, pairs, n, K, seed, max_error2, min_depth);
    int bad = 0;
    for (int s = first; s <= last; ++s) bad += fv_score_host(J, 0, K, s) != want ? 1 : 0;
    return bad;
}
// The same at EVERY split 0 .. n, cheaply: every hypothesis meets every pair once (fv_inlier), the count before a cut is summed
// forwards and the count from it backwards, independently, and the two add as the contract says (fv_key of the sum, fv_merge over
// the hypotheses).  O(n K) instead of O(n^2 K), for the jobs where fv_bad_pair_splits over every place would take minutes.
int fv_bad_pair_splits_all(const double T[16], const double *pairs, int n, int K, uint64_t seed, double max_error2, double min_depth, unsigned long long want) {
    const FeVerifyDev J = job_of(T, pairs, n, K, seed, max_error2, min_depth);
    std::vector<unsigned long long> key((size_t)n + 1, FV_KEY_NONE);
    if (n >= 3) {
        std::vector<uint32_t> before((size_t)n + 1), from((size_t)n + 1);
        for (int h = 0; h < K; ++h) {
            double R[9], t[3];
            if (!fv_hypothesis(J.cam, J.pairs, (uint32_t)n, seed, (uint32_t)h, R, t)) continue;
            before[0] = 0; from[n] = 0;
            for (int i = 0; i < n; ++i) before[i + 1] = before[i] + (fv_inlier(J.cam, R, t, pairs + (size_t)FV_PAIR * i, min_depth, max_error2) ? 1u : 0u);
            for (int i = n - 1; i >= 0; --i) from[i] = from[i + 1] + (fv_inlier(J.cam, R, t, pairs + (size_t)FV_PAIR * i, min_depth, max_error2) ? 1u : 0u);
            for (int s = 0; s <= n; ++s) key[s] = fv_merge(key[s], fv_key(before[s] + from[s], (uint32_t)h));
        }
    }
    int bad = 0;
    for (int s = 0; s <= n; ++s) bad += key[s] != want ? 1 : 0;
    return bad;
}
// the number of cuts 0 .. K of the hypothesis range at which the merge of the two sides' keys (given one key per hypothesis)
// differs from `want`
int fv_bad_hyp_splits(const unsigned long long *keys, int K, unsigned long long want) {
    int bad = 0;
    for (int cut = 0; cut <= K; ++cut) {
        unsigned long long a = FV_KEY_NONE, b = FV_KEY_NONE;
        for (int h = 0; h < cut; ++h) a = fv_merge(a, keys[h]);
        for (int h = cut; h < K; ++h) b = fv_merge(b, keys[h]);
        bad += fv_merge(a, b) != want ? 1 : 0;
    }
    return bad;
}
void fv_key_parts(unsigned long long key, int out[2]) { out[0] = fv_key_h(key); out[1] = fv_key_count(key); }
unsigned long long fv_key_of(uint32_t count, uint32_t h) { return fv_key(count, h); }

// The whole job as mskf_fe_verify computes it from the merged key (split / hsplit as in fv_score).  out: n_usable, n_inliers,
// best, status; pose: R[9], t[3], info[36], rms (49 doubles); inlier: n bytes.
void fv_verify(const double T[16], int n, const double *query_obs, const double *train_obs, const uint8_t *usable, int K, uint64_t seed, double max_error, double min_depth,
               double max_depth, int split, int hsplit, int out[4], double pose[49], uint8_t *inlier) {
    std::vector<double> p;
    std::vector<int> o;
    const int m = fv_stage_host(fv_cam(T), n, query_obs, train_obs, usable, min_depth, max_depth, p, o);
    const FeVerifyDev J = job_of(T, p.data(), m, K, seed, max_error * max_error, min_depth);
    const unsigned long long key = fv_score(T, p.data(), m, K, seed, max_error * max_error, min_depth, split, hsplit);
    const FvResult r = fv_finish_host(J, o.data(), n, key, inlier);
    out[0] = r.n_usable; out[1] = r.n_inliers; out[2] = r.best; out[3] = r.status;
    std::memcpy(pose, r.R, sizeof(r.R)); std::memcpy(pose + 9, r.t, sizeof(r.t)); std::memcpy(pose + 12, r.info, sizeof(r.info));
    pose[48] = r.rms;
}

// the refinement alone on the staged pairs idx[0 .. m): 1 and the refined R, t, info, rms, or 0
int fv_refine_of(const double T[16], double R[9], double t[3], const double *pairs, const int *idx, int m, double info[36], double *rms) {
    return fv_refine(fv_cam(T), R, t, pairs, idx, m, info, rms) ? 1 : 0;
}

// sizeof(FeVerifyDev) and the offsets of its fields, for the ctypes mirror of tests/test_gpu_verify.py
int fv_dev_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(FeVerifyDev), (int)offsetof(FeVerifyDev, pairs), (int)offsetof(FeVerifyDev, keys), (int)offsetof(FeVerifyDev, cam),
                     (int)offsetof(FeVerifyDev, seed), (int)offsetof(FeVerifyDev, max_error2), (int)offsetof(FeVerifyDev, min_depth), (int)offsetof(FeVerifyDev, n),
                     (int)offsetof(FeVerifyDev, K), (int)sizeof(FvCam)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
// sizeof(mskf_fe_verify_args) and the offsets of its fields in their order, for msckf_stereo_c_amd.ctypes_types.FeVerifyArgs
int fv_args_layout(int *out, int capacity) {
    typedef mskf_fe_verify_args A;
    const int v[] = {(int)sizeof(A), (int)offsetof(A, n), (int)offsetof(A, n_hypotheses), (int)offsetof(A, query_obs), (int)offsetof(A, train_obs), (int)offsetof(A, usable),
                     (int)offsetof(A, T_cam1_cam0), (int)offsetof(A, seed), (int)offsetof(A, max_error), (int)offsetof(A, min_depth), (int)offsetof(A, max_depth),
                     (int)offsetof(A, inlier), (int)offsetof(A, n_usable), (int)offsetof(A, n_inliers), (int)offsetof(A, best), (int)offsetof(A, status),
                     (int)offsetof(A, R), (int)offsetof(A, t), (int)offsetof(A, info), (int)offsetof(A, rms)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
