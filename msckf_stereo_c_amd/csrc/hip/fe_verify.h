// fe_verify.h — the opt-in stereo RANSAC pose check of matched feature pairs ("Geometric verification").  ONE
// source: the kernel of fe_verify.hip, the C ABI (mskf_fe_verify*) and the g++-compiled CPU harness
// (tests/cpp/fe_verify_test.cpp) all run these functions.  FP64, compiled with -ffp-contract=off: the operation order written
// here IS the arithmetic; sums go left to right.  Beyond + - * only / and sqrt are used (both correctly rounded on host and
// device), and no libm transcendental anywhere, so tests/verify_reference.py restates every function bit for bit.
//   observation  (x0, y0, x1, y1): a feature's undistorted normalised coordinates in cam0 and cam1;
//   camera       p_c1 = R10 p_c0 + t10 (the row-major 4x4 T_cam1_cam0 of mskf_calib);
//   triangulate  m = R10 (x0, y0, 1), A = (m0 - x1 m2, m1 - y1 m2), b = (x1 t10z - t10x, y1 t10z - t10y), depth d = (A.b)/(A.A),
//                point (x0 d, y0 d, d) in cam0;
//   usable       the caller's byte != 0 (absent: all), and on BOTH sides A.A > 0 and min_depth <= d <= max_depth (d finite);
//   draw         fv_draw(seed, h, n): three distinct indices into the n usable pairs, a function of its arguments alone;
//   fit          p_k = R p_q + t from three pairs by orthonormal triads; void if either triangle is too thin (FV_MIN_SIN2);
//   error2       p0 = R a + t, p1 = R10 p0 + t10; p0z < min_depth or p1z < min_depth: not an inlier; else the sum of the four
//                squared differences of (p0x/p0z, p0y/p0z, p1x/p1z, p1y/p1z) and the keyframe's observation;
//   inlier       error2 < max_error^2, strictly;
//   score        the integer count of inliers over all usable pairs; a void triad has no score and never wins; the highest
//                count wins, the LOWEST h among equal counts;
//   merge        counts over disjoint pair ranges add; keys over disjoint hypothesis ranges merge by max (fv_merge): the
//                result cannot depend on how pairs or hypotheses are cut over wavefronts, workgroups or launches;
//   refine       (host) FV_REFINE_ITERS Gauss-Newton steps on the winner's inlier set, which stays fixed.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FV_FN __host__ __device__ __forceinline__
#else
#define FV_FN inline
#endif

#define FV_MAX_N 4096                                // pairs of a job
#define FV_MAX_K 1024                                // hypotheses of a job
#define FV_HYP_BLOCK 64                              // hypotheses of a workgroup: one per lane
#define FV_MAX_BLOCKS (FV_MAX_K / FV_HYP_BLOCK)      // 16 keys come back per job at most
#define FV_TILE 256                                  // usable pairs the kernel stages at a time
#define FV_PAIR 7                                    // doubles of a staged pair: a (the query point in the query's cam0), obs_k
// |d1 x d2|^2 >= FV_MIN_SIN2 |d1|^2 |d2|^2, the squared sine of the sample triangle's angle at p0: scale-free.  A starting value
// nobody has tuned.
#define FV_MIN_SIN2 1e-4
#define FV_REFINE_ITERS 5
#define FV_KEY_NONE 0ull                             // no hypothesis (void triads only)
#define FV_DRAW_C 0x5FE7E21F5FE7E21FULL              // the draws' own constant (fe_brief.h has another)

struct FvCam { double R[9], t[3]; };                 // R10 row-major, t10

// One job of a k_fe_verify launch: n usable pairs of FV_PAIR doubles, K hypotheses.  n < 3 or K <= 0: its keys are FV_KEY_NONE.
struct FeVerifyDev {
    const double *pairs;                  // FV_PAIR n doubles, 8-byte aligned
    unsigned long long *keys;             // out: ceil(K / FV_HYP_BLOCK) keys, one per workgroup
    FvCam cam;
    uint64_t seed;
    double max_error2, min_depth;
    int n, K;
};

FV_FN FvCam fv_cam(const double T[16]) {
    FvCam c;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) c.R[3 * i + j] = T[4 * i + j]; c.t[i] = T[4 * i + 3]; }
    return c;
}

// ---- small fixed-order algebra
FV_FN double fv_dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
FV_FN void fv_mat_vec(const double M[9], const double v[3], double out[3]) {
    for (int i = 0; i < 3; ++i) out[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}
FV_FN void fv_cross(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- triangulation: false where A.A is not > 0 (then *d is not to be used)
FV_FN bool fv_triangulate(const FvCam &c, const double o[4], double *d) {
    const double ray[3] = {o[0], o[1], 1.0};
    double m[3];
    fv_mat_vec(c.R, ray, m);
    const double a0 = m[0] - o[2] * m[2], a1 = m[1] - o[3] * m[2];
    const double b0 = o[2] * c.t[2] - c.t[0], b1 = o[3] * c.t[2] - c.t[1];
    const double aa = a0 * a0 + a1 * a1, ab = a0 * b0 + a1 * b1;
    if (!(aa > 0.0)) return false;
    *d = ab / aa;
    return true;
}
FV_FN bool fv_depth_ok(double d, double min_depth, double max_depth) { return d >= min_depth && d <= max_depth; }      // (NaN: false)
FV_FN void fv_point(const double o[4], double d, double p[3]) { p[0] = o[0] * d; p[1] = o[1] * d; p[2] = d; }
// an observation's point, where the pair is usable on this side
FV_FN bool fv_usable_point(const FvCam &c, const double o[4], double min_depth, double max_depth, double p[3]) {
    double d;
    if (!fv_triangulate(c, o, &d) || !fv_depth_ok(d, min_depth, max_depth)) return false;
    fv_point(o, d, p);
    return true;
}

// ---- draws: splitmix64's finaliser; draw k = 1, 2, .. of the stream that `seed` names
FV_FN uint64_t fv_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
    z ^= z >> 27; z *= 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}
FV_FN uint64_t fv_rand(uint64_t seed, uint64_t k) { return fv_mix(fv_mix(seed + FV_DRAW_C) + 0x9E3779B97F4A7C15ULL * k); }
// three distinct indices 0 .. n - 1 (n >= 3) of hypothesis h: no redraws
FV_FN void fv_draw(uint64_t seed, uint32_t h, uint32_t n, uint32_t idx[3]) {
    const uint64_t k = 3ull * h;
    uint32_t i0 = (uint32_t)(fv_rand(seed, k + 1) % n);
    uint32_t i1 = (uint32_t)(fv_rand(seed, k + 2) % (n - 1));
    uint32_t i2 = (uint32_t)(fv_rand(seed, k + 3) % (n - 2));
    if (i1 >= i0) ++i1;
    const uint32_t lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    if (i2 >= lo) ++i2;
    if (i2 >= hi) ++i2;
    idx[0] = i0; idx[1] = i1; idx[2] = i2;
}

// ---- the triad of three points: F = (e1 e2 e3) as columns (row-major 3x3), c = their mean; false: void
FV_FN bool fv_triad(const double p[3][3], double F[9], double c[3]) {
    double d1[3], d2[3], cr[3];
    for (int i = 0; i < 3; ++i) { d1[i] = p[1][i] - p[0][i]; d2[i] = p[2][i] - p[0][i]; }
    fv_cross(d1, d2, cr);
    const double n1 = fv_dot3(d1, d1), n2 = fv_dot3(d2, d2), nc = fv_dot3(cr, cr);
    const double prod = n1 * n2;
    if (!(prod > 0.0) || !(nc >= FV_MIN_SIN2 * prod)) return false;
    const double s1 = sqrt(n1), s3 = sqrt(nc);
    double e1[3], e2[3], e3[3];
    for (int i = 0; i < 3; ++i) { e1[i] = d1[i] / s1; e3[i] = cr[i] / s3; }
    fv_cross(e3, e1, e2);
    for (int i = 0; i < 3; ++i) {
        F[3 * i] = e1[i]; F[3 * i + 1] = e2[i]; F[3 * i + 2] = e3[i];
        c[i] = ((p[0][i] + p[1][i]) + p[2][i]) / 3.0;
    }
    return true;
}
// p_k = R p_q + t from three pairs: R = F_k F_q^T, t = c_k - R c_q
FV_FN bool fv_fit3(const double pq[3][3], const double pk[3][3], double R[9], double t[3]) {
    double Fq[9], Fk[9], cq[3], ck[3];
    const bool okq = fv_triad(pq, Fq, cq), okk = fv_triad(pk, Fk, ck);
    if (!okq || !okk) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (Fk[3 * i] * Fq[3 * j] + Fk[3 * i + 1] * Fq[3 * j + 1]) + Fk[3 * i + 2] * Fq[3 * j + 2];
    double rc[3];
    fv_mat_vec(R, cq, rc);
    for (int i = 0; i < 3; ++i) t[i] = ck[i] - rc[i];
    return true;
}

// ---- the reprojection error of a pair (a, obs_k) under (R, t); false: behind a camera, never an inlier
FV_FN bool fv_error2(const FvCam &c, const double R[9], const double t[3], const double a[3], const double o[4], double min_depth, double *e2) {
    double q[3], p0[3], r1[3], p1[3];
    fv_mat_vec(R, a, q);
    for (int i = 0; i < 3; ++i) p0[i] = q[i] + t[i];
    fv_mat_vec(c.R, p0, r1);
    for (int i = 0; i < 3; ++i) p1[i] = r1[i] + c.t[i];
    if (!(p0[2] >= min_depth) || !(p1[2] >= min_depth)) return false;
    const double r0 = p0[0] / p0[2] - o[0], ry = p0[1] / p0[2] - o[1], r2 = p1[0] / p1[2] - o[2], r3 = p1[1] / p1[2] - o[3];
    *e2 = ((r0 * r0 + ry * ry) + r2 * r2) + r3 * r3;
    return true;
}
FV_FN bool fv_inlier(const FvCam &c, const double R[9], const double t[3], const double pair[FV_PAIR], double min_depth, double max_error2) {
    double e2;
    return fv_error2(c, R, t, pair, pair + 3, min_depth, &e2) && e2 < max_error2;
}

// ---- keys: a non-void hypothesis h (0 .. 65535) with `count` inliers; the maximum wins
FV_FN unsigned long long fv_key(uint32_t count, uint32_t h) { return (1ull << 32) | ((unsigned long long)count << 16) | (0xFFFFu - h); }
FV_FN unsigned long long fv_merge(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
FV_FN int fv_key_h(unsigned long long key) { return key == FV_KEY_NONE ? -1 : (int)(0xFFFFu - (uint32_t)(key & 0xFFFFu)); }
FV_FN int fv_key_count(unsigned long long key) { return (int)((key >> 16) & 0xFFFFu); }

// hypothesis h of a job: its (R, t) from the staged pairs (the keyframe's point is triangulated again from obs_k: the same
// function gives the same bits as the staging did); false: void
FV_FN bool fv_hypothesis(const FvCam &c, const double *pairs, uint32_t n, uint64_t seed, uint32_t h, double R[9], double t[3]) {
    uint32_t idx[3];
    fv_draw(seed, h, n, idx);
    double pq[3][3], pk[3][3];
    bool ok = true;
    for (int s = 0; s < 3; ++s) {
        const double *p = pairs + (size_t)FV_PAIR * idx[s];
        for (int i = 0; i < 3; ++i) pq[s][i] = p[i];
        double d = 0.0;
        ok = fv_triangulate(c, p + 3, &d) && ok;
        fv_point(p + 3, d, pk[s]);
    }
    return fv_fit3(pq, pk, R, t) && ok;
}

#include <vector>

// ---- staging (host): the usable pairs of a job in order, FV_PAIR doubles each, and their original indices
inline int fv_stage_host(const FvCam &c, int n, const double *query_obs, const double *train_obs, const uint8_t *usable, double min_depth, double max_depth,
                         std::vector<double> &pairs, std::vector<int> &orig) {
    pairs.clear(); orig.clear();
    for (int i = 0; i < n; ++i) {
        if (usable && !usable[i]) continue;
        double a[3], pk[3];
        const bool okq = fv_usable_point(c, query_obs + 4 * (size_t)i, min_depth, max_depth, a);
        const bool okk = fv_usable_point(c, train_obs + 4 * (size_t)i, min_depth, max_depth, pk);
        if (!okq || !okk) continue;
        for (int k = 0; k < 3; ++k) pairs.push_back(a[k]);
        for (int k = 0; k < 4; ++k) pairs.push_back(train_obs[4 * (size_t)i + k]);
        orig.push_back(i);
    }
    return (int)orig.size();
}

// ---- the score of the hypotheses h0 .. h1 - 1 over the staged pairs, with the pair list cut at `split` (counts add) — what a
// workgroup of the kernel computes for its 64 hypotheses with the tile quarters of its four wavefronts as the parts
inline unsigned long long fv_score_host(const FeVerifyDev &J, int h0, int h1, int split) {
    unsigned long long key = FV_KEY_NONE;
    if (J.n < 3) return key;
    if (split < 0) split = 0;
    if (split > J.n) split = J.n;
    for (int h = h0; h < h1; ++h) {
        double R[9], t[3];
        if (!fv_hypothesis(J.cam, J.pairs, (uint32_t)J.n, J.seed, (uint32_t)h, R, t)) continue;
        uint32_t lo = 0, hi = 0;
        for (int i = 0; i < split; ++i) lo += fv_inlier(J.cam, R, t, J.pairs + (size_t)FV_PAIR * i, J.min_depth, J.max_error2) ? 1u : 0u;
        for (int i = split; i < J.n; ++i) hi += fv_inlier(J.cam, R, t, J.pairs + (size_t)FV_PAIR * i, J.min_depth, J.max_error2) ? 1u : 0u;
        key = fv_merge(key, fv_key(lo + hi, (uint32_t)h));
    }
    return key;
}

// ---- refinement (host only)
// the unpivoted Cholesky solve of the 6 x 6 system H x = b (H symmetric, row-major); false: a pivot <= 0 (or NaN)
inline bool fv_chol6_solve(const double H[36], const double b[6], double x[6]) {
    double L[36];
    for (int i = 0; i < 36; ++i) L[i] = 0.0;
    for (int j = 0; j < 6; ++j) {
        double s = H[6 * j + j];
        for (int k = 0; k < j; ++k) s = s - L[6 * j + k] * L[6 * j + k];
        if (!(s > 0.0)) return false;
        const double ljj = sqrt(s);
        L[6 * j + j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
            double v = H[6 * i + j];
            for (int k = 0; k < j; ++k) v = v - L[6 * i + k] * L[6 * j + k];
            L[6 * i + j] = v / ljj;
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v = v - L[6 * i + k] * y[k];
        y[i] = v / L[6 * i + i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v = v - L[6 * k + i] * x[k];
        x[i] = v / L[6 * i + i];
    }
    return true;
}

// J^T J (6 x 6, order [theta, t]), J^T r and the sum of squared residuals of the pairs idx[0 .. m) under (R, t), summed in that
// order from 0.0.  Left perturbation p0 <- dR (R a) + t + dt: d p0 / d[theta, t] = [-[R a]x, I], chained through p1 = R10 p0 + t10
// and the two projections (u = x / z: du = (dx - u dz) / z).
inline void fv_normal_equations(const FvCam &c, const double R[9], const double t[3], const double *pairs, const int *idx, int m, double H[36], double g[6], double *ss) {
    for (int i = 0; i < 36; ++i) H[i] = 0.0;
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
    double S = 0.0;
    for (int s = 0; s < m; ++s) {
        const double *a = pairs + (size_t)FV_PAIR * idx[s], *o = a + 3;
        double q[3], p0[3], r1[3], p1[3];
        fv_mat_vec(R, a, q);
        for (int i = 0; i < 3; ++i) p0[i] = q[i] + t[i];
        fv_mat_vec(c.R, p0, r1);
        for (int i = 0; i < 3; ++i) p1[i] = r1[i] + c.t[i];
        // d p0: rows x, y, z over the six parameters
        const double D0[3][6] = {{0.0, q[2], -q[1], 1.0, 0.0, 0.0}, {-q[2], 0.0, q[0], 0.0, 1.0, 0.0}, {q[1], -q[0], 0.0, 0.0, 0.0, 1.0}};
        double D1[3][6];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 6; ++j) D1[i][j] = (c.R[3 * i] * D0[0][j] + c.R[3 * i + 1] * D0[1][j]) + c.R[3 * i + 2] * D0[2][j];
        const double u0 = p0[0] / p0[2], v0 = p0[1] / p0[2], u1 = p1[0] / p1[2], v1 = p1[1] / p1[2];
        const double r[4] = {u0 - o[0], v0 - o[1], u1 - o[2], v1 - o[3]};
        double Jm[4][6];
        for (int j = 0; j < 6; ++j) {
            Jm[0][j] = (D0[0][j] - u0 * D0[2][j]) / p0[2];
            Jm[1][j] = (D0[1][j] - v0 * D0[2][j]) / p0[2];
            Jm[2][j] = (D1[0][j] - u1 * D1[2][j]) / p1[2];
            Jm[3][j] = (D1[1][j] - v1 * D1[2][j]) / p1[2];
        }
        for (int k = 0; k < 4; ++k) {
            for (int i = 0; i < 6; ++i) {
                for (int j = i; j < 6; ++j) H[6 * i + j] = H[6 * i + j] + Jm[k][i] * Jm[k][j];
                g[i] = g[i] + Jm[k][i] * r[k];
            }
            S = S + r[k] * r[k];
        }
    }
    for (int i = 0; i < 6; ++i) for (int j = 0; j < i; ++j) H[6 * i + j] = H[6 * j + i];
    *ss = S;
}

// the rotation of the unit quaternion (theta / 2, 1) / |.|
inline void fv_small_rotation(const double th[3], double dR[9]) {
    const double vx = th[0] * 0.5, vy = th[1] * 0.5, vz = th[2] * 0.5;
    const double nn = sqrt(((vx * vx + vy * vy) + vz * vz) + 1.0);
    const double x = vx / nn, y = vy / nn, z = vz / nn, w = 1.0 / nn;
    dR[0] = 1.0 - 2.0 * (y * y + z * z); dR[1] = 2.0 * (x * y - w * z);       dR[2] = 2.0 * (x * z + w * y);
    dR[3] = 2.0 * (x * y + w * z);       dR[4] = 1.0 - 2.0 * (x * x + z * z); dR[5] = 2.0 * (y * z - w * x);
    dR[6] = 2.0 * (x * z - w * y);       dR[7] = 2.0 * (y * z + w * x);       dR[8] = 1.0 - 2.0 * (x * x + y * y);
}

// FV_REFINE_ITERS Gauss-Newton steps from (R, t) on the pairs idx[0 .. m) (ascending), then one more evaluation: info = J^T J
// and rms = sqrt(sum of squared residuals / (4 m)).  false: a Cholesky pivot <= 0 (or m = 0): R, t untouched, info zero, rms 0.
inline bool fv_refine(const FvCam &c, double R[9], double t[3], const double *pairs, const int *idx, int m, double info[36], double *rms) {
    double Rw[9], tw[3], H[36], g[6], S;
    for (int i = 0; i < 9; ++i) Rw[i] = R[i];
    for (int i = 0; i < 3; ++i) tw[i] = t[i];
    bool ok = m > 0;
    for (int it = 0; ok && it < FV_REFINE_ITERS; ++it) {
        fv_normal_equations(c, Rw, tw, pairs, idx, m, H, g, &S);
        double rhs[6], dx[6], dR[9], Rn[9];
        for (int i = 0; i < 6; ++i) rhs[i] = -g[i];
        if (!fv_chol6_solve(H, rhs, dx)) { ok = false; break; }
        fv_small_rotation(dx, dR);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (dR[3 * i] * Rw[j] + dR[3 * i + 1] * Rw[3 + j]) + dR[3 * i + 2] * Rw[6 + j];
        for (int i = 0; i < 9; ++i) Rw[i] = Rn[i];
        for (int i = 0; i < 3; ++i) tw[i] = tw[i] + dx[3 + i];
    }
    if (ok) {
        fv_normal_equations(c, Rw, tw, pairs, idx, m, H, g, &S);
        double dx[6];
        ok = fv_chol6_solve(H, g, dx);            // (the pivots of the final information matrix are checked as well)
    }
    if (!ok) {
        for (int i = 0; i < 36; ++i) info[i] = 0.0;
        *rms = 0.0;
        return false;
    }
    for (int i = 0; i < 9; ++i) R[i] = Rw[i];
    for (int i = 0; i < 3; ++i) t[i] = tw[i];
    for (int i = 0; i < 36; ++i) info[i] = H[i];
    *rms = sqrt(S / (4.0 * (double)m));
    return true;
}

// ---- a whole job on the host from the merged key: what mskf_fe_verify_batch_end does for every job, and the harness.
struct FvResult {
    int n_usable = 0, n_inliers = 0, best = -1, status = 1;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, info[36] = {0}, rms = 0;
};
// inlier (n_original bytes, may be null) is zeroed and set at the original indices of the winner's inliers
inline FvResult fv_finish_host(const FeVerifyDev &J, const int *orig, int n_original, unsigned long long key, uint8_t *inlier, bool refine = true) {
    FvResult r;
    r.n_usable = J.n;
    if (inlier) for (int i = 0; i < n_original; ++i) inlier[i] = 0;
    r.best = fv_key_h(key);
    if (r.best < 0) return r;
    double R[9], t[3];
    fv_hypothesis(J.cam, J.pairs, (uint32_t)J.n, J.seed, (uint32_t)r.best, R, t);
    std::vector<int> in;
    for (int i = 0; i < J.n; ++i)
        if (fv_inlier(J.cam, R, t, J.pairs + (size_t)FV_PAIR * i, J.min_depth, J.max_error2)) { in.push_back(i); if (inlier) inlier[orig[i]] = 1; }
    r.n_inliers = (int)in.size();
    r.status = 0;
    if (refine && !fv_refine(J.cam, R, t, J.pairs, in.data(), (int)in.size(), r.info, &r.rms)) r.status = 2;
    for (int i = 0; i < 9; ++i) r.R[i] = R[i];
    for (int i = 0; i < 3; ++i) r.t[i] = t[i];
    return r;
}
