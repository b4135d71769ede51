// fe_patch.h — the opt-in ZNCC patch check of temporal tracks and stereo matches ("Patch check"): is the patch
// around a tracked point still the patch it was tracked from?  ONE source: the kernel of fe_patch.hip (k_patch_points), the
// setter of the C ABI and the g++-compiled CPU harness (tests/cpp/fe_patch_test.cpp) all run these functions.  Integer
// arithmetic but three float32 operations per coordinate and four float64 operations per comparison; compiled with
// -ffp-contract=off like everything else.
//   parameters  half 2 .. 7: a patch is (2 half + 1)^2 samples, N of them; mode bits: 1 temporal, 2 stereo; thr2 = the
//               threshold squared, (double)t * (double)t, formed once on the host;
//   coordinate  x = fminf(fmaxf(x, 0), W - 1) (a NaN becomes 0); fx = floorf(x), ix = (int)fx, ax = (int)((x - fx) * 32.0f);
//   sample      at (dx, dy): the pixels at columns ix + dx, ix + dx + 1 and rows iy + dy, iy + dy + 1, each index clamped to
//               the image; s = (32-ax)(32-ay) I00 + ax (32-ay) I10 + (32-ax) ay I01 + ax ay I11; v = (s + 128) >> 8, 0 .. 1020;
//   sums        over the patch, exact: SA, SB, SAA, SBB, SAB, each below 2^32 (225 * 1020^2); in int64 num = N SAB - SA SB,
//               va = N SAA - SA^2, vb = N SBB - SB^2;
//   decision    va == 0 and vb == 0: passes (nothing to judge); else passes iff num > 0 and
//               (double)num * (double)num >= thr2 * ((double)va * (double)vb).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FP_FN __host__ __device__ __forceinline__
#else
#define FP_FN inline
#endif

#define FP_MIN_HALF 2
#define FP_MAX_HALF 7
enum { FP_TEMPORAL = 1, FP_STEREO = 2 };      // mode bits

// What the patch kernel reads of a stream beside its FeStreamDev: element i of a second array goes with descriptor i of the
// launch.  mode == 0 = this stream is not checked.
struct FePatchDev {
    double thr2_t, thr2_s;             // squared thresholds of the temporal / the stereo comparison
    int half, mode;
};

FP_FN double fp_thr2(float t) { return (double)t * (double)t; }

struct FpImage { const uint8_t *px; int w, h; };      // a dense level-0 plane, pitch == width
struct FpCoord { int i, a; };                         // whole pixel, and the fraction in 32nds (0 .. 31)

// one coordinate of a point in an image `size` pixels wide (or high)
FP_FN FpCoord fp_coord(float x, int size) {
    x = fminf(fmaxf(x, 0.f), (float)(size - 1));
    const float fx = floorf(x);
    return FpCoord{(int)fx, (int)((x - fx) * 32.0f)};
}

FP_FN int fp_clamp(int v, int size) { return v < 0 ? 0 : (v >= size ? size - 1 : v); }

// the sample at offset (dx, dy) of the point (cx, cy): 0 .. 1020
FP_FN uint32_t fp_sample(const FpImage &I, FpCoord cx, FpCoord cy, int dx, int dy) {
    const int x0 = fp_clamp(cx.i + dx, I.w), x1 = fp_clamp(cx.i + dx + 1, I.w);
    const uint8_t *r0 = I.px + (size_t)fp_clamp(cy.i + dy, I.h) * I.w, *r1 = I.px + (size_t)fp_clamp(cy.i + dy + 1, I.h) * I.w;
    const uint32_t ax = (uint32_t)cx.a, ay = (uint32_t)cy.a;
    const uint32_t s = (32u - ax) * (32u - ay) * r0[x0] + ax * (32u - ay) * r0[x1] + (32u - ax) * ay * r1[x0] + ax * ay * r1[x1];
    return (s + 128u) >> 8;
}

struct FpSums { uint32_t a, b, aa, bb, ab; };

// The sums over the samples j0, j0 + stride, ... of the patch (sample j lies at dx = j % (2 half + 1) - half, dy = j / (2 half
// + 1) - half): the whole patch with (0, 1), a lane's share of it with (lane, 16).
FP_FN FpSums fp_sums(const FpImage &A, float xa, float ya, const FpImage &B, float xb, float yb, int half, int j0, int stride) {
    const FpCoord ax = fp_coord(xa, A.w), ay = fp_coord(ya, A.h), bx = fp_coord(xb, B.w), by = fp_coord(yb, B.h);
    const int side = 2 * half + 1, n = side * side;
    FpSums s{0u, 0u, 0u, 0u, 0u};
    for (int j = j0; j < n; j += stride) {
        const int dy = j / side - half, dx = j % side - half;
        const uint32_t a = fp_sample(A, ax, ay, dx, dy), b = fp_sample(B, bx, by, dx, dy);
        s.a += a; s.b += b; s.aa += a * a; s.bb += b * b; s.ab += a * b;
    }
    return s;
}

// the decision on the sums of a whole patch
FP_FN bool fp_decide(const FpSums &s, int half, double thr2) {
    const long long n = (long long)(2 * half + 1) * (2 * half + 1);
    const long long num = n * (long long)s.ab - (long long)s.a * (long long)s.b;
    const long long va = n * (long long)s.aa - (long long)s.a * (long long)s.a, vb = n * (long long)s.bb - (long long)s.b * (long long)s.b;
    if (va == 0 && vb == 0) return true;
    return num > 0 && (double)num * (double)num >= thr2 * ((double)va * (double)vb);
}

// The gate for one point of a track call, as one of `stride` workers that take the samples lane, lane + stride, ...;
// `reduce` adds the workers' sums up, so that each of them holds the sums of the whole patch.  status: bit 0 = the temporal half
// survived, bit 1 = stereo inlier.  Returns the new status; FP_LOST in *what when the point is lost the way k_track4 loses one
// (the caller then zeroes out1, und0 and und1 and keeps out0).  The temporal comparison (in_pts in prev0 against out0 in
// curr0) runs first, on calls with do_temporal; a point lost there is not compared again.  The stereo comparison is out0 in
// curr0 against out1 in curr1.
enum { FP_KEEP = 0, FP_LOST = 1 };
template <class Reduce>
FP_FN int fp_gate_shared(const FePatchDev &P, const FpImage &prev0, const FpImage &curr0, const FpImage &curr1, int do_temporal, float xin, float yin,
                         float x0, float y0, float x1, float y1, int status, int lane, int stride, Reduce reduce, int *what) {
    *what = FP_KEEP;
    if ((P.mode & FP_TEMPORAL) && do_temporal && (status & 1)) {
        FpSums s = fp_sums(prev0, xin, yin, curr0, x0, y0, P.half, lane, stride);
        reduce(s);
        if (!fp_decide(s, P.half, P.thr2_t)) { *what = FP_LOST; return 0; }
    }
    if ((P.mode & FP_STEREO) && (status & 2)) {
        FpSums s = fp_sums(curr0, x0, y0, curr1, x1, y1, P.half, lane, stride);
        reduce(s);
        if (!fp_decide(s, P.half, P.thr2_s)) return status & ~2;
    }
    return status;
}

struct FpAlone { FP_FN void operator()(FpSums &) const {} };

// ... and for one point alone
FP_FN int fp_gate(const FePatchDev &P, const FpImage &prev0, const FpImage &curr0, const FpImage &curr1, int do_temporal, float xin, float yin, float x0,
                  float y0, float x1, float y1, int status, int *what) {
    return fp_gate_shared(P, prev0, curr0, curr1, do_temporal, xin, yin, x0, y0, x1, y1, status, 0, 1, FpAlone(), what);
}
