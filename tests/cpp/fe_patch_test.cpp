// csrc/hip/fe_patch.h (the header the patch kernel and the C ABI run) compiled for the host: a small shared library for
// tests/test_patch_reference.py, which compares it with the numpy restatement (tests/patch_reference.py).
#include <cstring>
#include "msckf_stereo_c_amd/csrc/hip/fe_patch.h"

extern "C" {
int fp_half_min(void) { return FP_MIN_HALF; }
int fp_half_max(void) { return FP_MAX_HALF; }
double fp_thr2_of(float t) { return fp_thr2(t); }

// out[0] = the whole pixel, out[1] = the fraction in 32nds
void fp_coord_of(float x, int size, int *out) { const FpCoord c = fp_coord(x, size); out[0] = c.i; out[1] = c.a; }

// the five sums of a comparison, out = SA, SB, SAA, SBB, SAB; returns the decision at thr2
int fp_compare(const uint8_t *a, int wa, int ha, float xa, float ya, const uint8_t *b, int wb, int hb, float xb, float yb, int half, double thr2, uint32_t *out) {
    const FpSums s = fp_sums(FpImage{a, wa, ha}, xa, ya, FpImage{b, wb, hb}, xb, yb, half, 0, 1);
    out[0] = s.a; out[1] = s.b; out[2] = s.aa; out[3] = s.bb; out[4] = s.ab;
    return fp_decide(s, half, thr2) ? 1 : 0;
}

// the gate over n points, in place as k_patch_points applies it
void fp_gate_points(const uint8_t *prev0, const uint8_t *curr0, const uint8_t *curr1, int w, int h, int mode, int half, float t_temporal, float t_stereo,
                    int do_temporal, int n, const float *in_pts, const float *out0, float *out1, float *und0, float *und1, uint8_t *status) {
    const FePatchDev P{fp_thr2(t_temporal), fp_thr2(t_stereo), half, mode};
    const FpImage p0{prev0, w, h}, c0{curr0, w, h}, c1{curr1, w, h};
    for (int i = 0; i < n; ++i) {
        int what;
        const float xin = do_temporal ? in_pts[2 * i] : out0[2 * i], yin = do_temporal ? in_pts[2 * i + 1] : out0[2 * i + 1];
        const int ns = fp_gate(P, p0, c0, c1, do_temporal, xin, yin, out0[2 * i], out0[2 * i + 1], out1[2 * i], out1[2 * i + 1], status[i], &what);
        if (what == FP_LOST) { out1[2 * i] = out1[2 * i + 1] = und0[2 * i] = und0[2 * i + 1] = und1[2 * i] = und1[2 * i + 1] = 0.f; }
        status[i] = (uint8_t)ns;
    }
}

// sizeof(FePatchDev) and the offsets of its fields, for the ctypes mirror of tests/test_gpu_patch.py
int fp_patch_dev_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(FePatchDev), (int)offsetof(FePatchDev, thr2_t), (int)offsetof(FePatchDev, thr2_s), (int)offsetof(FePatchDev, half),
                     (int)offsetof(FePatchDev, mode)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
