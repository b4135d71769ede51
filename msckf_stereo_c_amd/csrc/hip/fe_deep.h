// fe_deep.h — the opt-in deeper LK pyramids ("Deeper LK pyramids"): a stream may track over L = 5 .. 8 levels
// instead of 4.  ONE source for the size chain and the validity rule: the kernels (fe_deep.hip, fe_lk.h), the setter of the C
// ABI, the host mirror's yaml check and the g++-compiled CPU harness (tests/cpp/fe_deep_test.cpp) all run these functions.
//   sizes     level l + 1 is ((w_l + 1) / 2, (h_l + 1) / 2), the rule of the levels 1 .. 3;
//   validity  4 <= L <= 8, and both sides of level L - 1 are at least 15 (the LK window): 752 x 480 allows up to 6,
//             3840 x 2160 allows 8, 239 x 120 only 4.
// The extra levels 4 .. L - 1 travel beside PyrDev / FeStreamDev, which stay as they are: element i of a FeDeepDev array goes
// with descriptor i of a launch, and levels == 4 means "this stream is not deep".
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FDP_FN __host__ __device__ __forceinline__
#else
#define FDP_FN inline
#endif

#define FD_BASE_LEVELS 4       // == MSKF_LEVELS: what every stream has
#define FD_MAX_LEVELS 8
#define FD_EXTRA (FD_MAX_LEVELS - FD_BASE_LEVELS)
#define FD_MIN_SIDE 15         // == LK_WIN

FDP_FN int fd_half(int n) { return (n + 1) / 2; }
// side of level l of an image whose level 0 has side n
FDP_FN int fd_side(int n, int l) {
    for (int i = 0; i < l; ++i) n = fd_half(n);
    return n;
}
// the largest L (4 .. 8) a w x h image allows; 4 is always allowed (it is what runs without this option)
FDP_FN int fd_max_levels(int w, int h) {
    int L = FD_BASE_LEVELS;
    while (L < FD_MAX_LEVELS && fd_side(w, L) >= FD_MIN_SIDE && fd_side(h, L) >= FD_MIN_SIDE) ++L;
    return L;
}
// 0: fine, 1: L outside 4 .. 8, 2: the image is too small for L
FDP_FN int fd_validate(int w, int h, int L) {
    if (L < FD_BASE_LEVELS || L > FD_MAX_LEVELS) return 1;
    return L > fd_max_levels(w, h) ? 2 : 0;
}
// BORDER_REFLECT_101 for -n < i < 2 n - 1 (one reflection: a five-tap filter on a side of at least 3)
FDP_FN int fd_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
// one output pixel of pyr_down: the separable [1 4 6 4 1] filter, total weight 256, (s + 128) >> 8, reflect-101
FDP_FN uint8_t fd_pyr_down_px(const uint8_t *src, int W, int H, int x, int y) {
    const int x0 = fd_reflect(2 * x - 2, W), x1 = fd_reflect(2 * x - 1, W), x2 = 2 * x, x3 = fd_reflect(2 * x + 1, W), x4 = fd_reflect(2 * x + 2, W);
    int s = 0;
    for (int j = -2; j <= 2; ++j) {
        const uint8_t *row = src + (long long)fd_reflect(2 * y + j, H) * W;
        const int hs = (row[x0] + row[x4]) + 4 * (row[x1] + row[x3]) + 6 * row[x2];
        s += (j == -2 || j == 2 ? 1 : (j == 0 ? 6 : 4)) * hs;
    }
    return (uint8_t)((s + 128) >> 8);
}

// Levels 4 .. 7 of one pyramid (index l - 4); what a stream's L does not reach is null / 0.
struct PyrDeepDev {
    const uint8_t *lvl[FD_EXTRA];
    int w[FD_EXTRA], h[FD_EXTRA];
};
// What the deep instantiations of the track kernels read of a stream beside its FeStreamDev.
struct FeDeepDev {
    PyrDeepDev prev0, curr0, curr1;
    int levels;                        // 4 .. 8; 4 = this stream is not deep
    int pad_;
};
// One image of a push of a deep stream: level 3 in, levels 4 .. levels - 1 out (k_pyr_down_deep).
struct DeepPyrJob {
    const uint8_t *src;                // level 3, w x h
    uint8_t *dst[FD_EXTRA];
    int w, h, levels, pad_;
};
