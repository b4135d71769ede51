// csrc/hip/fe_deep.h (the header the deep-pyramid kernels, the C ABI and the host mirror run) compiled for the host: a small shared
// library for tests/test_deep_lk_reference.py, which compares it with the restated rule and with the oracle's pyr_down.
#include <cstddef>
#include "msckf_stereo_c_amd/csrc/hip/fe_deep.h"

extern "C" {
int fd_limits(void) { return FD_BASE_LEVELS | (FD_MAX_LEVELS << 8) | (FD_MIN_SIDE << 16); }
int fd_max_levels_of(int w, int h) { return fd_max_levels(w, h); }
int fd_validate_of(int w, int h, int L) { return fd_validate(w, h, L); }
int fd_side_of(int n, int l) { return fd_side(n, l); }

// one level of the chain as k_pyr_down_deep forms it: every output pixel through fd_pyr_down_px
void fd_pyr_down(const uint8_t *src, int W, int H, uint8_t *dst) {
    const int w = fd_half(W), h = fd_half(H);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) dst[y * w + x] = fd_pyr_down_px(src, W, H, x, y);
}

// sizeof(FeDeepDev), sizeof(PyrDeepDev), sizeof(DeepPyrJob) and the offsets of their fields, for the ctypes mirrors of the tests
int fd_dev_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(FeDeepDev), (int)sizeof(PyrDeepDev), (int)offsetof(PyrDeepDev, w), (int)offsetof(PyrDeepDev, h),
                     (int)offsetof(FeDeepDev, curr0), (int)offsetof(FeDeepDev, curr1), (int)offsetof(FeDeepDev, levels),
                     (int)sizeof(DeepPyrJob), (int)offsetof(DeepPyrJob, dst), (int)offsetof(DeepPyrJob, w), (int)offsetof(DeepPyrJob, levels)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
