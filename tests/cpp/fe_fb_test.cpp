// csrc/hip/fe_fb.h (the header the forward-backward kernel and the C ABI run) compiled for the host: a small shared library
// for tests/test_fb_reference.py, which compares it with the numpy restatement (tests/fb_reference.py).
#include <cstddef>
#include "msckf_stereo_c_amd/csrc/hip/fe_fb.h"

extern "C" {
float fb_max_error(void) { return FB_MAX_ERROR; }
int fb_mode_bits(void) { return FB_TEMPORAL | (FB_STEREO << 8); }
float fb_thr2_of(float t) { return fb_thr2(t); }

// the decision over n round trips: back = where the backward track ended, origin = where it should have
void fb_pass_points(int n, const float *back, const float *origin, const uint8_t *st, float thr2, uint8_t *out) {
    for (int i = 0; i < n; ++i) out[i] = fb_pass(back[2 * i], back[2 * i + 1], origin[2 * i], origin[2 * i + 1], st[i], thr2) ? 1 : 0;
}

// sizeof(FeFbDev) and the offsets of its fields, for the ctypes mirror of tests/test_fb_reference.py
int fb_dev_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(FeFbDev), (int)offsetof(FeFbDev, thr2_t), (int)offsetof(FeFbDev, thr2_s), (int)offsetof(FeFbDev, mode)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
