// csrc/hip/fe_mask.h (the header the mask kernels and the C ABI run) compiled for the host: a small shared library for
// tests/test_mask_reference.py, which compares it with the numpy restatement (tests/mask_reference.py).
#include <cstring>
#include "msckf_stereo_c_amd/csrc/hip/fe_mask.h"

extern "C" {
int fm_max_margin(void) { return FM_MAX_MARGIN; }
int fm_words_per_row(int w) { return fm_pitch_words(w); }

// src (rows `pitch` bytes apart) -> the eroded usable plane (w * h bytes of 0 / 1), its bit plane, and the bit plane unpacked
// again (0 / 255)
int fm_run(const uint8_t *src, long long pitch, int w, int h, int margin, uint8_t *usable, uint32_t *words, uint8_t *unpacked) {
    if (!src || !usable || !words || !unpacked || w <= 0 || h <= 0 || pitch < w || margin < 0 || margin > FM_MAX_MARGIN) return -1;
    fm_erode(src, (size_t)pitch, w, h, margin, usable);
    fm_pack(usable, w, h, words);
    fm_unpack(words, w, h, unpacked);
    return 0;
}

int fm_pixel_of(float v) { return fm_pixel(v); }
int fm_lookup(const uint32_t *words, int w, int h, int x, int y) { return fm_usable(words, fm_pitch_words(w), w, h, x, y) ? 1 : 0; }

// the gate over n points, in place as k_mask_points applies it; mask0 / mask1 may be null
void fm_gate_points(const uint32_t *mask0, const uint32_t *mask1, int w, int h, int n, const float *out0, float *out1, float *und0, float *und1,
                    uint8_t *status) {
    for (int i = 0; i < n; ++i) {
        int what;
        const int ns = fm_gate(mask0, mask1, fm_pitch_words(w), w, h, out0[2 * i], out0[2 * i + 1], out1[2 * i], out1[2 * i + 1], status[i], &what);
        if (what == FM_LOST) { out1[2 * i] = out1[2 * i + 1] = und0[2 * i] = und0[2 * i + 1] = und1[2 * i] = und1[2 * i + 1] = 0.f; }
        status[i] = (uint8_t)ns;
    }
}

// sizeof(FeMaskDev) and the offsets of its fields, for the ctypes mirror of tests/test_gpu_mask.py
int fm_mask_dev_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(FeMaskDev), (int)offsetof(FeMaskDev, mask0), (int)offsetof(FeMaskDev, mask1), (int)offsetof(FeMaskDev, pitch_w)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
