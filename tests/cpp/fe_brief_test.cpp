// csrc/hip/fe_brief.h (the header k_fe_describe and the C ABI run) compiled for the host: a small shared library for
// tests/test_brief_reference.py, which compares it with the numpy restatement (tests/brief_reference.py).
#include <cstddef>
#include <cstring>
#include "msckf_stereo_c_amd/csrc/hip/fe_brief.h"

static constexpr FbPattern kPattern = fb_make_pattern();       // what mskf_fe_descriptor_pattern copies out

extern "C" {
// ax, ay, bx, by of the 256 tests; returns the number of draws the generator made
int fb_pattern(int8_t out[4 * FB_TESTS]) {
    std::memcpy(out, kPattern.t, sizeof(kPattern.t));
    return kPattern.draws;
}

int fb_valid_of(float x, float y, int w, int h) { return fb_valid(x, y, w, h) ? 1 : 0; }
int fb_centre_of(float v) { return fb_centre(v); }

// n points of one image (rows `pitch` bytes apart) -> 32 n descriptor bytes and n validity bytes
int fb_describe(const uint8_t *img, int w, int h, long long pitch, const float *pts, int n, uint8_t *desc, uint8_t *valid) {
    if (!img || w <= 0 || h <= 0 || pitch < w || n < 0 || (n && (!pts || !desc || !valid))) return -1;
    for (int i = 0; i < n; ++i) valid[i] = (uint8_t)fb_describe_point(img, w, h, pitch, pts[2 * i], pts[2 * i + 1], kPattern.t, desc + (size_t)FB_BYTES * i);
    return 0;
}

// sizeof(FeDescribeDev) and the offsets of its fields, for the ctypes mirror of tests/test_gpu_describe.py
int fb_describe_dev_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(FeDescribeDev), (int)offsetof(FeDescribeDev, img), (int)offsetof(FeDescribeDev, w), (int)offsetof(FeDescribeDev, h),
                     (int)offsetof(FeDescribeDev, pitch), (int)offsetof(FeDescribeDev, pts), (int)offsetof(FeDescribeDev, n),
                     (int)offsetof(FeDescribeDev, desc), (int)offsetof(FeDescribeDev, valid)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
