// fe_mask.h — the opt-in per-camera image masks of a stream ("Image masks"): which pixels of cam0 / cam1 are
// scene.  ONE source: the kernels of fe_kernels.hip (k_detect_cells<true>, k_mask_points), the setter and getter of the C ABI
// and the g++-compiled CPU harness (tests/cpp/fe_mask_test.cpp) all run these functions.  Everything is integer arithmetic
// but the pixel rule, which is one float32 addition.
//   input     an 8-bit plane with a pitch, level-0 size: a pixel != 0 is usable, 0 is masked out;
//   margin    0 .. FM_MAX_MARGIN: a pixel stays usable iff every pixel OF THE IMAGE within Chebyshev distance `margin` is
//             non-zero in the input (pixels outside the image count as usable: the border of the image masks nothing);
//   plane     what the device holds, one per camera: 32-bit words, row pitch (W + 31) / 32 words, pixel x of row y is bit
//             x & 31 of word x >> 5, set = usable, the padding bits of a row's last word are 0.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__)
#define FM_FN __host__ __device__ __forceinline__
#else
#define FM_FN inline
#endif

#define FM_MAX_MARGIN 64

// What the mask kernels read of a stream beside its FeStreamDev: element i of a second array goes with descriptor i of the
// launch.  A null plane = that camera is not masked.
struct FeMaskDev {
    const uint32_t *mask0, *mask1;     // bit planes of cam0 / cam1
    int pitch_w;                       // words per row of either
    int pad_;
};

FM_FN int fm_pitch_words(int w) { return (w + 31) / 32; }

// the bit of pixel (x, y) of a plane; a pixel outside the image is usable, as for the erosion
FM_FN bool fm_usable(const uint32_t *plane, int pitch_w, int w, int h, int x, int y) {
    if (x < 0 || y < 0 || x >= w || y >= h) return true;
    return (plane[(size_t)y * pitch_w + (x >> 5)] >> (x & 31)) & 1u;
}

// the pixel a point lies in: float32 addition, then truncation
FM_FN int fm_pixel(float v) { return (int)(v + 0.5f); }

// The point gate, for one point of a track call.  status: bit 0 = the temporal half survived, bit 1 = stereo inlier.
// Returns the new status; FM_LOST in *what when the point is lost the way k_track4 loses one (the caller then zeroes out1,
// und0 and und1 and keeps out0).  A null plane masks nothing.
enum { FM_KEEP = 0, FM_LOST = 1 };
FM_FN int fm_gate(const uint32_t *mask0, const uint32_t *mask1, int pitch_w, int w, int h, float x0, float y0, float x1, float y1, int status,
                  int *what) {
    *what = FM_KEEP;
    if ((status & 1) && mask0 && !fm_usable(mask0, pitch_w, w, h, fm_pixel(x0), fm_pixel(y0))) { *what = FM_LOST; return 0; }
    if ((status & 2) && mask1 && !fm_usable(mask1, pitch_w, w, h, fm_pixel(x1), fm_pixel(y1))) return status & ~2;
    return status;
}

// ---- whole planes (host functions: the setter, the getter and the harness)

// dst[y * w + x] = 1 where the pixel stays usable, else 0.  Two passes of running counts: the zeros of the input in the row
// window x - margin .. x + margin, then the rows with a zero in their window in the column window y - margin .. y + margin
// (both windows cut at the image).
inline void fm_erode(const uint8_t *src, size_t pitch, int w, int h, int margin, uint8_t *dst) {
    std::vector<uint8_t> hor((size_t)w * h);
    std::vector<int> pre((size_t)(w > h ? w : h) + 1);
    for (int y = 0; y < h; ++y) {
        const uint8_t *row = src + (size_t)y * pitch;
        pre[0] = 0;
        for (int x = 0; x < w; ++x) pre[x + 1] = pre[x] + (row[x] == 0 ? 1 : 0);
        for (int x = 0; x < w; ++x) {
            const int a = x - margin < 0 ? 0 : x - margin, b = x + margin >= w ? w - 1 : x + margin;
            hor[(size_t)y * w + x] = pre[b + 1] - pre[a] == 0 ? 1 : 0;
        }
    }
    for (int x = 0; x < w; ++x) {
        pre[0] = 0;
        for (int y = 0; y < h; ++y) pre[y + 1] = pre[y] + (hor[(size_t)y * w + x] == 0 ? 1 : 0);
        for (int y = 0; y < h; ++y) {
            const int a = y - margin < 0 ? 0 : y - margin, b = y + margin >= h ? h - 1 : y + margin;
            dst[(size_t)y * w + x] = pre[b + 1] - pre[a] == 0 ? 1 : 0;
        }
    }
}

// the bit plane of a dense 0 / non-zero plane; `words` holds h * fm_pitch_words(w) words
inline void fm_pack(const uint8_t *usable, int w, int h, uint32_t *words) {
    const int pw = fm_pitch_words(w);
    for (int y = 0; y < h; ++y)
        for (int k = 0; k < pw; ++k) {
            uint32_t v = 0;
            for (int b = 0; b < 32 && 32 * k + b < w; ++b) v |= (usable[(size_t)y * w + 32 * k + b] ? 1u : 0u) << b;
            words[(size_t)y * pw + k] = v;
        }
}

// ... and back: 0 / 255 per pixel
inline void fm_unpack(const uint32_t *words, int w, int h, uint8_t *out) {
    const int pw = fm_pitch_words(w);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) out[(size_t)y * w + x] = fm_usable(words, pw, w, h, x, y) ? 255 : 0;
}
