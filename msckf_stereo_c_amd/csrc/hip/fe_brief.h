// fe_brief.h — the opt-in 256-bit binary descriptors of points of a level-0 image ("Descriptors"): upright,
// single-scale BRIEF over 5 x 5 box sums.  ONE source: the kernel of fe_describe.hip, the C ABI (mskf_fe_descriptor_pattern) and
// the g++-compiled CPU harness (tests/cpp/fe_brief_test.cpp) all run these functions.  Everything is integer arithmetic but the
// pixel rule, which is one float32 addition per coordinate.
//   pattern   FB_TESTS tests (ax, ay, bx, by), every coordinate in -FB_REACH .. FB_REACH, generated (fb_make_pattern);
//   pixel     pix(x, y) = I[clamp(y, 0, H - 1)][clamp(x, 0, W - 1)]: the border is replicated;
//   box       S(qx, qy) = sum of pix over |dx|, |dy| <= FB_BOX (at most 25 * 255 = 6375: 16 bits);
//   centre    fx = x + 0.5f, fy = y + 0.5f; valid iff 0 <= fx < (float)W and 0 <= fy < (float)H (false for NaN); ((int)fx, (int)fy);
//   bit t     S(c + a_t) < S(c + b_t), strictly, in byte t >> 3, bit t & 7 of the point's FB_BYTES bytes; an invalid point
//             gets FB_BYTES zero bytes and valid = 0.
// A point is worked on in three maps around its centre c, each filled element by element by one of the functions below (the
// kernel strides the elements over a wavefront, the host runs them in a loop):
//   patch  FB_PATCH x FB_PATCH pixels,           patch[r][q] = pix(cx - FB_HALF + q, cy - FB_HALF + r)
//   hsum   FB_PATCH rows x FB_MAP columns,       hsum[r][q]  = patch[r][q] + .. + patch[r][q + 4]
//   box    FB_MAP x FB_MAP,                      box[r][q]   = hsum[r][q] + .. + hsum[r + 4][q]  = S(cx - FB_REACH + q, cy - FB_REACH + r)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FBR_FN __host__ __device__ __forceinline__
#else
#define FBR_FN inline
#endif

#define FB_TESTS 256
#define FB_BYTES 32
#define FB_REACH 12                                  // largest offset of a test
#define FB_BOX 2                                     // radius of the box
#define FB_HALF (FB_REACH + FB_BOX)                  // 14: the footprint reaches this far from the centre
#define FB_PATCH (2 * FB_HALF + 1)                   // 29
#define FB_MAP (2 * FB_REACH + 1)                    // 25
#define FB_PATCH_N (FB_PATCH * FB_PATCH)             // 841
#define FB_HSUM_N (FB_PATCH * FB_MAP)                // 725
#define FB_MAP_N (FB_MAP * FB_MAP)                   // 625

// One job of a k_fe_describe launch: n points of one level-0 image.  pts holds x, y pairs; desc takes FB_BYTES bytes per point,
// valid one.  Nothing needs an alignment beyond that of its type.
struct FeDescribeDev {
    const uint8_t *img;                // level 0, rows `pitch` bytes apart
    int w, h;
    long long pitch;
    const float *pts;                  // in: x0, y0, x1, y1, .. in level-0 pixels
    int n, pad_;
    uint8_t *desc, *valid;             // out
};

// ---- the sampling pattern: ax, ay, bx, by of test 0, 1, ..
struct FbPattern { int8_t t[4 * FB_TESTS]; int draws; };

constexpr uint64_t fb_splitmix(uint64_t k) {          // draw k = 1, 2, ..
    uint64_t z = 0xB21EFB21EFB21EF5ULL + 0x9E3779B97F4A7C15ULL * k;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
    z ^= z >> 27; z *= 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}
// a sum of three uniforms on 0 .. 8, centred: bell-shaped around the point
constexpr int fb_coord(uint64_t z) { return (int)(z % 9) + (int)((z >> 16) % 9) + (int)((z >> 32) % 9) - FB_REACH; }

constexpr FbPattern fb_make_pattern() {
    FbPattern p{};
    uint64_t k = 0;
    for (int t = 0; t < FB_TESTS;) {
        const int ax = fb_coord(fb_splitmix(k + 1)), ay = fb_coord(fb_splitmix(k + 2));
        const int bx = fb_coord(fb_splitmix(k + 3)), by = fb_coord(fb_splitmix(k + 4));
        k += 4;
        if (ax == bx && ay == by) continue;          // compares a sum with itself: drawn again
        p.t[4 * t] = (int8_t)ax; p.t[4 * t + 1] = (int8_t)ay; p.t[4 * t + 2] = (int8_t)bx; p.t[4 * t + 3] = (int8_t)by;
        ++t;
    }
    p.draws = (int)k;
    return p;
}

// ---- a point: validity and centre
FBR_FN bool fb_valid(float x, float y, int w, int h) {
    const float fx = x + 0.5f, fy = y + 0.5f;
    return fx >= 0.f && fx < (float)w && fy >= 0.f && fy < (float)h;
}
FBR_FN int fb_centre(float v) { return (int)(v + 0.5f); }          // (fm_pixel of fe_mask.h; asked of valid points only)

// ---- the three maps
FBR_FN int fb_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

FBR_FN uint8_t fb_patch_at(const uint8_t *img, int w, int h, long long pitch, int cx, int cy, int i) {
    const int r = i / FB_PATCH, q = i - r * FB_PATCH;
    return img[(long long)fb_clamp(cy - FB_HALF + r, h) * pitch + fb_clamp(cx - FB_HALF + q, w)];
}
FBR_FN uint16_t fb_hsum_at(const uint8_t *patch, int i) {
    const int r = i / FB_MAP, q = i - r * FB_MAP;
    const uint8_t *p = patch + r * FB_PATCH + q;
    int s = 0;
    for (int d = 0; d <= 2 * FB_BOX; ++d) s += p[d];
    return (uint16_t)s;
}
FBR_FN uint16_t fb_box_at(const uint16_t *hsum, int i) {
    int s = 0;
    for (int d = 0; d <= 2 * FB_BOX; ++d) s += hsum[i + d * FB_MAP];
    return (uint16_t)s;
}

// ---- bit t of the descriptor, from the box map of the point and the pattern
FBR_FN bool fb_bit(const uint16_t *box, const int8_t *pat, int t) {
    const int8_t *p = pat + 4 * t;
    const int a = (p[1] + FB_REACH) * FB_MAP + (p[0] + FB_REACH), b = (p[3] + FB_REACH) * FB_MAP + (p[2] + FB_REACH);
    return box[a] < box[b];
}

// ---- one point on the host (the harness; the kernel does the same with the map elements strided over its lanes).
// Returns valid.
inline int fb_describe_point(const uint8_t *img, int w, int h, long long pitch, float x, float y, const int8_t *pat, uint8_t desc[FB_BYTES]) {
    for (int i = 0; i < FB_BYTES; ++i) desc[i] = 0;
    if (!fb_valid(x, y, w, h)) return 0;
    const int cx = fb_centre(x), cy = fb_centre(y);
    uint8_t patch[FB_PATCH_N];
    uint16_t hsum[FB_HSUM_N], box[FB_MAP_N];
    for (int i = 0; i < FB_PATCH_N; ++i) patch[i] = fb_patch_at(img, w, h, pitch, cx, cy, i);
    for (int i = 0; i < FB_HSUM_N; ++i) hsum[i] = fb_hsum_at(patch, i);
    for (int i = 0; i < FB_MAP_N; ++i) box[i] = fb_box_at(hsum, i);
    for (int t = 0; t < FB_TESTS; ++t)
        if (fb_bit(box, pat, t)) desc[t >> 3] |= (uint8_t)(1u << (t & 7));
    return 1;
}
