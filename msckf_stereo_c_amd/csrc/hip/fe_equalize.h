// fe_equalize.h — the arithmetic of the opt-in equalisation of pushed level-0 images ("Equalisation"): global
// histogram equalisation (mode 1) and CLAHE (mode 2).  ONE source: the kernels of fe_kernels.hip (k_eq_hist, k_eq_lut,
// k_eq_apply) and the g++-compiled CPU harness (tests/cpp/fe_equalize_test.cpp) both run these functions, the setter of the
// C ABI takes its geometry and its clip from them.  Histograms are integer counts (their accumulation order cannot matter);
// every float operation is a single IEEE-754 operation in the order written: compile with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EQ_FN __host__ __device__ __forceinline__
#else
#define EQ_FN inline
#endif

enum { EQ_OFF = 0, EQ_GLOBAL = 1, EQ_CLAHE = 2 };

// round to nearest even, then clamp to 0 .. 255
EQ_FN int eq_sat8(float x) {
    const int v = (int)rintf(x);
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---- tile geometry of CLAHE.  An image whose size the tile counts do not divide is extended on the right and at the bottom
// (virtually: a read with a reflected index) by tiles_x - w % tiles_x columns and tiles_y - h % tiles_y rows: a whole
// tiles_x / tiles_y when only the OTHER dimension is ragged.
struct EqGeom { int w, h, tiles_x, tiles_y, tw, th; };
EQ_FN EqGeom eq_geometry(int w, int h, int tiles_x, int tiles_y) {
    EqGeom g;
    g.w = w; g.h = h; g.tiles_x = tiles_x; g.tiles_y = tiles_y;
    int ew = w, eh = h;
    if (w % tiles_x != 0 || h % tiles_y != 0) { ew = w + (tiles_x - w % tiles_x); eh = h + (tiles_y - h % tiles_y); }
    g.tw = ew / tiles_x; g.th = eh / tiles_y;
    return g;
}
// column c >= 0 of the extended image -> column of the image: BORDER_REFLECT_101 (folded again while it is outside)
EQ_FN int eq_src_col(int c, int w) {
    if (w == 1) return 0;
    while (c < 0 || c >= w) c = c < 0 ? -c : 2 * (w - 1) - c;
    return c;
}
// row r >= 0 of the extended image -> row of the image: REFLECT_101 while r <= 2 h - 2, folded again beyond
EQ_FN int eq_src_row(int r, int h) {
    if (r < h) return r;
    if (h == 1) return 0;
    return (h - 1) - ((r - (h - 1)) % (h - 1));
}

// ---- CLAHE: the LUT of a tile from its histogram
// the clip of a tile of T pixels (0: no clip).  A bin never holds more than T, so a clip above T is T.
EQ_FN int eq_clip(double clip_limit, int T) {
    if (!(clip_limit > 0.0)) return 0;
    const double c = clip_limit * (double)T / 256.0;
    if (c >= (double)T) return T;
    const int ci = (int)c;
    return ci > 1 ? ci : 1;
}
EQ_FN int eq_excess(int count, int clip) { return clip > 0 && count > clip ? count - clip : 0; }
// bin i after the clip and the redistribution of `clipped` = sum of eq_excess over the bins: every bin gets clipped / 256,
// the residual goes one each to the bins 0, step, 2 step, ... (closed form of the serial walk: bin k step is reached while
// k < residual, and k step < 256 holds for all of them)
EQ_FN int eq_redistributed(int count, int i, int clip, int clipped) {
    if (clip <= 0) return count;
    int v = (count > clip ? clip : count) + clipped / 256;
    const int residual = clipped % 256;
    if (residual != 0) {
        const int step = 256 / residual > 1 ? 256 / residual : 1;
        if (i % step == 0 && i / step < residual) v += 1;
    }
    return v;
}
EQ_FN float eq_clahe_scale(int T) { return 255.f / (float)T; }
EQ_FN int eq_clahe_entry(int cum_inclusive, float lut_scale) { return eq_sat8((float)cum_inclusive * lut_scale); }

// ---- global mode: the LUT from the histogram of the whole image (total = w h pixels).  i0: first non-empty bin,
// n0 = hist[i0]; cum_inclusive = hist[0] + .. + hist[i] (the bins below i0 are empty, so the running sum that starts behind
// i0 is cum_inclusive - n0).  n0 == total: the image has one level and stays as it is.
EQ_FN float eq_global_scale(int total, int n0) { return 255.f / (float)(total - n0); }
EQ_FN int eq_global_entry(int i, int i0, int n0, int cum_inclusive, int total) {
    if (n0 == total) return i;
    if (i <= i0) return 0;
    return eq_sat8((float)(cum_inclusive - n0) * eq_global_scale(total, n0));
}

// ---- CLAHE: one pixel from the LUTs of the four tiles around it
// position p (x or y) along an axis of tiles of size t (inv_t = 1.f / t): the two tiles and their weights; the weights are
// formed BEFORE the tile indices are clamped
struct EqAxis { int t1, t2; float a, a1; };
EQ_FN float eq_inv(int t) { return 1.f / (float)t; }
EQ_FN int eq_axis_t1(int p, float inv_t) { return (int)floorf((float)p * inv_t - 0.5f); }     // unclamped: -1 .. n_tiles - 1
EQ_FN EqAxis eq_axis(int p, float inv_t, int n_tiles) {
    EqAxis o;
    const float f = (float)p * inv_t - 0.5f;
    const int t1 = (int)floorf(f);
    o.a = f - (float)t1; o.a1 = 1.f - o.a;
    o.t1 = t1 < 0 ? 0 : t1;
    o.t2 = t1 + 1 > n_tiles - 1 ? n_tiles - 1 : t1 + 1;
    return o;
}
// first position p in [0, limit] whose unclamped first tile is >= k (k >= 0), found with the pixel's own formula so that a
// region boundary and the pixels on either side of it can never disagree
EQ_FN int eq_axis_first(int k, int t, float inv_t, int limit) {
    int p = ((2 * k + 1) * t) / 2 - 2;
    if (p < 0) p = 0;
    if (p > limit) p = limit;
    while (p > 0 && eq_axis_t1(p - 1, inv_t) >= k) --p;
    while (p < limit && eq_axis_t1(p, inv_t) < k) ++p;
    return p;
}
EQ_FN int eq_interp(int l11, int l12, int l21, int l22, float xa, float xa1, float ya, float ya1) {
    const float top = (float)l11 * xa1 + (float)l12 * xa;
    const float bot = (float)l21 * xa1 + (float)l22 * xa;
    return eq_sat8(top * ya1 + bot * ya);
}

// ---- one image of an equalising push: what the three kernels read (fe_kernels.hip).  Planes are dense (pitch = width);
// dst is 16-byte aligned and may be src (every pixel is read and written by one lane, and the LUTs are complete before the
// apply kernel starts).
struct EqJob {
    const uint8_t *src;
    uint8_t *dst;
    int *part;                   // mode 1: n_strips x 256 partial histograms (every entry written by k_eq_hist: never cleared)
    uint8_t *lut;                // mode 1: 256 bytes; mode 2: tiles_y x tiles_x x 256
    int w, h, mode;
    int tiles_x, tiles_y, tw, th, clip;      // mode 2: eq_geometry, eq_clip
    int strip_rows, n_strips;                // mode 1: the row strips k_eq_hist's workgroups own
    int _pad;
};
// rows of a strip of mode 1: at most EQ_MAX_STRIPS strips per image
#define EQ_MAX_STRIPS 32
EQ_FN int eq_strip_rows(int h) { return (h + EQ_MAX_STRIPS - 1) / EQ_MAX_STRIPS; }
// the apply kernel's regions: between the tile centres the four tiles around a pixel do not change
EQ_FN int eq_regions(int mode, int tiles_x, int tiles_y) { return mode == EQ_CLAHE ? (tiles_x + 1) * (tiles_y + 1) : 1; }

// ---- whole-image restatements in terms of the functions above (host only: the harness; the kernels run the same functions
// with the sums and scans spread over a workgroup)
#if !defined(__HIP_DEVICE_COMPILE__)
inline void eq_lut_clahe_tile(const int hist[256], int T, int clip, uint8_t lut[256]) {
    int clipped = 0;
    for (int i = 0; i < 256; ++i) clipped += eq_excess(hist[i], clip);
    const float sc = eq_clahe_scale(T);
    int cum = 0;
    for (int i = 0; i < 256; ++i) { cum += eq_redistributed(hist[i], i, clip, clipped); lut[i] = (uint8_t)eq_clahe_entry(cum, sc); }
}
inline void eq_image_global(const uint8_t *src, uint8_t *dst, int w, int h) {
    int hist[256] = {0};
    const int total = w * h;
    for (int p = 0; p < total; ++p) ++hist[src[p]];
    int i0 = 0;
    while (hist[i0] == 0) ++i0;
    uint8_t lut[256];
    int cum = 0;
    for (int i = 0; i < 256; ++i) { cum += hist[i]; lut[i] = (uint8_t)eq_global_entry(i, i0, hist[i0], cum, total); }
    for (int p = 0; p < total; ++p) dst[p] = lut[src[p]];
}
// luts: tiles_y * tiles_x * 256 bytes of scratch
inline void eq_image_clahe(const uint8_t *src, uint8_t *dst, int w, int h, int tiles_x, int tiles_y, double clip_limit, uint8_t *luts) {
    const EqGeom g = eq_geometry(w, h, tiles_x, tiles_y);
    const int T = g.tw * g.th, clip = eq_clip(clip_limit, T);
    for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx) {
            int hist[256] = {0};
            for (int r = ty * g.th; r < (ty + 1) * g.th; ++r)
                for (int c = tx * g.tw; c < (tx + 1) * g.tw; ++c) ++hist[src[(size_t)eq_src_row(r, h) * w + eq_src_col(c, w)]];
            eq_lut_clahe_tile(hist, T, clip, luts + 256 * (size_t)(ty * tiles_x + tx));
        }
    const float inv_tw = eq_inv(g.tw), inv_th = eq_inv(g.th);
    for (int y = 0; y < h; ++y) {
        const EqAxis ay = eq_axis(y, inv_th, tiles_y);
        for (int x = 0; x < w; ++x) {
            const EqAxis ax = eq_axis(x, inv_tw, tiles_x);
            const int v = src[(size_t)y * w + x];
            const uint8_t *r1 = luts + 256 * (size_t)(ay.t1 * tiles_x), *r2 = luts + 256 * (size_t)(ay.t2 * tiles_x);
            dst[(size_t)y * w + x] = (uint8_t)eq_interp(r1[256 * ax.t1 + v], r1[256 * ax.t2 + v], r2[256 * ax.t1 + v], r2[256 * ax.t2 + v], ax.a, ax.a1, ay.a, ay.a1);
        }
    }
}
#endif
