// fe_pixfmt.h — the arithmetic of the input pixel formats of a stream ("Input pixel formats"): 16-bit grey,
// interleaved colour and 8-bit Bayer mosaics become the 8-bit grey level 0 of the stream on the device, inside the push.
// ONE source: the kernel of fe_kernels.hip (k_px_convert) and the g++-compiled CPU harness (tests/cpp/fe_pixfmt_test.cpp)
// both run these functions, the setter of the C ABI takes its format table from them.  Everything is integer arithmetic.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PX_FN __host__ __device__ __forceinline__
#else
#define PX_FN inline
#endif

// the values of mskf_fe_input_format.format (include/mskf_hip.h: MSKF_PIX_*).  A Bayer name spells the 2 x 2 tile at the
// image's top-left corner in reading order (row 0: x = 0, 1; row 1: x = 0, 1); this is not OpenCV's naming.
enum {
    PX_GRAY8 = 0, PX_GRAY16 = 1, PX_RGB8 = 2, PX_BGR8 = 3, PX_RGBA8 = 4, PX_BGRA8 = 5,
    PX_BAYER_RGGB8 = 6, PX_BAYER_GRBG8 = 7, PX_BAYER_GBRG8 = 8, PX_BAYER_BGGR8 = 9, PX_FORMATS = 10
};
#define PX_MAX_SHIFT 8

// bytes per pixel of the raw raster; 0: no such format
PX_FN int px_bpp(int format) {
    switch (format) {
        case PX_GRAY8: case PX_BAYER_RGGB8: case PX_BAYER_GRBG8: case PX_BAYER_GBRG8: case PX_BAYER_BGGR8: return 1;
        case PX_GRAY16: return 2;
        case PX_RGB8: case PX_BGR8: return 3;
        case PX_RGBA8: case PX_BGRA8: return 4;
        default: return 0;
    }
}
PX_FN bool px_is_bayer(int format) { return format >= PX_BAYER_RGGB8 && format <= PX_BAYER_BGGR8; }

// 16-bit grey: shift down, saturate
PX_FN int px_gray16(int v, int shift) {
    const int g = v >> shift;
    return g > 255 ? 255 : g;
}
// luma of 8-bit colour: 15-bit BT.601 weights (they sum to 32768: r = g = b = v gives v)
PX_FN int px_luma(int r, int g, int b) { return (9798 * r + 19235 * g + 3735 * b + 16384) >> 15; }

// REFLECT_101 of an index one step outside 0 .. n - 1 (-1 -> 1, n -> n - 2; n >= 2): the parity of the index, and with it
// the colour of the mosaic site, is kept
PX_FN int px_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// ---- Bayer.  The site classes of a mosaic: the colour the site samples, and for a green site the colour of its row
enum { PX_SITE_R = 0, PX_SITE_G_IN_R_ROW = 1, PX_SITE_G_IN_B_ROW = 2, PX_SITE_B = 3 };
PX_FN int px_bayer_site(int format, int x, int y) {
    // the red site of the 2 x 2 tile: RGGB (0, 0), GRBG (1, 0), GBRG (0, 1), BGGR (1, 1); blue sits diagonally opposite
    const int k = format - PX_BAYER_RGGB8, rx = k & 1, ry = k >> 1;
    const bool red_col = (x & 1) == rx, red_row = (y & 1) == ry;
    if (red_row) return red_col ? PX_SITE_R : PX_SITE_G_IN_R_ROW;
    return red_col ? PX_SITE_G_IN_B_ROW : PX_SITE_B;
}
// bilinear demosaic of one site from its 3 x 3 neighbourhood (c: the site; l r u d: the 4-neighbours; ul ur dl dr: the
// diagonal ones), then the luma
PX_FN int px_bayer_luma(int site, int c, int l, int r, int u, int d, int ul, int ur, int dl, int dr) {
    const int cross = (l + r + u + d + 2) >> 2, diag = (ul + ur + dl + dr + 2) >> 2;
    const int hor = (l + r + 1) >> 1, ver = (u + d + 1) >> 1;
    int R, G, B;
    if (site == PX_SITE_R) { R = c; G = cross; B = diag; }
    else if (site == PX_SITE_B) { B = c; G = cross; R = diag; }
    else if (site == PX_SITE_G_IN_R_ROW) { G = c; R = hor; B = ver; }
    else { G = c; B = hor; R = ver; }
    return px_luma(R, G, B);
}

// ---- one pixel of the converted image from the raw raster (rows `pitch` bytes apart), any format: what the kernel runs
// for row ends, border chunks of a mosaic and unaligned planes, and what the harness runs for every pixel
PX_FN int px_pixel(const uint8_t *src, size_t pitch, int w, int h, int format, int shift, int x, int y) {
    const uint8_t *row = src + (size_t)y * pitch;
    switch (format) {
        case PX_GRAY16: return px_gray16((int)row[2 * x] | ((int)row[2 * x + 1] << 8), shift);
        case PX_RGB8: return px_luma(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
        case PX_BGR8: return px_luma(row[3 * x + 2], row[3 * x + 1], row[3 * x]);
        case PX_RGBA8: return px_luma(row[4 * x], row[4 * x + 1], row[4 * x + 2]);
        case PX_BGRA8: return px_luma(row[4 * x + 2], row[4 * x + 1], row[4 * x]);
        case PX_BAYER_RGGB8: case PX_BAYER_GRBG8: case PX_BAYER_GBRG8: case PX_BAYER_BGGR8: {
            const int xl = px_reflect(x - 1, w), xr = px_reflect(x + 1, w);
            const uint8_t *ru = src + (size_t)px_reflect(y - 1, h) * pitch, *rd = src + (size_t)px_reflect(y + 1, h) * pitch;
            return px_bayer_luma(px_bayer_site(format, x, y), row[x], row[xl], row[xr], ru[x], rd[x], ru[xl], ru[xr], rd[xl], rd[xr]);
        }
        default: return row[x];
    }
}

// ---- one image of a converting push: what k_px_convert reads (fe_kernels.hip).  src: the raw raster, rows `pitch` bytes
// apart (pitch >= w * px_bpp(format)); dst: the dense 8-bit plane (pitch = w).  The kernel reads no byte outside
// [src, src + (h - 1) * pitch + w * bpp) and writes none outside [dst, dst + w * h).
struct PxJob {
    const uint8_t *src;
    uint8_t *dst;
    long long pitch;
    int w, h, format, shift;
};

// ---- whole image (host only: the harness)
#if !defined(__HIP_DEVICE_COMPILE__)
inline void px_convert_image(const uint8_t *src, size_t pitch, uint8_t *dst, int w, int h, int format, int shift) {
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) dst[(size_t)y * w + x] = (uint8_t)px_pixel(src, pitch, w, h, format, shift, x, y);
}
#endif
