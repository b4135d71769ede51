// CPU harness of csrc/hip/fe_pixfmt.h (tests/test_pixel_format_reference.py): the header the kernel runs, compiled with g++
// into a shared library and driven through ctypes.
#include <cstddef>
#include <cstdint>
#include "msckf_stereo_c_amd/csrc/hip/fe_pixfmt.h"

extern "C" {
// the raw raster src (rows `pitch` bytes apart) -> the dense 8-bit plane dst
int px_run(int format, int shift, const uint8_t *src, long long pitch, uint8_t *dst, int w, int h) {
    if (px_bpp(format) == 0 || shift < 0 || shift > PX_MAX_SHIFT || pitch < (long long)w * px_bpp(format)) return -1;
    px_convert_image(src, (size_t)pitch, dst, w, h, format, shift);
    return 0;
}
int px_bytes_per_pixel(int format) { return px_bpp(format); }
int px_luma_of(int r, int g, int b) { return px_luma(r, g, b); }
int px_gray16_of(int v, int shift) { return px_gray16(v, shift); }
int px_reflect_of(int i, int n) { return px_reflect(i, n); }
// sizeof(PxJob) and the offset of every field in declaration order, for the ctypes mirror of the GPU tests; returns the count
int px_job_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(PxJob), (int)offsetof(PxJob, src), (int)offsetof(PxJob, dst), (int)offsetof(PxJob, pitch),
                     (int)offsetof(PxJob, w), (int)offsetof(PxJob, h), (int)offsetof(PxJob, format), (int)offsetof(PxJob, shift)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
