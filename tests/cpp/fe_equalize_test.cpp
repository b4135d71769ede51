// CPU harness of csrc/hip/fe_equalize.h (tests/test_equalize_reference.py): the header the kernels run, compiled with g++
// into a shared library and driven through ctypes.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "msckf_stereo_c_amd/csrc/hip/fe_equalize.h"

extern "C" {
// mode 1: global, 2: CLAHE.  luts_out (may be null): tiles_y * tiles_x * 256 bytes, the per-tile LUTs of mode 2.
int eq_run(int mode, const uint8_t *src, uint8_t *dst, int w, int h, int tiles_x, int tiles_y, double clip_limit, uint8_t *luts_out) {
    if (mode == EQ_GLOBAL) { eq_image_global(src, dst, w, h); return 0; }
    if (mode != EQ_CLAHE) return -1;
    std::vector<uint8_t> own;
    if (!luts_out) { own.resize(256 * (size_t)tiles_x * tiles_y); luts_out = own.data(); }
    eq_image_clahe(src, dst, w, h, tiles_x, tiles_y, clip_limit, luts_out);
    return 0;
}
void eq_tile_size(int w, int h, int tiles_x, int tiles_y, int *tw, int *th) {
    const EqGeom g = eq_geometry(w, h, tiles_x, tiles_y);
    *tw = g.tw; *th = g.th;
}
int eq_row(int r, int h) { return eq_src_row(r, h); }
int eq_col(int c, int w) { return eq_src_col(c, w); }
// first position whose unclamped tile index reaches k: what the apply kernel cuts its regions with
int eq_first(int k, int t, int limit) { return eq_axis_first(k, t, eq_inv(t), limit); }
int eq_t1(int p, int t) { return eq_axis_t1(p, eq_inv(t)); }
// sizeof(EqJob) and the offset of every field in declaration order, for the ctypes mirror of the GPU tests; returns the count
int eq_job_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(EqJob), (int)offsetof(EqJob, src), (int)offsetof(EqJob, dst), (int)offsetof(EqJob, part), (int)offsetof(EqJob, lut),
                     (int)offsetof(EqJob, w), (int)offsetof(EqJob, h), (int)offsetof(EqJob, mode), (int)offsetof(EqJob, tiles_x),
                     (int)offsetof(EqJob, tiles_y), (int)offsetof(EqJob, tw), (int)offsetof(EqJob, th), (int)offsetof(EqJob, clip),
                     (int)offsetof(EqJob, strip_rows), (int)offsetof(EqJob, n_strips), (int)offsetof(EqJob, _pad)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
