// sizeof(FeStreamDev) and the offsets of its fields as csrc/hip/fe_device.h lays them out, for the ctypes mirror of
// tests/test_gpu_detector_edges.py (test_fe_stream_dev_layout_matches_the_header): host code, compiled into a shared library.
#include <cstddef>
#include "msckf_stereo_c_amd/csrc/hip/fe_device.h"

extern "C" {
// the size first, then every field in declaration order; returns the count
int fe_stream_dev_layout(int *out, int capacity) {
#define F(name) (int)offsetof(FeStreamDev, name)
    const int v[] = {(int)sizeof(FeStreamDev), F(prev0), F(curr0), F(curr1), F(cam0), F(cam1), F(R01), F(E), F(Hpred), F(epi_thresh), F(n_pts),
                     F(n_pts_dev), F(do_temporal), F(in_pts), F(out0), F(out1), F(und0), F(und1), F(status),
                     F(det_rows), F(det_cols), F(cell_w), F(cell_h), F(det_floor), F(cell_keys)};
#undef F
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
// the same of PyrDev: size, lvl, w, h
int pyr_dev_layout(int *out, int capacity) {
    const int v[] = {(int)sizeof(PyrDev), (int)offsetof(PyrDev, lvl), (int)offsetof(PyrDev, w), (int)offsetof(PyrDev, h)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}
}
