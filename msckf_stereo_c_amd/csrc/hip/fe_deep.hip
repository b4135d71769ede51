// fe_deep.hip — the pyramid kernel of the opt-in deeper LK pyramids (fe_deep.h; DESIGN.md §3, "Deeper LK pyramids").
//
//  k_pyr_down_deep : behind k_pyr_down3 of a push that has a deep stream: the levels 4 .. L - 1 of every image of the deep
//                    streams in one launch.  Nothing of it runs unless a stream asked for more than four levels.
// The deep instantiations of the track kernels live beside the kernels they instantiate (k_track4_deep in fe_kernels.hip,
// k_fb_points_deep in fe_fb.hip): they are the same bodies over l4_track<true> (fe_lk.h).
#include <hip/hip_runtime.h>
#include "fe_device.h"
#include "fe_deep.h"

// One workgroup per image.  Level 4 of a 3840 x 2160 image is 240 x 135 and every further level a quarter of the one below,
// so an image is at most 43 000 output pixels: the workgroup builds the levels in sequence, a pixel per lane and sweep (the
// 25 taps of fd_pyr_down_px, reflect-101 at every level, so odd sides and a 15-pixel top level need no case of their own),
// with a workgroup barrier between two levels.  A level is written and then read by this workgroup alone: no atomics and
// nothing between workgroups.
__global__ __launch_bounds__(256) void k_pyr_down_deep(const DeepPyrJob *jobs) {
    const DeepPyrJob &J = jobs[blockIdx.x];
    const uint8_t *src = J.src;
    int W = J.w, H = J.h;
    const int levels = J.levels;
    for (int l = FD_BASE_LEVELS; l < levels; ++l) {
        const int w = fd_half(W), h = fd_half(H), n = w * h;
        uint8_t *dst = J.dst[l - FD_BASE_LEVELS];      // (read where it lies: a copy of the job in registers indexed by l would go to scratch)
        for (int i = (int)threadIdx.x; i < n; i += 256) {
            const int y = i / w, x = i - y * w;
            dst[i] = fd_pyr_down_px(src, W, H, x, y);
        }
        __syncthreads();      // (orders the workgroup's global stores before its loads of the next level)
        src = dst; W = w; H = h;
    }
}

extern "C" void fe_launch_pyr_down_deep(const DeepPyrJob *jobs_dev, int n_jobs, hipStream_t st) {
    if (n_jobs <= 0) return;
    hipLaunchKernelGGL(k_pyr_down_deep, dim3(n_jobs), dim3(256), 0, st, jobs_dev);
}
