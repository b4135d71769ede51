// fe_describe.hip — k_fe_describe: the opt-in 256-bit binary descriptors of points of level-0 images (fe_brief.h has the
// contract and every function of the arithmetic; DESIGN.md §3, "Descriptors").  Not part of a frame's chain: a launch of
// its own behind mskf_fe_describe_batch_begin, over the jobs of every describing stream of a batch.
//
// One wavefront per point, in one-wave workgroups (they back-fill free slots).  The lanes load the clamped
// 29 x 29 patch into LDS, a separable 5-tap pass leaves the 25 x 25 map of box sums (16 bits each), lane l evaluates the
// tests l, 64 + l, 128 + l and 192 + l, and four ballots are the four 64-bit words of the descriptor, written as bytes so
// that the output needs no alignment.  Integer arithmetic only, but for the float32 addition of the pixel rule.
#include <hip/hip_runtime.h>
#include "fe_brief.h"

static_assert(FB_TESTS == 4 * 64 && FB_BYTES == 32, "a lane evaluates four tests, a ballot is one 64-bit word of the descriptor");

__constant__ FbPattern c_fb_pattern = fb_make_pattern();

__global__ __launch_bounds__(64) void k_fe_describe(const FeDescribeDev *jobs) {
    const FeDescribeDev &J = jobs[blockIdx.y];
    const int n = J.n, lane = threadIdx.x;
    __shared__ uint8_t s_patch[FB_PATCH_N];
    __shared__ uint16_t s_hsum[FB_HSUM_N], s_box[FB_MAP_N];
    for (int pt = blockIdx.x; pt < n; pt += gridDim.x) {           // (uniform over the wavefront)
        const float x = J.pts[2 * (size_t)pt], y = J.pts[2 * (size_t)pt + 1];
        uint8_t *desc = J.desc + (size_t)FB_BYTES * pt;
        if (!fb_valid(x, y, J.w, J.h)) {
            if (lane < FB_BYTES) desc[lane] = 0;
            if (lane == 0) J.valid[pt] = 0;
            continue;
        }
        const int cx = fb_centre(x), cy = fb_centre(y);
        __syncthreads();                                            // the previous point's tests have read s_box
        for (int i = lane; i < FB_PATCH_N; i += 64) s_patch[i] = fb_patch_at(J.img, J.w, J.h, J.pitch, cx, cy, i);
        __syncthreads();
        for (int i = lane; i < FB_HSUM_N; i += 64) s_hsum[i] = fb_hsum_at(s_patch, i);
        __syncthreads();
        for (int i = lane; i < FB_MAP_N; i += 64) s_box[i] = fb_box_at(s_hsum, i);
        __syncthreads();
        unsigned long long word[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) word[k] = __ballot(fb_bit(s_box, c_fb_pattern.t, 64 * k + lane));
        if (lane < FB_BYTES) {
            const int k = lane >> 3;
            const unsigned long long v = k == 0 ? word[0] : (k == 1 ? word[1] : (k == 2 ? word[2] : word[3]));
            desc[lane] = (uint8_t)(v >> (8 * (lane & 7)));
        }
        if (lane == 0) J.valid[pt] = 1;
    }
}

// jobs_dev[0 .. n_jobs): jobs of any image size and point count (n = 0: skipped); max_pts = the largest count among them.
extern "C" void fe_launch_describe(const FeDescribeDev *jobs_dev, int n_jobs, int max_pts, hipStream_t st) {
    if (n_jobs <= 0 || max_pts <= 0) return;
    const int gx = max_pts < 65535 ? max_pts : 65535;
    for (int j0 = 0; j0 < n_jobs; j0 += 65535) {
        const int nj = n_jobs - j0 < 65535 ? n_jobs - j0 : 65535;
        hipLaunchKernelGGL(k_fe_describe, dim3(gx, nj), dim3(64), 0, st, jobs_dev + j0);
    }
}
