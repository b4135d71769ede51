// fe_patch.hip — the point gate of the opt-in ZNCC patch check (fe_patch.h; DESIGN.md §3, "Patch check").
//
//  k_patch_points : behind a track launch of a batch that has a checking stream, over the same descriptors: a pure function of
//                   the track's outputs and the level-0 images.  Nothing of it runs unless a stream asked for the check.
#include <hip/hip_runtime.h>
#include "fe_device.h"
#include "fe_patch.h"

#define FP_ROW 16                      // lanes per point: one DPP row
#define FP_BLOCK 256
#define FP_PTS (FP_BLOCK / FP_ROW)     // points a block takes at a time

// the sums of the 16 lanes of a row, in every lane of it (xor butterfly inside the row: lanes of other rows take no part)
struct FpRowReduce {
    __device__ __forceinline__ void operator()(FpSums &s) const {
#pragma unroll
        for (int m = FP_ROW / 2; m > 0; m >>= 1) {
            s.a += (uint32_t)__shfl_xor((int)s.a, m, FP_ROW);
            s.b += (uint32_t)__shfl_xor((int)s.b, m, FP_ROW);
            s.aa += (uint32_t)__shfl_xor((int)s.aa, m, FP_ROW);
            s.bb += (uint32_t)__shfl_xor((int)s.bb, m, FP_ROW);
            s.ab += (uint32_t)__shfl_xor((int)s.ab, m, FP_ROW);
        }
    }
};

// Grid y = stream; a stream with mode 0 returns at once.  A 16-lane row per point, four points per wavefront: the lanes of a
// row take the samples j, j + 16, ... of both patches, the five sums are added up inside the row, every lane of it then holds
// them and decides alike, and lane 0 of the row writes.  Whatever a row branches on (its point's status, the verdict of its
// temporal comparison) is the same in its 16 lanes, so the lanes a shuffle reads from are always active with the reader.  The
// points of a stream are strided over the blocks of its grid row (the count may live on the device: n_pts_dev; the launch may be
// cut from an estimate below it).  No LDS.
__global__ __launch_bounds__(FP_BLOCK) void k_patch_points(const FeStreamDev *streams, const FePatchDev *patch) {
    const FePatchDev P = patch[blockIdx.y];
    if (P.mode == 0) return;
    const FeStreamDev &S = streams[blockIdx.y];
    const int n_pts = S.n_pts_dev ? *S.n_pts_dev : S.n_pts;
    const FpImage prev0{S.prev0.lvl[0], S.prev0.w[0], S.prev0.h[0]}, curr0{S.curr0.lvl[0], S.curr0.w[0], S.curr0.h[0]},
        curr1{S.curr1.lvl[0], S.curr1.w[0], S.curr1.h[0]};
    const int do_temporal = S.do_temporal;
    const int lane = threadIdx.x & (FP_ROW - 1);
    for (int pt = blockIdx.x * FP_PTS + threadIdx.x / FP_ROW; pt < n_pts; pt += gridDim.x * FP_PTS) {
        const int st = S.status[pt];
        if (!(st & 3)) continue;
        const mskf_point2f p0 = S.out0[pt], p1 = S.out1[pt];
        mskf_point2f pin = p0;
        if (do_temporal) pin = S.in_pts[pt];
        int what;
        const int ns = fp_gate_shared(P, prev0, curr0, curr1, do_temporal, pin.x, pin.y, p0.x, p0.y, p1.x, p1.y, st, lane, FP_ROW, FpRowReduce(), &what);
        if (lane == 0) {
            if (what == FP_LOST) {
                S.out1[pt] = mskf_point2f{0.f, 0.f}; S.und0[pt] = mskf_point2f{0.f, 0.f}; S.und1[pt] = mskf_point2f{0.f, 0.f};
            }
            if (ns != st) S.status[pt] = (uint8_t)ns;
        }
    }
}

// patch_dev[i] goes with streams_dev[i] (mode 0 = that stream is not checked)
extern "C" void fe_launch_patch_points(const FeStreamDev *streams_dev, const FePatchDev *patch_dev, int n_streams, int max_pts, hipStream_t st) {
    if (max_pts <= 0 || n_streams <= 0 || !patch_dev) return;
    hipLaunchKernelGGL(k_patch_points, dim3((max_pts + FP_PTS - 1) / FP_PTS, n_streams), dim3(FP_BLOCK), 0, st, streams_dev, patch_dev);
}
