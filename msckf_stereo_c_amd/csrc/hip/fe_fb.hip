// fe_fb.hip — the point gate of the opt-in forward-backward check (fe_fb.h; DESIGN.md §3, "Forward-backward check").
//
//  k_fb_points : behind a track launch of a batch that has a checking stream, over the same descriptors, after the mask and
//                the patch gate: a pure function of the track's outputs and the resident pyramids.  It runs l4_track (fe_lk.h),
//                the function k_track4 runs, with the pyramids' roles swapped.  Nothing of it runs unless a stream asked for it.
#include <hip/hip_runtime.h>
#include "fe_device.h"
#include "fe_lk.h"
#include "fe_fb.h"

// Shaped like k_track4: a one-wave workgroup, four points per wavefront, a 16-lane row per point, the same LDS staging and the
// same block -> (stream, point group) mapping (the point groups of one stream get block ids that are congruent modulo 8, so its
// pyramids travel through one L2); a block walks several point groups when the grid was cut from an estimate of a count that
// lives on the device.  A stream with mode 0 returns at once.  The two backward tracks run through ONE copy of the LK code (a
// two-trip loop):
//   trip 0, temporal (mode bit 1, calls with do_temporal, points with status bit 0): template at out0 in curr0, searched in
//           prev0 from in_pts, compared with in_pts.  A failing point is lost as k_track4 loses one.
//   trip 1, stereo (mode bit 2, points that still have status bit 1): template at out1 in curr1, searched in curr0 from out0,
//           compared with out0.  A failing point loses bit 1.
// `alive` = this row's point needs this trip's comparison; a trip no row of the wave needs is skipped, and only the results of
// alive rows are used.  Whatever the wave branches on around l4_track (which holds workgroup barriers) is uniform in the wave.
// Lane 0 of a row writes, and only what changes.
// The body is written once: k_fb_points is the DEEP = false instantiation; k_fb_points_deep (opt-in deeper LK pyramids, fe_deep.h)
// runs behind k_track4_deep, so that a backward track has its forward track's depth.  Each kernel owns its staging, as the track
// kernels do.
template <bool DEEP>
__device__ __forceinline__ void fb_body(const FeStreamDev *streams, const FeFbDev *fb, const FeDeepDev *deeps, int n_streams, int groups_per_stream,
                                        uint32_t (*s_T)[L4_TROWS * L4_DW + 2], uint32_t (*s_S)[L4_SROWS * L4_DW + 4]) {
    const int x = blockIdx.x & 7, qb = blockIdx.x >> 3;
    const int si = x + 8 * (qb / groups_per_stream), gi = qb - (qb / groups_per_stream) * groups_per_stream;
    if (si >= n_streams) return;
    const FeFbDev F = fb[si];
    if (F.mode == 0) return;
    const FeStreamDev &S = streams[si];
    const int n_pts = S.n_pts_dev ? *S.n_pts_dev : S.n_pts;
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    uint32_t *sT = s_T[g], *sS = s_S[g];
    const bool temporal = (F.mode & FB_TEMPORAL) && S.do_temporal, stereo = (F.mode & FB_STEREO) != 0;
#pragma nounroll
    for (int gq = gi; 4 * gq < n_pts; gq += groups_per_stream) {
        const int pt = 4 * gq + g;
        const bool in_range = pt < n_pts;
        int st = 0;
        mskf_point2f p0 = {0.f, 0.f}, p1 = {0.f, 0.f}, pin = {0.f, 0.f};
        if (in_range) {
            st = S.status[pt];
            p0 = S.out0[pt]; p1 = S.out1[pt];
            if (temporal) pin = S.in_pts[pt];
        }
        int ns = st;
        bool lost = false;
#pragma nounroll
        for (int ph = temporal ? 0 : 1; ph < (stereo ? 2 : 1); ++ph) {
            // template point, and the origin: the initial guess of the backward track and what its result is compared with
            const float tx = ph ? p1.x : p0.x, ty = ph ? p1.y : p0.y, ox = ph ? p0.x : pin.x, oy = ph ? p0.y : pin.y;
            const bool alive = ph ? (ns & 2) != 0 : (st & 1) != 0;
            float bx = 0.f, by = 0.f;
            int bst = 0;
            unsigned int dbg_iters = 0;
            if (__any(alive)) {
                if (DEEP) {
                    const FeDeepDev &P = deeps[si];
                    l4_track<true>(ph ? S.curr1 : S.curr0, ph ? S.curr0 : S.prev0, alive, tx, ty, ox, oy, sT, sS, r, bx, by, bst, dbg_iters,
                                   ph ? &P.curr1 : &P.curr0, ph ? &P.curr0 : &P.prev0, P.levels);
                } else l4_track(ph ? S.curr1 : S.curr0, ph ? S.curr0 : S.prev0, alive, tx, ty, ox, oy, sT, sS, r, bx, by, bst, dbg_iters);
            }
            if (alive && !fb_pass(bx, by, ox, oy, bst, ph ? F.thr2_s : F.thr2_t)) {
                if (ph == 0) { ns = 0; lost = true; }
                else ns &= ~2;
            }
        }
        if (in_range && r == 0) {
            if (lost) {
                S.out1[pt] = mskf_point2f{0.f, 0.f}; S.und0[pt] = mskf_point2f{0.f, 0.f}; S.und1[pt] = mskf_point2f{0.f, 0.f};
            }
            if (ns != st) S.status[pt] = (uint8_t)ns;
        }
    }
}

__global__ __launch_bounds__(64) void k_fb_points(const FeStreamDev *streams, const FeFbDev *fb, int n_streams, int groups_per_stream) {
    __shared__ uint32_t s_T[4][L4_TROWS * L4_DW + 2];
    __shared__ uint32_t s_S[4][L4_SROWS * L4_DW + 4];
    fb_body<false>(streams, fb, nullptr, n_streams, groups_per_stream, s_T, s_S);
}
__global__ __launch_bounds__(64) void k_fb_points_deep(const FeStreamDev *streams, const FeFbDev *fb, const FeDeepDev *deeps, int n_streams, int groups_per_stream) {
    __shared__ uint32_t s_T[4][L4_TROWS * L4_DW + 2];
    __shared__ uint32_t s_S[4][L4_SROWS * L4_DW + 4];
    fb_body<true>(streams, fb, deeps, n_streams, groups_per_stream, s_T, s_S);
}

// fb_dev[i] goes with streams_dev[i] (mode 0 = that stream is not checked); the grid of fe_launch_track
extern "C" void fe_launch_fb_points(const FeStreamDev *streams_dev, const FeFbDev *fb_dev, int n_streams, int max_pts, hipStream_t st) {
    if (max_pts <= 0 || n_streams <= 0 || !fb_dev) return;
    const int gps = (max_pts + 3) / 4;
    hipLaunchKernelGGL(k_fb_points, dim3(8 * ((n_streams + 7) / 8) * gps), dim3(64), 0, st, streams_dev, fb_dev, n_streams, gps);
}
// the deep instantiation over the same grid: deep_dev[i] goes with streams_dev[i] too
extern "C" void fe_launch_fb_points_deep(const FeStreamDev *streams_dev, const FeFbDev *fb_dev, const FeDeepDev *deep_dev, int n_streams, int max_pts, hipStream_t st) {
    if (max_pts <= 0 || n_streams <= 0 || !fb_dev || !deep_dev) return;
    const int gps = (max_pts + 3) / 4;
    hipLaunchKernelGGL(k_fb_points_deep, dim3(8 * ((n_streams + 7) / 8) * gps), dim3(64), 0, st, streams_dev, fb_dev, deep_dev, n_streams, gps);
}
