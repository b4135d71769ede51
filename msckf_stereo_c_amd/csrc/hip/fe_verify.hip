// fe_verify.hip — k_fe_verify: the hypotheses x pairs part of the opt-in stereo RANSAC pose check (fe_verify.h has the contract
// and every function of the arithmetic; DESIGN.md §3, "Geometric verification").  Not part of a frame's chain: ONE launch behind
// mskf_fe_verify_batch_begin, over the jobs of a batch.
//
// A workgroup of four wavefronts owns 64 hypotheses of one job: lane l of EVERY wavefront forms hypothesis 64 blockIdx.x + l
// (fv_draw + fv_fit3 on three staged pairs read from global memory) and holds its R, t in 24 VGPRs.  The usable pairs come
// through LDS in tiles of FV_TILE pairs of 7 doubles (14 KiB), and wavefront w scans the entries 64 w .. 64 w + 63 of each tile:
// the address is the same in all lanes, so the reads are broadcasts.  The camera, the threshold and the job record are the same
// for the whole workgroup and live in scalar registers.  The four counts of a hypothesis meet by integer addition through LDS,
// the 64 keys reduce by fv_merge (a maximum) across the lanes of wavefront 0, and lane 0 writes the workgroup's one key.  No
// atomics, no second launch, nothing but 64-bit keys goes back; integer counts and a maximum cannot depend on the order in
// which the parts meet.
#include <hip/hip_runtime.h>
#include "fe_verify.h"

#define FV_WAVES 4
static_assert(FV_TILE == 64 * FV_WAVES, "a wavefront scans 64 entries of a tile");
static_assert(FV_HYP_BLOCK == 64, "a hypothesis per lane");

__global__ __launch_bounds__(64 * FV_WAVES) void k_fe_verify(const FeVerifyDev *jobs) {
    const FeVerifyDev &J = jobs[blockIdx.y];
    const int n = J.n, K = J.K;
    if (64 * (int)blockIdx.x >= K) return;                                  // (uniform) the launch is cut for the batch's largest K
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    __shared__ double s_pair[FV_PAIR * FV_TILE];
    __shared__ uint32_t s_count[FV_WAVES][64];
    const FvCam cam = J.cam;
    const double max_error2 = J.max_error2, min_depth = J.min_depth;
    const double *__restrict__ pairs = J.pairs;
    const uint32_t h = 64u * blockIdx.x + (uint32_t)lane;
    double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0};          // (a dead lane's p0z = 0 < min_depth: it counts nothing)
    bool live = n >= 3 && h < (uint32_t)K;
    if (live) live = fv_hypothesis(cam, pairs, (uint32_t)n, J.seed, h, R, t);
    uint32_t count = 0;
    for (int t0 = 0; t0 < n; t0 += FV_TILE) {
        __syncthreads();                                                    // the previous tile has been read
        const int m = n - t0 < FV_TILE ? n - t0 : FV_TILE;                  // entries of this tile
        const double *src = pairs + (size_t)FV_PAIR * t0;
        for (int k = tid; k < FV_PAIR * m; k += 64 * FV_WAVES) s_pair[k] = src[k];
        __syncthreads();
        const int e1 = 64 * wave + 64 < m ? 64 * wave + 64 : m;
        for (int e = 64 * wave; e < e1; ++e)                                // (uniform over the wavefront)
            count += fv_inlier(cam, R, t, &s_pair[FV_PAIR * e], min_depth, max_error2) ? 1u : 0u;
    }
    s_count[wave][lane] = count;
    __syncthreads();
    if (wave != 0) return;
    uint32_t total = s_count[0][lane];
#pragma unroll
    for (int w = 1; w < FV_WAVES; ++w) total += s_count[w][lane];
    unsigned long long key = live ? fv_key(total, h) : FV_KEY_NONE;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) key = fv_merge(key, __shfl_xor(key, d, 64));
    if (lane == 0) J.keys[blockIdx.x] = key;
}

// jobs_dev[0 .. n_jobs): jobs of any n and K (K <= FV_MAX_K); max_K = the largest K among them.  Job j gets ceil(K_j / 64) keys.
extern "C" void fe_launch_verify(const FeVerifyDev *jobs_dev, int n_jobs, int max_K, hipStream_t st) {
    if (n_jobs <= 0 || max_K <= 0) return;
    const int gx = (max_K + FV_HYP_BLOCK - 1) / FV_HYP_BLOCK;
    for (int j0 = 0; j0 < n_jobs; j0 += 65535) {
        const int nj = n_jobs - j0 < 65535 ? n_jobs - j0 : 65535;
        hipLaunchKernelGGL(k_fe_verify, dim3(gx, nj), dim3(64 * FV_WAVES), 0, st, jobs_dev + j0);
    }
}
