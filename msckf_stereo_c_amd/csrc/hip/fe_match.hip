// fe_match.hip — k_fe_match: the opt-in brute-force Hamming matcher of 256-bit descriptors (fe_match.h has the contract and
// every function of the arithmetic; DESIGN.md §3, "Descriptor matching").  Not part of a frame's chain: ONE launch behind
// mskf_fe_match_batch_begin, over the jobs of a batch, cross-checked or not.
//
// A workgroup of four wavefronts owns 64 queries of one job: lane l of EVERY wavefront holds query q0 + l in 8 VGPRs.  The
// scanned set comes through LDS in tiles of FM_TILE descriptors (8 KiB, loaded 16 bytes per thread), and wavefront w scans
// the entries 64 w .. 64 w + 63 of each tile: the address is the same in all lanes, so the reads are broadcasts, and a pair
// costs 8 XOR and 8 accumulating popcounts.  The four parts meet through LDS under the header's merge rule, in every
// wavefront alike, so that each lane knows its query's whole result.  The split is always on: a frame's 437 queries are
// seven workgroups, which alone would leave most of the device idle when a job stands alone.
// Cross-check needs bwd(nearest(i)) only, and the workgroup has nearest(i) at hand: the same scan runs again with the
// train descriptor nearest(i) in the lane and the query set coming through LDS.  That costs nq instead of nt pairs per query,
// needs no second launch, no scratch memory and no atomics, and asks nothing of any other workgroup.
// Integer arithmetic only, but for the ratio test (fm_accept).
#include <hip/hip_runtime.h>
#include "fe_match.h"

#define FM_WAVES 4
static_assert(FM_TILE == 64 * FM_WAVES, "a wavefront scans 64 entries of a tile, a thread stages one validity byte");

struct __attribute__((packed)) FmMatchOut { mskf_match m; };      // the output needs no alignment

// the lane's 8 words from a 16-byte aligned descriptor
__device__ __forceinline__ void fm_load_own(const uint8_t *set, uint32_t index, uint32_t own[FM_WORDS]) {
    const uint4 *p = (const uint4 *)(set + (size_t)FM_BYTES * index);
    const uint4 a = p[0], b = p[1];
    own[0] = a.x; own[1] = a.y; own[2] = a.z; own[3] = a.w; own[4] = b.x; own[5] = b.y; own[6] = b.z; own[7] = b.w;
}

// own (where `active`) against set[0 .. n): the whole result, in every wavefront.  Called by all threads of the workgroup.
__device__ __forceinline__ FmPart fm_scan(const uint32_t own[FM_WORDS], bool active, const uint8_t *__restrict__ set, const uint8_t *__restrict__ valid, int n,
                                          uint4 *s_desc, uint8_t *s_valid, FmPart (*s_part)[64]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    FmPart p = fm_part_none();
    for (int t0 = 0; t0 < n; t0 += FM_TILE) {
        __syncthreads();                                            // the previous tile has been read
        const int m = n - t0 < FM_TILE ? n - t0 : FM_TILE;          // entries of this tile
        const uint4 *src = (const uint4 *)(set + (size_t)FM_BYTES * t0);
        for (int k = tid; k < 2 * m; k += 64 * FM_WAVES) s_desc[k] = src[k];
        s_valid[tid] = tid < m && (!valid || valid[t0 + tid]) ? 1 : 0;
        __syncthreads();
        for (int e = 64 * wave; e < 64 * wave + 64; ++e) {          // (uniform over the wavefront)
            if (!s_valid[e]) continue;
            const uint4 a = s_desc[2 * e], b = s_desc[2 * e + 1];
            const uint32_t t[FM_WORDS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            p = fm_insert(p, fm_distance(own, t), (uint32_t)(t0 + e));
        }
    }
    if (!active) p = fm_part_none();
    __syncthreads();                                                // the previous scan's parts have been read
    s_part[wave][lane] = p;
    __syncthreads();
    FmPart r = s_part[0][lane];
#pragma unroll
    for (int w = 1; w < FM_WAVES; ++w) r = fm_merge(r, s_part[w][lane]);
    return r;
}

__global__ __launch_bounds__(64 * FM_WAVES) void k_fe_match(const FeMatchDev *jobs) {
    const FeMatchDev J = jobs[blockIdx.y];
    const int nq = J.nq, nt = J.nt, lane = threadIdx.x & 63;
    __shared__ uint4 s_desc[2 * FM_TILE];
    __shared__ uint8_t s_valid[FM_TILE];
    __shared__ FmPart s_part[FM_WAVES][64];
    for (int q0 = 64 * blockIdx.x; q0 < nq; q0 += 64 * gridDim.x) {                  // (uniform over the workgroup)
        const int i = q0 + lane;
        const bool valid = i < nq && (!J.query_valid || J.query_valid[i]);
        uint32_t own[FM_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (valid) fm_load_own(J.query, (uint32_t)i, own);
        const FmPart p = fm_scan(own, valid, J.train, J.train_valid, nt, s_desc, s_valid, s_part);
        bool ok = fm_accept(p, J.max_distance, J.ratio);
        if (J.cross_check && __syncthreads_or(ok)) {                                  // (uniform: every wavefront holds the same results)
            if (ok) fm_load_own(J.train, p.key & 0xFFFFu, own);
            const FmPart b = fm_scan(own, ok, J.query, J.query_valid, nq, s_desc, s_valid, s_part);
            ok = ok && (b.key & 0xFFFFu) == (uint32_t)i;
        }
        if (i < nq && threadIdx.x < 64) { FmMatchOut o; o.m = fm_result(p, ok); ((FmMatchOut *)J.matches)[i] = o; }
    }
}

// jobs_dev[0 .. n_jobs): jobs of any size and count (nq = 0: skipped); max_nq = the largest query count among them, max_nt
// the largest train count (a launch is needed with max_nt = 0 too: its queries get "no neighbour").
extern "C" void fe_launch_match(const FeMatchDev *jobs_dev, int n_jobs, int max_nq, int max_nt, hipStream_t st) {
    (void)max_nt;
    if (n_jobs <= 0 || max_nq <= 0) return;
    const int gx = (max_nq + 63) / 64;
    for (int j0 = 0; j0 < n_jobs; j0 += 65535) {
        const int nj = n_jobs - j0 < 65535 ? n_jobs - j0 : 65535;
        hipLaunchKernelGGL(k_fe_match, dim3(gx, nj), dim3(64 * FM_WAVES), 0, st, jobs_dev + j0);
    }
}
