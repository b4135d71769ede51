// fe_kernels.hip — hand-written gfx950 kernels of the stereo KLT front-end.
//
//  k_pyr_down3    : cg::pyr_down x 3        (reference call sites image_processor.cpp:239,242): levels 1 .. 3 of an image in one launch
//  k_detect_cells : cg::CornerDetector      (:132,259,657) — per-cell integer Shi-Tomasi maximum (32x32 px tiles)
//  k_track4       : cg::optical_flow_multi_level (:410 temporal, :569 stereo) with the prediction (:321-350), the
//                   image-bounds gates (:416-424, :575-583), the stereo initial guess (:542-548), undistortion and
//                   the epipolar gate (:587-617): one launch per track call, four points per wavefront.
//  k_track4_ext   : — (opt-in camera models radtan8 / fov / ds, fe_cam_models.h): the second instantiation of k_track4's body,
//                   launched in its place for a batch in which a stream has an extended model.
//  k_track4_deep  : — (opt-in deeper LK pyramids, fe_deep.h): the third instantiation, launched for a batch in which a stream
//                   tracks over more than four levels; the extra levels come from k_pyr_down_deep (fe_deep.hip).
//  k_mask_points  : — (opt-in image masks, fe_mask.h): the point gate behind a track launch; k_detect_cells<true> is the
//                   detector of a push that has a masked stream.
//
// Arithmetic contract: every decision-bearing quantity is integer or a fixed
// sequence of IEEE-754 double operations; this file must be compiled with -ffp-contract=off.
// Work shapes: one 16-lane DPP row per tracked point (four points per wavefront, a lane owns one row of the 15x15
// window); the detector and the pyramid pass march 16-lane strips down segments of rows, four (strip, segment) jobs per
// one-wave workgroup, in registers and DPP only.  A launch covers every VIO stream of a context and fills the chip only
// when many streams are batched.
#include <stdlib.h>
#include <mutex>
#include "fe_device.h"
#include "fe_mask.h"

// ------------------------------------------------------------------------------------------ pyr_down
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) { i = (i < 0) ? -i : 2 * (n - 1) - i; }
    return i;
}

// ---- levels 1, 2 and 3 of one image in ONE launch, as a register / DPP row march (no LDS, no barrier, one-wave workgroups).
// Every level is the separable [1 4 6 4 1] / 256 filter with BORDER_REFLECT_101 of the level BELOW it, so the values are those
// of three separate passes bit for bit (reflecting level 0 alone does NOT give them: level k + 1 reflects the pixels of level k).
// A 16-lane DPP row is one JOB: a STRIP of 16 level-3 columns (a lane owns eight consecutive level-0 columns = four level-1,
// two level-2, one level-3 column) marched down the level-0 rows of a SEGMENT of level-3 rows; a wavefront carries four jobs.
// Per level-0 row a lane loads its eight bytes, takes the two pixels to its left and the one to its right from the neighbouring
// lanes (row_shr / row_shl) and forms four horizontal sums with 8-bit dot products.  The vertical pass of a level is a ring of
// the last five rows of that level's horizontal sums in registers (2 + 1 + 1 dwords per row, two sums per dword): a level-1 row
// comes out every second level-0 row, a level-2 row every fourth, a level-3 row every eighth, and each is passed on to the next
// level's horizontal sums straight from the registers.  A level-3 column needs the level-0 columns 8 x3 - 14 .. 8 x3 + 14: the
// two lanes at either end of a strip are halo, the twelve between them own outputs; a segment warms up on the 16 level-0 rows
// above the first level-0 row it owns and runs 8 rows past the last: 8 (rows + 3) level-0 rows for `rows` level-3 rows.
// Borders.  Columns: a lane at an image edge permutes the bytes of its extended row (v_perm with selectors computed once per
// lane: the out-of-image positions read the reflected column of THAT level, identity everywhere else).  Rows: level 0 is
// reflected at the loads; the rings of the levels 1 and 2 substitute the reflected rows of their level when the first / last
// row of the next level is formed (pd_vfix).
// Block -> (image, four jobs): the jobs of ONE image get block ids that are congruent modulo 8 (blocks b and b + 8 share an
// XCD: the halo rows and columns that neighbouring jobs read twice come from that XCD's L2).
#define P3_HALO 2              // halo lanes at either end of a strip
#define P3_OWN 12              // lanes of a 16-lane strip that own outputs
#define P3_SEG_ROWS 8          // level-3 rows of a segment in a launch that fills the device (measured: DESIGN.md section 6)
struct Pyr3Job { const uint8_t *src; uint8_t *d1, *d2, *d3; int w0, h0; };

namespace {
typedef uint32_t __attribute__((aligned(1))) pd_u32u;
typedef uint16_t __attribute__((aligned(1))) pd_u16u;
typedef unsigned long long __attribute__((aligned(1))) pd_u64u;
// the images live in global memory: typed so, a uniform base and a 32-bit lane offset make one global_load / global_store
typedef const __attribute__((address_space(1))) pd_u64u *pd_gld64;
typedef __attribute__((address_space(1))) pd_u32u *pd_gst32;
typedef __attribute__((address_space(1))) pd_u16u *pd_gst16;
typedef __attribute__((address_space(1))) uint8_t *pd_gst8;

template <int CTRL> __device__ __forceinline__ uint32_t pd_dpp0(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t pd_dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }

// four neighbouring horizontal [1 4 6 4 1] sums of the extended row e[-2 .. 8] (dwords e0 = e[-2 .. 1], e1 = e[2 .. 5],
// e2 = e[6 .. 8]): outputs centred on e[0], e[2], e[4], e[6], two per register in 16-bit lanes (a sum is below 2^12)
__device__ __forceinline__ uint2 pd_h4(uint32_t e0, uint32_t e1, uint32_t e2) {
    const uint32_t h0 = pd_dot4(e0, 0x04060401u, e1 & 255u), h1 = pd_dot4(e0, 0x04010000u, pd_dot4(e1, 0x00010406u, 0u));
    const uint32_t h2 = pd_dot4(e1, 0x04060401u, e2 & 255u), h3 = pd_dot4(e1, 0x04010000u, pd_dot4(e2, 0x00010406u, 0u));
    uint2 o; o.x = h0 | (h1 << 16); o.y = h2 | (h3 << 16);
    return o;
}
// vertical [1 4 6 4 1] of five rows of horizontal sums, both 16-bit lanes at once, rounded: the two output pixels are the bytes
// 1 and 3 of the result (s + 128 <= 16 * 16 * 255 + 128 < 2^16, so the lanes never carry into each other)
__device__ __forceinline__ uint32_t pd_v2(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t r4) {
    return (r0 + r4 + 0x00800080u) + ((r1 + r2 + r3) << 2) + (r2 << 1);
}
// store the n (1 .. 4) pixels of a group that lie inside the image row; the offset is that of the first pixel in its level
__device__ __forceinline__ void pd_store4(uint8_t *lvl, uint32_t off, int n, uint32_t px) {
    if (n >= 4) { *(pd_gst32)(lvl + off) = px; return; }
    *(pd_gst8)(lvl + off) = (uint8_t)px;
    if (n >= 2) *(pd_gst8)(lvl + off + 1u) = (uint8_t)(px >> 8);
    if (n >= 3) *(pd_gst8)(lvl + off + 2u) = (uint8_t)(px >> 16);
}
// v_perm selector of one dword of a lane's extended row (positions p0 .. p0 + 3; position p is the column cb - 2 + p of a level
// of width w): a position outside the image reads the position of its BORDER_REFLECT_101 column when that lies in the two
// source dwords (positions base .. base + 7; always, for a position a valid output needs), every other one keeps `ident`
__device__ uint32_t pd_fix_sel(int cb, int w, int p0, int base, uint32_t ident) {
    uint32_t sel = 0u;
    for (int b = 0; b < 4; ++b) {
        const int col = cb - 2 + p0 + b;
        uint32_t s = (ident >> (8 * b)) & 255u;
        if (col < 0 || col >= w) {
            const int sp = reflect101(col, w) - cb + 2 - base;
            if (sp >= 0 && sp < 8) s = (uint32_t)sp;
        }
        sel |= s << (8 * b);
    }
    return sel;
}
// the five ring rows a .. e = rows 2 yd - 2 .. 2 yd + 2 of a level of height hs, for the row yd of the next level: rows outside
// the image are replaced by their BORDER_REFLECT_101 rows (only the first and the last row of the next level reach outside)
__device__ __forceinline__ void pd_vfix(uint32_t &a, uint32_t &b, uint32_t c, uint32_t &d, uint32_t &e, int yd, int hs) {
    if (2 * yd + 1 == hs) { e = hs == 1 ? c : a; d = hs == 1 ? c : b; }       // rows hs, hs + 1 -> hs - 2, hs - 3
    else if (2 * yd + 2 == hs) e = c;                                          // row hs -> hs - 2
    if (yd == 0) { a = e; b = d; }                                             // rows -2, -1 -> 2, 1
}
}  // namespace

__global__ __launch_bounds__(64) void k_pyr_down3(const Pyr3Job *jobs, int n_jobs, int strips, int seg3, int waves) {
    const int xcd = blockIdx.x & 7, qb = blockIdx.x >> 3;
    const int ji = xcd + 8 * (qb / waves), wi = qb - (qb / waves) * waves;
    if (ji >= n_jobs) return;
    const Pyr3Job job = jobs[ji];
    const int w0 = job.w0, h0 = job.h0, w1 = (w0 + 1) >> 1, h1 = (h0 + 1) >> 1, w2 = (w1 + 1) >> 1, h2 = (h1 + 1) >> 1, w3 = (w2 + 1) >> 1, h3 = (h2 + 1) >> 1;
    const int lane = threadIdx.x, r = lane & 15;
    const int sj = 4 * wi + (lane >> 4);
    const int seg = sj / strips, strip = sj - seg * strips;
    const int x3 = P3_OWN * strip - P3_HALO + r;                 // the lane's level-3 column
    const int y3a = seg3 * seg, y3b = min(y3a + seg3, h3);       // the segment's level-3 rows
    const bool job_on = P3_OWN * strip < w3 && y3a < h3;
    if (!__any(job_on)) return;
    const bool own = job_on && r >= P3_HALO && r < P3_HALO + P3_OWN && x3 < w3;
    // ---- byte selectors of the extended rows (identity except in the lanes at the left / right image edge of a level)
    uint32_t sa0 = 0x03020100u, sa1 = 0x07060504u, sa2 = 0x07060504u, sb0 = 0x03020100u, sb1 = 0x07060504u, sc0 = 0x03020100u, sc1 = 0x07060504u;
    if (x3 >= 0 && 8 * x3 < w0 && (x3 == 0 || 8 * x3 + 8 >= w0 || 4 * x3 + 4 >= w1 || 2 * x3 + 2 >= w2)) {
        sa0 = pd_fix_sel(8 * x3, w0, 0, 0, sa0); sa1 = pd_fix_sel(8 * x3, w0, 4, 0, sa1); sa2 = pd_fix_sel(8 * x3, w0, 8, 4, sa2);
        sb0 = pd_fix_sel(4 * x3, w1, 0, 0, sb0); sb1 = pd_fix_sel(4 * x3, w1, 4, 0, sb1);
        sc0 = pd_fix_sel(2 * x3, w2, 0, 0, sc0); sc1 = pd_fix_sel(2 * x3, w2, 4, 0, sc1);
    }
    // ---- level-0 loads: eight bytes at the lane's first column.  A lane whose eight columns reach past the row loads the last
    // eight bytes of the row and shifts (the bytes past the edge are replaced through sa*); lanes outside the image read
    // clamped addresses, their values reach no valid output.  Images narrower than eight pixels load the eight bytes that end
    // with the image at the latest (an image holds at least eight bytes).
    const int c0 = min(max(8 * x3, 0), w0 - 1), cl = max(min(c0, w0 - 8), 0);
    const int sh0 = 8 * (c0 - cl), k0 = 2 * (h0 - 1);
    const uint32_t last8 = (uint32_t)max(w0 * h0 - 8, 0);
    auto load = [&](int s) -> uint2 {
        int y = max(s, -s);
        y = max(min(y, k0 - y), 0);                              // BORDER_REFLECT_101 of the rows a valid output needs, clamped
        const uint32_t a = (uint32_t)y * (uint32_t)w0 + (uint32_t)cl, ac = min(a, last8);     // (a <= last8 unless w0 < 8)
        const int sh = sh0 + 8 * (int)(a - ac);
        const unsigned long long q = *(pd_gld64)(job.src + ac) >> sh;
        uint2 o; o.x = (uint32_t)q; o.y = (uint32_t)(q >> 32);
        return o;
    };
    // ---- the march: step p of iteration `it` takes the level-0 row 8 t + p, t = y3a - 2 + it
    uint2 R0[5];
    uint32_t R1[5], R2[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) { R0[k].x = R0[k].y = 0u; R1[k] = R2[k] = 0u; }
    int t = y3a - 2;
    uint2 q[4];                                                  // rows are loaded four steps before they are used
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = load(8 * t + k);
    const int y1a = 4 * y3a, y1b = min(4 * (y3a + seg3), h1), y2a = 2 * y3a, y2b = min(2 * (y3a + seg3), h2);
    const int n1 = own ? min(w1 - 4 * x3, 4) : 0, n2 = own ? min(w2 - 2 * x3, 2) : 0;      // pixels of the lane inside a level-1 / level-2 row
#pragma unroll 1
    for (int it = 0; it < seg3 + 3; ++it, ++t) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const uint2 px = q[p & 3];
            q[p & 3] = load(8 * t + p + 4);
            // extended row e[-2 .. 8] of level 0 and its four horizontal sums
            const uint32_t lf = pd_dpp0<0x111>(px.y), rt = pd_dpp0<0x101>(px.x);
            const uint32_t e0 = __builtin_amdgcn_alignbyte(px.x, lf, 2), e1 = __builtin_amdgcn_alignbyte(px.y, px.x, 2), e2 = __builtin_amdgcn_alignbyte(rt, px.y, 2);
#pragma unroll
            for (int k = 0; k < 4; ++k) R0[k] = R0[k + 1];
            R0[4] = pd_h4(__builtin_amdgcn_perm(e1, e0, sa0), __builtin_amdgcn_perm(e1, e0, sa1), __builtin_amdgcn_perm(e2, e1, sa2));
            if (p & 1) continue;
            // ---- level-1 row y1 = (8 t + p) / 2 - 1: four pixels per lane
            const int y1 = 4 * t + p / 2 - 1;
            const uint32_t p1 = __builtin_amdgcn_perm(pd_v2(R0[0].y, R0[1].y, R0[2].y, R0[3].y, R0[4].y), pd_v2(R0[0].x, R0[1].x, R0[2].x, R0[3].x, R0[4].x), 0x07050301u);
            if (n1 > 0 && y1 >= y1a && y1 < y1b) pd_store4(job.d1, (uint32_t)(y1 * w1 + 4 * x3), n1, p1);
            {
                const uint32_t l1 = pd_dpp0<0x111>(p1), r1 = pd_dpp0<0x101>(p1);
                const uint32_t u0 = __builtin_amdgcn_alignbyte(p1, l1, 2), u1 = __builtin_amdgcn_alignbyte(r1, p1, 2);
                const uint32_t g0 = __builtin_amdgcn_perm(u1, u0, sb0), g1 = __builtin_amdgcn_perm(u1, u0, sb1);
#pragma unroll
                for (int k = 0; k < 4; ++k) R1[k] = R1[k + 1];
                R1[4] = pd_dot4(g0, 0x04060401u, g1 & 255u) | (pd_dot4(g0, 0x04010000u, pd_dot4(g1, 0x00010406u, 0u)) << 16);
            }
            if (p != 2 && p != 6) continue;
            // ---- level-2 row y2 = y1 / 2 - 1: two pixels per lane (the low half of p2)
            const int y2 = 2 * t - 1 + (p == 6);
            uint32_t p2;
            {
                uint32_t a = R1[0], b = R1[1], d = R1[3], e = R1[4];
                pd_vfix(a, b, R1[2], d, e, y2, h1);
                p2 = __builtin_amdgcn_perm(0u, pd_v2(a, b, R1[2], d, e), 0x0c0c0301u);
            }
            if (n2 > 0 && y2 >= y2a && y2 < y2b) {
                const uint32_t o = (uint32_t)(y2 * w2 + 2 * x3);
                if (n2 == 2) *(pd_gst16)(job.d2 + o) = (uint16_t)p2; else *(pd_gst8)(job.d2 + o) = (uint8_t)p2;
            }
            {
                const uint32_t l2 = pd_dpp0<0x111>(p2), r2 = pd_dpp0<0x101>(p2);
                const uint32_t u0 = __builtin_amdgcn_perm(p2, l2, 0x05040100u);              // e[-2 .. 1]; r2 = e[2] in its byte 0
                const uint32_t g0 = __builtin_amdgcn_perm(r2, u0, sc0), g1 = __builtin_amdgcn_perm(r2, u0, sc1);
#pragma unroll
                for (int k = 0; k < 4; ++k) R2[k] = R2[k + 1];
                R2[4] = pd_dot4(g0, 0x04060401u, g1 & 255u);
            }
            if (p != 6) continue;
            // ---- level-3 row y3 = y2 / 2 - 1: one pixel per lane
            const int y3 = t - 1;
            uint32_t a = R2[0], b = R2[1], d = R2[3], e = R2[4];
            pd_vfix(a, b, R2[2], d, e, y3, h2);
            const uint32_t p3 = (((a + e) + 4u * (b + d) + 6u * R2[2] + 128u) >> 8) & 255u;
            if (own && y3 >= y3a && y3 < y3b) *(pd_gst8)(job.d3 + (uint32_t)(y3 * w3 + x3)) = (uint8_t)p3;
        }
    }
}

extern "C" void fe_launch_pyr_down3(const Pyr3Job *jobs_dev, int n_jobs, int max_w0, int max_h0, hipStream_t st) {
    const int w3 = (((max_w0 + 1) / 2 + 1) / 2 + 1) / 2, h3 = (((max_h0 + 1) / 2 + 1) / 2 + 1) / 2;
    if (n_jobs <= 0 || w3 <= 0 || h3 <= 0) return;
    const int strips = (w3 + P3_OWN - 1) / P3_OWN;
    // level-3 rows per segment: long segments pay the 24 warm-up and run-out rows of level 0 less often, short ones give more
    // wavefronts (the 192-stream launch: 67-70 us with 8 rows = 6 k wavefronts, 79-80 us with 16); the segments of a launch are
    // made equally long
    int target = P3_SEG_ROWS;
    while (target > 4 && (long long)n_jobs * strips * ((h3 + target - 1) / target) / 4 < 2048) target /= 2;
    const int segs = (h3 + target - 1) / target, seg3 = (h3 + segs - 1) / segs;
    const int waves = (strips * segs + 3) / 4;
    hipLaunchKernelGGL(k_pyr_down3, dim3(8 * ((n_jobs + 7) / 8) * waves), dim3(64), 0, st, jobs_dev, n_jobs, strips, seg3, waves);
}

// ------------------------------------------------------------------------------------------ detector
#define DET_BORDER 8
#define DS_LANES 14            // lanes of a 16-lane strip that produce outputs (the two on the right only feed their neighbours)
#define DS_COLS (4 * DS_LANES) // output columns of a strip

// Per-cell maxima are merged as 64-bit keys  gen (8 bits) | score (24 bits) | ~order (32 bits):
//   score  = integer Shi-Tomasi score (< 2^24: two sums of 64 squared differences of bytes),
//   order  = row-major position inside the cell, complemented, so ties go to the first pixel in scan order,
//   gen    = push generation of the context (1..255): a newer push always wins the atomicMax, so the key array is
//            never cleared between frames (only when the generation wraps or the array is reallocated).
__device__ __forceinline__ unsigned long long det_key(unsigned int gen, int score, unsigned int order) {
    return ((unsigned long long)gen << 56) | ((unsigned long long)(unsigned int)score << 32) | (0xFFFFFFFFu - order);
}

// floor(sqrt(v)) for 0 <= v < 2^48, exact: the hardware estimate is corrected with integer compares.
__device__ __forceinline__ unsigned int isqrt48(unsigned long long v, double vd) {
    unsigned int r = (unsigned int)__builtin_amdgcn_sqrt(vd);
    while ((unsigned long long)r * r > v) --r;
    while ((unsigned long long)(r + 1) * (r + 1) <= v) ++r;
    return r;
}

template <int CTRL> __device__ __forceinline__ int det_dpp0(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }   // lanes without a source read 0
template <int CTRL> __device__ __forceinline__ unsigned long long det_dpp0_64(unsigned long long v) {
    const unsigned int lo = (unsigned int)det_dpp0<CTRL>((int)(unsigned int)v), hi = (unsigned int)det_dpp0<CTRL>((int)(unsigned int)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

typedef short det_v2s __attribute__((ext_vector_type(2)));
// a.lo * b.lo + a.hi * b.hi of two pairs of 16-bit lanes (three-operand form with an inline-constant addend: no move)
__device__ __forceinline__ int det_dot2(int a, int b) { return __builtin_amdgcn_sdot2(__builtin_bit_cast(det_v2s, a), __builtin_bit_cast(det_v2s, b), 0, true); }
__device__ __forceinline__ int det_pksub(uint32_t a, uint32_t b) { return __builtin_bit_cast(int, (det_v2s)(__builtin_bit_cast(det_v2s, a) - __builtin_bit_cast(det_v2s, b))); }

// Horizontal 8-sums of one gradient product for the lane's four output columns.  The lane holds the products of its four
// columns as the pair sums P01 = p0 + p1, P23 = p2 + p3 and the single products p0, p2; lane r + 1 holds the next four
// columns, lane r + 2 the four after (row_shl DPP inside the 16-lane strip):
//   H0 = P01 + P23 + (the same of lane r+1),  H2 = H0 - P01 + P01 of lane r+2,  H1 = H0 - p0 + p0'',  H3 = H2 - p2 + p2''.
__device__ __forceinline__ void det_hsum(int P01, int P23, int p0, int p2, int H[4]) {
    const int S = P01 + P23;
    H[0] = S + det_dpp0<0x101>(S);
    H[2] = H[0] + (det_dpp0<0x102>(P01) - P01);
    H[1] = H[0] + (det_dpp0<0x102>(p0) - p0);
    H[3] = H[2] + (det_dpp0<0x102>(p2) - p2);
}

struct DetPix { uint32_t lo, hi; };     // eight pixels of an image row: columns c - 4 .. c - 1 and c .. c + 3 of the lane's first column c

// Gradient products dx*dx, dx*dy, dy*dy (central differences) of the lane's four columns in the row `mid`, in the form
// det_hsum takes: P[4 i .. 4 i + 3] = P01, P23, p0, p2 of the product i.  The differences are formed two at a time in 16-bit
// lanes (byte permutes + packed subtract), the products and their pair sums are 16-bit dot products.
__device__ __forceinline__ void det_prod(uint32_t up, DetPix mid, uint32_t dn, int P[12]) {
    const uint32_t rn = (uint32_t)det_dpp0<0x101>((int)mid.hi);          // the pixels of lane r + 1 (its first one is needed)
    // pixels m0 .. m5 = columns c - 1 .. c + 4 as pairs of 16-bit lanes
    const uint32_t m01 = __builtin_amdgcn_perm(mid.hi, mid.lo, 0x0c040c03u);   // (lo.b3, hi.b0)
    const uint32_t m23 = __builtin_amdgcn_perm(0u, mid.hi, 0x0c020c01u);       // (hi.b1, hi.b2)
    const uint32_t m45 = __builtin_amdgcn_perm(rn, mid.hi, 0x0c040c03u);       // (hi.b3, rn.b0)
    const int D01 = det_pksub(m23, m01), D23 = det_pksub(m45, m23);            // dx of columns (0, 1) and (2, 3)
    const int E01 = det_pksub(__builtin_amdgcn_perm(0u, dn, 0x0c010c00u), __builtin_amdgcn_perm(0u, up, 0x0c010c00u));
    const int E23 = det_pksub(__builtin_amdgcn_perm(0u, dn, 0x0c030c02u), __builtin_amdgcn_perm(0u, up, 0x0c030c02u));
    const int D0 = D01 & 0xffff, D2 = D23 & 0xffff, E0 = E01 & 0xffff, E2 = E23 & 0xffff;   // (d, 0): picks the product of the even column
    P[0] = det_dot2(D01, D01); P[1] = det_dot2(D23, D23); P[2] = det_dot2(D0, D01); P[3] = det_dot2(D2, D23);
    P[4] = det_dot2(D01, E01); P[5] = det_dot2(D23, E23); P[6] = det_dot2(D0, E01); P[7] = det_dot2(D2, E23);
    P[8] = det_dot2(E01, E01); P[9] = det_dot2(E23, E23); P[10] = det_dot2(E0, E01); P[11] = det_dot2(E2, E23);
}
// V += the horizontal 8-sums of the twelve values P (the products of a row, or the difference of the products of two rows:
// the sums are linear and every term is an integer far below 2^31)
__device__ __forceinline__ void det_vadd(const int P[12], int Va[4], int Vb[4], int Vc[4]) {
    int Ha[4], Hb[4], Hc[4];
    det_hsum(P[0], P[1], P[2], P[3], Ha); det_hsum(P[4], P[5], P[6], P[7], Hb); det_hsum(P[8], P[9], P[10], P[11], Hc);
#pragma unroll
    for (int j = 0; j < 4; ++j) { Va[j] += Ha[j]; Vb[j] += Hb[j]; Vc[j] += Hc[j]; }
}

// cg::CornerDetector per-cell maxima of cam0 level 0 (image_processor.cpp:259, :657): integer Shi-Tomasi score
// (a + c) - isqrt((a - c)^2 + 4 b^2) of the 8x8 box sums a, b, c of the gradient products, maximum per detector cell with
// ties going to the first pixel in row-major order.
// Round 2 staged a 32x32 tile in LDS and ran three barrier-separated LDS passes over three product planes (24 LDS words
// per pixel, 124 VALU instructions per pixel, 304 us alone for 192 streams).  This version keeps everything in registers:
// a 16-lane DPP row is a STRIP of 64 columns (four per lane, 56 outputs) marched down a SEGMENT of rows.  Per row a lane
// loads eight bytes, forms its twelve products, the horizontal 8-sums come from the two lanes to the right (row_shl), and
// the vertical 8-sums are running sums: the products of the row leaving the window are RECOMPUTED from its pixels (re-read
// through L1/L2) and subtracted from those of the row entering it, and the horizontal sums of that one difference are
// added (the sums are linear: one set of them per step, not two) - cheaper than a ring of eight rows of twelve sums in
// registers, and there is no LDS, no barrier and no inter-wave traffic at all.  The exact score test needs the square root only for a pixel
// that beats the best score its own column has seen in the current cell (disc < (a + c - best)^2 is decided first), so
// after the first rows of a cell almost no pixel takes the expensive path.  At the bottom of a cell row the lanes of a
// strip merge their keys with a segmented DPP max (runs of lanes in the same cell) and the first lane of each run issues
// the one atomicMax.
// Block -> (stream, four jobs): the jobs (strip, segment) of ONE stream get block ids congruent modulo 8, so an image
// travels through the L2 of one XCD (blocks b and b + 8 share an XCD).
// MASKED (fe_mask.h; launched only when a stream of the push has a cam0 mask): masks[si].mask0 is the stream's bit plane, null
// = this stream is not masked.  A lane's first output column xs + 4 r is a multiple of 4, so the bits of its four columns
// are one aligned nibble of one word: one more small load per row, and a pixel whose bit is clear takes no part (its column's
// best score is not touched either, so the maximum is that of the usable pixels alone).  MASKED = false is the kernel as it
// was: it never looks at `masks`.
template <bool MASKED>
__global__ __launch_bounds__(64) void k_detect_cells(const FeStreamDev *streams, const FeMaskDev *masks, int n_streams, int strips, int seg_rows, int waves, unsigned int gen) {
    const int xcd = blockIdx.x & 7, qb = blockIdx.x >> 3;
    const int si = xcd + 8 * (qb / waves), wi = qb - (qb / waves) * waves;
    if (si >= n_streams) return;
    const FeStreamDev &S = streams[si];
    const int W = S.curr0.w[0], H = S.curr0.h[0];
    const int cw = S.cell_w, ch = S.cell_h, det_cols = S.det_cols, det_floor = S.det_floor;
    unsigned long long *const cell_keys = S.cell_keys;
    const int lane = threadIdx.x, r = lane & 15;
    const int job = 4 * wi + (lane >> 4);
    const int seg = job / strips, strip = job - seg * strips;
    const int xs = DET_BORDER + DS_COLS * strip;                 // first output column of the strip
    const int ys = DET_BORDER + seg_rows * seg;                  // first output row of the segment
    const int y_end = min(ys + seg_rows, H - DET_BORDER);
    const bool job_on = xs < W - DET_BORDER && ys < y_end;
    if (!__any(job_on)) return;
    // the lane's four product columns c0 .. c0 + 3 (outputs x = c0 + 4 + j); a lane right of the image reads clamped
    // addresses: its products only reach outputs that are not valid either
    const int c0 = xs - 4 + 4 * r;
    const int cl = min(c0, W - 4);
    const uint8_t *img = S.curr0.lvl[0];
    typedef uint32_t __attribute__((aligned(1))) u32u;
    auto load = [&](int row) -> DetPix {
        const uint8_t *p = img + (size_t)min(max(row, 0), H - 1) * W + cl;
        DetPix v; v.lo = *(const u32u *)(p - 4); v.hi = *(const u32u *)p; return v;
    };
    int xin[4], cx[4];
    bool col_ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = c0 + 4 + j;
        cx[j] = x / cw; xin[j] = x - cx[j] * cw;
        col_ok[j] = job_on && r < DS_LANES && x < W - DET_BORDER;
    }
    // the lane's mask word of a row: column (xs + 4 r) >> 5 of the plane (a lane right of the image reads the row's last word:
    // none of its columns is valid)
    const uint32_t *mrow = nullptr;
    int mpw = 0, msh = 0;
    if constexpr (MASKED) {
        mrow = masks[si].mask0; mpw = masks[si].pitch_w;
        if (mrow) mrow += min(c0 + 4, W - 1) >> 5;
        msh = (c0 + 4) & 31;
    }
    int Va[4] = {0, 0, 0, 0}, Vb[4] = {0, 0, 0, 0}, Vc[4] = {0, 0, 0, 0};
    // ---- fill the window of the first output row: product rows ys - 4 .. ys + 3
    int pr = ys - 4;
    // (the rows are loaded two steps before they are used: e_nx / l_nx are in flight while a step computes)
    DetPix e_mid = load(pr), e_dn = load(pr + 1), e_nx = load(pr + 2);
    uint32_t e_up = load(pr - 1).hi;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
        const DetPix nx = load(pr + 3);
        int P[12];
        det_prod(e_up, e_mid, e_dn.hi, P);
        det_vadd(P, Va, Vb, Vc);
        e_up = e_mid.hi; e_mid = e_dn; e_dn = e_nx; e_nx = nx; ++pr;
    }
    // ---- steady state: output row y sees the rows y - 4 .. y + 3; then the row pr = y + 4 enters and the row y - 4 leaves in
    // ONE set of horizontal sums, those of the difference of their products: V(y + 1) = V(y) + H(enter(y + 1) - leave(y))
    uint32_t l_up = load(ys - 5).hi;
    DetPix l_mid = load(ys - 4), l_dn = load(ys - 3), l_nx = load(ys - 2);
    int cy = ys / ch, yin = ys - cy * ch;
    int bs[4] = {0, 0, 0, 0};                                    // best score of the column in the current cell
    unsigned long long bk[4] = {0ULL, 0ULL, 0ULL, 0ULL};
    const int n_rows = seg_rows;                                 // (uniform trip count; rows past y_end are masked)
#pragma unroll 1
    for (int k = 0; k < n_rows; ++k) {
        const int y = ys + k;
        const bool row_ok = y < y_end;
        const DetPix enx = load(pr + 3), lnx = load(y - 1);
        uint32_t nib = 15u;                                      // usable columns of the lane in this row
        if constexpr (MASKED) { if (mrow) nib = (mrow[(size_t)min(y, H - 1) * mpw] >> msh) & 15u; }
        if (!MASKED || nib)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!(col_ok[j] && row_ok)) continue;
            if (MASKED && !((nib >> j) & 1u)) continue;
            const int a = Va[j], b = Vb[j], d = Vc[j];
            // score > T  <=>  isqrt(disc) < X := a + d - T  <=>  disc < X^2 (X > 0): decided exactly (everything is below
            // 2^50) before the square root.  T = the detection floor or the best score of this column in this cell: a
            // later pixel of the column only replaces the best with a strictly larger score (ties go to the first).
            const int X = (a + d) - max(det_floor, bs[j]);
            if (X <= 0) continue;
            const int df = a - d;
            if (abs(df) >= X || 2 * abs(b) >= X) continue;       // each term of disc alone already reaches X^2
            const double discd = (double)df * (double)df + 4.0 * ((double)b * (double)b);   // exact: < 2^48
            if (discd >= (double)X * (double)X) continue;
            const long long disc = (long long)df * df + 4LL * ((long long)b * b);
            const int score = (a + d) - (int)isqrt48((unsigned long long)disc, discd);
            bs[j] = score;
            bk[j] = det_key(gen, score, (unsigned int)(yin * cw + xin[j]));
        }
        {
            int Pe[12], Pl[12];
            det_prod(e_up, e_mid, e_dn.hi, Pe);
            det_prod(l_up, l_mid, l_dn.hi, Pl);
#pragma unroll
            for (int j = 0; j < 12; ++j) Pe[j] -= Pl[j];
            det_vadd(Pe, Va, Vb, Vc);
            e_up = e_mid.hi; e_mid = e_dn; e_dn = e_nx; e_nx = enx; ++pr;
            l_up = l_mid.hi; l_mid = l_dn; l_dn = l_nx; l_nx = lnx;
        }
        // ---- bottom of a cell row (or of the segment): merge the strip's keys per cell, one atomicMax per cell
        ++yin;
        const bool flush = job_on && row_ok && (yin == ch || y + 1 == y_end);
        if (cw < 4) {
            // cells narrower than a lane's four columns (images below 188 pixels with the 47-column detector grid): a lane may
            // touch three cells, so every column sends its own key
            if (flush) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (bk[j]) atomicMax(&cell_keys[cy * det_cols + cx[j]], bk[j]);
                    bs[j] = 0; bk[j] = 0ULL;
                }
            }
        } else if (__any(flush)) {
            // a lane's four columns lie in at most two cells (cells are at least four pixels wide): A = the cell of its
            // first column, B = the cell of its last one when that differs
            unsigned long long ka = 0ULL, kb = 0ULL;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long v = flush ? bk[j] : 0ULL;
                if (cx[j] == cx[0]) ka = v > ka ? v : ka; else kb = v > kb ? v : kb;
            }
            const bool two = cx[3] != cx[0];
#pragma unroll 1
            for (int pass = 0; pass < 2; ++pass) {
                unsigned long long kk = pass ? kb : ka;
                const int id = flush ? (pass ? (two ? cx[3] : -1 - r) : cx[0]) : -1 - r;     // (negative ids never match a neighbour)
                if (pass && !__any(flush && two)) break;
                // segmented max over runs of lanes with the same cell id: after the steps 1, 2, 4, 8 the first lane of a
                // run holds the maximum of the run
                {
                    const int o = det_dpp0<0x101>(id + 0x40000000) - 0x40000000; const unsigned long long v = det_dpp0_64<0x101>(kk);
                    if (o == id && v > kk) kk = v;
                }
                {
                    const int o = det_dpp0<0x102>(id + 0x40000000) - 0x40000000; const unsigned long long v = det_dpp0_64<0x102>(kk);
                    if (o == id && v > kk) kk = v;
                }
                {
                    const int o = det_dpp0<0x104>(id + 0x40000000) - 0x40000000; const unsigned long long v = det_dpp0_64<0x104>(kk);
                    if (o == id && v > kk) kk = v;
                }
                {
                    const int o = det_dpp0<0x108>(id + 0x40000000) - 0x40000000; const unsigned long long v = det_dpp0_64<0x108>(kk);
                    if (o == id && v > kk) kk = v;
                }
                const int left = det_dpp0<0x111>(id + 0x40000000) - 0x40000000;          // row_shr:1: the lane to the left (none: -2^30)
                if (id >= 0 && left != id && kk) atomicMax(&cell_keys[cy * det_cols + id], kk);
            }
            if (flush) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { bs[j] = 0; bk[j] = 0ULL; }
            }
        }
        if (yin == ch) { yin = 0; ++cy; }
    }
}

static void det_launch(const FeStreamDev *streams_dev, const FeMaskDev *masks_dev, int n_streams, int max_w, int max_h, unsigned int gen, hipStream_t st) {
    // rows per segment: short segments give more wavefronts (a launch should fill the device several times over) but every
    // segment pays seven window-filling rows
    const int strips = (max_w - 2 * DET_BORDER + DS_COLS - 1) / DS_COLS, rows = max_h - 2 * DET_BORDER;
    if (strips <= 0 || rows <= 0) return;
    int seg_rows = 32;
    while (seg_rows < 128 && (long long)n_streams * strips * ((rows + seg_rows - 1) / seg_rows) / 4 > 32768) seg_rows *= 2;
    const int segs = (rows + seg_rows - 1) / seg_rows;
    const int waves = (strips * segs + 3) / 4;
    if (masks_dev) hipLaunchKernelGGL(k_detect_cells<true>, dim3(8 * ((n_streams + 7) / 8) * waves), dim3(64), 0, st, streams_dev, masks_dev, n_streams, strips, seg_rows, waves, gen);
    else hipLaunchKernelGGL(k_detect_cells<false>, dim3(8 * ((n_streams + 7) / 8) * waves), dim3(64), 0, st, streams_dev, masks_dev, n_streams, strips, seg_rows, waves, gen);
}
extern "C" void fe_launch_detect(const FeStreamDev *streams_dev, int n_streams, int max_w, int max_h, unsigned int gen, hipStream_t st) {
    det_launch(streams_dev, nullptr, n_streams, max_w, max_h, gen, st);
}
// The masked instantiation: masks_dev[i] goes with streams_dev[i] (a null mask0 = that stream is not masked).
extern "C" void fe_launch_detect_masked(const FeStreamDev *streams_dev, const FeMaskDev *masks_dev, int n_streams, int max_w, int max_h, unsigned int gen, hipStream_t st) {
    if (!masks_dev) return;
    det_launch(streams_dev, masks_dev, n_streams, max_w, max_h, gen, st);
}

// ------------------------------------------------------------------------------------------ point math
// det_atan / det_tan, the deterministic atan / tan of the equidistant model, live in fe_cam_models.h with the opt-in camera
// models that also need them (one source for the kernel and the g++ harnesses).
#include "fe_cam_models.h"

// cv::undistortPoints (radtan: 5 fixed-point iterations; equidistant: cv::fisheye::undistortPoints, Newton on theta,
// <= 10 iterations), then R, then P = {1,1,0,0}.  Same operation sequence as oracle/o_image.cpp undistort_point.
__device__ __forceinline__ void undistort_pt(const CamDev &cam, const double *R, float u, float v, float &xo, float &yo) {
    const double fx = cam.K[0], fy = cam.K[1], cx = cam.K[2], cy = cam.K[3];
    double x = ((double)u - cx) / fx, y = ((double)v - cy) / fy;
    if (cam.model == MSKF_MODEL_EQUIDISTANT) {
        const double *k = cam.D;
        double theta_d = sqrt(x * x + y * y);
        const double half_pi = 1.5707963267948966;
        theta_d = theta_d > half_pi ? half_pi : (theta_d < -half_pi ? -half_pi : theta_d);
        double scale = 0.0;
        if (theta_d > 1e-8) {
            double theta = theta_d;
            for (int j = 0; j < 10; ++j) {
                const double t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
                const double k0t2 = k[0] * t2, k1t4 = k[1] * t4, k2t6 = k[2] * t6, k3t8 = k[3] * t8;
                const double fix = (theta * (1 + k0t2 + k1t4 + k2t6 + k3t8) - theta_d) /
                                   (1 + 3 * k0t2 + 5 * k1t4 + 7 * k2t6 + 9 * k3t8);
                theta = theta - fix;
                if (fabs(fix) < 1e-8) break;
            }
            scale = det_tan(theta) / theta_d;
        }
        x = x * scale; y = y * scale;
    } else {
        const double k1 = cam.D[0], k2 = cam.D[1], p1 = cam.D[2], p2 = cam.D[3];
        const double x0 = x, y0 = y;
        for (int j = 0; j < 5; ++j) {
            const double r2 = x * x + y * y;
            const double icdist = 1.0 / (1.0 + (k2 * r2 + k1) * r2);
            const double deltaX = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
            const double deltaY = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
            x = (x0 - deltaX) * icdist;
            y = (y0 - deltaY) * icdist;
        }
    }
    if (R) {
        const double X = R[0] * x + R[1] * y + R[2];
        const double Y = R[3] * x + R[4] * y + R[5];
        const double Wd = R[6] * x + R[7] * y + R[8];
        x = X / Wd; y = Y / Wd;
    } else {
        // identity rectification: X = 1*x + 0*y + 0 etc. are exact, W = 1
        x = x / 1.0; y = y / 1.0;
    }
    xo = (float)(x * 1.0 + 0.0);
    yo = (float)(y * 1.0 + 0.0);
}

// cg::project_points with zero rvec / tvec: (x, y) is the ray (x, y, 1); oracle/o_image.cpp distort_point
__device__ __forceinline__ void distort_pt(const CamDev &cam, float xf, float yf, float &uo, float &vo) {
    const double fx = cam.K[0], fy = cam.K[1], cx = cam.K[2], cy = cam.K[3];
    const double x = (double)xf, y = (double)yf;
    double xd, yd;
    if (cam.model == MSKF_MODEL_EQUIDISTANT) {
        const double *k = cam.D;
        const double r = sqrt(x * x + y * y);
        const double theta = det_atan(r);
        const double t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
        const double theta_d = theta * (1 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8);
        const double scale = (r > 1e-8) ? theta_d / r : 1.0;
        xd = x * scale; yd = y * scale;
    } else {
        const double k1 = cam.D[0], k2 = cam.D[1], p1 = cam.D[2], p2 = cam.D[3];
        const double r2 = x * x + y * y, r4 = r2 * r2;
        const double a1 = 2.0 * x * y, a2 = r2 + 2.0 * x * x, a3 = r2 + 2.0 * y * y;
        const double cdist = 1.0 + k1 * r2 + k2 * r4;
        xd = x * cdist + p1 * a1 + p2 * a2;
        yd = y * cdist + p1 * a3 + p2 * a1;
    }
    uo = (float)(xd * fx + cx);
    vo = (float)(yd * fy + cy);
}

// The opt-in camera models (fe_cam_models.h, which puts the same pixel step, rotation and rounding around them): what the extended
// instantiation of the track kernel calls.  A camera on a base model goes through undistort_pt / distort_pt themselves (the old operation
// sequence: a mixed batch runs base-model streams through the extended launch).  false = outside the model's domain, and
// then the outputs are 0.  `model` is uniform over a stream, so the switch is a scalar branch.
__device__ __forceinline__ bool undistort_pt_ext(const CamDev &cam, int model, const double *coef, const double *R, float u, float v, float &xo, float &yo) {
    if (model < FCM_RADTAN8) { undistort_pt(cam, R, u, v, xo, yo); return true; }
    return fcm_undistort_px(cam.K, model, coef, R, u, v, xo, yo);
}
__device__ __forceinline__ bool distort_pt_ext(const CamDev &cam, int model, const double *coef, float xf, float yf, float &uo, float &vo) {
    if (model < FCM_RADTAN8) { distort_pt(cam, xf, yf, uo, vo); return true; }
    return fcm_distort_px(cam.K, model, coef, xf, yf, uo, vo);
}

// ------------------------------------------------------------------------------------------ LK (l4_track and its parts: fe_lk.h)
#include "fe_lk.h"

// One launch per track call (mskf_fe_track*): for the four points of a wavefront, with the point state in registers,
//   temporal LK prev cam0 -> curr cam0 from the predicted position (:321-350, :410)      [do_temporal streams only]
//   -> image-bounds gate (:416-424) -> stereo initial guess undistort(cam0, R01) . distort(cam1) (:542-548)
//   -> stereo LK curr cam0 -> curr cam1 (:569) -> image-bounds gate (:575-583), undistorted points (:601-604, also what
//   publish() sends, :1154-1155) and the epipolar gate (:605-617).
// Round 2 ran this chain as five launches (two LK launches and three geometry launches, kernels that no longer exist, one thread
// per point for the geometry) with
// out0 / out1 / status making a round trip through global memory between each; the per-point double-precision geometry is
// a few hundred instructions, issued here once per wavefront for its four points (the sixteen lanes of a row compute the
// same values).  The two tracks run through ONE copy of the LK code (a two-trip loop), so the kernel is no larger.
// Outputs per point: out0 = cam0 point in the current image (tracked, or the input of a stereo-only stream), out1 = matched
// cam1 point, und0 / und1 = their undistorted normalised coordinates, status bit 0 = survived the temporal half, bit 1 =
// stereo match accepted; a point that fails the temporal half gets out1 = und0 = und1 = 0 and status 0.
// Block -> (stream, point group): the blocks b and b + 8 share an XCD (round-robin dispatch, speed only), so the point
// groups of ONE stream are given ids that are congruent modulo 8: a stream's pyramid levels then travel through one L2.
// The body is written once and instantiated twice: k_track4 (EXT = false: the two base models, the code object every default
// launch runs) and k_track4_ext (EXT = true: it also reads the streams' FeCamExtDev records, fe_cam_models.h; launched only for
// a batch in which a stream has an extended model).  Under EXT a point outside a model's domain takes no stereo trip (out1 = 0,
// stereo status 0) when its guess cannot be formed, and loses status bit 1 when und0 or und1 cannot; what could not be computed
// is written as 0.
// A third instantiation, k_track4_deep (EXT = DEEP = true; opt-in deeper LK pyramids, fe_deep.h), is launched only for a batch in
// which a stream tracks over more than four levels: every l4_track of a stream then starts at that stream's top level
// (FeDeepDev::levels; 4 for the other streams of the batch, which get the bits they always got).
template <bool EXT, bool DEEP>
__device__ __forceinline__ void track4_body(const FeStreamDev *streams, const FeCamExtDev *exts, const FeDeepDev *deeps, int n_streams, int groups_per_stream,
                                            uint32_t (*s_T)[L4_TROWS * L4_DW + 2], uint32_t (*s_S)[L4_SROWS * L4_DW + 4]) {
    const int x = blockIdx.x & 7, qb = blockIdx.x >> 3;
    const int si = x + 8 * (qb / groups_per_stream), gi = qb - (qb / groups_per_stream) * groups_per_stream;
    if (si >= n_streams) return;
    const FeStreamDev &S = streams[si];
    // the point count may live on the device (candidates chosen by fe_book1): the grid is then sized from an estimate and
    // a block takes several point groups if there are more
    const int n_pts = S.n_pts_dev ? *S.n_pts_dev : S.n_pts;
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    uint32_t *sT = s_T[g], *sS = s_S[g];
#pragma nounroll
    for (int gq = gi; 4 * gq < n_pts; gq += groups_per_stream) {
    const int pt = 4 * gq + g;
    const bool in_range = pt < n_pts;
    mskf_point2f pin = {0.f, 0.f};
    if (in_range) pin = S.in_pts[pt];
    unsigned int dbg_iters = 0, dbg_t = 0;
    // state of the point between the tracks
    float c0x = pin.x, c0y = pin.y;           // cam0 point in the current image
    bool ok = in_range;                        // survived the temporal half
    float tx = 0.f, ty = 0.f, gx = 0.f, gy = 0.f;
    bool alive = false;
    int ph = 1;
    if (S.do_temporal) {
        // predictFeatureTracking (:342-347): p2 = H p1, normalise, round to float
        const double *Hm = S.Hpred;
        const double px = (double)pin.x, py = (double)pin.y;
        const double X = Hm[0] * px + Hm[1] * py + Hm[2] * 1.0;
        const double Y = Hm[3] * px + Hm[4] * py + Hm[5] * 1.0;
        const double Z = Hm[6] * px + Hm[7] * py + Hm[8] * 1.0;
        tx = pin.x; ty = pin.y; gx = (float)(X / Z); gy = (float)(Y / Z);
        alive = in_range;
        ph = 0;
    }
    float c1x = 0.f, c1y = 0.f;
    int st1 = 0;
#pragma nounroll
    for (; ph < 2; ++ph) {
        if (ph == 1) {
            // stereo initial guess (:542-548) of the points that are still there
            gx = 0.f; gy = 0.f;
            bool guessed = ok;
            if (ok) {
                float rx, ry;
                if (EXT) {
                    const FeCamExtDev &X = exts[si];
                    guessed = undistort_pt_ext(S.cam0, X.model[0], X.coef[0], S.R01, c0x, c0y, rx, ry);
                    if (guessed) guessed = distort_pt_ext(S.cam1, X.model[1], X.coef[1], rx, ry, gx, gy);
                    if (!guessed) { gx = 0.f; gy = 0.f; }
                } else {
                    undistort_pt(S.cam0, S.R01, c0x, c0y, rx, ry);
                    distort_pt(S.cam1, rx, ry, gx, gy);
                }
            }
            tx = c0x; ty = c0y; alive = guessed;
        }
        float nx = 0.f, ny = 0.f;
        int st = 0;
        if (__any(alive)) {
            if (DEEP) {
                const FeDeepDev &P = deeps[si];
                l4_track<true>(ph ? S.curr0 : S.prev0, ph ? S.curr1 : S.curr0, alive, tx, ty, gx, gy, sT, sS, r, nx, ny, st, dbg_iters,
                               ph ? &P.curr0 : &P.prev0, ph ? &P.curr1 : &P.curr0, P.levels);
            } else l4_track(ph ? S.curr0 : S.prev0, ph ? S.curr1 : S.curr0, alive, tx, ty, gx, gy, sT, sS, r, nx, ny, st, dbg_iters);
        }
        if (ph == 0) {
            // temporal result and its image-bounds gate (:416-424)
            const int W = S.curr0.w[0], H = S.curr0.h[0];
            c0x = nx; c0y = ny;
            ok = alive && st != 0 && !(c0y < 0 || c0y > (float)(H - 1) || c0x < 0 || c0x > (float)(W - 1));
            dbg_t = dbg_iters; dbg_iters = 0;
        } else {
            c1x = alive ? nx : 0.f; c1y = alive ? ny : 0.f; st1 = alive ? st : 0;
        }
    }
    // stereo result: image-bounds gate (:575-583), undistorted points (:601-604), epipolar gate (:605-617)
    float u0x = 0.f, u0y = 0.f, u1x = 0.f, u1y = 0.f;
    int sst = st1;
    if (ok) {
        const int W1 = S.curr1.w[0], H1 = S.curr1.h[0];
        if (sst && (c1y < 0 || c1y > (float)(H1 - 1) || c1x < 0 || c1x > (float)(W1 - 1))) sst = 0;
        if (EXT) {
            const FeCamExtDev &X = exts[si];
            const bool in0 = undistort_pt_ext(S.cam0, X.model[0], X.coef[0], nullptr, c0x, c0y, u0x, u0y);
            const bool in1 = undistort_pt_ext(S.cam1, X.model[1], X.coef[1], nullptr, c1x, c1y, u1x, u1y);
            if (!in0 || !in1) sst = 0;
        } else {
            undistort_pt(S.cam0, nullptr, c0x, c0y, u0x, u0y);
            undistort_pt(S.cam1, nullptr, c1x, c1y, u1x, u1y);
        }
        if (sst) {
            const double *E = S.E;
            const double x0 = (double)u0x, y0 = (double)u0y, x1 = (double)u1x, y1 = (double)u1y;
            const double l0 = (E[0] * x0 + E[1] * y0) + E[2];
            const double l1 = (E[3] * x0 + E[4] * y0) + E[5];
            const double l2 = (E[6] * x0 + E[7] * y0) + E[8];
            const double err = fabs((x1 * l0 + y1 * l1) + l2) / sqrt(l0 * l0 + l1 * l1);
            if (err > S.epi_thresh) sst = 0;
        }
    }
    if (in_range && r == 0) {
        S.out0[pt] = mskf_point2f{c0x, c0y};
        S.out1[pt] = mskf_point2f{c1x, c1y};
        S.und0[pt] = mskf_point2f{u0x, u0y};
#ifdef LK_ITER_DBG
        ((unsigned int *)S.und1)[2 * pt] = dbg_t; ((unsigned int *)S.und1)[2 * pt + 1] = dbg_iters;
#else
        S.und1[pt] = mskf_point2f{u1x, u1y};
        (void)dbg_t;
#endif
        S.status[pt] = (uint8_t)(ok ? (1 | (sst ? 2 : 0)) : 0);
    }
    }
}
__global__ __launch_bounds__(64) void k_track4(const FeStreamDev *streams, int n_streams, int groups_per_stream) {
    __shared__ uint32_t s_T[4][L4_TROWS * L4_DW + 2];
    __shared__ uint32_t s_S[4][L4_SROWS * L4_DW + 4];
    track4_body<false, false>(streams, nullptr, nullptr, n_streams, groups_per_stream, s_T, s_S);
}
__global__ __launch_bounds__(64) void k_track4_ext(const FeStreamDev *streams, const FeCamExtDev *exts, int n_streams, int groups_per_stream) {
    __shared__ uint32_t s_T[4][L4_TROWS * L4_DW + 2];      // (each kernel owns its staging: an array two kernels share is laid out by
    __shared__ uint32_t s_S[4][L4_SROWS * L4_DW + 4];      // another rule, and k_track4's code object would no longer be the parent's)
    track4_body<true, false>(streams, exts, nullptr, n_streams, groups_per_stream, s_T, s_S);
}
__global__ __launch_bounds__(64) void k_track4_deep(const FeStreamDev *streams, const FeCamExtDev *exts, const FeDeepDev *deeps, int n_streams, int groups_per_stream) {
    __shared__ uint32_t s_T[4][L4_TROWS * L4_DW + 2];
    __shared__ uint32_t s_S[4][L4_SROWS * L4_DW + 4];
    track4_body<true, true>(streams, exts, deeps, n_streams, groups_per_stream, s_T, s_S);
}

// ------------------------------------------------------------------------------------------ bookkeeping (fe_book.h)
#include "fe_book.h"
// One workgroup per VIO stream: which = 0 after the first track call of the frame, 1 after the second.
__global__ __launch_bounds__(256) void k_fe_book(const FeBookDev *books, int which) {
    const FeBookDev &B = books[blockIdx.x];
    extern __shared__ int s_book[];
    FeBookScratch L;
    fe_book_scratch_init(L, s_book, B.cap, B.cand_cap, B.det_cap, B.n_codes, B.det_rows * B.det_cols);
    if (which == 0) fe_book1(B, L); else fe_book2(B, L);
}
// Dynamic LDS the bookkeeping kernel may use: 150 KiB once the attribute is granted (the 4K configuration's lists need more
// than the 64 KiB a kernel gets by default), 64 KiB otherwise.  mskf_stream_create sizes the device books against it.
extern "C" size_t fe_book_lds_budget(void) {
    static const size_t budget = []() -> size_t {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_fe_book), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        if (e != hipSuccess) { (void)hipGetLastError(); return 64 * 1024; }
        return 150 * 1024;
    }();
    return budget;
}
extern "C" void fe_launch_book(const FeBookDev *books_dev, int n_streams, int which, size_t scratch_bytes, hipStream_t st) {
    (void)fe_book_lds_budget();
    hipLaunchKernelGGL(k_fe_book, dim3(n_streams), dim3(256), scratch_bytes, st, books_dev, which);
}

// ------------------------------------------------------------------------------------------ equalisation (fe_equalize.h)
// Opt-in equalisation of level 0 of a push, ahead of k_pyr_down3 and k_detect_cells: at most three launches for both
// cameras of every stream of the push that has it on (blockIdx.y = image).
//   k_eq_hist  : a workgroup owns a CLAHE tile, or a strip of rows of a globally equalised image.  16-byte loads of the
//                aligned chunks that cover a row of its region (bytes outside the region masked; a chunk that reaches past
//                either end of the plane, and the reflected columns of the virtual extension, byte by byte); LDS integer
//                atomics into one sub-histogram per wavefront.  A tile goes on to its LUT in the same workgroup (clip,
//                closed-form redistribution, scan: 256 bytes out); a strip writes its 256 counts to scratch (no global
//                atomics, nothing to clear).
//   k_eq_lut   : global mode only, one workgroup per image: sums the strips, scans, writes the 256-byte LUT.
//   k_eq_apply : a workgroup owns a region between tile centres (the whole image in global mode), or a share of its rows;
//                the four LUTs of the region sit in LDS as one dword per level; a lane owns sixteen pixels: the 16-byte
//                chunks of the DESTINATION plane, whole ones stored as one dword x 4, the ends of a row byte by byte.
#include "fe_equalize.h"
namespace {
struct __attribute__((packed, aligned(1))) eq_u4 { uint32_t v[4]; };
// inclusive scan over the 256 threads of the workgroup (s: 256 ints of LDS, free on return after a barrier)
__device__ __forceinline__ int eq_block_scan(int v, int *s, int tid) {
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int t = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    return s[tid];
}
__device__ __forceinline__ void eq_count16(int *hw, const uint32_t v[4], int lo, int hi) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k >= lo && k < hi) atomicAdd(&hw[(v[k >> 2] >> (8 * (k & 3))) & 255u], 1);
}
}  // namespace

__global__ __launch_bounds__(256) void k_eq_hist(const EqJob *jobs) {
    const EqJob j = jobs[blockIdx.y];
    const int unit = blockIdx.x, tid = threadIdx.x;
    const int n_units = j.mode == EQ_CLAHE ? j.tiles_x * j.tiles_y : j.n_strips;
    if (unit >= n_units) return;
    __shared__ int s_hist[4][256];
    __shared__ int s_scan[256];
#pragma unroll
    for (int k = 0; k < 4; ++k) s_hist[k][tid] = 0;
    __syncthreads();
    // the region in coordinates of the (virtually extended) image: rows r0 .. r1 - 1, columns c0 .. c1 - 1
    int r0, r1, c0, c1;
    if (j.mode == EQ_CLAHE) {
        const int ty = unit / j.tiles_x, tx = unit - ty * j.tiles_x;
        r0 = ty * j.th; r1 = r0 + j.th; c0 = tx * j.tw; c1 = c0 + j.tw;
    } else {
        r0 = unit * j.strip_rows; r1 = min(j.h, r0 + j.strip_rows); c0 = 0; c1 = j.w;
    }
    int *hw = s_hist[tid >> 6];
    const int w = j.w, h = j.h, cr = min(c1, w);          // columns c0 .. cr - 1 are columns of the image itself
    if (cr > c0) {
        const uintptr_t img_b = (uintptr_t)j.src, img_e = img_b + (size_t)w * h;
        const int nch = (cr - c0 + 15) / 16 + 1;           // aligned chunks that can touch a row segment of cr - c0 bytes
        const int n_items = (r1 - r0) * nch;
        for (int idx = tid; idx < n_items; idx += 256) {
            const int rr = idx / nch, ch = idx - rr * nch;
            const uintptr_t a = img_b + (size_t)eq_src_row(r0 + rr, h) * w + c0, e = a + (size_t)(cr - c0);
            const uintptr_t q = (a & ~(uintptr_t)15) + 16 * (uintptr_t)ch;
            if (q >= e) continue;
            const int lo = a > q ? (int)(a - q) : 0, hi = e - q < 16 ? (int)(e - q) : 16;
            if (q >= img_b && q + 16 <= img_e) {
                const uint4 v = *reinterpret_cast<const uint4 *>(q);
                const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
                eq_count16(hw, vv, lo, hi);
            } else {
                for (int k = lo; k < hi; ++k) atomicAdd(&hw[*reinterpret_cast<const uint8_t *>(q + k)], 1);
            }
        }
    }
    if (c1 > w) {                                          // columns of the virtual extension
        const int cv0 = max(c0, w), nv = c1 - cv0, n_items = (r1 - r0) * nv;
        for (int idx = tid; idx < n_items; idx += 256) {
            const int rr = idx / nv, c = cv0 + idx - rr * nv;
            atomicAdd(&hw[j.src[(size_t)eq_src_row(r0 + rr, h) * w + eq_src_col(c, w)]], 1);
        }
    }
    __syncthreads();
    const int cnt = s_hist[0][tid] + s_hist[1][tid] + s_hist[2][tid] + s_hist[3][tid];
    if (j.mode != EQ_CLAHE) { j.part[256 * unit + tid] = cnt; return; }
    (void)eq_block_scan(eq_excess(cnt, j.clip), s_scan, tid);
    const int clipped = s_scan[255];
    __syncthreads();
    const int cum = eq_block_scan(eq_redistributed(cnt, tid, j.clip, clipped), s_scan, tid);
    j.lut[256 * (size_t)unit + tid] = (uint8_t)eq_clahe_entry(cum, eq_clahe_scale(j.tw * j.th));
}

__global__ __launch_bounds__(256) void k_eq_lut(const EqJob *jobs) {
    const EqJob j = jobs[blockIdx.x];
    if (j.mode != EQ_GLOBAL) return;
    const int tid = threadIdx.x;
    __shared__ int s_scan[256], s_cnt[256], s_i0;
    int cnt = 0;
    for (int s = 0; s < j.n_strips; ++s) cnt += j.part[256 * s + tid];
    s_cnt[tid] = cnt;
    if (tid == 0) s_i0 = 255;
    __syncthreads();
    if (cnt > 0) atomicMin(&s_i0, tid);
    const int cum = eq_block_scan(cnt, s_scan, tid);      // (its barriers also publish s_i0)
    const int i0 = s_i0;
    j.lut[tid] = (uint8_t)eq_global_entry(tid, i0, s_cnt[i0], cum, j.w * j.h);
}

__global__ __launch_bounds__(256) void k_eq_apply(const EqJob *jobs, int splits) {
    const EqJob j = jobs[blockIdx.y];
    const int region = blockIdx.x / splits, split = blockIdx.x - region * splits, tid = threadIdx.x;
    if (region >= eq_regions(j.mode, j.tiles_x, j.tiles_y)) return;
    const bool clahe = j.mode == EQ_CLAHE;
    const int w = j.w, h = j.h;
    int x0 = 0, x1 = w, y0 = 0, y1 = h, t1x = 0, t2x = 0, t1y = 0, t2y = 0;
    float inv_tw = 0.f, inv_th = 0.f;
    if (clahe) {
        // region (ry, rx): the pixels whose unclamped first tile is (ry - 1, rx - 1)
        const int nrx = j.tiles_x + 1, ry = region / nrx, rx = region - ry * nrx;
        inv_tw = eq_inv(j.tw); inv_th = eq_inv(j.th);
        x0 = rx == 0 ? 0 : eq_axis_first(rx - 1, j.tw, inv_tw, w); x1 = rx == j.tiles_x ? w : eq_axis_first(rx, j.tw, inv_tw, w);
        y0 = ry == 0 ? 0 : eq_axis_first(ry - 1, j.th, inv_th, h); y1 = ry == j.tiles_y ? h : eq_axis_first(ry, j.th, inv_th, h);
        t1x = max(rx - 1, 0); t2x = min(rx, j.tiles_x - 1); t1y = max(ry - 1, 0); t2y = min(ry, j.tiles_y - 1);
    }
    const int rp = (y1 - y0 + splits - 1) / splits, ya = y0 + split * rp, yb = min(y1, ya + rp);
    if (ya >= yb || x0 >= x1) return;
    __shared__ uint32_t s_lut[256];
    if (clahe) {
        const uint8_t *r1 = j.lut + 256 * (size_t)(t1y * j.tiles_x), *r2 = j.lut + 256 * (size_t)(t2y * j.tiles_x);
        s_lut[tid] = (uint32_t)r1[256 * t1x + tid] | ((uint32_t)r1[256 * t2x + tid] << 8) | ((uint32_t)r2[256 * t1x + tid] << 16) | ((uint32_t)r2[256 * t2x + tid] << 24);
    } else s_lut[tid] = j.lut[tid];
    __syncthreads();
    const int nch = (x1 - x0 + 15) / 16 + 1, n_items = (yb - ya) * nch;
    for (int idx = tid; idx < n_items; idx += 256) {
        const int rr = idx / nch, ch = idx - rr * nch, y = ya + rr;
        const size_t row = (size_t)y * w, pb = row + x0, pe = row + x1;
        const size_t P = (pb & ~(size_t)15) + 16 * (size_t)ch;
        if (P >= pe) continue;
        const int lo = pb > P ? (int)(pb - P) : 0, hi = pe - P < 16 ? (int)(pe - P) : 16;
        const bool whole = lo == 0 && hi == 16;
        uint32_t in[4] = {0u, 0u, 0u, 0u}, out[4] = {0u, 0u, 0u, 0u};
        if (whole) { const eq_u4 v = *reinterpret_cast<const eq_u4 *>(j.src + P); in[0] = v.v[0]; in[1] = v.v[1]; in[2] = v.v[2]; in[3] = v.v[3]; }
        else {
#pragma unroll
            for (int k = 0; k < 16; ++k) if (k >= lo && k < hi) in[k >> 2] |= (uint32_t)j.src[P + k] << (8 * (k & 3));
        }
        EqAxis ay = {0, 0, 0.f, 0.f};
        if (clahe) ay = eq_axis(y, inv_th, j.tiles_y);
        const int xb = (int)(P - row);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t v = (in[k >> 2] >> (8 * (k & 3))) & 255u, L = s_lut[v];
            uint32_t o = L;
            if (clahe) {
                const EqAxis ax = eq_axis(xb + k, inv_tw, j.tiles_x);
                o = (uint32_t)eq_interp((int)(L & 255u), (int)((L >> 8) & 255u), (int)((L >> 16) & 255u), (int)(L >> 24), ax.a, ax.a1, ay.a, ay.a1);
            }
            out[k >> 2] |= o << (8 * (k & 3));
        }
        if (whole) *reinterpret_cast<uint4 *>(j.dst + P) = make_uint4(out[0], out[1], out[2], out[3]);
        else {
#pragma unroll
            for (int k = 0; k < 16; ++k) if (k >= lo && k < hi) j.dst[P + k] = (uint8_t)(out[k >> 2] >> (8 * (k & 3)));
        }
    }
}

// max_units: most tiles / strips of a job; max_regions, splits: the apply kernel's grid (eq_regions, shares of a region's rows)
extern "C" void fe_launch_equalize(const EqJob *jobs_dev, int n_jobs, int max_units, int any_global, int max_regions, int splits, hipStream_t st) {
    if (n_jobs <= 0) return;
    hipLaunchKernelGGL(k_eq_hist, dim3(max_units, n_jobs), dim3(256), 0, st, jobs_dev);
    if (any_global) hipLaunchKernelGGL(k_eq_lut, dim3(n_jobs), dim3(256), 0, st, jobs_dev);
    hipLaunchKernelGGL(k_eq_apply, dim3(max_regions * splits, n_jobs), dim3(256), 0, st, jobs_dev, splits);
}

// ------------------------------------------------------------------------------------------ input pixel formats (fe_pixfmt.h)
// Opt-in conversion of the raw images of a push (16-bit grey, interleaved colour, 8-bit Bayer) into the streams' 8-bit level
// 0, ahead of the equalisation, k_pyr_down3 and k_detect_cells: ONE launch for both cameras of every converting stream of
// the push (blockIdx.y = image).  A bandwidth kernel: a lane owns a 16-byte chunk of the DESTINATION plane, sixteen grey
// pixels stored as one dword x 4, and loads their 32 / 48 / 64 source bytes as two / three / four dword x 4 (unaligned where
// the source row starts so); a mosaic loads the sixteen bytes of the three rows around the chunk and one byte either side
// of each.  The ends of a row, the chunks of a mosaic that touch the left or right border (the only place where a folded
// column index is formed) and planes whose rows do not start on 16 bytes go pixel by pixel through px_pixel, the function
// the CPU harness runs.  Consecutive lanes own consecutive chunks of a row.  The format is a field of the job: one switch
// per workgroup, none per pixel.
#include "fe_pixfmt.h"
namespace {
// The pointers of a job come out of a record in memory, so the compiler knows no address space for them and would issue flat
// accesses; images live in global memory, and the whole-chunk path says so (global_load / global_store_dwordx4).
#if defined(__HIP_DEVICE_COMPILE__)
#define PX_GLOBAL __attribute__((address_space(1)))
#else
#define PX_GLOBAL          // (the host pass only parses the kernels)
#endif
typedef const PX_GLOBAL uint8_t *px_gptr;
__device__ __forceinline__ px_gptr px_global(const uint8_t *p) { return (px_gptr)(uintptr_t)p; }
__device__ __forceinline__ uint32_t px_byte(const uint32_t *v, int i) { return (v[i >> 2] >> (8 * (i & 3))) & 255u; }
template <int NV>
__device__ __forceinline__ void px_load(uint32_t *v, px_gptr p) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const eq_u4 t = *reinterpret_cast<const PX_GLOBAL eq_u4 *>(p + 16 * q);
        v[4 * q] = t.v[0]; v[4 * q + 1] = t.v[1]; v[4 * q + 2] = t.v[2]; v[4 * q + 3] = t.v[3];
    }
}
// the sixteen pixels x0 .. x0 + 15 of row y (all inside the row), packed
template <int FMT>
__device__ __forceinline__ void px_chunk16(const PxJob &j, int x0, int y, uint32_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0u;
    constexpr int BPP = FMT == PX_GRAY16 ? 2 : (FMT == PX_RGB8 || FMT == PX_BGR8) ? 3 : 4;
    uint32_t v[4 * BPP];
    px_load<BPP>(v, px_global(j.src) + (size_t)y * (size_t)j.pitch + (size_t)x0 * BPP);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        int g;
        if (FMT == PX_GRAY16) g = px_gray16((int)((v[k >> 1] >> (16 * (k & 1))) & 0xFFFFu), j.shift);
        else {
            const int c0 = (int)px_byte(v, BPP * k), c1 = (int)px_byte(v, BPP * k + 1), c2 = (int)px_byte(v, BPP * k + 2);
            g = (FMT == PX_RGB8 || FMT == PX_RGBA8) ? px_luma(c0, c1, c2) : px_luma(c2, c1, c0);
        }
        out[k >> 2] |= (uint32_t)g << (8 * (k & 3));
    }
}
// the same for a mosaic; 1 <= x0 and x0 + 16 <= w - 1: every neighbour column is a column of the image
__device__ __forceinline__ void px_chunk16_bayer(const PxJob &j, int x0, int y, uint32_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0u;
    const px_gptr src = px_global(j.src);
    const px_gptr rows[3] = {src + (size_t)px_reflect(y - 1, j.h) * (size_t)j.pitch + x0, src + (size_t)y * (size_t)j.pitch + x0,
                             src + (size_t)px_reflect(y + 1, j.h) * (size_t)j.pitch + x0};
    uint32_t v[3][4], lft[3], rgt[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { px_load<1>(v[r], rows[r]); lft[r] = rows[r][-1]; rgt[r] = rows[r][16]; }
    const int site0 = px_bayer_site(j.format, x0, y), site1 = px_bayer_site(j.format, x0 + 1, y);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        int a[3], b[3], c[3];       // columns k - 1, k, k + 1 of the three rows
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[r] = (int)(k == 0 ? lft[r] : px_byte(v[r], k - 1));
            b[r] = (int)px_byte(v[r], k);
            c[r] = (int)(k == 15 ? rgt[r] : px_byte(v[r], k + 1));
        }
        const int g = px_bayer_luma((k & 1) ? site1 : site0, b[1], a[1], c[1], b[0], b[2], a[0], c[0], a[2], c[2]);
        out[k >> 2] |= (uint32_t)g << (8 * (k & 3));
    }
}
template <int FMT>
__device__ __forceinline__ void px_rows(const PxJob &j) {
    const int w = j.w, h = j.h;
    const int nch = (w + 15) / 16 + 1;                     // aligned chunks that can touch a row of w bytes
    const long long n_items = (long long)h * nch;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n_items; idx += (long long)gridDim.x * 256) {
        const int y = (int)(idx / nch), ch = (int)(idx - (long long)y * nch);
        const uintptr_t pb = (uintptr_t)j.dst + (size_t)y * w, pe = pb + (size_t)w;
        const uintptr_t P = (pb & ~(uintptr_t)15) + 16 * (uintptr_t)ch;
        if (P >= pe) continue;
        const int lo = pb > P ? (int)(pb - P) : 0, hi = pe - P < 16 ? (int)(pe - P) : 16;
        const int x0 = (int)((long long)P - (long long)pb);          // column of the chunk's first byte (negative before the row)
        bool whole = lo == 0 && hi == 16;
        if (FMT == PX_BAYER_RGGB8) whole = whole && x0 >= 1 && x0 + 16 <= w - 1;
        if (whole) {
            uint32_t out[4];
            if (FMT == PX_BAYER_RGGB8) px_chunk16_bayer(j, x0, y, out); else px_chunk16<FMT>(j, x0, y, out);
            *reinterpret_cast<PX_GLOBAL uint4 *>(P) = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
            for (int k = lo; k < hi; ++k) *reinterpret_cast<PX_GLOBAL uint8_t *>(P + k) = (uint8_t)px_pixel(j.src, (size_t)j.pitch, w, h, j.format, j.shift, x0 + k, y);
        }
    }
}
}  // namespace

__global__ __launch_bounds__(256) void k_px_convert(const PxJob *jobs) {
    const PxJob j = jobs[blockIdx.y];
    switch (j.format) {                                    // uniform over the workgroup
        case PX_GRAY16: px_rows<PX_GRAY16>(j); break;
        case PX_RGB8: px_rows<PX_RGB8>(j); break;
        case PX_BGR8: px_rows<PX_BGR8>(j); break;
        case PX_RGBA8: px_rows<PX_RGBA8>(j); break;
        case PX_BGRA8: px_rows<PX_BGRA8>(j); break;
        case PX_BAYER_RGGB8: case PX_BAYER_GRBG8: case PX_BAYER_GBRG8: case PX_BAYER_BGGR8: px_rows<PX_BAYER_RGGB8>(j); break;      // (the pattern is read from the job)
        default: break;
    }
}

// max_w, max_h: the largest image of the jobs (the grid covers its chunks; smaller images leave workgroups idle)
extern "C" void fe_launch_px_convert(const PxJob *jobs_dev, int n_jobs, int max_w, int max_h, hipStream_t st) {
    if (n_jobs <= 0 || max_w <= 0 || max_h <= 0) return;
    const long long items = (long long)max_h * ((max_w + 15) / 16 + 1);
    const long long wgs = (items + 255) / 256;
    hipLaunchKernelGGL(k_px_convert, dim3((unsigned)(wgs > 65535 ? 65535 : wgs), n_jobs), dim3(256), 0, st, jobs_dev);
}

// completion mark of the spinning wait (mskf_wait_event): one thread stores a sequence number into pinned host memory
// once everything enqueued before it on the stream (the D2H copies included) is done
__global__ void k_mark(volatile unsigned int *flag, unsigned int seq) {
    *flag = seq;
    __threadfence_system();
}
extern "C" void fe_launch_mark(volatile unsigned int *flag, unsigned int seq, hipStream_t st) {
    hipLaunchKernelGGL(k_mark, dim3(1), dim3(1), 0, st, flag, seq);
}

// Staging copies as a kernel of the stream itself (pinned host memory <-> device memory, both addressable from a kernel).
// hipMemcpyAsync hands such copies to the SDMA engines: a second kind of queue, shared by every stream of the process, with a
// cross-queue signal either side of each copy.  With sixteen busy streams the copies of all of them convoy behind whichever
// copy is waiting for its own stream's kernel, and now and then (one bench run in ten to twenty, round 4) every stream's next
// copy stood still for seconds up to a minute: every queue of the pipeline was found waiting in front of a staging copy.
// One launch moves up to MSKF_COPY_SEGS segments; 16-byte accesses (the arenas are 64-byte aligned), the odd bytes at the
// end of a segment one by one.
struct MskfCopySegs { void *dst[MSKF_COPY_SEGS]; const void *src[MSKF_COPY_SEGS]; unsigned long long bytes[MSKF_COPY_SEGS]; int blocks_per_seg; };
__global__ __launch_bounds__(256) void k_mskf_copy(MskfCopySegs segs) {
    const int seg = (int)blockIdx.x / segs.blocks_per_seg, b = (int)blockIdx.x - seg * segs.blocks_per_seg;
    const unsigned long long bytes = segs.bytes[seg], n16 = bytes >> 4;
    const uint4 *__restrict__ src = (const uint4 *)segs.src[seg];
    uint4 *__restrict__ dst = (uint4 *)segs.dst[seg];
    const unsigned long long stride = (unsigned long long)segs.blocks_per_seg * 256ULL;
    unsigned long long i = (unsigned long long)b * 256ULL + threadIdx.x;
    for (; i + 3ULL * stride < n16; i += 4ULL * stride) {          // four loads in flight per lane (the source may sit across PCIe)
        const uint4 a0 = src[i], a1 = src[i + stride], a2 = src[i + 2ULL * stride], a3 = src[i + 3ULL * stride];
        dst[i] = a0; dst[i + stride] = a1; dst[i + 2ULL * stride] = a2; dst[i + 3ULL * stride] = a3;
    }
    for (; i < n16; i += stride) dst[i] = src[i];
    if (b == 0 && threadIdx.x < (unsigned)(bytes & 15ULL)) ((uint8_t *)dst)[(n16 << 4) + threadIdx.x] = ((const uint8_t *)src)[(n16 << 4) + threadIdx.x];
}
extern "C" void fe_launch_copy(void *const *dst, const void *const *src, const size_t *bytes, int n_segs, hipStream_t st) {
    MskfCopySegs segs;
    size_t mx = 0;
    for (int i = 0; i < MSKF_COPY_SEGS; ++i) {
        segs.dst[i] = i < n_segs ? dst[i] : nullptr; segs.src[i] = i < n_segs ? src[i] : nullptr; segs.bytes[i] = i < n_segs ? bytes[i] : 0ULL;
        if (i < n_segs && bytes[i] > mx) mx = bytes[i];
    }
    if (n_segs <= 0 || mx == 0) return;
    size_t bps = (mx + 16383) / 16384;                  // 16 KiB per workgroup and sweep
    segs.blocks_per_seg = (int)(bps < 1 ? 1 : bps > 96 ? 96 : bps);
    hipLaunchKernelGGL(k_mskf_copy, dim3(segs.blocks_per_seg * n_segs), dim3(256), 0, st, segs);
}

extern "C" void fe_launch_track(const FeStreamDev *streams_dev, int n_streams, int max_pts, hipStream_t st) {
    if (max_pts <= 0) return;
    const int gps = (max_pts + 3) / 4;
    hipLaunchKernelGGL(k_track4, dim3(8 * ((n_streams + 7) / 8) * gps), dim3(64), 0, st, streams_dev, n_streams, gps);
}
// the extended instantiation over the same grid: cams_dev[i] goes with streams_dev[i]
extern "C" void fe_launch_track_ext(const FeStreamDev *streams_dev, const FeCamExtDev *cams_dev, int n_streams, int max_pts, hipStream_t st) {
    if (max_pts <= 0) return;
    const int gps = (max_pts + 3) / 4;
    hipLaunchKernelGGL(k_track4_ext, dim3(8 * ((n_streams + 7) / 8) * gps), dim3(64), 0, st, streams_dev, cams_dev, n_streams, gps);
}
// the deep instantiation over the same grid: cams_dev[i] and deep_dev[i] go with streams_dev[i]
extern "C" void fe_launch_track_deep(const FeStreamDev *streams_dev, const FeCamExtDev *cams_dev, const FeDeepDev *deep_dev, int n_streams, int max_pts, hipStream_t st) {
    if (max_pts <= 0) return;
    const int gps = (max_pts + 3) / 4;
    hipLaunchKernelGGL(k_track4_deep, dim3(8 * ((n_streams + 7) / 8) * gps), dim3(64), 0, st, streams_dev, cams_dev, deep_dev, n_streams, gps);
}

// ------------------------------------------------------------------------------------------ image masks: the point gate (fe_mask.h)
// Behind a track launch of a batch that has a masked stream, over the same descriptors: a pure function of the track's outputs.
// A point whose cam0 pixel is masked out is lost as k_track4 loses one (status 0, out1 = und0 = und1 = 0, out0 kept); else a
// stereo inlier whose cam1 pixel is masked out loses bit 1, like a point the epipolar gate refuses.  One lane per point, the
// points of a stream strided over the blocks of its grid row (the count may live on the device: n_pts_dev); streams without
// a mask return at once.
__global__ __launch_bounds__(256) void k_mask_points(const FeStreamDev *streams, const FeMaskDev *masks) {
    const FeMaskDev M = masks[blockIdx.y];
    if (!M.mask0 && !M.mask1) return;
    const FeStreamDev &S = streams[blockIdx.y];
    const int n_pts = S.n_pts_dev ? *S.n_pts_dev : S.n_pts;
    const int W = S.curr0.w[0], H = S.curr0.h[0];
    for (int pt = blockIdx.x * 256 + threadIdx.x; pt < n_pts; pt += gridDim.x * 256) {
        const int st = S.status[pt];
        if (!(st & 3)) continue;
        const mskf_point2f p0 = S.out0[pt], p1 = S.out1[pt];
        int what;
        const int ns = fm_gate(M.mask0, M.mask1, M.pitch_w, W, H, p0.x, p0.y, p1.x, p1.y, st, &what);
        if (what == FM_LOST) {
            S.out1[pt] = mskf_point2f{0.f, 0.f}; S.und0[pt] = mskf_point2f{0.f, 0.f}; S.und1[pt] = mskf_point2f{0.f, 0.f};
        }
        if (ns != st) S.status[pt] = (uint8_t)ns;
    }
}
extern "C" void fe_launch_mask_points(const FeStreamDev *streams_dev, const FeMaskDev *masks_dev, int n_streams, int max_pts, hipStream_t st) {
    if (max_pts <= 0 || n_streams <= 0 || !masks_dev) return;
    hipLaunchKernelGGL(k_mask_points, dim3((max_pts + 255) / 256, n_streams), dim3(256), 0, st, streams_dev, masks_dev);
}
