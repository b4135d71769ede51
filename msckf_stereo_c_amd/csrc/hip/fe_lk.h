// fe_lk.h — the pyramidal-LK device code of the front-end: l4_track (four points per wavefront, a 16-lane row per point, DPP row
// sums, LDS staging) with everything it is made of.  ONE source for the two kernels that track: k_track4 (fe_kernels.hip) and
// k_fb_points (fe_fb.hip, the forward-backward check), so that a backward track is the forward track's arithmetic by
// construction.  Device code only (PyrDev and MSKF_LEVELS come from fe_device.h, the deeper levels of an opt-in stream from
// fe_deep.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fe_device.h"
#include "fe_deep.h"

// ------------------------------------------------------------------------------------------ LK
#define LK_HALF 7
#define LK_WIN 15
#define LK_ITERS 30

// ---- DPP butterfly step of the row reductions (l4_row_sum).  All lanes of the row must be active.
template <int CTRL> __device__ __forceinline__ int dpp_add(int v) {
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
// (double)b * 2^-20, exactly, for |b| < 2^51, in ONE double-precision instruction: b is added (scalar unit) to the bit
// pattern of 1.5 * 2^32, whose mantissa LSB weighs 2^-20; subtracting 1.5 * 2^32 leaves b * 2^-20.  The plain form
// (int64 -> double conversion, then the scaling) is five double-rate instructions per value, and FP64 issues at half
// rate: these uniform conversions were a tenth of the kernel.
__device__ __forceinline__ double lk_scaled_f64(long long b) {
    return __longlong_as_double(b + 0x41F8000000000000LL) - 6442450944.0;
}

// ------------------------------------------------------------------------------------------ LK, four points per wavefront
// l4_track (the LK half of k_track4): pyramidal LK (OpenCV calcOpticalFlowPyrLK with OPTFLOW_USE_INITIAL_FLOW semantics, fixed point: every
// decision-bearing quantity is an integer or a fixed sequence of double operations) with a 16-lane row of the
// wavefront per point: lane r of a row owns image row r of the 16 x 16 search footprint, i.e. ALL 15 pixels of window
// row r.  What that buys over one wavefront per point (round 1: 2840 VALU instructions per point, now 1950):
//   * the per-point scalar work of an iteration (weights, 2 x 2 solve, convergence tests) is issued once for four points;
//   * the cross-lane reduction stays inside a DPP row (no cross-row step, no readlane);
//   * a lane walks 16 consecutive bytes, so the bilinear sample is two packed 16-bit dot products
//     (v_dot2_i32_i16 on byte pairs built with v_perm_b32) per row instead of four multiplies per pixel, the row below
//     comes from the neighbouring lane through a DPP row shift fused into the add, and the b1 / b2 sums are packed dot
//     products too (|diff| <= 8160 and |I| <= 4080 fit 16 bits).
// Iterations run in lock step for the four points of a wave; a point that has converged idles until the others have.
typedef short l4_v2s __attribute__((ext_vector_type(2)));
#define L4_DW 6                // staged dwords per row (24 bytes: the 16 a window reads + alignment + slack)
#define L4_TROWS 18            // template source rows: 17 interpolated rows need 18
#define L4_SROWS 20            // staged search rows: the 16 a window reads + 4 of slack
#define L4_MAXOX 8             // window column offset inside the staged rows: 0 .. 8
#define L4_MAXOY (L4_SROWS - 16)

typedef unsigned short l4_v2u __attribute__((ext_vector_type(2)));
// a * b + c on the 24-bit multiplier (full rate; exact while |a|, |b| < 2^23).  The compiler lowers the C expression to
// separate multiplies and a three-operand add, or to the quarter-rate 32 x 32 -> 64 bit multiply-add.
template <int KA, int KC> __device__ __forceinline__ int l4_mad24_k(int x) {        // KA * x + KC, inline constants
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "n"(KA), "v"(x), "n"(KC));
    return d;
}
template <int KA> __device__ __forceinline__ int l4_mad24_kv(int x, int c) {        // KA * x + c
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "n"(KA), "v"(x), "v"(c));
    return d;
}
__device__ __forceinline__ int l4_mad24(int a, int b, int c) {
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
    return d;
}
__device__ __forceinline__ int l4_mad24_vvv(int a, int b, int c) {
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ int l4_dot2(int pair, int w, int acc) {          // running sums: acc is the destination (v_dot2c)
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(l4_v2s, pair), __builtin_bit_cast(l4_v2s, w), acc, false);
}
// Same product with a CONSTANT addend.  The two-operand form above needs the addend in the destination register, i.e. a
// v_mov per call when it is a constant (47 of the 270 instructions of an LK iteration were such moves); with the clamp
// bit set the compiler has to take the three-operand encoding, whose addend is an inline constant or a scalar register.
// Saturation never triggers here (|sums| < 2^23), so the value is the same.
__device__ __forceinline__ int l4_dot2k(int pair, int w, int k) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(l4_v2s, pair), __builtin_bit_cast(l4_v2s, w), k, true);
}
// ((a >> 9), (b >> 9)) as two 16-bit lanes for 0 <= a, b < 2^24: one byte permute takes bits 8..23 of both, one packed
// shift drops the ninth bit (three instructions fewer per pair than shift, shift, pack)
__device__ __forceinline__ int l4_pack_shr9(int a, int b) {
    const l4_v2u v = __builtin_bit_cast(l4_v2u, __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x06050201u));
    return __builtin_bit_cast(int, (l4_v2u)(v >> (unsigned short)1));
}
// DPP row operations (a row = the 16 lanes of one point).  row_shl:n: lane i reads lane i + n, row_shr:n: lane i - n.
#define L4_SHL1 0x101
#define L4_SHR1 0x111
template <int CTRL> __device__ __forceinline__ int l4_dpp0(int v) {        // lanes without a source read 0
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
// 16-lane (row) sum of per-lane int32 partials whose total needs more than 32 bits: quad sums in 32 bits (four lanes of
// |v| < 2^28.9 stay below 2^31), the last two butterflies in 64 bits.  Every lane of the row ends up with the sum.
__device__ __forceinline__ long long l4_row_sum(int v) {
    v = dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
    long long s = (long long)v;
    {
        const int lo = __builtin_amdgcn_update_dpp(0, (int)s, 0x141, 0xf, 0xf, true), hi = __builtin_amdgcn_update_dpp(0, (int)(s >> 32), 0x141, 0xf, 0xf, true);
        s += (long long)(((unsigned long long)(unsigned int)hi << 32) | (unsigned int)lo);     // row_half_mirror
    }
    {
        const int lo = __builtin_amdgcn_update_dpp(0, (int)s, 0x140, 0xf, 0xf, true), hi = __builtin_amdgcn_update_dpp(0, (int)(s >> 32), 0x140, 0xf, 0xf, true);
        s += (long long)(((unsigned long long)(unsigned int)hi << 32) | (unsigned int)lo);     // row_mirror
    }
    return s;
}

// Stage ROWS x 24 bytes at image (x0, y0) as LDS dwords dst[row * 6 + c]; the 16 lanes of a point cooperate (r = lane & 15).
// Pixels outside the image are replicated from the border.
struct __attribute__((packed, aligned(4))) l4_u4 { uint32_t v[4]; };
struct __attribute__((packed, aligned(4))) l4_u2 { uint32_t v[2]; };
template <int ROWS>
__device__ __forceinline__ void l4_stage(const uint8_t *img, int w, int h, int x0, int y0, uint32_t *dst, int r, bool on) {
    const bool fast = x0 >= 0 && y0 >= 0 && x0 + 4 * L4_DW <= w && y0 + ROWS <= h;
    if (fast) {
        // inside the image: lane r takes row r whole (24 bytes = a 16-byte and an 8-byte load at a dword-aligned address),
        // lanes 0 .. ROWS-17 take rows 16 .. ROWS-1 as well: four loads with one address each instead of seven or eight
        // dword loads with an element -> (row, column) division each
        if (on) {
            const uint8_t *p = img + l4_mad24_vvv(y0 + r, w, x0);
            const l4_u4 a = *(const l4_u4 *)p;
            const l4_u2 b = *(const l4_u2 *)(p + 16);
            uint32_t *d = dst + L4_DW * r;
            d[0] = a.v[0]; d[1] = a.v[1]; d[2] = a.v[2]; d[3] = a.v[3]; d[4] = b.v[0]; d[5] = b.v[1];
            if (r < ROWS - 16) {
                const uint8_t *p2 = img + l4_mad24_vvv(y0 + 16 + r, w, x0);
                const l4_u4 a2 = *(const l4_u4 *)p2;
                const l4_u2 b2 = *(const l4_u2 *)(p2 + 16);
                uint32_t *d2 = dst + L4_DW * (16 + r);
                d2[0] = a2.v[0]; d2[1] = a2.v[1]; d2[2] = a2.v[2]; d2[3] = a2.v[3]; d2[4] = b2.v[0]; d2[5] = b2.v[1];
            }
        }
        return;
    }
    // at the border: pixels outside the image are replicated from the edge.  x0 is a multiple of four, so a staged dword lies
    // inside its row, or left of it (four copies of the first pixel), or right of it / across its end (the row's last four
    // pixels shifted down, the last pixel repeated): ONE dword load at a clamped position per element and a byte alignment.
    // (Round 2 loaded four clamped bytes per element: 230 instructions per call, and at the two coarse levels almost every
    // wavefront has a point near the border - a quarter of all LK instructions were this path.)
    constexpr int N = ROWS * L4_DW, PER = (N + 15) / 16;
    typedef uint32_t __attribute__((aligned(1))) l4_u32u;
    uint32_t v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = r + 16 * i;
        v[i] = 0;
        if (on && e < N) {
            const int row = (e * 43) >> 8, c = e - L4_DW * row;       // e / 6 for e < 128
            const uint8_t *rp = img + l4_mad24_vvv(min(max(y0 + row, 0), h - 1), w, 0);
            const int xb = x0 + 4 * c, xc = min(max(xb, 0), w - 4), sh = xb - xc;
            const uint32_t D = *(const l4_u32u *)(rp + xc);
            const uint32_t first = (D & 255u) * 0x01010101u, last = (D >> 24) * 0x01010101u;
            v[i] = sh < 0 ? first : sh >= 4 ? last : __builtin_amdgcn_alignbyte(last, D, (uint32_t)sh);
        }
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) { const int e = r + 16 * i; if (on && e < N) dst[e] = v[i]; }
}

// byte pair (b_k, b_k+1) of a byte string held in aligned dwords, as two 16-bit lanes
template <int K> __device__ __forceinline__ int l4_pair(const uint32_t *a) {
    constexpr int q = K >> 2, m = K & 3;
    if (m == 0) return (int)__builtin_amdgcn_perm(0u, a[q], 0x0c010c00u);
    if (m == 1) return (int)__builtin_amdgcn_perm(0u, a[q], 0x0c020c01u);
    if (m == 2) return (int)__builtin_amdgcn_perm(0u, a[q], 0x0c030c02u);
    return (int)__builtin_amdgcn_perm(a[q + 1], a[q], 0x0c040c03u);
}
template <int N, int K = 0> struct L4Pairs {
    static __device__ __forceinline__ void run(const uint32_t *a, int *pr) { pr[K] = l4_pair<K>(a); L4Pairs<N, K + 1>::run(a, pr); }
};
template <int N> struct L4Pairs<N, N> { static __device__ __forceinline__ void run(const uint32_t *, int *) {} };

__device__ __forceinline__ void l4_weights(float fa, float fb, int &wtop, int &wbot) {
    const int qa = __float2int_rn(fa * 16384.0f), qb = __float2int_rn(fb * 16384.0f);
    // (operands <= 2^14: 24-bit multiply-adds; the 32 x 32 -> 64 bit form the compiler picks otherwise is quarter rate)
    const int w00 = l4_mad24(16384 - qa, 16384 - qb, 8192) >> 14;
    const int w01 = l4_mad24(qa, 16384 - qb, 8192) >> 14;
    const int w10 = l4_mad24(16384 - qa, qb, 8192) >> 14;
    const int w11 = 16384 - w00 - w01 - w10;                    // may be -1: kept signed in its 16-bit lane
    wtop = (w00 & 0xffff) | (w01 << 16);
    wbot = (w10 & 0xffff) | (w11 << 16);
}

// Pyramidal LK of the four points of a wavefront (see above): templates around (ax, ay) in pyramid A, search in pyramid B
// from the initial guess (bx, by), both in level-0 pixels.  Every lane of the wavefront calls it (it stages through LDS and
// uses the workgroup barrier of the one-wave workgroup); `alive` marks the 16-lane rows that carry a point.  Returns the
// tracked position and the OpenCV status (0: lost).
// DEEP (opt-in deeper pyramids, fe_deep.h): the walk starts at level `levels` - 1 (4 .. 8, uniform over the workgroup) instead
// of 3 and takes the levels 4 and up from Ad / Bd; everything a level does is the same code.  DEEP = false is the function as
// it was: the extra arguments are not looked at.  (Under -DLK_ITER_DBG the iteration counter packs 8 bits per level: it covers
// the levels 0 .. 3, the iterations of deeper levels are not counted.)
template <bool DEEP = false>
__device__ __forceinline__ void l4_track(const PyrDev &A, const PyrDev &B, bool alive, float ax, float ay, float bx, float by,
                                         uint32_t *sT, uint32_t *sS, int r, float &out_x, float &out_y, int &out_status, unsigned int &dbg_iters,
                                         const PyrDeepDev *Ad = nullptr, const PyrDeepDev *Bd = nullptr, int levels = MSKF_LEVELS) {
    int status = 1;
    float ncx = 0.f, ncy = 0.f;
    const bool winrow = r < LK_WIN;                       // lane 15 only feeds the row below window row 14
    const int top = DEEP ? levels - 1 : MSKF_LEVELS - 1;
    for (int l = top; l >= 0; --l) {
        const bool hi = DEEP && l >= MSKF_LEVELS;
        const uint8_t *imA = hi ? Ad->lvl[l - MSKF_LEVELS] : A.lvl[l];
        const uint8_t *imB = hi ? Bd->lvl[l - MSKF_LEVELS] : B.lvl[l];
        const int aw = hi ? Ad->w[l - MSKF_LEVELS] : A.w[l], ah = hi ? Ad->h[l - MSKF_LEVELS] : A.h[l];
        const int bw = hi ? Bd->w[l - MSKF_LEVELS] : B.w[l], bh = hi ? Bd->h[l - MSKF_LEVELS] : B.h[l];
        const float sc = __int_as_float((127 - l) << 23);        // 2^-l exactly
        const float pwx = ax * sc - (float)LK_HALF, pwy = ay * sc - (float)LK_HALF;
        if (l == top) { ncx = bx * sc; ncy = by * sc; }
        else { ncx = ncx * 2.0f; ncy = ncy * 2.0f; }
        int ipx = (int)floorf(pwx), ipy = (int)floorf(pwy);
        bool lvl_on = alive && !(ipx < -LK_WIN || ipx >= aw || ipy < -LK_WIN || ipy >= ah);
        if (alive && !lvl_on && l == 0) status = 0;
        if (!lvl_on) { ipx = 0; ipy = 0; }                   // idle slot: any in-range position
        int wtop, wbot;
        l4_weights(lvl_on ? pwx - (float)ipx : 0.f, lvl_on ? pwy - (float)ipy : 0.f, wtop, wbot);
        // ---- stage the template source (18 x 24 B at the window's 4-aligned left edge) and the first search region
        const int ax0 = (ipx - 1) & ~3, ay0 = ipy - 1, oxa = ipx - 1 - ax0;
        float wx = ncx - (float)LK_HALF, wy = ncy - (float)LK_HALF;
        int inx0 = (int)floorf(wx), iny0 = (int)floorf(wy);
        const bool in_b0 = !(inx0 < -LK_WIN || inx0 >= bw || iny0 < -LK_WIN || iny0 >= bh);
        if (!(lvl_on && in_b0)) { inx0 = 0; iny0 = 0; }
        int bx0 = (inx0 - 2) & ~3, by0 = iny0 - 2;
        __syncthreads();
        l4_stage<L4_TROWS>(imA, aw, ah, ax0, ay0, sT, r, true);
        l4_stage<L4_SROWS>(imB, bw, bh, bx0, by0, sS, r, true);
        __syncthreads();
        // ---- interpolated template: lane r holds source row r + 1, so V = T(row r+1) + B(row r+2) is template row r + 1;
        //      rows 0 and 16 are the extra value E of lanes 0 and 15 (source rows 0 / 17 with the top / bottom weights)
        int V[17], E[17];
        {
            uint32_t d[6], a[5];
            int pr[17];
            const uint32_t *rp = sT + (r + 1) * L4_DW;
#pragma unroll
            for (int i = 0; i < 6; ++i) d[i] = rp[i];
#pragma unroll
            for (int i = 0; i < 5; ++i) a[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], oxa);
            L4Pairs<17>::run(a, pr);
            int Bv[17];
#pragma unroll
            for (int c = 0; c < 17; ++c) { V[c] = l4_dot2k(pr[c], wtop, 256); Bv[c] = l4_dot2k(pr[c], wbot, 0); }
            // extra row: source row 0 for lane 0 (top weights, added to its own B), source row 17 for lane 15 (bottom
            // weights, added to its own T)
            const uint32_t *ep = sT + (r == 0 ? 0 : 17) * L4_DW;
#pragma unroll
            for (int i = 0; i < 6; ++i) d[i] = ep[i];
#pragma unroll
            for (int i = 0; i < 5; ++i) a[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], oxa);
            L4Pairs<17>::run(a, pr);
            const int wsel = r == 0 ? wtop : wbot;
#pragma unroll
            for (int c = 0; c < 17; ++c) E[c] = l4_dot2(pr[c], wsel, r == 0 ? Bv[c] + 256 : V[c]) >> 9;
#pragma unroll
            for (int c = 0; c < 17; ++c) V[c] = (V[c] + l4_dpp0<L4_SHL1>(Bv[c])) >> 9;
            // lane 15 is no window row: it hands template row 16 to lane 14 as "the row below"
            if (r == 15) {
#pragma unroll
                for (int c = 0; c < 17; ++c) V[c] = E[c];
            }
        }
        // ---- Scharr gradients of window row r: rows above / below from the neighbouring lanes
        int Pp[8], Ixp[8], Iyp[8];       // packed pairs (column 2m, 2m + 1); column 15 is padding (zero gradient)
        int A11 = 0, A12 = 0, A22 = 0;
        {
            int f[17], e[17];
#pragma unroll
            for (int c = 0; c < 17; ++c) {
                const int up = __builtin_amdgcn_update_dpp(E[c], V[c], L4_SHR1, 0xf, 0xf, false);   // lane 0 keeps its E = template row 0
                const int dn = l4_dpp0<L4_SHL1>(V[c]);
                f[c] = up + dn; e[c] = dn - up;
            }
            // 24-bit multiply-adds (all terms are below 2^19): the 32-bit integer multiply issues at quarter rate
            int gx[16], gy[16], pv[16];
#pragma unroll
            for (int i = 0; i < 15; ++i) {
                const int sx = l4_mad24_kv<10>(V[i + 2] - V[i], l4_mad24_k<3, 16>(f[i + 2] - f[i]));
                const int sy = l4_mad24_kv<10>(e[i + 1], l4_mad24_k<3, 16>(e[i] + e[i + 2]));
                gx[i] = sx >> 5;
                gy[i] = sy >> 5;
                pv[i] = V[i + 1];
            }
            gx[15] = 0; gy[15] = 0; pv[15] = 0;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                // lane 15 is no window row: its gradients are zero, so its pixels drop out of every sum
                const int ix = (int)__builtin_amdgcn_perm((uint32_t)gx[2 * m + 1], (uint32_t)gx[2 * m], 0x05040100u);
                const int iy = (int)__builtin_amdgcn_perm((uint32_t)gy[2 * m + 1], (uint32_t)gy[2 * m], 0x05040100u);
                Ixp[m] = winrow ? ix : 0;
                Iyp[m] = winrow ? iy : 0;
                Pp[m] = (int)__builtin_amdgcn_perm((uint32_t)pv[2 * m + 1], (uint32_t)pv[2 * m], 0x05040100u);
                A11 = l4_dot2(Ixp[m], Ixp[m], A11); A12 = l4_dot2(Ixp[m], Iyp[m], A12); A22 = l4_dot2(Iyp[m], Iyp[m], A22);
            }
        }
        const long long A11s = l4_row_sum(A11), A12s = l4_row_sum(A12), A22s = l4_row_sum(A22);
        const double a11 = lk_scaled_f64(A11s), a12 = lk_scaled_f64(A12s), a22 = lk_scaled_f64(A22s);   // (double)A * 2^-20
        double D = a11 * a22 - a12 * a12;
        const double dd = a11 - a22;
        // minEig = numer / (2 * 15 * 15) < 1e-4  <=>  numer < 0x1.70a3d70a3d70bp-5: that constant is the smallest double whose
        // quotient by 450.0 rounds to >= 1e-4 (division is monotonic), so the test is the same without dividing
        const double numer = a22 + a11 - sqrt(dd * dd + 4.0 * a12 * a12);
        bool run = lvl_on && !(numer < 0x1.70a3d70a3d70bp-5 || D < 1.1920928955078125e-07);
        if (lvl_on && !run && l == 0) status = 0;
        const bool solved = run;
        D = 1.0 / D;
        float pdx = 0.f, pdy = 0.f;
        for (int it = 0; it < LK_ITERS; ++it) {
            if (!__any(run)) break;
#ifdef LK_ITER_DBG
            if (run && !hi) dbg_iters += 1u << (8 * l);
#endif
            int inx = (int)floorf(wx), iny = (int)floorf(wy);
            if (run && (inx < -LK_WIN || inx >= bw || iny < -LK_WIN || iny >= bh)) {
                if (l == 0) status = 0;
                run = false;
            }
            int ox = inx - bx0, oy = iny - by0;
            const bool need = run && (ox < 0 || ox > L4_MAXOX || oy < 0 || oy > L4_MAXOY);
            if (__any(need)) {
                if (need) { bx0 = (inx - 2) & ~3; by0 = iny - 2; }
                __syncthreads();
                l4_stage<L4_SROWS>(imB, bw, bh, bx0, by0, sS, r, need);
                __syncthreads();
                ox = inx - bx0; oy = iny - by0;
            }
            if (!run) { ox = 0; oy = 0; }                      // idle slot: stay inside the staged region
            int wt, wb;
            l4_weights(wx - (float)inx, wy - (float)iny, wt, wb);
            uint32_t d[5], a[4];
            const uint32_t *rp = sS + l4_mad24_kv<L4_DW>(oy + r, ox >> 2);
#pragma unroll
            for (int i = 0; i < 5; ++i) d[i] = rp[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], ox & 3);
            int pr[15];
            L4Pairs<15>::run(a, pr);
            int sv[16];                                      // 512 x the bilinear sample (< 2^23, positive)
#pragma unroll
            for (int k = 0; k < 15; ++k) {
                const int t = l4_dot2k(pr[k], wt, 256), b = l4_dot2k(pr[k], wb, 0);
                sv[k] = t + l4_dpp0<L4_SHL1>(b);
            }
            sv[15] = 0;
            int b1 = 0, b2 = 0;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const l4_v2s sp = __builtin_bit_cast(l4_v2s, l4_pack_shr9(sv[2 * m], sv[2 * m + 1]));
                const int df = __builtin_bit_cast(int, (l4_v2s)(sp - __builtin_bit_cast(l4_v2s, Pp[m])));
                b1 = l4_dot2(df, Ixp[m], b1);            // masked pixels carry Ix = Iy = 0
                b2 = l4_dot2(df, Iyp[m], b2);
            }
            const long long b1s = l4_row_sum(b1), b2s = l4_row_sum(b2);
            const double db1 = lk_scaled_f64(b1s), db2 = lk_scaled_f64(b2s);
            const float dx = (float)((a12 * db2 - a22 * db1) * D);
            const float dy = (float)((a12 * db1 - a11 * db2) * D);
            if (run) {
                wx += dx; wy += dy;
                if ((double)dx * (double)dx + (double)dy * (double)dy <= 1e-4) run = false;
                else if (it > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) {
                    wx -= dx * 0.5f; wy -= dy * 0.5f;
                    run = false;
                }
                pdx = dx; pdy = dy;
            }
        }
        if (solved) { ncx = wx + (float)LK_HALF; ncy = wy + (float)LK_HALF; }
    }
    out_x = ncx; out_y = ncy; out_status = status;
}
