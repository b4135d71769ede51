// ekf_direct.hip — k_ekf_direct_update: a Kalman update of the resident covariance with up to MSKF_DIRECT_MAX_ROWS
// caller-supplied measurement rows on the IMU block (velocity, position, a zero-velocity update): the reference's
// measurementUpdate arithmetic (msckf_vio.cpp:831-904) with a caller-supplied R in place of observation_noise * I.
//
// One workgroup per stream; a stream with m = 0 leaves at once.  P is updated in place: G = H P[0:21, :] and K^T = S^-1 G
// are complete in LDS, behind a barrier, before the first element of P is written, and the downdate of an element needs
// nothing of P but the element and its transpose.
//
// The arithmetic contract (the library is built with -ffp-contract=off, every sum starts from 0.0 unless it says
// otherwise and runs in ascending index order, one rounding per operation):
//   G[a][j]  = sum_{k<21} H[a][k] * P[k][j]                                           a < m, j < d
//   S[a][b]  = (sum_{k<21} G[a][k] * H[b][k]) + R[a][b]   for b <= a, S[b][a] = S[a][b]
//   L        : Cholesky, column by column: s = S[j][j]; s -= L[j][k] * L[j][k] (k < j); s <= 0 (or NaN) -> status 2;
//              L[j][j] = sqrt(s); for i > j: s = S[i][j]; s -= L[i][k] * L[j][k] (k < j); L[i][j] = s / L[j][j]
//   y        : s = r[i]; s -= L[i][k] * y[k] (k < i); y[i] = s / L[i][i];   gamma = sum_i y[i] * y[i]
//   gate > 0 && gamma > gate -> status 0
//   K^T[:,j] : forward  w[i] = (G[i][j] - sum as above over k < i of L[i][k] * w[k]) / L[i][i]   (s = G[i][j]; s -= ...)
//              backward x[i] = (w[i] - ... L[k][i] * x[k], k = i+1 .. m-1 ascending) / L[i][i], i = m-1 .. 0;  K^T[i][j] = x[i]
//   dx[j]    = sum_a K^T[a][j] * r[a]
//   P'[i][j] = P'[j][i] = ((P[i][j] - sum_a K^T[a][i] * G[a][j]) + (P[j][i] - sum_a K^T[a][j] * G[a][i])) * 0.5
#include "ekf_device.h"

#define DU_WG 256
#define DU_TILE 32
#define DU_MAX_LD (((EKF_IMU_DIM + 6 * MAX_CLONES_DEV) + 7) / 8 * 8)      // 408
static_assert(DU_WG == DU_TILE * 8, "a thread owns four rows of a tile, eight rows apart");

__global__ __launch_bounds__(DU_WG) void k_ekf_direct_update(const EkfDirectDev *streams) {
    const EkfDirectDev &S = streams[blockIdx.x];
    const int m = S.m;
    if (m <= 0) return;
    constexpr int N = EKF_IMU_DIM, M = MSKF_DIRECT_MAX_ROWS;
    __shared__ double sH[M * N], sG[M * DU_MAX_LD], sK[M * DU_MAX_LD];
    __shared__ double sS[M * M], sL[M * M], sr[M], sy[M];
    __shared__ double sB[DU_TILE * (DU_TILE + 1)], sN[DU_TILE * (DU_TILE + 1)];
    __shared__ int s_status;
    double *P = S.P;
    const int d = S.d, tid = threadIdx.x;
    const size_t ld = (size_t)S.ld;

    for (int i = tid; i < m * N; i += DU_WG) sH[i] = S.H[i];
    if (tid < m) sr[tid] = S.r[tid];
    __syncthreads();
    // G = H P[0:21, 0:d]: a thread per column, the 21 rows of P read row-coalesced
    for (int j = tid; j < d; j += DU_WG) {
        double g[M];
#pragma unroll
        for (int a = 0; a < M; ++a) g[a] = 0.0;
        for (int k = 0; k < N; ++k) {
            const double p = P[k * ld + j];
#pragma unroll
            for (int a = 0; a < M; ++a) if (a < m) g[a] += sH[a * N + k] * p;
        }
#pragma unroll
        for (int a = 0; a < M; ++a) if (a < m) sG[a * DU_MAX_LD + j] = g[a];
    }
    __syncthreads();
    // S = G[:, 0:21] H^T + R: lower triangle, mirrored
    if (tid < M * M) {
        const int a = tid / M, b = tid - M * a;
        if (a < m && b <= a) {
            double s = 0.0;
            for (int k = 0; k < N; ++k) s += sG[a * DU_MAX_LD + k] * sH[b * N + k];
            s = s + S.R[a * m + b];
            sS[a * M + b] = s;
            sS[b * M + a] = s;
        }
    }
    __syncthreads();
    // Cholesky factor, y = L^-1 r, gamma and the gate: one thread (m <= 6)
    if (tid == 0) {
        int status = 1;
        for (int j = 0; j < m && status == 1; ++j) {
            double s = sS[j * M + j];
            for (int k = 0; k < j; ++k) s -= sL[j * M + k] * sL[j * M + k];
            if (!(s > 0.0)) { status = 2; break; }
            const double ljj = sqrt(s);
            sL[j * M + j] = ljj;
            for (int i = j + 1; i < m; ++i) {
                double t = sS[i * M + j];
                for (int k = 0; k < j; ++k) t -= sL[i * M + k] * sL[j * M + k];
                sL[i * M + j] = t / ljj;
            }
        }
        double gamma = 0.0;
        if (status == 1) {
            for (int i = 0; i < m; ++i) {
                double s = sr[i];
                for (int k = 0; k < i; ++k) s -= sL[i * M + k] * sy[k];
                sy[i] = s / sL[i * M + i];
            }
            for (int i = 0; i < m; ++i) gamma += sy[i] * sy[i];
            if (S.gate > 0.0 && gamma > S.gate) status = 0;
        }
        *S.gamma = gamma;
        *S.status = status;
        s_status = status;
    }
    __syncthreads();
    if (s_status != 1) {          // gated out or S not positive definite: P is not touched, no correction
        for (int j = tid; j < d; j += DU_WG) S.delta_x[j] = 0.0;
        if (S.pos_var_out && tid < 3) S.pos_var_out[tid] = P[(12 + tid) * ld + (12 + tid)];
        return;
    }
    // K^T = S^-1 G column by column through L, and delta_x = K r
    for (int j = tid; j < d; j += DU_WG) {
        double w[M];
        for (int i = 0; i < m; ++i) {
            double s = sG[i * DU_MAX_LD + j];
            for (int k = 0; k < i; ++k) s -= sL[i * M + k] * w[k];
            w[i] = s / sL[i * M + i];
        }
        for (int i = m - 1; i >= 0; --i) {
            double s = w[i];
            for (int k = i + 1; k < m; ++k) s -= sL[k * M + i] * w[k];
            w[i] = s / sL[i * M + i];
        }
        double dx = 0.0;
        for (int a = 0; a < m; ++a) { sK[a * DU_MAX_LD + j] = w[a]; dx += w[a] * sr[a]; }
        S.delta_x[j] = dx;
    }
    __syncthreads();              // G and K^T are complete: from here on P is written
    // P <- ((I - K H) P + ((I - K H) P)^T) / 2, tile pair (I, J) / (J, I) at a time: both tiles are read and written along
    // their rows, the transposition goes through LDS.  Thread (r0 + 8 q, c), q = 0..3, of a 32 x 32 tile.
    const int c = tid & (DU_TILE - 1), r0 = tid >> 5;
    const int nt = (d + DU_TILE - 1) / DU_TILE;
    for (int I = 0; I < nt; ++I)
        for (int J = I; J < nt; ++J) {
            double A[4];
            // this thread's elements of tile (I, J): A = P[i][j] - sum_a K^T[a][i] G[a][j]; of tile (J, I), into LDS: the same
            // expression at the transposed position, i.e. the second bracket of the contract for the element (c, r) of (I, J)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 8 * q;
                const int gi = I * DU_TILE + r, gj = J * DU_TILE + c;
                A[q] = 0.0;
                if (gi < d && gj < d) {
                    double t = 0.0;
                    for (int a = 0; a < m; ++a) t += sK[a * DU_MAX_LD + gi] * sG[a * DU_MAX_LD + gj];
                    A[q] = P[gi * ld + gj] - t;
                }
                if (I == J) sB[r * (DU_TILE + 1) + c] = A[q];
                else {
                    const int hi = J * DU_TILE + r, hj = I * DU_TILE + c;
                    double b = 0.0;
                    if (hi < d && hj < d) {
                        double t = 0.0;
                        for (int a = 0; a < m; ++a) t += sK[a * DU_MAX_LD + hi] * sG[a * DU_MAX_LD + hj];
                        b = P[hi * ld + hj] - t;
                    }
                    sB[r * (DU_TILE + 1) + c] = b;
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 8 * q;
                const int gi = I * DU_TILE + r, gj = J * DU_TILE + c;
                const double v = (A[q] + sB[c * (DU_TILE + 1) + r]) * 0.5;
                if (gi < d && gj < d) {
                    P[gi * ld + gj] = v;
                    if (gi == gj && gi >= 12 && gi < 15 && S.pos_var_out) S.pos_var_out[gi - 12] = v;      // the epilogue
                }
                if (I != J) sN[r * (DU_TILE + 1) + c] = v;
            }
            __syncthreads();
            if (I != J) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = r0 + 8 * q;
                    const int hi = J * DU_TILE + r, hj = I * DU_TILE + c;
                    if (hi < d && hj < d) P[hi * ld + hj] = sN[c * (DU_TILE + 1) + r];
                }
            }
        }
}

extern "C" void ekf_launch_direct_update(const EkfDirectDev *d, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_ekf_direct_update, dim3((unsigned)n), dim3(DU_WG), 0, st, d);
}
