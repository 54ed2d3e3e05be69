// The 128 x 128 bf16 MFMA tile product shared by the CORAL and MMD kernels (coral_kernels.hip, mmd_kernels.hip).
//
// C[m][n] = sum_k P[m][k] Q[n][k] with P and Q row-major bf16 and K contiguous, so the MFMA fragments are plain
// 16-byte loads from global memory (no LDS): one tile per wavefront, 4 x NJ v_mfma_f32_32x32x16_bf16 accumulators,
// the next 32-wide K group loaded while the current one is multiplied.  Inside a K group the lane half h and element j
// of k-step s take k = 16h + 8s + j: A and B use the same permutation, so the sum is unchanged, and the two lanes of a
// row read 64 contiguous bytes per group.
// Accumulator element `reg` of acc[i][j] in lane l is C[32i + (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][32j + (l & 31)].
#pragma once
#include "common.h"

constexpr int CT = 128;          // tile edge (rows of P and of Q per job)
constexpr int KG = 32;           // K per loop iteration (two k-steps of 16)
constexpr int GN = 64;           // pixels per wavefront of the gradient products (128 x 64 tiles, tile_nt<2>)

// acc[i][j] += P[prow0 + 32i .. +32][k0:k1] . Q[qrow0 + 32j .. +32][k0:k1]^T  (rows clamped to pmax / qmax: the
// clamped rows compute values nobody stores); k1 - k0 a multiple of KG
template <int NJ>
static __device__ __forceinline__ void tile_nt(const bf16_t* __restrict__ P, size_t ldp, int prow0, int pmax,
                                               const bf16_t* __restrict__ Q, size_t ldq, int qrow0, int qmax,
                                               int k0, int k1, f32x16 (&acc)[4][NJ]) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const bf16_t* pp[4];
    const bf16_t* qp[NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        pp[i] = P + (size_t)min(prow0 + 32 * i + r, pmax) * ldp + 16 * h;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) qp[j] = Q + (size_t)min(qrow0 + 32 * j + r, qmax) * ldq + 16 * h;
    uint4 a[2][4], b[2][NJ], na[2][4], nb[2][NJ];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[s][i] = *(const uint4*)(pp[i] + k0 + 8 * s);
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[s][j] = *(const uint4*)(qp[j] + k0 + 8 * s);
    }
    for (int k = k0; k < k1; k += KG) {
        const int kn = (k + KG < k1) ? k + KG : k;      // the last iteration re-reads its own group (cached)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int i = 0; i < 4; ++i) na[s][i] = *(const uint4*)(pp[i] + kn + 8 * s);
#pragma unroll
            for (int j = 0; j < NJ; ++j) nb[s][j] = *(const uint4*)(qp[j] + kn + 8 * s);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[s][i]),
                                                                        __builtin_bit_cast(bf16x8, b[s][j]), acc[i][j], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a[s][i] = na[s][i];
#pragma unroll
            for (int j = 0; j < NJ; ++j) b[s][j] = nb[s][j];
        }
    }
}

// upper tile u of a T x T tile grid, row by row: (0,0) (0,1) .. (0,T-1) (1,1) ..
static __device__ __forceinline__ void upper_tile(int u, int T, int& I, int& J) {
    I = 0;
    while (u >= T - I) { u -= T - I; ++I; }
    J = I + u;
}
