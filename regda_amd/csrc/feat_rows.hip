// The two whole kernels the feature losses share (feat_rows.h): the fixed-order loss sum and the bf16 row norms.
#include "feat_rows.h"

__global__ void __launch_bounds__(256) rows_loss_sum_kernel(const float* __restrict__ part, int n, float* loss, float scale) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    s = block_sum4(s, red);
    if (threadIdx.x == 0) loss[0] += scale * s;
}

// lane l sums the elements 8 l + 512 t + e (e < 8) of its row in order, then the butterfly
__global__ void __launch_bounds__(256) rows_sumsq_kernel(const bf16_t* __restrict__ x, int rows, int d, float* __restrict__ out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const bf16_t* row = x + (size_t)r * d;
    float s = 0.f;
    for (int c = 8 * lane; c < d; c += 512) {
        const uint4 v = *(const uint4*)(row + c);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = __uint_as_float(w[e] << 16), hi = __uint_as_float(w[e] & 0xffff0000u);
            s += lo * lo;
            s += hi * hi;
        }
    }
    s = wave_sum(s);
    if (lane == 0) out[r] = s;
}

int rows_loss_sum(const float* part, int n, float* loss, float scale, hipStream_t st) {
    rows_loss_sum_kernel<<<1, 256, 0, st>>>(part, n, loss, scale);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

int rows_sumsq(const bf16_t* x, int rows, int d, float* out, hipStream_t st) {
    rows_sumsq_kernel<<<cdiv(rows, 4), 256, 0, st>>>(x, rows, d, out);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
