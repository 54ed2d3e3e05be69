// Category-level adversarial alignment (CLAN, Luo et al., CVPR 2019): the kernels around the discriminator of
// adv_kernels.hip.  DESIGN.md 4.2s.1.
//
//   P    [b*H*W][16] bf16     softmax(up(x1) + up(x2)), the row layout of rgda_adv_probs_fwd: what the discriminator reads
//   wmap [b*H*W] f32          1 - cos(softmax(up x1), softmax(up x2)): where the two heads disagree
//   WeightedBCEWithLogitsLoss (regda/loss.py:60-85) on the discriminator's map upsampled to the tile, weighted per pixel
//   by alpha + beta * wmap, with the gradients for the map (the transpose of the upsample) and for the weight
//
// Nothing of full size but P, wmap and the weight gradient is stored: the upsampled logits, the three softmaxes and the
// upsampled discriminator map are recomputed where they are needed.  Both transposes of the bilinear map run in gather
// form (one workgroup per low-resolution pixel over its footprint), every sum in a fixed order, no floating-point atomics.
#include "adv_rows.h"

// ---------------------------------------------------------------------------------------------- pair probabilities
// u1, u2 -> p1 = softmax(u1), p2 = softmax(u2) in place, q = softmax(u1 + u2)
template <int C>
static __device__ __forceinline__ void clan_pair(float (&p1)[C], float (&p2)[C], float (&q)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = p1[c] + p2[c];
    adv_softmax<C>(q);
    adv_softmax<C>(p1);
    adv_softmax<C>(p2);
}

// one thread per full-resolution pixel
template <int C>
__global__ void __launch_bounds__(256) clan_probs_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                             bf16_t* __restrict__ P, float* __restrict__ wmap, int b, int h,
                                                             int w, int H, int W) {
    const long long M = (long long)b * H * W;
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int X = (int)(m % W), Y = (int)((m / W) % H), n = (int)(m / ((long long)W * H));
    const Lerp ly = lerp_ac(Y, h, H), lx = lerp_ac(X, w, W);
    float p1[C], p2[C], q[C];
    adv_logits_at<C>(x1 + (size_t)n * C * h * w, h, w, ly, lx, p1);
    adv_logits_at<C>(x2 + (size_t)n * C * h * w, h, w, ly, lx, p2);
    clan_pair<C>(p1, p2, q);
    float s = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { s += p1[c] * p2[c]; a1 += p1[c] * p1[c]; a2 += p2[c] * p2[c]; }
    wmap[m] = 1.f - s / (sqrtf(a1) * sqrtf(a2));
    unsigned o[ADV_CP / 2];
#pragma unroll
    for (int c = 0; c < ADV_CP; c += 2) o[c / 2] = pack2bf(c < C ? q[c < C ? c : 0] : 0.f, c + 1 < C ? q[c + 1 < C ? c + 1 : 0] : 0.f);
    uint4* dst = (uint4*)(P + (size_t)m * ADV_CP);
    dst[0] = uint4{o[0], o[1], o[2], o[3]};
    dst[1] = uint4{o[4], o[5], o[6], o[7]};
}

// gather form, one workgroup per low-resolution pixel: over the full-resolution pixels whose footprint holds it, per head
// weight * (q (dP - <q, dP>) + p (g - <p, g>)), g the derivative of the weight map with respect to the head's probabilities
// times gw.  Per-thread sums in pixel order, then a fixed two-level LDS sum: 8 threads per accumulator add 32 partials
// each in index order, one thread adds those 8.
template <int C, bool GW>
__global__ void __launch_bounds__(256) clan_probs_bwd_kernel(const bf16_t* __restrict__ dP, const float* __restrict__ gw,
                                                             const float* __restrict__ x1, const float* __restrict__ x2,
                                                             float* __restrict__ dx1, float* __restrict__ dx2, int b, int h,
                                                             int w, int H, int W, float scale) {
    __shared__ float red[2 * C][256];
    __shared__ float red8[2 * C][8];
    const int px = blockIdx.x % w, py = (blockIdx.x / w) % h, n = blockIdx.x / (w * h);
    int y0, y1, x0, xe;
    adv_footprint(py, h, H, y0, y1);
    adv_footprint(px, w, W, x0, xe);
    const int nx = xe - x0 + 1, cnt = (y1 - y0 + 1) * nx;
    const float* xb1 = x1 + (size_t)n * C * h * w;
    const float* xb2 = x2 + (size_t)n * C * h * w;
    float acc1[C], acc2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc1[c] = acc2[c] = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int Y = y0 + i / nx, X = x0 + i % nx;
        const Lerp ly = lerp_ac(Y, h, H), lx = lerp_ac(X, w, W);
        const float wt = adv_weight_of(ly, py) * adv_weight_of(lx, px);
        if (wt == 0.f) continue;
        float p1[C], p2[C], q[C];
        adv_logits_at<C>(xb1, h, w, ly, lx, p1);
        adv_logits_at<C>(xb2, h, w, ly, lx, p2);
        clan_pair<C>(p1, p2, q);
        const size_t m = (size_t)n * H * W + (size_t)Y * W + X;
        const uint4* src = (const uint4*)(dP + m * ADV_CP);
        const uint4 v0 = src[0], v1 = src[1];
        const unsigned u[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float g = (c & 1) ? __uint_as_float(u[c / 2] & 0xffff0000u) : __uint_as_float(u[c / 2] << 16);
            dot += q[c] * g;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float g = (c & 1) ? __uint_as_float(u[c / 2] & 0xffff0000u) : __uint_as_float(u[c / 2] << 16);
            q[c] = wt * q[c] * (g - dot);           // term (a), the same for both heads
        }
        if constexpr (GW) {
            float s = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) { s += p1[c] * p2[c]; a1 += p1[c] * p1[c]; a2 += p2[c] * p2[c]; }
            // d wmap / d p1 = -(p2 / (n1 n2) - s p1 / (n1^3 n2)) and its mirror; <p1, .> of it: -(s - s a1 / a1) / (n1 n2) = 0
            // only in exact arithmetic, so the dot products are formed like any other softmax backward
            const float inv = 1.f / (sqrtf(a1) * sqrtf(a2)), k = -gw[m] * inv, r1 = s / a1, r2 = s / a2;
            float d1 = 0.f, d2 = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float g1 = k * (p2[c] - r1 * p1[c]), g2 = k * (p1[c] - r2 * p2[c]);
                d1 += p1[c] * g1;
                d2 += p2[c] * g2;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float g1 = k * (p2[c] - r1 * p1[c]), g2 = k * (p1[c] - r2 * p2[c]);
                acc1[c] += q[c] + wt * p1[c] * (g1 - d1);
                acc2[c] += q[c] + wt * p2[c] * (g2 - d2);
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) { acc1[c] += q[c]; acc2[c] += q[c]; }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) { red[c][threadIdx.x] = acc1[c]; red[C + c][threadIdx.x] = acc2[c]; }
    __syncthreads();
    const int a = threadIdx.x >> 3, j = threadIdx.x & 7;
    if (a < 2 * C) {
        float s = 0.f;
        for (int i = 0; i < 32; ++i) s += red[a][j * 32 + i];
        red8[a][j] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * C) {
        const int t = threadIdx.x;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += red8[t][i];
        float* dx = t < C ? dx1 : dx2;
        const int c = t < C ? t : t - C;
        dx[(((size_t)n * C + c) * h + py) * w + px] += scale * s;
    }
}

static int clan_probs_check(const void* P, const void* x1, const void* x2, int b, int C, int h, int w, int H, int W, int Cp) {
    if (!P || !x1 || !x2 || b < 1 || h < 1 || w < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    if (((uintptr_t)P & 15) || ((uintptr_t)x1 & 3) || ((uintptr_t)x2 & 3)) return RGDA_ERR_ARG;
    if (!class_count_ok(C) || Cp != ADV_CP) return RGDA_ERR_UNSUPPORTED;
    if (!adv_fits((long long)b * H * W, ADV_CP, 2) || !adv_fits((long long)b * C * h * w, 1, 4)) return RGDA_ERR_UNSUPPORTED;
    return RGDA_OK;
}

extern "C" int rgda_clan_probs_fwd(const float* x1, const float* x2, void* P, float* wmap, int b, int C, int h, int w, int H,
                                   int W, int Cp, rgda_stream_t stream) {
    if (!wmap || ((uintptr_t)wmap & 3)) return RGDA_ERR_ARG;
    if (int rc = clan_probs_check(P, x1, x2, b, C, h, w, H, W, Cp)) return rc;
    const unsigned grid = (unsigned)cdiv((long long)b * H * W, 256);
    hipStream_t st = to_stream(stream);
    return with_classes(C, [&](auto cc) -> int {
        constexpr int CC = decltype(cc)::value;
        clan_probs_fwd_kernel<CC><<<grid, 256, 0, st>>>(x1, x2, (bf16_t*)P, wmap, b, h, w, H, W);
        RGDA_CHECK_LAUNCH();
        return (int)RGDA_OK;
    });
}

extern "C" int rgda_clan_probs_bwd(const void* dP, const float* gw, const float* x1, const float* x2, float* dx1, float* dx2,
                                   int b, int C, int h, int w, int H, int W, int Cp, float scale, rgda_stream_t stream) {
    if (!dx1 || !dx2 || ((uintptr_t)dx1 & 3) || ((uintptr_t)dx2 & 3) || ((uintptr_t)gw & 3) || !(scale == scale)) return RGDA_ERR_ARG;
    if (int rc = clan_probs_check(dP, x1, x2, b, C, h, w, H, W, Cp)) return rc;
    if ((long long)b * h * w > 0x7fffffffLL) return RGDA_ERR_UNSUPPORTED;
    const unsigned grid = (unsigned)(b * h * w);
    hipStream_t st = to_stream(stream);
    return with_classes(C, [&](auto cc) -> int {
        constexpr int CC = decltype(cc)::value;
        if (gw) clan_probs_bwd_kernel<CC, true><<<grid, 256, 0, st>>>((const bf16_t*)dP, gw, x1, x2, dx1, dx2, b, h, w, H, W, scale);
        else clan_probs_bwd_kernel<CC, false><<<grid, 256, 0, st>>>((const bf16_t*)dP, gw, x1, x2, dx1, dx2, b, h, w, H, W, scale);
        RGDA_CHECK_LAUNCH();
        return (int)RGDA_OK;
    });
}

// ---------------------------------------------------------------------------------------------- weighted BCE
struct WbceArgs {
    const float* z;
    const float* target;
    const float* wmap;
    int b, hz, wz, H, W;
    float label, alpha, beta;
};
// the upsampled logit of full-resolution pixel (n, Y, X): the identity where the sizes agree (lerp_ac gives weight 1)
static __device__ __forceinline__ float wbce_logit_at(const WbceArgs& a, int n, const Lerp& ly, const Lerp& lx) {
    const float* q = a.z + (size_t)n * a.hz * a.wz;
    const float top = q[ly.i0 * a.wz + lx.i0] * lx.l0 + q[ly.i0 * a.wz + lx.i1] * lx.l1;
    const float bot = q[ly.i1 * a.wz + lx.i0] * lx.l0 + q[ly.i1 * a.wz + lx.i1] * lx.l1;
    return top * ly.l0 + bot * ly.l1;
}
static __device__ __forceinline__ float block_sum_256(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// one thread per full-resolution pixel: k * l into the workgroup's partial sum, the weight's gradient when asked
__global__ void __launch_bounds__(256) wbce_fwd_kernel(WbceArgs a, float kg, float* __restrict__ gw, float* __restrict__ part) {
    __shared__ float red[256];
    const long long M = (long long)a.b * a.H * a.W;
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    float v = 0.f;
    if (m < M) {
        const int X = (int)(m % a.W), Y = (int)((m / a.W) % a.H), n = (int)(m / ((long long)a.W * a.H));
        const float zu = wbce_logit_at(a, n, lerp_ac(Y, a.hz, a.H), lerp_ac(X, a.wz, a.W));
        const float t = a.target ? a.target[m] : a.label;
        const float l = fmaxf(zu, 0.f) - t * zu + log1pf(expf(-fabsf(zu)));
        v = a.wmap ? (a.alpha + a.beta * a.wmap[m]) * l : l;
        if (gw) gw[m] = kg * a.beta * l;
    }
    v = block_sum_256(v, red);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// one workgroup: the partials in a fixed order (thread i adds i, i + 256, ..; then the LDS tree)
__global__ void __launch_bounds__(256) wbce_sum_kernel(const float* __restrict__ part, int nb, float kg, float* __restrict__ loss,
                                                       int accumulate) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + kg * s;
}

// gather form of the upsample's transpose: one workgroup per pixel of z over its footprint
__global__ void __launch_bounds__(256) wbce_dz_kernel(WbceArgs a, float kg, float* __restrict__ dz) {
    __shared__ float red[256];
    const int px = blockIdx.x % a.wz, py = (blockIdx.x / a.wz) % a.hz, n = blockIdx.x / (a.wz * a.hz);
    int y0, y1, x0, x1;
    adv_footprint(py, a.hz, a.H, y0, y1);
    adv_footprint(px, a.wz, a.W, x0, x1);
    const int nx = x1 - x0 + 1, cnt = (y1 - y0 + 1) * nx;
    float acc = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int Y = y0 + i / nx, X = x0 + i % nx;
        const Lerp ly = lerp_ac(Y, a.hz, a.H), lx = lerp_ac(X, a.wz, a.W);
        const float wt = adv_weight_of(ly, py) * adv_weight_of(lx, px);
        if (wt == 0.f) continue;
        const size_t m = (size_t)n * a.H * a.W + (size_t)Y * a.W + X;
        const float zu = wbce_logit_at(a, n, ly, lx), e = expf(-fabsf(zu));
        const float t = a.target ? a.target[m] : a.label;
        const float sig = zu >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        const float k = a.wmap ? a.alpha + a.beta * a.wmap[m] : 1.f;
        acc += wt * k * (sig - t);
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) dz[blockIdx.x] = kg * acc;
}

static bool wbce_served(long long b, long long H, long long W) {
    return b >= 1 && H >= 1 && W >= 1 && H <= 0x7fffffffLL && W <= 0x7fffffffLL && b <= 0x7fffffffLL &&
           H * W <= ADV_BYTES_MAX && adv_fits(b * H * W, 1, 4);
}

extern "C" size_t rgda_wbce_logits_workspace(int b, int H, int W) {
    if (!wbce_served(b, H, W)) return 0;
    return ((size_t)cdiv((long long)b * H * W, 256) * 4 + 255) / 256 * 256;
}

extern "C" int rgda_wbce_logits(const float* z, int b, int hz, int wz, int H, int W, const float* target, float label,
                                const float* wmap, float alpha, float beta, float scale, int mean, float* loss, int accumulate,
                                float* dz, float* gw, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (!z || !loss || !ws || b < 1 || hz < 1 || wz < 1 || H < 1 || W < 1 || !(scale == scale)) return RGDA_ERR_ARG;
    if (!target && !(label == 0.f || label == 1.f)) return RGDA_ERR_ARG;
    if (wmap ? !(alpha == alpha && beta == beta) : gw != nullptr) return RGDA_ERR_ARG;       // no weight, no gradient for it
    if (((uintptr_t)z & 3) || ((uintptr_t)target & 3) || ((uintptr_t)wmap & 3) || ((uintptr_t)loss & 3) || ((uintptr_t)dz & 3) ||
        ((uintptr_t)gw & 3) || ((uintptr_t)ws & 15))
        return RGDA_ERR_ARG;
    if (!wbce_served(b, H, W) || !wbce_served(b, hz, wz)) return RGDA_ERR_UNSUPPORTED;
    if (ws_bytes < rgda_wbce_logits_workspace(b, H, W)) return RGDA_ERR_WORKSPACE;
    const long long n = (long long)b * H * W;
    const int nb = cdiv(n, 256);
    const float kg = mean ? scale / (float)n : scale;
    const WbceArgs a{z, target, wmap, b, hz, wz, H, W, label, alpha, beta};
    hipStream_t st = to_stream(stream);
    wbce_fwd_kernel<<<(unsigned)nb, 256, 0, st>>>(a, kg, gw, (float*)ws);
    RGDA_CHECK_LAUNCH();
    wbce_sum_kernel<<<1, 256, 0, st>>>((const float*)ws, nb, kg, loss, accumulate);
    RGDA_CHECK_LAUNCH();
    if (dz) {
        wbce_dz_kernel<<<(unsigned)(b * hz * wz), 256, 0, st>>>(a, kg, dz);
        RGDA_CHECK_LAUNCH();
    }
    return RGDA_OK;
}
