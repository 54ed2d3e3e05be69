// Output-space adversarial alignment: the kernels of FCDiscriminator (regda/models/Discriminator.py:4-28) and of the
// probability rows that feed it.  DESIGN.md 4.2s.
//
//   P  [b*H*W][Cp] bf16       softmax(upsample(logits)) (or given probabilities), the C classes zero-padded to Cp = 16
//   a1 .. a4                  four 4x4 / stride 2 / pad 1 convolutions + bias + LeakyReLU, pixel-major bf16 rows
//   z  f32 [b][H/32*W/32]     the one-channel classifier: a K = 16 * 512 dot product per output pixel
//
// The two matrix kernels are implicit GEMMs on v_mfma_f32_32x32x16_bf16 whose fragments are plain 16-byte loads from global
// memory (K is contiguous in both operands: the channels of one tap), as in gram_tile.h: a wavefront owns 64 pixels x
// 32 FJ channels, the four wavefronts of a workgroup take consecutive pixel blocks and share the weight rows through L1.
// With Cp = 16 one filter tap of the first layer is exactly one K slice of the instruction.
// The data gradient runs as four parity sub-convolutions in one launch (blockIdx.z): the output pixels of one (row
// parity, column parity) class see the same 2 x 2 subset of the 16 taps, so no zero tap reaches the matrix pipe.
// Every reduction runs in a fixed order; nothing here uses floating-point atomics.
#include "adv_rows.h"

// ---------------------------------------------------------------------------------------------- probabilities
// one thread per full-resolution pixel: C interpolated logits, softmax, Cp bf16 values (32 bytes)
template <int C, int MODE>
__global__ void __launch_bounds__(256) adv_probs_fwd_kernel(const float* __restrict__ x, bf16_t* __restrict__ P, int b, int h,
                                                            int w, int H, int W) {
    const long long M = (long long)b * H * W;
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int X = (int)(m % W), Y = (int)((m / W) % H), n = (int)(m / ((long long)W * H));
    float p[C];
    if constexpr (MODE == 0) {
        const Lerp ly = lerp_ac(Y, h, H), lx = lerp_ac(X, w, W);
        adv_probs_at<C>(x + (size_t)n * C * h * w, h, w, ly, lx, p);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = x[((size_t)n * C + c) * H * W + (size_t)Y * W + X];
    }
    unsigned o[ADV_CP / 2];
#pragma unroll
    for (int c = 0; c < ADV_CP; c += 2) o[c / 2] = pack2bf(c < C ? p[c < C ? c : 0] : 0.f, c + 1 < C ? p[c + 1 < C ? c + 1 : 0] : 0.f);
    uint4* dst = (uint4*)(P + (size_t)m * ADV_CP);
    dst[0] = uint4{o[0], o[1], o[2], o[3]};
    dst[1] = uint4{o[4], o[5], o[6], o[7]};
}

// gather form: one workgroup per low-resolution pixel sums, over the full-resolution pixels whose bilinear footprint
// holds it, weight * softmax-backward(dP); per-thread partial sums in pixel order, then a fixed LDS tree
template <int C>
__global__ void __launch_bounds__(256) adv_probs_bwd_kernel(const bf16_t* __restrict__ dP, const float* __restrict__ x,
                                                            float* __restrict__ dx, int b, int h, int w, int H, int W,
                                                            float scale) {
    __shared__ float red[256];
    const int px = blockIdx.x % w, py = (blockIdx.x / w) % h, n = blockIdx.x / (w * h);
    int y0, y1, x0, x1;
    adv_footprint(py, h, H, y0, y1);
    adv_footprint(px, w, W, x0, x1);
    const int nx = x1 - x0 + 1, cnt = (y1 - y0 + 1) * nx;
    const float* xb = x + (size_t)n * C * h * w;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int Y = y0 + i / nx, X = x0 + i % nx;
        const Lerp ly = lerp_ac(Y, h, H), lx = lerp_ac(X, w, W);
        const float wt = adv_weight_of(ly, py) * adv_weight_of(lx, px);
        if (wt == 0.f) continue;
        float p[C];
        adv_probs_at<C>(xb, h, w, ly, lx, p);
        const uint4* src = (const uint4*)(dP + ((size_t)n * H * W + (size_t)Y * W + X) * ADV_CP);
        const uint4 v0 = src[0], v1 = src[1];
        const unsigned u[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        float g[C], dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            g[c] = (c & 1) ? __uint_as_float(u[c / 2] & 0xffff0000u) : __uint_as_float(u[c / 2] << 16);
            dot += p[c] * g[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += wt * p[c] * (g[c] - dot);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        red[threadIdx.x] = acc[c];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) dx[(((size_t)n * C + c) * h + py) * w + px] += scale * red[0];
        __syncthreads();
    }
}

// the pack-only mode's gradient: dx[n][c][Y][X] += scale * dP[pixel][c]
template <int C>
__global__ void __launch_bounds__(256) adv_unpack_bwd_kernel(const bf16_t* __restrict__ dP, float* __restrict__ dx, int b, int H,
                                                             int W, float scale) {
    const long long M = (long long)b * H * W;
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const long long hw = (long long)H * W;
    const int n = (int)(m / hw);
    const long long r = m % hw;
#pragma unroll
    for (int c = 0; c < C; ++c) dx[((size_t)n * C + c) * hw + r] += scale * bf2f(dP[(size_t)m * ADV_CP + c]);
}

static int adv_probs_check(const void* a, const void* b2, int b, int C, int h, int w, int H, int W, int Cp, int mode) {
    if (!a || !b2 || b < 1 || h < 1 || w < 1 || H < 1 || W < 1 || (mode != 0 && mode != 1)) return RGDA_ERR_ARG;
    if (mode == 1 && (h != H || w != W)) return RGDA_ERR_ARG;
    if (((uintptr_t)a & 15) || ((uintptr_t)b2 & 3)) return RGDA_ERR_ARG;
    if (!class_count_ok(C) || Cp != ADV_CP) return RGDA_ERR_UNSUPPORTED;
    if (!adv_fits((long long)b * H * W, ADV_CP, 2) || !adv_fits((long long)b * C * H * W, 1, 4) ||
        !adv_fits((long long)b * C * h * w, 1, 4))
        return RGDA_ERR_UNSUPPORTED;
    return RGDA_OK;
}

extern "C" int rgda_adv_probs_fwd(const float* x, void* P, int b, int C, int h, int w, int H, int W, int Cp, int mode,
                                  rgda_stream_t stream) {
    if (int rc = adv_probs_check(P, x, b, C, h, w, H, W, Cp, mode)) return rc;
    const unsigned grid = (unsigned)cdiv((long long)b * H * W, 256);
    hipStream_t st = to_stream(stream);
    return with_classes(C, [&](auto cc) -> int {
        constexpr int CC = decltype(cc)::value;
        if (mode == 0) adv_probs_fwd_kernel<CC, 0><<<grid, 256, 0, st>>>(x, (bf16_t*)P, b, h, w, H, W);
        else adv_probs_fwd_kernel<CC, 1><<<grid, 256, 0, st>>>(x, (bf16_t*)P, b, h, w, H, W);
        RGDA_CHECK_LAUNCH();
        return (int)RGDA_OK;
    });
}

extern "C" int rgda_adv_probs_bwd(const void* dP, const float* x, float* dx, int b, int C, int h, int w, int H, int W, int Cp,
                                  int mode, float scale, rgda_stream_t stream) {
    if (!dx || (mode == 0 && !x) || !(scale == scale)) return RGDA_ERR_ARG;
    if (int rc = adv_probs_check(dP, dx, b, C, h, w, H, W, Cp, mode)) return rc;
    if ((long long)b * h * w > 0x7fffffffLL) return RGDA_ERR_UNSUPPORTED;
    hipStream_t st = to_stream(stream);
    return with_classes(C, [&](auto cc) -> int {
        constexpr int CC = decltype(cc)::value;
        if (mode == 0) adv_probs_bwd_kernel<CC><<<(unsigned)(b * h * w), 256, 0, st>>>((const bf16_t*)dP, x, dx, b, h, w, H, W, scale);
        else adv_unpack_bwd_kernel<CC><<<(unsigned)cdiv((long long)b * H * W, 256), 256, 0, st>>>((const bf16_t*)dP, dx, b, H, W, scale);
        RGDA_CHECK_LAUNCH();
        return (int)RGDA_OK;
    });
}

// ---------------------------------------------------------------------------------------------- convolutions
static __device__ __forceinline__ bf16x8 adv_frag(const bf16_t* p, bool ok) {
    uint4 v = ok ? *(const uint4*)p : uint4{0u, 0u, 0u, 0u};
    return __builtin_bit_cast(bf16x8, v);
}

// y[m][co] = lrelu(bias[co] + sum_{tap, ci} x[src(m, tap)][ci] * wgt[co][tap][ci]),  src = (2 ho - 1 + kh, 2 wo - 1 + kw).
// K16: Cin == 16, a tap is one k step (lane half h holds channels 8h .. 8h+7); otherwise Cin % 32 == 0 and inside a
// 32-channel group half h, step s hold channels 16h + 8s .. (the same permutation in both operands).
template <int FJ, bool K16>
__global__ void __launch_bounds__(256) disc_conv_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wgt,
                                                            const float* __restrict__ bias, bf16_t* __restrict__ y, int N, int H,
                                                            int W, int Cin, int Cout, float slope) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hf = lane >> 5;
    const int Ho = H >> 1, Wo = W >> 1, M = N * Ho * Wo;
    const int m0 = (blockIdx.x * 4 + wave) * 64;
    if (m0 >= M) return;
    const int co0 = blockIdx.y * 32 * FJ;
    const int koff = K16 ? 8 * hf : 16 * hf;
    int pn[2], py[2], px[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = min(m0 + 32 * i + r, M - 1);
        pn[i] = m / (Ho * Wo);
        const int rem = m % (Ho * Wo);
        py[i] = (rem / Wo) * 2 - 1;
        px[i] = (rem % Wo) * 2 - 1;
    }
    const bf16_t* wp[FJ];
#pragma unroll
    for (int j = 0; j < FJ; ++j) wp[j] = wgt + (size_t)(co0 + 32 * j + r) * 16 * Cin + koff;
    f32x16 acc[2][FJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    for (int tap = 0; tap < 16; ++tap) {
        const int kh = tap >> 2, kw = tap & 3;
        const bf16_t* ap[2];
        bool ok[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int hi = py[i] + kh, wi = px[i] + kw;
            ok[i] = hi >= 0 && hi < H && wi >= 0 && wi < W;
            ap[i] = x + (ok[i] ? ((size_t)(pn[i] * H + hi) * W + wi) * Cin : (size_t)0) + koff;
        }
        if constexpr (K16) {
            bf16x8 a[2], bq[FJ];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = adv_frag(ap[i], ok[i]);
#pragma unroll
            for (int j = 0; j < FJ; ++j) bq[j] = adv_frag(wp[j] + tap * 16, true);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < FJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], bq[j], acc[i][j], 0, 0, 0);
        } else {
            const int wo = tap * Cin;
            for (int c0 = 0; c0 < Cin; c0 += 32) {
                bf16x8 a[2][2], bq[2][FJ];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) a[s][i] = adv_frag(ap[i] + c0 + 8 * s, ok[i]);
#pragma unroll
                    for (int j = 0; j < FJ; ++j) bq[s][j] = adv_frag(wp[j] + wo + c0 + 8 * s, true);
                }
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < FJ; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][i], bq[s][j], acc[i][j], 0, 0, 0);
            }
        }
    }
    // accumulator element e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31
#pragma unroll
    for (int j = 0; j < FJ; ++j) {
        const int co = co0 + 32 * j + r;
        const float bv = bias ? bias[co] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * hf;
                if (m < M) {
                    float v = acc[i][j][e] + bv;
                    v = v > 0.f ? v : v * slope;
                    y[(size_t)m * Cout + co] = f2bf(v);
                }
            }
    }
}

// dx[n, hi, wi][ci] = mask * sum_{(kh, kw) of the pixel's parity class, co} dy[n, ho, wo][co] * wt[ci][kh * 4 + kw][co]
// with ho = (hi + 1 - kh) / 2, wo = (wi + 1 - kw) / 2; mask = below > 0 ? 1 : slope (below: the stored activation this
// gradient flows into, NULL for the probability rows).  blockIdx.z = 2 * (hi & 1) + (wi & 1).
template <int FI, int FJ>
__global__ void __launch_bounds__(256) disc_conv_bwd_data_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ wt,
                                                                 const bf16_t* __restrict__ below, bf16_t* __restrict__ dx, int N,
                                                                 int H, int W, int Cin, int Cout, float slope) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hf = lane >> 5;
    const int Ho = H >> 1, Wo = W >> 1, Mq = N * Ho * Wo;       // pixels of one parity class
    const int ph = blockIdx.z >> 1, pw = blockIdx.z & 1;
    const int m0 = (blockIdx.x * 4 + wave) * 32 * FI;
    if (m0 >= Mq) return;
    const int ci0 = blockIdx.y * 32 * FJ;
    int pn[FI], h2[FI], w2[FI];
#pragma unroll
    for (int i = 0; i < FI; ++i) {
        const int q = min(m0 + 32 * i + r, Mq - 1);
        pn[i] = q / (Ho * Wo);
        const int rem = q % (Ho * Wo);
        h2[i] = rem / Wo;
        w2[i] = rem % Wo;
    }
    const bf16_t* wp[FJ];
#pragma unroll
    for (int j = 0; j < FJ; ++j) wp[j] = wt + (size_t)min(ci0 + 32 * j + r, Cin - 1) * 16 * Cout + 16 * hf;
    f32x16 acc[FI][FJ];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        // even rows take kh = 1 (ho = hi / 2) and kh = 3 (ho = hi / 2 - 1); odd rows kh = 0 (ho = (hi + 1) / 2) and kh = 2
        const int ta = t >> 1, tb = t & 1;
        const int kh = (ph ? 0 : 1) + 2 * ta, kw = (pw ? 0 : 1) + 2 * tb;
        const int dh = ph ? 1 - ta : -ta, dw = pw ? 1 - tb : -tb;
        const bf16_t* ap[FI];
        bool ok[FI];
#pragma unroll
        for (int i = 0; i < FI; ++i) {
            const int ho = h2[i] + dh, wo = w2[i] + dw;
            ok[i] = ho >= 0 && ho < Ho && wo >= 0 && wo < Wo;
            ap[i] = dy + (ok[i] ? ((size_t)(pn[i] * Ho + ho) * Wo + wo) * Cout : (size_t)0) + 16 * hf;
        }
        const int wo_ = (kh * 4 + kw) * Cout;
        for (int c0 = 0; c0 < Cout; c0 += 32) {
            bf16x8 a[2][FI], bq[2][FJ];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int i = 0; i < FI; ++i) a[s][i] = adv_frag(ap[i] + c0 + 8 * s, ok[i]);
#pragma unroll
                for (int j = 0; j < FJ; ++j) bq[s][j] = adv_frag(wp[j] + wo_ + c0 + 8 * s, true);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int i = 0; i < FI; ++i)
#pragma unroll
                    for (int j = 0; j < FJ; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][i], bq[s][j], acc[i][j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int q = m0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * hf;
            if (q >= Mq) continue;
            const int n = q / (Ho * Wo), rem = q % (Ho * Wo);
            const size_t p = ((size_t)(n * H + 2 * (rem / Wo) + ph)) * W + 2 * (rem % Wo) + pw;
#pragma unroll
            for (int j = 0; j < FJ; ++j) {
                const int ci = ci0 + 32 * j + r;
                if (ci < Cin) {
                    float v = acc[i][j][e];
                    if (below) v *= (bf2f(below[p * Cin + ci]) > 0.f) ? 1.f : slope;
                    dx[p * Cin + ci] = f2bf(v);
                }
            }
        }
}

static int disc_conv_check(const void* p0, const void* p1, const void* p2, int N, int H, int W, int Cin, int Cout, float slope) {
    if (!p0 || !p1 || !p2 || N < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || Cin < 1 || Cout < 1 || !(slope == slope))
        return RGDA_ERR_ARG;
    if (((uintptr_t)p0 & 15) || ((uintptr_t)p1 & 15) || ((uintptr_t)p2 & 15)) return RGDA_ERR_ARG;
    if ((Cin != ADV_CP && (Cin % 32)) || (Cout % 32)) return RGDA_ERR_UNSUPPORTED;
    const long long M = (long long)N * H * W;
    if (!adv_fits(M, Cin, 2) || !adv_fits(M / 4, Cout, 2) || !adv_fits((long long)Cout * 16, Cin, 2)) return RGDA_ERR_UNSUPPORTED;
    return RGDA_OK;
}

extern "C" int rgda_disc_conv_fwd(const void* x, const void* wgt, const float* bias, void* y, int N, int H, int W, int Cin,
                                  int Cout, float slope, rgda_stream_t stream) {
    if (int rc = disc_conv_check(x, wgt, y, N, H, W, Cin, Cout, slope)) return rc;
    const int M = N * (H / 2) * (W / 2);
    hipStream_t st = to_stream(stream);
    const bool two = (Cout % 64) == 0;
    const dim3 grid(cdiv(M, 256), Cout / (two ? 64 : 32));
#define ADV_FWD(FJ, K16) \
    disc_conv_fwd_kernel<FJ, K16><<<grid, 256, 0, st>>>((const bf16_t*)x, (const bf16_t*)wgt, bias, (bf16_t*)y, N, H, W, Cin, Cout, slope)
    if (Cin == ADV_CP) { if (two) ADV_FWD(2, true); else ADV_FWD(1, true); }
    else { if (two) ADV_FWD(2, false); else ADV_FWD(1, false); }
#undef ADV_FWD
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_disc_conv_bwd_data(const void* dy, const void* wt, const void* below, void* dx, int N, int H, int W, int Cin,
                                       int Cout, float slope, rgda_stream_t stream) {
    if (int rc = disc_conv_check(dx, wt, dy, N, H, W, Cin, Cout, slope)) return rc;
    if (below && ((uintptr_t)below & 1)) return RGDA_ERR_ARG;
    const int Mq = N * (H / 2) * (W / 2);
    hipStream_t st = to_stream(stream);
    const bool two = (Cin % 64) == 0;
    // FI = 2: a wavefront owns 64 pixels of one parity class.  (FI = 4, 128 pixels and 6 fragment loads per 8 MFMAs instead
    // of 4 per 4, measured SLOWER at 8 x 512 x 512: layer 2 190 -> 262 us, layer 3 154 -> 173 us; the kernel waits for its
    // loads, and the larger tile halves the wavefronts that hide them.)
    const dim3 grid(cdiv(Mq, 256), cdiv(Cin, two ? 64 : 32), 4);
#define ADV_BWD(FI, FJ) \
    disc_conv_bwd_data_kernel<FI, FJ><<<grid, 256, 0, st>>>((const bf16_t*)dy, (const bf16_t*)wt, (const bf16_t*)below, (bf16_t*)dx, N, H, W, Cin, Cout, slope)
    if (two) ADV_BWD(2, 2); else ADV_BWD(2, 1);
#undef ADV_BWD
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

// y = bf16(lrelu(y + bias)) in place on bf16 rows [M][C]: the epilogue pass behind rgda_conv2d where the generic kernel
// forms the matrix product (layers 2-4 of the discriminator's forward); eight channels per thread
__global__ void __launch_bounds__(256) disc_bias_lrelu_kernel(bf16_t* __restrict__ y, const float* __restrict__ bias, long long n8,
                                                              int C, float slope) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const int c = (int)((i * 8) % C);
    uint4 v = ((const uint4*)y)[i];
    unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float lo = __uint_as_float(u[e] << 16) + bias[c + 2 * e], hi = __uint_as_float(u[e] & 0xffff0000u) + bias[c + 2 * e + 1];
        lo = lo > 0.f ? lo : lo * slope;
        hi = hi > 0.f ? hi : hi * slope;
        u[e] = pack2bf(lo, hi);
    }
    ((uint4*)y)[i] = uint4{u[0], u[1], u[2], u[3]};
}

extern "C" int rgda_disc_bias_lrelu(void* y, const float* bias, int64_t M, int C, float slope, rgda_stream_t stream) {
    if (!y || !bias || M < 1 || C < 1 || ((uintptr_t)y & 15) || !(slope == slope)) return RGDA_ERR_ARG;
    if ((C % 32) || !adv_fits(M, C, 2)) return RGDA_ERR_UNSUPPORTED;
    const long long n8 = M * C / 8;
    disc_bias_lrelu_kernel<<<(unsigned)cdiv(n8, 256), 256, 0, to_stream(stream)>>>((bf16_t*)y, bias, n8, C, slope);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

// ---------------------------------------------------------------------------------------------- bias gradient
// db[c] = sum_m g[m][c]: workgroup (k, cb) sums rows k * R .. of 32 channels (8 row phases per channel, joined in phase
// order), the second kernel adds the nb partials in block order
#define ADV_BIAS_ROWS 2048
__global__ void __launch_bounds__(256) disc_bias_partial_kernel(const bf16_t* __restrict__ g, long long M, int C,
                                                                float* __restrict__ part) {
    __shared__ float red[8][32];
    const int cl = threadIdx.x & 31, phs = threadIdx.x >> 5, c = blockIdx.y * 32 + cl;
    const long long r0 = (long long)blockIdx.x * ADV_BIAS_ROWS, r1 = min(r0 + ADV_BIAS_ROWS, M);
    float s = 0.f;
    for (long long m = r0 + phs; m < r1; m += 8) s += bf2f(g[(size_t)m * C + c]);
    red[phs][cl] = s;
    __syncthreads();
    if (phs == 0) {
#pragma unroll
        for (int k = 1; k < 8; ++k) s += red[k][cl];
        part[(size_t)blockIdx.x * C + c] = s;
    }
}
__global__ void __launch_bounds__(256) disc_bias_final_kernel(const float* __restrict__ part, int nb, int C, float* __restrict__ db) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int k = 0; k < nb; ++k) s += part[(size_t)k * C + c];
    db[c] = s;
}

extern "C" size_t rgda_disc_bias_grad_workspace(int64_t M, int C) {
    if (M < 1 || C < 32 || (C % 32) || !adv_fits(M, C, 2)) return 0;
    return ((size_t)cdiv(M, ADV_BIAS_ROWS) * C * 4 + 255) / 256 * 256;
}

extern "C" int rgda_disc_bias_grad(const void* g, int64_t M, int C, float* db, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (!g || !db || !ws || M < 1 || C < 1 || ((uintptr_t)ws & 15)) return RGDA_ERR_ARG;
    if ((C % 32) || !adv_fits(M, C, 2)) return RGDA_ERR_UNSUPPORTED;
    if (ws_bytes < rgda_disc_bias_grad_workspace(M, C)) return RGDA_ERR_WORKSPACE;
    const int nb = cdiv(M, ADV_BIAS_ROWS);
    hipStream_t st = to_stream(stream);
    disc_bias_partial_kernel<<<dim3(nb, C / 32), 256, 0, st>>>((const bf16_t*)g, M, C, (float*)ws);
    RGDA_CHECK_LAUNCH();
    disc_bias_final_kernel<<<cdiv(C, 256), 256, 0, st>>>((const float*)ws, nb, C, db);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

// ---------------------------------------------------------------------------------------------- head (512 -> 1) and BCE
// one wavefront per output pixel; w f32 [16 taps][C]
__global__ void __launch_bounds__(64) disc_head_fwd_kernel(const bf16_t* __restrict__ a, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ z, int H, int W,
                                                           int C) {
    const int Ho = H >> 1, Wo = W >> 1;
    const int wo = blockIdx.x % Wo, ho = (blockIdx.x / Wo) % Ho, n = blockIdx.x / (Wo * Ho);
    float s = 0.f;
    for (int tap = 0; tap < 16; ++tap) {
        const int hi = 2 * ho - 1 + (tap >> 2), wi = 2 * wo - 1 + (tap & 3);
        if (hi < 0 || hi >= H || wi < 0 || wi >= W) continue;
        const bf16_t* ap = a + ((size_t)(n * H + hi) * W + wi) * C;
        const float* wq = w + (size_t)tap * C;
        for (int c = threadIdx.x * 8; c < C; c += 512) {
            const uint4 v = *(const uint4*)(ap + c);
            const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                s += __uint_as_float(u[e] << 16) * wq[c + 2 * e] + __uint_as_float(u[e] & 0xffff0000u) * wq[c + 2 * e + 1];
        }
    }
    s = wave_sum(s);
    if (threadIdx.x == 0) z[blockIdx.x] = s + (bias ? bias[0] : 0.f);
}

// da[n, hi, wi][c] = mask(a) * sum over the (at most four) outputs that read the pixel of dz * w[tap][c]
__global__ void __launch_bounds__(256) disc_head_bwd_data_kernel(const float* __restrict__ dz, const bf16_t* __restrict__ a,
                                                                 const float* __restrict__ w, bf16_t* __restrict__ da, int N, int H,
                                                                 int W, int C, float slope) {
    const long long total = (long long)N * H * W * C;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const long long p = i / C;
    const int wi = (int)(p % W), hi = (int)((p / W) % H), n = (int)(p / ((long long)W * H));
    const int Ho = H >> 1, Wo = W >> 1;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int kh = ((hi & 1) ? 0 : 1) + 2 * (t >> 1), kw = ((wi & 1) ? 0 : 1) + 2 * (t & 1);
        const int ho = (hi + 1 - kh) / 2, wo = (wi + 1 - kw) / 2;
        if (hi + 1 - kh < 0 || ho >= Ho || wi + 1 - kw < 0 || wo >= Wo) continue;
        s += dz[(size_t)(n * Ho + ho) * Wo + wo] * w[(kh * 4 + kw) * C + c];
    }
    da[i] = f2bf(s * ((bf2f(a[i]) > 0.f) ? 1.f : slope));
}

// dw[tap][c] = sum_{n, ho, wo} dz * a[src(tap)][c]: a workgroup owns 16 channels of one tap; thread (phase, channel) adds the
// outputs phase, phase + 16, .. in index order and the 16 phases are joined in phase order.  The last workgroup sums dz
// into db (per-thread strided sums, then a fixed LDS tree).
__global__ void __launch_bounds__(256) disc_head_bwd_param_kernel(const float* __restrict__ dz, const bf16_t* __restrict__ a,
                                                                  float* __restrict__ dw, float* __restrict__ db, int N, int H,
                                                                  int W, int C) {
    __shared__ float red[256];
    const int Ho = H >> 1, Wo = W >> 1, nz = N * Ho * Wo;
    if (blockIdx.x == gridDim.x - 1) {
        float s = 0.f;
        for (int i = threadIdx.x; i < nz; i += 256) s += dz[i];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int k = 128; k > 0; k >>= 1) {
            if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
            __syncthreads();
        }
        if (threadIdx.x == 0) db[0] = red[0];
        return;
    }
    const int cl = threadIdx.x & 15, phs = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + cl;           // element (tap, c) of dw; C % 16 == 0: a workgroup stays inside one tap
    const int c = i % C, tap = i / C, kh = tap >> 2, kw = tap & 3;
    float s = 0.f;
    for (int q = phs; q < nz; q += 16) {
        const int wo = q % Wo, ho = (q / Wo) % Ho, n = q / (Wo * Ho);
        const int hi = 2 * ho - 1 + kh, wi = 2 * wo - 1 + kw;
        if (hi < 0 || hi >= H || wi < 0 || wi >= W) continue;
        s += dz[q] * bf2f(a[((size_t)(n * H + hi) * W + wi) * C + c]);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (phs == 0) {
#pragma unroll
        for (int k = 1; k < 16; ++k) s += red[k * 16 + cl];
        dw[i] = s;
    }
}

static int disc_head_check(const void* a, const void* w, const void* z, int N, int H, int W, int C) {
    if (!a || !w || !z || N < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 1) return RGDA_ERR_ARG;
    if (((uintptr_t)a & 15) || ((uintptr_t)w & 3) || ((uintptr_t)z & 3)) return RGDA_ERR_ARG;
    if ((C % 32) || !adv_fits((long long)N * H * W, C, 2)) return RGDA_ERR_UNSUPPORTED;
    return RGDA_OK;
}

extern "C" int rgda_disc_head_fwd(const void* a4, const float* w, const float* bias, float* z, int N, int H, int W, int C,
                                  rgda_stream_t stream) {
    if (int rc = disc_head_check(a4, w, z, N, H, W, C)) return rc;
    disc_head_fwd_kernel<<<(unsigned)(N * (H / 2) * (W / 2)), 64, 0, to_stream(stream)>>>((const bf16_t*)a4, w, bias, z, H, W, C);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_disc_head_bwd(const float* dz, const void* a4, const float* w, void* da4, float* dw, float* db, int N, int H,
                                  int W, int C, float slope, rgda_stream_t stream) {
    if (int rc = disc_head_check(a4, w, dz, N, H, W, C)) return rc;
    if ((!da4 && !dw) || (!dw != !db) || !(slope == slope) || ((uintptr_t)da4 & 1)) return RGDA_ERR_ARG;
    hipStream_t st = to_stream(stream);
    if (da4) {
        disc_head_bwd_data_kernel<<<(unsigned)cdiv((long long)N * H * W * C, 256), 256, 0, st>>>(dz, (const bf16_t*)a4, w, (bf16_t*)da4,
                                                                                                N, H, W, C, slope);
        RGDA_CHECK_LAUNCH();
    }
    if (dw) {
        disc_head_bwd_param_kernel<<<(unsigned)(C + 1), 256, 0, st>>>(dz, (const bf16_t*)a4, dw, db, N, H, W, C);
        RGDA_CHECK_LAUNCH();
    }
    return RGDA_OK;
}

// loss (+)= scale * mean(softplus(z) - t z) in the stable form max(z, 0) - t z + log1p(exp(-|z|));
// dz = scale / n * (sigmoid(z) - t) when asked.  One workgroup: strided per-thread sums, a fixed LDS tree.
__global__ void __launch_bounds__(256) bce_logits_kernel(const float* __restrict__ z, int n, float t, float scale,
                                                         float* __restrict__ loss, int accumulate, float* __restrict__ dz) {
    __shared__ float red[256];
    const float k = scale / (float)n;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = z[i], e = expf(-fabsf(v));
        s += fmaxf(v, 0.f) - t * v + log1pf(e);
        if (dz) dz[i] = k * ((v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e)) - t);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int q = 128; q > 0; q >>= 1) {
        if ((int)threadIdx.x < q) red[threadIdx.x] += red[threadIdx.x + q];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.f) + k * red[0];
}

extern "C" int rgda_bce_logits(const float* z, int n, float label, float scale, float* loss, int accumulate, float* dz,
                               rgda_stream_t stream) {
    if (!z || !loss || n < 1 || !(label == 0.f || label == 1.f) || !(scale == scale)) return RGDA_ERR_ARG;
    bce_logits_kernel<<<1, 256, 0, to_stream(stream)>>>(z, n, label, scale, loss, accumulate, dz);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
