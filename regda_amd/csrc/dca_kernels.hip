// Deep Covariance Alignment (regda/dca_modules.py:20-188: CategoryAlign_Module, ICR, CCR, MSE_intra, MSE_cross): forward +
// feature gradient in one call.  The (b, C, c, hw) product of get_context is never formed and the class probabilities are
// never written: both hot passes form them from the logits in registers.  Deterministic (no floating-point atomics, every
// sum in an order the launch geometry fixes).  The arithmetic contract is written next to rgda_dca_loss in
// include/rgda_hip.h.
//
//   context: one workgroup per (image, 64-channel tile) walks all pixels of its image once: per 128 pixels P -> LDS (one
//            pixel per thread) and the f32 feature tile -> LDS (read coalesced along the pixels; the next tile and its
//            logits already in flight), then wavefront q takes 32 of the 128 pixels: S (16 classes x 64 channels) += P x tile on
//            the fp32 MFMA 16 x 16 x 4, both operands from LDS, conflict-free.  The four wavefronts are combined as
//            (q0 + q1) + (q2 + q3); v = S / Z, the norm over the CLASS axis and u follow in the same workgroup, which
//            owns every class of its channels                                                  dca_context_kernel
//   cov    : m = mean_b u per side, centred over the channels, with the centred sum of squares  dca_center_kernel
//            R[i][j], one workgroup per entry                                                   dca_corr_kernel
//            L and W = dL/dR, one workgroup; loss[0] += weight * L                              dca_cov_loss_kernel
//            dL/dm of one side, one workgroup per class row                                     dca_cov_dmean_kernel
//   table  : per (image, channel): dL/du (cov: dL/dm / b; mse: +-2 (u1 - u2) / (b n c)), back through the normalisation
//            over the classes and the division by Z -> G[b][C][c]; mse: the squared differences as one partial per
//            workgroup for rows_loss_sum                                                        dca_table_kernel
//   grad   : one workgroup per (64 pixels, 256 channels, image): P again from the logits, a thread holds G of four
//            consecutive channels for every class in registers -> store4_bf16                   dca_grad_kernel
#include "feat_rows.h"

namespace {

constexpr int DC_PX = 128;       // pixels of one feature tile of the context pass
constexpr int DC_GPX = 64;       // pixels of one gradient workgroup
constexpr int DC_CH = 64;        // channels of one context workgroup
constexpr int DC_GCH = 256;      // channels of one gradient workgroup
constexpr int DC_CP = 16;        // classes of one LDS row of probabilities
constexpr float DC_EPS = 1e-12f; // F.normalize
constexpr float DC_LOW = 1e-6f;  // regularize: max(R_ij, 1e-6)

enum { DC_PROB = 0, DC_LOGITS = 1, DC_LOGITS2 = 2 };
enum { DC_COV = 0, DC_MSE = 1 };

struct Pred {
    const float* p1;
    const float* p2;
    int kind;
};

// the logits (or probabilities) of pixel p of image b: planes (b, C, hw), contiguous; l2 with two maps only
template <int C>
__device__ __forceinline__ void load_logits(const Pred& pr, int b, int p, int hw, float (&l1)[C], float (&l2)[C]) {
    const bool in = p < hw;
    const size_t base = (size_t)b * C * hw + (in ? p : 0);
#pragma unroll
    for (int k = 0; k < C; ++k) {
        l1[k] = in ? pr.p1[base + (size_t)k * hw] : 0.f;
        l2[k] = in && pr.kind == DC_LOGITS2 ? pr.p2[base + (size_t)k * hw] : 0.f;
    }
}
template <int C>
__device__ __forceinline__ void softmax_of(const float (&l)[C], float (&P)[C]) {
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < C; ++k) m = fmaxf(m, l[k]);
    // every workgroup of an image forms these again, on the critical path of its tile loop: the hardware exp2 and one
    // reciprocal per pixel (a library exp and a division per class cost more than the MFMAs of the tile)
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        P[k] = __expf(l[k] - m);
        s += P[k];
    }
    const float inv = __builtin_amdgcn_rcpf(s);
#pragma unroll
    for (int k = 0; k < C; ++k) P[k] = __fmul_rn(P[k], inv);
}
// the C probabilities of a pixel from what load_logits read; a pixel outside the image: zeros
template <int C>
__device__ __forceinline__ void probs_from(int kind, bool in, const float (&l1)[C], const float (&l2)[C], float (&P)[C]) {
    if (!in) {
#pragma unroll
        for (int k = 0; k < C; ++k) P[k] = 0.f;
        return;
    }
    if (kind == DC_PROB) {
#pragma unroll
        for (int k = 0; k < C; ++k) P[k] = l1[k];
        return;
    }
    softmax_of<C>(l1, P);
    if (kind == DC_LOGITS2) {
        float Q[C];
        softmax_of<C>(l2, Q);
#pragma unroll
        for (int k = 0; k < C; ++k) P[k] = __fmul_rn(__fadd_rn(P[k], Q[k]), 0.5f);
    }
}

struct DcPlan {
    int n;
    size_t off_u[2], off_nrm[2], off_z[2], off_g[2], off_cen, off_dm, off_small, off_part, bytes;
    int parts;
};

DcPlan make_plan(int ba, int bb, int c, int C, int ignore_bg) {
    DcPlan p;
    p.n = ignore_bg ? C - 1 : C;
    const int bs[2] = {ba, bb};
    size_t o = 256;
    for (int s = 0; s < 2; ++s) {
        p.off_u[s] = o;    o += a256((size_t)4 * bs[s] * p.n * c);
        p.off_nrm[s] = o;  o += a256((size_t)4 * bs[s] * c);
        p.off_z[s] = o;    o += a256((size_t)4 * bs[s] * C);
        p.off_g[s] = o;    o += a256((size_t)4 * bs[s] * C * c);
    }
    p.off_cen = o;    o += a256((size_t)8 * p.n * c);
    p.off_dm = o;     o += a256((size_t)8 * p.n * c);
    p.off_small = o;  o += a256((size_t)4 * (2 * p.n + 2 * p.n * p.n));
    p.parts = cdiv(c, 256) * (ba > bb ? ba : bb);
    p.off_part = o;   o += a256((size_t)4 * p.parts);
    p.bytes = o;
    return p;
}

}  // namespace

// grid (ceil(c / 64), b).  u, v: (b, n, c) with n = C - (ignore_bg ? 1 : 0); Z: (b, C); nrm: (b, c), the norm over the
// classes before its clamp.  v, Z, nrm optional.  Per 128 pixels: the tile (32 loads per thread) and the logits of the
// NEXT 128 pixels are in flight in registers while the MFMAs run on the current ones.
template <int C>
__global__ void __launch_bounds__(256) dca_context_kernel(FeatView f, Pred pr, int c, int ignore_bg, float* __restrict__ u,
                                                          float* __restrict__ v, float* __restrict__ Z,
                                                          float* __restrict__ nrm) {
    __shared__ float Ps[DC_PX * DC_CP];              // [pixel][class]
    __shared__ float tile[DC_CH][DC_PX + 4];         // rows 4 mod 64 apart: the MFMA operand read (16 channels x 4 pixels) hits
                                                     // 64 banks; afterwards the partials [wavefront][class][channel]
    __shared__ float zred[4][DC_CP];
    const int b = blockIdx.y, c0 = blockIdx.x * DC_CH, hw = f.hw;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* fb = f.x + (size_t)b * f.ldb;
    // acc[j][r]: class 4 (lane / 16) + r, channel c0 + 16 j + lane % 16, over this wavefront's pixels
    f32x4 acc[4];
    float z[C], l1[C], l2[C], r[32];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < C; ++k) z[k] = 0.f;
    const int lr = lane & 15, lq = lane >> 4;
    auto load = [&](int p0) {                        // wavefront w: the channels w + 4 i, the pixels p0 + lane and + 64
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ch = c0 + w + 4 * i;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int p = p0 + 64 * hf + lane;
                r[2 * i + hf] = (ch < c && p < hw) ? fb[(size_t)ch * f.ldc + p] : 0.f;
            }
        }
        if (tid < DC_PX) load_logits<C>(pr, b, p0 + tid, hw, l1, l2);
    };
    const int nsub = (hw + DC_PX - 1) / DC_PX;
    load(0);
    for (int s = 0; s < nsub; ++s) {
        if (tid < DC_PX) {                           // the probabilities of these 128 pixels, one pixel per thread
            float P[C];
            probs_from<C>(pr.kind, s * DC_PX + tid < hw, l1, l2, P);
#pragma unroll
            for (int k = 0; k < C; ++k) {
                Ps[tid * DC_CP + k] = P[k];
                z[k] += P[k];
            }
#pragma unroll
            for (int k = C; k < DC_CP; ++k) Ps[tid * DC_CP + k] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            tile[w + 4 * i][lane] = r[2 * i];
            tile[w + 4 * i][64 + lane] = r[2 * i + 1];
        }
        __syncthreads();
        if (s + 1 < nsub) load((s + 1) * DC_PX);
        // A = P (class lr, pixel lq of four), B = the tile (pixel lq, channel 16 j + lr): pixels w * 32 + 4 kk + lq
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int pl = w * 32 + 4 * kk + lq;
            const float a = Ps[pl * DC_CP + lr];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, tile[16 * j + lr][pl], acc[j], 0, 0, 0);
        }
        __syncthreads();
    }
    float* comb = &tile[0][0];
    // Z: a butterfly per wavefront, then (w0 + w1) + (w2 + w3)
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const float t = wave_sum(z[k]);
        if (lane == 0) zred[w][k] = t;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) comb[(w * DC_CP + 4 * lq + q) * 64 + 16 * j + lr] = acc[j][q];
    __syncthreads();
    const int ch = c0 + lane;
    if (blockIdx.x == 0 && Z && tid < C) Z[b * C + tid] = (zred[0][tid] + zred[1][tid]) + (zred[2][tid] + zred[3][tid]);
    if (w != 0 || ch >= c) return;
    const int k0 = ignore_bg ? 1 : 0, n = C - k0;
    float vv[C];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const float S = (comb[k * 64 + lane] + comb[(DC_CP + k) * 64 + lane]) +
                        (comb[(2 * DC_CP + k) * 64 + lane] + comb[(3 * DC_CP + k) * 64 + lane]);
        const float Zk = (zred[0][k] + zred[1][k]) + (zred[2][k] + zred[3][k]);
        vv[k] = __fdiv_rn(S, Zk);
        if (k >= k0) ss = __fmaf_rn(vv[k], vv[k], ss);
    }
    const float N = sqrtf(ss), d = fmaxf(N, DC_EPS);
    if (nrm) nrm[(size_t)b * c + ch] = N;
#pragma unroll
    for (int k = 0; k < C; ++k)
        if (k >= k0) {
            const size_t e = ((size_t)b * n + (k - k0)) * c + ch;
            u[e] = __fdiv_rn(vv[k], d);
            if (v) v[e] = vv[k];
        }
}

// grid (n, 2): class row i of side blockIdx.y.  cen[side][i][:] = mean_b u - its mean over the channels; sq[side * n + i] =
// the sum of squares of that row.
__global__ void __launch_bounds__(256) dca_center_kernel(const float* __restrict__ ua, const float* __restrict__ ub, int ba,
                                                         int bb, int n, int c, float* __restrict__ cen,
                                                         float* __restrict__ sq) {
    __shared__ float red[4], red2[4];
    const int i = blockIdx.x, side = blockIdx.y;
    const float* u = side ? ub : ua;
    const int b = side ? bb : ba;
    float* row = cen + ((size_t)side * n + i) * c;
    float s = 0.f;
    float m0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // the first 2048 channels stay in registers for the second pass
    for (int base = threadIdx.x; base < c; base += 2048) {     // eight channels at a time: their loads are in flight together
        float m[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = 0.f;
#pragma unroll 4
        for (int q = 0; q < b; ++q)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (base + 256 * j < c) m[j] += u[((size_t)q * n + i) * c + base + 256 * j];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (base + 256 * j < c) {
                m[j] = __fdiv_rn(m[j], (float)b);
                row[base + 256 * j] = m[j];
                s += m[j];
                if (base == (int)threadIdx.x) m0[j] = m[j];
            }
    }
    const float mean = __fdiv_rn(block_sum4(s, red), (float)c);
    float t = 0.f;
    for (int base = threadIdx.x; base < c; base += 2048) {     // each thread reads back what it wrote (past 2048 channels)
        float d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            d[j] = base + 256 * j < c ? (base == (int)threadIdx.x ? m0[j] : row[base + 256 * j]) - mean : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (base + 256 * j < c) {
                row[base + 256 * j] = d[j];
                t = __fmaf_rn(d[j], d[j], t);
            }
    }
    t = block_sum4(t, red2);
    if (threadIdx.x == 0) sq[side * n + i] = t;
}

// grid (n * n): R[i][j] = <cen_a[i], cen_b[j]> / (sqrt(sq_a[i]) sqrt(sq_b[j]))
__global__ void __launch_bounds__(256) dca_corr_kernel(const float* __restrict__ cen, const float* __restrict__ sq, int n, int c,
                                                       float* __restrict__ R) {
    __shared__ float red[4];
    const int i = blockIdx.x / n, j = blockIdx.x - i * n;
    const float* a = cen + (size_t)i * c;
    const float* b = cen + ((size_t)n + j) * c;
    float s = 0.f;
#pragma unroll 8
    for (int ch = threadIdx.x; ch < c; ch += 256) s = __fmaf_rn(a[ch], b[ch], s);
    s = block_sum4(s, red);
    if (threadIdx.x == 0) R[blockIdx.x] = __fdiv_rn(s, sqrtf(sq[i]) * sqrtf(sq[n + j]));
}

// one workgroup, thread t the entry t of R (n * n <= 256).  L = -mean_i log R_ii - mean_{i != j} log(1 - max(R_ij, 1e-6));
// W = dL/dR (an off-diagonal entry at or below 1e-6: 0).  No clamp on the diagonal: a non-positive entry gives NaN.
__global__ void __launch_bounds__(256) dca_cov_loss_kernel(const float* __restrict__ R, int n, float weight, float* __restrict__ W,
                                                           float* loss) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    float term = 0.f;
    if (t < n * n) {
        const int i = t / n, j = t - i * n;
        const float r = R[t];
        float wv;
        if (i == j) {
            term = -logf(r) / (float)n;
            wv = -1.f / ((float)n * r);
        } else {
            const float nn = (float)(n * (n - 1));
            term = -logf(1.f - fmaxf(r, DC_LOW)) / nn;
            wv = r > DC_LOW ? 1.f / (nn * (1.f - r)) : 0.f;
        }
        W[t] = wv;
    }
    term = block_sum4(term, red);
    if (t == 0) loss[0] += weight * term;
}

// grid (n, sides), side = side0 + blockIdx.y, class row i of that side:
//   side 0: dm_a[i] = sum_j W_ij (cen_b[j] / (|a_i| |b_j|) - R_ij cen_a[i] / |a_i|^2)
//   side 1: dm_b[i] = sum_j W_ji (cen_a[j] / (|a_j| |b_i|) - R_ji cen_b[i] / |b_i|^2),   j ascending
__global__ void __launch_bounds__(256) dca_cov_dmean_kernel(const float* __restrict__ cen, const float* __restrict__ sq,
                                                            const float* __restrict__ R, const float* __restrict__ W, int n,
                                                            int c, int side0, float* __restrict__ dm) {
    __shared__ float ca[16], cb[16];
    const int i = blockIdx.x, side = side0 + blockIdx.y;
    const float* own = cen + ((size_t)side * n + i) * c;
    const float* oth = cen + (size_t)(1 - side) * n * c;
    if (threadIdx.x < n) {
        const int j = threadIdx.x, e = side ? j * n + i : i * n + j;
        const float so = sq[side * n + i], sj = sq[(1 - side) * n + j];
        ca[j] = __fdiv_rn(W[e], sqrtf(so) * sqrtf(sj));
        cb[j] = __fdiv_rn(W[e] * R[e], so);
    }
    __syncthreads();
    float* out = dm + ((size_t)side * n + i) * c;
    for (int ch = threadIdx.x; ch < c; ch += 256) {
        const float x = own[ch];
        float o[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = j < n ? oth[(size_t)j * c + ch] : 0.f;
        float g = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < n) {
                g = __fmaf_rn(ca[j], o[j], g);
                g = __fmaf_rn(-cb[j], x, g);
            }
        out[ch] = g;
    }
}

// grid (ceil(c / 256), b), thread = one channel of one image.  gu[k]: cov: dm[k] / b; mse: scale * (u - uo), scale = 2 / count.
//   gv = (gu - u <gu, u>) / N   (N < 1e-12: gu / 1e-12),   G[b][k0 + k][ch] = gv / Z[b][k0 + k],   G[b][0] = 0 with ignore_bg
// part (mse, optional): per workgroup the sum of (u - uo)^2.
__global__ void __launch_bounds__(256) dca_table_kernel(const float* __restrict__ u, const float* __restrict__ uo,
                                                        const float* __restrict__ dm, const float* __restrict__ nrm,
                                                        const float* __restrict__ Z, int b, int n, int c, int C, float scale,
                                                        float* __restrict__ G, float* __restrict__ part) {
    __shared__ float red[4];
    const int ch = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, k0 = C - n;
    float sqd = 0.f;
    if (ch < c) {
        float uu[16], gu[16];
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            uu[k] = gu[k] = 0.f;
            if (k < n) {
                const size_t e = ((size_t)q * n + k) * c + ch;
                uu[k] = u[e];
                if (dm) {
                    gu[k] = __fdiv_rn(dm[(size_t)k * c + ch], (float)b);
                } else {
                    const float d = uu[k] - uo[e];
                    gu[k] = scale * d;
                    sqd = __fmaf_rn(d, d, sqd);
                }
                dot = __fmaf_rn(gu[k], uu[k], dot);
            }
        }
        const float N = nrm[(size_t)q * c + ch];
        const bool clamped = N < DC_EPS;
        if (k0) G[((size_t)q * C) * c + ch] = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < n) {
                const float gv = clamped ? gu[k] / DC_EPS : __fdiv_rn(gu[k] - uu[k] * dot, N);
                G[((size_t)q * C + k0 + k) * c + ch] = __fdiv_rn(gv, Z[q * C + k0 + k]);
            }
    }
    if (part) {
        sqd = block_sum4(sqd, red);
        if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = sqd;
    }
}

// grid (ceil(hw / 64), ceil(c / 256), b): out row b * hw + p, channels ch .. ch + 3 = weight * sum_k P[b][k][p] G[b][k][ch]
// (k ascending, fused multiply-adds), one 8-byte store per thread and pixel; a wavefront writes 512 consecutive bytes.
template <int C>
__global__ void __launch_bounds__(256) dca_grad_kernel(Pred pr, const float* __restrict__ G, int hw, int c, float weight,
                                                       bf16_t* __restrict__ out, int ld, int accumulate) {
    __shared__ float Ps[DC_GPX * DC_CP];
    const int b = blockIdx.z, p0 = blockIdx.x * DC_GPX;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < DC_GPX) {
        float l1[C], l2[C], P[C];
        load_logits<C>(pr, b, p0 + tid, hw, l1, l2);
        probs_from<C>(pr.kind, p0 + tid < hw, l1, l2, P);
#pragma unroll
        for (int k = 0; k < C; ++k) Ps[tid * DC_CP + k] = P[k];
    }
    const int ch = blockIdx.y * DC_GCH + 4 * lane;
    const bool live = ch < c;                         // c % 32 == 0: four channels are in or out together
    float4 g[C];
#pragma unroll
    for (int k = 0; k < C; ++k)
        g[k] = live ? *(const float4*)(G + ((size_t)b * C + k) * c + ch) : float4{0.f, 0.f, 0.f, 0.f};
    // the old rows of all 16 pixels of this thread are read before the first one is needed
    bf16_t* dst = out + ((size_t)b * hw + p0 + w) * ld + ch;
    uint2 old[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        old[i] = accumulate && live && p0 + w + 4 * i < hw ? *(const uint2*)(dst + (size_t)4 * i * ld) : uint2{0u, 0u};
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int pl = w + 4 * i;
        if (p0 + pl < hw) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const float P = Ps[pl * DC_CP + k];
                a0 = __fmaf_rn(P, g[k].x, a0);
                a1 = __fmaf_rn(P, g[k].y, a1);
                a2 = __fmaf_rn(P, g[k].z, a2);
                a3 = __fmaf_rn(P, g[k].w, a3);
            }
            // store4_bf16's accumulate, with the old values already here: they join in fp32 before the one rounding
            store4_bf16(dst + (size_t)4 * i * ld, __fadd_rn(__fmul_rn(weight, a0), __uint_as_float(old[i].x << 16)),
                        __fadd_rn(__fmul_rn(weight, a1), __uint_as_float(old[i].x & 0xffff0000u)),
                        __fadd_rn(__fmul_rn(weight, a2), __uint_as_float(old[i].y << 16)),
                        __fadd_rn(__fmul_rn(weight, a3), __uint_as_float(old[i].y & 0xffff0000u)), 0);
        }
    }
}

namespace {

struct Side {
    const float* feat;
    int b;
    long long ldc, ldb;
    Pred pr;
};

bool side_ok(const Side& s, int hw, int c) {
    if (!s.feat || !s.pr.p1 || (s.pr.kind == DC_LOGITS2 && !s.pr.p2)) return false;
    return s.b >= 1 && feat_view_ok(s.b, hw, s.ldc, s.ldb, c);
}

int launch_context(const Side& s, int hw, int c, int C, int ignore_bg, float* u, float* v, float* Z, float* nrm,
                   hipStream_t st) {
    return with_classes(C, [&](auto cc) -> int {
        constexpr int CC = decltype(cc)::value;
        dca_context_kernel<CC><<<dim3(cdiv(c, DC_CH), s.b), 256, 0, st>>>(FeatView{s.feat, s.ldc, s.ldb, hw, s.b * hw}, s.pr, c,
                                                                          ignore_bg, u, v, Z, nrm);
        RGDA_CHECK_LAUNCH();
        return (int)RGDA_OK;
    });
}

int launch_grad(const Side& s, const float* G, int hw, int c, int C, float weight, bf16_t* out, int ld, int accumulate,
                hipStream_t st) {
    return with_classes(C, [&](auto cc) -> int {
        constexpr int CC = decltype(cc)::value;
        dca_grad_kernel<CC><<<dim3(cdiv(hw, DC_GPX), cdiv(c, DC_GCH), s.b), 256, 0, st>>>(s.pr, G, hw, c, weight, out, ld,
                                                                                        accumulate);
        RGDA_CHECK_LAUNCH();
        return (int)RGDA_OK;
    });
}

bool shape_ok(int hw, int c, int pred_kind) {
    return hw >= 1 && c >= 32 && !(c & 31) && pred_kind >= DC_PROB && pred_kind <= DC_LOGITS2;
}

}  // namespace

extern "C" size_t rgda_dca_context_workspace(int b, int c) {
    if (b < 1 || c < 32 || (c & 31)) return 0;
    return a256((size_t)4 * b * c);
}

extern "C" int rgda_dca_context(const float* feat, int b, int hw, int64_t ldc, int64_t ldb, const float* pred1,
                                const float* pred2, int pred_kind, int c, int C, int ignore_bg, float* u, float* v, float* Z,
                                void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (!u || !ws || ((uintptr_t)ws & 255) || !shape_ok(hw, c, pred_kind)) return RGDA_ERR_ARG;
    const Side s{feat, b, (long long)ldc, (long long)ldb, Pred{pred1, pred2, pred_kind}};
    if (!side_ok(s, hw, c)) return RGDA_ERR_ARG;
    if (!class_count_ok(C)) return RGDA_ERR_UNSUPPORTED;
    if (ws_bytes < rgda_dca_context_workspace(b, c)) return RGDA_ERR_WORKSPACE;
    return launch_context(s, hw, c, C, ignore_bg != 0, u, v, Z, (float*)ws, to_stream(stream));
}

extern "C" size_t rgda_dca_loss_workspace(int b_a, int b_b, int c, int C, int ignore_bg) {
    if (b_a < 1 || b_b < 1 || c < 32 || (c & 31) || !class_count_ok(C)) return 0;
    return make_plan(b_a, b_b, c, C, ignore_bg != 0).bytes;
}

extern "C" int rgda_dca_loss(const float* feat_a, int b_a, int64_t ldc_a, int64_t ldb_a, const float* pred1_a,
                             const float* pred2_a, void* dfeat_a, const float* feat_b, int b_b, int64_t ldc_b, int64_t ldb_b,
                             const float* pred1_b, const float* pred2_b, void* dfeat_b, int hw, int c, int C, int pred_kind,
                             int ignore_bg, int kind, float* loss, int lddf, int accumulate, float weight, void* ws,
                             size_t ws_bytes, rgda_stream_t stream) {
    if (!loss || !ws || ((uintptr_t)ws & 255) || !shape_ok(hw, c, pred_kind)) return RGDA_ERR_ARG;
    if (kind != DC_COV && kind != DC_MSE) return RGDA_ERR_ARG;
    const Side sd[2] = {{feat_a, b_a, (long long)ldc_a, (long long)ldb_a, Pred{pred1_a, pred2_a, pred_kind}},
                        {feat_b, b_b, (long long)ldc_b, (long long)ldb_b, Pred{pred1_b, pred2_b, pred_kind}}};
    if (!side_ok(sd[0], hw, c) || !side_ok(sd[1], hw, c)) return RGDA_ERR_ARG;
    if (!grad_rows_ok(dfeat_a, lddf, c, 16) || !grad_rows_ok(dfeat_b, lddf, c, 16)) return RGDA_ERR_ARG;
    if (kind == DC_MSE && b_a != b_b) return RGDA_ERR_ARG;
    if (!class_count_ok(C)) return RGDA_ERR_UNSUPPORTED;
    const DcPlan p = make_plan(b_a, b_b, c, C, ignore_bg != 0);
    if (ws_bytes < p.bytes) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    char* wsp = (char*)ws;
    float *u[2], *nrm[2], *Z[2], *G[2];
    for (int s = 0; s < 2; ++s) {
        u[s] = (float*)(wsp + p.off_u[s]);
        nrm[s] = (float*)(wsp + p.off_nrm[s]);
        Z[s] = (float*)(wsp + p.off_z[s]);
        G[s] = (float*)(wsp + p.off_g[s]);
    }
    float* cen = (float*)(wsp + p.off_cen);
    float* dm = (float*)(wsp + p.off_dm);
    float* sq = (float*)(wsp + p.off_small);
    float* R = sq + 2 * p.n;
    float* W = R + p.n * p.n;
    float* part = (float*)(wsp + p.off_part);
    void* dfeat[2] = {dfeat_a, dfeat_b};
    const int n = p.n;
    for (int s = 0; s < 2; ++s) {
        const int rc = launch_context(sd[s], hw, c, C, ignore_bg != 0, u[s], nullptr, Z[s], nrm[s], st);
        if (rc != RGDA_OK) return rc;
    }
    if (kind == DC_COV) {
        dca_center_kernel<<<dim3(n, 2), 256, 0, st>>>(u[0], u[1], b_a, b_b, n, c, cen, sq);
        RGDA_CHECK_LAUNCH();
        dca_corr_kernel<<<n * n, 256, 0, st>>>(cen, sq, n, c, R);
        RGDA_CHECK_LAUNCH();
        dca_cov_loss_kernel<<<1, 256, 0, st>>>(R, n, weight, W, loss);
        RGDA_CHECK_LAUNCH();
        if (!dfeat_a && !dfeat_b) return RGDA_OK;
        const int side0 = dfeat_a ? 0 : 1, sides = dfeat_a && dfeat_b ? 2 : 1;
        dca_cov_dmean_kernel<<<dim3(n, sides), 256, 0, st>>>(cen, sq, R, W, n, c, side0, dm);
        RGDA_CHECK_LAUNCH();
    }
    const float count = (float)b_a * (float)n * (float)c;
    for (int s = 1; s >= 0; --s) {                  // side b first: with mse it also leaves the loss partials
        const bool lossy = kind == DC_MSE && s == 1;
        if (!dfeat[s] && !lossy) continue;
        dca_table_kernel<<<dim3(cdiv(c, 256), sd[s].b), 256, 0, st>>>(
            u[s], u[1 - s], kind == DC_COV ? dm + (size_t)s * n * c : nullptr, nrm[s], Z[s], sd[s].b, n, c, C,
            2.f / count, G[s], lossy ? part : nullptr);
        RGDA_CHECK_LAUNCH();
    }
    if (kind == DC_MSE && rows_loss_sum(part, cdiv(c, 256) * b_b, loss, weight / count, st) != RGDA_OK) return RGDA_ERR_LAUNCH;
    for (int s = 0; s < 2; ++s) {
        if (!dfeat[s]) continue;
        const int rc = launch_grad(sd[s], G[s], hw, c, C, weight, (bf16_t*)dfeat[s], lddf, accumulate, st);
        if (rc != RGDA_OK) return rc;
    }
    return RGDA_OK;
}
