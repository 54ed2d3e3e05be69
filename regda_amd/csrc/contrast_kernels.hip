// Pixel-to-pixel contrastive loss (regda/gast/contrastive.py::PixelContrastLoss, Wang et al., ICCV 2021, with
// hard-anchor sampling): the selection tables, and forward + feature gradient in one call.  Deterministic (no
// floating-point atomics; the selected rows are distinct, so the scatter needs none).
//
//   select : per image one workgroup: key = 2 class + easy (easy: predict == label) per feature pixel, 2C for ignored and
//            out-of-range labels; a stable counting sort of the pixel indices by key -> order; the key totals -> counts
//                                                                                            pc_select_kernel
//   rows   : rank -> pixel through order / counts; row r = view * A + anchor                 pc_rows_kernel
//   gather : X = bf16(feat rows), once, pixel-major [NP][k] and channel-major [k][NP]; NP = N rounded up to 128, the
//            padding zero                                                                    pc_gather_kernel
//   gram   : one wavefront per (upper 128 x 128 tile, K split): the raw accumulators -> part   pc_gram_kernel
//   reduce : G = (sum of the splits, in order) / temperature, fp32, to both triangles         pc_reduce_kernel
//   row    : one wavefront per row: m, neg, sum over positives of lp and of 1 / d, P          pc_row_kernel
//   loss   : loss[0] += weight * -(T / Tb) / N * sum_r rowloss_r, in order                    rows_loss_sum
//   pair   : M = bf16(W + W^T) [NP][NP], the padding zero                                     pc_pair_kernel
//   grad   : C[c][r] = sum_q X^T[c][q] M[r][q] (the shape of mmd_grad_kernel);
//            dfeat[pixel of r][c] (+)= weight / T * C[c][r]                                   pc_grad_kernel
// The feature view, the staging tile, the loss sum and the gradient store are those of feat_rows.h.
#include "feat_rows.h"

namespace {

constexpr int PC_MAX_CLASSES = 16;
constexpr int PC_MAX_HW = 16384;             // keys of one image sit in LDS as bytes
constexpr int PC_MAX_ROWS = 4096;
constexpr int PC_MAX_SPLIT = 8;
constexpr int PC_SPLIT_JOBS = 256;           // K is split until the tile jobs reach about one per CU

struct PcPlan {
    int N, np, T, U, S, kchunk;
    size_t off_pix, off_cls, off_xp, off_xt, off_stat, off_g, off_part, off_m, bytes;
};

PcPlan make_plan(int N, int k) {
    PcPlan p;
    p.N = N;
    p.np = (N + CT - 1) / CT * CT;
    p.T = p.np / CT;
    p.U = p.T * (p.T + 1) / 2;
    const int groups = k / KG;
    int S = PC_SPLIT_JOBS / p.U;
    S = S < 1 ? 1 : (S > PC_MAX_SPLIT ? PC_MAX_SPLIT : S);
    if (S > groups) S = groups;
    const int per = (groups + S - 1) / S;
    p.S = (groups + per - 1) / per;            // no empty split
    p.kchunk = per * KG;
    size_t o = 0;
    p.off_pix = o;  o += a256((size_t)p.np * 4);
    p.off_cls = o;  o += a256((size_t)p.np * 4);
    p.off_xp = o;   o += a256((size_t)p.np * k * 2);
    p.off_xt = o;   o += a256((size_t)k * p.np * 2);
    p.off_stat = o; o += a256((size_t)5 * p.np * 4);
    p.off_g = o;    o += a256((size_t)p.np * p.np * 4);
    p.off_part = o; o += a256((size_t)p.U * p.S * CT * CT * 4);
    p.off_m = o;    o += a256((size_t)p.np * p.np * 2);
    p.bytes = o;
    return p;
}

}  // namespace

// One workgroup per image.  Pass 1 (coalesced): the key of every feature pixel to LDS.  Pass 2: thread t counts the keys
// of its contiguous pixel chunk -> hist[key][t].  An exclusive scan over (key, t) turns the counts into the first output
// slot of every (key, chunk); pass 3 walks the chunk again in pixel order: a stable sort.
__global__ void __launch_bounds__(256) pc_select_kernel(const int64_t* __restrict__ labels, const void* __restrict__ predict,
                                                        int predict_kind, int C, int H, int W, int h, int w, int ignore_label,
                                                        int32_t* __restrict__ counts, int32_t* __restrict__ order,
                                                        int* __restrict__ flag) {
    __shared__ unsigned char keys[PC_MAX_HW];
    __shared__ int hist[(2 * PC_MAX_CLASSES + 1) * 256];
    __shared__ int part[256];
    const int img = blockIdx.x, tid = threadIdx.x, hw = h * w, K = 2 * C + 1;
    const int ry = H / h, rx = W / w;
    const int64_t* lab = labels + (size_t)img * H * W;
    bool bad = false;
    for (int p = tid; p < hw; p += 256) {
        const int y = p / w, x = p - y * w;
        const int64_t l = lab[(size_t)(y * ry) * W + x * rx];
        int key = 2 * C;
        if (l != (int64_t)ignore_label) {
            if (l >= 0 && l < C) {
                int64_t pr;
                if (predict_kind == RGDA_PREDICT_LOGITS) {
                    const float* lg = (const float*)predict + (size_t)img * C * hw + p;
                    float best = lg[0];
                    int bi = 0;
                    for (int c = 1; c < C; ++c) {
                        const float v = lg[(size_t)c * hw];
                        if (v > best) { best = v; bi = c; }
                    }
                    pr = bi;
                } else {
                    pr = ((const int64_t*)predict)[(size_t)img * hw + p];
                }
                key = 2 * (int)l + (pr == l ? 1 : 0);
            } else {
                bad = true;
            }
        }
        keys[p] = (unsigned char)key;
    }
    if (bad) atomicOr(flag, 4);
    for (int e = tid; e < K * 256; e += 256) hist[e] = 0;
    __syncthreads();
    const int chunk = (hw + 255) / 256;
    const int p0 = min(tid * chunk, hw), p1 = min(p0 + chunk, hw);
    for (int p = p0; p < p1; ++p) hist[keys[p] * 256 + tid] += 1;
    __syncthreads();
    // exclusive scan of the K * 256 counts in (key, thread) order: thread t owns entries [t K, (t + 1) K)
    int s = 0;
    for (int e = tid * K; e < (tid + 1) * K; ++e) s += hist[e];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
    }
    __syncthreads();
    int run = part[tid];
    for (int e = tid * K; e < (tid + 1) * K; ++e) { const int v = hist[e]; hist[e] = run; run += v; }
    __syncthreads();
    if (tid < 2 * C) counts[(size_t)img * 2 * C + tid] = hist[(tid + 1) * 256] - hist[tid * 256];
    __syncthreads();
    int32_t* ord = order + (size_t)img * hw;
    for (int p = p0; p < p1; ++p) {
        const int slot = hist[keys[p] * 256 + tid]++;
        ord[slot] = p;
    }
}

// row r = v A + a -> its global pixel row (image * hw + pixel) and class.  A rank outside its list or an anchor outside
// the tables cannot be reached from the host plan; it is clamped so that no address leaves the buffers.
__global__ void __launch_bounds__(256) pc_rows_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ counts,
                                                      const int32_t* __restrict__ anchors, const int32_t* __restrict__ ranks,
                                                      int A, int n_view, int b, int hw, int C, int N, int np,
                                                      int* __restrict__ rowpix, int* __restrict__ rowcls) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= np) return;
    if (r >= N) { rowpix[r] = 0; rowcls[r] = -1; return; }
    const int v = r / A, a = r - v * A;
    const int img = min(max(anchors[3 * a], 0), b - 1), cls = min(max(anchors[3 * a + 1], 0), C - 1);
    const int hk = anchors[3 * a + 2];
    const int32_t* cnt = counts + (size_t)img * 2 * C;
    int off = 0;
    for (int c = 0; c < 2 * cls; ++c) off += cnt[c];
    int len = cnt[2 * cls];
    if (v >= hk) { off += len; len = cnt[2 * cls + 1]; }
    const int rank = min(max(ranks[(size_t)a * n_view + v], 0), max(len - 1, 0));
    const int slot = min(max(off + rank, 0), hw - 1);
    const int pix = min(max(order[(size_t)img * hw + slot], 0), hw - 1);
    rowpix[r] = img * hw + pix;
    rowcls[r] = cls;
}

// 64 rows x 64 channels per workgroup: bf16(feat) to the channel-major image and, through LDS, to the pixel-major one;
// the padding rows are written as zeros
__global__ void __launch_bounds__(256) pc_gather_kernel(FeatView f, const int* __restrict__ rowpix, int N, int np, int k,
                                                        bf16_t* __restrict__ xt, bf16_t* __restrict__ xp) {
    const int r0 = blockIdx.x * 64;
    stage_tile64(f, [=](int r) { return r0 + r < N ? rowpix[r0 + r] : -1; }, 64, nullptr, blockIdx.y * 64, k, xt, np, r0, xp);
}

// job = (upper tile u, split s), one wavefront each: the accumulators of X[I] X[J]^T over the split's channels go to
// part[job] in register order (element reg of acc[i][j] of lane l at ((4 i + j) 16 + reg) 64 + l)
__global__ void __launch_bounds__(256, 1) pc_gram_kernel(const bf16_t* __restrict__ xp, int np, int k, int T, int S, int kchunk,
                                                         int njobs, float* __restrict__ part) {
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (job >= njobs) return;
    const int u = job / S, s = job - u * S;
    int I, J;
    upper_tile(u, T, I, J);
    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x16{};
    const int k0 = s * kchunk, k1 = min(k0 + kchunk, k);
    tile_nt<4>(xp, k, I * CT, np - 1, xp, k, J * CT, np - 1, k0, k1, acc);
    float* dst = part + (size_t)job * CT * CT + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) dst[((i * 4 + j) * 16 + reg) * 64] = acc[i][j][reg];
}

// one workgroup per upper tile: G = (part[u][0] + part[u][1] + ..) / temperature to (I, J) and, mirrored, to (J, I)
__global__ void __launch_bounds__(256) pc_reduce_kernel(const float* __restrict__ part, int np, int T, int S, float temperature,
                                                        float* __restrict__ G) {
    const int u = blockIdx.x;
    int I, J;
    upper_tile(u, T, I, J);
    const float* src = part + (size_t)u * S * CT * CT;
    for (int e = threadIdx.x; e < CT * CT; e += 256) {
        float v = src[e];
        for (int s = 1; s < S; ++s) v += src[(size_t)s * CT * CT + e];
        v = __fdiv_rn(v, temperature);
        const int lane = e & 63, reg = (e >> 6) & 15, ij = e >> 10, i = ij >> 2, j = ij & 3;
        const int row = I * CT + 32 * i + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        const int col = J * CT + 32 * j + (lane & 31);
        G[(size_t)row * np + col] = v;
        if (I != J) G[(size_t)col * np + row] = v;
    }
}

// one wavefront per row r < N, columns q < N lane-strided, every sum a lane-strided partial then the butterfly:
//   m = max_q G_rq;  neg = sum over q of another class of exp(G_rq - m);
//   over the positives (same class, q != r): lp = l - log(exp(l) + neg + eps), sum lp, P, s1 = sum 1 / (exp(l) + neg + eps)
// stat: [0] m, [1] neg, [2] s1, [3] c = cscale / (P + eps), [4] rowloss = sum lp / (P + eps); rows >= N: zeros
__global__ void __launch_bounds__(256) pc_row_kernel(const float* __restrict__ G, const int* __restrict__ rowcls, int N, int np,
                                                     float eps, float cscale, float* __restrict__ stat) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= np) return;
    if (r >= N) {
        if (lane < 5) stat[(size_t)lane * np + r] = 0.f;
        return;
    }
    const float* g = G + (size_t)r * np;
    const int cls = rowcls[r];
    float m = -INFINITY;
    for (int q = lane; q < N; q += 64) m = fmaxf(m, g[q]);
    m = wave_max(m);
    float neg = 0.f;
    for (int q = lane; q < N; q += 64)
        if (rowcls[q] != cls) neg += expf(g[q] - m);
    neg = wave_sum(neg);
    float slp = 0.f, s1 = 0.f, P = 0.f;
    for (int q = lane; q < N; q += 64)
        if (rowcls[q] == cls && q != r) {
            const float l = g[q] - m;
            const float d = expf(l) + neg + eps;
            slp += l - logf(d);
            s1 += 1.f / d;
            P += 1.f;
        }
    slp = wave_sum(slp);
    s1 = wave_sum(s1);
    P = wave_sum(P);
    if (lane == 0) {
        stat[r] = m;
        stat[(size_t)np + r] = neg;
        stat[(size_t)2 * np + r] = s1;
        stat[(size_t)3 * np + r] = cscale / (P + eps);
        stat[(size_t)4 * np + r] = slp / (P + eps);
    }
}

// W_rq = d L / d l_rq: c_r (1 - e / (e + neg_r + eps)) for a positive q, -c_r e s1_r for a negative q, 0 on the
// diagonal, e = exp(G_rq - m_r).  M_rq = bf16(W_rq + W_qr) (G is stored symmetric, so W_qr is read from the same G_rq).
static __device__ __forceinline__ float pc_w(float g, bool pos, float m, float neg, float s1, float c, float eps) {
    const float e = expf(g - m);
    return pos ? c * (1.f - e / (e + neg + eps)) : -c * e * s1;
}
__global__ void __launch_bounds__(256) pc_pair_kernel(const float* __restrict__ G, const int* __restrict__ rowcls,
                                                      const float* __restrict__ stat, int N, int np, float eps,
                                                      bf16_t* __restrict__ M) {
    const int r = blockIdx.y;
    const int q = (blockIdx.x * 256 + threadIdx.x) * 2;
    if (q >= np) return;
    float v[2] = {0.f, 0.f};
    if (r < N) {
        const int cls = rowcls[r];
        const float mr = stat[r], nr = stat[(size_t)np + r], sr = stat[(size_t)2 * np + r], cr = stat[(size_t)3 * np + r];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int qq = q + e;
            if (qq < N && qq != r) {
                const float g = G[(size_t)r * np + qq];
                const bool pos = rowcls[qq] == cls;
                v[e] = pc_w(g, pos, mr, nr, sr, cr, eps) +
                       pc_w(g, pos, stat[qq], stat[(size_t)np + qq], stat[(size_t)2 * np + qq], stat[(size_t)3 * np + qq], eps);
            }
        }
    }
    *(unsigned*)(M + (size_t)r * np + q) = pack2bf(v[0], v[1]);
}

// every row of dfeat, its first k columns, to zero (accumulate == 0)
__global__ void __launch_bounds__(256) pc_zero_rows_kernel(bf16_t* __restrict__ out, long long rows, int k, int ld) {
    const int q = k >> 2;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * q) return;
    const long long row = e / q;
    const int c = (int)(e - row * q) * 4;
    *(uint2*)(out + (size_t)row * ld + c) = uint2{0u, 0u};
}

// C[c][r] = sum_q X^T[c][q] M[r][q]: a lane's registers 4g .. 4g+3 are four consecutive channels of one selected row
// -> one 8-byte store into that pixel's bf16 gradient row
__global__ void __launch_bounds__(256, 1) pc_grad_kernel(const bf16_t* __restrict__ xt, const bf16_t* __restrict__ M,
                                                         const int* __restrict__ rowpix, bf16_t* __restrict__ out, int ld, int N,
                                                         int np, int k, int njobs, float scale, int accumulate) {
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (job >= njobs) return;
    const int T = (k + CT - 1) / CT;
    const int mt = job % T, nt = job / T;
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};
    tile_nt<2>(xt, np, mt * CT, k - 1, M, np, nt * GN, N - 1, 0, np, acc);
    // selected row r scatters to its pixel's gradient row; every column takes scale * acc
    grad_tile_store(acc, mt, nt, N, k, accumulate, [=](int r) { return out + (size_t)rowpix[r] * ld; },
                    [=](int) { return [=](F4 a, int) { return F4{scale * a.v0, scale * a.v1, scale * a.v2, scale * a.v3}; }; });
}

extern "C" int rgda_pixel_contrast_select(const int64_t* labels, const void* predict, int predict_kind, int b, int C, int H,
                                          int W, int h, int w, int ignore_label, int32_t* counts, int32_t* order, int* flag,
                                          rgda_stream_t stream) {
    if (!labels || !predict || !counts || !order || !flag) return RGDA_ERR_ARG;
    if (b <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return RGDA_ERR_ARG;
    if (predict_kind != RGDA_PREDICT_LABELS && predict_kind != RGDA_PREDICT_LOGITS) return RGDA_ERR_ARG;
    if (C < 2 || C > PC_MAX_CLASSES || H % h || W % w || (long long)h * w > PC_MAX_HW) return RGDA_ERR_UNSUPPORTED;
    pc_select_kernel<<<b, 256, 0, to_stream(stream)>>>(labels, predict, predict_kind, C, H, W, h, w, ignore_label, counts, order,
                                                       flag);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" size_t rgda_pixel_contrast_loss_workspace(int N, int k) {
    if (N < 1 || N > PC_MAX_ROWS || k < 32 || (k & 31)) return 0;
    return make_plan(N, k).bytes;
}

extern "C" int rgda_pixel_contrast_loss(const float* feat, int b, int hw, int64_t ldc, int64_t ldb, int k, int C,
                                        const int32_t* order, const int32_t* counts, const int32_t* anchors, int A,
                                        const int32_t* ranks, int n_view, float temperature, float base_temperature, float eps,
                                        float* loss, void* dfeat, int lddf, int accumulate, float weight, void* ws,
                                        size_t ws_bytes, rgda_stream_t stream) {
    if (!feat || !order || !counts || !anchors || !ranks || !loss || !ws || ((uintptr_t)ws & 255)) return RGDA_ERR_ARG;
    if (b <= 0 || hw <= 0 || k < 32 || (k & 31) || A < 0 || n_view < 0) return RGDA_ERR_ARG;
    if (!(temperature > 0.f) || !(base_temperature > 0.f) || !(eps >= 0.f)) return RGDA_ERR_ARG;
    if ((long long)b * hw > (1ll << 24) || !feat_view_ok(b, hw, ldc, ldb, k)) return RGDA_ERR_ARG;
    if (!grad_rows_ok(dfeat, lddf, k, 16)) return RGDA_ERR_ARG;
    if (C < 2 || C > PC_MAX_CLASSES) return RGDA_ERR_UNSUPPORTED;
    const long long Nl = (long long)A * n_view;
    if (Nl < 1 || Nl > PC_MAX_ROWS) return RGDA_ERR_UNSUPPORTED;
    const int N = (int)Nl;
    const PcPlan p = make_plan(N, k);
    if (ws_bytes < p.bytes) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    char* wsp = (char*)ws;
    int* rowpix = (int*)(wsp + p.off_pix);
    int* rowcls = (int*)(wsp + p.off_cls);
    bf16_t* xp = (bf16_t*)(wsp + p.off_xp);
    bf16_t* xt = (bf16_t*)(wsp + p.off_xt);
    float* stat = (float*)(wsp + p.off_stat);
    float* G = (float*)(wsp + p.off_g);
    float* part = (float*)(wsp + p.off_part);
    bf16_t* M = (bf16_t*)(wsp + p.off_m);
    const int np = p.np;
    pc_rows_kernel<<<cdiv(np, 256), 256, 0, st>>>(order, counts, anchors, ranks, A, n_view, b, hw, C, N, np, rowpix, rowcls);
    RGDA_CHECK_LAUNCH();
    pc_gather_kernel<<<dim3(np / 64, cdiv(k, 64)), 256, 0, st>>>(FeatView{feat, (long long)ldc, (long long)ldb, hw, b * hw}, rowpix, N, np, k, xt, xp);
    RGDA_CHECK_LAUNCH();
    pc_gram_kernel<<<cdiv(p.U * p.S, 4), 256, 0, st>>>(xp, np, k, p.T, p.S, p.kchunk, p.U * p.S, part);
    RGDA_CHECK_LAUNCH();
    pc_reduce_kernel<<<p.U, 256, 0, st>>>(part, np, p.T, p.S, temperature, G);
    RGDA_CHECK_LAUNCH();
    const float cscale = -(temperature / base_temperature) / (float)N;
    pc_row_kernel<<<np / 4, 256, 0, st>>>(G, rowcls, N, np, eps, cscale, stat);
    RGDA_CHECK_LAUNCH();
    if (rows_loss_sum(stat + (size_t)4 * np, N, loss, weight * cscale, st) != RGDA_OK) return RGDA_ERR_LAUNCH;
    if (!dfeat) return RGDA_OK;
    pc_pair_kernel<<<dim3(cdiv(np / 2, 256), np), 256, 0, st>>>(G, rowcls, stat, N, np, eps, M);
    RGDA_CHECK_LAUNCH();
    if (!accumulate) {
        const long long rows = (long long)b * hw;
        pc_zero_rows_kernel<<<cdiv(rows * (k >> 2), 256), 256, 0, st>>>((bf16_t*)dfeat, rows, k, lddf);
        RGDA_CHECK_LAUNCH();
    }
    const int njobs = cdiv(k, CT) * cdiv(N, GN);
    pc_grad_kernel<<<cdiv(njobs, 4), 256, 0, st>>>(xt, M, rowpix, (bf16_t*)dfeat, lddf, N, np, k, njobs, weight / temperature,
                                                   accumulate);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
