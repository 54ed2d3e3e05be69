// Class-aware whitening loss (regda/gast/class_ware_whiten.py::ClassWareWhitening with class_ids = range(C), as built by
// Aligner.__init__, regda/gast/alignment.py:71, and called by Aligner.whiten_class_ware, :165-170): forward and the
// gradient w.r.t. the feature map, deterministic (no floating-point atomics).
//
// Every pixel belongs to at most one class, so the pixels are sorted by class once and every later pass touches a
// pixel's row once:
//   index  : per-class pixel counts and the class-sorted pixel list sidx (stable: pixels of a class in image order;
//            each class padded with -1 to a multiple of 64 rows), the class of every 64-row tile; a label outside
//            [0, C) that is not ignore_label counts as ignored and sets flag bit 2      whiten_index_kernel
//   mean   : mu[c][ch] = sum over the class's pixels / n_c, fp32, fixed order          whiten_mean_kernel
//   centre : Xc = bf16(X - mu[class]), once, in sorted row order (pad rows 0), in two layouts: channel-major
//            [k][NP] (the covariance product sums over pixels) and pixel-major [NP][k] (the gradient product sums
//            over channels)                                                            whiten_center_kernel
//   cov    : one workgroup per (class, group): the s x s Gram block of the class's rows, the rows dealt to the four
//            wavefronts in 32-row groups, the four partials added in wavefront order through LDS;
//            D = S / (n_c - 1) - I in fp32; bf16(D) to the workspace; mean(D^2) -> lpart[class][group]
//            (n_c <= 1: 0)                                                             whiten_cov_kernel
//   loss   : loss[0] += weight * sum(lpart), fixed order                                rows_loss_sum
//   zero   : accumulate == 0 only: the rows of ignored pixels and of classes with n_c <= 1 := 0   whiten_zero_kernel
//   grad   : per (64-row tile, group): dX^T = bf16(D) . Xc^T -> dfeat[pixel][group block]
//            = 4 weight / (s^2 (n_c - 1)) * dX (+ dfeat), rows scattered back through sidx  whiten_grad_kernel
//
// Both products are C[m][n] = sum_k P[m][k] Q[n][k] with P and Q row-major bf16 and K contiguous (the layout of
// coral_kernels.hip): v_mfma_f32_32x32x16_bf16 fragments are plain 16-byte loads from global memory, lane half h and
// element j of k-step t take k = 16h + 8t + j in both operands.  The feature view, the staging tile, the sums and the
// gradient store are those of feat_rows.h.
#include "feat_rows.h"

namespace {

constexpr int RT = 64;           // rows per tile of the sorted order: every class starts on a tile boundary
// workspace header (256 bytes of int32): flag | cnt[16] | off[17]

struct WhitenPlan {
    int n, k, C, G, s, NP;
    size_t off_sidx, off_tcls, off_mean, off_ct, off_xp, off_dmat, off_lpart, bytes;
};

bool block_ok(int s) { return s == 32 || s == 64 || s == 96 || s == 128; }

WhitenPlan make_plan(int n, int k, int C, int G) {
    WhitenPlan p;
    p.n = n; p.k = k; p.C = C; p.G = G; p.s = k / G;
    p.NP = (n + RT - 1) / RT * RT + RT * C;          // every class padded to whole tiles
    size_t o = 256;                                   // header
    p.off_sidx = o;  o += a256((size_t)p.NP * 4);
    p.off_tcls = o;  o += a256((size_t)(p.NP / RT) * 4);
    p.off_mean = o;  o += a256((size_t)C * k * 4);
    p.off_ct = o;    o += a256((size_t)k * p.NP * 2);
    p.off_xp = o;    o += a256((size_t)p.NP * k * 2);
    p.off_dmat = o;  o += a256((size_t)C * k * p.s * 2);
    p.off_lpart = o; o += a256((size_t)C * G * 4);
    p.bytes = o;
    return p;
}

}  // namespace

// one workgroup: counts, offsets, the stable class-sorted pixel list and the class of every tile.  Serial in n: one
// round of C ballots and three barriers per 1024 labels -- 8 rounds at the 8192 labels of the production shape, which
// is the range it is meant for (a few 10^4 labels); the accepted maximum n = 2^24 is 16384 rounds and would want a
// multi-workgroup sort.
__global__ void __launch_bounds__(1024) whiten_index_kernel(const int64_t* __restrict__ labels, int n, int C, int ignore_label,
                                                            int NP, int* __restrict__ hdr, int* __restrict__ sidx,
                                                            int* __restrict__ tcls) {
    __shared__ int cnt[16], off[17], run[16], wcnt[16][16], bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 16) { cnt[tid] = 0; run[tid] = 0; }
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const long long l = labels[i];
        if (l == ignore_label) continue;
        if (l < 0 || l >= C) atomicOr(&bad, 4);
        else atomicAdd(&cnt[(int)l], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int c = 0; c < 16; ++c) {
            off[c] = o;
            o += (cnt[c] + RT - 1) / RT * RT;
        }
        off[16] = o;
        hdr[0] = bad;
        for (int c = 0; c < 16; ++c) hdr[1 + c] = cnt[c];
        for (int c = 0; c <= 16; ++c) hdr[17 + c] = off[c];
    }
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        int l = -1;
        if (i < n) {
            const long long ll = labels[i];
            if (ll != ignore_label && ll >= 0 && ll < C) l = (int)ll;
        }
        int rank = 0;
        for (int c = 0; c < C; ++c) {
            const unsigned long long m = __ballot(l == c);
            if (l == c) rank = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[wave][c] = __popcll(m);
        }
        __syncthreads();
        if (l >= 0) {
            int pre = 0;
            for (int w = 0; w < wave; ++w) pre += wcnt[w][l];
            sidx[off[l] + run[l] + pre + rank] = i;
        }
        __syncthreads();
        if (tid < C) {
            int t = 0;
            for (int w = 0; w < 16; ++w) t += wcnt[w][tid];
            run[tid] += t;
        }
        __syncthreads();
    }
    for (int c = 0; c < C; ++c)
        for (int j = off[c] + cnt[c] + tid; j < off[c + 1]; j += 1024) sidx[j] = -1;
    for (int j = off[C] + tid; j < NP; j += 1024) sidx[j] = -1;
    for (int t = tid; t < NP / RT; t += 1024) {
        const int r = t * RT;
        int cls = -1;
        for (int c = 0; c < C; ++c)
            if (r >= off[c] && r < off[c + 1]) cls = c;
        tcls[t] = cls;
    }
}

// one workgroup per channel: for every class the fp32 sum over its pixels (sorted order), thread-strided then a fixed tree
__global__ void __launch_bounds__(256) whiten_mean_kernel(FeatView f, const int* __restrict__ hdr, const int* __restrict__ sidx,
                                                          float* __restrict__ mean, int k, int C) {
    __shared__ float red[4];
    const int ch = blockIdx.x;
    for (int c = 0; c < C; ++c) {
        const int nc = hdr[1 + c], o = hdr[17 + c];
        if (nc <= 1) continue;
        float s = 0.f;
        for (int j = threadIdx.x; j < nc; j += 256) s += feat_at(f, sidx[o + j], ch);
        s = block_sum4(s, red);
        if (threadIdx.x == 0) mean[(size_t)c * k + ch] = s / (float)nc;
        __syncthreads();
    }
}

// 64 channels x one 64-row tile per workgroup: bf16(x - mu[class]) (0 for the pad rows) to the channel-major image and,
// through LDS, to the pixel-major image (skipped when xp == nullptr).  Tiles of no class or of a class with n_c <= 1
// are not written: nobody reads them.
__global__ void __launch_bounds__(256) whiten_center_kernel(FeatView f, const int* __restrict__ hdr, const int* __restrict__ sidx,
                                                            const int* __restrict__ tcls, const float* __restrict__ mean,
                                                            bf16_t* __restrict__ ct, bf16_t* __restrict__ xp, int k, int NP) {
    const int cls = tcls[blockIdx.x];
    if (cls < 0 || hdr[1 + cls] <= 1) return;
    const int j0 = blockIdx.x * RT;
    stage_tile64(f, [=](int r) { return sidx[j0 + r]; }, RT, mean + (size_t)cls * k, blockIdx.y * 64, k, ct, NP, j0, xp);
}

// workgroup (group g, class c): S = Xc[class rows][group block]^T Xc[...], NT = s / 32 blocks of 32 channels a side
template <int NT>
__global__ void __launch_bounds__(256) whiten_cov_kernel(const bf16_t* __restrict__ ct, int NP, const int* __restrict__ hdr,
                                                         int G, bf16_t* __restrict__ dmat, float* __restrict__ lpart) {
    __shared__ float red[NT * NT * 1024];
    constexpr int s = 32 * NT;
    const int g = blockIdx.x, c = blockIdx.y;
    const int nc = hdr[1 + c];
    if (nc <= 1) {
        if (threadIdx.x == 0) lpart[c * G + g] = 0.f;
        return;
    }
    const int k0 = hdr[17 + c];
    const int ngroups = (hdr[18 + c] - k0) / 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const bf16_t* base[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) base[i] = ct + (size_t)(g * s + 32 * i + r) * NP + k0 + 16 * h;
    f32x16 acc[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x16{};
    for (int kg = wave; kg < ngroups; kg += 4) {
        uint4 a[2][NT];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < NT; ++i) a[t][i] = *(const uint4*)(base[i] + kg * 32 + 8 * t);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[t][i]),
                                                                        __builtin_bit_cast(bf16x8, a[t][j]), acc[i][j], 0, 0, 0);
    }
    // ((w0 + w1) + w2) + w3, in the accumulator's own order
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int q = 0; q < 16; ++q) red[((i * NT + j) * 16 + q) * 64 + lane] = acc[i][j][q];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[i][j][q] += red[((i * NT + j) * 16 + q) * 64 + lane];
        }
        __syncthreads();
    }
    if (wave != 0) return;
    const float inv = 1.f / (float)(nc - 1);
    bf16_t* dm = dmat + (size_t)(c * G + g) * s * s;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = 32 * i + (q & 3) + 8 * (q >> 2) + 4 * h, col = 32 * j + r;
                const float v = acc[i][j][q] * inv - (row == col ? 1.f : 0.f);
                sq += v * v;
                dm[row * s + col] = f2bf(v);
            }
    sq = wave_sum(sq);
    if (lane == 0) lpart[c * G + g] = sq / (float)(s * s);
}

// one wavefront per pixel: rows that the gradient product does not write (ignored label, class with n_c <= 1) := 0
__global__ void __launch_bounds__(256) whiten_zero_kernel(const int64_t* __restrict__ labels, const int* __restrict__ hdr, int n,
                                                          int C, int ignore_label, bf16_t* __restrict__ dfeat, int lddf, int k) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n) return;
    const long long l = labels[p];
    if (l != ignore_label && l >= 0 && l < C && hdr[1 + (int)l] > 1) return;
    uint4* row = (uint4*)(dfeat + (size_t)p * lddf);
    for (int v = threadIdx.x & 63; v < k / 8; v += 64) row[v] = uint4{0u, 0u, 0u, 0u};
}

// wavefront job (tile t, group g): C[c'][row] = sum_c D[c'][c] Xc[row][c] = dX[row][c']; a lane's registers 4q .. 4q+3
// are four consecutive channels of one row -> one 8-byte store into the pixel-major bf16 gradient row of its pixel
template <int NT>
__global__ void __launch_bounds__(256) whiten_grad_kernel(const bf16_t* __restrict__ dmat, const bf16_t* __restrict__ xp,
                                                          const int* __restrict__ hdr, const int* __restrict__ sidx,
                                                          const int* __restrict__ tcls, int njobs, int G, int k,
                                                          bf16_t* __restrict__ dfeat, int lddf, int accumulate, float weight) {
    constexpr int s = 32 * NT;
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (job >= njobs) return;
    const int t = job / G, g = job - t * G;
    const int cls = tcls[t];
    if (cls < 0) return;
    const int nc = hdr[1 + cls];
    if (nc <= 1) return;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const bf16_t* dp[NT];
    const bf16_t* xq[2];
#pragma unroll
    for (int i = 0; i < NT; ++i) dp[i] = dmat + ((size_t)(cls * G + g) * s + 32 * i + r) * s + 16 * h;
#pragma unroll
    for (int j = 0; j < 2; ++j) xq[j] = xp + (size_t)(t * RT + 32 * j + r) * k + g * s + 16 * h;
    f32x16 acc[NT][2];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};
#pragma unroll
    for (int kk = 0; kk < s; kk += 32) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            uint4 a[NT], b[2];
#pragma unroll
            for (int i = 0; i < NT; ++i) a[i] = *(const uint4*)(dp[i] + kk + 8 * u);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *(const uint4*)(xq[j] + kk + 8 * u);
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[i]),
                                                                        __builtin_bit_cast(bf16x8, b[j]), acc[i][j], 0, 0, 0);
        }
    }
    const float scale = 4.f * weight / ((float)(s * s) * (float)(nc - 1));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int pix = sidx[t * RT + 32 * j + r];
        if (pix < 0) continue;
        bf16_t* orow = dfeat + (size_t)pix * lddf + g * s;
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = 32 * i + 8 * q + 4 * h;
                float v0 = acc[i][j][4 * q] * scale, v1 = acc[i][j][4 * q + 1] * scale;
                float v2 = acc[i][j][4 * q + 2] * scale, v3 = acc[i][j][4 * q + 3] * scale;
                store4_bf16(orow + c, v0, v1, v2, v3, accumulate);
            }
    }
}

extern "C" size_t rgda_whiten_loss_workspace(int n, int k, int C, int groups) {
    if (n <= 0 || n > (1 << 24) || k <= 0 || groups <= 0 || k % groups || !class_count_ok(C) || !block_ok(k / groups)) return 0;
    return make_plan(n, k, C, groups).bytes;
}

extern "C" int rgda_whiten_loss(const float* feat, int b, int hw, int64_t ldc, int64_t ldb, const int64_t* labels, int k,
                                int C, int groups, int ignore_label, float* loss, void* dfeat, int lddf, int accumulate,
                                float weight, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (!feat || !labels || !loss || !ws) return RGDA_ERR_ARG;
    if (b <= 0 || hw <= 0 || k <= 0 || groups <= 0 || k % groups) return RGDA_ERR_ARG;
    const long long nn = (long long)b * hw;
    if (nn > (1 << 24)) return RGDA_ERR_ARG;
    if (!feat_view_ok(b, hw, ldc, ldb, k) || !grad_rows_ok(dfeat, lddf, k, 16)) return RGDA_ERR_ARG;
    if ((uintptr_t)ws & 255) return RGDA_ERR_ARG;          // the 16-byte fragment loads of ct, xp and dmat start at 256-byte offsets
    if (!class_count_ok(C)) return RGDA_ERR_UNSUPPORTED;
    if (!block_ok(k / groups)) return RGDA_ERR_UNSUPPORTED;
    const int n = (int)nn;
    const WhitenPlan p = make_plan(n, k, C, groups);
    if (ws_bytes < p.bytes) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    char* w = (char*)ws;
    int* hdr = (int*)w;
    int* sidx = (int*)(w + p.off_sidx);
    int* tcls = (int*)(w + p.off_tcls);
    float* mean = (float*)(w + p.off_mean);
    bf16_t* ct = (bf16_t*)(w + p.off_ct);
    bf16_t* xp = dfeat ? (bf16_t*)(w + p.off_xp) : nullptr;
    bf16_t* dmat = (bf16_t*)(w + p.off_dmat);
    float* lpart = (float*)(w + p.off_lpart);
    const FeatView f{feat, (long long)ldc, (long long)ldb, hw, n};
    const int G = groups, NT = p.s / 32, tiles = p.NP / RT;
    whiten_index_kernel<<<1, 1024, 0, st>>>(labels, n, C, ignore_label, p.NP, hdr, sidx, tcls);
    RGDA_CHECK_LAUNCH();
    whiten_mean_kernel<<<k, 256, 0, st>>>(f, hdr, sidx, mean, k, C);
    RGDA_CHECK_LAUNCH();
    whiten_center_kernel<<<dim3(tiles, cdiv(k, 64)), 256, 0, st>>>(f, hdr, sidx, tcls, mean, ct, xp, k, p.NP);
    RGDA_CHECK_LAUNCH();
    const dim3 cg(G, C);
    switch (NT) {
        case 1: whiten_cov_kernel<1><<<cg, 256, 0, st>>>(ct, p.NP, hdr, G, dmat, lpart); break;
        case 2: whiten_cov_kernel<2><<<cg, 256, 0, st>>>(ct, p.NP, hdr, G, dmat, lpart); break;
        case 3: whiten_cov_kernel<3><<<cg, 256, 0, st>>>(ct, p.NP, hdr, G, dmat, lpart); break;
        default: whiten_cov_kernel<4><<<cg, 256, 0, st>>>(ct, p.NP, hdr, G, dmat, lpart); break;
    }
    RGDA_CHECK_LAUNCH();
    if (rows_loss_sum(lpart, C * G, loss, weight, st) != RGDA_OK) return RGDA_ERR_LAUNCH;
    if (!dfeat) return RGDA_OK;
    bf16_t* df = (bf16_t*)dfeat;
    if (!accumulate) {
        whiten_zero_kernel<<<cdiv(n, 4), 256, 0, st>>>(labels, hdr, n, C, ignore_label, df, lddf, k);
        RGDA_CHECK_LAUNCH();
    }
    const int njobs = tiles * G;
    const int grid = cdiv(njobs, 4);
    switch (NT) {
        case 1: whiten_grad_kernel<1><<<grid, 256, 0, st>>>(dmat, xp, hdr, sidx, tcls, njobs, G, k, df, lddf, accumulate, weight); break;
        case 2: whiten_grad_kernel<2><<<grid, 256, 0, st>>>(dmat, xp, hdr, sidx, tcls, njobs, G, k, df, lddf, accumulate, weight); break;
        case 3: whiten_grad_kernel<3><<<grid, 256, 0, st>>>(dmat, xp, hdr, sidx, tcls, njobs, G, k, df, lddf, accumulate, weight); break;
        default: whiten_grad_kernel<4><<<grid, 256, 0, st>>>(dmat, xp, hdr, sidx, tcls, njobs, G, k, df, lddf, accumulate, weight); break;
    }
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
