// CORAL domain loss (regda/gast/coral.py::CoralLoss, is_sqrt=False) as used by Aligner.align_domain
// (regda/gast/alignment.py:79-84): forward and the gradient w.r.t. both feature maps, deterministic (no atomics).
//
//   mean   : mu[c] = sum of the rows / n, fp32, fixed order                          coral_mean_kernel
//   centre : Xc = bf16(X - mu), once, in two layouts: channel-major [d][n_pad] (the covariance product sums over
//            pixels) and pixel-major [n][d] (the gradient product sums over channels)   coral_center_kernel
//   cov    : per (upper 128x128 tile of the d x d matrix, K chunk of one domain's pixels): Xc^T Xc partials, fp32,
//            one wavefront per job, split-K partials to the workspace                 coral_cov_kernel
//   reduce : D = sum(source partials) / (ns - 1) - sum(target partials) / (nt - 1) in a fixed order; bf16(D) to both
//            triangles; per-band sum of D^2                                           coral_reduce_kernel
//   loss   : loss[0] += weight * sum(D^2) / (4 d^2), one thread, fixed order            rows_loss_sum
//   grad   : dX^T = D . Xc^T  ->  dfeat = (+/-) weight / (d^2 (n - 1)) * dX (+ dfeat)      coral_grad_kernel
//
// Both products are C[m][n] = sum_k P[m][k] Q[n][k] with P and Q row-major bf16 and K contiguous: the tile routine of
// gram_tile.h (a 128 x 128 tile per wavefront, fragments loaded straight from global memory, no LDS).  The feature view,
// the staging tile, the sums and the gradient store are those of feat_rows.h.
#include "feat_rows.h"

namespace {

constexpr int TILE_FLOATS = CT * CT;

int round32(int x) { return (x + 31) & ~31; }

// split-K of the covariance product: a few jobs per domain and upper tile so that about 1024 wavefronts (one per
// SIMD of the 256 CUs) run in one round
struct CoralPlan {
    int d, ns, nt, nsp, ntp, T, U, Ss, St, chs, cht;
    size_t off_mean, off_cts, off_ctt, off_xs, off_xt, off_part, off_dbf, off_lpart, bytes;
};

void split(int npad, int U, int& S, int& chunk) {
    int want = 1024 / (2 * U);
    if (want < 1) want = 1;
    if (want > npad / KG) want = npad / KG;
    chunk = round32(cdiv(npad, want));
    S = cdiv(npad, chunk);
}

CoralPlan make_plan(int ns, int nt, int d) {
    CoralPlan p;
    p.d = d; p.ns = ns; p.nt = nt;
    p.nsp = round32(ns); p.ntp = round32(nt);
    p.T = cdiv(d, CT);
    p.U = p.T * (p.T + 1) / 2;
    split(p.nsp, p.U, p.Ss, p.chs);
    split(p.ntp, p.U, p.St, p.cht);
    size_t o = 0;
    p.off_mean = o;  o += a256((size_t)2 * d * 4);
    p.off_cts = o;   o += a256((size_t)d * p.nsp * 2);
    p.off_ctt = o;   o += a256((size_t)d * p.ntp * 2);
    p.off_xs = o;    o += a256((size_t)ns * d * 2);
    p.off_xt = o;    o += a256((size_t)nt * d * 2);
    p.off_part = o;  o += a256((size_t)p.U * (p.Ss + p.St) * TILE_FLOATS * 4);
    p.off_dbf = o;   o += a256((size_t)d * d * 2);
    p.off_lpart = o; o += a256((size_t)p.U * 4 * 4);
    p.bytes = o;
    return p;
}

}  // namespace

// one workgroup per (channel, domain): fp32 sum over the n rows, thread-strided then a fixed tree
__global__ void __launch_bounds__(256) coral_mean_kernel(FeatView fs, FeatView ft, float* __restrict__ mean, int d) {
    __shared__ float red[4];
    const int c = blockIdx.x;
    const FeatView f = blockIdx.y ? ft : fs;
    const float s = block_sum4(feat_channel_partial(f, c), red);
    if (threadIdx.x == 0) mean[blockIdx.y * d + c] = s / (float)f.n;
}

// 64 channels x 64 rows per workgroup: bf16(x - mu) to the channel-major image (coalesced along the rows) and,
// through LDS, to the pixel-major image (coalesced along the channels; skipped when xs == nullptr)
__global__ void __launch_bounds__(256) coral_center_kernel(FeatView fs, FeatView ft, const float* __restrict__ mean,
                                                           bf16_t* cts, bf16_t* ctt, int ldcs, int ldct,
                                                           bf16_t* xs, bf16_t* xt, int d) {
    const bool tgt = blockIdx.z != 0;
    const FeatView f = tgt ? ft : fs;
    const int g0 = blockIdx.x * 64;
    if (g0 >= f.n) return;
    stage_tile64(f, [g0](int r) { return g0 + r; }, f.n - g0, mean + (tgt ? d : 0), blockIdx.y * 64, d, tgt ? ctt : cts,
                 tgt ? ldct : ldcs, g0, tgt ? xt : xs);
}

// job = u * (Ss + St) + q: upper tile u, K chunk q (q < Ss: source, else target).  Partials in the accumulator's own
// order: part[job][((i * 4 + j) * 16 + reg) * 64 + lane] (every store instruction writes 256 contiguous bytes)
__global__ void __launch_bounds__(256, 1) coral_cov_kernel(const bf16_t* __restrict__ cts, const bf16_t* __restrict__ ctt,
                                                           int nsp, int ntp, int Ss, int St, int chs, int cht, int T,
                                                           int njobs, int d, float* __restrict__ part) {
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (job >= njobs) return;
    const int S = Ss + St;
    const int u = job / S, q = job - u * S;
    int I, J;
    upper_tile(u, T, I, J);
    const bool tgt = q >= Ss;
    const bf16_t* X = tgt ? ctt : cts;
    const int ld = tgt ? ntp : nsp, ch = tgt ? cht : chs;
    const int k0 = (tgt ? q - Ss : q) * ch;
    const int k1 = min(k0 + ch, ld);
    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x16{};
    tile_nt<4>(X, ld, I * CT, d - 1, X, ld, J * CT, d - 1, k0, k1, acc);
    const int lane = threadIdx.x & 63;
    float* out = part + (size_t)job * TILE_FLOATS + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) out[((i * 4 + j) * 16 + r) * 64] = acc[i][j][r];
}

// one workgroup per (upper tile, 32-row band): D in fp32 from the partials (source chunks in order, then target
// chunks), bf16(D) to D[row][col] and, for tiles off the diagonal, through LDS to D[col][row]; the band's sum of D^2
// (off-diagonal tiles count twice) -> lpart[u * 4 + band]
__global__ void __launch_bounds__(256) coral_reduce_kernel(const float* __restrict__ part, int Ss, int St, int T, int d,
                                                           float inv_s, float inv_t, bf16_t* __restrict__ dbf,
                                                           float* __restrict__ lpart) {
    __shared__ float tr[CT][33];
    __shared__ float red[4];
    const int u = blockIdx.x, band = blockIdx.y;
    int I, J;
    upper_tile(u, T, I, J);
    const int S = Ss + St;
    const float* pb = part + (size_t)u * S * TILE_FLOATS + band * 4096;
    float sq = 0.f;
    for (int m = 0; m < 16; ++m) {
        const int e = threadIdx.x + 256 * m;
        const int lane = e & 63, reg = (e >> 6) & 15, j = e >> 10;
        float cs = 0.f, ct = 0.f;
        for (int q = 0; q < Ss; ++q) cs += pb[(size_t)q * TILE_FLOATS + e];
        for (int q = Ss; q < S; ++q) ct += pb[(size_t)q * TILE_FLOATS + e];
        const float v = cs * inv_s - ct * inv_t;
        const int rl = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), cl = 32 * j + (lane & 31);
        const int row = I * CT + 32 * band + rl, col = J * CT + cl;
        tr[cl][rl] = v;
        if (row < d && col < d) {
            dbf[(size_t)row * d + col] = f2bf(v);
            sq += v * v;
        }
    }
    if (I != J) {
        __syncthreads();
        for (int m = 0; m < 16; ++m) {
            const int e = threadIdx.x + 256 * m;
            const int rl = e & 31, cl = e >> 5;
            const int row = I * CT + 32 * band + rl, col = J * CT + cl;
            if (row < d && col < d) dbf[(size_t)col * d + row] = f2bf(tr[cl][rl]);
        }
        sq *= 2.f;
    }
    sq = block_sum4(sq, red);
    if (threadIdx.x == 0) lpart[u * 4 + band] = sq;
}

// job < js: source, else target.  C[c'][p] = sum_c D[c'][c] Xc[p][c] = dX[p][c']: a lane's registers 4g .. 4g+3 are
// four consecutive channels of one pixel -> one 8-byte store into the pixel-major bf16 gradient rows
struct GradSide {
    const bf16_t* x;
    bf16_t* out;
    int n, ld;
    float scale;
};
__global__ void __launch_bounds__(256, 1) coral_grad_kernel(const bf16_t* __restrict__ dbf, GradSide gs, GradSide gt, int js,
                                                            int njobs, int d, int accumulate) {
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (job >= njobs) return;
    const bool tgt = job >= js;
    const GradSide g = tgt ? gt : gs;
    const int jj = tgt ? job - js : job;
    const int T = (d + CT - 1) / CT;
    const int mt = jj % T, nt = jj / T;
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};
    tile_nt<2>(dbf, d, mt * CT, d - 1, g.x, d, nt * GN, g.n - 1, 0, d, acc);
    // row p of this side's gradient; every column takes acc * scale
    grad_tile_store(acc, mt, nt, g.n, d, accumulate, [=](int p) { return g.out + (size_t)p * g.ld; },
                    [=](int) {
                        return [=](F4 a, int) { return F4{a.v0 * g.scale, a.v1 * g.scale, a.v2 * g.scale, a.v3 * g.scale}; };
                    });
}

extern "C" size_t rgda_coral_loss_workspace(int ns, int nt, int d) {
    if (ns < 2 || nt < 2 || d < 32 || (d & 31)) return 0;
    return make_plan(ns, nt, d).bytes;
}

extern "C" int rgda_coral_loss(const float* feat_s, int bs, int hws, int64_t ldcs, int64_t ldbs,
                               const float* feat_t, int bt, int hwt, int64_t ldct, int64_t ldbt, int d, float* loss,
                               void* dfeat_s, int ldds, void* dfeat_t, int lddt, int accumulate, float weight, void* ws,
                               size_t ws_bytes, rgda_stream_t stream) {
    if (!feat_s || !feat_t || !loss || !ws) return RGDA_ERR_ARG;
    if (bs <= 0 || bt <= 0 || hws <= 0 || hwt <= 0 || d < 32 || (d & 31)) return RGDA_ERR_ARG;
    const long long ns = (long long)bs * hws, nt = (long long)bt * hwt;
    if (ns < 2 || nt < 2 || ns > (1 << 30) || nt > (1 << 30)) return RGDA_ERR_ARG;
    if (!feat_view_ok(bs, hws, ldcs, ldbs, d) || !feat_view_ok(bt, hwt, ldct, ldbt, d)) return RGDA_ERR_ARG;
    if (!grad_rows_ok(dfeat_s, ldds, d, 8) || !grad_rows_ok(dfeat_t, lddt, d, 8)) return RGDA_ERR_ARG;
    const CoralPlan p = make_plan((int)ns, (int)nt, d);
    if (ws_bytes < p.bytes) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    char* w = (char*)ws;
    float* mean = (float*)(w + p.off_mean);
    bf16_t* cts = (bf16_t*)(w + p.off_cts);
    bf16_t* ctt = (bf16_t*)(w + p.off_ctt);
    const bool grad = dfeat_s || dfeat_t;
    bf16_t* xs = grad ? (bf16_t*)(w + p.off_xs) : nullptr;
    bf16_t* xt = grad ? (bf16_t*)(w + p.off_xt) : nullptr;
    float* part = (float*)(w + p.off_part);
    bf16_t* dbf = (bf16_t*)(w + p.off_dbf);
    float* lpart = (float*)(w + p.off_lpart);
    // the K padding of the channel-major images must be zero (it enters the covariance sums)
    if (p.nsp != ns && zero_bytes(cts, (size_t)d * p.nsp * 2, stream) != RGDA_OK) return RGDA_ERR_LAUNCH;
    if (p.ntp != nt && zero_bytes(ctt, (size_t)d * p.ntp * 2, stream) != RGDA_OK) return RGDA_ERR_LAUNCH;
    const FeatView fs{feat_s, (long long)ldcs, (long long)ldbs, hws, (int)ns};
    const FeatView ft{feat_t, (long long)ldct, (long long)ldbt, hwt, (int)nt};
    coral_mean_kernel<<<dim3(d, 2), 256, 0, st>>>(fs, ft, mean, d);
    RGDA_CHECK_LAUNCH();
    coral_center_kernel<<<dim3(cdiv(ns > nt ? ns : nt, 64), cdiv(d, 64), 2), 256, 0, st>>>(fs, ft, mean, cts, ctt, p.nsp,
                                                                                           p.ntp, xs, xt, d);
    RGDA_CHECK_LAUNCH();
    const int njobs = p.U * (p.Ss + p.St);
    coral_cov_kernel<<<cdiv(njobs, 4), 256, 0, st>>>(cts, ctt, p.nsp, p.ntp, p.Ss, p.St, p.chs, p.cht, p.T, njobs, d, part);
    RGDA_CHECK_LAUNCH();
    coral_reduce_kernel<<<dim3(p.U, 4), 256, 0, st>>>(part, p.Ss, p.St, p.T, d, 1.f / (float)(ns - 1), 1.f / (float)(nt - 1),
                                                      dbf, lpart);
    RGDA_CHECK_LAUNCH();
    if (rows_loss_sum(lpart, p.U * 4, loss, weight / (4.f * (float)d * (float)d), st) != RGDA_OK) return RGDA_ERR_LAUNCH;
    if (!grad) return RGDA_OK;
    const float dd = (float)d * (float)d;
    const int T = p.T;
    const int js = dfeat_s ? T * cdiv(ns, GN) : 0;
    const int jt = dfeat_t ? T * cdiv(nt, GN) : 0;
    const GradSide gs{xs, (bf16_t*)dfeat_s, (int)ns, ldds, weight / (dd * (float)(ns - 1))};
    const GradSide gt{xt, (bf16_t*)dfeat_t, (int)nt, lddt, -weight / (dd * (float)(nt - 1))};
    coral_grad_kernel<<<cdiv(js + jt, 4), 256, 0, st>>>(dbf, gs, gt, js, js + jt, d, accumulate);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
