// Multi-kernel MMD domain loss (regda/gast/mmd.py::MMDLoss, kernel_type 'rbf' and 'linear'): forward and the gradient
// w.r.t. both feature maps, deterministic (no atomics).  `total` = the source rows followed by the target rows, n = ns + nt.
//
//   mean   : per channel the two domain sums (fp32, fixed order) -> mean_s, mean_t, mu = (sum_s + sum_t) / n    mmd_mean_kernel
//   centre : Xc = bf16(total - mu), once, in two layouts: pixel-major [n_pad][d] (the Gram product sums over channels)
//            and channel-major [d][n_pad] (the gradient product sums over pixels); n_pad = n rounded up to 128, the
//            padding zero                                                               mmd_center_kernel
//   norms  : r_i = sum_c Xc[i][c]^2 (fp32, of the rounded row); csum[c] = sum_i Xc[i][c]     rows_sumsq, mmd_colsum_kernel
//   bw     : bw = fix_sigma, or (2 n sum r_i - 2 |csum|^2) / (n^2 - n) = the mean pairwise squared distance; / kernel_mul^(kernel_num / 2);
//            1 / bw_q = 1 / (bw kernel_mul^q) to the workspace -- on the device, no read-back          mmd_bandwidth_kernel
//   pairs  : one wavefront per upper 128 x 128 tile of the n x n matrix, K = d: g = Xc Xc^T, l2 = max(r_i + r_j - 2 g, 0)
//            (0 on the diagonal), kappa = sum_q exp(-l2 / bw_q), s_ij = a_i a_j with a = 1/ns (source), -1/nt (target),
//            0 (padding); the tile's sum of s kappa (twice off the diagonal) -> lpart; W = bf16(s sum_q exp(-l2 / bw_q) / bw_q)
//            (0 on the diagonal) to both triangles of W [n_pad][n_pad]; the row sums (and, off the diagonal, the column
//            sums) of the rounded W per tile -> rp[other tile index][row]                  mmd_pair_kernel
//   reduce : rho_i = sum over the tile columns of rp, in order; loss[0] += weight * sum(lpart), in order     mmd_rho_kernel, rows_loss_sum
//   grad   : C[c][p] = sum_j Xc^T[c][j] W[p][j] (the shape of coral_grad_kernel);
//            dfeat[p][c] (+)= -4 weight (rho_p Xc[p][c] - C[c][p])                           mmd_grad_kernel
//   linear : L = |mean_s - mean_t|^2 / d; rows 2 (mean_s - mean_t) / (d ns), -2 (...) / (d nt)   mmd_linear_loss_kernel, mmd_linear_grad_kernel
//
// d L / d x_i = sum_j 2 s_ij kappa'(l2_ij) 2 (x_i - x_j) with kappa' = -sum_q exp(-l2 / bw_q) / bw_q (the bandwidth is a
// constant of the backward, as in the reference: it is taken from `.data`), which is the -4 (rho_i x_i - sum_j W_ij x_j)
// above; distances do not see the shift by mu.  The feature view, the staging tile, the sums and the gradient store are
// those of feat_rows.h.
#include "feat_rows.h"

namespace {

constexpr int MAX_KERNELS = 8;
constexpr int MAX_ROWS = 32768;  // W is n_pad^2 bf16: 2 GB at the limit

struct MmdPlan {
    int d, ns, nt, n, np, T, U;
    size_t off_mean, off_xp, off_xt, off_r, off_rho, off_csum, off_bw, off_rp, off_lpart, off_w, bytes;
};

MmdPlan make_plan(int ns, int nt, int d) {
    MmdPlan p;
    p.d = d; p.ns = ns; p.nt = nt; p.n = ns + nt;
    p.np = (p.n + CT - 1) / CT * CT;
    p.T = p.np / CT;
    p.U = p.T * (p.T + 1) / 2;
    size_t o = 0;
    p.off_mean = o;  o += a256((size_t)3 * d * 4);
    p.off_xp = o;    o += a256((size_t)p.np * d * 2);
    p.off_xt = o;    o += a256((size_t)d * p.np * 2);
    p.off_r = o;     o += a256((size_t)p.np * 4);
    p.off_rho = o;   o += a256((size_t)p.np * 4);
    p.off_csum = o;  o += a256((size_t)d * 4);
    p.off_bw = o;    o += 256;
    p.off_rp = o;    o += a256((size_t)p.T * p.np * 4);
    p.off_lpart = o; o += a256((size_t)p.U * 4);
    p.off_w = o;     o += a256((size_t)p.np * p.np * 2);
    p.bytes = o;
    return p;
}

}  // namespace

// one workgroup per channel: fp32 sums over the source rows and over the target rows, thread-strided then a fixed tree;
// mean[c] = mean_s, mean[d + c] = mean_t, mean[2d + c] = mu
__global__ void __launch_bounds__(256) mmd_mean_kernel(FeatView fs, FeatView ft, float* __restrict__ mean, int d) {
    __shared__ float red[2][4];
    const int c = blockIdx.x;
    float ss = feat_channel_partial(fs, c), st = feat_channel_partial(ft, c);
    ss = block_sum4(ss, red[0]);
    st = block_sum4(st, red[1]);
    if (threadIdx.x == 0) {
        mean[c] = ss / (float)fs.n;
        mean[d + c] = st / (float)ft.n;
        mean[2 * d + c] = (ss + st) / (float)(fs.n + ft.n);
    }
}

// 64 channels x 64 rows of one domain per workgroup: bf16(x - mu) to the channel-major image (coalesced along the
// rows) and, through LDS, to the pixel-major image (coalesced along the channels)
__global__ void __launch_bounds__(256) mmd_center_kernel(FeatView fs, FeatView ft, const float* __restrict__ mu,
                                                         bf16_t* __restrict__ xt, bf16_t* __restrict__ xp, int np, int d) {
    const bool tgt = blockIdx.z != 0;
    const FeatView f = tgt ? ft : fs;
    const int g0 = blockIdx.x * 64;
    if (g0 >= f.n) return;
    stage_tile64(f, [g0](int r) { return g0 + r; }, f.n - g0, mu, blockIdx.y * 64, d, xt, np, (tgt ? fs.n : 0) + g0, xp);
}

// one workgroup per channel: csum[c] = sum over the rows of the channel-major image (the padding is zero)
__global__ void __launch_bounds__(256) mmd_colsum_kernel(const bf16_t* __restrict__ xt, float* __restrict__ csum, int np) {
    __shared__ float red[4];
    const bf16_t* row = xt + (size_t)blockIdx.x * np;
    float s = 0.f;
    for (int k = threadIdx.x; k < np; k += 256) s += bf2f(row[k]);
    s = block_sum4(s, red);
    if (threadIdx.x == 0) csum[blockIdx.x] = s;
}

// one workgroup: the bandwidth (MMDLoss.guassian_kernel, mmd.py:31-36) -> bwv[q] = 1 / (bw kernel_mul^q), q < kernel_num;
// bwv[8] = bw of q = 0.  inv_pairs = 1 / (n^2 - n), inv_div = 1 / kernel_mul^(kernel_num / 2)
__global__ void __launch_bounds__(256) mmd_bandwidth_kernel(const float* __restrict__ r, const float* __restrict__ csum, int n,
                                                            int np, int d, float fix_sigma, float inv_pairs, float inv_div,
                                                            float kernel_mul, int kernel_num, float* __restrict__ bwv) {
    __shared__ float red[4];
    float sr = 0.f, sc = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) sr += r[i];
    for (int c = threadIdx.x; c < d; c += 256) sc += csum[c] * csum[c];
    sr = block_sum4(sr, red);
    __syncthreads();
    sc = block_sum4(sc, red);
    if (threadIdx.x == 0) {
        float bw = fix_sigma > 0.f ? fix_sigma : (2.f * (float)n * sr - 2.f * sc) * inv_pairs;
        bw *= inv_div;
        bwv[8] = bw;
        float m = 1.f;
        for (int q = 0; q < MAX_KERNELS; ++q) {
            bwv[q] = q < kernel_num ? 1.f / (bw * m) : 0.f;
            m *= kernel_mul;
        }
    }
}

// job = upper tile (I, J), one wavefront each.  Row i of the tile is a P row, column j a Q row of the Gram product.
// The epilogue goes through LDS one 32 x 32 accumulator block at a time (a rolled loop: the 256 accumulator elements of
// a lane with an exponential loop each do not fit the register file when unrolled): a lane then owns 16 consecutive
// columns of one row -> 32-byte stores of W, and for the mirrored block 16 consecutive rows of one column.  The four
// wavefronts of a workgroup take the same path (a wavefront past the last job repeats it and stores nothing), so the
// workgroup barriers are uniform.
#define MMD_DUMP(ii, jj)                                                                      \
    case (ii) * 4 + (jj):                                                                     \
        _Pragma("unroll") for (int reg = 0; reg < 16; ++reg)                                  \
            gl[wv][(reg & 3) + 8 * (reg >> 2) + 4 * h][cl] = acc[ii][jj][reg];                \
        break;
__global__ void __launch_bounds__(256, 1) mmd_pair_kernel(const bf16_t* __restrict__ xp, const float* __restrict__ r,
                                                          const float* __restrict__ bwv, int kernel_num, int ns, int n, int np,
                                                          int d, int T, int njobs, float as, float at, bf16_t* __restrict__ W,
                                                          float* __restrict__ rp, float* __restrict__ lpart) {
    __shared__ float gl[4][32][33];
    __shared__ bf16_t wl[4][32][34];
    __shared__ float racc[4][CT], cacc[4][CT];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, cl = lane & 31, h = lane >> 5;
    const bool active = blockIdx.x * 4 + wv < njobs;
    const int job = active ? blockIdx.x * 4 + wv : njobs - 1;
    int I, J;
    upper_tile(job, T, I, J);
    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x16{};
    tile_nt<4>(xp, d, I * CT, np - 1, xp, d, J * CT, np - 1, 0, d, acc);
    racc[wv][lane] = racc[wv][lane + 64] = 0.f;
    cacc[wv][lane] = cacc[wv][lane + 64] = 0.f;
    const float ibv = bwv[lane & 7];             // lane q holds 1 / bw_q: read back per q with a lane broadcast
    const int own = lane >> 1, e0 = (lane & 1) * 16;      // the row (column) a lane owns and its first column (row)
    float lsum = 0.f;
#pragma unroll 1
    for (int t = 0; t < 16; ++t) {
        const int i = t >> 2, j = t & 3;
        __syncthreads();                         // the previous block's reads of gl and wl are done
        switch (t) {
            MMD_DUMP(0, 0) MMD_DUMP(0, 1) MMD_DUMP(0, 2) MMD_DUMP(0, 3)
            MMD_DUMP(1, 0) MMD_DUMP(1, 1) MMD_DUMP(1, 2) MMD_DUMP(1, 3)
            MMD_DUMP(2, 0) MMD_DUMP(2, 1) MMD_DUMP(2, 2) MMD_DUMP(2, 3)
            MMD_DUMP(3, 0) MMD_DUMP(3, 1) MMD_DUMP(3, 2) MMD_DUMP(3, 3)
        }
        __syncthreads();
        const int ib0 = I * CT + 32 * i, jb0 = J * CT + 32 * j;
        {
            const int ig = ib0 + own, jb = jb0 + e0;
            const float ri = r[ig];
            const float ai = ig < ns ? as : (ig < n ? at : 0.f);
            float rs = 0.f;
            unsigned pk[8];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int jg = jb + e;
                const float aj = jg < ns ? as : (jg < n ? at : 0.f);
                const float l2 = ig == jg ? 0.f : fmaxf(ri + r[jg] - 2.f * gl[wv][own][e0 + e], 0.f);
                const float s = ai * aj;
                float kap = 0.f, wsum = 0.f;
                for (int q = 0; q < kernel_num; ++q) {
                    const float ib = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ibv), q));
                    const float ex = __expf(-l2 * ib);
                    kap += ex;
                    wsum += ex * ib;
                }
                lsum += s * kap;
                const bf16_t w = ig == jg ? (bf16_t)0 : f2bf(s * wsum);
                rs += bf2f(w);
                wl[wv][own][e0 + e] = w;
                if (e & 1) pk[e >> 1] |= (unsigned)w << 16;
                else pk[e >> 1] = w;
            }
            if (active) {
                uint4* dst = (uint4*)(W + (size_t)ig * np + jb);
                dst[0] = uint4{pk[0], pk[1], pk[2], pk[3]};
                dst[1] = uint4{pk[4], pk[5], pk[6], pk[7]};
            }
            rs += __shfl_xor(rs, 1, 64);
            if (!(lane & 1)) racc[wv][32 * i + own] += rs;
        }
        __syncthreads();
        if (I != J) {                            // the mirrored block: column `own`, rows e0 .. e0 + 15
            float cs = 0.f;
            unsigned pk[8];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const bf16_t w = wl[wv][e0 + e][own];
                cs += bf2f(w);
                if (e & 1) pk[e >> 1] |= (unsigned)w << 16;
                else pk[e >> 1] = w;
            }
            if (active) {
                uint4* dst = (uint4*)(W + (size_t)(jb0 + own) * np + ib0 + e0);
                dst[0] = uint4{pk[0], pk[1], pk[2], pk[3]};
                dst[1] = uint4{pk[4], pk[5], pk[6], pk[7]};
            }
            cs += __shfl_xor(cs, 1, 64);
            if (!(lane & 1)) cacc[wv][32 * j + own] += cs;
        }
    }
    __syncthreads();
    if (I != J) lsum *= 2.f;
    lsum = wave_sum(lsum);
    if (!active) return;
    rp[(size_t)J * np + I * CT + lane] = racc[wv][lane];
    rp[(size_t)J * np + I * CT + lane + 64] = racc[wv][lane + 64];
    if (I != J) {
        rp[(size_t)I * np + J * CT + lane] = cacc[wv][lane];
        rp[(size_t)I * np + J * CT + lane + 64] = cacc[wv][lane + 64];
    }
    if (lane == 0) lpart[job] = lsum;
}
#undef MMD_DUMP

__global__ void __launch_bounds__(256) mmd_rho_kernel(const float* __restrict__ rp, float* __restrict__ rho, int np, int T) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    float s = 0.f;
    for (int b = 0; b < T; ++b) s += rp[(size_t)b * np + i];
    rho[i] = s;
}

// job < js: source, else target.  C[c][p] = sum_j Xc^T[c][j] W[p][j]: a lane's registers 4g .. 4g+3 are four consecutive
// channels of one pixel -> one 8-byte store into the pixel-major bf16 gradient rows
__global__ void __launch_bounds__(256, 1) mmd_grad_kernel(const bf16_t* __restrict__ xt, const bf16_t* __restrict__ xp,
                                                          const bf16_t* __restrict__ W, const float* __restrict__ rho, GradRows gs,
                                                          GradRows gt, int js, int njobs, int d, int np, float scale, int accumulate) {
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (job >= njobs) return;
    const bool tgt = job >= js;
    const GradRows g = tgt ? gt : gs;
    const int jj = tgt ? job - js : job;
    const int T = (d + CT - 1) / CT;
    const int mt = jj % T, nt = jj / T;
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{};
    tile_nt<2>(xt, np, mt * CT, d - 1, W, np, g.row0 + nt * GN, g.row0 + g.n - 1, 0, np, acc);
    // row p of this side's gradient; a column loads its rho and its row of Xc once, then scale * (rho x - acc) per quad
    grad_tile_store(acc, mt, nt, g.n, d, accumulate, [=](int p) { return g.out + (size_t)p * g.ld; },
                    [=](int p) {
                        const bf16_t* xrow = xp + (size_t)(g.row0 + p) * d;
                        const float rh = rho[g.row0 + p];
                        return [=](F4 a, int c) {
                            const uint2 x = *(const uint2*)(xrow + c);
                            return F4{scale * (rh * __uint_as_float(x.x << 16) - a.v0),
                                      scale * (rh * __uint_as_float(x.x & 0xffff0000u) - a.v1),
                                      scale * (rh * __uint_as_float(x.y << 16) - a.v2),
                                      scale * (rh * __uint_as_float(x.y & 0xffff0000u) - a.v3)};
                        };
                    });
}

// linear MMD (MMDLoss.forward_linear, mmd.py:41-44): loss[0] += scale * sum_c (mean_s - mean_t)^2, scale = weight / d
__global__ void __launch_bounds__(256) mmd_linear_loss_kernel(const float* __restrict__ mean, int d, float* loss, float scale) {
    __shared__ float red[4];
    float s = 0.f;
    for (int c = threadIdx.x; c < d; c += 256) {
        const float dl = mean[c] - mean[d + c];
        s += dl * dl;
    }
    s = block_sum4(s, red);
    if (threadIdx.x == 0) loss[0] += scale * s;
}

// one thread per (row, four channels); blockIdx.y: 0 source, 1 target.  sc = +/- 2 weight / (d n_side)
__global__ void __launch_bounds__(256) mmd_linear_grad_kernel(const float* __restrict__ mean, GradRows gs, GradRows gt, int d,
                                                              float scs, float sct, int accumulate) {
    const GradRows g = blockIdx.y ? gt : gs;
    if (!g.out) return;
    const float sc = blockIdx.y ? sct : scs;
    const int q = d >> 2;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)g.n * q) return;
    const int row = (int)(e / q), c = (int)(e - (long long)row * q) * 4;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = sc * (mean[c + k] - mean[d + c + k]);
    store4_bf16(g.out + (size_t)row * g.ld + c, v[0], v[1], v[2], v[3], accumulate);
}

extern "C" size_t rgda_mmd_loss_workspace(int ns, int nt, int d) {
    if (ns < 2 || nt < 2 || d < 32 || (d & 31) || (long long)ns + nt > MAX_ROWS) return 0;
    return make_plan(ns, nt, d).bytes;
}

extern "C" int rgda_mmd_loss(const float* feat_s, int bs, int hws, int64_t ldcs, int64_t ldbs, const float* feat_t, int bt,
                             int hwt, int64_t ldct, int64_t ldbt, int d, int kernel_type, float kernel_mul, int kernel_num,
                             float fix_sigma, float* loss, void* dfeat_s, int ldds, void* dfeat_t, int lddt, int accumulate,
                             float weight, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (!feat_s || !feat_t || !loss || !ws || ((uintptr_t)ws & 255)) return RGDA_ERR_ARG;
    if (bs <= 0 || bt <= 0 || hws <= 0 || hwt <= 0 || d < 32 || (d & 31)) return RGDA_ERR_ARG;
    if (kernel_type != RGDA_MMD_RBF && kernel_type != RGDA_MMD_LINEAR) return RGDA_ERR_ARG;
    if (kernel_num < 1 || !(kernel_mul > 0.f)) return RGDA_ERR_ARG;
    if (kernel_num > MAX_KERNELS) return RGDA_ERR_UNSUPPORTED;
    const long long ns = (long long)bs * hws, nt = (long long)bt * hwt;
    if (ns < 2 || nt < 2) return RGDA_ERR_ARG;
    if (ns + nt > MAX_ROWS) return RGDA_ERR_UNSUPPORTED;
    if (!feat_view_ok(bs, hws, ldcs, ldbs, d) || !feat_view_ok(bt, hwt, ldct, ldbt, d)) return RGDA_ERR_ARG;
    if (!grad_rows_ok(dfeat_s, ldds, d, 8) || !grad_rows_ok(dfeat_t, lddt, d, 8)) return RGDA_ERR_ARG;
    const MmdPlan p = make_plan((int)ns, (int)nt, d);
    // the linear form uses the means only: the first region of the plan
    if (ws_bytes < (kernel_type == RGDA_MMD_LINEAR ? p.off_xp : p.bytes)) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    char* w = (char*)ws;
    float* mean = (float*)(w + p.off_mean);
    const FeatView fs{feat_s, (long long)ldcs, (long long)ldbs, hws, (int)ns};
    const FeatView ft{feat_t, (long long)ldct, (long long)ldbt, hwt, (int)nt};
    const GradRows gs{(bf16_t*)dfeat_s, 0, (int)ns, ldds};
    const GradRows gt{(bf16_t*)dfeat_t, (int)ns, (int)nt, lddt};
    const bool grad = dfeat_s || dfeat_t;
    mmd_mean_kernel<<<d, 256, 0, st>>>(fs, ft, mean, d);
    RGDA_CHECK_LAUNCH();
    if (kernel_type == RGDA_MMD_LINEAR) {
        mmd_linear_loss_kernel<<<1, 256, 0, st>>>(mean, d, loss, weight / (float)d);
        RGDA_CHECK_LAUNCH();
        if (!grad) return RGDA_OK;
        const long long most = (ns > nt ? ns : nt) * (d >> 2);
        mmd_linear_grad_kernel<<<dim3(cdiv(most, 256), 2), 256, 0, st>>>(mean, gs, gt, d, 2.f * weight / ((float)d * (float)ns),
                                                                        -2.f * weight / ((float)d * (float)nt), accumulate);
        RGDA_CHECK_LAUNCH();
        return RGDA_OK;
    }
    bf16_t* xp = (bf16_t*)(w + p.off_xp);
    bf16_t* xt = (bf16_t*)(w + p.off_xt);
    float* r = (float*)(w + p.off_r);
    float* rho = (float*)(w + p.off_rho);
    float* csum = (float*)(w + p.off_csum);
    float* bwv = (float*)(w + p.off_bw);
    float* rp = (float*)(w + p.off_rp);
    float* lpart = (float*)(w + p.off_lpart);
    bf16_t* W = (bf16_t*)(w + p.off_w);
    const int n = p.n, np = p.np;
    // the padding of both images must be zero (it enters the row norms, the column sums and the gradient product)
    if (np != n) {
        if (zero_bytes(xp + (size_t)n * d, (size_t)(np - n) * d * 2, stream) != RGDA_OK) return RGDA_ERR_LAUNCH;
        if (zero_bytes(xt, (size_t)d * np * 2, stream) != RGDA_OK) return RGDA_ERR_LAUNCH;
    }
    mmd_center_kernel<<<dim3(cdiv(ns > nt ? ns : nt, 64), cdiv(d, 64), 2), 256, 0, st>>>(fs, ft, mean + 2 * d, xt, xp, np, d);
    RGDA_CHECK_LAUNCH();
    if (rows_sumsq(xp, np, d, r, st) != RGDA_OK) return RGDA_ERR_LAUNCH;
    mmd_colsum_kernel<<<d, 256, 0, st>>>(xt, csum, np);
    RGDA_CHECK_LAUNCH();
    const double pairs = (double)n * (double)n - (double)n;
    double div = 1.0;
    for (int q = 0; q < kernel_num / 2; ++q) div *= (double)kernel_mul;
    mmd_bandwidth_kernel<<<1, 256, 0, st>>>(r, csum, n, np, d, fix_sigma, (float)(1.0 / pairs), (float)(1.0 / div), kernel_mul,
                                            kernel_num, bwv);
    RGDA_CHECK_LAUNCH();
    mmd_pair_kernel<<<cdiv(p.U, 4), 256, 0, st>>>(xp, r, bwv, kernel_num, (int)ns, n, np, d, p.T, p.U, 1.f / (float)ns,
                                                  -1.f / (float)nt, W, rp, lpart);
    RGDA_CHECK_LAUNCH();
    if (rows_loss_sum(lpart, p.U, loss, weight, st) != RGDA_OK) return RGDA_ERR_LAUNCH;
    if (!grad) return RGDA_OK;
    mmd_rho_kernel<<<cdiv(np, 256), 256, 0, st>>>(rp, rho, np, p.T);
    RGDA_CHECK_LAUNCH();
    const int T = cdiv(d, CT);
    const int js = dfeat_s ? T * cdiv(ns, GN) : 0;
    const int jt = dfeat_t ? T * cdiv(nt, GN) : 0;
    mmd_grad_kernel<<<cdiv(js + jt, 4), 256, 0, st>>>(xt, xp, W, rho, gs, gt, js, js + jt, d, np, -4.f * weight, accumulate);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
