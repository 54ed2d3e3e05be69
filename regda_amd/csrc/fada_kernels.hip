// Feature-space, class-level adversarial alignment: the kernels of PixelDiscriminator (regda/models/Discriminator.py:60-78,
// FADA, Wang et al. 2020) that the generic convolution routes do not provide.  DESIGN.md 4.2t.
//
//   X  [b*h*w][k] bf16        the f32 NCHW feature map packed pixel-major (rgda_feat_pack_rows; its inverse for dx)
//   a1 [M][ndf], a2 [M][ndf/2]  D.0 / D.2: rgda_conv2d (3 x 3, pad 1) + rgda_disc_bias_lrelu, stored after the LeakyReLU
//   z  [M][32]                the two heads stacked: cls1 in columns 0 .. nc-1, cls2 in nc .. 2nc-1, the rest dead (zero)
//
// The head is an implicit GEMM on v_mfma_f32_32x32x16_bf16 whose fragments are plain 16-byte loads (K is contiguous in
// both operands: the channels of one tap), as in adv_kernels.hip.  A tile is 32 pixels x 32 columns (the head forward
// splits its K over the four wavefronts of a workgroup, see there); the weights go in as the A operand, so a lane ends up with 16 of the 32 columns of ONE pixel (the other 16 sit in lane ^ 32) and the
// log-softmax over a pixel's columns is 16 registers and one half-wave exchange.  The data gradient takes the pixels as A
// (a lane then owns one output channel: coalesced 2-byte stores along the channels).
// Every reduction runs in a fixed order; nothing here uses floating-point atomics.
#include "feat_rows.h"

#define FADA_CP 32                       // columns of a head row: 2 nc <= 32
#define FADA_MAX_CLASSES 16
#define FADA_BYTES_MAX 0x7fffffffLL      // row buffers are addressed below 2^31 bytes

static inline bool fada_fits(long long rows, long long cols, long long elem) { return rows * cols * elem <= FADA_BYTES_MAX; }

// ---------------------------------------------------------------------------------------------- pack / unpack
// a 64-pixel x 64-channel tile through LDS: loads coalesced along the pixels of one channel, stores along the channels
// of one pixel.  grid (pixel tiles, channel tiles, images)
__global__ void __launch_bounds__(256) feat_pack_rows_kernel(const float* __restrict__ x, int hw, long long ldc, long long ldb,
                                                             int k, bf16_t* __restrict__ rows, int ld) {
    __shared__ bf16_t tile[64][66];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const float* xb = x + (size_t)b * ldb;
    if (p0 + tx < hw)
        for (int cc = ty; cc < 64; cc += 4)
            if (c0 + cc < k) tile[cc][tx] = f2bf(xb[(size_t)(c0 + cc) * ldc + p0 + tx]);
    __syncthreads();
    if (c0 + tx < k)
        for (int pp = ty; pp < 64; pp += 4)
            if (p0 + pp < hw) rows[((size_t)b * hw + p0 + pp) * ld + c0 + tx] = tile[tx][pp];
}

// dx[b][c][p] (+)= scale * rows[b * hw + p][c]
__global__ void __launch_bounds__(256) feat_unpack_rows_kernel(const bf16_t* __restrict__ rows, int ld, float* __restrict__ dx,
                                                               int hw, long long ldc, long long ldb, int k, float scale,
                                                               int accumulate) {
    __shared__ bf16_t tile[64][66];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    if (c0 + tx < k)
        for (int pp = ty; pp < 64; pp += 4)
            if (p0 + pp < hw) tile[tx][pp] = rows[((size_t)b * hw + p0 + pp) * ld + c0 + tx];
    __syncthreads();
    float* db = dx + (size_t)b * ldb;
    if (p0 + tx < hw)
        for (int cc = ty; cc < 64; cc += 4)
            if (c0 + cc < k) {
                float* dst = db + (size_t)(c0 + cc) * ldc + p0 + tx;
                const float v = __fmul_rn(scale, bf2f(tile[cc][tx]));      // two roundings, never a fused multiply-add
                *dst = accumulate ? __fadd_rn(*dst, v) : v;
            }
}

static int fada_pack_check(const void* x, const void* rows, int ld, int b, int hw, long long ldc, long long ldb, int k) {
    if (!x || !rows || b < 1 || hw < 1 || k < 1 || ld < 1) return RGDA_ERR_ARG;
    if (((uintptr_t)x & 3) || ((uintptr_t)rows & 15) || ld < k || !feat_view_ok(b, hw, ldc, ldb, k)) return RGDA_ERR_ARG;
    if ((ld & 7) || b > 65535 || cdiv(k, 64) > 65535 || !fada_fits((long long)b * hw, ld, 2)) return RGDA_ERR_UNSUPPORTED;
    return RGDA_OK;
}

extern "C" int rgda_feat_pack_rows(const float* x, int b, int hw, int64_t ldc, int64_t ldb, int k, void* rows, int ld,
                                   rgda_stream_t stream) {
    if (int rc = fada_pack_check(x, rows, ld, b, hw, ldc, ldb, k)) return rc;
    feat_pack_rows_kernel<<<dim3(cdiv(hw, 64), cdiv(k, 64), b), 256, 0, to_stream(stream)>>>(x, hw, ldc, ldb, k, (bf16_t*)rows, ld);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_feat_unpack_rows(const void* rows, int ld, float* dx, int b, int hw, int64_t ldc, int64_t ldb, int k,
                                     float scale, int accumulate, rgda_stream_t stream) {
    if (int rc = fada_pack_check(dx, rows, ld, b, hw, ldc, ldb, k)) return rc;
    if (!(scale == scale)) return RGDA_ERR_ARG;
    feat_unpack_rows_kernel<<<dim3(cdiv(hw, 64), cdiv(k, 64), b), 256, 0, to_stream(stream)>>>((const bf16_t*)rows, ld, dx, hw, ldc,
                                                                                             ldb, k, scale, accumulate);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

// ---------------------------------------------------------------------------------------------- the 3 x 3 / pad 1 tiles
static __device__ __forceinline__ bf16x8 fada_frag(const bf16_t* p, bool ok) {
    uint4 v = ok ? *(const uint4*)p : uint4{0u, 0u, 0u, 0u};
    return __builtin_bit_cast(bf16x8, v);
}

// pixel m of N x H x W -> (image, row, column), m clamped by the caller
struct FadaPix { int n, y, x; };
static __device__ __forceinline__ FadaPix fada_pix(int m, int H, int W) {
    FadaPix p;
    p.n = m / (H * W);
    const int rem = m - p.n * H * W;
    p.y = rem / W;
    p.x = rem - p.y * W;
    return p;
}

// Head forward.  z[m][j] = bias[j] + sum_{tap, c} a[src(m, tap)][c] * wgt[j][tap][c], src = (y - 1 + kh, x - 1 + kw); border
// taps load nothing and feed zeros.  A workgroup owns ONE tile of 32 pixels x 32 columns and its four wavefronts split K:
// wavefront w takes the (tap, 32-channel group) steps w, w + 4, ..., the four partial tiles meet in LDS and wavefront 0
// adds them in wavefront order (fixed) and runs the epilogue.  At 8 x 32 x 32 feature pixels that is 256 workgroups with
// a dependent chain of 9 Ch / 128 steps each, not 64 workgroups with 9 Ch / 32.
// Lane (r, hf) of a wavefront: pixel m0 + r, columns (e & 3) + 8 (e >> 2) + 4 hf, e < 16.  Inside a 32-channel group half
// hf, step s hold channels 16 hf + 8 s .. (the same permutation in both operands).
//   zout != NULL: z f32 [M][32] stored (the module path).
//   x2 != NULL:   soft labels a[k] = min(softmax_k(x2[m][:] / T), clip) in registers, log-softmax over the 2 nc live
//                 columns, part[workgroup] = sum over its pixels of -sum_k a[k] * logp[side * nc + k], and
//                 dz bf16 [M][32] = gscale * (S * softmax(z)_j - a'_j), dead columns zero (the step path).
__global__ void __launch_bounds__(256) fada_head_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ wgt,
                                                        const float* __restrict__ bias, int N, int H, int W, int Ch, int nc,
                                                        float* __restrict__ zout, const float* __restrict__ x2, int side,
                                                        float invT, float clip, float gscale, float* __restrict__ part,
                                                        bf16_t* __restrict__ dz) {
    __shared__ float partial[3][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hf = lane >> 5;
    const int M = N * H * W;
    const int m0 = blockIdx.x * 32;
    const int m = min(m0 + r, M - 1);
    const bool mine = m0 + r < M;
    const FadaPix px = fada_pix(m, H, W);
    const bf16_t* wp = wgt + (size_t)r * 9 * Ch + 16 * hf;
    const int groups = Ch >> 5, steps = 9 * groups;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll 2
    for (int it = wave; it < steps; it += 4) {
        const int tap = it / groups, c0 = (it - tap * groups) << 5;
        const int yy = px.y - 1 + tap / 3, xx = px.x - 1 + tap % 3;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const bf16_t* ap = a + (ok ? ((size_t)(px.n * H + yy) * W + xx) * Ch : (size_t)0) + 16 * hf + c0;
        const bf16_t* wq = wp + tap * Ch + c0;
        bf16x8 fa[2], fw[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            fa[s] = fada_frag(ap + 8 * s, ok);
            fw[s] = fada_frag(wq + 8 * s, true);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[s], fa[s], acc, 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) partial[wave - 1][e][lane] = acc[e];
    }
    __syncthreads();
    if (wave > 0) return;
    // accumulator element e of lane (r, hf): weight row (column of z) (e & 3) + 8 (e >> 2) + 4 hf, pixel r
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e)
        v[e] = (((acc[e] + partial[0][e][lane]) + partial[1][e][lane]) + partial[2][e][lane]) + bias[(e & 3) + 8 * (e >> 2) + 4 * hf];
    if (zout && mine) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *(float4*)(zout + (size_t)m * FADA_CP + 8 * g + 4 * hf) = float4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
    }
    if (!x2) return;
    const int live = 2 * nc, lo = side * nc;
    // log-softmax over the live columns: this lane's 16, then the other half-wave's
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if ((e & 3) + 8 * (e >> 2) + 4 * hf < live) mx = fmaxf(mx, v[e]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if ((e & 3) + 8 * (e >> 2) + 4 * hf < live) se += expf(v[e] - mx);
    se += __shfl_xor(se, 32, 64);
    const float lse = mx + logf(se), inv = 1.f / se;
    // the soft labels of this pixel: x2 f32 (N, nc, H, W); both half-waves form the same maximum, sum and S
    const size_t hw = (size_t)H * W;
    const float* xq = x2 + (size_t)px.n * nc * hw + ((size_t)px.y * W + px.x);
    float m2 = -INFINITY;
    for (int k = 0; k < nc; ++k) m2 = fmaxf(m2, xq[k * hw] * invT);
    float s2 = 0.f;
    for (int k = 0; k < nc; ++k) s2 += expf(xq[k * hw] * invT - m2);
    const float i2 = 1.f / s2;
    float S = 0.f;
    for (int k = 0; k < nc; ++k) S += fminf(expf(xq[k * hw] * invT - m2) * i2, clip);
    float g[16], lp = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int col = (e & 3) + 8 * (e >> 2) + 4 * hf, k = col - lo;
        float ak = 0.f;
        if (k >= 0 && k < nc) ak = fminf(expf(xq[k * hw] * invT - m2) * i2, clip);
        g[e] = col < live ? gscale * (S * expf(v[e] - mx) * inv - ak) : 0.f;
        if (k >= 0 && k < nc) lp -= ak * (v[e] - lse);
    }
    if (!mine) lp = 0.f;
    else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *(uint2*)(dz + (size_t)m * FADA_CP + 8 * q + 4 * hf) = uint2{pack2bf(g[4 * q], g[4 * q + 1]), pack2bf(g[4 * q + 2], g[4 * q + 3])};
    }
    lp = wave_sum(lp);
    if (lane == 0) part[blockIdx.x] = lp;
}

// Data gradient of a 3 x 3 / pad 1 layer with 32 output columns (the head; D.2 at ndf = 64 has the same geometry):
// da[m][ci] = mask * sum_{tap, co} dz[src(m, tap)][co] * wt[ci][tap][co],  src = (y + 1 - kh, x + 1 - kw),
// mask = below[m][ci] > 0 ? 1 : slope.  A wavefront owns 32 pixels x 32 FJ channels.
template <int FJ>
__global__ void __launch_bounds__(256) fada_head_bwd_data_kernel(const bf16_t* __restrict__ dz, const bf16_t* __restrict__ wt,
                                                                 const bf16_t* __restrict__ below, bf16_t* __restrict__ da, int N,
                                                                 int H, int W, int Ch, float slope) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hf = lane >> 5;
    const int M = N * H * W;
    const int m0 = (blockIdx.x * 4 + wave) * 32;
    if (m0 >= M) return;
    const int ci0 = blockIdx.y * 32 * FJ;
    const FadaPix px = fada_pix(min(m0 + r, M - 1), H, W);
    const bf16_t* wp[FJ];
#pragma unroll
    for (int j = 0; j < FJ; ++j) wp[j] = wt + (size_t)(ci0 + 32 * j + r) * 9 * FADA_CP + 16 * hf;
    f32x16 acc[FJ];
#pragma unroll
    for (int j = 0; j < FJ; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    for (int tap = 0; tap < 9; ++tap) {
        const int yy = px.y + 1 - tap / 3, xx = px.x + 1 - tap % 3;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const bf16_t* ap = dz + (ok ? ((size_t)(px.n * H + yy) * W + xx) * FADA_CP : (size_t)0) + 16 * hf;
        bf16x8 fa[2], fw[2][FJ];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            fa[s] = fada_frag(ap + 8 * s, ok);
#pragma unroll
            for (int j = 0; j < FJ; ++j) fw[s][j] = fada_frag(wp[j] + tap * FADA_CP + 8 * s, true);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < FJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s], fw[s][j], acc[j], 0, 0, 0);
    }
    // accumulator element e of lane l: pixel row (e & 3) + 8 (e >> 2) + 4 (l >> 5), channel column l & 31
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int m = m0 + (e & 3) + 8 * (e >> 2) + 4 * hf;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
            const size_t o = (size_t)m * Ch + ci0 + 32 * j + r;
            da[o] = f2bf(acc[j][e] * ((bf2f(below[o]) > 0.f) ? 1.f : slope));
        }
    }
}

static int fada_head_check(const void* a, const void* w, int N, int H, int W, int Ch) {
    if (!a || !w || N < 1 || H < 1 || W < 1 || Ch < 1) return RGDA_ERR_ARG;
    if (((uintptr_t)a & 15) || ((uintptr_t)w & 15)) return RGDA_ERR_ARG;
    const long long M = (long long)N * H * W;
    if ((Ch % 32) || !fada_fits(M, Ch, 2) || !fada_fits(M, FADA_CP, 4) || !fada_fits((long long)FADA_CP * 9, Ch, 2))
        return RGDA_ERR_UNSUPPORTED;
    return RGDA_OK;
}

extern "C" size_t rgda_fada_head_workspace(int64_t M) {
    if (M < 1 || M > 0x7fffffffLL) return 0;
    return a256((size_t)cdiv(M, 32) * 4);
}

extern "C" int rgda_fada_head(const void* a2, const void* wh, const float* bias, int N, int H, int W, int Ch, int nc, float* z,
                              const float* x2, int side, float T, float clip, float scale, float* loss, void* dz, void* ws,
                              size_t ws_bytes, rgda_stream_t stream) {
    if (int rc = fada_head_check(a2, wh, N, H, W, Ch)) return rc;
    if (!bias || ((uintptr_t)bias & 3) || ((uintptr_t)z & 15) || (!z && !x2)) return RGDA_ERR_ARG;
    if (x2) {
        if (!loss || !dz || !ws || ((uintptr_t)x2 & 3) || ((uintptr_t)dz & 15) || ((uintptr_t)ws & 3) || (side != 0 && side != 1) ||
            !(T > 0.f) || !(clip > 0.f) || !(scale == scale))
            return RGDA_ERR_ARG;
    }
    if (nc < 1 || nc > FADA_MAX_CLASSES) return RGDA_ERR_UNSUPPORTED;
    const long long M = (long long)N * H * W;
    if (x2 && ws_bytes < rgda_fada_head_workspace(M)) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    const int nb = cdiv(M, 32);
    fada_head_kernel<<<nb, 256, 0, st>>>((const bf16_t*)a2, (const bf16_t*)wh, bias, N, H, W, Ch, nc, z, x2, side,
                                         x2 ? 1.f / T : 0.f, clip, x2 ? scale / (float)M : 0.f, (float*)ws, (bf16_t*)dz);
    RGDA_CHECK_LAUNCH();
    if (x2) return rows_loss_sum((const float*)ws, nb, loss, scale / (float)M, st);
    return RGDA_OK;
}

extern "C" int rgda_fada_head_bwd_data(const void* dz, const void* wt, const void* below, void* da, int N, int H, int W, int Ch,
                                       float slope, rgda_stream_t stream) {
    if (int rc = fada_head_check(dz, wt, N, H, W, Ch)) return rc;
    if (!da || !below || ((uintptr_t)da & 15) || ((uintptr_t)below & 15) || !(slope == slope)) return RGDA_ERR_ARG;
    const long long M = (long long)N * H * W;
    hipStream_t st = to_stream(stream);
    const bool two = (Ch % 64) == 0;
    const dim3 grid(cdiv(M, 128), Ch / (two ? 64 : 32));
    if (grid.y > 65535) return RGDA_ERR_UNSUPPORTED;
    if (two) fada_head_bwd_data_kernel<2><<<grid, 256, 0, st>>>((const bf16_t*)dz, (const bf16_t*)wt, (const bf16_t*)below, (bf16_t*)da, N, H, W, Ch, slope);
    else fada_head_bwd_data_kernel<1><<<grid, 256, 0, st>>>((const bf16_t*)dz, (const bf16_t*)wt, (const bf16_t*)below, (bf16_t*)da, N, H, W, Ch, slope);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

// ---------------------------------------------------------------------------------------------- LeakyReLU mask pass
// g *= (a > 0 ? 1 : slope) in place on bf16 rows, eight values per thread: behind the generic data gradient of D.2
__global__ void __launch_bounds__(256) lrelu_mask_rows_kernel(bf16_t* __restrict__ g, const bf16_t* __restrict__ a, long long n8,
                                                              float slope) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const uint4 gv = ((const uint4*)g)[i], av = ((const uint4*)a)[i];
    unsigned u[4] = {gv.x, gv.y, gv.z, gv.w};
    const unsigned w[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float lo = __uint_as_float(u[e] << 16) * ((__uint_as_float(w[e] << 16) > 0.f) ? 1.f : slope);
        const float hi = __uint_as_float(u[e] & 0xffff0000u) * ((__uint_as_float(w[e] & 0xffff0000u) > 0.f) ? 1.f : slope);
        u[e] = pack2bf(lo, hi);
    }
    ((uint4*)g)[i] = uint4{u[0], u[1], u[2], u[3]};
}

extern "C" int rgda_lrelu_mask_rows(void* g, const void* a, int64_t M, int C, float slope, rgda_stream_t stream) {
    if (!g || !a || M < 1 || C < 1 || ((uintptr_t)g & 15) || ((uintptr_t)a & 15) || !(slope == slope)) return RGDA_ERR_ARG;
    if ((C % 8) || !fada_fits(M, C, 2)) return RGDA_ERR_UNSUPPORTED;
    const long long n8 = M * C / 8;
    lrelu_mask_rows_kernel<<<(unsigned)cdiv(n8, 256), 256, 0, to_stream(stream)>>>((bf16_t*)g, (const bf16_t*)a, n8, slope);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
