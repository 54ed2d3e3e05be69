// What the losses on the instance-normalised feature map share (coral, mmd, whiten, contrast, triplet kernels): the
// strided view of the f32 NCHW map, the 64 x 64 staging tile to the two bf16 images, the fixed-order block and loss sums,
// and the store of weight * dL/dfeat into the pixel-major bf16 gradient rows.  Every routine here is the arithmetic the
// kernels had each on their own, operand for operand: none of them is told which loss calls it.
#pragma once
#include "common.h"
#include "gram_tile.h"

static inline size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- the feature map, read in place: row g = image g / hw, pixel g % hw; the pixels of one image are contiguous
struct FeatView {
    const float* x;
    long long ldc, ldb;          // channel and image strides (elements)
    int hw, n;                   // pixels per image, rows
};
static __device__ __forceinline__ const float* feat_row(const FeatView& f, int g) {      // channel 0 of row g
    const int b = g / f.hw, p = g - b * f.hw;
    return f.x + (size_t)b * f.ldb + p;
}
static __device__ __forceinline__ float feat_at(const FeatView& f, int g, int c) { return feat_row(f, g)[(size_t)c * f.ldc]; }
// the strides an entry point accepts for b images of hw pixels and d channels
static inline bool feat_view_ok(int b, int hw, long long ldc, long long ldb, int d) {
    return ldc >= hw && (b <= 1 || ldb >= ldc * d);
}

// ---- the gradient rows: rows row0 .. row0 + n of the staged order go to out[0 .. n), pixel-major bf16, ld elements apart
struct GradRows {
    bf16_t* out;
    int row0, n, ld;
};
// absent, or d channels wide in whole 16-byte vectors and aligned to `align` bytes
static inline bool grad_rows_ok(const void* p, int ld, int d, int align) {
    return !p || (ld >= d && !(ld & 7) && !((uintptr_t)p & (uintptr_t)(align - 1)));
}

struct F4 {
    float v0, v1, v2, v3;
};
// four consecutive channels of one gradient row, one 8-byte store; accumulate: the old bf16 values join the fp32 ones
// before the one rounding
static __device__ __forceinline__ void store4_bf16(bf16_t* dst4, float v0, float v1, float v2, float v3, int accumulate) {
    uint2* dst = (uint2*)dst4;
    if (accumulate) {
        const uint2 o = *dst;
        v0 += __uint_as_float(o.x << 16);
        v1 += __uint_as_float(o.x & 0xffff0000u);
        v2 += __uint_as_float(o.y << 16);
        v3 += __uint_as_float(o.y & 0xffff0000u);
    }
    *dst = uint2{pack2bf(v0, v1), pack2bf(v2, v3)};
}

// ---- sums in a fixed order.  Workgroup of 256: a butterfly per wavefront, then (w0 + w1) + (w2 + w3); every thread
// gets the sum.  `red` is read until the next barrier.
static __device__ __forceinline__ float block_sum4(float s, float* red) {
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// channel c over the rows of a view: this thread's strided partial of a workgroup of 256, for block_sum4 (left to the
// caller, so that a kernel with several sums reads for all of them before its first barrier)
static __device__ __forceinline__ float feat_channel_partial(const FeatView& f, int c) {
    float s = 0.f;
    for (int g = threadIdx.x; g < f.n; g += 256) s += feat_at(f, g, c);
    return s;
}
// feat_rows.hip: loss[0] += scale * sum(part[0 .. n)), one workgroup; out[r] = the sum of squares of bf16 row r of
// x [rows][d], one wavefront per row.  Both return RGDA_OK or RGDA_ERR_LAUNCH.  Internal to the library: not exported.
__attribute__((visibility("hidden"))) int rows_loss_sum(const float* part, int n, float* loss, float scale, hipStream_t st);
__attribute__((visibility("hidden"))) int rows_sumsq(const bf16_t* x, int rows, int d, float* out, hipStream_t st);

// ---- the staging tile: 64 rows x the 64 channels from c0 of a workgroup of 256.  rowf(r) is the row of the view that
// tile row r < nrows stages, or negative: a padding row, staged as zeros; tile rows from nrows on are not touched.
// bf16(x - mu[c]) (bf16(x) without mu) goes to the channel-major image ct[c][col0 + r] (coalesced along the rows) and,
// through LDS, to the pixel-major image xp[col0 + r][c] (coalesced along the channels; skipped when xp == nullptr).
template <class RowF>
static __device__ __forceinline__ void stage_tile64(const FeatView& f, RowF rowf, int nrows, const float* mu, int c0, int d,
                                                    bf16_t* ct, int ldct, int col0, bf16_t* xp) {
    __shared__ bf16_t tile[64][66];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    if (tx < nrows) {
        const int g = rowf(tx);
        const float* src = feat_row(f, max(g, 0));
        for (int cc = ty; cc < 64; cc += 4) {
            const int c = c0 + cc;
            if (c < d) {
                bf16_t v = 0;
                if (g >= 0) v = mu ? f2bf(src[(size_t)c * f.ldc] - mu[c]) : f2bf(src[(size_t)c * f.ldc]);
                ct[(size_t)c * ldct + (col0 + tx)] = v;
                tile[tx][cc] = v;
            }
        }
    }
    if (!xp) return;
    __syncthreads();
    for (int gg = ty; gg < 64; gg += 4) {
        const int c = c0 + tx;
        if (gg < nrows && c < d) xp[(size_t)(col0 + gg) * d + c] = tile[gg][tx];
    }
}

// ---- the epilogue of a 128 x 64 gradient tile (tile_nt<2>: channels mt * CT .., tile columns nt * GN ..): a lane's
// registers 4q .. 4q+3 are four consecutive channels c of one column p -> store4_bf16 into rowf(p) + c, for p < n and
// c < d.  colf(p) is asked once per column and gives that column's functor (the four accumulators, c) -> the four values,
// so what a column needs once (its row of another table) is loaded once.  Columns past n - 1 are clamped for both.
template <class RowF, class ColF>
static __device__ __forceinline__ void grad_tile_store(const f32x16 (&acc)[4][2], int mt, int nt, int n, int d, int accumulate,
                                                       RowF rowf, ColF colf) {
    const int lane = threadIdx.x & 63, h = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = nt * GN + 32 * j + (lane & 31);
        const int pc = min(p, n - 1);
        bf16_t* orow = rowf(pc);
        const auto valf = colf(pc);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = mt * CT + 32 * i + 8 * q + 4 * h;
                if (p < n && c < d) {
                    const F4 v = valf(F4{acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]}, c);
                    store4_bf16(orow + c, v.v0, v.v1, v.v2, v.v3, accumulate);
                }
            }
    }
}
