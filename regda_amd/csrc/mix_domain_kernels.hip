// Cross-domain mixing (regda/utils/classmix.py:17-53, regda/utils/cutmix.py:15-31): the pixels of a source batch that a
// predicate selects -- a set of source classes, or one box -- are pasted over the target batch in place, in one launch
// (include/rgda_hip.h: rgda_domain_mix).  A streaming pass: no LDS, no floating-point arithmetic, no atomics.
// rgda_domain_mix_table is the same pass with every image's predicate read from a device table and the image written out
// of place (the mix inside a training step); rgda_mix_select_classes fills that table's class sets from the source labels
// (the DACS draw: integer ORs only) and rgda_mix_write_table carries the host's draw to the device in its arguments.
#include "common.h"

#include <string.h>

namespace {

constexpr int MIXD_THREADS = 256;
constexpr int MIXD_MAX_BLOCKS = 2048;           // 256 CUs x 8 workgroups; larger batches walk the quads grid-stride

typedef __attribute__((ext_vector_type(2))) long long i64x2;

// One thread owns a quad: four consecutive pixels of one row (fewer at a ragged row end): columns [x, x + cnt) of row y of
// image n, `row` = n * H + y.  `paste` is the 4-bit mask of its pasted pixels.
//   paste == 0     : nothing else is read or written.
//   paste == full, vec : every plane moves with one 16-byte load and store (the int64 planes with two stores).
//   otherwise      : pixel by pixel.
// OUT_OF_PLACE (rgda_domain_mix_table): the image goes img_in -> img_out with every pixel written (both may be null: no
// image work), and a predicate that can select nothing in the quad reads no label; otherwise img_out is the target image,
// pasted in place, and img_in is not read.  ONE routine for both entry points: the predicate, the routes, the pasted values
// and the flag cannot drift apart.
template <bool OUT_OF_PLACE>
__device__ __forceinline__ void mix_quad(const float* __restrict__ img_s, const int64_t* __restrict__ label_s,
                                         const float* img_in, float* img_out, int64_t* __restrict__ label_t,
                                         float* __restrict__ soft_t, int64_t* __restrict__ regs_t, long long n, long long row,
                                         int y, int x, int cnt, int C, long long plane, int W, int mode, uint32_t class_bits,
                                         int y0, int y1, int x0, int x1, int ignore_label, int* __restrict__ flag, int vec) {
    unsigned inside = (1u << cnt) - 1;                          // the pixels of the quad the predicate may select
    bool live = true;
    if (mode == RGDA_MIX_BOX) {
        if (y < y0 || y >= y1 || x + cnt <= x0 || x >= x1) {    // rows and quads outside the box read nothing
            live = false;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < x0 || x + e >= x1) inside &= ~(1u << e);
        }
    } else if (OUT_OF_PLACE && !class_bits) {
        live = false;                                           // an empty class set: rgda_domain_mix does not launch
    }
    const bool image = !OUT_OF_PLACE || img_out != nullptr;
    const long long o = row * W + x;                            // pixel offset inside an [N][H][W] plane stack
    const long long oi = n * 3 * plane + (long long)y * W + x;
    long long l[4] = {0, 0, 0, 0};
    unsigned paste = 0;
    if (live) {
        if (vec) {
            const i64x2 a = reinterpret_cast<const i64x2*>(label_s + o)[0];
            const i64x2 b = reinterpret_cast<const i64x2*>(label_s + o)[1];
            l[0] = a.x; l[1] = a.y; l[2] = b.x; l[3] = b.y;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) l[e] = label_s[o + e];
        }
        unsigned bad = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in_range = l[e] >= 0 && l[e] < C;
            if (!in_range && l[e] != ignore_label) bad |= 1u << e;
            if (mode == RGDA_MIX_BOX || (in_range && ((class_bits >> (l[e] & 31)) & 1u))) paste |= 1u << e;
        }
        paste &= inside;
        if ((bad & inside) && flag) *flag = 1;                  // every writer stores 1
    }
    if (!paste) {
        if (OUT_OF_PLACE && image) {                            // the quad is the clean tile's
            if (vec) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    *reinterpret_cast<f32x4*>(img_out + oi + ch * plane) = *reinterpret_cast<const f32x4*>(img_in + oi + ch * plane);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < cnt)
                        for (int ch = 0; ch < 3; ++ch) img_out[oi + ch * plane + e] = img_in[oi + ch * plane + e];
            }
        }
        return;
    }
    const long long os = n * C * plane + (long long)y * W + x;
    if (vec && paste == 0xfu) {
        if (image) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                *reinterpret_cast<f32x4*>(img_out + oi + ch * plane) = *reinterpret_cast<const f32x4*>(img_s + oi + ch * plane);
        }
        if (label_t) {
            reinterpret_cast<i64x2*>(label_t + o)[0] = i64x2{l[0], l[1]};
            reinterpret_cast<i64x2*>(label_t + o)[1] = i64x2{l[2], l[3]};
        }
        if (soft_t)
            for (int c = 0; c < C; ++c)
                *reinterpret_cast<f32x4*>(soft_t + os + c * plane) =
                    f32x4{l[0] == c ? 1.f : 0.f, l[1] == c ? 1.f : 0.f, l[2] == c ? 1.f : 0.f, l[3] == c ? 1.f : 0.f};
        if (regs_t) {
            reinterpret_cast<i64x2*>(regs_t + o)[0] = i64x2{0, 0};
            reinterpret_cast<i64x2*>(regs_t + o)[1] = i64x2{0, 0};
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!((paste >> e) & 1u)) {
                if (OUT_OF_PLACE && image && e < cnt)
                    for (int ch = 0; ch < 3; ++ch) img_out[oi + ch * plane + e] = img_in[oi + ch * plane + e];
                continue;
            }
            if (image) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) img_out[oi + ch * plane + e] = img_s[oi + ch * plane + e];
            }
            if (label_t) label_t[o + e] = l[e];
            if (soft_t)
                for (int c = 0; c < C; ++c) soft_t[os + c * plane + e] = l[e] == c ? 1.f : 0.f;
            if (regs_t) regs_t[o + e] = 0;
        }
    }
}

// Quad q of the N * H * QW quads is columns [4 * (q % QW), +4) of row q / QW.
__global__ void __launch_bounds__(MIXD_THREADS) domain_mix_kernel(
    const float* __restrict__ img_s, const int64_t* __restrict__ label_s, float* __restrict__ img_t,
    int64_t* __restrict__ label_t, float* __restrict__ soft_t, int64_t* __restrict__ regs_t, long long quads, int QW, int C,
    int H, int W, int mode, uint32_t class_bits, int y0, int y1, int x0, int x1, int ignore_label, int* __restrict__ flag,
    int vec) {
    const long long plane = (long long)H * W;
    for (long long q = (long long)blockIdx.x * MIXD_THREADS + threadIdx.x; q < quads;
         q += (long long)gridDim.x * MIXD_THREADS) {
        const long long row = q / QW;
        const int x = (int)(q - row * QW) * 4;
        mix_quad<false>(img_s, label_s, nullptr, img_t, label_t, soft_t, regs_t, row / H, row, (int)(row % H), x, min(4, W - x),
                        C, plane, W, mode, class_bits, y0, y1, x0, x1, ignore_label, flag, vec);
    }
}

// The same walk with image n's predicate from row n of the table (five words, the same for every thread of a row).
__global__ void __launch_bounds__(MIXD_THREADS) domain_mix_table_kernel(
    const float* __restrict__ img_s, const int64_t* __restrict__ label_s, const float* img_in, float* img_out,
    int64_t* __restrict__ label_t, float* __restrict__ soft_t, const int32_t* __restrict__ table, long long quads, int QW,
    int C, int H, int W, int mode, int ignore_label, int* __restrict__ flag, int vec) {
    const long long plane = (long long)H * W;
    for (long long q = (long long)blockIdx.x * MIXD_THREADS + threadIdx.x; q < quads;
         q += (long long)gridDim.x * MIXD_THREADS) {
        const long long row = q / QW;
        const int x = (int)(q - row * QW) * 4;
        const long long n = row / H;
        const int32_t* t = table + n * RGDA_MIX_TABLE_COLS;
        mix_quad<true>(img_s, label_s, img_in, img_out, label_t, soft_t, nullptr, n, row, (int)(row % H), x, min(4, W - x), C,
                       plane, W, mode, (uint32_t)t[0], t[1], t[2], t[3], t[4], ignore_label, flag, vec);
    }
}

// ---- rgda_mix_select_classes
constexpr int SEL_THREADS = 256;
constexpr int SEL_PAIRS = 8;                    // 16-byte loads of one thread: 2048 pairs = 32 KB of labels per workgroup
constexpr int SEL_MAX_BPI = 256;                // workgroups per image at most; larger tiles walk block-stride

__global__ void __launch_bounds__(64) mix_clear_kernel(uint32_t* __restrict__ ws, int n) {
    for (int i = threadIdx.x; i < n; i += 64) ws[i] = 0;
}

static __device__ __forceinline__ uint32_t label_bit(long long l, int C, int ignore_label, int* __restrict__ flag) {
    if (l >= 0 && l < C) return 1u << (int)l;
    if (l != ignore_label && flag) *flag = 1;                   // every writer stores 1
    return 0;
}

// grid (workgroups per image, N): the classes that occur in this workgroup's share of image n, ORed per thread, per
// wave (shuffles), per workgroup (LDS), then ONE atomic OR into the image's word
__global__ void __launch_bounds__(SEL_THREADS) mix_presence_kernel(const int64_t* __restrict__ label_s, uint32_t* __restrict__ ws,
                                                                   long long HW, int C, int ignore_label,
                                                                   int* __restrict__ flag, int vec) {
    __shared__ uint32_t part[SEL_THREADS / 64];
    const int n = blockIdx.y;
    const int64_t* lab = label_s + (long long)n * HW;
    const long long stride = (long long)gridDim.x * SEL_THREADS;
    uint32_t bits = 0;
    if (vec) {
        const long long pairs = HW / 2;                         // HW is even on this route
        for (long long i = (long long)blockIdx.x * SEL_THREADS + threadIdx.x; i < pairs; i += stride) {
            const i64x2 v = reinterpret_cast<const i64x2*>(lab)[i];
            bits |= label_bit(v.x, C, ignore_label, flag) | label_bit(v.y, C, ignore_label, flag);
        }
    } else {
        for (long long i = (long long)blockIdx.x * SEL_THREADS + threadIdx.x; i < HW; i += stride)
            bits |= label_bit(lab[i], C, ignore_label, flag);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
#pragma unroll
        for (int w = 0; w < SEL_THREADS / 64; ++w) all |= part[w];
        if (all) atomicOr(ws + n, all);
    }
}

// one wave per image, lane c = class c: selected iff present and fewer than (P + 1) / 2 present classes come before it
// in (rank, class id) order
__global__ void __launch_bounds__(64) mix_choice_kernel(const uint8_t* __restrict__ ranks, const uint32_t* __restrict__ ws,
                                                        int32_t* __restrict__ table, int C) {
    const int n = blockIdx.x, c = threadIdx.x;
    const uint32_t present = ws[n];                             // only bits below C were ever set
    const int k = (__popc(present) + 1) / 2;
    bool sel = false;
    if (c < C && ((present >> c) & 1u)) {
        const int r = ranks[n * C + c];
        int before = 0;
        for (int d = 0; d < C; ++d) {
            const int rd = ranks[n * C + d];
            if (((present >> d) & 1u) && (rd < r || (rd == r && d < c))) ++before;
        }
        sel = r < C && before < k;
    }
    const unsigned long long m = __ballot(sel);
    if (c == 0) table[(long long)n * RGDA_MIX_TABLE_COLS] = (int32_t)(uint32_t)m;
}

// ---- rgda_mix_write_table: the draw travels in the launch's own argument block
struct MixDraw {
    uint32_t ranks[RGDA_MIX_WRITE_MAX_IMAGES * 32 / 4];         // N * C bytes, C <= 32
};
__global__ void __launch_bounds__(256) mix_write_table_kernel(int32_t* __restrict__ table, uint8_t* __restrict__ ranks, MixDraw d,
                                                              int N, int C, uint32_t class_bits, int y0, int y1, int x0,
                                                              int x1) {
    for (int i = threadIdx.x; i < N * RGDA_MIX_TABLE_COLS; i += 256) {
        const int col = i % RGDA_MIX_TABLE_COLS;
        table[i] = col == 0 ? (int32_t)class_bits : col == 1 ? y0 : col == 2 ? y1 : col == 3 ? x0 : col == 4 ? x1 : 0;
    }
    if (ranks)
        for (int i = threadIdx.x; i < N * C; i += 256) ranks[i] = (uint8_t)(d.ranks[i >> 2] >> (8 * (i & 3)));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int rgda_domain_mix(const float* img_s, const int64_t* label_s, float* img_t, int64_t* label_t, float* soft_t,
                               int64_t* regs_t, int N, int C, int H, int W, int mode, uint32_t class_bits, int y0, int y1,
                               int x0, int x1, int ignore_label, int* flag, rgda_stream_t stream) {
    if (!img_s || !label_s || !img_t || N < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    if (C < 1 || C > 32) return RGDA_ERR_ARG;                   // one bit of class_bits per class
    if (mode == RGDA_MIX_CLASS) {
        if (C < 32 && (class_bits >> C)) return RGDA_ERR_ARG;
        if (!class_bits) return RGDA_OK;                        // an empty class set pastes nothing
    } else if (mode == RGDA_MIX_BOX) {
        if (y0 < 0 || y0 > y1 || y1 > H || x0 < 0 || x0 > x1 || x1 > W) return RGDA_ERR_ARG;
        if (y0 == y1 || x0 == x1) return RGDA_OK;               // an empty box pastes nothing
    } else {
        return RGDA_ERR_ARG;
    }
    const bool vec = W % 4 == 0 && aligned16(img_s) && aligned16(label_s) && aligned16(img_t) &&
                     (!label_t || aligned16(label_t)) && (!soft_t || aligned16(soft_t)) && (!regs_t || aligned16(regs_t));
    const int QW = (W + 3) / 4;
    const long long quads = (long long)N * H * QW;
    const long long want = (quads + MIXD_THREADS - 1) / MIXD_THREADS;
    const int blocks = want < MIXD_MAX_BLOCKS ? (int)want : MIXD_MAX_BLOCKS;
    domain_mix_kernel<<<blocks, MIXD_THREADS, 0, to_stream(stream)>>>(img_s, label_s, img_t, label_t, soft_t, regs_t, quads,
                                                                      QW, C, H, W, mode, class_bits, y0, y1, x0, x1,
                                                                      ignore_label, flag, vec ? 1 : 0);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_domain_mix_table(const float* img_s, const int64_t* label_s, const float* img_in, float* img_out,
                                     int64_t* label_t, float* soft_t, const int32_t* table, int N, int C, int H, int W,
                                     int mode, int ignore_label, int* flag, rgda_stream_t stream) {
    if (!img_s || !label_s || !table || !aligned16(table) || N < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    if (C < 1 || C > 32) return RGDA_ERR_ARG;                   // one bit of class_bits per class
    if (mode != RGDA_MIX_CLASS && mode != RGDA_MIX_BOX) return RGDA_ERR_ARG;
    if ((img_in == nullptr) != (img_out == nullptr)) return RGDA_ERR_ARG;
    if (!img_out && !label_t && !soft_t) return RGDA_OK;        // nothing to write
    const bool vec = W % 4 == 0 && aligned16(img_s) && aligned16(label_s) && (!img_in || aligned16(img_in)) &&
                     (!img_out || aligned16(img_out)) && (!label_t || aligned16(label_t)) && (!soft_t || aligned16(soft_t));
    const int QW = (W + 3) / 4;
    const long long quads = (long long)N * H * QW;
    const long long want = (quads + MIXD_THREADS - 1) / MIXD_THREADS;
    const int blocks = want < MIXD_MAX_BLOCKS ? (int)want : MIXD_MAX_BLOCKS;
    domain_mix_table_kernel<<<blocks, MIXD_THREADS, 0, to_stream(stream)>>>(img_s, label_s, img_in, img_out, label_t, soft_t,
                                                                            table, quads, QW, C, H, W, mode, ignore_label,
                                                                            flag, vec ? 1 : 0);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_mix_select_classes(const int64_t* label_s, const uint8_t* ranks, int32_t* table, uint32_t* ws, int N,
                                       int C, int H, int W, int ignore_label, int* flag, rgda_stream_t stream) {
    if (!label_s || !ranks || !ws || ((uintptr_t)ws & 3) || !table || !aligned16(table)) return RGDA_ERR_ARG;
    if (N < 1 || N > 65535 || H < 1 || W < 1 || C < 1 || C > 32) return RGDA_ERR_ARG;   // N is the grid's y extent
    const long long HW = (long long)H * W;
    const bool vec = HW % 2 == 0 && aligned16(label_s);         // then every image starts on a 16-byte boundary
    const long long per_block = (long long)SEL_THREADS * SEL_PAIRS * 2;
    const long long want = (HW + per_block - 1) / per_block;
    const int bpi = want < SEL_MAX_BPI ? (int)want : SEL_MAX_BPI;
    mix_clear_kernel<<<1, 64, 0, to_stream(stream)>>>(ws, N);
    RGDA_CHECK_LAUNCH();
    mix_presence_kernel<<<dim3(bpi, N), SEL_THREADS, 0, to_stream(stream)>>>(label_s, ws, HW, C, ignore_label, flag, vec ? 1 : 0);
    RGDA_CHECK_LAUNCH();
    mix_choice_kernel<<<N, 64, 0, to_stream(stream)>>>(ranks, ws, table, C);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_mix_write_table(int32_t* table, uint8_t* ranks, const uint8_t* ranks_host, int N, int C,
                                    uint32_t class_bits, int y0, int y1, int x0, int x1, rgda_stream_t stream) {
    if (!table || !aligned16(table) || N < 1 || C < 1 || C > 32) return RGDA_ERR_ARG;
    if (C < 32 && (class_bits >> C)) return RGDA_ERR_ARG;
    if (y0 < 0 || y0 > y1 || x0 < 0 || x0 > x1) return RGDA_ERR_ARG;
    if ((ranks == nullptr) != (ranks_host == nullptr)) return RGDA_ERR_ARG;
    if (N > RGDA_MIX_WRITE_MAX_IMAGES) return RGDA_ERR_UNSUPPORTED;
    MixDraw d = {};
    if (ranks_host) memcpy(d.ranks, ranks_host, (size_t)N * C);
    mix_write_table_kernel<<<1, 256, 0, to_stream(stream)>>>(table, ranks, d, N, C, class_bits, y0, y1, x0, x1);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
