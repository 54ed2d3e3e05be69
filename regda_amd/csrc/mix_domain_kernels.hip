// Cross-domain mixing (regda/utils/classmix.py:17-53, regda/utils/cutmix.py:15-31): the pixels of a source batch that a
// predicate selects -- a set of source classes, or one box -- are pasted over the target batch in place, in one launch
// (include/rgda_hip.h: rgda_domain_mix).  A streaming pass: no LDS, no floating-point arithmetic, no atomics.
#include "common.h"

namespace {

constexpr int MIXD_THREADS = 256;
constexpr int MIXD_MAX_BLOCKS = 2048;           // 256 CUs x 8 workgroups; larger batches walk the quads grid-stride

typedef __attribute__((ext_vector_type(2))) long long i64x2;

// One thread owns a quad: four consecutive pixels of one row (fewer at a ragged row end).  Quad q of the N * H * QW quads
// is columns [4 * (q % QW), +4) of row q / QW.  `paste` is the 4-bit mask of its pasted pixels.
//   paste == 0     : nothing else is read or written.
//   paste == full, vec : every plane moves with one 16-byte load and store (the int64 planes with two stores).
//   otherwise      : pixel by pixel.
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
        const int y = (int)(row % H);
        const long long n = row / H;
        const int cnt = min(4, W - x);
        unsigned inside = (1u << cnt) - 1;                      // the pixels of the quad the predicate may select
        if (mode == RGDA_MIX_BOX) {
            if (y < y0 || y >= y1 || x + cnt <= x0 || x >= x1) continue;        // rows and quads outside the box read nothing
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < x0 || x + e >= x1) inside &= ~(1u << e);
        }
        const long long o = row * W + x;                        // pixel offset inside an [N][H][W] plane stack
        long long l[4] = {0, 0, 0, 0};
        if (vec) {
            const i64x2 a = reinterpret_cast<const i64x2*>(label_s + o)[0];
            const i64x2 b = reinterpret_cast<const i64x2*>(label_s + o)[1];
            l[0] = a.x; l[1] = a.y; l[2] = b.x; l[3] = b.y;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) l[e] = label_s[o + e];
        }
        unsigned paste = 0, bad = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in_range = l[e] >= 0 && l[e] < C;
            if (!in_range && l[e] != ignore_label) bad |= 1u << e;
            if (mode == RGDA_MIX_BOX || (in_range && ((class_bits >> (l[e] & 31)) & 1u))) paste |= 1u << e;
        }
        paste &= inside;
        if ((bad & inside) && flag) *flag = 1;                  // every writer stores 1
        if (!paste) continue;
        const long long oi = n * 3 * plane + (long long)y * W + x;
        const long long os = n * C * plane + (long long)y * W + x;
        if (vec && paste == 0xfu) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                *reinterpret_cast<f32x4*>(img_t + oi + ch * plane) = *reinterpret_cast<const f32x4*>(img_s + oi + ch * plane);
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
                if (!((paste >> e) & 1u)) continue;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) img_t[oi + ch * plane + e] = img_s[oi + ch * plane + e];
                if (label_t) label_t[o + e] = l[e];
                if (soft_t)
                    for (int c = 0; c < C; ++c) soft_t[os + c * plane + e] = l[e] == c ? 1.f : 0.f;
                if (regs_t) regs_t[o + e] = 0;
            }
        }
    }
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
