// IAST, instance-adaptive pseudo-labels (regda/utils/tools.py:323-373: ias_thresh and the loop body of generate_pseudo).
// Per batch the reference copies the probabilities to the host, builds one Python list of fp16 confidences per class,
// takes np.percentile of each and thresholds every pixel through apply_along_axis.  Here:
//   hist        per pixel the first maximum over the classes and its value -> arg (uint8), maxp (f32); maxp rounded to
//               fp16 (round to nearest even, what astype(np.float16) does) is counted in a per-class histogram over the
//               non-negative fp16 bit patterns 0 .. 0x7C00.  An fp16 has 31745 such values, so the histogram IS the
//               reference's list: nothing is lost.
//   percentile  one workgroup per class: np.percentile(method='linear') of [T_c] + the class's fp16 values in f64 from
//               two order statistics of the histogram with T_c merged in
//   label       arg + 1, 0 where (double)maxp < cls_thresh[arg].
// Integer atomics only: two runs give the same bits.
#include "common.h"

namespace {

constexpr int BINS = RGDA_IAST_BINS;
// A confident model puts most pixels of a class into the bin of 1.0.  Lanes of a wave with the same (class, bin) add
// once; bins from 0.5 (0x3800) to 1.0 (0x3C00) are counted in LDS per workgroup (16 classes: 65 600 B; the whole useful
// range [1/16, 1] would not fit) and flushed once, the others go to global memory directly (they are spread out).
constexpr int HOT_LO = 0x3800, HOT_HI = 0x3C00, HOT_N = HOT_HI - HOT_LO + 1;
constexpr int PEEL = 2;                  // wave leaders aggregated before the remaining lanes add one by one

static size_t align256_(size_t x) { return (x + 255) & ~(size_t)255; }

struct IastWs {
    int* hist;
    float* maxp;
    uint8_t* arg;
};
static IastWs carve(void* ws, int c, size_t npix) {
    char* base = (char*)ws;
    IastWs r;
    r.hist = (int*)base;
    base += align256_((size_t)c * BINS * 4);
    r.maxp = (float*)base;
    base += align256_(npix * 4);
    r.arg = (uint8_t*)base;
    return r;
}

__device__ __forceinline__ void hist_add(int* lh, int* __restrict__ hist, int key, int n) {
    const int cls = key >> 16, bits = key & 0xffff;
    if (bits >= HOT_LO && bits <= HOT_HI)
        atomicAdd(&lh[cls * HOT_N + bits - HOT_LO], n);
    else
        atomicAdd(&hist[cls * BINS + bits], n);
}

// A workgroup walks tiles of PIX x 256 pixels; a thread's PIX pixels are 256 apart, so every load of a wave is one 256 B
// run of one class plane and all PIX x C loads of a tile are in flight together.  Few, long-lived workgroups: every one
// of them flushes its non-zero LDS bins at the end, which on spread-out confidences costs more than the pixels' own adds.
constexpr int PIX = 4;
constexpr int HIST_BLOCKS = 512;
template <int C>
__global__ void __launch_bounds__(256) iast_hist_kernel(const float* __restrict__ probs, uint8_t* __restrict__ arg,
                                                        float* __restrict__ maxp, int* __restrict__ hist, int hw, int npix) {
    extern __shared__ int lh[];          // [C][HOT_N]
    for (int i = threadIdx.x; i < C * HOT_N; i += 256) lh[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int ntile = (int)(((long long)npix + PIX * 256 - 1) / (PIX * 256));
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        float v[PIX][C];
        long long at[PIX];
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            at[k] = (long long)tile * (PIX * 256) + k * 256 + threadIdx.x;
            if (at[k] < npix) {
                const int i = (int)at[k], img = i / hw;
                const float* p = probs + (size_t)img * C * hw + (i - img * hw);
#pragma unroll
                for (int c = 0; c < C; ++c) v[k][c] = p[(size_t)c * hw];
            }
        }
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            int key = -1;
            if (at[k] < npix) {
                float best = v[k][0];
                int a = 0;
#pragma unroll
                for (int c = 1; c < C; ++c)
                    if (v[k][c] > best) { best = v[k][c]; a = c; }      // the first maximum
                arg[at[k]] = (uint8_t)a;
                maxp[at[k]] = best;
                const int bits = __builtin_bit_cast(unsigned short, (_Float16)best);      // round to nearest even
                if (bits <= 0x7C00) key = (a << 16) | bits;             // (outside the contract: not counted)
            }
            for (int it = 0; it < PEEL; ++it) {
                const unsigned long long live = __ballot(key >= 0);
                if (!live) break;
                const int leader = __ffsll((long long)live) - 1;
                const int lk = __shfl(key, leader, 64);
                const unsigned long long same = __ballot(key == lk);
                if (lane == leader) hist_add(lh, hist, lk, __popcll(same));
                if (key == lk) key = -1;
            }
            if (key >= 0) hist_add(lh, hist, key, 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * HOT_N; i += 256) {
        const int v = lh[i];
        if (v) atomicAdd(&hist[(i / HOT_N) * BINS + HOT_LO + i % HOT_N], v);
    }
}

__device__ __forceinline__ double half_value(int bits) {
    return (double)__builtin_bit_cast(_Float16, (unsigned short)bits);
}

// np.percentile(arr, 100 q) (method 'linear') for arr = [T] + the class's fp16 values as f64, n = count + 1:
//   v = (n - 1) q, lo = floor(v), hi = min(lo + 1, n - 1), t = v - lo, a / b the lo-th / hi-th smallest,
//   a + (b - a) t, or b - (b - a) (1 - t) where t >= 0.5 (numpy's _lerp), every operation rounded on its own.
// Thread i owns CHUNK consecutive bins; a block scan of the chunk counts finds the thread that holds a rank.
constexpr int CHUNK = (BINS + 255) / 256;
__global__ void __launch_bounds__(256) iast_percentile_kernel(const int* __restrict__ hist, const double* __restrict__ prepend,
                                                              const double* __restrict__ q, float* __restrict__ out) {
    __shared__ int sc[256];
    __shared__ int s_below;
    __shared__ double s_val[2];
    const int cls = blockIdx.x, t = threadIdx.x;
    const int* h = hist + (size_t)cls * BINS;
    const double T = prepend[cls];
    if (t == 0) s_below = 0;
    __syncthreads();
    const int j0 = t * CHUNK, j1 = min(j0 + CHUNK, BINS);
    int s = 0, below = 0;                // below: the values < T (T goes in front of its equals; equal values are alike)
    for (int j = j0; j < j1; ++j) {
        const int v = h[j];
        s += v;
        below += (half_value(j) < T) ? v : 0;
    }
    if (below) atomicAdd(&s_below, below);
    sc[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = t >= off ? sc[t - off] : 0;
        __syncthreads();
        sc[t] += add;
        __syncthreads();
    }
    const int count = sc[255];
    if (count == 0) {                    // a class without pixels: the list holds T alone
        if (t == 0) out[cls] = (float)T;
        return;
    }
    const long long n = (long long)count + 1;
    const double v = __dmul_rn((double)(n - 1), q[cls]);
    long long lo = (long long)floor(v);
    lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
    const long long hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    const double frac = __dsub_rn(v, (double)lo);
    const int incl = sc[t], excl = incl - s, pos_T = s_below;
    for (int k = 0; k < 2; ++k) {
        const long long rank = k ? hi : lo;
        if (rank == pos_T) {
            if (t == 0) s_val[k] = T;
            continue;
        }
        const int r = (int)(rank < pos_T ? rank : rank - 1);       // rank among the histogram's values
        if (excl <= r && r < incl) {
            int seen = excl, j = j0;
            for (; j < j1 - 1; ++j) {
                if (seen + h[j] > r) break;
                seen += h[j];
            }
            s_val[k] = half_value(j);
        }
    }
    __syncthreads();
    if (t == 0) {
        const double a = s_val[0], b = s_val[1], d = __dsub_rn(b, a);
        const double r = frac >= 0.5 ? __dsub_rn(b, __dmul_rn(d, __dsub_rn(1.0, frac))) : __dadd_rn(a, __dmul_rn(d, frac));
        out[cls] = (float)r;
    }
}

__global__ void __launch_bounds__(256) iast_label_kernel(const uint8_t* __restrict__ arg, const float* __restrict__ maxp,
                                                         const double* __restrict__ cls_thresh, uint8_t* __restrict__ label,
                                                         int c, int npix) {
    __shared__ double thr[RGDA_MAX_CLASSES];
    if (threadIdx.x < c) thr[threadIdx.x] = cls_thresh[threadIdx.x];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
        const int a = min((int)arg[i], c - 1);       // (arg comes from rgda_iast_hist: always below c)
        label[i] = ((double)maxp[i] < thr[a]) ? (uint8_t)0 : (uint8_t)(a + 1);
    }
}

static int shape_status(int n, int c, int H, int W) {
    if (n <= 0 || H <= 0 || W <= 0) return RGDA_ERR_ARG;
    if ((long long)n * H * W >= (1ll << 31)) return RGDA_ERR_ARG;       // pixel index and counts: 32 bits
    if (!class_count_ok(c)) return RGDA_ERR_UNSUPPORTED;
    return RGDA_OK;
}

}  // namespace

extern "C" size_t rgda_iast_workspace(int n, int c, int H, int W) {
    if (shape_status(n, c, H, W) != RGDA_OK) return 0;
    const size_t npix = (size_t)n * H * W;
    return align256_((size_t)c * BINS * 4) + align256_(npix * 4) + align256_(npix);
}

extern "C" int rgda_iast_hist(const float* probs, int n, int c, int H, int W, void* ws, size_t ws_bytes,
                              rgda_stream_t stream) {
    if (!probs || !ws) return RGDA_ERR_ARG;
    if (int st = shape_status(n, c, H, W)) return st;
    if (ws_bytes < rgda_iast_workspace(n, c, H, W)) return RGDA_ERR_WORKSPACE;
    const int npix = n * H * W;
    const IastWs a = carve(ws, c, (size_t)npix);
    if (zero_bytes(a.hist, (size_t)c * BINS * 4, stream) != RGDA_OK) return RGDA_ERR_LAUNCH;
    const int blocks = min(cdiv(npix, PIX * 256), HIST_BLOCKS);
    return with_classes(c, [&](auto cc) -> int {
        constexpr int C = decltype(cc)::value;
        const size_t lds = (size_t)C * HOT_N * 4;
        if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)iast_hist_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)lds) != hipSuccess)
            return RGDA_ERR_LAUNCH;
        iast_hist_kernel<C><<<blocks, 256, lds, to_stream(stream)>>>(probs, a.arg, a.maxp, a.hist, H * W, npix);
        RGDA_CHECK_LAUNCH();
        return RGDA_OK;
    });
}

extern "C" int rgda_iast_percentile(const double* prepend, const double* q, float* out, int c, const void* ws,
                                    size_t ws_bytes, rgda_stream_t stream) {
    if (!prepend || !q || !out || !ws) return RGDA_ERR_ARG;
    if (!class_count_ok(c)) return RGDA_ERR_UNSUPPORTED;
    if (ws_bytes < (size_t)c * BINS * 4) return RGDA_ERR_WORKSPACE;
    iast_percentile_kernel<<<c, 256, 0, to_stream(stream)>>>((const int*)ws, prepend, q, out);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_iast_label(const double* cls_thresh, uint8_t* label, int n, int c, int H, int W, const void* ws,
                               size_t ws_bytes, rgda_stream_t stream) {
    if (!cls_thresh || !label || !ws) return RGDA_ERR_ARG;
    if (int st = shape_status(n, c, H, W)) return st;
    if (ws_bytes < rgda_iast_workspace(n, c, H, W)) return RGDA_ERR_WORKSPACE;
    const int npix = n * H * W;
    const IastWs a = carve(const_cast<void*>(ws), c, (size_t)npix);
    iast_label_kernel<<<min(cdiv(npix, 256 * 4), 2048), 256, 0, to_stream(stream)>>>(a.arg, a.maxp, cls_thresh, label, c, npix);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
