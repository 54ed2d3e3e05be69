// Pseudo-label analysis (regda/gast/pseudo_generation.py:158-235: analysis_pseudo_labels and range_static).
// Per image the reference makes 100 passes over the (C, H, W) soft label, one per entropy bin, each with full-size
// temporaries and two host syncs.  Here:
//   analysis  one pass: per pixel the pseudo_selection decision, the entropy (fp64, rounded once), the difficulty
//             1 - p[gt], the bin(s) of the entropy -> per-image integer tables, counted in LDS per workgroup and flushed
//             once with integer atomics.  The difficulty is a multiple of 2^-24, so its sum is an exact integer too.
//   fold      one workgroup: the per-image quotients of the reference's loop (:195-207) in fp64, image after image,
//             added to a running state on the device.
// Integer atomics only, a fixed image order: two runs give the same bits.  Layouts: include/rgda_hip.h.
#include "common.h"

// the maximum pass of pseudo_selection (label_kernels.hip): per-image per-class maxima, flag bit 0 on a value outside [0, 1]
__global__ void pseudo_max_kernel(const float* __restrict__ soft, float* classmax, int* flag, int hw, int chunk);

namespace {

constexpr int RMAX = RGDA_ANALYSIS_MAX_BINS;
constexpr int PIX = 4, TILE = PIX * 256;      // pixels of a thread and of a workgroup per step
// Workgroups of a launch: one per step up to MAX_WG, shared among the images.  The pass is bound by the fp64 logarithms,
// not by the read, so it wants several waves per SIMD; every workgroup also flushes its non-zero LDS entries.  One sweep
// of a tuning build (RGDA_ANALYSIS_WG), one whole update at 1 x C x 1024 x 1024 with entropies spread over the bins, at
// 128 / 256 / 512 / 1024 workgroups: 93 / 63 / 53 / 59 us at 6 classes, 175 / 112 / 100 / 93 us at 16.
constexpr int MAX_WG = 512;
constexpr int MAX_CHUNK = 16384;              // pixels of one workgroup of the maximum pass

struct Tables {       // one image's tables, in int64 elements
    int rows, used, hit, inbin, diff24, len;
};
static __host__ __device__ inline Tables tables_of(int c, int R) {
    Tables t;
    t.rows = R + 1;
    t.used = 0;
    t.hit = t.rows * c;
    t.inbin = 2 * t.rows * c;
    t.diff24 = t.inbin + t.rows;
    t.len = t.diff24 + t.rows;
    return t;
}

struct Lds {
    unsigned* used;
    unsigned* hit;
    unsigned* inbin;
    unsigned long long* diff24;
    const float* lo;
    const float* hi;
};

// the largest i with lo[i] <= e (0 where there is none): lo is sorted
__device__ __forceinline__ int bin_candidate(const float* lo, int R, float e) {
    int a = 0, n = R;
    while (n > 1) {
        const int half = n >> 1;
        if (lo[a + half] <= e) { a += half; n -= half; } else n = half;
    }
    return a;
}

template <int C>
__device__ __forceinline__ void count_row(const Lds& s, int row, int pseudo, bool hit, unsigned d24) {
    atomicAdd(&s.inbin[row], 1u);
    if (d24) atomicAdd(&s.diff24[row], (unsigned long long)d24);
    if (pseudo >= 0) {
        atomicAdd(&s.used[row * C + pseudo], 1u);
        if (hit) atomicAdd(&s.hit[row * C + pseudo], 1u);
    }
}

struct Pixel {
    float entropy;
    unsigned d24;       // difficulty * 2^24
    int pseudo;         // the selected class, -1: none
    int flags;
    bool hit;
};

// one pixel's measures from p[0..C) and its ground truth.  No branches: a thread's PIX pixels are measured side by side,
// so their fp64 logarithm chains overlap.
template <int C>
__device__ __forceinline__ Pixel measure(const float (&p)[C], long long g, const float (&thr)[C], int ignore_label) {
    Pixel r;
    int cnt = 0, first = 0;
    float pg = 0.f;
    double e = 0.0;
    r.flags = 0;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const float v = p[k];
        r.flags |= (v >= 0.f && v <= 1.f) ? 0 : 1;            // also NaN
        const bool pass = v > thr[k];
        first = (pass && cnt == 0) ? k : first;
        cnt += pass ? 1 : 0;
        pg = (g == (long long)k) ? v : pg;
        const double pk = (double)v;
        e = __dadd_rn(e, __dmul_rn(-pk, log(pk)));            // no contraction: what numpy computes, term by term
    }
    const bool ignored = g == (long long)ignore_label;
    r.flags |= (!ignored && (g < 0 || g >= C)) ? 2 : 0;
    r.pseudo = cnt == 1 ? first : -1;
    r.hit = !ignored && g == (long long)r.pseudo;
    const float diff = ignored ? 1.f : __fsub_rn(1.f, pg);    // in [0, 1] within the contract, a multiple of 2^-24
    r.d24 = (unsigned)(fminf(fmaxf(diff, 0.f), 1.f) * 0x1p24f);
    r.entropy = (float)e;
    return r;
}

// a measured pixel -> the LDS tables (a pixel that raised a flag bit is skipped)
template <int C>
__device__ __forceinline__ void count(const Pixel& x, int R, const Lds& s) {
    if (x.flags) return;
    if (x.entropy != x.entropy) {
        count_row<C>(s, R, x.pseudo, x.hit, x.d24);
        return;
    }
    const int cand = bin_candidate(s.lo, R, x.entropy);
#pragma unroll
    for (int d = -1; d <= 1; ++d) {
        const int j = cand + d;
        if (j >= 0 && j < R && s.lo[j] <= x.entropy && x.entropy < s.hi[j]) count_row<C>(s, j, x.pseudo, x.hit, x.d24);
    }
}

// Grid (workgroups per image, b).  VEC: 16-byte loads, four consecutive pixels per thread (every plane and the image's
// gt row start on a 16-byte boundary: hw % 4 == 0 and aligned bases); otherwise a thread's pixels are 256 apart.
template <int C, bool VEC>
__global__ void __launch_bounds__(256) analysis_kernel(const float* __restrict__ soft, const int64_t* __restrict__ gt,
                                                       const float* __restrict__ classmax, const float* __restrict__ lo,
                                                       const float* __restrict__ hi, long long* __restrict__ tables,
                                                       int* __restrict__ flag, int hw, int R, float top, float low,
                                                       int ignore_label) {
    __shared__ unsigned s_used[(RMAX + 1) * C], s_hit[(RMAX + 1) * C], s_inbin[RMAX + 1];
    __shared__ unsigned long long s_diff24[RMAX + 1];
    __shared__ float s_lo[RMAX], s_hi[RMAX];
    const int b = blockIdx.y, tid = threadIdx.x;
    const Tables t = tables_of(C, R);
    for (int i = tid; i < t.rows * C; i += 256) { s_used[i] = 0; s_hit[i] = 0; }
    for (int i = tid; i < t.rows; i += 256) { s_inbin[i] = 0; s_diff24[i] = 0; }
    for (int i = tid; i < R; i += 256) { s_lo[i] = lo[i]; s_hi[i] = hi[i]; }
    float thr[C];
#pragma unroll
    for (int k = 0; k < C; ++k) thr[k] = fmaxf(__fmul_rn(classmax[b * C + k], top), low);      // pseudo_pick_kernel's rule
    __syncthreads();
    const Lds s = {s_used, s_hit, s_inbin, s_diff24, s_lo, s_hi};
    const float* base = soft + (size_t)b * C * hw;
    const int64_t* g = gt + (size_t)b * hw;
    const int ntile = (hw + TILE - 1) / TILE;
    int flags = 0;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        float v[PIX][C];
        long long gv[PIX];
        bool valid[PIX];
        if constexpr (VEC) {
            const int i0 = tile * TILE + tid * PIX;
#pragma unroll
            for (int j = 0; j < PIX; ++j) valid[j] = i0 < hw;        // hw % 4 == 0: four pixels or none
            if (i0 < hw) {
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    const float4 q = *(const float4*)(base + (size_t)k * hw + i0);
                    v[0][k] = q.x; v[1][k] = q.y; v[2][k] = q.z; v[3][k] = q.w;
                }
                const longlong2 g0 = *(const longlong2*)(g + i0), g1 = *(const longlong2*)(g + i0 + 2);
                gv[0] = g0.x; gv[1] = g0.y; gv[2] = g1.x; gv[3] = g1.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < PIX; ++j) {
                const int at = tile * TILE + j * 256 + tid;
                valid[j] = at < hw;
                if (valid[j]) {
#pragma unroll
                    for (int k = 0; k < C; ++k) v[j][k] = base[(size_t)k * hw + at];
                    gv[j] = g[at];
                }
            }
        }
        Pixel px[PIX];
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            if (!valid[j]) {          // past the image: a pixel that measures cleanly and is not counted
                gv[j] = ignore_label;
#pragma unroll
                for (int k = 0; k < C; ++k) v[j][k] = 1.f;
            }
            px[j] = measure<C>(v[j], gv[j], thr, ignore_label);
        }
#pragma unroll
        for (int j = 0; j < PIX; ++j)
            if (valid[j]) {
                flags |= px[j].flags;
                count<C>(px[j], R, s);
            }
    }
    if (flags) atomicOr(flag, flags);
    __syncthreads();
    unsigned long long* T = (unsigned long long*)tables + (size_t)b * t.len;
    for (int i = tid; i < t.rows * C; i += 256) {
        if (s_used[i]) atomicAdd(&T[t.used + i], (unsigned long long)s_used[i]);
        if (s_hit[i]) atomicAdd(&T[t.hit + i], (unsigned long long)s_hit[i]);
    }
    for (int i = tid; i < t.rows; i += 256) {
        if (s_inbin[i]) atomicAdd(&T[t.inbin + i], (unsigned long long)s_inbin[i]);
        if (s_diff24[i]) atomicAdd(&T[t.diff24 + i], s_diff24[i]);
    }
}

struct State {        // byte offsets into the running state
    size_t total, acc_sum, diffi_sum, images, acc_cnt, diffi_cnt, flag, bytes;
};
static __host__ __device__ inline State state_of(int c, int R) {
    State s;
    s.total = 0;
    s.acc_sum = (size_t)tables_of(c, R).len * 8;
    s.diffi_sum = s.acc_sum + (size_t)R * 8;
    s.images = s.diffi_sum + (size_t)R * 8;
    s.acc_cnt = s.images + 8;
    s.diffi_cnt = s.acc_cnt + (size_t)R * 4;
    s.flag = s.diffi_cnt + (size_t)R * 4;
    s.bytes = (s.flag + 4 + 7) & ~(size_t)7;
    return s;
}

__global__ void __launch_bounds__(256) analysis_fold_kernel(const long long* __restrict__ tables, const int* __restrict__ bflag,
                                                            char* __restrict__ state, int b, int c, int R) {
    const Tables t = tables_of(c, R);
    const State s = state_of(c, R);
    const int tid = threadIdx.x;
    long long* total = (long long*)(state + s.total);
    for (int j = tid; j < t.len; j += 256) {
        long long sum = 0;
        for (int img = 0; img < b; ++img) sum += tables[(size_t)img * t.len + j];
        total[j] += sum;
    }
    if (tid < R) {      // R <= 256: one bin per thread, the images in order
        double acc_sum = ((double*)(state + s.acc_sum))[tid], diffi_sum = ((double*)(state + s.diffi_sum))[tid];
        int acc_cnt = ((int*)(state + s.acc_cnt))[tid], diffi_cnt = ((int*)(state + s.diffi_cnt))[tid];
        for (int img = 0; img < b; ++img) {
            const long long* T = tables + (size_t)img * t.len;
            long long used = 0, hit = 0;
            for (int k = 0; k < c; ++k) {
                used += T[t.used + tid * c + k] + T[t.used + R * c + k];
                hit += T[t.hit + tid * c + k] + T[t.hit + R * c + k];
            }
            const long long d24 = T[t.diff24 + tid] + T[t.diff24 + R];
            acc_sum += (double)hit / ((double)used + 1e-7);
            acc_cnt += used != 0;
            diffi_sum += ((double)d24 * 0x1p-24) / ((double)T[t.inbin + tid] + 1e-7);
            diffi_cnt += d24 != 0;
        }
        ((double*)(state + s.acc_sum))[tid] = acc_sum;
        ((double*)(state + s.diffi_sum))[tid] = diffi_sum;
        ((int*)(state + s.acc_cnt))[tid] = acc_cnt;
        ((int*)(state + s.diffi_cnt))[tid] = diffi_cnt;
    }
    if (tid == 0) {
        *(long long*)(state + s.images) += b;
        *(int*)(state + s.flag) |= *bflag;
    }
}

static int shape_status(int b, int c, int R) {
    if (b <= 0 || R < 1 || R > RMAX) return RGDA_ERR_ARG;
    if (!class_count_ok(c)) return RGDA_ERR_UNSUPPORTED;
    return RGDA_OK;
}
static size_t tables_bytes_of(int b, int c, int R) { return (size_t)b * tables_of(c, R).len * 8; }

}  // namespace

extern "C" size_t rgda_pseudo_analysis_workspace(int b, int c, int R) {
    if (shape_status(b, c, R) != RGDA_OK) return 0;
    return (tables_bytes_of(b, c, R) + 8 + (size_t)b * c * 4 + 15) & ~(size_t)15;
}

extern "C" int rgda_pseudo_analysis(const float* soft, const int64_t* gt, const float* lo, const float* hi, int b, int c, int H,
                                    int W, int R, float cutoff_top, float cutoff_low, int ignore_label, void* tables,
                                    size_t tables_bytes, rgda_stream_t stream) {
    if (!soft || !gt || !lo || !hi || !tables || H <= 0 || W <= 0) return RGDA_ERR_ARG;
    if (int st = shape_status(b, c, R)) return st;
    if ((long long)b * H * W >= (1ll << 31)) return RGDA_ERR_ARG;       // pixel index and counts: 32 bits
    // one image: the passes step through it in int arithmetic (the maximum pass by its chunk); grid y: b and b * c
    if ((long long)H * W > (1ll << 31) - MAX_CHUNK || (long long)b * c > 65535) return RGDA_ERR_ARG;
    if (((uintptr_t)soft & 3) || ((uintptr_t)gt & 7) || ((uintptr_t)tables & 7)) return RGDA_ERR_ARG;
    const size_t need = rgda_pseudo_analysis_workspace(b, c, R);
    if (tables_bytes < need) return RGDA_ERR_WORKSPACE;
    const int hw = H * W;
    int* flag = (int*)((char*)tables + tables_bytes_of(b, c, R));
    float* classmax = (float*)(flag + 2);
    if (zero_bytes(tables, need, stream) != RGDA_OK) return RGDA_ERR_LAUNCH;
    hipStream_t st = to_stream(stream);
    // the maximum pass takes 16-byte loads when hw and its chunk are multiples of 4, whatever the base: a chunk that is
    // not keeps it on its scalar loads where the planes do not start on 16-byte boundaries
    const int chunk = ((uintptr_t)soft & 15) ? MAX_CHUNK - 1 : MAX_CHUNK;
    pseudo_max_kernel<<<dim3(cdiv(hw, chunk), b * c), 256, 0, st>>>(soft, classmax, flag, hw, chunk);
    RGDA_CHECK_LAUNCH();
    const bool vec = !(hw & 3) && !((uintptr_t)soft & 15) && !((uintptr_t)gt & 15);
    int max_wg = MAX_WG;
    if (const char* e = TUNE_ENV("RGDA_ANALYSIS_WG")) max_wg = max(atoi(e), 1);            // tuning experiments only
    const dim3 grid(min(cdiv(hw, TILE), max(max_wg / b, 1)), b);
    return with_classes(c, [&](auto cc) -> int {
        constexpr int C = decltype(cc)::value;
        if (vec)
            analysis_kernel<C, true><<<grid, 256, 0, st>>>(soft, gt, classmax, lo, hi, (long long*)tables, flag, hw, R,
                                                            cutoff_top, cutoff_low, ignore_label);
        else
            analysis_kernel<C, false><<<grid, 256, 0, st>>>(soft, gt, classmax, lo, hi, (long long*)tables, flag, hw, R,
                                                             cutoff_top, cutoff_low, ignore_label);
        RGDA_CHECK_LAUNCH();
        return RGDA_OK;
    });
}

extern "C" size_t rgda_pseudo_analysis_fold_workspace(int c, int R) {
    if (shape_status(1, c, R) != RGDA_OK) return 0;
    return state_of(c, R).bytes;
}

extern "C" int rgda_pseudo_analysis_fold(const void* tables, size_t tables_bytes, int b, int c, int R, void* state,
                                         size_t state_bytes, rgda_stream_t stream) {
    if (!tables || !state || (((uintptr_t)tables | (uintptr_t)state) & 7)) return RGDA_ERR_ARG;
    if (int st = shape_status(b, c, R)) return st;
    if (tables_bytes < rgda_pseudo_analysis_workspace(b, c, R) || state_bytes < state_of(c, R).bytes) return RGDA_ERR_WORKSPACE;
    const int* bflag = (const int*)((const char*)tables + tables_bytes_of(b, c, R));
    analysis_fold_kernel<<<1, 256, 0, to_stream(stream)>>>((const long long*)tables, bflag, (char*)state, b, c, R);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
