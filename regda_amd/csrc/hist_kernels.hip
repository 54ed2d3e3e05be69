// Histogram matching of the source tile (include/rgda_hip.h: rgda_hist_style carries the contract): per channel, the
// grey-level distribution of a source plane is mapped onto that of its partner target plane.  Four launches --
//   setup   the rows as served (Head; a bad row becomes a copy and sets the flag) and the zeroed counters
//   hist    counts[(N + M) 3][256] of ALL planes: a workgroup owns a contiguous chunk of one plane, bins in LDS (one
//           private copy per wave, integer LDS atomics), then integer global atomics of the nonzero bins
//   lut     one workgroup per (source image, channel): prefix sums, the occupied target levels compacted, a binary search
//           per source level, L in fp64 and the correction D[v] = (float)(beta (L[v] - v) / std_s)
//   apply   out = x + D[v(x)] (D in LDS), or the copy of an off row; the source tile is read once
// Only integers are summed: the result does not depend on the order of the atomics.
// rgda_hist_style_write_table carries the host's table to the device in its launch arguments.
#include "common.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int HS_IMGS = RGDA_STYLE_MAX_IMAGES;
constexpr int HS_MAX_SIDE = 4096;
constexpr int HS_THREADS = 256;
constexpr int HS_WAVES = HS_THREADS / 64;
constexpr int HS_BINS = 256;
constexpr int HS_CHUNK = 8192;              // elements of a plane per workgroup (a multiple of 4): 32 workgroups at 512 x 512

struct Norm2 {
    float mean_s[3], std_s[3], mean_t[3], std_t[3];
};

// The rows as served, at the base of the workspace: 256 bytes
struct Head {
    int src_q[HS_IMGS];                     // blend_q of source image n, -1: copy it
    int src_p[HS_IMGS];                     // its partner
    int pad[2 * HS_IMGS];
};
static_assert(sizeof(Head) == 256, "Head is 256 bytes");

// the workspace: Head, counts uint32 [(N + M) 3][256], D f32 [N 3][256]
struct Layout {
    size_t counts, D, total;
};
Layout layout(int N, int M) {
    Layout l;
    l.counts = sizeof(Head);
    l.D = l.counts + (size_t)(N + M) * 3 * HS_BINS * sizeof(uint32_t);
    l.total = l.D + (size_t)N * 3 * HS_BINS * sizeof(float);
    return l;
}

__device__ __forceinline__ bool row_ok(const int* __restrict__ row, int M) {
    return row[0] >= 0 && row[0] < M && row[1] >= 0 && row[1] <= RGDA_HIST_BLEND_ONE && (row[2] == 0 || row[2] == 1);
}

// the grey level of a normalised pixel: fmaxf / fminf drop a NaN, so the result is a bin for every bit pattern
__device__ __forceinline__ int level(float x, float std, float mean) {
    return (int)fminf(fmaxf(rintf(fmaf(x, std, mean)), 0.f), 255.f);
}

// How `cnt` floats at p are walked: `head` single elements up to the first 16-byte boundary, nvec groups of four, `tail`
// single elements.  A pointer that is not a multiple of 4 bytes never reaches a boundary: all single.
struct Span {
    int head, nvec, tail;
};
__device__ __forceinline__ Span span_of(const void* p, int cnt) {
    const uintptr_t a = (uintptr_t)p;
    Span s;
    s.head = (a & 3) ? cnt : min(cnt, (int)(((16 - (a & 15)) & 15) >> 2));
    s.nvec = (cnt - s.head) >> 2;
    s.tail = cnt - s.head - 4 * s.nvec;
    return s;
}

// grid over the (N + M) 3 x 256 counters; workgroup 0 also writes the Head
__global__ void __launch_bounds__(HS_THREADS) hist_setup_kernel(const int* __restrict__ table, Head* __restrict__ head,
                                                                uint32_t* __restrict__ counts, int n_counts, int N, int M,
                                                                int* __restrict__ flag) {
    const int i = blockIdx.x * HS_THREADS + threadIdx.x;
    if (i < n_counts) counts[i] = 0u;
    if (blockIdx.x == 0 && threadIdx.x < HS_IMGS) {
        const int t = threadIdx.x;
        int q = -1, p = 0;
        if (t < N) {
            const int* row = table + t * RGDA_STYLE_TABLE_COLS;
            if (!row_ok(row, M)) {
                if (flag) *flag = 1;
            } else if (row[2] == 1) {
                q = row[1];
                p = row[0];
            }
        }
        head->src_q[t] = q;
        head->src_p[t] = p;
        head->pad[t] = 0;
        head->pad[HS_IMGS + t] = 0;
    }
}

// grid (chunks, (N + M) 3): one chunk of one plane into the workgroup's LDS bins, the nonzero bins onto the counters
__global__ void __launch_bounds__(HS_THREADS) hist_count_kernel(const float* __restrict__ img_s, const float* __restrict__ img_t,
                                                                uint32_t* __restrict__ counts, int N, int HW, Norm2 nm) {
    __shared__ uint32_t s_bin[HS_WAVES][HS_BINS];
    const int plane = blockIdx.y, img = plane / 3, ch = plane % 3, tid = threadIdx.x;
    const bool src = img < N;
    const float* base = (src ? img_s + (size_t)img * 3 * HW : img_t + (size_t)(img - N) * 3 * HW) + (size_t)ch * HW;
    const float mean = src ? nm.mean_s[ch] : nm.mean_t[ch], std = src ? nm.std_s[ch] : nm.std_t[ch];
    const int start = blockIdx.x * HS_CHUNK, cnt = min(HS_CHUNK, HW - start);
    const float* p = base + start;
    for (int i = tid; i < HS_WAVES * HS_BINS; i += HS_THREADS) (&s_bin[0][0])[i] = 0u;
    __syncthreads();
    uint32_t* mine = s_bin[tid >> 6];
    const Span sp = span_of(p, cnt);
    for (int i = tid; i < sp.head; i += HS_THREADS) atomicAdd(mine + level(p[i], std, mean), 1u);
    const float* pv = p + sp.head;
    for (int i = tid; i < sp.nvec; i += HS_THREADS) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(pv + 4 * i);
        atomicAdd(mine + level(v.x, std, mean), 1u);
        atomicAdd(mine + level(v.y, std, mean), 1u);
        atomicAdd(mine + level(v.z, std, mean), 1u);
        atomicAdd(mine + level(v.w, std, mean), 1u);
    }
    if (tid < sp.tail) atomicAdd(mine + level(pv[4 * sp.nvec + tid], std, mean), 1u);
    __syncthreads();
    uint32_t sum = 0u;
#pragma unroll
    for (int w = 0; w < HS_WAVES; ++w) sum += s_bin[w][tid];
    if (sum) atomicAdd(counts + (size_t)plane * HS_BINS + tid, sum);
}

// grid (N + M) 3: a workgroup per plane, a thread per level.  Source planes: L and D; every plane: its row of `hist`
__global__ void __launch_bounds__(HS_THREADS) hist_lut_kernel(const Head* __restrict__ head, const uint32_t* __restrict__ counts,
                                                              float* __restrict__ D, uint32_t* __restrict__ hist,
                                                              double* __restrict__ lut, int N, Norm2 nm) {
#pragma clang fp contract(off)
    __shared__ uint32_t s_cs[HS_BINS], s_ct[HS_BINS];       // the counts, then their inclusive prefix sums
    __shared__ uint32_t s_cu[HS_BINS];                      // ct at the occupied target levels
    __shared__ int s_u[HS_BINS], s_k;                       // the occupied target levels, their number
    const int plane = blockIdx.x, v = threadIdx.x;
    if (hist) hist[(size_t)plane * HS_BINS + v] = counts[(size_t)plane * HS_BINS + v];
    if (plane >= N * 3) return;
    const int n = plane / 3, ch = plane % 3;
    const int q = head->src_q[n];
    if (q < 0) {                                            // off, or not served: never read by the apply pass
        if (lut) lut[(size_t)plane * HS_BINS + v] = (double)v;
        return;
    }
    const int tp = (N + head->src_p[n]) * 3 + ch;
    const uint32_t hs = counts[(size_t)plane * HS_BINS + v], ht = counts[(size_t)tp * HS_BINS + v];
    s_cs[v] = hs;
    s_ct[v] = ht;
    __syncthreads();
    uint32_t cs = 0u, ct = 0u;
    int rank = 0;                                           // occupied target levels below v
    for (int i = 0; i <= v; ++i) {
        cs += s_cs[i];
        ct += s_ct[i];
        rank += (i < v && s_ct[i] > 0u) ? 1 : 0;
    }
    if (ht > 0u) {
        s_u[rank] = v;
        s_cu[rank] = ct;
    }
    if (v == HS_BINS - 1) s_k = rank + (ht > 0u ? 1 : 0);   // >= 1: the target plane has HW >= 1 pixels
    __syncthreads();
    double L = (double)v;
    if (hs > 0u) {
        const int k = s_k;
        int lo = -1, hi = k;                                // the largest j with cu[j] <= cs: cu[lo] <= cs < cu[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_cu[mid] <= cs) lo = mid; else hi = mid;
        }
        if (lo < 0) {
            L = (double)s_u[0];
        } else if (lo == k - 1) {
            L = (double)s_u[k - 1];
        } else {
            const unsigned long long num = (unsigned long long)(cs - s_cu[lo]) * (unsigned long long)(s_u[lo + 1] - s_u[lo]);
            const unsigned long long den = (unsigned long long)(s_cu[lo + 1] - s_cu[lo]);
            const double frac = (double)num / (double)den;
            L = (double)s_u[lo] + frac;
        }
    }
    const double beta = (double)q / (double)RGDA_HIST_BLEND_ONE;
    const double diff = L - (double)v;
    const double prod = beta * diff;
    D[(size_t)plane * HS_BINS + v] = (float)(prod / (double)nm.std_s[ch]);
    if (lut) lut[(size_t)plane * HS_BINS + v] = L;
}

// grid (chunks, N 3): one chunk of one source plane -- x + D[v(x)], or the copy of an off row.  16-byte loads and stores
// where source and result reach a 16-byte boundary together
__global__ void __launch_bounds__(HS_THREADS) hist_apply_kernel(const float* __restrict__ img_s, float* __restrict__ out,
                                                                const Head* __restrict__ head, const float* __restrict__ D,
                                                                int HW, Norm2 nm) {
    __shared__ float s_d[HS_BINS];
    const int plane = blockIdx.y, ch = plane % 3, tid = threadIdx.x;
    const bool on = head->src_q[plane / 3] >= 0;            // the same for every thread of the workgroup
    const int start = blockIdx.x * HS_CHUNK, cnt = min(HS_CHUNK, HW - start);
    const float* src = img_s + (size_t)plane * HW + start;
    float* dst = out + (size_t)plane * HW + start;
    Span sp = span_of(src, cnt);
    if (((uintptr_t)src & 15) != ((uintptr_t)dst & 15)) sp = Span{cnt, 0, 0};
    const float* sv = src + sp.head;
    float* dv = dst + sp.head;
    if (!on) {                                              // a copy, no arithmetic
        for (int i = tid; i < sp.head; i += HS_THREADS) dst[i] = src[i];
        for (int i = tid; i < sp.nvec; i += HS_THREADS)
            *reinterpret_cast<f32x4*>(dv + 4 * i) = *reinterpret_cast<const f32x4*>(sv + 4 * i);
        if (tid < sp.tail) dv[4 * sp.nvec + tid] = sv[4 * sp.nvec + tid];
        return;
    }
    s_d[tid] = D[(size_t)plane * HS_BINS + tid];
    __syncthreads();
    const float mean = nm.mean_s[ch], std = nm.std_s[ch];
    for (int i = tid; i < sp.head; i += HS_THREADS) dst[i] = src[i] + s_d[level(src[i], std, mean)];
    for (int i = tid; i < sp.nvec; i += HS_THREADS) {
        f32x4 x = *reinterpret_cast<const f32x4*>(sv + 4 * i);
        x.x += s_d[level(x.x, std, mean)];
        x.y += s_d[level(x.y, std, mean)];
        x.z += s_d[level(x.z, std, mean)];
        x.w += s_d[level(x.w, std, mean)];
        *reinterpret_cast<f32x4*>(dv + 4 * i) = x;
    }
    if (tid < sp.tail) {
        const float x = sv[4 * sp.nvec + tid];
        dv[4 * sp.nvec + tid] = x + s_d[level(x, std, mean)];
    }
}

// ---- rgda_hist_style_write_table: the table travels in the launch's own argument block
struct HistDraw {
    int rows[HS_IMGS * RGDA_STYLE_TABLE_COLS];
};
__global__ void __launch_bounds__(64) hist_write_table_kernel(int* __restrict__ table, HistDraw d, int n) {
    for (int i = threadIdx.x; i < n * RGDA_STYLE_TABLE_COLS; i += 64) table[i] = d.rows[i];
}

bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" size_t rgda_hist_style_workspace(int N, int M, int H, int W) {
    if (N < 1 || M < 1 || H < 1 || W < 1 || N > HS_IMGS || M > HS_IMGS || H > HS_MAX_SIDE || W > HS_MAX_SIDE) return 0;
    return layout(N, M).total;
}

extern "C" int rgda_hist_style(const float* img_s, const float* img_t, float* out, const int32_t* table, void* ws, int N, int M,
                               int H, int W, float mean_sr, float mean_sg, float mean_sb, float std_sr, float std_sg,
                               float std_sb, float mean_tr, float mean_tg, float mean_tb, float std_tr, float std_tg,
                               float std_tb, uint32_t* hist, double* lut, int* flag, rgda_stream_t stream) {
    if (!img_s || !img_t || !out || !ws || !aligned_to(ws, 16) || !table || !aligned_to(table, 16)) return RGDA_ERR_ARG;
    if (!aligned_to(hist, 4) || !aligned_to(lut, 8)) return RGDA_ERR_ARG;
    if (N < 1 || M < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    const Norm2 nm = {{mean_sr, mean_sg, mean_sb}, {std_sr, std_sg, std_sb}, {mean_tr, mean_tg, mean_tb}, {std_tr, std_tg, std_tb}};
    for (int c = 0; c < 3; ++c) {
        if (!(nm.std_s[c] > 0.f) || !(nm.std_t[c] > 0.f) || !isfinite(nm.std_s[c]) || !isfinite(nm.std_t[c])) return RGDA_ERR_ARG;
        if (!isfinite(nm.mean_s[c]) || !isfinite(nm.mean_t[c])) return RGDA_ERR_ARG;
    }
    if (N > HS_IMGS || M > HS_IMGS || H > HS_MAX_SIDE || W > HS_MAX_SIDE) return RGDA_ERR_UNSUPPORTED;
    const int HW = H * W;                               // <= 2^24
    const size_t plane = (size_t)3 * HW * sizeof(float);
    if (overlap(out, N * plane, img_s, N * plane) || overlap(out, N * plane, img_t, M * plane)) return RGDA_ERR_ARG;
    const Layout l = layout(N, M);
    char* base = (char*)ws;
    Head* head = (Head*)base;
    uint32_t* counts = (uint32_t*)(base + l.counts);
    float* D = (float*)(base + l.D);
    hipStream_t s = to_stream(stream);
    const int planes = (N + M) * 3, n_counts = planes * HS_BINS, chunks = cdiv(HW, HS_CHUNK);
    hist_setup_kernel<<<cdiv(n_counts, HS_THREADS), HS_THREADS, 0, s>>>(table, head, counts, n_counts, N, M, flag);
    RGDA_CHECK_LAUNCH();
    hist_count_kernel<<<dim3(chunks, planes), HS_THREADS, 0, s>>>(img_s, img_t, counts, N, HW, nm);
    RGDA_CHECK_LAUNCH();
    hist_lut_kernel<<<planes, HS_THREADS, 0, s>>>(head, counts, D, hist, lut, N, nm);
    RGDA_CHECK_LAUNCH();
    hist_apply_kernel<<<dim3(chunks, N * 3), HS_THREADS, 0, s>>>(img_s, out, head, D, HW, nm);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_hist_style_write_table(int32_t* table, const int32_t* host, int N, int M, int H, int W,
                                           rgda_stream_t stream) {
    if (!table || !aligned_to(table, 16) || !host || N < 1 || M < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    if (N > HS_IMGS || M > HS_IMGS) return RGDA_ERR_UNSUPPORTED;
    HistDraw d = {};
    for (int n = 0; n < N; ++n) {
        const int32_t* r = host + n * RGDA_STYLE_TABLE_COLS;
        if (r[0] < 0 || r[0] >= M || r[1] < 0 || r[1] > RGDA_HIST_BLEND_ONE || (r[2] != 0 && r[2] != 1)) return RGDA_ERR_ARG;
        memcpy(d.rows + n * RGDA_STYLE_TABLE_COLS, r, 3 * sizeof(int32_t));        // column 3 stays 0
    }
    hist_write_table_kernel<<<1, 64, 0, to_stream(stream)>>>(table, d, N);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
