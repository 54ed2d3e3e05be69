// Batched sliding-window inference (include/rgda_hip.h: rgda_window_gather / _scatter / _finish): the window loop of
// regda/utils/tools.py:61-97 with K windows (x V test-time views) per network forward instead of one.  Every value is
// moved, or added in the order the per-window path adds it (teacher_kernels.hip), so the batched route reproduces
// window_crop + dihedral, tta_predict's de-augmented mean + window_accumulate, and window_normalise + argmax (+ the
// confusion matrix) bit for bit.  A window table row is (image, y1, x1), int32, in DEVICE memory (a plan can record the
// call); rows are checked where they are read, an invalid row is skipped and sets *flag.
// rgda_window_gather_scaled / rgda_scale_merge run the same loop over the image at several scales (tools.py:108-129).
#include "common.h"

namespace {

constexpr int WIN_THREADS = 256;
constexpr int WIN_MAX_K = 1024;                 // window rows per scatter launch (staged in LDS: 12 KiB)

// View v = (f, k) = (v >> 2, v & 3) in tta_predict's order: view = R^k(F^f(tile)) of a T x T tile (rgda_dihedral_nchw
// with flip_first = 1).  Output pixel (i, j) of the view reads tile pixel (y, x):
__device__ __forceinline__ void view_source(int v, int T, int i, int j, int& y, int& x) {
    y = i; x = j;
    for (int s = 0; s < (v & 3); ++s) { const int t = y; y = x; x = T - 1 - t; }     // R(z)[i][j] = z[j][T-1-i]
    if (v >> 2) x = T - 1 - x;
}

// ... and the inverse: tile pixel (y, x) sits at (i, j) of the view (F first, then R k times: (y, x) -> (T-1-x, y)).
// De-augmenting the view (rgda_dihedral_nchw with flip_first = 0, rot (4-k)%4) reads exactly that element.
__device__ __forceinline__ void view_position(int v, int T, int y, int x, int& i, int& j) {
    i = y; j = (v >> 2) ? T - 1 - x : x;
    for (int s = 0; s < (v & 3); ++s) { const int t = i; i = T - 1 - j; j = t; }
}

__device__ __forceinline__ bool window_ok(int img, int y1, int x1, int n, int H, int W, int Th, int Tw) {
    return img >= 0 && img < n && y1 >= 0 && x1 >= 0 && y1 <= H - Th && x1 <= W - Tw;
}

// out[r = w*V + v][c][i][j] = view v of window w; src fp32 NCHW, or uint8 HWC through lut[c][byte]
__global__ void __launch_bounds__(WIN_THREADS) window_gather_kernel(const float* __restrict__ src_f32,
                                                                    const uint8_t* __restrict__ src_u8,
                                                                    const float* __restrict__ lut,
                                                                    const int32_t* __restrict__ wins, int K, int V, int n,
                                                                    int C, int H, int W, int Th, int Tw,
                                                                    float* __restrict__ out, int* __restrict__ flag) {
    const long long plane = (long long)Th * Tw, total = (long long)K * V * C * plane;
    for (long long e = (long long)blockIdx.x * WIN_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * WIN_THREADS) {
        const int j = (int)(e % Tw), i = (int)((e / Tw) % Th);
        const long long rc = e / plane;
        const int c = (int)(rc % C), r = (int)(rc / C);
        const int w = r / V, v = r - w * V;
        const int img = wins[3 * w], y1 = wins[3 * w + 1], x1 = wins[3 * w + 2];
        if (!window_ok(img, y1, x1, n, H, W, Th, Tw)) {
            out[e] = 0.f;
            if (flag) *flag = 1;
            continue;
        }
        int y, x;
        view_source(v, Th, i, j, y, x);
        y += y1; x += x1;
        out[e] = src_u8 ? lut[c * 256 + src_u8[(((long long)img * H + y) * W + x) * 3 + c]]
                        : src_f32[(((long long)img * C + c) * H + y) * W + x];
    }
}

// One thread per pixel (img, y, x) of the flattened image rows [row0, row0 + rows): walks the K windows in table order
// (pre_slide's visiting order) and adds each covering window's value -- with V = 8 first the de-augmented mean of its
// views, summed in view order as tta_predict sums them -- into full, and 1 into count.
__global__ void __launch_bounds__(WIN_THREADS) window_scatter_kernel(const float* __restrict__ pred,
                                                                     const int32_t* __restrict__ wins, int K, int V, int n,
                                                                     int C, int H, int W, int Th, int Tw, int row0,
                                                                     int rows, float scale, float* __restrict__ full,
                                                                     float* __restrict__ count, int* __restrict__ flag) {
    __shared__ int s_win[3 * WIN_MAX_K];
    for (int k = threadIdx.x; k < 3 * K; k += WIN_THREADS) s_win[k] = wins[k];
    __syncthreads();
    const long long total = (long long)rows * W, plane = (long long)Th * Tw;
    if (flag && blockIdx.x == 0)
        for (int w = threadIdx.x; w < K; w += WIN_THREADS)
            if (!window_ok(s_win[3 * w], s_win[3 * w + 1], s_win[3 * w + 2], n, H, W, Th, Tw)) *flag = 1;
    for (long long e = (long long)blockIdx.x * WIN_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * WIN_THREADS) {
        const int x = (int)(e % W);
        const long long row = row0 + e / W;
        const int img = (int)(row / H), y = (int)(row % H);
        int hits = 0;
        for (int c = 0; c < C; ++c) {
            float acc = full[(((long long)img * C + c) * H + y) * W + x];
            for (int w = 0; w < K; ++w) {
                const int wi = s_win[3 * w], y1 = s_win[3 * w + 1], x1 = s_win[3 * w + 2];
                if (wi != img || y < y1 || y >= y1 + Th || x < x1 || x >= x1 + Tw || !window_ok(wi, y1, x1, n, H, W, Th, Tw))
                    continue;
                const int wy = y - y1, wx = x - x1;
                float t = 0.f;
                if (V == 1) {
                    t = pred[((long long)w * C + c) * plane + (long long)wy * Tw + wx];
                } else {
                    for (int v = 0; v < V; ++v) {
                        int pi, pj;
                        view_position(v, Th, wy, wx, pi, pj);
                        const float u = scale * pred[(((long long)w * V + v) * C + c) * plane + (long long)pi * Tw + pj];
                        t = v ? t + u : u;
                    }
                }
                acc += t;
                if (c == 0) ++hits;
            }
            full[(((long long)img * C + c) * H + y) * W + x] = acc;
        }
        if (hits) {
            float cnt = count[(long long)img * H * W + (long long)y * W + x];
            for (int h = 0; h < hits; ++h) cnt += 1.f;
            count[(long long)img * H * W + (long long)y * W + x] = cnt;
        }
    }
}

// full /= count (window_norm_kernel's __fdiv_rn), then the first maximum over the classes (argmax_nchw_kernel) as uint8
// or int64 labels, and the confusion matrix of the pixels with y_true >= 0 (confusion_kernel: LDS histogram, one
// 64-bit atomic per nonzero cell per workgroup).
__global__ void __launch_bounds__(WIN_THREADS) window_finish_kernel(float* __restrict__ full, const float* __restrict__ count,
                                                                    int C, long long HW, long long total,
                                                                    uint8_t* __restrict__ lab_u8, int64_t* __restrict__ lab_i64,
                                                                    const int64_t* __restrict__ yt,
                                                                    unsigned long long* __restrict__ cm, int* __restrict__ flag) {
    extern __shared__ unsigned int hist[];       // [C*C] when cm
    if (cm) {
        for (int i = threadIdx.x; i < C * C; i += WIN_THREADS) hist[i] = 0;
        __syncthreads();
    }
    int bad = 0;
    for (long long i = (long long)blockIdx.x * WIN_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * WIN_THREADS) {
        const long long img = i / HW, p = i % HW;
        float* s = full + img * C * HW + p;
        const float cnt = count[i];
        float best = 0.f;
        int arg = 0;
        for (int c = 0; c < C; ++c) {
            const float v = __fdiv_rn(s[(long long)c * HW], cnt);
            s[(long long)c * HW] = v;
            if (c == 0) best = v;
            else if (v > best) { best = v; arg = c; }
        }
        if (lab_u8) lab_u8[i] = (uint8_t)arg;
        if (lab_i64) lab_i64[i] = arg;
        if (cm) {
            const long long t = yt[i];
            if (t >= C) bad = 1;
            else if (t >= 0) atomicAdd(&hist[(int)t * C + arg], 1u);
        }
    }
    if (cm) {
        if (bad) atomicOr(flag, 1);
        __syncthreads();
        for (int i = threadIdx.x; i < C * C; i += WIN_THREADS)
            if (hist[i]) atomicAdd(&cm[i], (unsigned long long)hist[i]);
    }
}

// Multi-scale testing (regda/utils/tools.py:108-129): the align_corners=True resize of resize_ac_kernel
// (teacher_kernels.hip) fused into the window gather and into the per-scale merge.  Source position of output index I
// along an axis with `in` source samples, exactly as resize_ac_kernel forms it (f = s * (float)I, truncate, clamp the
// upper neighbour); the callers blend in its association with contraction off.  i0 is also kept inside the source, which
// changes nothing where resize_ac_kernel itself stays inside it.
__device__ __forceinline__ void ac_source(float s, int I, int in, int& i0, int& i1, float& l) {
#pragma clang fp contract(off)
    const float f = s * (float)I;
    i0 = (int)f;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    l = f - (float)i0;
}

// Pixel (Y, X) of plane c of the Hs x Ws image resize_ac_kernel would make of the (normalised) H x W source `img`; a uint8
// tap goes through lut first.
__device__ __forceinline__ float scaled_pixel(const float* __restrict__ f32, const uint8_t* __restrict__ u8,
                                              const float* __restrict__ lut, int H, int W, float sy, float sx, int Y, int X) {
#pragma clang fp contract(off)
    int ya, yb, xa, xb;
    float ly, lx;
    ac_source(sy, Y, H, ya, yb, ly);
    ac_source(sx, X, W, xa, xb, lx);
    const float my = 1.f - ly, mx = 1.f - lx;
    const long long oa = (long long)ya * W, ob = (long long)yb * W;
    float taa, tab, tba, tbb;
    if (u8) {
        taa = lut[u8[(oa + xa) * 3]]; tab = lut[u8[(oa + xb) * 3]];
        tba = lut[u8[(ob + xa) * 3]]; tbb = lut[u8[(ob + xb) * 3]];
    } else {
        taa = f32[oa + xa]; tab = f32[oa + xb];
        tba = f32[ob + xa]; tbb = f32[ob + xb];
    }
    const float top = mx * taa + lx * tab;                               // ATen's association
    const float bot = mx * tba + lx * tbb;
    return my * top + ly * bot;
}

// window_gather_kernel on that image, which is never stored: window rows index, and are checked against, the Hs x Ws
// image.  blockIdx.y walks the planes rc = (w*V + v)*C + c, so the window row, the view and the channel are uniform in
// a workgroup; a thread makes VEC consecutive pixels of one output row (VEC = 4: Tw % 4 == 0, out 16-byte aligned).
template <int VEC>
__global__ void __launch_bounds__(WIN_THREADS) window_gather_scaled_kernel(const float* __restrict__ src_f32,
                                                                           const uint8_t* __restrict__ src_u8,
                                                                           const float* __restrict__ lut,
                                                                           const int32_t* __restrict__ wins, int planes, int V,
                                                                           int n, int C, int H, int W, int Hs, int Ws,
                                                                           int Th, int Tw, float sy, float sx,
                                                                           float* __restrict__ out, int* __restrict__ flag) {
    const int per_row = Tw / VEC, per = Th * per_row;
    for (int rc = blockIdx.y; rc < planes; rc += gridDim.y) {
        const int c = rc % C, r = rc / C;
        const int w = r / V, v = r - w * V;
        const int img = wins[3 * w], y1 = wins[3 * w + 1], x1 = wins[3 * w + 2];
        const bool ok = window_ok(img, y1, x1, n, Hs, Ws, Th, Tw);
        if (!ok && flag && threadIdx.x == 0) *flag = 1;
        const float* f32 = src_f32 ? src_f32 + ((long long)img * C + c) * H * W : nullptr;
        const uint8_t* u8 = src_u8 ? src_u8 + (long long)img * H * W * 3 + c : nullptr;
        const float* t = src_u8 ? lut + c * 256 : nullptr;
        float* o = out + (long long)rc * Th * Tw;
        for (int q = blockIdx.x * WIN_THREADS + threadIdx.x; q < per; q += gridDim.x * WIN_THREADS) {
            const int i = q / per_row, j = (q - i * per_row) * VEC;
            float res[VEC];
#pragma unroll
            for (int u = 0; u < VEC; ++u) {
                res[u] = 0.f;
                if (ok) {
                    int y, x;
                    view_source(v, Th, i, j + u, y, x);
                    res[u] = scaled_pixel(f32, u8, t, H, W, sy, sx, y + y1, x + x1);
                }
            }
            if (VEC == 4) *reinterpret_cast<float4*>(o + (long long)i * Tw + j) = make_float4(res[0], res[1], res[2], res[3]);
            else o[(long long)i * Tw + j] = res[0];
        }
    }
}

// acc[n][c][Y][X] += resize_ac(full_s / count_s)[n][c][Y][X], cnt[n][0][Y][X] += 1: window_norm_kernel's __fdiv_rn on the
// four taps, resize_ac_kernel's blend, one add.  One thread per output pixel: the coordinates and the four count taps
// once, then the classes.  full_s is only read.
__global__ void __launch_bounds__(WIN_THREADS) scale_merge_kernel(const float* __restrict__ full_s,
                                                                  const float* __restrict__ count_s, int n, int C, int Hs,
                                                                  int Ws, int H, int W, float sy, float sx,
                                                                  float* __restrict__ acc, float* __restrict__ cnt) {
#pragma clang fp contract(off)
    const long long HW = (long long)H * W, HWs = (long long)Hs * Ws, total = (long long)n * HW;
    for (long long e = (long long)blockIdx.x * WIN_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * WIN_THREADS) {
        const long long img = e / HW, p = e % HW;
        const int X = (int)(p % W), Y = (int)(p / W);
        int ya, yb, xa, xb;
        float ly, lx;
        ac_source(sy, Y, Hs, ya, yb, ly);
        ac_source(sx, X, Ws, xa, xb, lx);
        const float my = 1.f - ly, mx = 1.f - lx;
        const long long oaa = (long long)ya * Ws + xa, oab = (long long)ya * Ws + xb;
        const long long oba = (long long)yb * Ws + xa, obb = (long long)yb * Ws + xb;
        const float* k = count_s + img * HWs;
        const float kaa = k[oaa], kab = k[oab], kba = k[oba], kbb = k[obb];
        for (int c = 0; c < C; ++c) {
            const float* s = full_s + (img * C + c) * HWs;
            const float top = mx * __fdiv_rn(s[oaa], kaa) + lx * __fdiv_rn(s[oab], kab);
            const float bot = mx * __fdiv_rn(s[oba], kba) + lx * __fdiv_rn(s[obb], kbb);
            float* a = acc + (img * C + c) * HW + p;
            *a = *a + (my * top + ly * bot);
        }
        cnt[e] = cnt[e] + 1.f;
    }
}

int grid_of(long long total, int cap) { long long g = (total + WIN_THREADS - 1) / WIN_THREADS; return (int)(g > cap ? cap : (g < 1 ? 1 : g)); }

// the scale exactly as ATen computes it (area_pixel_compute_scale, align_corners): a float division on the host
float ac_scale(int in, int out) { return (out > 1) ? (float)(in - 1) / (float)(out - 1) : 0.f; }

}  // namespace

extern "C" int rgda_window_gather(const float* src_f32, const uint8_t* src_u8, const float* lut, const int32_t* windows,
                                  int K, int views, int n, int C, int H, int W, int Th, int Tw, float* out, int* flag,
                                  rgda_stream_t stream) {
    if (!windows || !out || (!src_f32) == (!src_u8) || (src_u8 && (!lut || C != 3))) return RGDA_ERR_ARG;
    if (K < 1 || n < 1 || C < 1 || Th < 1 || Tw < 1 || H < Th || W < Tw) return RGDA_ERR_ARG;
    if ((views != 1 && views != 8) || (views == 8 && Th != Tw)) return RGDA_ERR_ARG;
    const long long total = (long long)K * views * C * Th * Tw;
    window_gather_kernel<<<grid_of(total, 65535), WIN_THREADS, 0, to_stream(stream)>>>(src_f32, src_u8, lut, windows, K, views,
                                                                                         n, C, H, W, Th, Tw, out, flag);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_window_gather_scaled(const float* src_f32, const uint8_t* src_u8, const float* lut,
                                         const int32_t* windows, int K, int views, int n, int C, int H, int W, int Hs, int Ws,
                                         int Th, int Tw, float* out, int* flag, rgda_stream_t stream) {
    if (!windows || !out || (!src_f32) == (!src_u8) || (src_u8 && (!lut || C != 3))) return RGDA_ERR_ARG;
    if (K < 1 || n < 1 || C < 1 || H < 1 || W < 1 || Th < 1 || Tw < 1 || Hs < Th || Ws < Tw) return RGDA_ERR_ARG;
    if ((views != 1 && views != 8) || (views == 8 && Th != Tw)) return RGDA_ERR_ARG;
    const long long planes = (long long)K * views * C;
    if (planes > 0x7fffffffLL || (long long)Th * Tw > (1LL << 30)) return RGDA_ERR_ARG;
    const bool vec = Tw % 4 == 0 && (uintptr_t)out % 16 == 0;
    const dim3 grid(grid_of((long long)Th * Tw / (vec ? 4 : 1), 1024), (unsigned)(planes > 65535 ? 65535 : planes));
    auto kernel = vec ? window_gather_scaled_kernel<4> : window_gather_scaled_kernel<1>;
    kernel<<<grid, WIN_THREADS, 0, to_stream(stream)>>>(src_f32, src_u8, lut, windows, (int)planes, views, n, C, H, W, Hs, Ws,
                                                        Th, Tw, ac_scale(H, Hs), ac_scale(W, Ws), out, flag);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_scale_merge(const float* full_s, const float* count_s, int n, int C, int Hs, int Ws, int H, int W,
                                float* acc, float* cnt, rgda_stream_t stream) {
    if (!full_s || !count_s || !acc || !cnt || n < 1 || C < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    scale_merge_kernel<<<grid_of((long long)n * H * W, 65535), WIN_THREADS, 0, to_stream(stream)>>>(
        full_s, count_s, n, C, Hs, Ws, H, W, ac_scale(Hs, H), ac_scale(Ws, W), acc, cnt);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_window_scatter(const float* pred, const int32_t* windows, int K, int views, int n, int C, int H, int W,
                                   int Th, int Tw, int row0, int rows, float* full, float* count, int* flag,
                                   rgda_stream_t stream) {
    if (!pred || !windows || !full || !count) return RGDA_ERR_ARG;
    if (K < 1 || K > WIN_MAX_K || n < 1 || C < 1 || Th < 1 || Tw < 1 || H < Th || W < Tw) return RGDA_ERR_ARG;
    if ((views != 1 && views != 8) || (views == 8 && Th != Tw)) return RGDA_ERR_ARG;
    if ((long long)n * H > 0x7fffffffLL || row0 < 0 || rows < 1 || (long long)row0 + rows > (long long)n * H) return RGDA_ERR_ARG;
    const float scale = 1.0f / (float)views;
    window_scatter_kernel<<<grid_of((long long)rows * W, 65535), WIN_THREADS, 0, to_stream(stream)>>>(
        pred, windows, K, views, n, C, H, W, Th, Tw, row0, rows, scale, full, count, flag);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_window_finish(float* full, const float* count, int n, int C, int H, int W, uint8_t* labels_u8,
                                  int64_t* labels_i64, const int64_t* y_true, int64_t* cm, int* flag, rgda_stream_t stream) {
    if (!full || !count || n < 1 || C < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    if (labels_u8 && C > 256) return RGDA_ERR_ARG;
    if ((!y_true) != (!cm) || (cm && (!flag || C > 64))) return RGDA_ERR_ARG;
    const long long HW = (long long)H * W, total = (long long)n * HW;
    // each workgroup counts < 2^32 pixels into its 32-bit LDS cells
    const int grid = grid_of(total, cm ? 1024 : 65535);
    window_finish_kernel<<<grid, WIN_THREADS, cm ? (size_t)C * C * 4 : 0, to_stream(stream)>>>(
        full, count, C, HW, total, labels_u8, labels_i64, y_true, (unsigned long long*)cm, flag);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
