// Fourier style transfer of the source tile (include/rgda_hip.h: rgda_fourier_style carries the contract): the amplitudes
// of the (2b + 1)^2 lowest frequencies of a source image are replaced with its partner target image's, the phase is kept.
// No full FFT: the change is a low-rank update, computed as a pruned separable DFT in six launches --
//   setup      the rows as served (Head) and the twiddle tables tw_x[kx][x], tw_y[ky][y] (fp64 sincospi, rounded once)
//   rows       R[plane][kx][y] = sum_x S[y][x] e^{-2 pi i kx x / W}          (source and needed target planes)
//   columns    F[plane][ky][kx] = sum_y R[kx][y] e^{-2 pi i ky y / H}         (+ky and -ky from the same loads)
//   coef       D = (|F_T| - |F_S|) F_S / |F_S|, times (kx ? 2 : 1) / HW, written over F_S
//   syn cols   G[plane][kx][y] = sum_ky D[ky][kx] e^{+2 pi i ky y / H}
//   syn rows   out = ((S + sum_kx Re(G[kx][y] e^{+2 pi i kx x / W})) - mean) / std, or the copy of an off row
// Every sum has a fixed order: a lane's own terms in sequence, then the xor butterfly of the wave (analysis), or two / four
// interleaved partial sums in sequence (synthesis).  No atomics.
// rgda_fourier_style_write_table carries the host's table to the device in its launch arguments.
#include "common.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int FS_BMAX = RGDA_STYLE_MAX_B;
constexpr int FS_IMGS = RGDA_STYLE_MAX_IMAGES;
constexpr int FS_MAX_SIDE = 4096;           // FS_RA rows of W floats are staged in LDS: 128 KB at the widest tile
constexpr int FS_THREADS = 256;
constexpr int FS_RA = 8;                    // rows per workgroup in the row analysis: a twiddle load serves eight rows
constexpr int FS_RB = 4;                    // rows per workgroup in the row synthesis

struct Norm2 {
    float mean_s[3], std_s[3], mean_t[3], std_t[3];
};

// The rows as the kernels serve them, at the base of the workspace: 256 bytes
struct Head {
    int src_b[FS_IMGS];                     // the half-width of source image n, -1: copy it
    int src_p[FS_IMGS];                     // its partner
    int tgt_b[FS_IMGS];                     // the largest half-width any source image needs of target image m, -1: none
    int pad[FS_IMGS];
};
static_assert(sizeof(Head) == 256, "Head is 256 bytes");

// the workspace: Head, tw_x [KX][W], tw_y [KX][H], R [(N + M) 3][KX][H], F [(N + M) 3][KY][KX], G [N 3][KX][H], float2 each
struct Layout {
    int Bc, KX, KY;                         // the largest b the tile admits, Bc + 1, 2 Bc + 1
    size_t tw_x, tw_y, R, F, G, total;
};
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
Layout layout(int N, int M, int H, int W) {
    Layout l;
    const int fit = ((H < W ? H : W) - 1) / 2;
    l.Bc = fit < FS_BMAX ? fit : FS_BMAX;
    l.KX = l.Bc + 1;
    l.KY = 2 * l.Bc + 1;
    const size_t c = sizeof(float2);
    l.tw_x = sizeof(Head);
    l.tw_y = up16(l.tw_x + (size_t)l.KX * W * c);
    l.R = up16(l.tw_y + (size_t)l.KX * H * c);
    l.F = up16(l.R + (size_t)(N + M) * 3 * l.KX * H * c);
    l.G = up16(l.F + (size_t)(N + M) * 3 * l.KY * l.KX * c);
    l.total = up16(l.G + (size_t)N * 3 * l.KX * H * c);
    return l;
}

// a row as served: partner in [0, M), 0 <= b <= Bc (the cap and the tile's fit), on 0 or 1
__device__ __forceinline__ bool row_ok(const int* __restrict__ row, int M, int Bc) {
    return row[0] >= 0 && row[0] < M && row[1] >= 0 && row[1] <= Bc && (row[2] == 0 || row[2] == 1);
}

// grid over the (Bc + 1)(W + H) twiddles; workgroup 0 also writes the Head (a bad row becomes a copy and sets the flag)
__global__ void __launch_bounds__(FS_THREADS) fourier_setup_kernel(const int* __restrict__ table, Head* __restrict__ head,
                                                                   float2* __restrict__ twx, float2* __restrict__ twy, int N,
                                                                   int M, int H, int W, int Bc, int* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * FS_THREADS + threadIdx.x;
    const long long nx = (long long)(Bc + 1) * W, ny = (long long)(Bc + 1) * H;
    if (i < nx + ny) {
        const bool isx = i < nx;
        const long long j = isx ? i : i - nx;
        const int L = isx ? W : H;
        const int k = (int)(j / L), x = (int)(j % L);
        const int p = (int)(((long long)k * x) % L);            // the phase index, reduced in integers
        double s, c;
        sincospi(2.0 * (double)p / (double)L, &s, &c);
        (isx ? twx : twy)[j] = make_float2((float)c, (float)s);
    }
    if (blockIdx.x == 0 && threadIdx.x < FS_IMGS) {
        const int t = threadIdx.x;
        int sb = -1, sp = 0, tb = -1;
        if (t < N) {
            const int* row = table + t * RGDA_STYLE_TABLE_COLS;
            if (!row_ok(row, M, Bc)) {
                if (flag) *flag = 1;
            } else if (row[2] == 1) {
                sb = row[1];
                sp = row[0];
            }
        }
        if (t < M)
            for (int n = 0; n < N; ++n) {
                const int* row = table + n * RGDA_STYLE_TABLE_COLS;
                if (row_ok(row, M, Bc) && row[2] == 1 && row[0] == t && row[1] > tb) tb = row[1];
            }
        head->src_b[t] = sb;
        head->src_p[t] = sp;
        head->tgt_b[t] = tb;
        head->pad[t] = 0;
    }
}

// grid (row groups, (N + M) 3): FS_RA rows of one plane on the raw grey scale in LDS; a wave per kx, the lanes over x
__global__ void __launch_bounds__(FS_THREADS) fourier_rows_kernel(const float* __restrict__ img_s, const float* __restrict__ img_t,
                                                                  const Head* __restrict__ head, const float2* __restrict__ twx,
                                                                  float2* __restrict__ R, int N, int H, int W, int KX, Norm2 nm) {
    extern __shared__ float s_row[];            // [FS_RA][W]
    const int plane = blockIdx.y, img = plane / 3, ch = plane % 3, tid = threadIdx.x;
    const bool src = img < N;
    const int bb = src ? head->src_b[img] : head->tgt_b[img - N];
    if (bb < 0) return;                         // the same for every thread of the workgroup
    const size_t hw = (size_t)H * W;
    const float* p = (src ? img_s + (size_t)img * 3 * hw : img_t + (size_t)(img - N) * 3 * hw) + (size_t)ch * hw;
    const float mean = src ? nm.mean_s[ch] : nm.mean_t[ch], std = src ? nm.std_s[ch] : nm.std_t[ch];
    const int y0 = blockIdx.x * FS_RA, rows = min(FS_RA, H - y0);
    for (int i = tid; i < FS_RA * W; i += FS_THREADS)
        s_row[i] = i < rows * W ? fmaf(p[(size_t)y0 * W + i], std, mean) : 0.f;
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int kx = wave; kx <= bb; kx += FS_THREADS / 64) {
        const float2* t = twx + (size_t)kx * W;
        float re[FS_RA] = {}, im[FS_RA] = {};
        for (int x = lane; x < W; x += 64) {
            const float2 w = t[x];
#pragma unroll
            for (int r = 0; r < FS_RA; ++r) {
                const float v = s_row[r * W + x];
                re[r] = fmaf(v, w.x, re[r]);
                im[r] = fmaf(-v, w.y, im[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < FS_RA; ++r) {
            const float a = wave_sum(re[r]), b = wave_sum(im[r]);
            if (lane == r && r < rows) R[((size_t)plane * KX + kx) * H + y0 + r] = make_float2(a, b);
        }
    }
}

// grid (KX, (N + M) 3): a workgroup per kx, its waves over ky = 0..b, the lanes over y; -ky comes from the same loads
__global__ void __launch_bounds__(FS_THREADS) fourier_cols_kernel(const Head* __restrict__ head, const float2* __restrict__ twy,
                                                                  const float2* __restrict__ R, float2* __restrict__ F, int N,
                                                                  int H, int Bc) {
    const int KX = Bc + 1, KY = 2 * Bc + 1;
    const int plane = blockIdx.y, img = plane / 3, kx = blockIdx.x, lane = threadIdx.x & 63;
    const int bb = img < N ? head->src_b[img] : head->tgt_b[img - N];
    if (kx > bb) return;                        // bb < 0 leaves here too; no barrier below
    const float2* r = R + ((size_t)plane * KX + kx) * H;
    for (int ky = threadIdx.x >> 6; ky <= bb; ky += FS_THREADS / 64) {
        const float2* t = twy + (size_t)ky * H;
        float pr = 0.f, pi = 0.f, mr = 0.f, mi = 0.f;
        for (int y = lane; y < H; y += 64) {
            const float2 a = r[y], w = t[y];
            pr = fmaf(a.y, w.y, fmaf(a.x, w.x, pr));            // a e^{-i theta}
            pi = fmaf(-a.x, w.y, fmaf(a.y, w.x, pi));
            mr = fmaf(-a.y, w.y, fmaf(a.x, w.x, mr));           // a e^{+i theta}
            mi = fmaf(a.x, w.y, fmaf(a.y, w.x, mi));
        }
        pr = wave_sum(pr); pi = wave_sum(pi); mr = wave_sum(mr); mi = wave_sum(mi);
        if (lane == 0) {
            F[((size_t)plane * KY + Bc + ky) * KX + kx] = make_float2(pr, pi);
            if (ky) F[((size_t)plane * KY + Bc - ky) * KX + kx] = make_float2(mr, mi);
        }
    }
}

// grid (bins / 256, N 3): D over F_S, scaled by (kx ? 2 : 1) / HW (the half spectrum stands for both halves)
__global__ void __launch_bounds__(FS_THREADS) fourier_coef_kernel(const Head* __restrict__ head, float2* __restrict__ F, int N,
                                                                  int Bc, float inv_hw) {
    const int KX = Bc + 1, KY = 2 * Bc + 1;
    const int plane = blockIdx.y, n = plane / 3, ch = plane % 3;
    const int bb = head->src_b[n];
    const int i = blockIdx.x * FS_THREADS + threadIdx.x;
    if (bb < 0 || i >= KY * KX) return;
    const int ky = i / KX - Bc, kx = i % KX;
    if (ky < -bb || ky > bb || kx > bb) return;
    const int m = head->src_p[n];
    float2* fs = F + (size_t)plane * KY * KX + i;
    const float2 s = *fs, t = F[(size_t)((N + m) * 3 + ch) * KY * KX + i];
    const float as = hypotf(s.x, s.y), at = hypotf(t.x, t.y);
    const float sc = kx ? 2.f * inv_hw : inv_hw;
    float2 d;
    if (as > 0.f) {
        const float g = (at - as) / as;
        d = make_float2(g * s.x * sc, g * s.y * sc);
    } else {
        d = make_float2(at * sc, 0.f);          // |F_S| = 0: the phase is 0
    }
    *fs = d;
}

// grid (H / 256, KX, N 3): a thread per (kx, y); +ky and -ky in pairs, four interleaved partial sums
__global__ void __launch_bounds__(FS_THREADS) fourier_syn_cols_kernel(const Head* __restrict__ head, const float2* __restrict__ twy,
                                                                      const float2* __restrict__ D, float2* __restrict__ G, int H,
                                                                      int Bc) {
    const int KX = Bc + 1, KY = 2 * Bc + 1;
    const int plane = blockIdx.z, kx = blockIdx.y, y = blockIdx.x * FS_THREADS + threadIdx.x;
    const int bb = head->src_b[plane / 3];
    if (kx > bb || y >= H) return;
    const float2* d = D + (size_t)plane * KY * KX + kx;      // d[ky * KX], ky + Bc the row
    const float2 d0 = d[(size_t)Bc * KX];
    float re[4] = {d0.x, 0.f, 0.f, 0.f}, im[4] = {d0.y, 0.f, 0.f, 0.f};
    for (int k0 = 1; k0 <= bb; k0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ky = k0 + u;
            if (ky <= bb) {
                const float2 w = twy[(size_t)ky * H + y], p = d[(size_t)(Bc + ky) * KX], q = d[(size_t)(Bc - ky) * KX];
                re[u] = fmaf(-(p.y - q.y), w.y, fmaf(p.x + q.x, w.x, re[u]));    // p e^{+i theta} + q e^{-i theta}
                im[u] = fmaf(p.x - q.x, w.y, fmaf(p.y + q.y, w.x, im[u]));
            }
        }
    }
    G[((size_t)plane * KX + kx) * H + y] = make_float2((re[0] + re[1]) + (re[2] + re[3]), (im[0] + im[1]) + (im[2] + im[3]));
}

// grid (row groups, N 3): FS_RB rows of one source plane -- the correction added, normalised; or the copy of an off row
__global__ void __launch_bounds__(FS_THREADS) fourier_syn_rows_kernel(const float* __restrict__ img_s, float* __restrict__ out,
                                                                      const Head* __restrict__ head, const float2* __restrict__ twx,
                                                                      const float2* __restrict__ G, int H, int W, int KX, Norm2 nm,
                                                                      int vec) {
    __shared__ float2 s_g[(FS_BMAX + 1) * FS_RB];
    const int plane = blockIdx.y, ch = plane % 3, tid = threadIdx.x;
    const int bb = min(head->src_b[plane / 3], KX - 1);
    const int y0 = blockIdx.x * FS_RB, rows = min(FS_RB, H - y0);
    const size_t base = (size_t)plane * H * W + (size_t)y0 * W;
    const float* src = img_s + base;
    float* dst = out + base;
    const int cnt = rows * W;                   // the rows are contiguous
    if (bb < 0) {                               // a copy, no arithmetic
        if (vec) {
            for (int i = tid * 4; i < cnt; i += FS_THREADS * 4)
                *reinterpret_cast<f32x4*>(dst + i) = *reinterpret_cast<const f32x4*>(src + i);
        } else {
            for (int i = tid; i < cnt; i += FS_THREADS) dst[i] = src[i];
        }
        return;
    }
    for (int i = tid; i < (bb + 1) * FS_RB; i += FS_THREADS) {
        const int kx = i / FS_RB, r = i % FS_RB;
        s_g[i] = r < rows ? G[((size_t)plane * KX + kx) * H + y0 + r] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const float mean = nm.mean_s[ch], std = nm.std_s[ch];
    for (int x = tid; x < W; x += FS_THREADS) {
        float a0[FS_RB] = {}, a1[FS_RB] = {};
        for (int kx = 0; kx <= bb; kx += 2) {
            const float2 w = twx[(size_t)kx * W + x];
#pragma unroll
            for (int r = 0; r < FS_RB; ++r) {
                const float2 g = s_g[kx * FS_RB + r];
                a0[r] = fmaf(-g.y, w.y, fmaf(g.x, w.x, a0[r]));        // Re(g e^{+i theta})
            }
            if (kx + 1 <= bb) {
                const float2 v = twx[(size_t)(kx + 1) * W + x];
#pragma unroll
                for (int r = 0; r < FS_RB; ++r) {
                    const float2 g = s_g[(kx + 1) * FS_RB + r];
                    a1[r] = fmaf(-g.y, v.y, fmaf(g.x, v.x, a1[r]));
                }
            }
        }
#pragma unroll
        for (int r = 0; r < FS_RB; ++r)
            if (r < rows) {
                const float s = fmaf(src[(size_t)r * W + x], std, mean);
                dst[(size_t)r * W + x] = ((s + (a0[r] + a1[r])) - mean) / std;
            }
    }
}

// ---- rgda_fourier_style_write_table: the table travels in the launch's own argument block
struct StyleDraw {
    int rows[FS_IMGS * RGDA_STYLE_TABLE_COLS];
};
__global__ void __launch_bounds__(64) fourier_write_table_kernel(int* __restrict__ table, StyleDraw d, int n) {
    for (int i = threadIdx.x; i < n * RGDA_STYLE_TABLE_COLS; i += 64) table[i] = d.rows[i];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" size_t rgda_fourier_style_workspace(int N, int M, int H, int W) {
    if (N < 1 || M < 1 || H < 1 || W < 1 || N > FS_IMGS || M > FS_IMGS || H > FS_MAX_SIDE || W > FS_MAX_SIDE) return 0;
    return layout(N, M, H, W).total;
}

extern "C" int rgda_fourier_style(const float* img_s, const float* img_t, float* out, const int32_t* table, void* ws, int N,
                                  int M, int H, int W, float mean_sr, float mean_sg, float mean_sb, float std_sr, float std_sg,
                                  float std_sb, float mean_tr, float mean_tg, float mean_tb, float std_tr, float std_tg,
                                  float std_tb, int* flag, rgda_stream_t stream) {
    if (!img_s || !img_t || !out || !ws || !aligned16(ws) || !table || !aligned16(table)) return RGDA_ERR_ARG;
    if (N < 1 || M < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    const Norm2 nm = {{mean_sr, mean_sg, mean_sb}, {std_sr, std_sg, std_sb}, {mean_tr, mean_tg, mean_tb}, {std_tr, std_tg, std_tb}};
    for (int c = 0; c < 3; ++c) {
        if (!(nm.std_s[c] > 0.f) || !(nm.std_t[c] > 0.f) || !isfinite(nm.std_s[c]) || !isfinite(nm.std_t[c])) return RGDA_ERR_ARG;
        if (!isfinite(nm.mean_s[c]) || !isfinite(nm.mean_t[c])) return RGDA_ERR_ARG;
    }
    if (N > FS_IMGS || M > FS_IMGS || H > FS_MAX_SIDE || W > FS_MAX_SIDE) return RGDA_ERR_UNSUPPORTED;
    const size_t plane = (size_t)3 * H * W * sizeof(float);
    if (overlap(out, N * plane, img_s, N * plane) || overlap(out, N * plane, img_t, M * plane)) return RGDA_ERR_ARG;
    const Layout l = layout(N, M, H, W);
    char* base = (char*)ws;
    Head* head = (Head*)base;
    float2* twx = (float2*)(base + l.tw_x);
    float2* twy = (float2*)(base + l.tw_y);
    float2* R = (float2*)(base + l.R);
    float2* F = (float2*)(base + l.F);
    float2* G = (float2*)(base + l.G);
    hipStream_t s = to_stream(stream);
    const int planes = (N + M) * 3;
    const size_t lds = (size_t)FS_RA * W * sizeof(float);
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)fourier_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds) != hipSuccess)
        return RGDA_ERR_LAUNCH;
    fourier_setup_kernel<<<cdiv((long long)l.KX * (W + H), FS_THREADS), FS_THREADS, 0, s>>>(table, head, twx, twy, N, M, H, W, l.Bc,
                                                                                           flag);
    RGDA_CHECK_LAUNCH();
    fourier_rows_kernel<<<dim3(cdiv(H, FS_RA), planes), FS_THREADS, lds, s>>>(img_s, img_t, head, twx, R, N, H, W, l.KX, nm);
    RGDA_CHECK_LAUNCH();
    fourier_cols_kernel<<<dim3(l.KX, planes), FS_THREADS, 0, s>>>(head, twy, R, F, N, H, l.Bc);
    RGDA_CHECK_LAUNCH();
    fourier_coef_kernel<<<dim3(cdiv(l.KY * l.KX, FS_THREADS), N * 3), FS_THREADS, 0, s>>>(head, F, N, l.Bc,
                                                                                          (float)(1.0 / ((double)H * W)));
    RGDA_CHECK_LAUNCH();
    fourier_syn_cols_kernel<<<dim3(cdiv(H, FS_THREADS), l.KX, N * 3), FS_THREADS, 0, s>>>(head, twy, F, G, H, l.Bc);
    RGDA_CHECK_LAUNCH();
    const int vec = W % 4 == 0 && aligned16(img_s) && aligned16(out);
    fourier_syn_rows_kernel<<<dim3(cdiv(H, FS_RB), N * 3), FS_THREADS, 0, s>>>(img_s, out, head, twx, G, H, W, l.KX, nm, vec);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_fourier_style_write_table(int32_t* table, const int32_t* host, int N, int M, int H, int W,
                                              rgda_stream_t stream) {
    if (!table || !aligned16(table) || !host || N < 1 || M < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    if (N > FS_IMGS || M > FS_IMGS) return RGDA_ERR_UNSUPPORTED;
    StyleDraw d = {};
    const int side = H < W ? H : W;
    for (int n = 0; n < N; ++n) {
        const int32_t* r = host + n * RGDA_STYLE_TABLE_COLS;
        if (r[0] < 0 || r[0] >= M || r[1] < 0 || (r[2] != 0 && r[2] != 1)) return RGDA_ERR_ARG;
        if (r[1] > FS_BMAX || 2 * (long long)r[1] + 1 > side) return RGDA_ERR_UNSUPPORTED;
        memcpy(d.rows + n * RGDA_STYLE_TABLE_COLS, r, 3 * sizeof(int32_t));        // column 3 stays 0
    }
    fourier_write_table_kernel<<<1, 64, 0, to_stream(stream)>>>(table, d, N);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
