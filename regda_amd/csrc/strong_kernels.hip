// Strong (photometric) augmentation of the student's tile: colour jitter and Gaussian blur of normalised tiles, image by
// image from a device table (include/rgda_hip.h: rgda_strong_augment carries the contract).  Three launches: the per-image
// constants (switches, radius, hue matrix and taps, built ONCE per image, and the cleared sum), the image means of the grey
// value after brightness (64-bit fixed point, order-independent), the transform (a 32 x 32 tile + halo of all three
// channels in LDS, the pointwise steps on the way in, both blur passes in LDS).
// rgda_strong_write_table carries the host's table to the device in its launch arguments.
#include "common.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int SA_S = 32;                                // output tile edge
constexpr int SA_THREADS = 256;                         // S rows x S/4 quads in the store phase
constexpr int SA_RMAX = RGDA_STRONG_MAX_RADIUS;
constexpr int SA_LW = SA_S + 2 * SA_RMAX;               // 56: the staged window's edge at the largest radius
// LDS: window 3 x 56 x 56 floats (37632 B) + horizontal pass 3 x 56 x 32 floats (21504 B) = 59136 B, two workgroups per
// CU.  Rows of 56 and 32 dwords: the lanes of a wave read consecutive dwords of a row, which the banks serve in full.
constexpr int SA_IN = 3 * SA_LW * SA_LW;
constexpr int SA_HP = 3 * SA_LW * SA_S;
constexpr int SA_FRAC = 24;                             // a grey value is summed as round(g * 2^24)
constexpr int SA_MEAN_THREADS = 256;
constexpr int SA_MEAN_MAX_BPI = 128;                    // workgroups per image at most; larger images walk block-stride

struct Norm {
    float mean[3], std[3];
};

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float grey(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }
__device__ __forceinline__ float denorm(float v, float mean, float std) { return (v * std + mean) / 255.f; }

// flags of row n as the kernels read them; anything but 0..3 reads as 0 (a copy)
__device__ __forceinline__ int row_flags(const float* __restrict__ row) {
    const float f = row[5];
    return (f == 1.f) ? 1 : (f == 2.f) ? 2 : (f == 3.f) ? 3 : 0;
}
// the blur radius of a row, or -1 where the row asks for a blur this library does not serve
__device__ __forceinline__ int row_radius(const float* __restrict__ row, int H, int W) {
    const float sigma = row[4];
    if (!(sigma > 0.f && sigma <= 4.f)) return -1;
    const int R = (int)ceilf(3.f * sigma);
    return (R >= 1 && R <= SA_RMAX && R < H && R < W) ? R : -1;
}

// What the two passes need of image n, in the call's workspace: 128 bytes per image
struct ImgPar {
    unsigned long long sum;                     // of round(grey * 2^24) over the image (strong_mean_kernel)
    int flags, R;                               // the switches as served, the blur radius (0 without blur)
    float M[9];                                 // the hue matrix
    float tap[SA_RMAX + 1];                     // tap[d], d = 0..R
    float pad[6];
};
static_assert(sizeof(ImgPar) == 128, "ImgPar is 128 bytes");

// one thread per image: the constants in fp64, each rounded once; a row whose blur is not served becomes a copy and sets
// the flag (every writer stores 1)
__global__ void __launch_bounds__(64) strong_setup_kernel(const float* __restrict__ table, ImgPar* __restrict__ par, int N, int H,
                                                          int W, int* __restrict__ flag) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const float* row = table + (long long)n * RGDA_STRONG_TABLE_COLS;
    ImgPar p = {};
    p.flags = row_flags(row);
    if (p.flags & 2) {
        p.R = row_radius(row, H, W);
        if (p.R < 0) {
            if (flag) *flag = 1;
            p.flags = 0;
            p.R = 0;
        }
    }
    if (p.flags & 1) {
        // the header's T (RGB -> YIQ) and its inverse (adjugate / determinant)
        const double T[3][3] = {{0.299, 0.587, 0.114}, {0.596, -0.274, -0.322}, {0.211, -0.523, 0.312}};
        double Ti[3][3];
        const double det = T[0][0] * (T[1][1] * T[2][2] - T[1][2] * T[2][1]) - T[0][1] * (T[1][0] * T[2][2] - T[1][2] * T[2][0]) +
                           T[0][2] * (T[1][0] * T[2][1] - T[1][1] * T[2][0]);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
                Ti[i][j] = (T[r0][c0] * T[r1][c1] - T[r0][c1] * T[r1][c0]) / det;
            }
        const double th = (double)row[3], c = cos(th), s = sin(th);
        const double Rm[3][3] = {{1.0, 0.0, 0.0}, {0.0, c, -s}, {0.0, s, c}};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double acc = 0.0;
                for (int k = 0; k < 3; ++k)
                    for (int l = 0; l < 3; ++l) acc += Ti[i][k] * Rm[k][l] * T[l][j];
                p.M[3 * i + j] = (float)acc;
            }
    }
    if (p.R) {
        const double sigma = (double)row[4];
        double w[SA_RMAX + 1], norm = 1.0;
        w[0] = 1.0;
        for (int d = 1; d <= p.R; ++d) {
            w[d] = exp(-(double)(d * d) / (2.0 * sigma * sigma));
            norm += 2.0 * w[d];
        }
        for (int d = 0; d <= p.R; ++d) p.tap[d] = (float)(w[d] / norm);
    }
    par[n] = p;
}

// grid (workgroups per image, N): sum over this workgroup's pixels of round(grey(clamp(u * fb)) * 2^24), integers from the
// first add on, so the total does not depend on the order of anything
__global__ void __launch_bounds__(SA_MEAN_THREADS) strong_mean_kernel(const float* __restrict__ img,
                                                                      const float* __restrict__ table,
                                                                      ImgPar* __restrict__ par, long long HW, Norm nm) {
    __shared__ unsigned long long part[SA_MEAN_THREADS / 64];
    const int n = blockIdx.y;
    const float* row = table + (long long)n * RGDA_STRONG_TABLE_COLS;
    if (!(par[n].flags & 1)) return;
    const float fb = row[0];
    const float* p = img + (long long)n * 3 * HW;
    unsigned long long acc = 0;
    for (long long i = (long long)blockIdx.x * SA_MEAN_THREADS + threadIdx.x; i < HW;
         i += (long long)gridDim.x * SA_MEAN_THREADS) {
        const float r = clamp01(denorm(p[i], nm.mean[0], nm.std[0]) * fb);
        const float g = clamp01(denorm(p[i + HW], nm.mean[1], nm.std[1]) * fb);
        const float b = clamp01(denorm(p[i + 2 * HW], nm.mean[2], nm.std[2]) * fb);
        acc += (unsigned long long)__float2int_rn(clamp01(grey(r, g, b)) * (float)(1 << SA_FRAC));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
#pragma unroll
        for (int w = 0; w < SA_MEAN_THREADS / 64; ++w) all += part[w];
        atomicAdd(&par[n].sum, all);
    }
}

// mirror without repeating the edge: -1 -> 1, L -> L - 2; then cut to [0, L) so that no table row can leave the image
__device__ __forceinline__ int reflect(int i, int L) {
    if (i < 0) i = -i;
    if (i >= L) i = 2 * (L - 1) - i;
    return min(max(i, 0), L - 1);
}

// grid (tiles, N): one workgroup writes the tile [Y0, Y0 + th) x [X0, X0 + tw) of the three channels of image n
__global__ void __launch_bounds__(SA_THREADS) strong_augment_kernel(const float* __restrict__ img_in, float* __restrict__ img_out,
                                                                    const float* __restrict__ table,
                                                                    const ImgPar* __restrict__ par, int H, int W, Norm nm,
                                                                    int vec_out, int vec_copy) {
    __shared__ float s_in[SA_IN];               // [3][lh][lw] at row stride SA_LW: the window after steps 1 to 4
    __shared__ float s_hp[SA_HP];               // [3][lh][tw] at row stride SA_S: after the horizontal pass
    __shared__ float s_tap[SA_RMAX + 1];
    const int n = blockIdx.y, tid = threadIdx.x;
    const float* row = table + (long long)n * RGDA_STRONG_TABLE_COLS;
    const ImgPar* ip = par + n;                 // the same for every thread of the workgroup
    const int flags = ip->flags;
    const int R = min(max(ip->R, 0), SA_RMAX);
    const int tiles_x = (W + SA_S - 1) / SA_S;
    const int Y0 = (blockIdx.x / tiles_x) * SA_S, X0 = (blockIdx.x % tiles_x) * SA_S;
    const int th = min(SA_S, H - Y0), tw = min(SA_S, W - X0);
    const long long plane = (long long)H * W;
    const float* src = img_in + (long long)n * 3 * plane;
    float* dst = img_out + (long long)n * 3 * plane;
    const int a = tid / (SA_S / 4), b = (tid % (SA_S / 4)) * 4;
    const bool active = a < th && b < tw;
    const int cnt = min(4, tw - b);
    const long long o = (long long)(Y0 + a) * W + X0 + b;

    if (!flags) {                                               // both bits clear: a copy, no arithmetic
        if (!active) return;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if (vec_copy && cnt == 4) {
                *reinterpret_cast<f32x4*>(dst + ch * plane + o) = *reinterpret_cast<const f32x4*>(src + ch * plane + o);
            } else {
                for (int e = 0; e < cnt; ++e) dst[ch * plane + o + e] = src[ch * plane + o + e];
            }
        }
        return;
    }

    const bool jitter = flags & 1;
    const float fb = row[0], fc = row[1], fs = row[2];
    if (tid <= R) s_tap[tid] = ip->tap[tid];    // (read after the barrier behind the window load)
    float m = 0.f;
    if (jitter) m = (float)((double)ip->sum * (1.0 / (double)(1 << SA_FRAC)) / (double)plane);
    float M[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = ip->M[k];

    // the window [Y0 - R, Y0 + th + R) x [X0 - R, X0 + tw + R), reflected into the image, steps 1 to 4 on the way in:
    // a lane per column (lw <= 56 of the wave's 64), a wave per row
    const int lh = th + 2 * R, lw = tw + 2 * R;
    const int lx = tid & 63;
    if (lx < lw) {
        const int sx = reflect(X0 - R + lx, W);
        for (int ly = tid >> 6; ly < lh; ly += SA_THREADS / 64) {
            const long long p = (long long)reflect(Y0 - R + ly, H) * W + sx;
            float r = denorm(src[p], nm.mean[0], nm.std[0]);
            float g = denorm(src[p + plane], nm.mean[1], nm.std[1]);
            float bl = denorm(src[p + 2 * plane], nm.mean[2], nm.std[2]);
            if (jitter) {
                r = clamp01(r * fb); g = clamp01(g * fb); bl = clamp01(bl * fb);
                r = clamp01((r - m) * fc + m); g = clamp01((g - m) * fc + m); bl = clamp01((bl - m) * fc + m);
                const float y = grey(r, g, bl);
                r = clamp01((r - y) * fs + y); g = clamp01((g - y) * fs + y); bl = clamp01((bl - y) * fs + y);
                const float r2 = clamp01(M[0] * r + M[1] * g + M[2] * bl);
                const float g2 = clamp01(M[3] * r + M[4] * g + M[5] * bl);
                const float b2 = clamp01(M[6] * r + M[7] * g + M[8] * bl);
                r = r2; g = g2; bl = b2;
            }
            const int q = ly * SA_LW + lx;
            s_in[q] = r;
            s_in[SA_LW * SA_LW + q] = g;
            s_in[2 * SA_LW * SA_LW + q] = bl;
        }
    }
    __syncthreads();

    if (R) {
        // horizontal pass: every row of the window, the tile's columns -- a lane per column, eight rows at a time
        const int x = tid & (SA_S - 1);
        if (x < tw) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                for (int ly = tid / SA_S; ly < lh; ly += SA_THREADS / SA_S) {
                    const float* in = s_in + ch * SA_LW * SA_LW + ly * SA_LW + x;      // in[R + d] is the tap at distance d
                    float acc = 0.f;
                    for (int d = -R; d <= R; ++d) acc += s_tap[d < 0 ? -d : d] * in[R + d];
                    s_hp[(ch * SA_LW + ly) * SA_S + x] = acc;
                }
        }
        __syncthreads();
    }
    if (!active) return;
    // vertical pass, step 6 and the store: this thread's quad of each channel
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (R) {
            for (int d = -R; d <= R; ++d) {
                const float t = s_tap[d < 0 ? -d : d];
                const float* hp = s_hp + (ch * SA_LW + a + R + d) * SA_S + b;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < cnt) v[e] += t * hp[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) v[e] = s_in[ch * SA_LW * SA_LW + a * SA_LW + b + e];
        }
        const float mean = nm.mean[ch], std = nm.std[ch];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (255.f * v[e] - mean) / std;
        if (vec_out && cnt == 4) {
            *reinterpret_cast<f32x4*>(dst + ch * plane + o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            for (int e = 0; e < cnt; ++e) dst[ch * plane + o + e] = v[e];
        }
    }
}

// ---- rgda_strong_write_table: the table travels in the launch's own argument block
struct StrongDraw {
    float rows[RGDA_MIX_WRITE_MAX_IMAGES * RGDA_STRONG_TABLE_COLS];
};
__global__ void __launch_bounds__(128) strong_write_table_kernel(float* __restrict__ table, StrongDraw d, int n) {
    for (int i = threadIdx.x; i < n * RGDA_STRONG_TABLE_COLS; i += 128) table[i] = d.rows[i];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t rgda_strong_augment_workspace(int N) { return N > 0 ? (size_t)N * sizeof(ImgPar) : 0; }

extern "C" int rgda_strong_augment(const float* img_in, float* img_out, const float* table, void* ws, int N, int H, int W,
                                   float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b,
                                   int* flag, rgda_stream_t stream) {
    if (!img_in || !img_out || !ws || ((uintptr_t)ws & 7) || !table || !aligned16(table)) return RGDA_ERR_ARG;
    if (N < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    if (!(std_r > 0.f) || !(std_g > 0.f) || !(std_b > 0.f)) return RGDA_ERR_ARG;
    const long long HW = (long long)H * W;
    if (N > 65535 || HW >= (1ll << 31)) return RGDA_ERR_UNSUPPORTED;        // N is the grid's y extent
    const uintptr_t bytes = (uintptr_t)N * 3 * HW * sizeof(float), pi = (uintptr_t)img_in, po = (uintptr_t)img_out;
    if (pi < po + bytes && po < pi + bytes) return RGDA_ERR_ARG;            // out of place only
    const Norm nm = {{mean_r, mean_g, mean_b}, {std_r, std_g, std_b}};
    ImgPar* par = (ImgPar*)ws;
    const bool vec_out = W % 4 == 0 && aligned16(img_out);
    const bool vec_copy = vec_out && aligned16(img_in);
    strong_setup_kernel<<<(N + 63) / 64, 64, 0, to_stream(stream)>>>(table, par, N, H, W, flag);
    RGDA_CHECK_LAUNCH();
    const long long want = (HW + SA_MEAN_THREADS * 8 - 1) / (SA_MEAN_THREADS * 8);
    const int bpi = want < SA_MEAN_MAX_BPI ? (int)want : SA_MEAN_MAX_BPI;
    strong_mean_kernel<<<dim3(bpi, N), SA_MEAN_THREADS, 0, to_stream(stream)>>>(img_in, table, par, HW, nm);
    RGDA_CHECK_LAUNCH();
    const long long tiles = (long long)((H + SA_S - 1) / SA_S) * ((W + SA_S - 1) / SA_S);
    strong_augment_kernel<<<dim3((unsigned)tiles, (unsigned)N), SA_THREADS, 0, to_stream(stream)>>>(
        img_in, img_out, table, par, H, W, nm, vec_out ? 1 : 0, vec_copy ? 1 : 0);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_strong_write_table(float* table, const float* host, int N, int H, int W, rgda_stream_t stream) {
    if (!table || !aligned16(table) || !host || N < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    if (N > RGDA_MIX_WRITE_MAX_IMAGES) return RGDA_ERR_UNSUPPORTED;
    StrongDraw d = {};
    for (int n = 0; n < N; ++n) {
        const float* r = host + n * RGDA_STRONG_TABLE_COLS;
        for (int k = 0; k < 5; ++k)
            if (!isfinite(r[k])) return RGDA_ERR_ARG;
        if (r[0] < 0.f || r[1] < 0.f || r[2] < 0.f) return RGDA_ERR_ARG;
        if (r[5] != 0.f && r[5] != 1.f && r[5] != 2.f && r[5] != 3.f) return RGDA_ERR_ARG;
        if (r[5] >= 2.f) {
            if (!(r[4] > 0.f && r[4] <= 4.f)) return RGDA_ERR_UNSUPPORTED;
            const int R = (int)ceilf(3.f * r[4]);
            if (R >= H || R >= W) return RGDA_ERR_UNSUPPORTED;
        }
        memcpy(d.rows + n * RGDA_STRONG_TABLE_COLS, r, 6 * sizeof(float));     // columns 6 and 7 stay 0
    }
    strong_write_table_kernel<<<1, 128, 0, to_stream(stream)>>>(table, d, N);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
