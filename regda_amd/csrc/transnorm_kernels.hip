// Transferable Normalization (regda/trans_norm.py:169-230, Wang et al., NeurIPS 2019): forward and backward of the layer,
// training and eval mode, deterministic (no floating-point atomics, every sum in a fixed order).  The definition, the
// arithmetic and the workspace layout are at rgda_transnorm_fwd / rgda_transnorm_bwd in include/rgda_hip.h.
//
// x f32, read in place: element (i, c, p) at x[i * ldb + c * ldc + p], p < s contiguous; samples [0, n_src) are the
// source half, [n_src, n) the target half.  y, g and dx have strides of their own.
//
// Two routes, chosen from s alone in tn_plane_route(): s >= TN_PLANE_MIN (16) takes the plane route, s < 16 the row route.
//   plane : a wavefront owns a run of 64 units of one plane (a unit: a float4 where s % 4 == 0 and every base and stride
//           is 16-byte aligned, else one float -- the scalar fallback, which also serves odd s); a workgroup's four
//           wavefronts take the runs of one (channel, domain) round-robin, K workgroups per (channel, domain) when
//           n / 2 * s is large.  Every wave-load is 1 KiB (256 B scalar) of one plane.
//   row   : lane = channel (64 channels per workgroup), the four wavefronts take samples round-robin and a lane walks its
//           channel's s values; for s = 1 (a 2-D input) a wave-load is 256 contiguous bytes of one sample's row.
// Both leave the same partial records, so the finalize stages are shared.
//
// Training forward, 3 launches, x read twice, y written once, nothing of the input's size in between:
//   stats    : per (channel, domain, k) a record (count, mean, M2).  A thread keeps SHIFTED sums about the first value it
//              reads (sum (x - x0), sum (x - x0)^2: no cancellation when |mean| >> std); threads, wavefronts and the K
//              records are merged pairwise by Chan's formula in double, in a fixed order      tn_stats_{plane,row}_kernel
//   finalize : ONE workgroup (the sum over the channels of prob needs all of them; a stage of its own instead of the last
//              workgroup to arrive: no device-scope fence or ticket in the streaming kernel).  Biased
//              variance -> rstd, unbiased -> running update (in place) and alpha; saved f32 [5][C]   tn_finalize_kernel
//   apply    : y = ((x - mean_d) * rstd_d * w + b) * (1 + alpha) in double from the fp32 constants, rounded once
//                                                                                             tn_apply_{plane,row}_kernel
// Eval forward, 2 launches: tn_finalize_eval_kernel (the saved block from the running vectors), apply.
// Backward, 3 launches, g and x read twice each, dx written once:
//   reduce   : per (channel, domain, k) sum g and sum g * xhat (thread sums in fp32, merged in double)
//                                                                                             tn_bwd_reduce_{plane,row}_kernel
//   finalize : the K records in order; dweight, dbias; per channel and domain the three coefficients of the apply pass
//                                                                                             tn_bwd_finalize_kernel
//   apply    : dx = A_d g - B_d - xhat D_d                                                    tn_bwd_apply_{plane,row}_kernel
// Eval backward: the apply launch alone (dx = g (1 + alpha) w rstd_t); reduce + finalize only when dweight / dbias are
// asked for.
#include <math.h>

#include "feat_rows.h"

namespace {

constexpr int TN_PLANE_MIN = 16;        // s >= 16: plane route
constexpr int TN_MAX_K = 64;            // workgroups per (channel, domain)

bool tn_plane_route(int s) { return s >= TN_PLANE_MIN; }

struct TnView {                          // an f32 map of n samples, C channels, s contiguous values per plane
    long long ldc, ldb;
};

struct TnGeom {
    int n, n_src, C, s;
    int K;                               // records per (channel, domain)
    int vec;                             // plane route: float4 units
    int units, runs;                     // plane route: units per plane, runs of 64 units per plane
};

struct Rec {                             // Chan's record
    double n, mean, m2;
};

// ---- shared arithmetic
static __device__ __forceinline__ Rec rec_merge(const Rec& a, const Rec& b) {       // a before b
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    Rec r;
    r.n = a.n + b.n;
    const double d = b.mean - a.mean, f = b.n / r.n;
    r.mean = a.mean + d * f;
    r.m2 = a.m2 + b.m2 + d * d * a.n * f;
    return r;
}
static __device__ __forceinline__ double shfl_down_d(double v, int o) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_down(lo, o, 64);
    hi = __shfl_down(hi, o, 64);
    return __hiloint2double(hi, lo);
}
// lane 0 of the wavefront gets the records of lanes 0 .. 63 merged as a tree: (l, l + 32), then 16, 8, 4, 2, 1
static __device__ __forceinline__ Rec wave_merge(Rec r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Rec b;
        b.n = shfl_down_d(r.n, o);
        b.mean = shfl_down_d(r.mean, o);
        b.m2 = shfl_down_d(r.m2, o);
        r = rec_merge(r, b);
    }
    return r;
}
static __device__ __forceinline__ double wave_sum_d(double v) {      // lane 0: the same tree
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_down_d(v, o);
    return v;
}
// a thread's shifted sums -> its record
struct Shifted {
    float x0, s1, s2;
    int n;
};
static __device__ __forceinline__ void shifted_add(Shifted& a, float x) {
    if (a.n == 0) a.x0 = x;
    const float d = x - a.x0;
    a.s1 += d;
    a.s2 += d * d;
    ++a.n;
}
static __device__ __forceinline__ Rec shifted_rec(const Shifted& a) {
    Rec r{0.0, 0.0, 0.0};
    if (a.n == 0) return r;
    r.n = (double)a.n;
    const double m = (double)a.s1 / r.n;
    r.mean = (double)a.x0 + m;
    r.m2 = fmax((double)a.s2 - (double)a.s1 * m, 0.0);
    return r;
}
// y of one value: double from the fp32 constants, each operation rounded once in the order of the definition (never
// contracted: the tests restate it operation by operation), one rounding to fp32
static __device__ __forceinline__ float tn_y(float x, float mean, float rstd, float w, float b, double a1) {
#pragma clang fp contract(off)
    const double xh = ((double)x - (double)mean) * (double)rstd;
    const double z = xh * (double)w + (double)b;
    return (float)(z * a1);
}
static __device__ __forceinline__ float tn_xhat(float x, float mean, float rstd) {
#pragma clang fp contract(off)
    return (x - mean) * rstd;
}

// ---- plane route: the runs of (channel c, samples [i0, i0 + nd)) that wavefront `wv` of `nw` takes, in order
// run r -> sample i0 + r / runs, units (r % runs) * 64 + lane
#define TN_PLANE_LOOP(g, i0, nd, wv, nw, ...)                                              \
    for (long long r_ = (wv); r_ < (long long)(nd) * (g).runs; r_ += (nw)) {                 \
        const int i_ = (i0) + (int)(r_ / (g).runs);                                           \
        const int u_ = (int)(r_ - (long long)(i_ - (i0)) * (g).runs) * 64 + lane;            \
        if (u_ < (g).units) { __VA_ARGS__ }                                                     \
    }

template <int VEC>
__global__ void __launch_bounds__(256) tn_stats_plane_kernel(const float* __restrict__ x, TnView vx, TnGeom g,
                                                             double* __restrict__ part) {
    __shared__ Rec red[4];
    const int c = blockIdx.x, d = blockIdx.y, k = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = d ? g.n_src : 0, nd = d ? g.n - g.n_src : g.n_src;
    const float* xc = x + (size_t)c * vx.ldc;
    Shifted a{0.f, 0.f, 0.f, 0};
    TN_PLANE_LOOP(g, i0, nd, k * 4 + wave, g.K * 4, {
        const float* p = xc + (size_t)i_ * vx.ldb;
        if (VEC) {
            const float4 v = *(const float4*)(p + 4 * (size_t)u_);
            shifted_add(a, v.x);
            shifted_add(a, v.y);
            shifted_add(a, v.z);
            shifted_add(a, v.w);
        } else {
            shifted_add(a, p[u_]);
        }
    })
    const Rec r = wave_merge(shifted_rec(a));
    if (lane == 0) red[wave] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        const Rec t = rec_merge(rec_merge(red[0], red[1]), rec_merge(red[2], red[3]));
        double* o = part + ((size_t)(c * 2 + d) * g.K + k) * 3;
        o[0] = t.n;
        o[1] = t.mean;
        o[2] = t.m2;
    }
}

// row route: workgroup (64 channels from c0, domain d, k); wavefront w takes the samples k * 4 + w, + 4 K, ...
__global__ void __launch_bounds__(256) tn_stats_row_kernel(const float* __restrict__ x, TnView vx, TnGeom g,
                                                           double* __restrict__ part) {
    __shared__ Rec red[4][64];
    const int d = blockIdx.y, k = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int i0 = d ? g.n_src : 0, nd = d ? g.n - g.n_src : g.n_src;
    Shifted a{0.f, 0.f, 0.f, 0};
    if (c < g.C) {
        const float* xc = x + (size_t)c * vx.ldc;
        for (int i = k * 4 + wave; i < nd; i += 4 * g.K) {
            const float* p = xc + (size_t)(i0 + i) * vx.ldb;
            for (int q = 0; q < g.s; ++q) shifted_add(a, p[q]);
        }
    }
    red[wave][lane] = shifted_rec(a);
    __syncthreads();
    if (wave == 0 && c < g.C) {
        const Rec t = rec_merge(rec_merge(red[0][lane], red[1][lane]), rec_merge(red[2][lane], red[3][lane]));
        double* o = part + ((size_t)(c * 2 + d) * g.K + k) * 3;
        o[0] = t.n;
        o[1] = t.mean;
        o[2] = t.m2;
    }
}

// the finalize workgroup: 1024 threads (one workgroup must see every channel; 256 threads took 15 us at C = 2048, each
// walking eight channels' records, divisions and square roots in turn)
constexpr int TN_FIN = 1024;
// the sum of the workgroup's values in a fixed order (the wavefront tree, then the 16 wavefronts ascending); every thread
// gets it
static __device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int w = 1; w < TN_FIN / 64; ++w) t += red[w];
    return t;
}

// one workgroup.  saved [5][C]: mean_s, rstd_s, mean_t, rstd_t, alpha
__global__ void __launch_bounds__(TN_FIN) tn_finalize_kernel(const double* __restrict__ part, int C, int K, float eps, float mom,
                                                          float* __restrict__ rm_s, float* __restrict__ rv_s,
                                                          float* __restrict__ rm_t, float* __restrict__ rv_t,
                                                          float* __restrict__ saved) {
    __shared__ double red[TN_FIN / 64];
    double psum = 0.0;
    for (int c = threadIdx.x; c < C; c += TN_FIN) {
        double q[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const double* p = part + (size_t)(c * 2 + d) * K * 3;
            Rec t{p[0], p[1], p[2]};
            for (int k = 1; k < K; ++k) t = rec_merge(t, Rec{p[3 * k], p[3 * k + 1], p[3 * k + 2]});
            const double var_b = t.m2 / t.n, var_u = t.m2 / (t.n - 1.0);
            saved[(size_t)(2 * d) * C + c] = (float)t.mean;
            saved[(size_t)(2 * d + 1) * C + c] = (float)(1.0 / sqrt(var_b + (double)eps));
            q[d] = t.mean / sqrt(var_u + (double)eps);
            float* rm = d ? rm_t : rm_s;
            float* rv = d ? rv_t : rv_s;
            if (rm) {
                rm[c] = (float)((1.0 - (double)mom) * (double)rm[c] + (double)mom * t.mean);
                rv[c] = (float)((1.0 - (double)mom) * (double)rv[c] + (double)mom * var_u);
            }
        }
        const double prob = 1.0 / (1.0 + fabs(q[0] - q[1]));
        saved[(size_t)4 * C + c] = (float)prob;          // read back below by the thread that wrote it
        psum += (double)(float)prob;       // the rounded value: C * prob / sum is exactly 1 for C = 1
    }
    const double tot = block_sum_d(psum, red);
    for (int c = threadIdx.x; c < C; c += TN_FIN) {
        const double prob = (double)saved[(size_t)4 * C + c];
        saved[(size_t)4 * C + c] = (float)((double)C * prob / tot);
    }
}

// eval: the saved block from the running vectors (alpha from all four, no update)
__global__ void __launch_bounds__(TN_FIN) tn_finalize_eval_kernel(int C, float eps, const float* __restrict__ rm_s,
                                                               const float* __restrict__ rv_s, const float* __restrict__ rm_t,
                                                               const float* __restrict__ rv_t, float* __restrict__ saved) {
    __shared__ double red[TN_FIN / 64];
    double psum = 0.0;
    for (int c = threadIdx.x; c < C; c += TN_FIN) {
        const double ms = rm_s[c], vs = rv_s[c], mt = rm_t[c], vt = rv_t[c];
        const double is = 1.0 / sqrt(vs + (double)eps), it = 1.0 / sqrt(vt + (double)eps);
        saved[c] = (float)ms;
        saved[(size_t)C + c] = (float)is;
        saved[(size_t)2 * C + c] = (float)mt;
        saved[(size_t)3 * C + c] = (float)it;
        const double prob = 1.0 / (1.0 + fabs(ms / sqrt(vs + (double)eps) - mt / sqrt(vt + (double)eps)));
        saved[(size_t)4 * C + c] = (float)prob;
        psum += (double)(float)prob;       // the rounded value: C * prob / sum is exactly 1 for C = 1
    }
    const double tot = block_sum_d(psum, red);
    for (int c = threadIdx.x; c < C; c += TN_FIN) {
        const double prob = (double)saved[(size_t)4 * C + c];
        saved[(size_t)4 * C + c] = (float)((double)C * prob / tot);
    }
}

// the five constants of channel c for domain d (eval: the target's for every sample)
struct TnConst {
    float mean, rstd, w, b;
    double a1;
};
static __device__ __forceinline__ TnConst tn_const(const float* __restrict__ saved, const float* __restrict__ weight,
                                                   const float* __restrict__ bias, int C, int c, int d) {
    TnConst k;
    k.mean = saved[(size_t)(2 * d) * C + c];
    k.rstd = saved[(size_t)(2 * d + 1) * C + c];
    k.w = weight ? weight[c] : 1.f;
    k.b = bias ? bias[c] : 0.f;
    k.a1 = 1.0 + (double)saved[(size_t)4 * C + c];
    return k;
}

// plane route: workgroup (channel c, k of gridDim.y) over the runs of all n samples
template <int VEC>
__global__ void __launch_bounds__(256) tn_apply_plane_kernel(const float* __restrict__ x, TnView vx, float* __restrict__ y,
                                                             TnView vy, TnGeom g, int eval, const float* __restrict__ saved,
                                                             const float* __restrict__ weight, const float* __restrict__ bias) {
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TnConst ks = tn_const(saved, weight, bias, g.C, c, eval ? 1 : 0), kt = tn_const(saved, weight, bias, g.C, c, 1);
    const float* xc = x + (size_t)c * vx.ldc;
    float* yc = y + (size_t)c * vy.ldc;
    TN_PLANE_LOOP(g, 0, g.n, blockIdx.y * 4 + wave, gridDim.y * 4, {
        const TnConst& q = i_ < g.n_src ? ks : kt;
        const float* p = xc + (size_t)i_ * vx.ldb;
        float* o = yc + (size_t)i_ * vy.ldb;
        if (VEC) {
            const float4 v = *(const float4*)(p + 4 * (size_t)u_);
            float4 r;
            r.x = tn_y(v.x, q.mean, q.rstd, q.w, q.b, q.a1);
            r.y = tn_y(v.y, q.mean, q.rstd, q.w, q.b, q.a1);
            r.z = tn_y(v.z, q.mean, q.rstd, q.w, q.b, q.a1);
            r.w = tn_y(v.w, q.mean, q.rstd, q.w, q.b, q.a1);
            *(float4*)(o + 4 * (size_t)u_) = r;
        } else {
            o[u_] = tn_y(p[u_], q.mean, q.rstd, q.w, q.b, q.a1);
        }
    })
}

// row route: workgroup (64 channels, k of gridDim.y); wavefront w takes the samples k * 4 + w, + 4 gridDim.y, ...
__global__ void __launch_bounds__(256) tn_apply_row_kernel(const float* __restrict__ x, TnView vx, float* __restrict__ y,
                                                           TnView vy, TnGeom g, int eval, const float* __restrict__ saved,
                                                           const float* __restrict__ weight, const float* __restrict__ bias) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    if (c >= g.C) return;
    const TnConst ks = tn_const(saved, weight, bias, g.C, c, eval ? 1 : 0), kt = tn_const(saved, weight, bias, g.C, c, 1);
    const float* xc = x + (size_t)c * vx.ldc;
    float* yc = y + (size_t)c * vy.ldc;
    for (int i = blockIdx.y * 4 + wave; i < g.n; i += 4 * gridDim.y) {
        const TnConst& q = i < g.n_src ? ks : kt;
        const float* p = xc + (size_t)i * vx.ldb;
        float* o = yc + (size_t)i * vy.ldb;
        for (int e = 0; e < g.s; ++e) o[e] = tn_y(p[e], q.mean, q.rstd, q.w, q.b, q.a1);
    }
}

// ---- backward.  bpart [C][2][K][2]: sum g, sum g xhat
template <int VEC>
__global__ void __launch_bounds__(256) tn_bwd_reduce_plane_kernel(const float* __restrict__ gy, TnView vg,
                                                                  const float* __restrict__ x, TnView vx, TnGeom g, int eval,
                                                                  const float* __restrict__ saved, double* __restrict__ bpart) {
    __shared__ double red[4][2];
    const int c = blockIdx.x, d = blockIdx.y, k = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = d ? g.n_src : 0, nd = d ? g.n - g.n_src : g.n_src;
    const int ds = eval ? 1 : d;
    const float mean = saved[(size_t)(2 * ds) * g.C + c], rstd = saved[(size_t)(2 * ds + 1) * g.C + c];
    const float* xc = x + (size_t)c * vx.ldc;
    const float* gc = gy + (size_t)c * vg.ldc;
    float s1 = 0.f, s2 = 0.f;
    TN_PLANE_LOOP(g, i0, nd, k * 4 + wave, g.K * 4, {
        const float* p = xc + (size_t)i_ * vx.ldb;
        const float* q = gc + (size_t)i_ * vg.ldb;
        if (VEC) {
            const float4 v = *(const float4*)(p + 4 * (size_t)u_);
            const float4 h = *(const float4*)(q + 4 * (size_t)u_);
            s1 += (h.x + h.y) + (h.z + h.w);
            s2 += (h.x * tn_xhat(v.x, mean, rstd) + h.y * tn_xhat(v.y, mean, rstd)) +
                  (h.z * tn_xhat(v.z, mean, rstd) + h.w * tn_xhat(v.w, mean, rstd));
        } else {
            const float h = q[u_];
            s1 += h;
            s2 += h * tn_xhat(p[u_], mean, rstd);
        }
    })
    const double t1 = wave_sum_d((double)s1), t2 = wave_sum_d((double)s2);
    if (lane == 0) {
        red[wave][0] = t1;
        red[wave][1] = t2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* o = bpart + ((size_t)(c * 2 + d) * g.K + k) * 2;
        o[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        o[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    }
}

__global__ void __launch_bounds__(256) tn_bwd_reduce_row_kernel(const float* __restrict__ gy, TnView vg,
                                                                const float* __restrict__ x, TnView vx, TnGeom g, int eval,
                                                                const float* __restrict__ saved, double* __restrict__ bpart) {
    __shared__ double red[4][2][64];
    const int d = blockIdx.y, k = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int i0 = d ? g.n_src : 0, nd = d ? g.n - g.n_src : g.n_src;
    const int ds = eval ? 1 : d;
    double s1 = 0.0, s2 = 0.0;
    if (c < g.C) {
        const float mean = saved[(size_t)(2 * ds) * g.C + c], rstd = saved[(size_t)(2 * ds + 1) * g.C + c];
        const float* xc = x + (size_t)c * vx.ldc;
        const float* gc = gy + (size_t)c * vg.ldc;
        for (int i = k * 4 + wave; i < nd; i += 4 * g.K) {
            const float* p = xc + (size_t)(i0 + i) * vx.ldb;
            const float* q = gc + (size_t)(i0 + i) * vg.ldb;
            float r1 = 0.f, r2 = 0.f;
            for (int e = 0; e < g.s; ++e) {
                const float h = q[e];
                r1 += h;
                r2 += h * tn_xhat(p[e], mean, rstd);
            }
            s1 += (double)r1;
            s2 += (double)r2;
        }
    }
    red[wave][0][lane] = s1;
    red[wave][1][lane] = s2;
    __syncthreads();
    if (wave == 0 && c < g.C) {
        double* o = bpart + ((size_t)(c * 2 + d) * g.K + k) * 2;
        o[0] = (red[0][0][lane] + red[1][0][lane]) + (red[2][0][lane] + red[3][0][lane]);
        o[1] = (red[0][1][lane] + red[1][1][lane]) + (red[2][1][lane] + red[3][1][lane]);
    }
}

// thread = channel.  coef [6][C]: per domain A = rstd a w, B = rstd mean_d(gh), D = rstd mean_d(gh xhat), with
// a = 1 + alpha, gh = g a w
__global__ void __launch_bounds__(256) tn_bwd_finalize_kernel(const double* __restrict__ bpart, TnGeom g, int eval,
                                                              const float* __restrict__ saved, const float* __restrict__ weight,
                                                              float* __restrict__ coef, float* __restrict__ dweight,
                                                              float* __restrict__ dbias) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= g.C) return;
    const double a = 1.0 + (double)saved[(size_t)4 * g.C + c];
    const double w = weight ? (double)weight[c] : 1.0;
    double sg[2], sx[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const double* p = bpart + (size_t)(c * 2 + d) * g.K * 2;
        double t1 = p[0], t2 = p[1];
        for (int k = 1; k < g.K; ++k) {
            t1 += p[2 * k];
            t2 += p[2 * k + 1];
        }
        sg[d] = t1;
        sx[d] = t2;
        if (!eval) {
            const double cnt = (double)(d ? g.n - g.n_src : g.n_src) * (double)g.s;
            const double rstd = (double)saved[(size_t)(2 * d + 1) * g.C + c];
            coef[(size_t)(3 * d) * g.C + c] = (float)(rstd * a * w);
            coef[(size_t)(3 * d + 1) * g.C + c] = (float)(rstd * a * w * t1 / cnt);
            coef[(size_t)(3 * d + 2) * g.C + c] = (float)(rstd * a * w * t2 / cnt);
        }
    }
    if (dweight) dweight[c] = (float)(a * (sx[0] + sx[1]));
    if (dbias) dbias[c] = (float)(a * (sg[0] + sg[1]));
}

struct TnBwdConst {
    float mean, rstd, A, B, D;
};
static __device__ __forceinline__ TnBwdConst tn_bwd_const(const float* __restrict__ saved, const float* __restrict__ coef,
                                                          const float* __restrict__ weight, int C, int c, int d, int eval) {
    TnBwdConst k;
    if (eval) {          // dx = g (1 + alpha) w rstd_t
        const double a1 = 1.0 + (double)saved[(size_t)4 * C + c];
        k.mean = 0.f;
        k.rstd = 0.f;
        k.A = (float)(a1 * (weight ? (double)weight[c] : 1.0) * (double)saved[(size_t)3 * C + c]);
        k.B = 0.f;
        k.D = 0.f;
        return k;
    }
    k.mean = saved[(size_t)(2 * d) * C + c];
    k.rstd = saved[(size_t)(2 * d + 1) * C + c];
    k.A = coef[(size_t)(3 * d) * C + c];
    k.B = coef[(size_t)(3 * d + 1) * C + c];
    k.D = coef[(size_t)(3 * d + 2) * C + c];
    return k;
}
static __device__ __forceinline__ float tn_dx(float gv, float xv, const TnBwdConst& k, int eval) {
#pragma clang fp contract(off)
    if (eval) return (float)((double)gv * (double)k.A);
    const double xh = ((double)xv - (double)k.mean) * (double)k.rstd;
    return (float)(((double)k.A * (double)gv - (double)k.B) - xh * (double)k.D);
}

template <int VEC>
__global__ void __launch_bounds__(256) tn_bwd_apply_plane_kernel(const float* __restrict__ gy, TnView vg,
                                                                 const float* __restrict__ x, TnView vx, float* __restrict__ dx,
                                                                 TnView vd, TnGeom g, int eval, const float* __restrict__ saved,
                                                                 const float* __restrict__ coef,
                                                                 const float* __restrict__ weight) {
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TnBwdConst ks = tn_bwd_const(saved, coef, weight, g.C, c, 0, eval), kt = tn_bwd_const(saved, coef, weight, g.C, c, 1, eval);
    const float* xc = x + (size_t)c * vx.ldc;
    const float* gc = gy + (size_t)c * vg.ldc;
    float* dc = dx + (size_t)c * vd.ldc;
    TN_PLANE_LOOP(g, 0, g.n, blockIdx.y * 4 + wave, gridDim.y * 4, {
        const TnBwdConst& q = i_ < g.n_src ? ks : kt;
        const float* p = xc + (size_t)i_ * vx.ldb;
        const float* h = gc + (size_t)i_ * vg.ldb;
        float* o = dc + (size_t)i_ * vd.ldb;
        if (VEC) {
            const float4 gv = *(const float4*)(h + 4 * (size_t)u_);
            float4 v = gv;
            if (!eval) v = *(const float4*)(p + 4 * (size_t)u_);
            float4 r;
            r.x = tn_dx(gv.x, v.x, q, eval);
            r.y = tn_dx(gv.y, v.y, q, eval);
            r.z = tn_dx(gv.z, v.z, q, eval);
            r.w = tn_dx(gv.w, v.w, q, eval);
            *(float4*)(o + 4 * (size_t)u_) = r;
        } else {
            o[u_] = tn_dx(h[u_], eval ? 0.f : p[u_], q, eval);
        }
    })
}

__global__ void __launch_bounds__(256) tn_bwd_apply_row_kernel(const float* __restrict__ gy, TnView vg,
                                                               const float* __restrict__ x, TnView vx, float* __restrict__ dx,
                                                               TnView vd, TnGeom g, int eval, const float* __restrict__ saved,
                                                               const float* __restrict__ coef, const float* __restrict__ weight) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    if (c >= g.C) return;
    const TnBwdConst ks = tn_bwd_const(saved, coef, weight, g.C, c, 0, eval), kt = tn_bwd_const(saved, coef, weight, g.C, c, 1, eval);
    const float* xc = x + (size_t)c * vx.ldc;
    const float* gc = gy + (size_t)c * vg.ldc;
    float* dc = dx + (size_t)c * vd.ldc;
    for (int i = blockIdx.y * 4 + wave; i < g.n; i += 4 * gridDim.y) {
        const TnBwdConst& q = i < g.n_src ? ks : kt;
        const float* p = xc + (size_t)i * vx.ldb;
        const float* h = gc + (size_t)i * vg.ldb;
        float* o = dc + (size_t)i * vd.ldb;
        for (int e = 0; e < g.s; ++e) o[e] = tn_dx(h[e], eval ? 0.f : p[e], q, eval);
    }
}

// ---- host side
bool tn_aligned(const void* p, long long ldc, long long ldb) { return !((uintptr_t)p & 15) && !(ldc & 3) && !(ldb & 3); }

// the sizes both entry points serve (the pointer and stride checks are their own)
bool tn_served(int n, int n_src, int C, int s, int training) {
    if (n < 1 || C < 1 || s < 1 || C > (1 << 20)) return false;
    if ((long long)n * s > (1ll << 30)) return false;
    if (!training) return true;
    // each half needs two values per channel (the unbiased variance divides by count - 1)
    return n_src >= 1 && n_src < n && (long long)n_src * s >= 2 && (long long)(n - n_src) * s >= 2;
}

// K: records per (channel, domain).  Enough workgroups to fill the chip when C is small, at most 8 runs (plane) or 8
// samples (row) per wavefront when the halves are large, never more than there is work for.
TnGeom tn_geom(int n, int n_src, int C, int s, bool vec) {
    TnGeom g;
    g.n = n;
    g.n_src = n_src;
    g.C = C;
    g.s = s;
    g.vec = vec ? 1 : 0;
    g.units = vec ? s / 4 : s;
    g.runs = cdiv(g.units, 64);
    const int nd = n - n_src > n_src ? n - n_src : n_src;          // the larger half (eval: all samples)
    long long work, groups;                                          // wavefront jobs per (channel, domain); channel groups
    if (tn_plane_route(s)) {
        work = (long long)nd * g.runs;
        groups = C;
    } else {
        work = nd;
        groups = cdiv(C, 64);
    }
    long long K = (work + 31) / 32;                                  // 8 jobs per wavefront
    const long long fill = (1024 + 2 * groups - 1) / (2 * groups);   // ~1024 workgroups in the launch
    if (K < fill) K = fill;
    const long long most = (work + 3) / 4;
    if (K > most) K = most;
    if (K > TN_MAX_K) K = TN_MAX_K;
    if (K < 1) K = 1;
    g.K = (int)K;
    return g;
}

size_t tn_fwd_bytes(int C, int K) { return a256((size_t)C * 2 * K * 3 * sizeof(double)); }
size_t tn_bwd_off_coef(int C, int K) { return a256((size_t)C * 2 * K * 2 * sizeof(double)); }
size_t tn_bwd_bytes(int C, int K) { return tn_bwd_off_coef(C, K) + a256((size_t)6 * C * sizeof(float)); }

bool tn_view_ok(int n, int C, int s, long long ldc, long long ldb) {
    return ldc >= s && (n <= 1 || ldb >= ldc * C);
}

}  // namespace

extern "C" size_t rgda_transnorm_fwd_workspace(int n, int n_src, int C, int s, int training) {
    if (!tn_served(n, n_src, C, s, training)) return 0;
    if (!training) return 256;
    return tn_fwd_bytes(C, tn_geom(n, n_src, C, s, false).K);
}

extern "C" int rgda_transnorm_fwd(const float* x, int n, int n_src, int C, int s, int64_t ldc, int64_t ldb, const float* weight,
                                  const float* bias, float* rm_s, float* rv_s, float* rm_t, float* rv_t, float eps, float momentum,
                                  int training, float* y, int64_t ldc_y, int64_t ldb_y, float* saved, void* ws, size_t ws_bytes,
                                  rgda_stream_t stream) {
    if (!x || !y || !saved || !ws) return RGDA_ERR_ARG;
    if (n < 1 || C < 1 || s < 1) return RGDA_ERR_ARG;
    if (!(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return RGDA_ERR_ARG;
    if ((weight == nullptr) != (bias == nullptr)) return RGDA_ERR_ARG;
    const int nrun = (rm_s ? 1 : 0) + (rv_s ? 1 : 0) + (rm_t ? 1 : 0) + (rv_t ? 1 : 0);
    if (nrun != 0 && nrun != 4) return RGDA_ERR_ARG;
    if (!training && nrun != 4) return RGDA_ERR_ARG;
    if (training && (n_src < 0 || n_src > n)) return RGDA_ERR_ARG;
    if (!tn_view_ok(n, C, s, ldc, ldb) || !tn_view_ok(n, C, s, ldc_y, ldb_y)) return RGDA_ERR_ARG;
    if ((uintptr_t)ws & 255) return RGDA_ERR_ARG;
    if (!tn_served(n, n_src, C, s, training)) return RGDA_ERR_UNSUPPORTED;
    const bool plane = tn_plane_route(s);
    const bool vec = plane && !(s & 3) && tn_aligned(x, ldc, ldb) && tn_aligned(y, ldc_y, ldb_y);
    if (!training) n_src = 0;
    const TnGeom g = tn_geom(n, n_src, C, s, vec);
    if (training && ws_bytes < tn_fwd_bytes(C, g.K)) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    const TnView vx{(long long)ldc, (long long)ldb}, vy{(long long)ldc_y, (long long)ldb_y};
    double* part = (double*)ws;
    if (training) {
        if (plane) {
            if (vec) tn_stats_plane_kernel<1><<<dim3(C, 2, g.K), 256, 0, st>>>(x, vx, g, part);
            else tn_stats_plane_kernel<0><<<dim3(C, 2, g.K), 256, 0, st>>>(x, vx, g, part);
        } else {
            tn_stats_row_kernel<<<dim3(cdiv(C, 64), 2, g.K), 256, 0, st>>>(x, vx, g, part);
        }
        RGDA_CHECK_LAUNCH();
        tn_finalize_kernel<<<1, TN_FIN, 0, st>>>(part, C, g.K, eps, momentum, rm_s, rv_s, rm_t, rv_t, saved);
    } else {
        tn_finalize_eval_kernel<<<1, TN_FIN, 0, st>>>(C, eps, rm_s, rv_s, rm_t, rv_t, saved);
    }
    RGDA_CHECK_LAUNCH();
    // the apply pass covers both halves: twice the records' share of the work per channel group
    const int KA = g.K * 2 > 65535 ? 65535 : g.K * 2;
    if (plane) {
        if (vec) tn_apply_plane_kernel<1><<<dim3(C, KA), 256, 0, st>>>(x, vx, y, vy, g, !training, saved, weight, bias);
        else tn_apply_plane_kernel<0><<<dim3(C, KA), 256, 0, st>>>(x, vx, y, vy, g, !training, saved, weight, bias);
    } else {
        tn_apply_row_kernel<<<dim3(cdiv(C, 64), KA), 256, 0, st>>>(x, vx, y, vy, g, !training, saved, weight, bias);
    }
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" size_t rgda_transnorm_bwd_workspace(int n, int n_src, int C, int s, int training) {
    if (!tn_served(n, n_src, C, s, training)) return 0;
    return tn_bwd_bytes(C, tn_geom(n, training ? n_src : 0, C, s, false).K);
}

extern "C" int rgda_transnorm_bwd(const float* g, int64_t ldc_g, int64_t ldb_g, const float* x, int n, int n_src, int C, int s,
                                  int64_t ldc, int64_t ldb, const float* weight, const float* saved, int training, float* dx,
                                  int64_t ldc_dx, int64_t ldb_dx, float* dweight, float* dbias, void* ws, size_t ws_bytes,
                                  rgda_stream_t stream) {
    if (!g || !x || !saved || !ws) return RGDA_ERR_ARG;
    if (n < 1 || C < 1 || s < 1) return RGDA_ERR_ARG;
    if (training && (n_src < 0 || n_src > n)) return RGDA_ERR_ARG;
    if (!tn_view_ok(n, C, s, ldc, ldb) || !tn_view_ok(n, C, s, ldc_g, ldb_g)) return RGDA_ERR_ARG;
    if (dx && !tn_view_ok(n, C, s, ldc_dx, ldb_dx)) return RGDA_ERR_ARG;
    if ((uintptr_t)ws & 255) return RGDA_ERR_ARG;
    if (!tn_served(n, n_src, C, s, training)) return RGDA_ERR_UNSUPPORTED;
    const bool plane = tn_plane_route(s);
    const bool vec = plane && !(s & 3) && tn_aligned(x, ldc, ldb) && tn_aligned(g, ldc_g, ldb_g) &&
                     (!dx || tn_aligned(dx, ldc_dx, ldb_dx));
    if (!training) n_src = 0;
    const TnGeom gm = tn_geom(n, n_src, C, s, vec);
    if (ws_bytes < tn_bwd_bytes(C, gm.K)) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    const TnView vx{(long long)ldc, (long long)ldb}, vg{(long long)ldc_g, (long long)ldb_g},
        vd{(long long)ldc_dx, (long long)ldb_dx};
    double* bpart = (double*)ws;
    float* coef = (float*)((char*)ws + tn_bwd_off_coef(C, gm.K));
    const int eval = !training;
    if (training || dweight || dbias) {
        if (plane) {
            if (vec) tn_bwd_reduce_plane_kernel<1><<<dim3(C, 2, gm.K), 256, 0, st>>>(g, vg, x, vx, gm, eval, saved, bpart);
            else tn_bwd_reduce_plane_kernel<0><<<dim3(C, 2, gm.K), 256, 0, st>>>(g, vg, x, vx, gm, eval, saved, bpart);
        } else {
            tn_bwd_reduce_row_kernel<<<dim3(cdiv(C, 64), 2, gm.K), 256, 0, st>>>(g, vg, x, vx, gm, eval, saved, bpart);
        }
        RGDA_CHECK_LAUNCH();
        tn_bwd_finalize_kernel<<<cdiv(C, 256), 256, 0, st>>>(bpart, gm, eval, saved, weight, coef, dweight, dbias);
        RGDA_CHECK_LAUNCH();
    }
    if (!dx) return RGDA_OK;
    const int KA = gm.K * 2 > 65535 ? 65535 : gm.K * 2;
    if (plane) {
        if (vec) tn_bwd_apply_plane_kernel<1><<<dim3(C, KA), 256, 0, st>>>(g, vg, x, vx, dx, vd, gm, eval, saved, coef, weight);
        else tn_bwd_apply_plane_kernel<0><<<dim3(C, KA), 256, 0, st>>>(g, vg, x, vx, dx, vd, gm, eval, saved, coef, weight);
    } else {
        tn_bwd_apply_row_kernel<<<dim3(cdiv(C, 64), KA), 256, 0, st>>>(g, vg, x, vx, dx, vd, gm, eval, saved, coef, weight);
    }
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
