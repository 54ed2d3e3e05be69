// Semantic-aware whitening loss (regda/gast/SAW.py:54-107, Peng et al., CVPR 2022): forward and the gradient w.r.t. the
// feature map, deterministic (no floating-point atomics).  The definition, the tie rule and the workspace layout are at
// rgda_saw_loss in include/rgda_hip.h.
//
// For every selected class the channels are ranked by |w|; the C channels of rank g, each scaled by the sigmoid of its
// |w|, form group g, and the off-diagonal covariances of every group are penalised.  Five launches (the first clears
// the flag word), whatever k and the number of groups:
//   plan  : ranks by counting (exact, no sort), per (class, 16 channels): rank(c) = the channels with larger |w|, or
//           equal |w| and lower index.  A rank below G fills slot (rank, class): ch, wgh = sigmoid(|w|), and the inverse
//           table inv[c][class] = rank (-1: no slot).  A non-finite weight sets flag bit 0 and ranks as +inf, so the
//           ranks stay a permutation and every slot is filled                              saw_plan_kernel
//   gram  : one workgroup per (image, group): the nod = C (C - 1) / 2 dot products over the pixels -- thread t adds the
//           pixels t + 256 i in ascending i, a butterfly per wavefront, (w0 + w1) + (w2 + w3) --, cov = dot / (hw - 1),
//           s = the sum of |cov| in pair order, the active bit s > margin, the pair signs, the partial loss; then, for an
//           active group with a gradient buffer, the slot gradients
//           wgh_j coef sum_{j' != j} sign(cov_jj') wgh_j' x_j'[p] (j' ascending) into the fp32 scratch   saw_gram_kernel
//   loss  : loss[0] += weight / B * sum of the partials, fixed order                         rows_loss_sum
//   grad  : per (image, 64 pixels, 64 channels): a channel's gradient is gathered through inv from its <= C slots in
//           class order (inactive groups skipped), transposed through LDS and stored into the pixel-major bf16 rows
//                                                                                           saw_grad_kernel
#include <math.h>

#include "feat_rows.h"

namespace {

constexpr int SAW_MAX_K = 4096;

bool saw_classes_ok(int C) { return C == 2 || C == 4 || C == 6 || C == 8 || C == 16; }

struct SawPlan {
    int G, nod, TS;
    long long jobs;              // b * G
    size_t off_tab, off_s, off_lpart, off_ch, off_wgh, off_inv, off_slot, bytes_loss, bytes;
};

SawPlan make_plan(int b, int hw, int k, int C) {
    SawPlan p;
    p.G = k / C;
    p.nod = C * (C - 1) / 2;
    p.TS = (p.nod + 1 + 3) & ~3;                      // bytes per (image, group): the active byte, then the pair signs
    p.jobs = (long long)b * p.G;
    size_t o = 256;                                   // header: the flag word
    p.off_tab = o;   o += a256((size_t)p.jobs * p.TS);
    p.off_s = o;     o += a256((size_t)p.jobs * 4);
    p.off_lpart = o; o += a256((size_t)p.jobs * 4);
    p.off_ch = o;    o += a256((size_t)p.G * C * 4);
    p.off_wgh = o;   o += a256((size_t)p.G * C * 4);
    p.off_inv = o;   o += a256((size_t)k * C * 4);
    p.bytes_loss = o;                                 // what a call without a gradient buffer needs
    p.off_slot = o;  o += a256((size_t)p.jobs * C * hw * 4);
    p.bytes = o;
    return p;
}

// does the entry point serve these sizes?  (the pointer and stride checks are its own)
bool saw_served(int b, int hw, int k, int C) {
    if (!saw_classes_ok(C) || b <= 0 || hw < 2 || k < C || k > SAW_MAX_K) return false;
    if ((long long)b * hw > (1 << 24)) return false;
    return (long long)b * (k / C) <= 0x7fffffffll;
}

struct SawSel {
    int v[16];
};

}  // namespace

// workgroup (16 channels, class j): the row of the class in LDS; thread (channel i, part q) counts over the channels
// q, q + 16, ...; the 16 integer partials of a channel are added through LDS
__global__ void __launch_bounds__(256) saw_plan_kernel(const float* __restrict__ cls_w, long long ldw, SawSel sel, int k, int C,
                                                       int G, int* __restrict__ flag, int* __restrict__ ch,
                                                       float* __restrict__ wgh, int* __restrict__ inv) {
    __shared__ float a[SAW_MAX_K];
    __shared__ int part[16][17];
    const int j = blockIdx.y;
    const float* row = cls_w + (size_t)sel.v[j] * ldw;
    int bad = 0;
    for (int c = threadIdx.x; c < k; c += 256) {
        float v = fabsf(row[c]);
        if (!(v <= 3.402823466e38f)) {          // Inf or NaN
            bad = 1;
            v = __builtin_inff();
        }
        a[c] = v;
    }
    if (bad) atomicOr(flag, 1);
    __syncthreads();
    const int i = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + i;
    const float v = a[min(c, k - 1)];
    int n = 0;
    for (int o = q; o < k; o += 16) {
        const float u = a[o];
        n += (u > v || (u == v && o < c)) ? 1 : 0;
    }
    part[i][q] = n;
    __syncthreads();
    if (q != 0 || c >= k) return;
    int rank = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) rank += part[i][t];
    if (rank < G) {
        ch[rank * C + j] = c;
        wgh[rank * C + j] = (float)(1.0 / (1.0 + exp(-(double)v)));      // the sigmoid, rounded once
        inv[c * C + j] = rank;
    } else {
        inv[c * C + j] = -1;
    }
}

template <int C>
__global__ void __launch_bounds__(256) saw_gram_kernel(FeatView f, const int* __restrict__ ch, const float* __restrict__ wgh,
                                                       int G, long long njobs, float margin, float coef,
                                                       signed char* __restrict__ tab, int TS, float* __restrict__ sv,
                                                       float* __restrict__ lpart, float* __restrict__ slot) {
    constexpr int NOD = C * (C - 1) / 2;
    __shared__ float red[4][NOD];
    __shared__ float acov[NOD];
    __shared__ float sgn[C][C];
    __shared__ int act;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hw = f.hw;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) {
        const int b = (int)(job / G), g = (int)(job - (long long)b * G);
        const float* src[C];
        float w[C];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            src[j] = f.x + (size_t)b * f.ldb + (size_t)ch[g * C + j] * f.ldc;
            w[j] = wgh[g * C + j];
        }
        float acc[NOD];
#pragma unroll
        for (int q = 0; q < NOD; ++q) acc[q] = 0.f;
        for (int p = tid; p < hw; p += 256) {
            float x[C];
#pragma unroll
            for (int j = 0; j < C; ++j) x[j] = w[j] * src[j][p];
            int q = 0;
#pragma unroll
            for (int j = 0; j < C; ++j)
#pragma unroll
                for (int jj = j + 1; jj < C; ++jj) {
                    acc[q] += x[j] * x[jj];
                    ++q;
                }
        }
#pragma unroll
        for (int q = 0; q < NOD; ++q) {
            const float v = wave_sum(acc[q]);
            if (lane == 0) red[wave][q] = v;
        }
        __syncthreads();
        if (tid < NOD) {
            const float c = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) / (float)(hw - 1);
            const float sg = (c > 0.f) ? 1.f : ((c < 0.f) ? -1.f : 0.f);
            int j = 0, rest = tid;                     // pair tid = (j, jj), j < jj, row-major
            while (rest >= C - 1 - j) {
                rest -= C - 1 - j;
                ++j;
            }
            const int jj = j + 1 + rest;
            acov[tid] = fabsf(c);
            sgn[j][jj] = sg;
            sgn[jj][j] = sg;
            tab[(size_t)job * TS + 1 + tid] = (signed char)sg;
        }
        if (tid < C) sgn[tid][tid] = 0.f;
        __syncthreads();
        if (tid == 0) {
            float s = 0.f;
            for (int q = 0; q < NOD; ++q) s += acov[q];
            const int on = s > margin ? 1 : 0;
            act = on;
            tab[(size_t)job * TS] = (signed char)on;
            sv[job] = s;
            lpart[job] = on ? (s - margin) / (float)NOD : 0.f;
        }
        __syncthreads();
        if (slot && act) {
            float* dst = slot + (size_t)job * C * hw;
            for (int p = tid; p < hw; p += 256) {
                float x[C];
#pragma unroll
                for (int j = 0; j < C; ++j) x[j] = w[j] * src[j][p];
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    float v = 0.f;
#pragma unroll
                    for (int jj = 0; jj < C; ++jj) v += sgn[j][jj] * x[jj];
                    dst[(size_t)j * hw + p] = w[j] * coef * v;
                }
            }
        }
        __syncthreads();                               // the LDS tables are rewritten by the next job
    }
}

// workgroup (image b, 64 pixels from p0, 64 channels from c0)
__global__ void __launch_bounds__(256) saw_grad_kernel(const int* __restrict__ inv, const signed char* __restrict__ tab, int TS,
                                                       const float* __restrict__ slot, int C, int G, int k, int hw, int tiles,
                                                       bf16_t* __restrict__ dfeat, int lddf, int accumulate) {
    __shared__ float tile[64][65];                     // [channel][pixel]
    __shared__ int from[64][16];                       // [channel][class]: the group whose slot gradient is gathered, or -1
    __shared__ int touched[64];
    const int b = blockIdx.x / tiles, p0 = (blockIdx.x - b * tiles) * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int p = p0 + tx;
    // the slots of the tile's channels that are active in this image, all looked up at once (two dependent loads each)
    for (int i = threadIdx.x; i < 64 * C; i += 256) {
        const int cc = i / C, j = i - cc * C, c = c0 + cc;
        int g = c < k ? inv[c * C + j] : -1;
        if (g >= 0 && !tab[((size_t)b * G + g) * TS]) g = -1;
        from[cc][j] = g;
    }
    __syncthreads();
    for (int cc = ty; cc < 64; cc += 4) {
        float v = 0.f;
        int t = 0;
        for (int j = 0; j < C; ++j) {                  // class order
            const int g = from[cc][j];
            if (g < 0) continue;
            t = 1;
            if (p < hw) v += slot[(((size_t)b * G + g) * C + j) * hw + p];
        }
        tile[cc][tx] = v;
        if (tx == 0) touched[cc] = t;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 1024; i += 256) {
        const int px = i >> 4, q = i & 15, c = c0 + 4 * q, pp = p0 + px;
        if (pp >= hw || c >= k) continue;
        bf16_t* row = dfeat + ((size_t)b * hw + pp) * lddf;
        const float v[4] = {tile[4 * q][px], tile[4 * q + 1][px], tile[4 * q + 2][px], tile[4 * q + 3][px]};
        const bool all = touched[4 * q] && touched[4 * q + 1] && touched[4 * q + 2] && touched[4 * q + 3];
        if (c + 3 < k && (!accumulate || all)) {
            store4_bf16(row + c, v[0], v[1], v[2], v[3], accumulate);
        } else {                                       // the last channels of a row, or a channel that receives nothing
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < k && (!accumulate || touched[4 * q + e]))
                    row[c + e] = f2bf(accumulate ? v[e] + bf2f(row[c + e]) : v[e]);
        }
    }
}

extern "C" size_t rgda_saw_loss_workspace(int b, int hw, int k, int C) {
    if (!saw_served(b, hw, k, C)) return 0;
    return make_plan(b, hw, k, C).bytes;
}

extern "C" int rgda_saw_loss(const float* feat, int b, int hw, int64_t ldc, int64_t ldb, int k, const float* cls_w, int n_cls,
                             int64_t ldw, const int32_t* selected, int C, float margin, float* loss, void* dfeat, int lddf,
                             int accumulate, float weight, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (!feat || !cls_w || !selected || !loss || !ws) return RGDA_ERR_ARG;
    if (b <= 0 || hw <= 0 || k <= 0 || n_cls <= 0 || ldw < k) return RGDA_ERR_ARG;
    if (!(margin >= 0.f)) return RGDA_ERR_ARG;        // negative or NaN
    if (!saw_served(b, hw, k, C)) return RGDA_ERR_UNSUPPORTED;
    SawSel sel;
    for (int j = 0; j < 16; ++j) sel.v[j] = 0;
    for (int j = 0; j < C; ++j) {
        const int c = selected[j];
        if (c < 0 || c >= n_cls) return RGDA_ERR_ARG;
        for (int i = 0; i < j; ++i)
            if (sel.v[i] == c) return RGDA_ERR_ARG;
        sel.v[j] = c;
    }
    if (!feat_view_ok(b, hw, ldc, ldb, k) || !grad_rows_ok(dfeat, lddf, k, 16)) return RGDA_ERR_ARG;
    if ((uintptr_t)ws & 255) return RGDA_ERR_ARG;
    const SawPlan p = make_plan(b, hw, k, C);
    if (ws_bytes < (dfeat ? p.bytes : p.bytes_loss)) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    char* w = (char*)ws;
    int* flag = (int*)w;
    signed char* tab = (signed char*)(w + p.off_tab);
    float* sv = (float*)(w + p.off_s);
    float* lpart = (float*)(w + p.off_lpart);
    int* ch = (int*)(w + p.off_ch);
    float* wgh = (float*)(w + p.off_wgh);
    int* inv = (int*)(w + p.off_inv);
    float* slot = dfeat ? (float*)(w + p.off_slot) : nullptr;
    const FeatView f{feat, (long long)ldc, (long long)ldb, hw, b * hw};
    if (zero_bytes(w, 256, stream) != RGDA_OK) return RGDA_ERR_LAUNCH;
    saw_plan_kernel<<<dim3(cdiv(k, 16), C), 256, 0, st>>>(cls_w, (long long)ldw, sel, k, C, p.G, flag, ch, wgh, inv);
    RGDA_CHECK_LAUNCH();
    const float coef = (float)((double)weight / ((double)b * p.nod * (double)(hw - 1)));
    const int grid = (int)p.jobs;
    switch (C) {
        case 2: saw_gram_kernel<2><<<grid, 256, 0, st>>>(f, ch, wgh, p.G, p.jobs, margin, coef, tab, p.TS, sv, lpart, slot); break;
        case 4: saw_gram_kernel<4><<<grid, 256, 0, st>>>(f, ch, wgh, p.G, p.jobs, margin, coef, tab, p.TS, sv, lpart, slot); break;
        case 6: saw_gram_kernel<6><<<grid, 256, 0, st>>>(f, ch, wgh, p.G, p.jobs, margin, coef, tab, p.TS, sv, lpart, slot); break;
        case 8: saw_gram_kernel<8><<<grid, 256, 0, st>>>(f, ch, wgh, p.G, p.jobs, margin, coef, tab, p.TS, sv, lpart, slot); break;
        default: saw_gram_kernel<16><<<grid, 256, 0, st>>>(f, ch, wgh, p.G, p.jobs, margin, coef, tab, p.TS, sv, lpart, slot); break;
    }
    RGDA_CHECK_LAUNCH();
    if (rows_loss_sum(lpart, (int)p.jobs, loss, weight / (float)b, st) != RGDA_OK) return RGDA_ERR_LAUNCH;
    if (!dfeat) return RGDA_OK;
    const int tiles = cdiv(hw, 64);
    saw_grad_kernel<<<dim3(b * tiles, cdiv(k, 64)), 256, 0, st>>>(inv, tab, p.TS, slot, C, p.G, k, hw, tiles, (bf16_t*)dfeat,
                                                                  lddf, accumulate);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
