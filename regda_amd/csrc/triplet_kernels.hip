// Batch-hard triplet loss (regda/gast/triple.py::TripletLoss, Hermans et al., arXiv:1703.07737): forward + feature
// gradient in one call.  The n x n distance matrix is never stored; deterministic (no floating-point atomics, every
// reduction in a fixed order).  The arithmetic contract is written next to rgda_triplet_loss in include/rgda_hip.h.
//
//   stage  : Xf = the f32 rows, pixel-major [NP][k]; Xh = bf16(Xf); lab = int32 labels, TP_NONE for ignored rows and the
//            padding; NP = n rounded up to 128, the padding zero                               tp_stage_kernel
//   sq     : s_i = sum_c Xh_ic^2, one wavefront per row                                       rows_sumsq
//   mine   : one wavefront per 128 x 128 tile (I, J) of ALL T x T tiles: G = Xh[I] Xh[J]^T in registers; a lane holds one
//            column (an anchor of J) and 64 rows (candidates of I), so the search over the candidates runs in registers
//            and ends with ONE exchange between the two half-waves: (max, argmax | same label), (min, argmin | other
//            label) per (tile row I, anchor) -> part                                          tp_mine_kernel
//   final  : one wavefront per anchor: the T partials combined (ties to the lowest index) -> p, n; the two selected
//            distances recomputed from the f32 rows; clamp, sqrt, hinge                        tp_final_kernel
//   loss   : m, the number of active hinges, loss[0] += weight * sum hinge / m, one workgroup  tp_loss_kernel
//   grad   : one workgroup per row r: the anchors that selected r are found by scanning the target tables (ballots into
//            an LDS bit mask) and added in ascending anchor order                              tp_grad_kernel
// The feature view and the row norms are those of feat_rows.h; the stage tile here is f32 with two pixel-major outputs
// and the labels, so it stays its own.
#include "feat_rows.h"

namespace {

constexpr int TP_MAX_ROWS = 16384;
constexpr int TP_NONE = (int)0x80000000;     // staged label of a row that takes no part
constexpr float TP_CLAMP = 1e-12f;
constexpr int TP_LIST = 1024;                // anchors per target row listed in LDS (more: the mask is walked instead)

struct TpPlan {
    int n, np, T;
    size_t off_lab, off_s, off_p, off_n, off_tp, off_tn, off_dp, off_dn, off_h, off_part, off_xh, off_xf, bytes;
};

TpPlan make_plan(int n, int k) {
    TpPlan p;
    p.n = n;
    p.np = (n + CT - 1) / CT * CT;
    p.T = p.np / CT;
    const size_t v = a256((size_t)p.np * 4);
    size_t o = 256;                            // the stats block
    p.off_lab = o;  o += v;
    p.off_s = o;    o += v;
    p.off_p = o;    o += v;
    p.off_n = o;    o += v;
    p.off_tp = o;   o += v;
    p.off_tn = o;   o += v;
    p.off_dp = o;   o += v;
    p.off_dn = o;   o += v;
    p.off_h = o;    o += v;
    p.off_part = o; o += a256((size_t)16 * p.T * p.np);
    p.off_xh = o;   o += a256((size_t)p.np * k * 2);
    p.off_xf = o;   o += a256((size_t)p.np * k * 4);
    p.bytes = o;
    return p;
}

struct Pick {
    float v;
    int i;
};
// the better of two (value, index) candidates of a maximum (MAX) or minimum search; index < 0: no candidate.  Equal
// values go to the lower index, so the operator is associative and commutative and any combination order gives the same
// pair.
template <bool MAX>
__device__ __forceinline__ Pick pick(Pick a, Pick b) {
    const bool better = MAX ? b.v > a.v : b.v < a.v;
    const bool take = b.i >= 0 && (a.i < 0 || better || (b.v == a.v && b.i < a.i));
    return take ? b : a;
}
template <bool MAX>
__device__ __forceinline__ Pick wave_pick(Pick a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Pick b;
        b.v = __shfl_xor(a.v, o, 64);
        b.i = __shfl_xor(a.i, o, 64);
        a = pick<MAX>(a, b);
    }
    return a;
}

}  // namespace

// 64 rows x 64 channels per workgroup: the strided feature rows -> Xf (f32) and Xh (bf16), pixel-major, through LDS;
// the padding rows as zeros.  The workgroups of the first channel block also stage the labels.
__global__ void __launch_bounds__(256) tp_stage_kernel(FeatView f, const int64_t* __restrict__ labels, int has_ignore, int ignore_label,
                                                       int n, int np, int k, float* __restrict__ xf, bf16_t* __restrict__ xh,
                                                       int* __restrict__ lab) {
    __shared__ float tile[64][65];
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int r = r0 + tx;
    if (blockIdx.y == 0 && ty == 0) {
        int l = TP_NONE;
        if (r < n) {
            const int64_t v = labels[r];
            if (!(has_ignore && v == (int64_t)ignore_label)) l = (int)v;
        }
        lab[r] = l;
    }
    const int rc = min(r, n - 1);
    for (int cc = ty; cc < 64; cc += 4) {
        const int c = c0 + cc;
        if (c < k) tile[tx][cc] = r < n ? feat_at(f, rc, c) : 0.f;
    }
    __syncthreads();
    const int c = c0 + tx;
    if (c < k)
        for (int rr = ty; rr < 64; rr += 4) {
            const float v = tile[rr][tx];
            xf[(size_t)(r0 + rr) * k + c] = v;
            xh[(size_t)(r0 + rr) * k + c] = f2bf(v);
        }
}

// job = I * T + J, one wavefront each.  Candidates are the 128 rows of tile I (the P operand), anchors the 128 rows of
// tile J (the Q operand): lane l holds the anchors J 128 + 32 j + (l & 31), j < 4, and of each the 64 candidates
// I 128 + 32 i + (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) in ascending order.  d2 = (s_i + s_j) - 2 G_ij.
// part: four [T][NP] tables (max value, max index, min value, min index), index -1 where the tile holds no candidate.
__global__ void __launch_bounds__(256, 1) tp_mine_kernel(const bf16_t* __restrict__ xh, const float* __restrict__ s,
                                                         const int* __restrict__ lab, int np, int k, int T,
                                                         float* __restrict__ pmaxv, int* __restrict__ pmaxi,
                                                         float* __restrict__ pminv, int* __restrict__ pmini) {
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (job >= T * T) return;
    const int I = job / T, J = job - I * T;
    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x16{};
    tile_nt<4>(xh, k, I * CT, np - 1, xh, k, J * CT, np - 1, 0, k, acc);
    const int h = lane >> 5;
    int la[4];
    float sa[4];
    Pick mx[4], mn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = J * CT + 32 * j + (lane & 31);
        la[j] = lab[col];
        sa[j] = s[col];
        mx[j] = Pick{-INFINITY, -1};
        mn[j] = Pick{INFINITY, -1};
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = I * CT + 32 * i + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            const int lc = lab[row];
            const float sc = s[row];
            if (lc != TP_NONE) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d2 = __fsub_rn(__fadd_rn(sc, sa[j]), __fmul_rn(2.f, acc[i][j][reg]));
                    if (lc == la[j]) {
                        if (mx[j].i < 0 || d2 > mx[j].v) mx[j] = Pick{d2, row};
                    } else {
                        if (mn[j].i < 0 || d2 < mn[j].v) mn[j] = Pick{d2, row};
                    }
                }
            }
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        Pick o;
        o.v = __shfl_xor(mx[j].v, 32, 64);
        o.i = __shfl_xor(mx[j].i, 32, 64);
        const Pick a = pick<true>(mx[j], o);
        o.v = __shfl_xor(mn[j].v, 32, 64);
        o.i = __shfl_xor(mn[j].i, 32, 64);
        const Pick b = pick<false>(mn[j], o);
        if (h == 0) {
            const size_t e = (size_t)I * np + J * CT + 32 * j + lane;
            pmaxv[e] = a.v;
            pmaxi[e] = a.i;
            pminv[e] = b.v;
            pmini[e] = b.i;
        }
    }
}

// one wavefront per anchor r < NP.  A row without a label (ignored, padding) and an anchor without a negative take no
// part: hinge 0, no targets.  Otherwise the squared distances to p and n are direct fp32 sums over the f32 rows (lane l
// accumulates the channels l + 64 t in order with a fused multiply-add, then the butterfly).
//   P, N   : the selected indices (-1: none)          TP, TN : the same where the pair carries gradient, else -1
//   DP, DN : d_ap, d_an where the pair carries gradient, else 0          H : the hinge where it is positive, else 0
__global__ void __launch_bounds__(256) tp_final_kernel(const float* __restrict__ xf, const int* __restrict__ lab,
                                                       const float* __restrict__ pmaxv, const int* __restrict__ pmaxi,
                                                       const float* __restrict__ pminv, const int* __restrict__ pmini,
                                                       int np, int k, int T, float margin, int* __restrict__ P,
                                                       int* __restrict__ N, int* __restrict__ TP, int* __restrict__ TN,
                                                       float* __restrict__ DP, float* __restrict__ DN, float* __restrict__ H) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= np) return;
    Pick mx{-INFINITY, -1}, mn{INFINITY, -1};
    if (lab[r] != TP_NONE) {
        for (int I = lane; I < T; I += 64) {
            const size_t e = (size_t)I * np + r;
            mx = pick<true>(mx, Pick{pmaxv[e], pmaxi[e]});
            mn = pick<false>(mn, Pick{pminv[e], pmini[e]});
        }
    }
    mx = wave_pick<true>(mx);
    mn = wave_pick<false>(mn);
    const int p = mx.i, q = mn.i;
    float dp = 0.f, dn = 0.f, hinge = 0.f;
    int tp = -1, tn = -1;
    if (p >= 0 && q >= 0) {
        const float* xr = xf + (size_t)r * k;
        const float* xp = xf + (size_t)p * k;
        const float* xq = xf + (size_t)q * k;
        float sp = 0.f, sn = 0.f;
        for (int c = lane; c < k; c += 64) {
            const float x = xr[c], a = x - xp[c], b = x - xq[c];
            sp = __fmaf_rn(a, a, sp);
            sn = __fmaf_rn(b, b, sn);
        }
        sp = wave_sum(sp);
        sn = wave_sum(sn);
        const float d_ap = sqrtf(fmaxf(sp, TP_CLAMP)), d_an = sqrtf(fmaxf(sn, TP_CLAMP));
        const float hg = d_ap - d_an + margin;
        if (hg > 0.f) {
            hinge = hg;
            if (sp >= TP_CLAMP) { dp = d_ap; tp = p; }
            if (sn >= TP_CLAMP) { dn = d_an; tn = q; }
        }
    }
    if (lane == 0) {
        P[r] = p;
        N[r] = q;
        TP[r] = tp;
        TN[r] = tn;
        DP[r] = dp;
        DN[r] = dn;
        H[r] = hinge;
    }
}

// m = the anchors with a negative, act = the positive hinges, loss[0] += weight * sum H / m: 256 strided partials, a
// butterfly per wavefront, then (w0 + w1) + (w2 + w3).  stats[0] = m, stats[1] = act.
__global__ void __launch_bounds__(256) tp_loss_kernel(const int* __restrict__ N, const float* __restrict__ H, int n,
                                                      float weight, float* __restrict__ loss, int* __restrict__ stats) {
    __shared__ float red[3][4];
    float sum = 0.f, m = 0.f, act = 0.f;            // counts up to 16384 are exact in fp32
    for (int i = threadIdx.x; i < n; i += 256) {
        const float hv = H[i];
        sum += hv;
        m += N[i] >= 0 ? 1.f : 0.f;
        act += hv > 0.f ? 1.f : 0.f;
    }
    sum = wave_sum(sum);
    m = wave_sum(m);
    act = wave_sum(act);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = sum;
        red[1][threadIdx.x >> 6] = m;
        red[2][threadIdx.x >> 6] = act;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float S = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const float M = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const float A = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
        stats[0] = (int)M;
        stats[1] = (int)A;
        if (M > 0.f) loss[0] += weight * (S / M);
    }
}

// one workgroup per gradient row r < n, thread t the channels t + 256 u.  With c = weight / m:
//   g  = (c / DP_r) (x_r - x_p) - (c / DN_r) (x_r - x_n)                      the row's own anchor
//   g -= (c / DP_i) (x_i - x_r)   for every anchor i != r with TP_i = r       } in ascending i, the two kinds
//   g += (c / DN_i) (x_i - x_r)   for every anchor i with TN_i = r            } interleaved
// The anchors are found with one pass over TP / TN: the ballots of 64 anchors each go to an LDS bit mask, then into an
// ordered list (entry: i, bit 31 set for a positive); a row selected by more than TP_LIST anchors walks the mask.
__global__ void __launch_bounds__(256) tp_grad_kernel(const float* __restrict__ xf, const int* __restrict__ TP,
                                                      const int* __restrict__ TN, const float* __restrict__ DP,
                                                      const float* __restrict__ DN, const int* __restrict__ stats,
                                                      float weight, int np, int k, bf16_t* __restrict__ out, int ld,
                                                      int accumulate) {
    __shared__ unsigned long long mp[TP_MAX_ROWS / 64], mq[TP_MAX_ROWS / 64];
    __shared__ int cnt[TP_MAX_ROWS / 64];
    __shared__ unsigned list[TP_LIST];
    __shared__ int total_s;
    const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int words = np >> 6;
    for (int base = 0; base < np; base += 256) {
        const int i = base + tid;
        const bool in = i < np;
        const unsigned long long bp = __ballot(in && i != r && TP[i] == r);
        const unsigned long long bq = __ballot(in && TN[i] == r);
        if (lane == 0 && (base >> 6) + wave < words) {
            mp[(base >> 6) + wave] = bp;
            mq[(base >> 6) + wave] = bq;
        }
    }
    __syncthreads();
    if (tid < words) cnt[tid] = __popcll(mp[tid] | mq[tid]);
    __syncthreads();
    if (tid < words) {
        int off = 0;
        for (int w = 0; w < tid; ++w) off += cnt[w];
        if (tid == words - 1) total_s = off + cnt[tid];
        const unsigned long long wp = mp[tid];
        unsigned long long both = wp | mq[tid];
        while (both && off < TP_LIST) {
            const int b = __ffsll((long long)both) - 1;
            both &= both - 1;
            list[off++] = (unsigned)(tid * 64 + b) | (((wp >> b) & 1ull) ? 0x80000000u : 0u);
        }
    }
    __syncthreads();
    const int total = total_s;
    const int m = stats[0];
    const float c = m > 0 ? weight / (float)m : 0.f;
    const int p = TP[r], q = TN[r];
    const bool own = p >= 0 || q >= 0;
    const bool any = m > 0 && (own || total > 0);
    if (accumulate && !any) return;
    const float cp = p >= 0 ? c / DP[r] : 0.f, cq = q >= 0 ? c / DN[r] : 0.f;
    const float* xr = xf + (size_t)r * k;
    const float* xp = xf + (size_t)max(p, 0) * k;
    const float* xq = xf + (size_t)max(q, 0) * k;
    bf16_t* orow = out + (size_t)r * ld;
    for (int ch = tid; ch < k; ch += 256) {
        float g = 0.f;
        if (any) {
            const float x = xr[ch];
            if (p >= 0) g = __fmul_rn(cp, x - xp[ch]);
            if (q >= 0) g = __fmaf_rn(-cq, x - xq[ch], g);
            if (total <= TP_LIST) {
                for (int e = 0; e < total; ++e) {
                    const unsigned ent = list[e];
                    const int i = (int)(ent & 0x7fffffffu);
                    const float d = xf[(size_t)i * k + ch] - x;
                    g = (ent >> 31) ? __fmaf_rn(-(c / DP[i]), d, g) : __fmaf_rn(c / DN[i], d, g);
                }
            } else {
                for (int w = 0; w < words; ++w) {
                    const unsigned long long wp = mp[w];
                    unsigned long long both = wp | mq[w];
                    while (both) {
                        const int b = __ffsll((long long)both) - 1;
                        both &= both - 1;
                        const int i = w * 64 + b;
                        const float d = xf[(size_t)i * k + ch] - x;
                        g = ((wp >> b) & 1ull) ? __fmaf_rn(-(c / DP[i]), d, g) : __fmaf_rn(c / DN[i], d, g);
                    }
                }
            }
            if (accumulate) g += bf2f(orow[ch]);
        }
        orow[ch] = f2bf(g);
    }
}

extern "C" size_t rgda_triplet_loss_workspace(int n, int k) {
    if (n < 2 || n > TP_MAX_ROWS || k < 32 || (k & 31)) return 0;
    return make_plan(n, k).bytes;
}

extern "C" int rgda_triplet_loss(const float* feat, int b, int hw, int64_t ldc, int64_t ldb, const int64_t* labels, int k,
                                 float margin, int has_ignore, int ignore_label, float* loss, void* dfeat, int lddf,
                                 int accumulate, float weight, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (!feat || !labels || !loss || !ws || ((uintptr_t)ws & 255)) return RGDA_ERR_ARG;
    if (b <= 0 || hw <= 0 || k < 32 || (k & 31) || !(margin >= 0.f)) return RGDA_ERR_ARG;
    if (!feat_view_ok(b, hw, ldc, ldb, k) || !grad_rows_ok(dfeat, lddf, k, 16)) return RGDA_ERR_ARG;
    const long long nl = (long long)b * hw;
    if (nl < 2) return RGDA_ERR_ARG;
    if (nl > TP_MAX_ROWS) return RGDA_ERR_UNSUPPORTED;
    const int n = (int)nl;
    const TpPlan p = make_plan(n, k);
    if (ws_bytes < p.bytes) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    char* wsp = (char*)ws;
    int* stats = (int*)wsp;
    int* lab = (int*)(wsp + p.off_lab);
    float* s = (float*)(wsp + p.off_s);
    int* P = (int*)(wsp + p.off_p);
    int* N = (int*)(wsp + p.off_n);
    int* TP = (int*)(wsp + p.off_tp);
    int* TN = (int*)(wsp + p.off_tn);
    float* DP = (float*)(wsp + p.off_dp);
    float* DN = (float*)(wsp + p.off_dn);
    float* H = (float*)(wsp + p.off_h);
    const size_t tn = (size_t)p.T * p.np;
    float* pmaxv = (float*)(wsp + p.off_part);
    int* pmaxi = (int*)(pmaxv + tn);
    float* pminv = (float*)(pmaxi + tn);
    int* pmini = (int*)(pminv + tn);
    bf16_t* xh = (bf16_t*)(wsp + p.off_xh);
    float* xf = (float*)(wsp + p.off_xf);
    const int np = p.np, T = p.T;
    tp_stage_kernel<<<dim3(np / 64, cdiv(k, 64)), 256, 0, st>>>(FeatView{feat, (long long)ldc, (long long)ldb, hw, n}, labels,
                                                                has_ignore, ignore_label, n, np, k, xf, xh, lab);
    RGDA_CHECK_LAUNCH();
    if (rows_sumsq(xh, np, k, s, st) != RGDA_OK) return RGDA_ERR_LAUNCH;
    tp_mine_kernel<<<cdiv((long long)T * T, 4), 256, 0, st>>>(xh, s, lab, np, k, T, pmaxv, pmaxi, pminv, pmini);
    RGDA_CHECK_LAUNCH();
    tp_final_kernel<<<np / 4, 256, 0, st>>>(xf, lab, pmaxv, pmaxi, pminv, pmini, np, k, T, margin, P, N, TP, TN, DP, DN, H);
    RGDA_CHECK_LAUNCH();
    tp_loss_kernel<<<1, 256, 0, st>>>(N, H, n, weight, loss, stats);
    RGDA_CHECK_LAUNCH();
    if (!dfeat) return RGDA_OK;
    tp_grad_kernel<<<n, 256, 0, st>>>(xf, TP, TN, DP, DN, stats, weight, np, k, (bf16_t*)dfeat, lddf, accumulate);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
