// loss_calc(multi=True) with the losses of the --ls / --lt flags (tools/train_ssl_reg.py:52-63,134-158):
// CrossEntropy (rgda_upsample_ce; regda/utils/tools.py:240-254, regda/gast/balance.py:88-101) and OhemCrossEntropy,
// FocalLoss, GHMLoss, UPSLoss, UVEMLoss (rgda_upsample_loss; balance.py:104-216,306-435).
//
// Every one of them is a per-pixel function of the bilinearly upsampled logits.  One row-per-workgroup upsample /
// log-softmax / horizontal-contraction pass computes the loss and d loss / d logits; except for CE and focal the gradient
// also depends on a statistic of the whole batch (a count, a histogram, a k-th largest value), so the row pass runs twice
// around a global stage.  CE is the stat-less kind: grad, col and reduce only, no header, no scratch.
//   stat     (one workgroup per output row; not for CE / focal): the per-pixel decision value -- OHEM: the (class-weighted)
//            CE, GHM: the bucket of |p_y - 1|, UPS / UVEM: the uncertainty weight of the soft label -- goes to scratch;
//            counts and the GHM histograms go to integer atomics (order-independent, so deterministic)
//   finalize (one workgroup): denominators, the GHM acc_sum EMA (head 1, then head 2), the OHEM branch
//   select   (OHEM only, six passes that return at once unless the top-k branch is taken): radix select of the n_min-th
//            largest 64-bit key (f32 bits of the loss : inverted pixel index); keys are unique, so exactly n_min pixels
//            are kept and of equal losses the lowest pixel index goes first
//   grad     (one workgroup per output row): the logits again, the per-pixel weight from scratch and the global scalars,
//            per-row loss partials, d loss / d logits contracted horizontally
//   col / reduce: vertical contraction; fixed-order double reduction of the row partials.
// No float atomics anywhere; nothing is read back to the host.
//
// GDPLoss (rgda_upsample_gdp; balance.py:218-303) runs on the same passes: GHM's stat pass as it is (the same |p_y - 1|,
// bins and edges), a global stage of its own (symmetrised histogram, acc_sum EMA, bin weights) and the GDP branch of the
// grad pass, whose per-pixel weight is the bin weight + the optional prototype weight + the optional class weight.
//
// IAST's entropy / KLD region regularisers (rgda_upsample_reg; regda/utils/tools.py:376-398) are a row pass of their own
// on the same staging, contraction and reduction, behind a count pass for their two denominators (at the end of this file).
#include "common.h"
#include <cmath>

namespace {

constexpr int KIND_CE = 0;               // rgda_upsample_ce: a kind of this file only, not an rgda_loss_kind
constexpr size_t MAX_ROW_LDS = RGDA_LOSS_ROW_LDS_MAX;   // dynamic LDS of the grad pass: the widest row served
constexpr int GHM_BINS = 30;
constexpr int SEL_PASSES = 6;
constexpr int SEL_BINS = 2048;
// radix digits of the 64-bit OHEM key, from the top: the loss bits in 11 + 11 + 10, the inverted index in 11 + 11 + 10
__constant__ int kSelShift[SEL_PASSES] = {53, 42, 32, 21, 10, 0};
__constant__ int kSelWidth[SEL_PASSES] = {11, 11, 10, 11, 11, 10};

// Counters and histograms are spread over CNT_REPL copies (workgroup i adds to copy i % CNT_REPL): thousands of
// workgroups adding to ONE address serialise on it.  finalize sums the copies (integers: any order gives the same total).
constexpr int CNT_REPL = 64;
enum { CNT_VALID, CNT_LIT, CNT_U, CNT_KEPT0, CNT_KEPT1, CNT_SLOTS = 8 };

struct LossHdr {
    // zeroed at the start of every call (up to `cut`)
    int cnt[CNT_REPL][CNT_SLOTS];        // label != ignore_label; label != -1 (GHMLoss's denominator uses the literal,
                                         // balance.py:214); u <= t && valid (UPS / UVEM); OHEM: loss > thresh per head
    int ghm_hist[CNT_REPL][2][32];
    int sel_active[2];                   // OHEM: the top-k branch is still being resolved
    int sel_arrived[SEL_PASSES][2];
    int sel_hist[SEL_PASSES][2][SEL_BINS];
    // written by finalize / select
    unsigned long long cut[2];           // OHEM: a pixel is kept iff its key >= cut
    unsigned long long prefix[2];
    int rem[2];
    float denom[2];
    float acc[2][32];                    // GHM acc_sum after the head-1 and after the head-2 update
    float bw[2][32];                     // GDP bins_weight of the head-1 and of the head-2 call
};

struct LossParams {
    float thresh;                        // OHEM
    float m, t, cl, cr, inv_gamma;       // UPS / UVEM
    float gamma;                         // focal
    float mom, omm;                      // GHM
    float gscale;                        // CE: 0.5 / #pixels (mean over all pixels, then over the two heads)
};

static size_t align256_(size_t x) { return (x + 255) & ~(size_t)255; }

static size_t scratch_bytes(int kind, size_t n) {
    switch (kind) {
        case RGDA_LOSS_OHEM: return 2 * n * 4;
        case RGDA_LOSS_GHM:
        case RGDA_LOSS_GDP: return 2 * n;
        case RGDA_LOSS_UPS:
        case RGDA_LOSS_UVEM: return n * 4;
        default: return 0;
    }
}

// the upsampled logits z of one head at one output pixel and their maximum m, from the two low-res rows staged in LDS
template <int C>
__device__ __forceinline__ void up_logits(const float* rows, int w, int hd, const Lerp& ly, const Lerp& lx, float z[C],
                                          float& m) {
    m = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* r = rows + ((hd * C + c) * 2) * w;
        float top = __fadd_rn(__fmul_rn(lx.l0, r[lx.i0]), __fmul_rn(lx.l1, r[lx.i1]));
        float bot = __fadd_rn(__fmul_rn(lx.l0, r[w + lx.i0]), __fmul_rn(lx.l1, r[w + lx.i1]));
        z[c] = __fadd_rn(__fmul_rn(ly.l0, top), __fmul_rn(ly.l1, bot));
        m = fmaxf(m, z[c]);
    }
}

// the softmax of the upsampled logits z of one head at one output pixel:
// m = max z, e = exp(z - m), se = sum e (classes in order), zl = z of class li
template <int C>
__device__ __forceinline__ void up_softmax(const float* rows, int w, int hd, const Lerp& ly, const Lerp& lx, int li,
                                           float& m, float e[C], float& se, float& zl) {
    float z[C];
    up_logits<C>(rows, w, hd, ly, lx, z, m);
    se = 0.f;
    zl = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { e[c] = expf(z[c] - m); se += e[c]; zl = (c == li) ? z[c] : zl; }
}

// the vertical interpolation of output row Y: lerp_ac with its rounding spelled out.  FUSED: l1 = fma(scale, Y, -i0), one
// rounding (the OHEM..UVEM kinds); else l1 = f32(scale * Y) - i0 (CE).  Which of the two the compiler made of lerp_ac
// depended on where it placed the code; fixed here, every kind keeps its bits.
template <bool FUSED>
__device__ __forceinline__ Lerp row_lerp(int Y, int h, int H) {
#pragma clang fp contract(off)
    const float scale = (H > 1) ? __fdiv_rn((float)(h - 1), (float)(H - 1)) : 0.f;
    const float src = scale * (float)Y;
    Lerp r;
    r.i0 = (int)src;
    r.i1 = r.i0 + ((r.i0 < h - 1) ? 1 : 0);
    r.l1 = FUSED ? __builtin_fmaf(scale, (float)Y, -(float)r.i0) : src - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

// rows[2 heads][C][2][w]: the low-res rows y0, y1 of both heads
template <int C>
__device__ __forceinline__ void stage_rows(float* rows, const float* p1, const float* p2, int b, int y0, int y1, int h,
                                           int w) {
    const int hw = h * w;
    for (int i = threadIdx.x; i < 2 * C * 2 * w; i += 256) {
        int x = i % w, r = (i / w) & 1, c = (i / (2 * w)) % C, hd = i / (2 * w * C);
        const float* p = hd ? p2 : p1;
        rows[i] = p[((size_t)b * C + c) * hw + (r ? y1 : y0) * w + x];
    }
}

// UVEMLoss.get_weight (balance.py:398-426) in f32, branch for branch; NaN u (a soft label with an exact 0) falls through
// to the right branch at x = 0, as in the reference
__device__ __forceinline__ float uvem_weight(float u, const LossParams& p) {
    float left = 1.f;
    if (p.m > 0.f) {
        float d = __fsub_rn((u <= p.m && u >= 0.f) ? u : 1.f, p.m);
        float wl = __fadd_rn(__fmul_rn(p.cl, __fmul_rn(d, d)), 1.f);
        left = powf(fminf(fmaxf(wl, 0.f), 1.f), p.inv_gamma);
    }
    float right = 0.f;
    if (p.m < p.t) {
        float d = __fsub_rn((u > p.m && u <= p.t) ? u : 0.f, p.m);
        float wr = __fadd_rn(__fmul_rn(p.cr, __fmul_rn(d, d)), 1.f);
        right = powf(fminf(fmaxf(wr, 0.f), 1.f), p.inv_gamma);
    }
    float wgt = (u <= p.m) ? left : right;
    return (u >= p.t) ? 0.f : wgt;
}

// torch.bucketize(g, edges, right=False): the number of edges below g; edges = f32(k / 30), the last one f32(1 + 1e-3)
__device__ __forceinline__ int ghm_bucket(float g, const float* edges) {
    int k = (g > 0.f) ? min((int)__fmul_rn(g, (float)GHM_BINS), GHM_BINS) : 0;
    while (k <= GHM_BINS && edges[k] < g) ++k;
    while (k > 0 && !(edges[k - 1] < g)) --k;
    return k;
}

// ---------------------------------------------------------------------------------------------------- stat pass
template <int KIND, int C>
__global__ void __launch_bounds__(256) loss_stat_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                        const int64_t* __restrict__ label, const float* __restrict__ soft,
                                                        const float* __restrict__ class_weight, LossHdr* hdr,
                                                        void* scratch, int h, int w, int H, int W, int ignore_label,
                                                        LossParams prm) {
    extern __shared__ float rows[];
    __shared__ int s_cnt[3], s_kept[2], s_hist[2][32];
    __shared__ float s_edges[GHM_BINS + 1];
    const int b = blockIdx.y, Y = blockIdx.x;
    const size_t n = (size_t)gridDim.y * H * W;
    const Lerp ly = row_lerp<true>(Y, h, H);
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 2) s_kept[threadIdx.x] = 0;
    if (threadIdx.x < 64) s_hist[threadIdx.x >> 5][threadIdx.x & 31] = 0;
    if (KIND == RGDA_LOSS_GHM && threadIdx.x <= GHM_BINS)
        s_edges[threadIdx.x] = threadIdx.x < GHM_BINS ? (float)((double)threadIdx.x / GHM_BINS) : (float)(1.0 + 1e-3);
    if (KIND == RGDA_LOSS_OHEM || KIND == RGDA_LOSS_GHM) stage_rows<C>(rows, p1, p2, b, ly.i0, ly.i1, h, w);
    __syncthreads();
    int valid_n = 0, lit_n = 0, u_n = 0, kept0 = 0, kept1 = 0;
    for (int X = threadIdx.x; X < W; X += 256) {
        const size_t pix = ((size_t)b * H + Y) * W + X;
        const long long lab = label[pix];
        const bool valid = lab != ignore_label;
        const int li = valid ? (int)lab : 0;
        valid_n += valid;
        lit_n += lab != -1;
        if constexpr (KIND == RGDA_LOSS_OHEM || KIND == RGDA_LOSS_GHM) {
            const Lerp lx = lerp_ac(X, w, W);
#pragma unroll
            for (int hd = 0; hd < 2; ++hd) {
                float m, e[C], se, zl;
                up_softmax<C>(rows, w, hd, ly, lx, li, m, e, se, zl);
                if constexpr (KIND == RGDA_LOSS_OHEM) {
                    // CE as log_softmax + nll: log(se) - (z_l - max) >= 0, ignored pixels 0; times the class weight
                    float ce = valid ? logf(se) - (zl - m) : 0.f;
                    float v = valid ? ce * (class_weight ? class_weight[hd * C + li] : 1.f) : 0.f;
                    ((float*)scratch)[hd * n + pix] = v;
                    if (v > prm.thresh) { if (hd == 0) ++kept0; else ++kept1; }
                } else {
                    float py = 0.f;
#pragma unroll
                    for (int c = 0; c < C; ++c) py = (c == li) ? e[c] / se : py;
                    float g = valid ? fabsf(py - 1.f) : -1.f;
                    if (g >= 0.f && g <= 1.f) atomicAdd(&s_hist[hd][min((int)__fmul_rn(g, (float)GHM_BINS), GHM_BINS - 1)], 1);
                    ((uint8_t*)scratch)[hd * n + pix] = (uint8_t)ghm_bucket(g, s_edges);
                }
            }
        } else {            // UPS / UVEM: u = sum_c -s log s of the soft label at full resolution
            float u = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float s = soft[(((size_t)b * C + c) * H + Y) * W + X];
                u += (-s) * logf(s);
            }
            u_n += (u <= prm.t) && valid;
            float f = (u > prm.t) ? 0.f : (KIND == RGDA_LOSS_UVEM ? uvem_weight(u, prm) : 1.f);
            ((float*)scratch)[pix] = f;
        }
    }
    if (valid_n) atomicAdd(&s_cnt[0], valid_n);
    if (lit_n) atomicAdd(&s_cnt[1], lit_n);
    if (u_n) atomicAdd(&s_cnt[2], u_n);
    if (kept0) atomicAdd(&s_kept[0], kept0);
    if (kept1) atomicAdd(&s_kept[1], kept1);
    __syncthreads();
    const int rep = (blockIdx.y * gridDim.x + blockIdx.x) % CNT_REPL;
    if (threadIdx.x == 0) {
        int* cnt = hdr->cnt[rep];
        atomicAdd(&cnt[CNT_VALID], s_cnt[0]);
        atomicAdd(&cnt[CNT_LIT], s_cnt[1]);
        atomicAdd(&cnt[CNT_U], s_cnt[2]);
        atomicAdd(&cnt[CNT_KEPT0], s_kept[0]);
        atomicAdd(&cnt[CNT_KEPT1], s_kept[1]);
    }
    if (KIND == RGDA_LOSS_GHM && threadIdx.x < 64) {
        const int v = s_hist[threadIdx.x >> 5][threadIdx.x & 31];
        if (v) atomicAdd(&hdr->ghm_hist[rep][threadIdx.x >> 5][threadIdx.x & 31], v);
    }
}

// ---------------------------------------------------------------------------------------------------- global stage
__global__ void __launch_bounds__(64) loss_finalize_kernel(int kind, int heads, LossHdr* hdr, float* acc_sum,
                                                           LossParams prm, long long npix) {
    const int t = threadIdx.x;
    if (kind == RGDA_LOSS_GHM && t < GHM_BINS) {
        // acc_sum = momentum * acc_sum + (1 - momentum) * histc(g), once per head (balance.py:201-204); one head: the
        // second "head" is the same prediction and reuses the first state
        float a = acc_sum[t];
        for (int hd = 0; hd < heads; ++hd) {
            int n = 0;
            for (int r = 0; r < CNT_REPL; ++r) n += hdr->ghm_hist[r][hd][t];
            const float bins = (float)n;
            a = prm.mom > 0.f ? __fadd_rn(__fmul_rn(prm.mom, a), __fmul_rn(prm.omm, bins)) : bins;
            hdr->acc[hd][t] = a;
        }
        if (heads == 1) hdr->acc[1][t] = a;
        acc_sum[t] = a;
    }
    __shared__ int s_tot[CNT_SLOTS];
    if (t < CNT_SLOTS) {
        int n = 0;
        for (int r = 0; r < CNT_REPL; ++r) n += hdr->cnt[r][t];
        s_tot[t] = n;
    }
    __syncthreads();
    if (t >= 2) return;
    float denom = 0.f;
    if (kind == RGDA_LOSS_OHEM) {
        const int n_min = s_tot[CNT_VALID] / 5;
        const int kept = s_tot[CNT_KEPT0 + t];
        if (kept < n_min) {              // loss.topk(n_min) (balance.py:130-131)
            hdr->sel_active[t] = 1;
            hdr->rem[t] = n_min;
            hdr->prefix[t] = 0ull;
            denom = (float)n_min;
        } else {                         // loss[loss > thresh]: key >= (bits(thresh) + 1) : 0
            hdr->cut[t] = (unsigned long long)(__float_as_uint(prm.thresh) + 1u) << 32;
            denom = (float)kept;         // 0 when every label is ignored: NaN loss, zero gradient
        }
    } else if (kind == RGDA_LOSS_FOCAL) {
        denom = (float)npix;
    } else if (kind == RGDA_LOSS_GHM) {
        denom = __fadd_rn((float)s_tot[CNT_LIT], 1e-7f);
    } else {
        denom = __fadd_rn((float)s_tot[CNT_U], 1e-7f);
    }
    hdr->denom[t] = denom;
}

// GDPLoss's global stage (balance.py:261-270,290-295), one workgroup.  Per head call, head 1 first:
//   bins = (histc(g) + flip(histc(g))) * 0.5;  acc_sum = momentum * acc_sum + (1 - momentum) * bins  (momentum 0: bins)
//   bins_weight = where(acc_sum != 0, 1 - acc_sum / (sum(acc_sum) + 1e-7), 0) / (max + 1e-7)
// The 30-element sum is taken in double in bin order and rounded once, the maximum in bin order: every lane of the
// first wave walks the same staged values, so all of them hold the same bits.  One head: the second "head" is the same
// prediction and reuses the first state, as in GHM.
__global__ void __launch_bounds__(64) gdp_finalize_kernel(int heads, LossHdr* hdr, float* acc_sum, float* bins_weight,
                                                          LossParams prm) {
    const int t = threadIdx.x;
    __shared__ float s_a[GHM_BINS], s_b[GHM_BINS];
    float a = t < GHM_BINS ? acc_sum[t] : 0.f, bw = 0.f;
    for (int hd = 0; hd < heads; ++hd) {
        if (t < GHM_BINS) {
            int n = 0, nf = 0;
            for (int r = 0; r < CNT_REPL; ++r) { n += hdr->ghm_hist[r][hd][t]; nf += hdr->ghm_hist[r][hd][GHM_BINS - 1 - t]; }
            const float bins = __fmul_rn(__fadd_rn((float)n, (float)nf), 0.5f);
            a = prm.mom > 0.f ? __fadd_rn(__fmul_rn(prm.mom, a), __fmul_rn(prm.omm, bins)) : bins;
            s_a[t] = a;
        }
        __syncthreads();
        double tot = 0.0;
        for (int i = 0; i < GHM_BINS; ++i) tot += (double)s_a[i];
        const float den = __fadd_rn((float)tot, 1e-7f);
        const float v = (t < GHM_BINS && a != 0.f) ? __fsub_rn(1.f, __fdiv_rn(a, den)) : 0.f;
        if (t < GHM_BINS) s_b[t] = v;
        __syncthreads();
        float mx = s_b[0];
        for (int i = 1; i < GHM_BINS; ++i) mx = fmaxf(mx, s_b[i]);
        bw = __fdiv_rn(v, __fadd_rn(mx, 1e-7f));
        if (t < 32) hdr->bw[hd][t] = t < GHM_BINS ? bw : 0.f;
        __syncthreads();
    }
    if (t < 32 && heads == 1) hdr->bw[1][t] = t < GHM_BINS ? bw : 0.f;
    if (t < GHM_BINS) { acc_sum[t] = a; bins_weight[t] = bw; }
    if (t < 2) {                         // the denominator is GHM's: #(label != -1) + 1e-7 (balance.py:284)
        int n = 0;
        for (int r = 0; r < CNT_REPL; ++r) n += hdr->cnt[r][CNT_LIT];
        hdr->denom[t] = __fadd_rn((float)n, 1e-7f);
    }
}

// One radix pass of the OHEM top-k: histogram of one digit of the keys that match the prefix resolved so far; the last
// workgroup to arrive finds the digit of the rem-th largest key.  Keys: f32 bits of the loss (>= 0, so the bit pattern
// is monotone) in the high word, n - 1 - pixel index in the low word: unique, ties of the loss go to the lower index.
__global__ void __launch_bounds__(256) ohem_select_kernel(LossHdr* hdr, const float* __restrict__ vbuf, long long n,
                                                          int pass) {
    const int hd = blockIdx.y;
    if (!hdr->sel_active[hd]) return;    // the threshold branch, or resolved by an earlier pass
    __shared__ int hist[SEL_BINS];
    __shared__ int s_last;
    const int shift = kSelShift[pass], width = kSelWidth[pass], top = shift + width;
    const unsigned long long pre = hdr->prefix[hd];
    const unsigned mask = (1u << width) - 1u;
    for (int i = threadIdx.x; i < SEL_BINS; i += 256) hist[i] = 0;
    __syncthreads();
    const float* v = vbuf + (size_t)hd * n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(v[i]) << 32) | (unsigned)(n - 1 - i);
        if (top == 64 || (key >> top) == (pre >> top)) atomicAdd(&hist[(unsigned)(key >> shift) & mask], 1);
    }
    __syncthreads();
    int* gh = hdr->sel_hist[pass][hd];
    for (int i = threadIdx.x; i <= (int)mask; i += 256)
        if (hist[i]) atomicAdd(&gh[i], hist[i]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();                 // release: this workgroup's histogram adds before its arrival
        s_last = atomicAdd(&hdr->sel_arrived[pass][hd], 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();                     // acquire: every workgroup's adds are visible
    // thread t owns the eight digits below nb - 8 t (from the top); a block scan finds the one whose count crosses rem
    const int nb = (int)mask + 1, t = threadIdx.x;
    int cnt[8], s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int d = nb - 1 - (8 * t + j);
        cnt[j] = d >= 0 ? __hip_atomic_load(&gh[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        s += cnt[j];
    }
    int* sc = hist;
    sc[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = t >= off ? sc[t - off] : 0;
        __syncthreads();
        sc[t] += add;
        __syncthreads();
    }
    const int incl = sc[t], excl = incl - s, rem = hdr->rem[hd];
    if (excl < rem && rem <= incl) {
        int above = excl, j = 0;
        for (; j < 7; ++j) {
            if (above + cnt[j] >= rem) break;
            above += cnt[j];
        }
        const int d = nb - 1 - (8 * t + j);
        const int left = rem - above;
        const unsigned long long prefix = pre | ((unsigned long long)d << shift);
        if (cnt[j] == left || pass == SEL_PASSES - 1) {
            hdr->cut[hd] = prefix;       // every key of this digit is needed: the smallest one with the prefix
            hdr->sel_active[hd] = 0;
        } else {
            hdr->prefix[hd] = prefix;
            hdr->rem[hd] = left;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- grad pass
// T[b][Y][hd][c][x] = sum_X G[hd][c][X] * Rx[X][x], the horizontal interpolation of every output column read back from
// lxi / lxl: recomputing lerp_ac here (an IEEE divide each) cost 13 000 calls per workgroup -- more than the per-pixel
// loss arithmetic
template <int C>
__device__ __forceinline__ void contract_row(const float* G, const int* lxi, const float* lxl, float* T, int b, int Y,
                                             int w, int H, int W) {
    const float inv_scale = (w > 1) ? (float)(W - 1) / (float)(w - 1) : 0.f;
    for (int o = threadIdx.x; o < 2 * C * w; o += 256) {
        int x = o % w, hc = o / w;
        int lo = (w > 1) ? max(0, (int)floorf((float)(x - 1) * inv_scale) - 1) : 0;
        int hi = (w > 1) ? min(W - 1, (int)ceilf((float)(x + 1) * inv_scale) + 1) : W - 1;
        float acc = 0.f;
        for (int X = lo; X <= hi; ++X) {
            const int i0 = lxi[X], i1 = i0 + ((i0 < w - 1) ? 1 : 0);
            const float l1 = lxl[X], l0 = __fsub_rn(1.f, l1);
            float wt = ((i0 == x) ? l0 : 0.f) + ((i1 == x) ? l1 : 0.f);
            acc += wt * G[hc * W + X];
        }
        T[(((size_t)b * H + Y) * 2 * C + hc) * w + x] = acc;
    }
}

// dynamic LDS: rows[2 heads][c][2][w] | G[2][c][W] (with gradients) | lxi[W] | lxl[W]
static size_t grad_lds(int c, int w, int W, bool want) {
    return ((size_t)2 * c * 2 * w + (want ? (size_t)2 * c * W : 0) + (size_t)2 * W) * 4;
}

template <int KIND, int C>
__global__ void __launch_bounds__(256) loss_grad_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                        const int64_t* __restrict__ label,
                                                        const float* __restrict__ class_weight,
                                                        const float* __restrict__ pixel_weight,
                                                        const LossHdr* __restrict__ hdr, const void* __restrict__ scratch,
                                                        float* partial, float* T, int h, int w, int H, int W,
                                                        int ignore_label, LossParams prm, int want_grad) {
    extern __shared__ float lds[];
    float* rows = lds;
    float* G = lds + 2 * C * 2 * w;
    int* lxi = (int*)(G + (want_grad ? 2 * C * W : 0));
    float* lxl = (float*)(lxi + W);
    __shared__ float s_acc[2][32];
    const int b = blockIdx.y, Y = blockIdx.x;
    const size_t n = (size_t)gridDim.y * H * W;
    const Lerp ly = row_lerp<KIND != KIND_CE>(Y, h, H);
    if (KIND == RGDA_LOSS_GHM && threadIdx.x < 64) s_acc[threadIdx.x >> 5][threadIdx.x & 31] = hdr->acc[threadIdx.x >> 5][threadIdx.x & 31];
    if (KIND == RGDA_LOSS_GDP && threadIdx.x < 64) s_acc[threadIdx.x >> 5][threadIdx.x & 31] = hdr->bw[threadIdx.x >> 5][threadIdx.x & 31];
    // GDP: the number of weight terms, 1 + prototype_refine + class_balance (balance.py:283)
    const float gdp_div = 1.f + (pixel_weight ? 1.f : 0.f) + (class_weight ? 1.f : 0.f);
    stage_rows<C>(rows, p1, p2, b, ly.i0, ly.i1, h, w);
    float inv_d0 = 0.f, inv_d1 = 0.f;    // CE has no header
    unsigned long long cut0 = 0ull, cut1 = 0ull;
    if constexpr (KIND != KIND_CE) {
        inv_d0 = 1.f / hdr->denom[0], inv_d1 = 1.f / hdr->denom[1];
        cut0 = hdr->cut[0], cut1 = hdr->cut[1];
    }
    __syncthreads();
    float lsum0 = 0.f, lsum1 = 0.f;
    for (int X = threadIdx.x; X < W; X += 256) {
        const Lerp lx = lerp_ac(X, w, W);
        lxi[X] = lx.i0;
        lxl[X] = lx.l1;
        const size_t pix = ((size_t)b * H + Y) * W + X;
        const long long lab = label[pix];
        const bool valid = lab != ignore_label;
        const int li = valid ? (int)lab : 0;
        float f = 0.f;
        if constexpr (KIND == RGDA_LOSS_UPS || KIND == RGDA_LOSS_UVEM) f = ((const float*)scratch)[pix];
        if constexpr (KIND == RGDA_LOSS_GDP) f = pixel_weight ? pixel_weight[pix] : 0.f;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            float m, e[C], se, zl;
            up_softmax<C>(rows, w, hd, ly, lx, li, m, e, se, zl);
            float lp, gs;                // this pixel's term of the head's loss sum, d(call loss) / d ce
            if constexpr (KIND == KIND_CE) {
                // the CE arithmetic of its own: lse - z_l, not the generic log(se) - (z_l - m) below (other rounding)
                const float lse = m + logf(se);
                const float wgt = valid ? (class_weight ? class_weight[hd * C + li] : 1.f) : 0.f;
                lp = valid ? (lse - zl) * wgt : 0.f;
                gs = wgt * prm.gscale;
            } else {
                const float ce = valid ? logf(se) - (zl - m) : 0.f;
                const float cw = (valid && class_weight) ? class_weight[hd * C + li] : 1.f;
                const float inv_d = hd ? inv_d1 : inv_d0;
                float dce;               // d(head loss) / d ce
                if constexpr (KIND == RGDA_LOSS_OHEM) {
                    const float v = ((const float*)scratch)[hd * n + pix];
                    const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)(n - 1 - pix);
                    const bool sel = key >= (hd ? cut1 : cut0);
                    lp = sel ? v : 0.f;
                    dce = sel ? cw * inv_d : 0.f;
                } else if constexpr (KIND == RGDA_LOSS_FOCAL) {
                    // (1 - pt)^gamma * ce, pt = exp(-ce); d/d ce = (1 - pt)^gamma + gamma (1 - pt)^(gamma - 1) pt ce
                    const float pt = expf(-ce), q = 1.f - pt;
                    const float qg = prm.gamma == 2.f ? q * q : powf(q, prm.gamma);
                    // gamma == 0 is the plain CE: the second term is 0 for every q, also at q == 0 (a CE of exactly 0),
                    // where powf(0, -1) = inf would make it 0 * inf; torch's pow backward gives 0 there too
                    const float qg1 = prm.gamma == 2.f ? q : (prm.gamma == 0.f ? 0.f : powf(q, prm.gamma - 1.f));
                    lp = qg * ce;
                    dce = (qg + prm.gamma * qg1 * pt * ce) * inv_d;
                } else if constexpr (KIND == RGDA_LOSS_GHM) {
                    const int ind = ((const uint8_t*)scratch)[hd * n + pix];
                    const float wg = (ind > 0 && ind <= GHM_BINS) ? 1.f / s_acc[hd][ind - 1] : 0.f;
                    lp = ce * wg;
                    dce = wg * inv_d;
                } else if constexpr (KIND == RGDA_LOSS_GDP) {
                    // weight_bins (+ weight_prototype) (+ class weight), in the reference's order (balance.py:277-283);
                    // a pixel with p_y == 1 exactly has bucket 0: counted in the histogram, bin weight 0
                    const int ind = ((const uint8_t*)scratch)[hd * n + pix];
                    float wp = (ind > 0 && ind <= GHM_BINS) ? s_acc[hd][ind - 1] : 0.f;
                    if (pixel_weight) wp = __fadd_rn(wp, f);
                    if (class_weight) wp = __fadd_rn(wp, valid ? cw : 0.f);
                    lp = __fdiv_rn(__fmul_rn(ce, wp), gdp_div);
                    dce = __fdiv_rn(wp, gdp_div) * inv_d;
                } else {                 // UPS / UVEM: f = 0 where u > t (the gated CE), the uncertainty weight else
                    const float wt = f * cw;
                    lp = wt * ce;
                    dce = wt * inv_d;
                }
                gs = valid ? dce * 0.5f : 0.f;                        // / num heads (tools.py:252)
            }
            if (hd == 0) lsum0 += lp; else lsum1 += lp;
            if (want_grad) {
#pragma unroll
                for (int c = 0; c < C; ++c) G[(hd * C + c) * W + X] = (e[c] / se - ((c == li) ? 1.f : 0.f)) * gs;
            }
        }
    }
    __shared__ float red[2][4];
    lsum0 = wave_sum(lsum0); lsum1 = wave_sum(lsum1);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lsum0; red[1][threadIdx.x >> 6] = lsum1; }
    __syncthreads();
    if (threadIdx.x < 2)
        partial[((size_t)b * H + Y) * 2 + threadIdx.x] =
            red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    if (!want_grad) return;
    contract_row<C>(G, lxi, lxl, T, b, Y, w, H, W);
}

// vertical contraction T -> g[head][b][c][y][x]; ACC (rgda_upsample_reg, accumulate): one f32 add of the finished value
// onto what g holds
template <int C, bool ACC>
__device__ __forceinline__ void col_contract(const float* __restrict__ T, float* g1, float* g2, int b_n, int h, int w,
                                             int H) {
    int i = blockIdx.x * 256 + threadIdx.x;
    int total = 2 * b_n * C * h * w;
    if (i >= total) return;
    int x = i % w, y = (i / w) % h, c = (i / (w * h)) % C, b = (i / (w * h * C)) % b_n, hd = i / (w * h * C * b_n);
    const float inv_scale = (h > 1) ? (float)(H - 1) / (float)(h - 1) : 0.f;
    int lo = (h > 1) ? max(0, (int)floorf((float)(y - 1) * inv_scale) - 1) : 0;
    int hi = (h > 1) ? min(H - 1, (int)ceilf((float)(y + 1) * inv_scale) + 1) : H - 1;
    float acc = 0.f;
    for (int Y = lo; Y <= hi; ++Y) {
        Lerp ly = lerp_ac(Y, h, H);
        float wt = ((ly.i0 == y) ? ly.l0 : 0.f) + ((ly.i1 == y) ? ly.l1 : 0.f);
        acc += wt * T[(((size_t)b * H + Y) * 2 * C + hd * C + c) * w + x];
    }
    float* g = (hd ? g2 : g1) + (((size_t)b * C + c) * h + y) * w + x;
    *g = ACC ? __fadd_rn(*g, acc) : acc;
}
template <int C, bool ACC = false>
__global__ void __launch_bounds__(256) loss_col_kernel(const float* __restrict__ T, float* g1, float* g2, int b_n, int h,
                                                       int w, int H) {
    col_contract<C, ACC>(T, g1, g2, b_n, h, w, H);
}
// the accumulate variant behind a device-side gate: *live == 0 leaves g1, g2 untouched (x + 0 is not x for x = -0)
template <int C>
__global__ void __launch_bounds__(256) loss_col_gated_kernel(const float* __restrict__ T, float* g1, float* g2, int b_n,
                                                             int h, int w, int H, const int* __restrict__ live) {
    if (*live == 0) return;
    col_contract<C, true>(T, g1, g2, b_n, h, w, H);
}

// per head: the row partials in a fixed order in double, / the head's denominator -- CE (no header): * 1 / #pixels,
// torch.mean; then the mean over the two heads
__global__ void __launch_bounds__(256) loss_reduce_kernel(const float* __restrict__ partial, const LossHdr* hdr,
                                                          double inv_npix, float* loss, int n) {
    __shared__ double red[2][256];
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { s0 += partial[2 * i]; s1 += partial[2 * i + 1]; }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float l0, l1;
        if (hdr) {
            l0 = (float)(red[0][0] / (double)hdr->denom[0]), l1 = (float)(red[1][0] / (double)hdr->denom[1]);
        } else {
            l0 = (float)(red[0][0] * inv_npix), l1 = (float)(red[1][0] * inv_npix);
        }
        loss[0] = (l0 + l1) / 2.f;
    }
}

// dynamic LDS above 64 KB needs the kernel's attribute raised first (as label_kernels.hip does for pearson_sim_kernel)
static int lds_attr(const void* kernel, size_t lds) {
    if (lds <= 64 * 1024) return RGDA_OK;
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess ? RGDA_OK
                                                                                                            : RGDA_ERR_LAUNCH;
}

// one call's operands and the workspace pieces its entry point laid out (hdr and scratch: null for CE)
struct LossCall {
    const float *p1, *p2, *soft, *class_weight;
    const int64_t* label;
    float *acc_sum, *loss, *g1, *g2;
    const float* pixel_weight;           // GDP
    float* bins_weight;                  // GDP
    LossHdr* hdr;
    void* scratch;
    float *partial, *T;
    int heads, b, h, w, H, W, ignore_label;
    LossParams prm;
};

// the passes of one call, in stream order
template <int KIND, int C>
static int run_passes(const LossCall& a, rgda_stream_t stream) {
    hipStream_t st = to_stream(stream);
    const int want = a.g1 != nullptr;
    const long long n = (long long)a.b * a.H * a.W;
    const dim3 rows_grid(a.H, a.b);
    if constexpr (KIND != KIND_CE) {
        if constexpr (KIND != RGDA_LOSS_FOCAL) {
            constexpr bool uv = KIND == RGDA_LOSS_UPS || KIND == RGDA_LOSS_UVEM;
            const size_t zero = KIND == RGDA_LOSS_OHEM ? offsetof(LossHdr, cut) : offsetof(LossHdr, sel_arrived);
            if (zero_bytes(a.hdr, zero, stream) != RGDA_OK) return RGDA_ERR_LAUNCH;
            const size_t lds = uv ? 0 : (size_t)2 * C * 2 * a.w * 4;
            // GDP's statistic pass is GHM's, the same instantiation
            constexpr int STAT = KIND == RGDA_LOSS_GDP ? (int)RGDA_LOSS_GHM : KIND;
            if (lds_attr((const void*)loss_stat_kernel<STAT, C>, lds) != RGDA_OK) return RGDA_ERR_LAUNCH;
            loss_stat_kernel<STAT, C><<<rows_grid, 256, lds, st>>>(a.p1, a.p2, a.label, a.soft, a.class_weight, a.hdr,
                                                                a.scratch, a.h, a.w, a.H, a.W, a.ignore_label, a.prm);
            RGDA_CHECK_LAUNCH();
        }
        if constexpr (KIND == RGDA_LOSS_GDP)
            gdp_finalize_kernel<<<1, 64, 0, st>>>(a.heads, a.hdr, a.acc_sum, a.bins_weight, a.prm);
        else
            loss_finalize_kernel<<<1, 64, 0, st>>>(KIND, a.heads, a.hdr, a.acc_sum, a.prm, n);
        RGDA_CHECK_LAUNCH();
        if constexpr (KIND == RGDA_LOSS_OHEM) {
            const int blocks = (int)min((long long)cdiv(n, 256 * 8), 512ll);
            for (int pass = 0; pass < SEL_PASSES; ++pass) {
                ohem_select_kernel<<<dim3(blocks, 2), 256, 0, st>>>(a.hdr, (const float*)a.scratch, n, pass);
                RGDA_CHECK_LAUNCH();
            }
        }
    }
    const size_t lds = grad_lds(C, a.w, a.W, want);
    if (lds_attr((const void*)loss_grad_kernel<KIND, C>, lds) != RGDA_OK) return RGDA_ERR_LAUNCH;
    loss_grad_kernel<KIND, C><<<rows_grid, 256, lds, st>>>(a.p1, a.p2, a.label, a.class_weight, a.pixel_weight, a.hdr,
                                                        a.scratch, a.partial, a.T, a.h, a.w, a.H, a.W, a.ignore_label, a.prm, want);
    RGDA_CHECK_LAUNCH();
    if (want) {
        loss_col_kernel<C><<<cdiv((long long)2 * a.b * C * a.h * a.w, 256), 256, 0, st>>>(a.T, a.g1, a.g2, a.b, a.h, a.w,
                                                                                       a.H);
        RGDA_CHECK_LAUNCH();
    }
    loss_reduce_kernel<<<1, 256, 0, st>>>(a.partial, a.hdr, 1.0 / (double)n, a.loss, a.b * a.H);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

template <int C>
static int run_kind(int kind, const LossCall& a, rgda_stream_t stream) {
    switch (kind) {
        case KIND_CE: return run_passes<KIND_CE, C>(a, stream);
        case RGDA_LOSS_OHEM: return run_passes<RGDA_LOSS_OHEM, C>(a, stream);
        case RGDA_LOSS_FOCAL: return run_passes<RGDA_LOSS_FOCAL, C>(a, stream);
        case RGDA_LOSS_GHM: return run_passes<RGDA_LOSS_GHM, C>(a, stream);
        case RGDA_LOSS_UPS: return run_passes<RGDA_LOSS_UPS, C>(a, stream);
        case RGDA_LOSS_UVEM: return run_passes<RGDA_LOSS_UVEM, C>(a, stream);
        case RGDA_LOSS_GDP: return run_passes<RGDA_LOSS_GDP, C>(a, stream);
        default: return RGDA_ERR_ARG;
    }
}

// the class counts served: common.h, class_count_ok
static int run_kind(int kind, int c, const LossCall& a, rgda_stream_t stream) {
    return with_classes(c, [&](auto cc) { return run_kind<decltype(cc)::value>(kind, a, stream); });
}

// ------------------------------------------------------------------------ entropy / KLD regularisers (rgda_upsample_reg)
// IAST's region regularisers (regda/utils/tools.py:376-398) on the row pass above:
//   count    #(w_e > 0), #(w_k > 0) over the batch: integer atomics over CNT_REPL copies
//   grad     one workgroup per output row: the upsampled logits, log p = (z - m) - log(sum e) (never log(p): a
//            probability that underflows gives 0 * finite = 0), the four row partials (term x head), d / d logits
//            contracted horizontally
//   col / reduce: as above (col with the accumulate variant).
struct RegHdr {
    int cnt[CNT_REPL][2];                // w_e > 0, w_k > 0
};

struct RegParams {
    float se, sk;                        // lambda * 0.5 (the mean over the two heads); 0 for a term that is off
    int terms, empty_is_zero, ignore_label;
};

// a pixel's two weights: the caller's map, or derived from the label (entropy: ignored pixels, KLD: labelled pixels)
__device__ __forceinline__ void reg_weights(const int64_t* __restrict__ label, const float* __restrict__ w_ent,
                                            const float* __restrict__ w_kld, size_t pix, const RegParams& prm, float& we,
                                            float& wk) {
    const bool need_label = ((prm.terms & RGDA_REG_ENT) && !w_ent) || ((prm.terms & RGDA_REG_KLD) && !w_kld);
    const bool ignored = need_label ? label[pix] == prm.ignore_label : false;
    we = (prm.terms & RGDA_REG_ENT) ? (w_ent ? w_ent[pix] : (ignored ? 1.f : 0.f)) : 0.f;
    wk = (prm.terms & RGDA_REG_KLD) ? (w_kld ? w_kld[pix] : (ignored ? 0.f : 1.f)) : 0.f;
}

__global__ void __launch_bounds__(256) reg_count_kernel(const int64_t* __restrict__ label, const float* __restrict__ w_ent,
                                                        const float* __restrict__ w_kld, RegHdr* hdr, long long n,
                                                        RegParams prm) {
    __shared__ int s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int ne = 0, nk = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float we, wk;
        reg_weights(label, w_ent, w_kld, (size_t)i, prm, we, wk);
        ne += we > 0.f;
        nk += wk > 0.f;
    }
    if (ne) atomicAdd(&s_cnt[0], ne);
    if (nk) atomicAdd(&s_cnt[1], nk);
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&hdr->cnt[blockIdx.x % CNT_REPL][threadIdx.x], s_cnt[threadIdx.x]);
}

// the two denominators from the copies (any order: integers), by every workgroup that needs them; s_tot: int[2] in LDS,
// valid after the caller's next barrier
__device__ __forceinline__ void reg_totals(const RegHdr* __restrict__ hdr, int* s_tot) {
    if (threadIdx.x < 2) {
        int n = 0;
        for (int r = 0; r < CNT_REPL; ++r) n += hdr->cnt[r][threadIdx.x];
        s_tot[threadIdx.x] = n;
    }
}

template <int C>
__global__ void __launch_bounds__(256) reg_grad_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                       const int64_t* __restrict__ label, const float* __restrict__ w_ent,
                                                       const float* __restrict__ w_kld, const RegHdr* __restrict__ hdr,
                                                       float* partial, float* T, int h, int w, int H, int W, RegParams prm,
                                                       int want_grad) {
    extern __shared__ float lds[];
    float* rows = lds;
    float* G = lds + 2 * C * 2 * w;
    int* lxi = (int*)(G + (want_grad ? 2 * C * W : 0));
    float* lxl = (float*)(lxi + W);
    __shared__ int s_tot[2];
    const int b = blockIdx.y, Y = blockIdx.x;
    const Lerp ly = row_lerp<false>(Y, h, H);
    reg_totals(hdr, s_tot);
    stage_rows<C>(rows, p1, p2, b, ly.i0, ly.i1, h, w);
    __syncthreads();
    // an empty region: 1 / 0 = inf and 0 * inf = NaN as the reference's 0 / 0, or a term of exactly 0
    const float inv_de = (s_tot[0] == 0 && prm.empty_is_zero) ? 0.f : 1.f / (float)s_tot[0];
    const float inv_dk = (s_tot[1] == 0 && prm.empty_is_zero) ? 0.f : 1.f / (float)s_tot[1];
    const float ge = (prm.terms & RGDA_REG_ENT) ? prm.se * inv_de : 0.f;
    const float gk = (prm.terms & RGDA_REG_KLD) ? prm.sk * inv_dk : 0.f;
    constexpr float inv_c = 1.f / (float)C;
    float lsum[4] = {0.f, 0.f, 0.f, 0.f};       // entropy head 1, 2; KLD head 1, 2
    for (int X = threadIdx.x; X < W; X += 256) {
        const Lerp lx = lerp_ac(X, w, W);
        lxi[X] = lx.i0;
        lxl[X] = lx.l1;
        const size_t pix = ((size_t)b * H + Y) * W + X;
        float we, wk;
        reg_weights(label, w_ent, w_kld, pix, prm, we, wk);
        const float ae = we * ge, ak = wk * gk;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            float z[C], e[C], m, se = 0.f;
            up_logits<C>(rows, w, hd, ly, lx, z, m);
#pragma unroll
            for (int c = 0; c < C; ++c) { z[c] -= m; e[c] = expf(z[c]); se += e[c]; }
            const float lg = logf(se), inv_se = 1.f / se;
            float ent = 0.f, sl = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                z[c] -= lg;              // log p
                e[c] *= inv_se;          // p
                ent -= e[c] * z[c];
                sl += z[c];
            }
            lsum[hd] += we * ent;
            lsum[2 + hd] += wk * (-sl * inv_c);
            if (want_grad) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    G[(hd * C + c) * W + X] = ae * (-e[c] * (z[c] + ent)) + ak * (e[c] - inv_c);
            }
        }
    }
    __shared__ float red[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lsum[k] = wave_sum(lsum[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = lsum[k];
    }
    __syncthreads();
    if (threadIdx.x < 4)
        partial[((size_t)b * H + Y) * 4 + threadIdx.x] =
            red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    if (!want_grad) return;
    contract_row<C>(G, lxi, lxl, T, b, Y, w, H, W);
}

// per term and head: the row partials in a fixed order in double, / the term's count; then the mean over the heads
__global__ void __launch_bounds__(256) reg_reduce_kernel(const float* __restrict__ partial, const RegHdr* __restrict__ hdr,
                                                         float* loss, int n, RegParams prm) {
    __shared__ double red[4][256];
    __shared__ int s_tot[2];
    reg_totals(hdr, s_tot);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256)
        for (int k = 0; k < 4; ++k) s[k] += partial[4 * (size_t)i + k];
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 2) {
        const int t = threadIdx.x;
        float v = 0.f;
        if ((prm.terms & (t ? RGDA_REG_KLD : RGDA_REG_ENT)) && !(s_tot[t] == 0 && prm.empty_is_zero)) {
            const double d = (double)s_tot[t];
            v = ((float)(red[2 * t][0] / d) + (float)(red[2 * t + 1][0] / d)) / 2.f;
        }
        loss[t] = v;
    }
}

struct RegCall {
    const float *p1, *p2, *w_ent, *w_kld;
    const int64_t* label;
    float *loss, *g1, *g2;
    RegHdr* hdr;
    float *partial, *T;
    int b, h, w, H, W, accumulate;
    RegParams prm;
};

template <int C>
static int run_reg(const RegCall& a, rgda_stream_t stream) {
    hipStream_t st = to_stream(stream);
    const int want = a.g1 != nullptr;
    const long long n = (long long)a.b * a.H * a.W;
    if (zero_bytes(a.hdr, sizeof(RegHdr), stream) != RGDA_OK) return RGDA_ERR_LAUNCH;
    reg_count_kernel<<<(int)min((long long)cdiv(n, 256 * 8), 1024ll), 256, 0, st>>>(a.label, a.w_ent, a.w_kld, a.hdr, n, a.prm);
    RGDA_CHECK_LAUNCH();
    const size_t lds = grad_lds(C, a.w, a.W, want);
    if (lds_attr((const void*)reg_grad_kernel<C>, lds) != RGDA_OK) return RGDA_ERR_LAUNCH;
    reg_grad_kernel<C><<<dim3(a.H, a.b), 256, lds, st>>>(a.p1, a.p2, a.label, a.w_ent, a.w_kld, a.hdr, a.partial, a.T, a.h, a.w,
                                                      a.H, a.W, a.prm, want);
    RGDA_CHECK_LAUNCH();
    if (want) {
        const int blocks = cdiv((long long)2 * a.b * C * a.h * a.w, 256);
        if (a.accumulate)
            loss_col_kernel<C, true><<<blocks, 256, 0, st>>>(a.T, a.g1, a.g2, a.b, a.h, a.w, a.H);
        else
            loss_col_kernel<C, false><<<blocks, 256, 0, st>>>(a.T, a.g1, a.g2, a.b, a.h, a.w, a.H);
        RGDA_CHECK_LAUNCH();
    }
    reg_reduce_kernel<<<1, 256, 0, st>>>(a.partial, a.hdr, a.loss, a.b * a.H, a.prm);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

// ------------------------------------------------------------------------ PyCDA region pyramid term (rgda_upsample_pycda)
// The student's mean prediction over every square region of a pyramid must match the teacher's label distribution of
// that region (the contract: include/rgda_hip.h).  Every level's regions are unions of whole base cells, squares of
// min(sizes[0], 8) pixels, so the per-pixel work happens once and the pyramid is sums of cells:
//   cell     one workgroup per band of base-cell rows and 256 columns: q = softmax(upsampled logits) per head and the
//            clamped soft label in 2^24 fixed point, summed over each cell's pixels: across the cell's lanes by DPP, down
//            its rows in the registers of the cell's owner lane, written once with plain stores
//   pyramid  one launch per step of the chain base -> sizes[...] -> image (steps of at most x4, so a region sums at most 16
//            children, in row-major order, one thread per sum): f64 sums of q, int64 sums of the targets
//   count    n_l, the regions with an active class: integer compares, integer atomics
//   coef     per (region, head, class): the loss term and a = -w_l T / (max(n_l, 1) |r| (Q + 1e-7)), both in f64;
//            per-workgroup loss partials by a fixed tree
//   push     A[cell][head][class] = sum_l a_l[the cell's region], levels in order
//   reduce   the partials in a fixed order -> loss[1 + L]
//   grad     the row pass again: dz_k = q_k (A_k - sum_c A_c q_c) * 0.5 weight, contracted horizontally; col as above.
// No float atomics; nothing is read back.
constexpr int PY_MAX_LEVELS = 6;
constexpr int PY_MAX_CHAIN = 24;          // base, <= 6 sizes, the x4 steps between them up to an image side of 2^30
constexpr double PY_FIX = 16777216.0;     // 2^24
constexpr double PY_EPS = 1e-7;

struct PyGeom {
    int b, H, W, nk, L;
    int size[PY_MAX_CHAIN], ry[PY_MAX_CHAIN], rx[PY_MAX_CHAIN];     // the chain: side, regions down and across one image
    long long off[PY_MAX_CHAIN];          // first region of the chain level in lvq / lvt
    int map[PY_MAX_LEVELS];               // level l of the caller -> chain index
    long long coff[PY_MAX_LEVELS];        // first region of level l in coef
    float lw[PY_MAX_LEVELS];
    long long thr_fix;                    // rint(thresh * 2^24)
};

// pixels of region (ry, rx) of a level of side s: border squares are clipped
__device__ __forceinline__ long long py_area(int s, int ry, int rx, int H, int W) {
    const long long y0 = (long long)ry * s, x0 = (long long)rx * s;
    const long long y1 = min(y0 + s, (long long)H), x1 = min(x0 + s, (long long)W);
    return (y1 - y0) * (x1 - x0);
}

// v summed over the aligned group of S = 2 / 4 / 8 lanes, the same bits in every lane of the group (f32 and integer
// addition commute): quad permutes, then the mirror of each half row
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ float group_sum(float v, int S) {
    v += dpp_f<0xB1>(v);                  // quad_perm [1, 0, 3, 2]
    if (S >= 4) v += dpp_f<0x4E>(v);      // quad_perm [2, 3, 0, 1]
    if (S >= 8) v += dpp_f<0x141>(v);     // row_half_mirror
    return v;
}
__device__ __forceinline__ int group_sum(int v, int S) {
    v += dpp_i<0xB1>(v);
    if (S >= 4) v += dpp_i<0x4E>(v);
    if (S >= 8) v += dpp_i<0x141>(v);
    return v;
}

// one workgroup per (band of S rows, image, chunk of 256 columns); a cell's sums live in the registers of its owner lane
template <int C>
__global__ void __launch_bounds__(256) pycda_cell_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                         const float* __restrict__ soft, double* __restrict__ lvq,
                                                         long long* __restrict__ lvt, int* flag, int* n_active,
                                                         int levels, int h, int w, int H, int W, int S, int ncx) {
    extern __shared__ float rows[];
    // the counters of the count pass, which runs behind this one
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < levels) n_active[threadIdx.x] = 0;
    const int band = blockIdx.x, b = blockIdx.y;
    const int X = blockIdx.z * 256 + threadIdx.x;
    const bool in = X < W;
    const bool owner = (threadIdx.x & (S - 1)) == 0;      // 256 % S == 0: X % S == threadIdx.x % S
    const Lerp lx = lerp_ac(in ? X : W - 1, w, W);
    float accq[2][C];
    long long acct[C];
#pragma unroll
    for (int c = 0; c < C; ++c) accq[0][c] = accq[1][c] = 0.f, acct[c] = 0;
    bool bad = false;
    for (int r = 0; r < S; ++r) {
        const int Y = band * S + r;
        if (Y >= H) break;
        const Lerp ly = row_lerp<false>(Y, h, H);
        __syncthreads();                  // the row before is consumed
        stage_rows<C>(rows, p1, p2, b, ly.i0, ly.i1, h, w);
        __syncthreads();
        const float* sp = soft + (((size_t)b * C) * H + Y) * W + (in ? X : 0);
        // every lane of a cell takes part in its sum: lanes past the row's end add 0
#pragma unroll
        for (int c = 0; c < C; ++c) {
            int t = 0;
            if (in) {
                const float s = sp[(size_t)c * H * W];
                bad |= !(s >= 0.f && s <= 1.f);
                t = (int)rintf(__fmul_rn(fminf(fmaxf(s, 0.f), 1.f), 16777216.f));      // fmaxf(NaN, 0) = 0
            }
            acct[c] += group_sum(t, S);
        }
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            float m, e[C], se, zl;
            up_softmax<C>(rows, w, hd, ly, lx, 0, m, e, se, zl);
#pragma unroll
            for (int c = 0; c < C; ++c) accq[hd][c] += group_sum(in ? e[c] / se : 0.f, S);
        }
    }
    if (bad && flag) atomicOr(flag, 1);
    if (!(owner && in)) return;
    const size_t cell = ((size_t)b * gridDim.x + band) * ncx + X / S;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        lvq[cell * 2 * C + c] = (double)accq[0][c];
        lvq[cell * 2 * C + C + c] = (double)accq[1][c];
        lvt[cell * C + c] = acct[c];
    }
}

// chain level k from k - 1: one thread per (region, value), value = 2 C sums of q, then C sums of the targets
__global__ void __launch_bounds__(256) pycda_pyramid_kernel(double* __restrict__ lvq, long long* __restrict__ lvt, PyGeom g,
                                                            int k, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int rxk = g.rx[k], ryk = g.ry[k], rxp = g.rx[k - 1], ryp = g.ry[k - 1];
    if (i >= (long long)g.b * ryk * rxk * 3 * C) return;
    const int j = (int)(i % (3 * C));
    const long long r = i / (3 * C);
    const int rx = (int)(r % rxk), ry = (int)((r / rxk) % ryk), bb = (int)(r / ((long long)rxk * ryk));
    const int f = g.size[k] / g.size[k - 1];
    const int cy1 = (int)min((long long)(ry + 1) * f, (long long)ryp), cx1 = (int)min((long long)(rx + 1) * f, (long long)rxp);
    if (j < 2 * C) {
        const double* src = lvq + g.off[k - 1] * 2 * C + j;
        double s = 0.0;
        for (int cy = ry * f; cy < cy1; ++cy)
            for (int cx = rx * f; cx < cx1; ++cx) s += src[(((long long)bb * ryp + cy) * rxp + cx) * 2 * C];
        lvq[(g.off[k] + r) * 2 * C + j] = s;
    } else {
        const long long* src = lvt + g.off[k - 1] * C + (j - 2 * C);
        long long s = 0;
        for (int cy = ry * f; cy < cy1; ++cy)
            for (int cx = rx * f; cx < cx1; ++cx) s += src[(((long long)bb * ryp + cy) * rxp + cx) * C];
        lvt[(g.off[k] + r) * C + (j - 2 * C)] = s;
    }
}

// n_active[l]: grid (blocks, L), one thread per region
__global__ void __launch_bounds__(256) pycda_count_kernel(const long long* __restrict__ lvt, PyGeom g, int C, int* n_active) {
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int l = blockIdx.y, k = g.map[l];
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r < (long long)g.b * g.ry[k] * g.rx[k]) {
        const int rx = (int)(r % g.rx[k]), ry = (int)((r / g.rx[k]) % g.ry[k]);
        const long long bound = g.thr_fix * py_area(g.size[k], ry, rx, g.H, g.W);
        bool any = false;
        for (int c = 0; c < C; ++c) any |= lvt[(g.off[k] + r) * C + c] > bound;
        if (any) atomicAdd(&s_cnt, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&n_active[l], s_cnt);
}

// grid (blocks, L), one thread per (region, head, class): coef and the workgroup's two loss partials (head 1, head 2)
__global__ void __launch_bounds__(256) pycda_coef_kernel(const double* __restrict__ lvq, const long long* __restrict__ lvt,
                                                         PyGeom g, int C, const int* __restrict__ n_active,
                                                         float* __restrict__ coef, double* __restrict__ ploss) {
    __shared__ double red[2][256];
    const int l = blockIdx.y, k = g.map[l];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    double term = 0.0;
    int hd = 0;
    if (i < (long long)g.b * g.ry[k] * g.rx[k] * 2 * C) {
        const int hc = (int)(i % (2 * C)), c = hc % C;
        hd = hc / C;
        const long long r = i / (2 * C);
        const int rx = (int)(r % g.rx[k]), ry = (int)((r / g.rx[k]) % g.ry[k]);
        const long long area = py_area(g.size[k], ry, rx, g.H, g.W);
        const long long tf = lvt[(g.off[k] + r) * C + c];
        float a = 0.f;
        if (tf > g.thr_fix * area) {
            const double T = (double)tf / ((double)area * PY_FIX);
            const double Q = lvq[(g.off[k] + r) * 2 * C + hc] / (double)area + PY_EPS;
            const double n = (double)max(n_active[l], 1);
            term = -T * log(Q);
            a = (float)(-(double)g.lw[l] * T / (n * (double)area * Q));
        }
        coef[(g.coff[l] + r) * 2 * C + hc] = a;
    }
    red[0][threadIdx.x] = hd == 0 ? term : 0.0;
    red[1][threadIdx.x] = hd == 1 ? term : 0.0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x < 2) ploss[((size_t)l * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = red[threadIdx.x][0];
}

// A[cell][head][class]: one thread per value, the levels added in order
__global__ void __launch_bounds__(256) pycda_push_kernel(const float* __restrict__ coef, PyGeom g, int C, float* __restrict__ A) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)g.b * g.ry[0] * g.rx[0] * 2 * C) return;
    const int hc = (int)(i % (2 * C));
    const long long cell = i / (2 * C);
    const int cx = (int)(cell % g.rx[0]), cy = (int)((cell / g.rx[0]) % g.ry[0]), bb = (int)(cell / ((long long)g.rx[0] * g.ry[0]));
    float acc = 0.f;
    for (int l = 0; l < g.L; ++l) {
        const int k = g.map[l], f = g.size[k] / g.size[0];
        const long long r = ((long long)bb * g.ry[k] + cy / f) * g.rx[k] + cx / f;
        acc += coef[(g.coff[l] + r) * 2 * C + hc];
    }
    A[i] = acc;
}

// loss[0] = total, loss[1 + l] = level l: the partials in a fixed order, / max(n_l, 1), the mean over the heads
__global__ void __launch_bounds__(256) pycda_reduce_kernel(const double* __restrict__ ploss, const int* __restrict__ n_active,
                                                           PyGeom g, int nblk, float* loss) {
    __shared__ double red[2][256];
    __shared__ double s_level[PY_MAX_LEVELS];
    for (int l = 0; l < g.L; ++l) {
        double s0 = 0.0, s1 = 0.0;
        for (int i = threadIdx.x; i < nblk; i += 256) { s0 += ploss[((size_t)l * nblk + i) * 2]; s1 += ploss[((size_t)l * nblk + i) * 2 + 1]; }
        red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const double n = (double)max(n_active[l], 1);
            s_level[l] = 0.5 * (red[0][0] / n + red[1][0] / n);
            loss[1 + l] = (float)s_level[l];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int l = 0; l < g.L; ++l) tot += (double)g.lw[l] * s_level[l];
        loss[0] = (float)tot;
    }
}

template <int C>
__global__ void __launch_bounds__(256) pycda_grad_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                         const float* __restrict__ A, float* T, int h, int w, int H, int W,
                                                         int S, int ncx, int ncy, float gs) {
    extern __shared__ float lds[];
    float* rows = lds;
    float* G = lds + 2 * C * 2 * w;
    int* lxi = (int*)(G + 2 * C * W);
    float* lxl = (float*)(lxi + W);
    const int b = blockIdx.y, Y = blockIdx.x;
    const Lerp ly = row_lerp<false>(Y, h, H);
    stage_rows<C>(rows, p1, p2, b, ly.i0, ly.i1, h, w);
    __syncthreads();
    for (int X = threadIdx.x; X < W; X += 256) {
        const Lerp lx = lerp_ac(X, w, W);
        lxi[X] = lx.i0;
        lxl[X] = lx.l1;
        const float* a = A + (((size_t)b * ncy + Y / S) * ncx + X / S) * 2 * C;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            float m, e[C], se, zl;
            up_softmax<C>(rows, w, hd, ly, lx, 0, m, e, se, zl);
            float ac[C], dot = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) { e[c] = e[c] / se; ac[c] = a[hd * C + c]; dot += ac[c] * e[c]; }
#pragma unroll
            for (int c = 0; c < C; ++c) G[(hd * C + c) * W + X] = e[c] * (ac[c] - dot) * gs;
        }
    }
    __syncthreads();
    contract_row<C>(G, lxi, lxl, T, b, Y, w, H, W);
}

// the chain and the workspace layout of one call; false: sizes outside the contract
struct PyLayout {
    PyGeom g;
    size_t lvq, lvt, coef, A, ploss, T, total;      // byte offsets
    int nblk;                             // workgroups of the coef pass per level
    long long most;                       // regions of the largest level
};

static bool py_layout(int b, int c, int h, int w, int H, int W, const int* sizes, int L, PyLayout& o) {
    if (!sizes || L < 1 || L > PY_MAX_LEVELS || b <= 0 || c <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return false;
    if ((long long)b * H * W >= (1ll << 31)) return false;
    PyGeom& g = o.g;
    g = PyGeom{};
    g.b = b, g.H = H, g.W = W, g.L = L;
    if (max(H, W) > (1 << 30)) return false;
    int img = 2;                          // the image level: the smallest power of two that covers the image
    while (img < max(H, W)) img <<= 1;
    int nk = 0;
    for (int l = 0; l < L; ++l) {
        int s = sizes[l];
        if (s == 0) {
            if (l != L - 1) return false;
            s = img;
        } else {
            if (s < 2 || s > 256 || (s & (s - 1))) return false;
            if (l > 0 && s <= sizes[l - 1]) return false;
        }
        if (nk == 0) g.size[nk++] = min(s, 8);
        while (g.size[nk - 1] < s) {      // steps of at most x4
            if (nk >= PY_MAX_CHAIN) return false;
            g.size[nk] = (int)min((long long)g.size[nk - 1] * 4, (long long)s);
            ++nk;
        }
        g.map[l] = nk - 1;                // an image level no larger than the last finite size is that level
    }
    g.nk = nk;
    long long regions = 0, cregions = 0;
    for (int k = 0; k < nk; ++k) {
        g.ry[k] = (H + g.size[k] - 1) / g.size[k], g.rx[k] = (W + g.size[k] - 1) / g.size[k];
        g.off[k] = regions;
        regions += (long long)b * g.ry[k] * g.rx[k];
    }
    long long most = 0;
    for (int l = 0; l < L; ++l) {
        const long long r = (long long)b * g.ry[g.map[l]] * g.rx[g.map[l]];
        g.coff[l] = cregions;
        cregions += r;
        most = max(most, r);
    }
    o.most = most;
    o.nblk = cdiv(most * 2 * c, 256);
    size_t at = 0;
    o.lvq = at, at += align256_((size_t)regions * 2 * c * 8);
    o.lvt = at, at += align256_((size_t)regions * c * 8);
    o.coef = at, at += align256_((size_t)cregions * 2 * c * 4);
    o.A = at, at += align256_((size_t)b * g.ry[0] * g.rx[0] * 2 * c * 4);
    o.ploss = at, at += align256_((size_t)L * o.nblk * 2 * 8);
    o.T = at, at += (size_t)b * H * 2 * c * w * 4;
    o.total = at;
    return true;
}

struct PyCall {
    const float *p1, *p2, *soft;
    float *loss, *g1, *g2;
    int *n_active, *flag;
    char* ws;
    int h, w, accumulate;
    float gs;
};

template <int C>
static int run_pycda(const PyCall& a, const PyLayout& lay, rgda_stream_t stream) {
    hipStream_t st = to_stream(stream);
    const PyGeom& g = lay.g;
    double* lvq = (double*)(a.ws + lay.lvq);
    long long* lvt = (long long*)(a.ws + lay.lvt);
    float* coef = (float*)(a.ws + lay.coef);
    float* A = (float*)(a.ws + lay.A);
    double* ploss = (double*)(a.ws + lay.ploss);
    float* T = (float*)(a.ws + lay.T);
    const size_t clds = (size_t)2 * C * 2 * a.w * 4;      // the staged rows: within the gradient pass's need, checked there
    if (lds_attr((const void*)pycda_cell_kernel<C>, clds) != RGDA_OK) return RGDA_ERR_LAUNCH;
    pycda_cell_kernel<C><<<dim3(g.ry[0], g.b, cdiv(g.W, 256)), 256, clds, st>>>(a.p1, a.p2, a.soft, lvq, lvt, a.flag, a.n_active,
                                                                               g.L, a.h, a.w, g.H, g.W, g.size[0], g.rx[0]);
    RGDA_CHECK_LAUNCH();
    for (int k = 1; k < g.nk; ++k) {
        pycda_pyramid_kernel<<<cdiv((long long)g.b * g.ry[k] * g.rx[k] * 3 * C, 256), 256, 0, st>>>(lvq, lvt, g, k, C);
        RGDA_CHECK_LAUNCH();
    }
    pycda_count_kernel<<<dim3(cdiv(lay.most, 256), g.L), 256, 0, st>>>(lvt, g, C, a.n_active);
    RGDA_CHECK_LAUNCH();
    pycda_coef_kernel<<<dim3(lay.nblk, g.L), 256, 0, st>>>(lvq, lvt, g, C, a.n_active, coef, ploss);
    RGDA_CHECK_LAUNCH();
    pycda_reduce_kernel<<<1, 256, 0, st>>>(ploss, a.n_active, g, lay.nblk, a.loss);
    RGDA_CHECK_LAUNCH();
    if (!a.g1) return RGDA_OK;
    pycda_push_kernel<<<cdiv((long long)g.b * g.ry[0] * g.rx[0] * 2 * C, 256), 256, 0, st>>>(coef, g, C, A);
    RGDA_CHECK_LAUNCH();
    const size_t lds = grad_lds(C, a.w, g.W, true);
    if (lds_attr((const void*)pycda_grad_kernel<C>, lds) != RGDA_OK) return RGDA_ERR_LAUNCH;
    pycda_grad_kernel<C><<<dim3(g.H, g.b), 256, lds, st>>>(a.p1, a.p2, A, T, a.h, a.w, g.H, g.W, g.size[0], g.rx[0], g.ry[0],
                                                        a.gs);
    RGDA_CHECK_LAUNCH();
    const int blocks = cdiv((long long)2 * g.b * C * a.h * a.w, 256);
    if (a.accumulate)
        loss_col_kernel<C, true><<<blocks, 256, 0, st>>>(T, a.g1, a.g2, g.b, a.h, a.w, g.H);
    else
        loss_col_kernel<C, false><<<blocks, 256, 0, st>>>(T, a.g1, a.g2, g.b, a.h, a.w, g.H);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

// ------------------------------------------------------------------------ region-overlap term (rgda_upsample_overlap)
// Dice / soft Jaccard / Tversky / focal-Tversky of the upsampled logits against hard labels (the contract:
// include/rgda_hip.h): three sums per head and class over the whole batch, and a per-pixel gradient whose two
// coefficients per head and class are functions of those sums.  No per-pixel scratch:
//   stat     one workgroup per output row: q = softmax(upsampled logits) per head in registers, TP / FP / FN per head and
//            class summed per thread, across the wave by DPP (a fixed butterfly), across the four waves in order; one
//            partial of 6 C floats per row with plain stores.  1 - q_y is taken as the sum of the other classes' q: no
//            cancellation.  Y_c per row: integer LDS atomics, plain stores
//   stage    one workgroup: every value's row partials in double, rows in order within contiguous chunks and the chunks
//            in order; T_c, the loss, and per head and class the two coefficients dL/dq for pixels with y == c and for
//            the others, with 0.5 * weight folded in (f64, rounded once)
//   grad     the row pass again: u_c from the coefficient table (scalar loads: SGPR-resident), dz_k = q_k (u_k - sum_c
//            q_c u_c) over valid pixels, contracted horizontally; col as above (accumulate: behind the n > 0 gate).
// No float atomics; nothing is read back.
constexpr int OV_STAGE_THREADS = 1024;
constexpr double OV_EPS = 1e-7;

struct OvParams {
    double alpha, beta, gamma, smooth, gs;
    int heads;
};

// v summed over the wave, the same bits in every lane, without the LDS crossbar
__device__ __forceinline__ float wave_sum_dpp(float v) {
    return xor_add<32>(xor_add<16>(xor_add<8>(group_sum(v, 8))));
}

template <int C>
__global__ void __launch_bounds__(256) overlap_stat_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                           const int64_t* __restrict__ label, float* __restrict__ partial,
                                                           int* __restrict__ ycnt, int* flag, int h, int w, int H, int W,
                                                           int ignore_label) {
    extern __shared__ float rows[];
    __shared__ int s_cnt[C];
    __shared__ float red[4][6 * C];
    const int b = blockIdx.y, Y = blockIdx.x;
    const Lerp ly = row_lerp<false>(Y, h, H);
    if (threadIdx.x < C) s_cnt[threadIdx.x] = 0;
    stage_rows<C>(rows, p1, p2, b, ly.i0, ly.i1, h, w);
    __syncthreads();
    float acc[2][3][C];                   // head x (TP, FP, FN) x class
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[i / 3][i % 3][c] = 0.f;
    bool bad = false;
    for (int X = threadIdx.x; X < W; X += 256) {
        const long long lab = label[((size_t)b * H + Y) * W + X];
        const bool inr = lab >= 0 && lab < C;
        bad |= lab != ignore_label && !inr;
        if (lab == ignore_label || !inr) continue;
        const int li = (int)lab;
        atomicAdd(&s_cnt[li], 1);
        const Lerp lx = lerp_ac(X, w, W);
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            float m, e[C], se, zl;
            up_softmax<C>(rows, w, hd, ly, lx, li, m, e, se, zl);
            const float inv_se = 1.f / se;
            float others = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float q = e[c] * inv_se;
                acc[hd][0][c] += (c == li) ? q : 0.f;
                acc[hd][1][c] += (c == li) ? 0.f : q;
                others += (c == li) ? 0.f : q;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) acc[hd][2][c] += (c == li) ? others : 0.f;
        }
    }
    if (bad && flag) atomicOr(flag, 1);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float v = wave_sum_dpp(acc[i / 3][i % 3][c]);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i * C + c] = v;
        }
    __syncthreads();
    const size_t row = (size_t)b * H + Y;
    if (threadIdx.x < 6 * C)
        partial[row * 6 * C + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (threadIdx.x < C) ycnt[row * C + threadIdx.x] = s_cnt[threadIdx.x];
}

// coef f32[2 heads][C][2] = dL/dq of a pixel with y == c, of the others (times 0.5 * weight); *live = n, the present classes
__global__ void __launch_bounds__(OV_STAGE_THREADS) overlap_stage_kernel(const float* __restrict__ partial,
                                                                         const int* __restrict__ ycnt, int nrows, int C,
                                                                         OvParams prm, float* __restrict__ coef, int* live,
                                                                         float* loss, float* index, int* present) {
    __shared__ double s_part[OV_STAGE_THREADS];
    __shared__ double s_tot[7 * RGDA_MAX_CLASSES];
    __shared__ double s_term[2 * RGDA_MAX_CLASSES];
    const int t = threadIdx.x, nv = 7 * C, nchunk = OV_STAGE_THREADS / nv;      // nv <= 112: at least 9 chunks
    const int j = t % nv, k = t / nv;
    if (k < nchunk) {
        const int r0 = (int)((long long)k * nrows / nchunk), r1 = (int)((long long)(k + 1) * nrows / nchunk);
        double s = 0.0;
        if (j < 6 * C)
            for (int r = r0; r < r1; ++r) s += (double)partial[(size_t)r * 6 * C + j];
        else
            for (int r = r0; r < r1; ++r) s += (double)ycnt[(size_t)r * C + (j - 6 * C)];      // integers: exact
        s_part[k * nv + j] = s;
    }
    __syncthreads();
    if (t < nv) {
        double s = 0.0;
        for (int i = 0; i < nchunk; ++i) s += s_part[i * nv + t];
        s_tot[t] = s;
    }
    __syncthreads();
    int n = 0;
    for (int c = 0; c < C; ++c) n += s_tot[6 * C + c] > 0.0;
    if (t < 2 * C) {
        const int hd = t / C, c = t % C;
        const double TP = s_tot[(hd * 3 + 0) * C + c], FP = s_tot[(hd * 3 + 1) * C + c], FN = s_tot[(hd * 3 + 2) * C + c];
        const bool on = s_tot[6 * C + c] > 0.0;
        const double N = TP + prm.smooth, M = prm.alpha * FP + prm.beta * FN + OV_EPS, D = N + M, r = M / D;
        const double kc = on ? prm.gamma * pow(r, prm.gamma - 1.0) / (double)n * prm.gs : 0.0;
        s_term[t] = on ? pow(r, prm.gamma) : 0.0;
        coef[t * 2] = (float)(-kc * (D - (1.0 - prm.beta) * N) / (D * D));
        coef[t * 2 + 1] = (float)(kc * prm.alpha * N / (D * D));
        if (index && hd < prm.heads) index[t] = on ? (float)(N / D) : 0.f;
    }
    if (present && t < C) present[t] = (int)s_tot[6 * C + t];
    __syncthreads();
    if (t == 0) {
        double l0 = 0.0, l1 = 0.0;
        for (int c = 0; c < C; ++c) { l0 += s_term[c]; l1 += s_term[C + c]; }
        const double tot = prm.heads == 2 ? 0.5 * (l0 + l1) : l0;
        loss[0] = n > 0 ? (float)(tot / (double)n) : 0.f;
        *live = n;
    }
}

template <int C>
__global__ void __launch_bounds__(256) overlap_grad_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                           const int64_t* __restrict__ label,
                                                           const float* __restrict__ coef, float* T, int h, int w, int H,
                                                           int W, int ignore_label) {
    extern __shared__ float lds[];
    float* rows = lds;
    float* G = lds + 2 * C * 2 * w;
    int* lxi = (int*)(G + 2 * C * W);
    float* lxl = (float*)(lxi + W);
    const int b = blockIdx.y, Y = blockIdx.x;
    const Lerp ly = row_lerp<false>(Y, h, H);
    stage_rows<C>(rows, p1, p2, b, ly.i0, ly.i1, h, w);
    float ua[2][C], ub[2][C];             // uniform addresses: scalar loads
#pragma unroll
    for (int i = 0; i < 2 * C; ++i) { ua[i / C][i % C] = coef[2 * i]; ub[i / C][i % C] = coef[2 * i + 1]; }
    __syncthreads();
    for (int X = threadIdx.x; X < W; X += 256) {
        const Lerp lx = lerp_ac(X, w, W);
        lxi[X] = lx.i0;
        lxl[X] = lx.l1;
        const long long lab = label[((size_t)b * H + Y) * W + X];
        const bool valid = lab != ignore_label && lab >= 0 && lab < C;
        const int li = valid ? (int)lab : 0;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            float m, e[C], se, zl, u[C], dot = 0.f;
            up_softmax<C>(rows, w, hd, ly, lx, li, m, e, se, zl);
            const float inv_se = 1.f / se;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                e[c] *= inv_se;
                u[c] = (c == li) ? ua[hd][c] : ub[hd][c];
                dot += e[c] * u[c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) G[(hd * C + c) * W + X] = valid ? e[c] * (u[c] - dot) : 0.f;
        }
    }
    __syncthreads();
    contract_row<C>(G, lxi, lxl, T, b, Y, w, H, W);
}

// the workspace of one call: byte offsets
struct OvLayout {
    size_t partial, ycnt, coef, T, total;
};

static OvLayout ov_layout(int b, int c, int h, int w, int H) {
    (void)h;
    OvLayout o;
    const size_t nrows = (size_t)b * H;
    size_t at = 0;
    o.partial = at, at += align256_(nrows * 6 * c * 4);
    o.ycnt = at, at += align256_(nrows * c * 4);
    o.coef = at, at += align256_((size_t)4 * c * 4 + 4);      // the table, then n
    o.T = at, at += nrows * 2 * c * w * 4;
    o.total = at;
    return o;
}

struct OvCall {
    const float *p1, *p2;
    const int64_t* label;
    float *loss, *index, *g1, *g2;
    int *present, *flag;
    char* ws;
    int b, h, w, H, W, ignore_label, accumulate;
    OvParams prm;
};

template <int C>
static int run_overlap(const OvCall& a, rgda_stream_t stream) {
    hipStream_t st = to_stream(stream);
    const OvLayout lay = ov_layout(a.b, C, a.h, a.w, a.H);
    float* partial = (float*)(a.ws + lay.partial);
    int* ycnt = (int*)(a.ws + lay.ycnt);
    float* coef = (float*)(a.ws + lay.coef);
    int* live = (int*)(coef + 4 * C);
    float* T = (float*)(a.ws + lay.T);
    const dim3 rows_grid(a.H, a.b);
    const size_t slds = (size_t)2 * C * 2 * a.w * 4;      // the staged rows: within the gradient pass's need
    if (lds_attr((const void*)overlap_stat_kernel<C>, slds) != RGDA_OK) return RGDA_ERR_LAUNCH;
    overlap_stat_kernel<C><<<rows_grid, 256, slds, st>>>(a.p1, a.p2, a.label, partial, ycnt, a.flag, a.h, a.w, a.H, a.W,
                                                        a.ignore_label);
    RGDA_CHECK_LAUNCH();
    overlap_stage_kernel<<<1, OV_STAGE_THREADS, 0, st>>>(partial, ycnt, a.b * a.H, C, a.prm, coef, live, a.loss, a.index,
                                                        a.present);
    RGDA_CHECK_LAUNCH();
    if (!a.g1) return RGDA_OK;
    const size_t lds = grad_lds(C, a.w, a.W, true);
    if (lds_attr((const void*)overlap_grad_kernel<C>, lds) != RGDA_OK) return RGDA_ERR_LAUNCH;
    overlap_grad_kernel<C><<<rows_grid, 256, lds, st>>>(a.p1, a.p2, a.label, coef, T, a.h, a.w, a.H, a.W, a.ignore_label);
    RGDA_CHECK_LAUNCH();
    const int blocks = cdiv((long long)2 * a.b * C * a.h * a.w, 256);
    if (a.accumulate)
        loss_col_gated_kernel<C><<<blocks, 256, 0, st>>>(T, a.g1, a.g2, a.b, a.h, a.w, a.H, live);
    else
        loss_col_kernel<C, false><<<blocks, 256, 0, st>>>(T, a.g1, a.g2, a.b, a.h, a.w, a.H);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

}  // namespace

size_t loss_row_lds_bytes(int c, int w, int W, bool want) { return grad_lds(c, w, W, want); }

extern "C" size_t rgda_upsample_ce_workspace(int b, int c, int h, int w, int H, int W) {
    (void)W;
    return align256_((size_t)b * H * 2 * 4) + (size_t)b * H * 2 * c * w * 4;
}

extern "C" int rgda_upsample_ce(const float* p1, const float* p2, const int64_t* label, const float* class_weight,
                                float* loss, float* g1, float* g2, int b, int c, int h, int w, int H, int W,
                                int ignore_label, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (!p1 || !p2 || !label || !loss || !ws || ((g1 == nullptr) != (g2 == nullptr))) return RGDA_ERR_ARG;
    if (!class_count_ok(c)) return RGDA_ERR_UNSUPPORTED;
    if (b <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return RGDA_ERR_ARG;
    if (ws_bytes < rgda_upsample_ce_workspace(b, c, h, w, H, W)) return RGDA_ERR_WORKSPACE;
    if (grad_lds(c, w, W, g1 != nullptr) > MAX_ROW_LDS) return RGDA_ERR_UNSUPPORTED;
    LossCall a{};
    a.p1 = p1, a.p2 = p2, a.label = label, a.class_weight = class_weight;
    a.loss = loss, a.g1 = g1, a.g2 = g2;
    a.partial = (float*)ws;
    a.T = (float*)((char*)ws + align256_((size_t)b * H * 2 * 4));
    a.heads = 2, a.b = b, a.h = h, a.w = w, a.H = H, a.W = W, a.ignore_label = ignore_label;
    a.prm.gscale = (float)(0.5 / ((double)b * H * W));
    return run_kind(KIND_CE, c, a, stream);
}

extern "C" size_t rgda_upsample_loss_workspace(int kind, int b, int c, int h, int w, int H, int W) {
    if (kind < RGDA_LOSS_OHEM || kind > RGDA_LOSS_UVEM || b <= 0 || c <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
        return 0;
    const size_t n = (size_t)b * H * W;
    return align256_(sizeof(LossHdr)) + align256_((size_t)b * H * 2 * 4) + align256_((size_t)b * H * 2 * c * w * 4) +
           scratch_bytes(kind, n);
}

extern "C" int rgda_upsample_loss(int kind, int heads, const float* p1, const float* p2, const int64_t* label, const float* soft,
                                  const float* class_weight, float* acc_sum, double m, double t, double gamma,
                                  float thresh, double momentum, float* loss, float* g1, float* g2, int b, int c, int h,
                                  int w, int H, int W, int ignore_label, void* ws, size_t ws_bytes,
                                  rgda_stream_t stream) {
    if (kind < RGDA_LOSS_OHEM || kind > RGDA_LOSS_UVEM || (heads != 1 && heads != 2)) return RGDA_ERR_ARG;
    if (heads == 1 && p2 != p1) return RGDA_ERR_ARG;
    if (!p1 || !p2 || !label || !loss || !ws || ((g1 == nullptr) != (g2 == nullptr))) return RGDA_ERR_ARG;
    if (b <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return RGDA_ERR_ARG;
    if ((long long)b * H * W >= (1ll << 31)) return RGDA_ERR_ARG;         // pixel index and OHEM key low word: 32 bits
    if ((kind == RGDA_LOSS_UPS || kind == RGDA_LOSS_UVEM) && (!soft || !(t > 0.0))) return RGDA_ERR_ARG;
    if (kind == RGDA_LOSS_UVEM && !(gamma > 0.0 && m >= 0.0)) return RGDA_ERR_ARG;
    if (kind == RGDA_LOSS_GHM && (!acc_sum || !(momentum >= 0.0 && momentum < 1.0))) return RGDA_ERR_ARG;
    if (kind == RGDA_LOSS_FOCAL && !(gamma >= 0.0)) return RGDA_ERR_ARG;
    if (kind == RGDA_LOSS_OHEM && !(thresh >= 0.f)) return RGDA_ERR_ARG;
    // the reference's FocalLoss / GHMLoss take no class balancer
    if ((kind == RGDA_LOSS_FOCAL || kind == RGDA_LOSS_GHM) && class_weight) return RGDA_ERR_ARG;
    if (!class_count_ok(c)) return RGDA_ERR_UNSUPPORTED;
    if (ws_bytes < rgda_upsample_loss_workspace(kind, b, c, h, w, H, W)) return RGDA_ERR_WORKSPACE;
    if (grad_lds(c, w, W, g1 != nullptr) > MAX_ROW_LDS) return RGDA_ERR_UNSUPPORTED;
    LossCall a{};
    a.p1 = p1, a.p2 = p2, a.soft = soft, a.class_weight = class_weight, a.label = label;
    a.acc_sum = acc_sum, a.loss = loss, a.g1 = g1, a.g2 = g2;
    char* base = (char*)ws;
    a.hdr = (LossHdr*)base;
    base += align256_(sizeof(LossHdr));
    a.partial = (float*)base;
    base += align256_((size_t)b * H * 2 * 4);
    a.T = (float*)base;
    base += align256_((size_t)b * H * 2 * c * w * 4);
    a.scratch = base;
    a.heads = heads, a.b = b, a.h = h, a.w = w, a.H = H, a.W = W, a.ignore_label = ignore_label;
    LossParams& prm = a.prm;
    prm.thresh = thresh;
    prm.m = (float)m;
    prm.t = (float)t;
    prm.cl = m > 0.0 ? (float)(-1.0 / (m * m)) : 0.f;                   // balance.py:408,417: -1 / m^2, -1 / (t - m)^2
    prm.cr = m < t ? (float)(-1.0 / ((t - m) * (t - m))) : 0.f;
    prm.inv_gamma = gamma > 0.0 ? (float)(1.0 / gamma) : 0.f;
    prm.gamma = (float)gamma;
    prm.mom = (float)momentum;
    prm.omm = (float)(1.0 - momentum);
    return run_kind(kind, c, a, stream);
}

extern "C" size_t rgda_upsample_gdp_workspace(int b, int c, int h, int w, int H, int W) {
    if (b <= 0 || c <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
    const size_t n = (size_t)b * H * W;
    return align256_(sizeof(LossHdr)) + align256_((size_t)b * H * 2 * 4) + align256_((size_t)b * H * 2 * c * w * 4) +
           scratch_bytes(RGDA_LOSS_GDP, n);
}

extern "C" int rgda_upsample_gdp(int heads, const float* p1, const float* p2, const int64_t* label,
                                 const float* pixel_weight, const float* class_weight, float* acc_sum, float* bins_weight,
                                 double momentum, float* loss, float* g1, float* g2, int b, int c, int h, int w, int H,
                                 int W, int ignore_label, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (heads != 1 && heads != 2) return RGDA_ERR_ARG;
    if (!p1 || !p2 || !label || !loss || !ws || ((g1 == nullptr) != (g2 == nullptr))) return RGDA_ERR_ARG;
    if (heads == 1 && p2 != p1) return RGDA_ERR_ARG;
    if (!acc_sum || !bins_weight || !(momentum >= 0.0 && momentum < 1.0)) return RGDA_ERR_ARG;
    if (b <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return RGDA_ERR_ARG;
    if ((long long)b * H * W >= (1ll << 31)) return RGDA_ERR_ARG;
    if (!class_count_ok(c)) return RGDA_ERR_UNSUPPORTED;
    if (ws_bytes < rgda_upsample_gdp_workspace(b, c, h, w, H, W)) return RGDA_ERR_WORKSPACE;
    if (grad_lds(c, w, W, g1 != nullptr) > MAX_ROW_LDS) return RGDA_ERR_UNSUPPORTED;
    LossCall a{};
    a.p1 = p1, a.p2 = p2, a.class_weight = class_weight, a.pixel_weight = pixel_weight, a.label = label;
    a.acc_sum = acc_sum, a.bins_weight = bins_weight, a.loss = loss, a.g1 = g1, a.g2 = g2;
    char* base = (char*)ws;
    a.hdr = (LossHdr*)base;
    base += align256_(sizeof(LossHdr));
    a.partial = (float*)base;
    base += align256_((size_t)b * H * 2 * 4);
    a.T = (float*)base;
    base += align256_((size_t)b * H * 2 * c * w * 4);
    a.scratch = base;
    a.heads = heads, a.b = b, a.h = h, a.w = w, a.H = H, a.W = W, a.ignore_label = ignore_label;
    a.prm.mom = (float)momentum;
    a.prm.omm = (float)(1.0 - momentum);
    return run_kind(RGDA_LOSS_GDP, c, a, stream);
}

extern "C" size_t rgda_upsample_reg_workspace(int b, int c, int h, int w, int H, int W) {
    if (b <= 0 || c <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
    return align256_(sizeof(RegHdr)) + align256_((size_t)b * H * 4 * 4) + (size_t)b * H * 2 * c * w * 4;
}

extern "C" int rgda_upsample_reg(int heads, const float* p1, const float* p2, const int64_t* label, const float* w_ent,
                                 const float* w_kld, int terms, float lambda_ent, float lambda_kld, int accumulate,
                                 int empty_is_zero, float* loss, float* g1, float* g2, int b, int c, int h, int w, int H,
                                 int W, int ignore_label, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (heads != 1 && heads != 2) return RGDA_ERR_ARG;
    if (!p1 || !p2 || !loss || !ws || ((g1 == nullptr) != (g2 == nullptr))) return RGDA_ERR_ARG;
    if (heads == 1 && p2 != p1) return RGDA_ERR_ARG;
    if (terms < 1 || terms > (RGDA_REG_ENT | RGDA_REG_KLD)) return RGDA_ERR_ARG;
    // a derived mask reads the label
    if (!label && (((terms & RGDA_REG_ENT) && !w_ent) || ((terms & RGDA_REG_KLD) && !w_kld))) return RGDA_ERR_ARG;
    if (b <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return RGDA_ERR_ARG;
    if ((long long)b * H * W >= (1ll << 31)) return RGDA_ERR_ARG;         // the two counts: 32 bits
    if (!class_count_ok(c)) return RGDA_ERR_UNSUPPORTED;
    if (ws_bytes < rgda_upsample_reg_workspace(b, c, h, w, H, W)) return RGDA_ERR_WORKSPACE;
    if (grad_lds(c, w, W, g1 != nullptr) > MAX_ROW_LDS) return RGDA_ERR_UNSUPPORTED;
    RegCall a{};
    a.p1 = p1, a.p2 = p2, a.label = label, a.w_ent = w_ent, a.w_kld = w_kld;
    a.loss = loss, a.g1 = g1, a.g2 = g2;
    char* base = (char*)ws;
    a.hdr = (RegHdr*)base;
    base += align256_(sizeof(RegHdr));
    a.partial = (float*)base;
    base += align256_((size_t)b * H * 4 * 4);
    a.T = (float*)base;
    a.b = b, a.h = h, a.w = w, a.H = H, a.W = W, a.accumulate = accumulate != 0;
    a.prm.terms = terms, a.prm.empty_is_zero = empty_is_zero != 0, a.prm.ignore_label = ignore_label;
    a.prm.se = 0.5f * lambda_ent, a.prm.sk = 0.5f * lambda_kld;
    return with_classes(c, [&](auto cc) { return run_reg<decltype(cc)::value>(a, stream); });
}

extern "C" size_t rgda_upsample_pycda_workspace(int b, int c, int h, int w, int H, int W, const int* sizes, int levels) {
    PyLayout lay;
    return py_layout(b, c, h, w, H, W, sizes, levels, lay) ? lay.total : 0;
}

extern "C" int rgda_upsample_pycda(int heads, const float* p1, const float* p2, const float* soft, const int* sizes,
                                   const float* level_weight, int levels, double thresh, float weight, int accumulate,
                                   float* loss, int* n_active, float* g1, float* g2, int* flag, int b, int c, int h, int w,
                                   int H, int W, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (heads != 1 && heads != 2) return RGDA_ERR_ARG;
    if (!p1 || !p2 || !soft || !sizes || !loss || !n_active || !ws || ((g1 == nullptr) != (g2 == nullptr))) return RGDA_ERR_ARG;
    if (heads == 1 && p2 != p1) return RGDA_ERR_ARG;
    if (!(thresh >= 0.0 && thresh <= 1.0) || !std::isfinite(weight)) return RGDA_ERR_ARG;
    if (b <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return RGDA_ERR_ARG;
    if (!class_count_ok(c)) return RGDA_ERR_UNSUPPORTED;
    PyLayout lay;
    if (!py_layout(b, c, h, w, H, W, sizes, levels, lay)) return RGDA_ERR_ARG;
    for (int l = 0; l < levels; ++l) {
        lay.g.lw[l] = level_weight ? level_weight[l] : 1.f / (float)levels;
        if (!std::isfinite(lay.g.lw[l])) return RGDA_ERR_ARG;
    }
    if (ws_bytes < lay.total) return RGDA_ERR_WORKSPACE;
    if (b > 65535) return RGDA_ERR_UNSUPPORTED;                             // grid y of the row passes
    if (grad_lds(c, w, W, true) > MAX_ROW_LDS) return RGDA_ERR_UNSUPPORTED;
    lay.g.thr_fix = llrint(thresh * PY_FIX);
    PyCall a{};
    a.p1 = p1, a.p2 = p2, a.soft = soft, a.loss = loss, a.g1 = g1, a.g2 = g2, a.n_active = n_active, a.flag = flag;
    a.ws = (char*)ws, a.h = h, a.w = w, a.accumulate = accumulate != 0;
    a.gs = 0.5f * weight;
    return with_classes(c, [&](auto cc) { return run_pycda<decltype(cc)::value>(a, lay, stream); });
}

extern "C" size_t rgda_upsample_overlap_workspace(int b, int c, int h, int w, int H, int W) {
    if (b <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || !class_count_ok(c)) return 0;
    if ((long long)b * H * W >= (1ll << 31)) return 0;
    return ov_layout(b, c, h, w, H).total;
}

extern "C" int rgda_upsample_overlap(int heads, const float* p1, const float* p2, const int64_t* label, double alpha,
                                     double beta, double gamma, double smooth, float weight, int accumulate, float* loss,
                                     float* index, int* present, float* g1, float* g2, int* flag, int b, int c, int h, int w,
                                     int H, int W, int ignore_label, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (heads != 1 && heads != 2) return RGDA_ERR_ARG;
    if (!p1 || !p2 || !label || !loss || !ws || ((g1 == nullptr) != (g2 == nullptr))) return RGDA_ERR_ARG;
    if (heads == 1 && p2 != p1) return RGDA_ERR_ARG;
    if (!(std::isfinite(alpha) && alpha >= 0.0) || !(std::isfinite(beta) && beta >= 0.0)) return RGDA_ERR_ARG;
    if (!(std::isfinite(smooth) && smooth >= 0.0) || !(gamma >= 1.0 && gamma <= 8.0)) return RGDA_ERR_ARG;
    if (!(std::isfinite(weight) && weight >= 0.f)) return RGDA_ERR_ARG;
    if (b <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return RGDA_ERR_ARG;
    if ((long long)b * H * W >= (1ll << 31)) return RGDA_ERR_ARG;         // the class counts: 32 bits
    if (!class_count_ok(c)) return RGDA_ERR_UNSUPPORTED;
    if (ws_bytes < ov_layout(b, c, h, w, H).total) return RGDA_ERR_WORKSPACE;
    if (b > 65535) return RGDA_ERR_UNSUPPORTED;                             // grid y of the row passes
    const bool want = g1 != nullptr;      // without gradients the rows alone are staged
    if (grad_lds(c, w, W, want) > MAX_ROW_LDS) return RGDA_ERR_UNSUPPORTED;
    OvCall a{};
    a.p1 = p1, a.p2 = p2, a.label = label, a.loss = loss, a.index = index, a.present = present, a.g1 = g1, a.g2 = g2;
    a.flag = flag, a.ws = (char*)ws, a.b = b, a.h = h, a.w = w, a.H = H, a.W = W, a.ignore_label = ignore_label;
    a.accumulate = accumulate != 0;
    a.prm.alpha = alpha, a.prm.beta = beta, a.prm.gamma = gamma, a.prm.smooth = smooth, a.prm.heads = heads;
    a.prm.gs = 0.5 * (double)weight;
    return with_classes(c, [&](auto cc) { return run_overlap<decltype(cc)::value>(a, stream); });
}
