/*
 * rgda_hip.h -- C ABI of librgda_hip.so: the MI355X (gfx950) kernels behind the
 * RegDA self-training (SSL) step.  One process per GPU; every entry point only
 * ENQUEUES work on the caller's HIP stream (no host sync, no allocation, no
 * retained pointers, no global mutable state).  All buffers are device memory
 * owned by the caller (PyTorch tensors' data_ptr()).
 *
 * The reference (StuLiu/RegDA) has no FFI: its operator interface for this path
 * is a set of Python callables.  Each entry point below names the reference
 * callable (file:line under /root/reference) it replaces; the Python mirror of
 * those callables lives in regda_amd/ and calls these symbols through ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Return value: 0 on success, negative rgda_status otherwise (rgda_strerror()).
 * Layout vocabulary: "NCHW f32" = the reference's tensors at the API boundary;
 * "PxC bf16" = the internal pixel-major activation matrix [N*H*W][ld] with
 * channels contiguous (row stride ld elements), bf16.
 */
#ifndef RGDA_HIP_H
#define RGDA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGDA_ABI_VERSION 10
/* Per-channel statistics are accumulated into RGDA_STAT_REPLICAS interleaved copies (workgroup b adds to
 * copy b % 8, i.e. the copy of the XCD it runs on, so the atomics stay inside one XCD's L2); consumers
 * sum the copies.  A "stats"/"sums" buffer is therefore rgda_stat_t[RGDA_STAT_REPLICAS][2][C], zeroed by the caller.
 *
 * rgda_stat_t is 64-bit FIXED POINT (ABI 4; fp32 before): every workgroup reduces its rows in a fixed order, converts
 * the partial sum to round(v * 2^FRAC) and adds it with an integer atomic.  Integer addition is associative, so the
 * totals -- and everything computed from them: BatchNorm outputs, running statistics, BatchNorm gradients -- do not
 * depend on the order in which workgroups retire: two runs of the same step are bit-identical (fp32 atomics made the
 * batch statistics differ in the last bits from run to run, which moved thresholded pseudo labels).
 *   forward  (sum y, sum y^2 of conv outputs):  FRAC = 26 -> resolution 1.5e-8 per partial (below BatchNorm's eps by
 *            three orders of magnitude after the division by the row count), range |partial|, |total| < 2^33 = 8.6e9
 *   backward (sum g', sum g' xhat):             FRAC = 40 -> resolution 9e-13 per partial, range 2^19 = 5.2e5
 * Beyond the range: a workgroup partial that is out of range or not finite adds a poison value (3 * 2^60 units); the
 * consumers add the copies without wrapping (128-bit) and read a total of 2^59 units or more as NaN.  That channel's
 * (mean, invstd), BatchNorm outputs, running statistics and gradients are then NaN; the other channels are unaffected.
 * Not guaranteed in two cases: a first sum (sum y, sum g') whose poisons are offset by in-range partials of the opposite
 * sign that add up to about -3 * 2^60 units per poison can land back in range (sums of squares cannot: their partials are
 * never negative); and once one copy's own 64-bit accumulator has received 2^63 units (16 x the range) it wraps, and a
 * total can then read finite where it lands within 2^59 units of a nonzero multiple of 2^64. */
#define RGDA_STAT_REPLICAS 8
#define RGDA_STAT_FRAC_FWD 26
#define RGDA_STAT_FRAC_BWD 40
typedef int64_t rgda_stat_t;
#define RGDA_LAYOUT_TILE 64      /* tile edge of rgda_weight_transpose_batched (block accounting of its table) */

typedef void* rgda_stream_t; /* hipStream_t */

enum rgda_status {
    RGDA_OK = 0,
    RGDA_ERR_ARG = -1,       /* bad shape / null pointer / unsupported parameter */
    RGDA_ERR_WORKSPACE = -2, /* workspace too small */
    RGDA_ERR_LAUNCH = -3,    /* hipGetLastError() after launch != hipSuccess */
    RGDA_ERR_UNSUPPORTED = -4
};

int rgda_abi_version(void);
/* The LDS a class-specific launch needs and the most its entry point accepts (beyond it: RGDA_ERR_UNSUPPORTED), so that
 * a caller can refuse a shape before it launches anything.  which: RGDA_LDS_LOSS_ROW = the row pass of rgda_upsample_ce /
 * rgda_upsample_loss with gradients (n = logits width w, W = label width), RGDA_LDS_PCL = rgda_pcl_loss (n = K),
 * RGDA_LDS_REFINE = the prototype view of rgda_label_refine* (n = k).  c: the class count.  0 for an unknown `which`. */
enum { RGDA_LDS_LOSS_ROW = 0, RGDA_LDS_PCL = 1, RGDA_LDS_REFINE = 2 };
size_t rgda_class_lds(int which, int c, int n, int W);
size_t rgda_class_lds_limit(int which);
const char* rgda_strerror(int status);

/* ------------------------------------------------------------------ labels */

/* pseudo_selection(mask, cutoff_top, cutoff_low, 'tensor', ignore_label)
 *   regda/gast/pseudo_generation.py:59-93.
 * soft: NCHW f32 (b,c,hw) probabilities.  out: (b,hw) int64.
 * ws: >= rgda_pseudo_select_workspace(b,c) bytes; on return (stream order)
 *   ws[0 .. b*c) f32 = per-image per-class max, then one int32 flag word:
 *   bit0 = some value < 0 or > 1 (the reference asserts, :71).
 * If classmax_ready != 0 the per-class maxima already sit in ws (written by
 * rgda_label_refine) and the reduction pass is skipped. */
size_t rgda_pseudo_select_workspace(int b, int c);
int rgda_pseudo_select(const float* soft, int64_t* out, int b, int c, int hw, float cutoff_top,
                       float cutoff_low, int ignore_label, int classmax_ready, void* ws,
                       size_t ws_bytes, rgda_stream_t stream);

/* Homogenizer.forward(pseudo_labels, regions)  (LRH)
 *   regda/utils/local_region_homog.py:125-152 (+ torch_scatter.scatter sum, :140).
 * labels, regions, out: (b,hw) int64.  Region ids must lie in [0, max_regions);
 * pixels with ids outside are left unchanged and flag bit0 is set; labels
 * outside [0,class_num) other than ignore_label set bit1 (the reference's
 * one_hot would raise).  ws layout: int32 hist[b][max_regions][class_num],
 * int32 ids[b][max_regions], int32 flag.  Bit-exact vs the reference. */
size_t rgda_lrh_workspace(int b, int max_regions, int class_num);
int rgda_lrh(const int64_t* labels, const int64_t* regions, int64_t* out, int b, int hw,
             int class_num, int ignore_label, float percent, int max_regions, void* ws,
             size_t ws_bytes, rgda_stream_t stream);

/* pseudo_selection followed by Homogenizer.forward in one pass over the soft labels -- the chain of the SSL step
 * (tools/train_ssl_reg.py:224-228): out = LRH(pseudo_selection(soft), regions) exactly as the two calls above give it
 * (bit-exact), without the intermediate int64 label tensor.  classmax: f32 [b][c] per-image per-class maxima of `soft`
 * (what rgda_label_refine leaves in its workspace, or rgda_pseudo_select's ws[0 .. b*c)).  6 <= class_num <= 16, hw % 4 == 0,
 * max_regions <= 65535 (RGDA_ERR_UNSUPPORTED otherwise: use the two calls).  ws: rgda_pseudo_lrh_workspace bytes,
 * 16-byte aligned: int32 hist[b][R][C], int32 ids[b][R], int32 flag (bit0: a region id outside [0, R)), then scratch. */
size_t rgda_pseudo_lrh_workspace(int b, int hw, int max_regions, int class_num);
int rgda_pseudo_lrh(const float* soft, const float* classmax, const int64_t* regions, int64_t* out, int b, int hw,
                    int class_num, float cutoff_top, float cutoff_low, int ignore_label, float percent,
                    int max_regions, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* SAM.get_local_regions, the region-map assembly only   regda/utils/local_region_homog.py:51-56.
 * masks: uint8 [K][HW] (non-zero = inside), the automatic mask generator's masks in ITS order; areas int64 [K];
 * regions int32 [HW] out: 1 + the last mask index with area >= area_threshold covering the pixel, 0 where none does
 * (later masks overwrite earlier ones).  The generator itself (third-party segment_anything) is not part of this
 * library.  Bit-exact. */
int rgda_masks_to_regions(const uint8_t* masks, const int64_t* areas, int32_t* regions, int K, int64_t HW,
                          int64_t area_threshold, rgda_stream_t stream);

/* Aligner.label_refine(None, feat_t, [p1,p2], soft, refine=1, mode='all', temp)
 *   regda/gast/alignment.py:194-265 (+ _pearson_dist :396-423, _softmax_T, _logits_norm).
 * feat: NCHW f32 (b,k,h,w); protos (c,k) f32; p1,p2: NCHW f32 (b,c,h,w);
 * soft/out: NCHW f32 (b,c,H,W) (out may alias soft).  ws >= workspace bytes:
 * f32 sim[b][c][h*w] then f32 classmax[b][c] (+ int32 flag) laid out so that
 * `classmax` can be handed to rgda_pseudo_select (returned offset).  6 <= c <= 16 (all three label_refine entries); with the prototype view the centred
 * prototypes sit in LDS: c * k floats plus the partial sums within 160 KB (c = 16: k = 2048 fits, 4096 does not; beyond it RGDA_ERR_UNSUPPORTED). */
size_t rgda_label_refine_workspace(int b, int c, int h, int w);
size_t rgda_label_refine_classmax_offset(int b, int c, int h, int w);
int rgda_label_refine(const float* feat, const float* protos, const float* p1, const float* p2,
                      const float* soft, float* out, int b, int k, int c, int h, int w, int H,
                      int W, float temp, void* ws, size_t ws_bytes, rgda_stream_t stream);
/* The other `mode`s of label_refine with label_t_sup=None (alignment.py:199,212-236): `views` bit 0 = prototype view
 * ('p'), bit 1 = prediction view ('l'), 3 = 'all' (= rgda_label_refine).  A view that is not asked for needs no
 * inputs: feat / protos may be NULL for views == 2, p1 / p2 for views == 1.  A single prediction tensor
 * (alignment.py:232-234) is passed as p1 == p2: (s + s) * 0.5 is s exactly. */
int rgda_label_refine_views(const float* feat, const float* protos, const float* p1, const float* p2,
                            const float* soft, float* out, int b, int k, int c, int h, int w, int H,
                            int W, float temp, int views, void* ws, size_t ws_bytes,
                            rgda_stream_t stream);

/* label_refine WITH the superpixel view (label_t_sup given, alignment.py:238-258): label_t_sup (b, H*W) int64 superpixel
 * ids in [0, max_regions).  Per (image, superpixel, class) the maximum of `soft` over the superpixel's pixels (the
 * reference's torch_scatter.scatter(reduce='max')), gathered back per pixel, softmax_T(., temp) over the classes divided by
 * its per-pixel maximum + 1e-7 = sup_weight; the pixels of the superpixel with the LARGEST id of the whole batch are
 * `ignored` and keep the weight of the other views.  views: 3 = mode 'all' (weight * sup_weight), 0 = mode 's' (sup_weight
 * alone; feat / protos / p1 / p2 may be NULL and h, w are not used -- pass 1); 1 / 2 are served too (the reference's modes
 * 'p' / 'l' do not look at label_t_sup).  Workspace: rgda_label_refine's, then the maxima table, then two int32 at
 * rgda_label_refine_sup_flag_offset: [0] the largest id met, [1] non-zero when an id lay outside [0, max_regions) (such
 * pixels are treated as `ignored`; the reference would fault in scatter).  The per-class maxima of `out` are left at
 * rgda_label_refine_classmax_offset as by rgda_label_refine. */
size_t rgda_label_refine_sup_workspace(int b, int c, int h, int w, int max_regions);
size_t rgda_label_refine_sup_flag_offset(int b, int c, int h, int w, int max_regions);
int rgda_label_refine_sup(const float* feat, const float* protos, const float* p1, const float* p2,
                          const float* soft, const int64_t* label_t_sup, float* out, int b, int k, int c,
                          int h, int w, int H, int W, float temp, int views, int max_regions, void* ws,
                          size_t ws_bytes, rgda_stream_t stream);

/* Aligner.update_prototype(feat, label)  regda/gast/alignment.py:86-90,300-327,456-481.
 * feat NCHW f32 (b,k,h,w); label (b,H,W) int64 with H = 16h, W = 16w;
 * protos (c,k) f32 updated in place; label_ds (b,h*w) int64 out.
 * ws: f32 sums[c][k], f32 cnt[c].  6 <= c <= 16 (rgda_proto_stats too). */
size_t rgda_proto_update_workspace(int c, int k);
int rgda_proto_update(const float* feat, const int64_t* label, float* protos, int64_t* label_ds,
                      int b, int k, int c, int h, int w, int scale, int ignore_label,
                      float min_ratio, float decay, void* ws, size_t ws_bytes,
                      rgda_stream_t stream);
/* The two halves of rgda_proto_update, for data-parallel ranks (ABI 9).  rgda_proto_stats leaves the
 * sufficient statistics of _compute_local_prototypes (alignment.py:300-327) in `stats` (rgda_proto_update_workspace
 * bytes): f32 sums[c][k] = sum of feat over the pixels whose downscaled label is class c, f32 cnt[c] = their number,
 * then an int32 flag word (bit 2: a label outside [0, c) that is not ignore_label).  Both add over batches: the ranks all-reduce (sum) the first c * k + c floats and each calls
 * rgda_proto_apply -- local = sums / (cnt + 1e-7), the old prototype where cnt < 1 (:318-321), EMA (:435-438) -- which
 * gives the prototypes of the concatenated global batch on every rank.  rgda_proto_update == stats + apply.
 * rgda_proto_apply takes 0 <= decay < 1: decay 0 on zero prototypes is Aligner.init_avg (alignment.py:121-122) over
 * statistics summed across batches (update_avg, :107-119) -- classes without pixels stay 0. */
int rgda_proto_stats(const float* feat, const int64_t* label, int64_t* label_ds, int b, int k, int c,
                     int h, int w, int scale, int ignore_label, float min_ratio, void* stats,
                     size_t stats_bytes, rgda_stream_t stream);
int rgda_proto_apply(float* protos, const void* stats, int c, int k, float decay, rgda_stream_t stream);

/* loss_calc([p1,p2], label, CrossEntropy, multi=True) forward + d(loss)/d(logits)
 *   regda/utils/tools.py:240-254; regda/gast/balance.py:88-101.
 * p1,p2: NCHW f32 (b,c,h,w) logits; label (b,H,W) int64; class_weight: NULL or
 * f32[2][c] per-head per-class weights (ClassBalance, balance.py:27-43).
 * loss: f32[1] (mean over ALL pixels, mean over heads).  g1,g2: NULL or
 * NCHW f32 (b,c,h,w) gradients of `loss` w.r.t. p1,p2.  6 <= c <= 16. */
size_t rgda_upsample_ce_workspace(int b, int c, int h, int w, int H, int W);
int rgda_upsample_ce(const float* p1, const float* p2, const int64_t* label,
                     const float* class_weight, float* loss, float* g1, float* g2, int b, int c,
                     int h, int w, int H, int W, int ignore_label, void* ws, size_t ws_bytes,
                     rgda_stream_t stream);

/* loss_calc([p1,p2], label, loss_fn, multi=True) / loss_calc_uvem(..., label_soft, ...) with the losses of the --ls / --lt
 * flags (tools/train_ssl_reg.py:52-63,134-158; tools/train_src.py:33-34; tools/train_align_reg.py:55-56), forward +
 * d(loss)/d(logits), sync-free (every batch statistic stays on the device):
 *   RGDA_LOSS_OHEM   OhemCrossEntropy (regda/gast/balance.py:104-133): n_min = #valid / 5; mean of the losses > thresh
 *                    (thresh = f32 -log 0.7), or of the n_min largest when fewer are kept (ties: lowest pixel index
 *                    first); class_weight optional.  All labels ignored: loss NaN, gradient 0.
 *   RGDA_LOSS_FOCAL  FocalLoss(alpha=None, reduction='mean') (:136-158): mean of (1 - exp(-ce))^gamma * ce over ALL pixels.
 *   RGDA_LOSS_GHM    GHMLoss(bins=30) (:161-216): acc_sum (device f32[30], in/out) = momentum * acc_sum + (1 - momentum)
 *                    * histc(|p_y - 1|), once per head (head 1 first); weight 1 / acc_sum[bucketize(g) - 1];
 *                    sum(ce * weight) / (#(label != -1) + 1e-7).  momentum 0: acc_sum = the histogram.
 *   RGDA_LOSS_UPS    UPSLoss (:306-345): u = sum_c -s log s of the soft label `soft` (NCHW f32 (b,c,H,W)); CE where
 *                    u <= t, times class_weight (optional); sum / (#(u <= t and valid) + 1e-7).
 *   RGDA_LOSS_UVEM   UVEMLoss (:348-426): as UPS, times UVEMLoss.get_weight(u) with (m, t, gamma).
 * Each loss is applied per head after the bilinear (align_corners=True) upsample to the label size and the two heads
 * are averaged (regda/utils/tools.py:240-254, balance.py:438-460).  heads 1: one loss_fn call on one prediction (p2 == p1;
 * the loss is that call's, g1 + g2 its gradient, GHM's acc_sum is updated once).  class_weight: NULL or f32[2][c] (per head, the
 * ClassBalance state of that head's call); must be NULL for FOCAL and GHM.  Parameters a kind does not use are ignored.
 * loss: f32[1].  g1, g2: NULL or NCHW f32 (b,c,h,w).  6 <= c <= 16; b * H * W < 2^31.  ws: rgda_upsample_loss_workspace
 * bytes (0 = bad arguments); the per-pixel scratch is 8 (OHEM), 2 (GHM), 4 (UPS / UVEM) or 0 (focal) bytes per pixel.
 * Deterministic: integer atomics for counts and histograms, fixed-order reductions, no float atomics. */
enum rgda_loss_kind {
    RGDA_LOSS_OHEM = 1,
    RGDA_LOSS_FOCAL = 2,
    RGDA_LOSS_GHM = 3,
    RGDA_LOSS_UPS = 4,
    RGDA_LOSS_UVEM = 5,
    RGDA_LOSS_GDP = 6          /* served by rgda_upsample_gdp; rgda_upsample_loss answers RGDA_ERR_ARG for it */
};
size_t rgda_upsample_loss_workspace(int kind, int b, int c, int h, int w, int H, int W);
int rgda_upsample_loss(int kind, int heads, const float* p1, const float* p2, const int64_t* label,
                       const float* soft, const float* class_weight, float* acc_sum, double m, double t, double gamma, float thresh,
                       double momentum, float* loss, float* g1, float* g2, int b, int c, int h, int w, int H,
                       int W, int ignore_label, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* loss_calc([p1,p2], label, GDPLoss(bins=30), multi=True) forward + d(loss)/d(logits)
 *   regda/gast/balance.py:218-303; regda/utils/tools.py:240-254.
 * Per head call (head 1 first) on the logits upsampled bilinearly (align_corners=True) to the label size:
 *   g = |softmax(z)[label] - 1| (-1 where ignored); bins = histc(g, 30, 0, 1); bins = (bins + flip(bins)) * 0.5 (:261-262);
 *   acc_sum (device f32[30], in/out) = momentum * acc_sum + (1 - momentum) * bins, or bins at momentum 0 (:267-270);
 *   bins_weight = where(acc_sum != 0, 1 - acc_sum / (sum(acc_sum) + 1e-7), 0) / (max + 1e-7) (:290-295; device f32[30],
 *   out: the weights of the LAST head call); weight = bins_weight[bucketize(g) - 1] (0 outside 1..30: a pixel with
 *   p_y == 1 exactly is counted in the histogram and weighs 0) + pixel_weight[pixel] + class_weight[head][label], the
 *   two optional terms present iff their pointer is non-NULL, / the number of terms (:277-283);
 *   loss = sum(ce * weight) / (#(label != -1) + 1e-7) (:284), mean over the heads.  Weights carry no gradient.
 * pixel_weight: NULL or f32[b*H*W] (Aligner.get_prototype_weight_4pixel, rgda_proto_pixel_weight; shared by both heads);
 * class_weight: NULL or f32[2][c].  heads, p1, p2, label, loss, g1, g2, the class counts and the size limit: as
 * rgda_upsample_loss.  The statistic pass is RGDA_LOSS_GHM's own kernel; workspace: rgda_upsample_gdp_workspace bytes
 * (2 bytes of scratch per pixel).  All labels ignored: loss 0, gradient 0.  Deterministic, nothing read back. */
size_t rgda_upsample_gdp_workspace(int b, int c, int h, int w, int H, int W);
int rgda_upsample_gdp(int heads, const float* p1, const float* p2, const int64_t* label,
                      const float* pixel_weight, const float* class_weight, float* acc_sum, float* bins_weight,
                      double momentum, float* loss, float* g1, float* g2, int b, int c, int h, int w, int H,
                      int W, int ignore_label, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* entropyloss(logits, weight) / kldloss(logits, weight), IAST's region regularisers   regda/utils/tools.py:376-398
 * forward + d / d(logits), on the same pipeline.  Per head on the logits upsampled bilinearly (align_corners=True, the
 * arithmetic of rgda_upsample_ce) to (H, W); h == H, w == W is the plain call on full-resolution logits:
 *   ent = sum_pix w_e * (-sum_c p_c log p_c) / #(w_e > 0)          kld = sum_pix w_k * (-(1/c) sum_c log p_c) / #(w_k > 0)
 * with log p = z - logsumexp(z), never log(p): a probability that underflows contributes 0.
 * terms: RGDA_REG_ENT | RGDA_REG_KLD, the terms computed; a term that is off costs nothing, its loss slot is 0 and its
 *   weight map and lambda are not looked at.
 * w_ent, w_kld: f32[b*H*W] (any float: it multiplies the term, only > 0 counts in the denominator), or NULL = derived in
 *   registers from `label` (int64 (b,H,W); may be NULL when no term derives): w_e = (label == ignore_label),
 *   w_k = (label != ignore_label), IAST's ignored and confident regions.
 * loss: f32[2] = (ent, kld), unscaled, the mean over the heads.  g1, g2: NULL or NCHW f32 (b,c,h,w), per head the
 *   gradient of 0.5 * (lambda_ent * ent_h + lambda_kld * kld_h); accumulate 0: written, 1: added onto what they hold
 *   (one f32 addition of the finished value).  heads 1: one prediction (p2 == p1; g1 + g2 is its gradient, no 0.5).
 * empty_is_zero: a term whose denominator is 0 is 0 / 0 = NaN with a NaN gradient as in the reference (0), or exactly 0
 *   with a gradient of exactly 0 (1).
 * The two counts are taken on the device with integer atomics, the sums in a fixed order: deterministic, nothing read
 * back.  6 <= c <= 16 and the row-LDS limit of rgda_upsample_ce (RGDA_ERR_UNSUPPORTED); b * H * W < 2^31. */
enum rgda_reg_term { RGDA_REG_ENT = 1, RGDA_REG_KLD = 2 };
size_t rgda_upsample_reg_workspace(int b, int c, int h, int w, int H, int W);
int rgda_upsample_reg(int heads, const float* p1, const float* p2, const int64_t* label, const float* w_ent,
                      const float* w_kld, int terms, float lambda_ent, float lambda_kld, int accumulate,
                      int empty_is_zero, float* loss, float* g1, float* g2, int b, int c, int h, int w, int H, int W,
                      int ignore_label, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* PyCDA region pyramid term (Lian et al., ICCV 2019, "Constructing Self-motivated Pyramid Curriculums"): at every level of
 * a pyramid of square regions the student's mean prediction over a region must match the teacher's label distribution
 * of that region.  Forward + d / d(logits) on the upsample-loss pipeline.  The reference has no such code; this is the
 * contract (restated in float64 by tests/pycda_ref.py).
 * Inputs: p1, p2 student logits NCHW f32 (b,c,h,w); soft teacher probabilities NCHW f32 (b,c,H,W), every value finite
 *   and in [0, 1]: a value outside is clamped into it, NaN counts as 0, and either raises bit 0 of *flag (device int32,
 *   may be NULL; never cleared here).
 * Levels: sizes, a HOST int array of `levels` entries (1 <= levels <= 6), read during the call: finite sizes are powers
 *   of two in [2, 256], strictly increasing, optionally followed by one 0 = the whole image; so every coarser region is
 *   a union of whole cells of the finest level.  At size s image n is cut into ceil(H/s) x ceil(W/s) squares anchored at
 *   (0, 0), border squares clipped; |r| is a region's real pixel count.
 * Targets (exact integers): Tfix_r(c) = sum_{i in r} rint(soft_i(c) * 2^24) as int64; class c is active in r iff
 *   Tfix_r(c) > rint(thresh * 2^24) * |r| (strict, in integers; 0 <= thresh <= 1); T_r(c) = Tfix_r(c) / (|r| * 2^24);
 *   n_l = the regions of level l, over the batch, with at least one active class.
 * Predictions: per head q = softmax of the logits upsampled bilinearly (align_corners=True, the arithmetic of
 *   rgda_upsample_ce); Q_r(c) = mean_{i in r} q_i(c).
 * Loss: L_{l,hd} = sum_{r, active c} -T_r(c) log(Q_r(c) + 1e-7) / max(n_l, 1); level[l] = the mean of L_{l,hd} over the
 *   heads; total = sum_l level_weight[l] * level[l].  level_weight: a HOST f32 array of `levels` entries, or NULL = 1 /
 *   levels each.  A level without an active region is exactly 0 with a gradient of exactly 0.  Targets carry no gradient.
 * Outputs: loss f32[1 + levels] = total, then the levels, all unscaled; n_active int32[levels]; g1, g2: NULL or NCHW f32
 *   (b,c,h,w), per head the gradient of 0.5 * weight * total_hd; heads 1: p2 == p1, g1 + g2 is the gradient, no 0.5 (the
 *   convention of rgda_upsample_reg).  accumulate 0: written, 1: added onto what they hold (one f32 addition of the
 *   finished value).
 * Limits: 6 <= c <= 16 and the row-LDS limit of rgda_upsample_ce, with gradients (RGDA_ERR_UNSUPPORTED); b * H * W <
 *   2^31; b <= 65535.  ws: rgda_upsample_pycda_workspace bytes (0 = bad arguments).  Every check comes before anything
 *   touches the GPU.  Deterministic: no float atomics, every sum in a fixed order or in integers; nothing is read back. */
size_t rgda_upsample_pycda_workspace(int b, int c, int h, int w, int H, int W, const int* sizes, int levels);
int rgda_upsample_pycda(int heads, const float* p1, const float* p2, const float* soft, const int* sizes,
                        const float* level_weight, int levels, double thresh, float weight, int accumulate, float* loss,
                        int* n_active, float* g1, float* g2, int* flag, int b, int c, int h, int w, int H, int W, void* ws,
                        size_t ws_bytes, rgda_stream_t stream);

/* Region-overlap term (Dice / soft Jaccard / Tversky, Salehi et al. 2017 / focal-Tversky, Abraham & Khan 2019) of the
 * upsampled logits against hard labels.  Forward + d / d(logits) on the upsample-loss pipeline.  The reference has no
 * such code; this is the contract (restated in float64 by tests/overlap_ref.py).
 * Inputs: p1, p2 logits NCHW f32 (b,c,h,w); label int64 (b,H,W).  A pixel is valid iff label != ignore_label; a valid
 *   label outside [0, c) counts as ignored and raises bit 0 of *flag (device int32, may be NULL; never cleared here).
 * Predictions: per head q = softmax of the logits upsampled bilinearly (align_corners=True, the arithmetic of
 *   rgda_upsample_ce) to (H, W); h == H, w == W is the plain call on full-resolution logits.
 * Sums over the valid pixels i of the whole batch, per head and class, each one a sum of non-negative terms:
 *   TP_c = sum q_i(c) [y_i == c];  FP_c = sum q_i(c) [y_i != c];  FN_c = sum (1 - q_i(c)) [y_i == c];
 *   Y_c = #{y_i == c} (an exact integer).
 * Index and loss: N_c = TP_c + smooth; M_c = alpha FP_c + beta FN_c + 1e-7; T_c = N_c / (N_c + M_c); class c is present
 *   iff Y_c > 0, n = #present; loss_hd = (1 / n) sum_{present c} (M_c / (N_c + M_c))^gamma; the loss is the mean over the
 *   heads.  alpha = beta = 0.5: Dice; alpha = beta = 1: soft Jaccard; gamma > 1: focal-Tversky.  Labels carry no
 *   gradient.  n == 0 (everything ignored): a loss of exactly 0 and a gradient of exactly 0; with accumulate = 1 the
 *   gradient buffers are then left untouched.
 * Parameters: alpha, beta, smooth finite and >= 0; 1 <= gamma <= 8; weight finite and >= 0; anything else is
 *   RGDA_ERR_ARG.
 * Outputs: loss f32[1], unscaled; index f32[heads][c] (may be NULL) = T_c, 0 for an absent class; present int32[c] (may
 *   be NULL) = Y_c; g1, g2: NULL or NCHW f32 (b,c,h,w), per head the gradient of 0.5 * weight * loss_hd; heads 1: p2 ==
 *   p1, g1 + g2 is the gradient, no 0.5 (the convention of rgda_upsample_reg / _pycda).  accumulate 0: written, 1: added
 *   onto what they hold (one f32 addition of the finished value).
 * Limits: 6 <= c <= 16 and the row-LDS limit of rgda_upsample_ce (RGDA_ERR_UNSUPPORTED); b * H * W < 2^31; b <= 65535.
 *   ws: rgda_upsample_overlap_workspace bytes (0 = bad arguments).  Every check comes before anything touches the GPU.
 * Deterministic: no float atomics, Y_c summed in integers, the float sums combined in a fixed order that does not
 *   depend on workgroup scheduling; two calls give identical bits; nothing is read back. */
size_t rgda_upsample_overlap_workspace(int b, int c, int h, int w, int H, int W);
int rgda_upsample_overlap(int heads, const float* p1, const float* p2, const int64_t* label, double alpha, double beta,
                          double gamma, double smooth, float weight, int accumulate, float* loss, float* index,
                          int* present, float* g1, float* g2, int* flag, int b, int c, int h, int w, int H, int W,
                          int ignore_label, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* IAST, instance-adaptive pseudo-labels: ias_thresh and the loop body of generate_pseudo   regda/utils/tools.py:323-373
 * Three stages over one workspace of rgda_iast_workspace(n, c, H, W) bytes (0 = bad arguments), laid out as
 *   int32 hist[c][RGDA_IAST_BINS] | f32 maxp[n*H*W] | uint8 arg[n*H*W], each piece starting on a 256-byte boundary.
 * rgda_iast_hist: probs NCHW f32 (n,c,H,W).  CONTRACT: every value is finite and 0 <= p <= 1 (a softmax); a maximum outside
 *   it is not counted.  Per pixel arg = the FIRST maximum over the classes, maxp its value; hist[arg][bits] counts maxp
 *   rounded to fp16 (round to nearest even, numpy's astype(float16)) by its bit pattern 0 .. 0x7C00 -- an exact
 *   histogram of the per-class fp16 lists the reference builds.  The histogram is cleared by the call.
 * rgda_iast_percentile: out[k] = f32(np.percentile([prepend[k]] + the fp16 values of class k (as f64), 100 * q[k])), the
 *   'linear' method in f64 as numpy evaluates it; prepend, q: device f64[c], 0 <= q <= 1; a class without pixels
 *   returns prepend[k].  Needs only the histogram piece of the workspace.
 * rgda_iast_label: label (uint8, n*H*W) = arg + 1, 0 where (double)maxp < cls_thresh[arg]; cls_thresh: device f64[c].
 * 6 <= c <= 16 (RGDA_ERR_UNSUPPORTED); n * H * W < 2^31.  Integer atomics only: deterministic. */
#define RGDA_IAST_BINS 0x7C01
size_t rgda_iast_workspace(int n, int c, int H, int W);
int rgda_iast_hist(const float* probs, int n, int c, int H, int W, void* ws, size_t ws_bytes, rgda_stream_t stream);
int rgda_iast_percentile(const double* prepend, const double* q, float* out, int c, const void* ws, size_t ws_bytes,
                         rgda_stream_t stream);
int rgda_iast_label(const double* cls_thresh, uint8_t* label, int n, int c, int H, int W, const void* ws,
                    size_t ws_bytes, rgda_stream_t stream);

/* analysis_pseudo_labels + range_static: entropy-binned accuracy tables   regda/gast/pseudo_generation.py:158-235
 * The reference makes R = 100 passes per image over the (C, H, W) soft label; here one pass bins every pixel.
 * rgda_pseudo_analysis: soft NCHW f32 (b,c,H,W), gt int64 (b,H,W), lo / hi: device f32[R], the bin edges as the reference
 *   compares them (f32(1.0 * i * step), f32(1.0 * i * step + step), step = log(c) / R).  Per pixel
 *     pseudo      the decision of rgda_pseudo_select (threshold max(classmax * cutoff_top, cutoff_low) in f32, strict >,
 *                 exactly one passing class).  The per-image per-class maxima are NOT an argument: the call runs the
 *                 maximum pass of rgda_pseudo_select itself, into the tail of `tables`.
 *     entropy     sum_c -p_c * log(p_c) in fp64 in class order, rounded once to f32 (:185 sums in f32); NaN where a
 *                 probability is exactly 0, as in the reference
 *     difficulty  1 - p[gt] in f32, 1 where gt == ignore_label (:188-191); always a multiple of 2^-24
 *   and the pixel is counted in every bin i with lo[i] <= entropy < hi[i] (the candidate bin and both neighbours are
 *   tested: the rounded edges of some (c, R) overlap or gap by an ulp); a NaN entropy is counted in row R instead (the
 *   reference keeps such a pixel in every bin's used / true / difficulty sums, :226, :232, but in no bin's pixel count,
 *   :233; the fold adds row R accordingly).  tables, written by the call (cleared first), per image T = (R + 1) * (2 * c + 2)
 *   int64:   used[R + 1][c] (pixels whose pseudo label is class k) | hit[R + 1][c] (of those, pseudo == gt) |
 *            inbin[R + 1] | diff24[R + 1] (the sum of difficulty * 2^24: exact)
 *   then, after the b images, int32 flag (bit 0: a probability outside [0, 1] or not finite, :71; bit 1: a gt outside
 *   [0, c) that is not ignore_label, :189; such pixels are skipped), int32 pad, f32 classmax[b][c].
 *   rgda_pseudo_analysis_workspace(b, c, R): the bytes of `tables` (0 = bad arguments); 8-byte aligned.
 * rgda_pseudo_analysis_fold: one workgroup adds a batch's tables to a running state, image after image (:195-207):
 *     acc = cnt_true / (cnt_used + 1e-7), acc_cnt += (cnt_used != 0)       cnt_* = the sums over the classes, row R added
 *     diffi = (diff24 / 2^24) / (inbin + 1e-7), diffi_cnt += (diff24 != 0)  diff24 with row R added, inbin without
 *   both quotients in fp64 from the exact integers (the reference: f32).  state, rgda_pseudo_analysis_fold_workspace(c, R)
 *   bytes, zeroed by the caller before the first batch, 8-byte aligned:
 *     int64 total[T] (as one image's tables, row R kept apart) | f64 acc_sum[R] | f64 diffi_sum[R] | int64 images |
 *     int32 acc_cnt[R] | int32 diffi_cnt[R] | int32 flag (the batches' flags or-ed) | padding to 8 bytes.
 * soft needs 4-byte alignment only: where it, gt or H * W rule out 16-byte loads, both passes take scalar loads.
 * 6 <= c <= 16 (RGDA_ERR_UNSUPPORTED); 1 <= R <= 256, b * H * W < 2^31, H * W <= 2^31 - 16384 (the passes' int steps),
 * b * c <= 65535 (grid y of the maximum pass), null or misaligned pointers (RGDA_ERR_ARG); a short
 * buffer (RGDA_ERR_WORKSPACE); all before any launch.  Integer atomics only and a fixed image order: deterministic, and
 * nothing is read back. */
#define RGDA_ANALYSIS_MAX_BINS 256
size_t rgda_pseudo_analysis_workspace(int b, int c, int R);
int rgda_pseudo_analysis(const float* soft, const int64_t* gt, const float* lo, const float* hi, int b, int c, int H, int W,
                         int R, float cutoff_top, float cutoff_low, int ignore_label, void* tables, size_t tables_bytes,
                         rgda_stream_t stream);
size_t rgda_pseudo_analysis_fold_workspace(int c, int R);
int rgda_pseudo_analysis_fold(const void* tables, size_t tables_bytes, int b, int c, int R, void* state, size_t state_bytes,
                              rgda_stream_t stream);

/* Aligner.get_prototype_weight_4pixel(feats, label_hard)   regda/gast/alignment.py:267-281 (+ _pearson_dist :396-423).
 * feat NCHW f32 (b,k,h,w); protos (c,k) f32; label (b,H,W) int64; out f32[b*H*W]:
 *   sim = 1 / pearson_dist(feat, protos) at (b,c,h,w) -> bilinear align_corners=True to (H,W) -> softmax over the classes
 *   (temperature 1: the reference's `temp` argument is unused) -> / (per-pixel max + 1e-7) -> the value at the pixel's
 *   label, 0 where the label is ignore_label (or outside [0, c)).
 * sim: NULL, or the similarity map f32 (b,c,h,w) already computed (the base of rgda_label_refine's workspace after a call
 * with the prototype view): the similarity pass is skipped, feat / protos / ws may be NULL and k is not used.
 * 6 <= c <= 16; without sim the prototype limits of rgda_label_refine apply (k % 4 == 0, c * k floats + partial sums in
 * LDS); the pick pass stages 2 * c * w floats in at most 64 KB of LDS (c = 16: w <= 512). */
size_t rgda_proto_pixel_weight_workspace(int b, int c, int k, int h, int w);
int rgda_proto_pixel_weight(const float* feat, const float* protos, const float* sim, const int64_t* label,
                            float* out, int b, int k, int c, int h, int w, int H, int W, int ignore_label,
                            void* ws, size_t ws_bytes, rgda_stream_t stream);

/* Deeplabv2 eval-branch output  regda/models/Encoder.py:152-155:
 * (softmax(up(x1)) + softmax(up(x2))) / 2, up = bilinear align_corners=True.  6 <= c <= 16. */
int rgda_teacher_probs(const float* p1, const float* p2, float* probs, int b, int c, int h, int w,
                       int H, int W, rgda_stream_t stream);

/* ClassBalance._local_freq counts (balance.py:45-53): cnt[c] int32 += #pixels per class. */
int rgda_class_count(const int64_t* label, int32_t* cnt, int64_t n, int c, rgda_stream_t stream);

/* ------------------------------------------------------------- conv stack  */

/* Implicit-GEMM convolution on PxC bf16 activations, bf16 MFMA, fp32 accumulate.
 * Replaces nn.Conv2d forward (cuDNN) for every conv of regda/_resnets.py:72-112,
 * regda/models/Encoder.py:8-65, and -- with mode=1 and transposed weights -- the
 * data-gradient of the same convs.
 *   x   : [N*H*W][ldx] bf16, Cin channels used
 *   wgt : [Cout][kh*kw][Cin] bf16  (mode 1: [Cin_of_fwd][kh*kw][Cout_of_fwd])
 *   y   : [N*Ho*Wo][ldy] bf16
 *   res : NULL or [N*Ho*Wo][ldres] bf16 added to the result before the store
 *   res_relu_mask : NULL or uint8 [N*Ho*Wo][Cout/8] sign bits (rgda_bn_train_apply): res is added only where its
 *          bit is set -- the gradient of a residual connection gated by the ReLU it passed through, so that gated
 *          copy never has to be written to memory
 *   stats: NULL or rgda_stat_t[stat_groups][RGDA_STAT_REPLICAS][2][Cout] (FRAC_FWD); per-channel sum and sum of squares of
 *          the (bf16-rounded) outputs are accumulated order-independently (BatchNorm batch stats)
 *   stat_groups: the statistics groups, equal blocks of WHOLE images: N % stat_groups != 0 is RGDA_ERR_ARG (here and in
 *          rgda_conv2d_grouped, rgda_conv2d_bnbwd's `groups` and rgda_conv2d_bnin's, as in rgda_stem_conv)
 *   mode 0: y[n,ho,wo] = sum x[n, ho*stride-pad+kh*dil, wo*stride-pad+kw*dil] * w
 *   mode 1: y[n,ho,wo] = sum x[n, (ho+pad-kh*dil)/stride, (wo+pad-kw*dil)/stride] * w
 *           (terms with a non-integer or out-of-range source are zero)
 * Requires Cin % 32 == 0, Cout % 8 == 0, ld* % 8 == 0. */
int rgda_conv2d(const void* x, int ldx, const void* wgt, void* y, int ldy, const void* res,
                int ldres, const uint8_t* res_relu_mask, rgda_stat_t* stats, int stat_groups, int N, int H, int W,
                int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, int mode,
                rgda_stream_t stream);

/* Several INDEPENDENT rgda_conv2d calls as (at most) one launch per eight: a descriptor holds exactly rgda_conv2d's
 * arguments.  Same results as calling rgda_conv2d on each in turn (no output of one may be an input of another).  Problems
 * served by the small-tile kernel (conv_igemm_kernel<128, 64, 3, 2, 2, true, false>: what the tiny maps of the PPM branches
 * get, regda/models/Encoder.py:30-51 -- four scales x two statistics groups, 4 - 36 workgroups each) share launches; any
 * other is launched on its own.  Every descriptor is validated before anything is launched.
 * rgda_conv2d_grouped_launches: the number of kernel launches the list makes (negative: the status it would fail with). */
typedef struct rgda_conv2d_desc {
    const void* x; const void* wgt; void* y; const void* res; const uint8_t* res_relu_mask; rgda_stat_t* stats;
    int ldx, ldy, ldres, stat_groups;
    int N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil, mode;
} rgda_conv2d_desc;
int rgda_conv2d_grouped(const rgda_conv2d_desc* descs, int n, rgda_stream_t stream);
int rgda_conv2d_grouped_launches(const rgda_conv2d_desc* descs, int n);

/* Forward conv with an INFERENCE-mode BatchNorm (+ residual + ReLU) folded into the epilogue -- the EMA teacher's
 * conv + BN + ReLU units (regda/models/Encoder.py:152-155 runs the model in eval()):
 *   y = act((conv(x) - running_mean) / sqrt(running_var + eps) * gamma + beta + res). */
int rgda_conv2d_bneval(const void* x, int ldx, const void* wgt, void* y, int ldy, const void* res, int ldres,
                       const float* running_mean, const float* running_var, const float* gamma,
                       const float* beta, float eps, int relu, int N, int H, int W, int Cin, int Ho, int Wo,
                       int Cout, int kh, int kw, int stride, int pad, int dil, rgda_stream_t stream);

/* rgda_conv2d (normally the data-gradient, mode 1) with the BatchNorm-backward REDUCTION of the layer that consumes
 * its output fused into the epilogue: with g = the stored result (after the residual add),
 *   g' = g * [bn_y > 0 if relu] * nscale[n][c],  xhat = (bn_x - mean) * invstd  (mean/invstd from bn_mi[group]),
 * ([bn_y > 0] is read from bn_relu_mask instead when that is given, see rgda_bn_train_apply)
 * sums[group][REPLICAS][2][Cout] += (sum g', sum g' * xhat) -- exactly what rgda_bn_bwd_reduce would compute
 * from the stored tensor, without re-reading it.
 * relu == 2 (ABI 6): the consumer's activation was never written (it ran on ITS consumer's operand path,
 * rgda_conv2d_bnin): [bn_y > 0] is recomputed from bn_x as [fma(bn_x, scale, shift) > 0] with the forward's own
 * (scale, shift) = (gamma * invstd, fma(-mean, scale, beta)); bn_gamma / bn_beta f32 [Cout] are needed only then. */
int rgda_conv2d_bnbwd(const void* x, int ldx, const void* wgt, void* y, int ldy, const void* res, int ldres,
                      const uint8_t* res_relu_mask, rgda_stat_t* sums, int groups, const void* bn_y, int bn_ldy, const uint8_t* bn_relu_mask,
                      const void* bn_x, int bn_ldx,
                      const float* bn_mi, const float* bn_nscale, int rows_per_image, int relu,
                      const float* bn_gamma, const float* bn_beta, int N, int H,
                      int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                      int mode, rgda_stream_t stream);

/* BatchNorm (+ ReLU) on the CONSUMER's operand path (ABI 6).  The reference's bottleneck runs conv -> bn -> relu -> conv
 * (regda/_resnets.py:92-112); as separate passes the normalised activation is written and read back once per unit.
 * Here the producing convolution leaves its RAW output and its statistic accumulators, and the consuming convolution
 * applies  a = relu(fma(x, scale, shift)),  scale = gamma * invstd, shift = fma(-mean, scale, beta)  to the operand tile
 * on its way to the matrix pipe (mean / invstd from `stats` exactly as rgda_bn_train_apply derives them: biased batch
 * variance, eps inside the square root).  The activation is never written; padding positions contribute zeros as in the
 * reference (the padding of conv2 pads the ACTIVATION).  One workgroup of the launch also writes `mi` (mean, invstd per
 * group, for the backward pass) and updates running_mean / running_var (momentum, unbiased variance) group after group
 * and num_batches_tracked += groups -- nn.BatchNorm2d's train-mode side effects (regda/resnet.py:170-181 keeps every
 * BatchNorm trainable; tools/train_ssl_reg.py:210-212 runs source then target).
 * The struct is HOST memory holding DEVICE pointers; it is consumed before the call returns. */
typedef struct rgda_bn_operand {
    const rgda_stat_t* stats;       /* [groups][REPLICAS][2][C] (FRAC_FWD) of the producing convolution, complete */
    const float* gamma;             /* f32 [C] */
    const float* beta;              /* f32 [C] */
    float* mi;                      /* NULL or out f32 [groups][2][C]: mean, invstd */
    float* running_mean;            /* NULL or f32 [C], updated in place (both or neither) */
    float* running_var;
    int64_t* num_batches_tracked;   /* NULL or += groups */
    float eps, momentum;
    int groups;                     /* equal blocks of whole images, normalised independently (= stat_groups of the call) */
    int relu;
} rgda_bn_operand;
/* rgda_conv2d (mode 0) whose operand x [N*H*W][ldx] is the RAW output of the producing convolution and bn_in describes
 * the BatchNorm (+ ReLU) between them.  Served: Cin <= 512 and the geometries rgda_conv2d_bnin_supported() reports
 * (1x1 and 3x3 convolutions with >= 512 tiles of 128 x 128, and the 3x3 / dilation 1 convolutions on 32-wide maps);
 * anything else returns RGDA_ERR_UNSUPPORTED and the caller materialises the activation with rgda_bn_train_apply.
 * rgda_conv2d_bnin_supported: 0 = not served, 1 = served, 2 = served AND measured faster than the apply pass it
 * replaces (the model defers a unit only then). */
int rgda_conv2d_bnin_supported(int64_t M, int Cout, int Cin, int kh, int kw, int stride, int pad, int dil, int H, int W,
                               int Ho, int Wo, int groups);
int rgda_conv2d_bnin(const rgda_bn_operand* bn_in, const void* x, int ldx, const void* wgt, void* y, int ldy,
                     const void* res, int ldres, rgda_stat_t* stats, int stat_groups, int N, int H, int W, int Cin,
                     int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, rgda_stream_t stream);

/* The kernel instantiation that serves a convolution call, as rocprofv3 names it ("conv_igemm_kernel<128, 128, 2, 2, 4,
 * false, false>", "conv3x3_halo_kernel<1, 4, true>", ...), decided by the library's own dispatch (nothing is launched):
 * variant 0 = rgda_conv2d (has_stats / stat_groups as in the call), 1 = rgda_conv2d_bneval, 2 = rgda_conv2d_bnbwd,
 * 3 = rgda_conv2d_bnin; rgda_conv2d_wgrad_kernel: the instantiation a layer of rgda_conv2d_wgrad_grouped maps to
 * (layers with the same name share launches).  NULL where the call would be refused.  bench.py labels its per-launch
 * HIP-event timings with these, so that they can be matched against rocprof kernel statistics. */
const char* rgda_conv2d_kernel(int variant, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw,
                               int stride, int pad, int dil, int mode, int has_stats, int stat_groups);

/* Which conv_igemm_kernel<BC, BP, STAGES, ...> instantiation rgda_conv2d picks for a problem: returns
 * BC | BP << 10 | STAGES << 20 (STAGES 82 / 83 = 8-wave workgroups with a 2 / 3 stage ring), or a negative
 * status.  rows_per_group = rows of one BatchNorm group when fused statistics with groups > 1 are requested, else 0.
 * (Nothing in this repository calls it: bench.py and the tests take the instantiation's full name from
 * rgda_conv2d_kernel.  It stays for hosts built against the ABI.) */
int rgda_conv2d_tile(int64_t M, int Cout, int kh, int kw, int Cin, int rows_per_group);

/* Weight gradient: dw[co][tap][ci] (f32, row stride taps*Cin) +=
 *   sum_p dy[p][co] * x[src(p,tap)][ci]   (same geometry as mode 0 above).
 * Reproducible: the pixel (K) dimension of a layer is split over several workgroups only through the workspace --
 * every split leaves its partial tile there, the LAST workgroup of a tile to arrive (a counter per tile) adds the
 * partials in split order 0, 1, ... and is the only one that adds to dw (ABI 4; every split added to dw with fp32
 * atomics before: the arrival order moved the last bits from run to run).  ws: rgda_conv2d_wgrad_workspace bytes, or NULL = never
 * split (slow for layers with few tiles).  The first 64 KiB of ws are tile counters: ZERO them once after
 * allocation; every call leaves them zero.  Calls that share a ws must be ordered on one stream. */
int rgda_conv2d_wgrad(const void* x, int ldx, const void* dy, int lddy, float* dw, int N, int H,
                      int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride,
                      int pad, int dil, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* The weight gradients of several layers in as few launches as possible (same arithmetic as n calls of
 * rgda_conv2d_wgrad, accumulated into each dw).  Layers that map to the same kernel instantiation share a
 * launch (up to 16 per launch): autograd hands the reference one conv-backward at a time
 * (tools/train_ssl_reg.py:236 loss.backward()), but the gradients are only needed by clip + SGD
 * (tools/train_ssl_reg.py:237-238), so the host may collect them while the data-gradient chain runs on.
 * `descs` is a host array; it is consumed before the call returns. */
typedef struct rgda_wgrad_desc {
    const void* x;      /* bf16 [N*H*W][ldx] */
    const void* dy;     /* bf16 [N*Ho*Wo][lddy] */
    float* dw;          /* f32 [Cout][kh*kw][Cin] */
    int ldx, lddy;
    int N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil;
    /* ABI 5: where dw's rows live, so that a gradient can be written straight into a slice of a wider tensor.
     * lddw: elements between consecutive (co, tap) rows of dw (0 = Cin: dense).  co_split (0 = off; a power of two
     * dividing Cout; 1x1 layers only): output row r of the layer is dw row (r % co_split) * (Cout / co_split) +
     * r / co_split -- a layer whose Cout stacks T filters of co_split channels, [t][co], lands in a [co][t][Cin]
     * tensor (the PPM branches of the heads' 3x3 convolution, regda/models/Encoder.py:29-37,54-60). */
    int lddw, co_split;
} rgda_wgrad_desc;
size_t rgda_conv2d_wgrad_workspace(const rgda_wgrad_desc* descs, int n);
const char* rgda_conv2d_wgrad_kernel(const rgda_wgrad_desc* desc);
int rgda_conv2d_wgrad_grouped(const rgda_wgrad_desc* descs, int n, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* Stem im2col: NCHW f32 image (N,3,H,W) -> [N*Ho*Wo][Kp] bf16 patches of the
 * 7x7/2 pad-3 conv (regda/_resnets.py:150-151), k index = (kh*7+kw)*3+c, zero padded to Kp. */
int rgda_stem_im2col(const float* img, void* col, int N, int H, int W, int Ho, int Wo, int Kp,
                     rgda_stream_t stream);

/* The same convolution in ONE kernel straight from the NCHW f32 image (no patch matrix): y PxC bf16 [N*Ho*Wo][ldy],
 * wgt bf16 [64][192] (k = (kh*7+kw)*3+c, zero padded), epilogue as rgda_conv2d (per-group BatchNorm statistics) or
 * rgda_conv2d_bneval (inference BatchNorm + ReLU).  Wo % 64 must be 0 (RGDA_ERR_UNSUPPORTED otherwise: use
 * rgda_stem_im2col + rgda_conv2d).  The image batch is ONE tensor: the row groups are consecutive blocks of images. */
int rgda_stem_conv(const float* img, const void* wgt, void* y, int ldy, rgda_stat_t* stats, int stat_groups, int N,
                   int H, int W, int Ho, int Wo, rgda_stream_t stream);
int rgda_stem_conv_bneval(const float* img, const void* wgt, void* y, int ldy, const float* running_mean,
                          const float* running_var, const float* gamma, const float* beta, float eps, int relu,
                          int N, int H, int W, int Ho, int Wo, rgda_stream_t stream);

/* BatchNorm2d (train) on PxC bf16, nn.BatchNorm2d defaults (eps 1e-5, momentum .1):
 *  finalize: stats rgda_stat_t[REPLICAS][2][C] (sum,sumsq over M rows, FRAC_FWD) -> mean/invstd f32[2][C] in `mi`,
 *            running_mean/var/num_batches_tracked update.  If stats==NULL, eval mode:
 *            mi is filled from the running statistics.
 *  apply   : y = act( (x-mean)*invstd*gamma+beta [+ res] ) [* nscale[n][c]]
 *  bwd     : two passes (reduce, apply) -- see kernels.
 * `groups` (>= 1): the M rows are `groups` equal blocks of rows (the source and the target batch of one
 * SSL step run through the network together) that are normalised INDEPENDENTLY, like the reference's two
 * separate forward calls; stats / sums are laid out [groups][REPLICAS][2][C], mi [groups][2][C]; running
 * statistics are updated group after group. */
int rgda_bn_stats(const void* x, int ldx, rgda_stat_t* stats, int64_t M, int C, rgda_stream_t stream);
int rgda_bn_finalize(const rgda_stat_t* stats, float* mi, float* running_mean, float* running_var,
                     int64_t* num_batches_tracked, int64_t M, int C, int groups, float eps,
                     float momentum, rgda_stream_t stream);
int rgda_bn_apply(const void* x, int ldx, const float* mi, const float* gamma, const float* beta,
                  const void* res, int ldres, const float* nscale, int rows_per_image, void* y,
                  int ldy, int64_t M, int C, int relu, int groups, rgda_stream_t stream);
/* bn_finalize + bn_apply in one launch (the training forward): statistics -> (mean, invstd) -> y, `mi` and the
 * running statistics are written by one designated workgroup per channel block.
 * relu_mask (optional, needs relu): uint8 [M][C/8], bit e of byte k = [y[row][8k+e] > 0] -- the only thing the
 * backward pass needs from y; reading it instead of y saves 15/16 of that operand's HBM traffic there. */
int rgda_bn_train_apply(const void* x, int ldx, const rgda_stat_t* stats, float* mi, float* running_mean,
                        float* running_var, int64_t* num_batches_tracked, const float* gamma,
                        const float* beta, const void* res, int ldres, const float* nscale,
                        int rows_per_image, void* y, int ldy, uint8_t* relu_mask, int64_t M, int C, int relu,
                        int groups, float eps, float momentum, rgda_stream_t stream);
/* sums rgda_stat_t[REPLICAS][2][C] (FRAC_BWD) must be ZERO on entry (the caller clears one arena per backward pass):
 * sums[0] += sum(g'), sums[1] += sum(g' * xhat), g' = g*[y>0]*nscale.  With relu, [y>0] comes from relu_mask
 * when given, else from y.
 * relu == 2 (ABI 6): [y>0] is recomputed from x, [fma(x, gamma * invstd, fma(-mean, gamma * invstd, beta)) > 0] -- the
 * unit's activation was never written (rgda_conv2d_bnin); gamma / beta are needed only then. */
int rgda_bn_bwd_reduce(const void* g, int ldg, const void* y, int ldy, const uint8_t* relu_mask, const void* x,
                       int ldx, const float* mi, const float* nscale, int rows_per_image, rgda_stat_t* sums,
                       int64_t M, int C, int relu, const float* gamma, const float* beta, int groups,
                       rgda_stream_t stream);
/* dx = gamma*invstd*(g' - sum(g')/M - xhat*sum(g' xhat)/M); gmask (optional) = g';
 * dgamma += sum(g' xhat), dbeta += sum(g') (f32, accumulated)
 * relu == 2 (ABI 6, needs beta): the ReLU sign from x as in rgda_bn_bwd_reduce; act_out (optional, bf16 [M][ldact]) then
 * receives the activation relu(fma(x, scale, shift)) itself -- bit for bit what the consuming convolution's operand
 * path fed the matrix pipe -- for that convolution's weight gradient (rgda_conv2d_wgrad), written here beside the
 * read of x this pass does anyway instead of in the forward pass. */
int rgda_bn_bwd_apply(const void* g, int ldg, const void* y, int ldy, const uint8_t* relu_mask, const void* x,
                      int ldx, const float* mi, const float* gamma, const float* nscale,
                      int rows_per_image, const rgda_stat_t* sums, void* dx, int lddx, void* gmask,
                      int ldgm, float* dgamma, float* dbeta, int64_t M, int C, int relu, const float* beta,
                      void* act_out, int ldact, int groups, rgda_stream_t stream);

/* BatchNorm of SMALL maps, several layers per launch (the PPM branches' conv -> BatchNorm -> ReLU on s x s maps,
 * regda/models/Encoder.py:30-51; nn.BatchNorm2d in train mode per statistics group, as rgda_bn_train_apply /
 * rgda_bn_bwd_reduce + rgda_bn_bwd_apply).  One workgroup owns 128 channels of one layer and all of its rows: it forms the
 * statistics itself -- sums of the stored bf16 values in a fixed order -- and applies them; up to eight descriptors share a
 * launch.  M = all rows (groups * rows per group), rows per group in [2, 320] forward, <= 320 backward (a workgroup keeps
 * its rows in registers); larger maps take the general entry points.
 * Forward: y = [relu]((x - mean) * invstd * gamma + beta), mi[groups][2][C] = (mean, invstd), running statistics updated
 * group after group, num_batches_tracked += groups, relu_mask (optional) = sign bits of y.
 * Backward: dx, dgamma += , dbeta += (atomic adds, as rgda_bn_bwd_apply); the ReLU gate from relu_mask or y. */
typedef struct rgda_bn_small_fwd_desc {
    const void* x; void* y; uint8_t* relu_mask; const float* gamma; const float* beta; float* mi;
    float* running_mean; float* running_var; int64_t* num_batches_tracked;
    int64_t M; int ldx, ldy, C, groups, relu; float eps, momentum;
} rgda_bn_small_fwd_desc;
typedef struct rgda_bn_small_bwd_desc {
    const void* g; const void* y; const uint8_t* relu_mask; const void* x; void* dx; const float* mi; const float* gamma;
    float* dgamma; float* dbeta;
    int64_t M; int ldg, ldy, ldx, lddx, C, groups, relu;
} rgda_bn_small_bwd_desc;
int rgda_bn_train_small(const rgda_bn_small_fwd_desc* descs, int n, rgda_stream_t stream);
int rgda_bn_bwd_small(const rgda_bn_small_bwd_desc* descs, int n, rgda_stream_t stream);

/* MaxPool2d(3,2,1) on PxC bf16 (regda/_resnets.py:153); idx = argmax tap (uint8). */
int rgda_maxpool_fwd(const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, int Ho,
                     int Wo, rgda_stream_t stream);
int rgda_maxpool_bwd(const void* gy, const uint8_t* idx, void* gx, int N, int H, int W, int C,
                     int Ho, int Wo, rgda_stream_t stream);
/* The same pooling over relu(BatchNorm(x)) of the RAW stem convolution output x (rgda_bn_operand above; conv1 -> bn1 ->
 * relu -> maxpool, regda/_resnets.py:150-153): the stem's activation is never written. */
int rgda_maxpool_fwd_bnin(const rgda_bn_operand* bn_in, const void* x, void* y, uint8_t* idx, int N, int H, int W,
                          int C, int Ho, int Wo, rgda_stream_t stream);

/* InstanceNorm2d(C, affine=False, eps) (regda/models/Encoder.py:123,146-147).
 * x [N*HW][ldx] bf16 -> y0,y1 (optional, bf16 PxC, ld ldy) and feat NCHW f32 (optional);
 * mi f32[N][2][C] mean/invstd saved for backward. */
int rgda_instnorm_fwd(const void* x, int ldx, void* y0, void* y1, int ldy, float* feat_nchw,
                      float* mi, int N, int HW, int C, float eps, rgda_stream_t stream);
/* g = ga + gb + gc (bf16 PxC, any may be NULL; ga/gb share ldg); dx bf16 */
int rgda_instnorm_bwd(const void* ga, const void* gb, int ldg, const void* gc, int ldgc,
                      const void* x, int ldx, const float* mi, void* dx, int lddx, int N, int HW,
                      int C, rgda_stream_t stream);

/* Spatial linear map shared by AdaptiveAvgPool2d / bilinear(align_corners=False)
 * and their transposes (regda/models/Encoder.py:16-18,48-51):
 *   out[n][i][c] (+)= sum_j Mx[i][j] * in[n][j][c],  Mx f32 [I][J] row-major.
 * in: bf16 [N*J][ldin]; out: bf16 [N*I][ldout] (out_f32 != 0: f32). */
int rgda_spatial_mix(const void* in, int ldin, const float* Mx, void* out, int ldout, int N, int I,
                     int J, int C, int accumulate, int out_f32, rgda_stream_t stream);

/* out[n][i][c] = sum over nsrc <= 4 sources of sum_j mats[q][i][j] * ins[q][n][j][c]  (bf16 out, no accumulate):
 * the summed backward of the four adaptive-average-pool branches of one PPM head pair in a single pass.
 * ins/ldins/mats/Js are HOST arrays of length nsrc (device pointers inside). */
int rgda_spatial_mix_multi(int nsrc, const void* const* ins, const int* ldins, const float* const* mats,
                           const int* Js, void* out, int ldout, int N, int I, int C, rgda_stream_t stream);

/* 1x1 classifier with bias (regda/models/Encoder.py:40): hidden [M][ldh] bf16 ->
 * logits NCHW f32 (N,ncls,HW); backward gives dhidden (bf16), dW f32[ncls][C] +=, db +=.  6 <= ncls <= 16.
 * ws (optional, rgda_classifier_bwd_workspace bytes): per-workgroup partial sums + a deterministic reduction instead of
 * atomics (NULL: atomics). */
int rgda_classifier_fwd(const void* hidden, int ldh, const float* w, const float* bias,
                        float* logits, int N, int HW, int C, int ncls, rgda_stream_t stream);
size_t rgda_classifier_bwd_workspace(int64_t M, int C, int ncls);
int rgda_classifier_bwd(const void* hidden, int ldh, const float* w, const float* glogits,
                        void* dhidden, int lddh, float* dw, float* db, int N, int HW, int C,
                        int ncls, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* ------------------------------------------------------------- optimizer   */

/* sum of squares of a flat f32 buffer -> out[0] (f32, overwritten).  ws: f32[1024]. */
int rgda_sumsq(const float* g, int64_t n, float* out, float* ws, rgda_stream_t stream);

/* clip_grad_norm_(max_norm, 2) + SGD(momentum, weight_decay) + EMA shadow + bf16 mirror
 *   tools/train_ssl_reg.py:174-175,239-241; regda/utils/ema.py:46-51.
 * coef = min(1, max_norm / (sqrt(gnorm_sq[0]) * gscale + 1e-6)); g = g*gscale*coef (gscale = 1/world)
 * v = momentum*v + (g + wd*p); p -= lr*v; shadow = (1-d)*p + d*shadow (if shadow);
 * p_bf16 = bf16(p) (if given); shadow_bf16 = bf16(shadow) (if given: the EMA teacher's mirror).
 * lr is read from device memory (lr_dev[0]). */
int rgda_sgd_step(float* p, const float* g, float* v, float* shadow, void* p_bf16, void* shadow_bf16,
                  const float* gnorm_sq, const float* lr_dev, int64_t n, float momentum,
                  float weight_decay, float max_norm, float gscale, float ema_decay,
                  int first_step, rgda_stream_t stream);

/* The stem's weight gradient straight from the NCHW f32 image (no patch matrix): dw f32 [64][147], k = (kh*7+kw)*3+c,
 * += sum_p dy[p][co] * bf16(patch(p)[k]) (the products rgda_stem_im2col + rgda_conv2d_wgrad form, summed in a fixed order:
 * reproducible).  dy bf16 [N*Ho*Wo][lddy].  ws: rgda_stem_wgrad_workspace(N, H, W) bytes (0 = this geometry is not
 * served), 16-byte aligned; calls that share it must be ordered on one stream.  Wo % 64 must be 0
 * (RGDA_ERR_UNSUPPORTED otherwise).  Replaces the tail of regda/_resnets.py:150-151's backward. */
size_t rgda_stem_wgrad_workspace(int N, int H, int W);
int rgda_stem_wgrad(const float* img, const void* dy, int lddy, float* dw, void* ws, size_t ws_bytes, int N, int H,
                    int W, int Ho, int Wo, rgda_stream_t stream);

/* w [Co][T][Ci] f32 -> wt [Ci][T][Co] bf16 (weights for the data-gradient pass). */
int rgda_weight_transpose_bf16(const float* w, void* wt, int Co, int T, int Ci, rgda_stream_t stream);
/* every derived bf16 weight layout of a model in one launch: device table[n][8] int64 = {src f32*, dst bf16*,
 * Co, T, Ci, first_block, src_ld, mode}.  src element (co,tap,ci) = src[(co*T+tap)*src_ld + ci] (src_ld > Ci: a
 * channel slice of a wider tensor); mode 0: dst[ci][tap][co] (the data-gradient operand), 1: dst[tap][co][ci],
 * 2: dst[co][tap][ci].  A row owns ceil(Ci/RGDA_LAYOUT_TILE)*ceil(Co/RGDA_LAYOUT_TILE)*T consecutive blocks starting
 * at first_block. */
int rgda_weight_transpose_batched(const int64_t* table, int n, int64_t total_blocks, rgda_stream_t stream);
int rgda_cast_bf16(const float* src, void* dst, int64_t n, rgda_stream_t stream);
int rgda_cast_f32(const void* src_bf16, float* dst, int64_t n, rgda_stream_t stream);
/* Gradient exchange with bf16 payloads and fp32 accumulation (regda_amd/ddp.py, payload 'bf16'; the reference has no
 * data-parallel path): recv bf16 [world][shard_elems] = this rank's shard of a bucket as every rank sent
 * it (all-to-all); out bf16 [shard_elems] = bf16(sum over ranks IN RANK ORDER of float(recv[r])) -- the same bits on
 * every rank.  shard_elems % 8 == 0. */
int rgda_ddp_accumulate_bf16(const void* recv, int world, void* out, int64_t shard_elems, rgda_stream_t stream);

/* ---- the collectives themselves, through RCCL (xGMI), for a host without torch.distributed ("RCCL wrappers
 * for (e)"; the reference is single-GPU, tools/train_ssl_reg.py has no counterpart).  One communicator per process and
 * GPU: rank 0 draws the 128-byte id (rgda_comm_unique_id) and the HOST ships it to the other ranks by whatever channel it
 * has (a file, a socket, MPI, a torch.distributed store); every rank then calls rgda_comm_init on the device it has made
 * current.  The calls enqueue on the caller's stream like every other entry point; buffers are caller-owned device
 * memory.  dtype: RGDA_COMM_*.  librccl.so is resolved at the first call (a copy the process already holds is
 * preferred); without it these return RGDA_ERR_UNSUPPORTED and nothing else of the library is affected.
 *   all_reduce : buf[n] <- sum over ranks, in place (the flat fp32 gradient's buckets, the prototype statistics
 *                sums[c][k] + cnt[c] of rgda_proto_stats, ClassBalance's int64 pixel counts)
 *   all_to_all : rank r's send[j * n_per_rank ...] -> rank j's recv[r * n_per_rank ...]   (bf16 payload, phase 1)
 *   all_gather : recv[r * n_per_rank ...] <- rank r's send[n_per_rank]                    (bf16 payload, phase 2) */
typedef void* rgda_comm_t;
#define RGDA_COMM_ID_BYTES 128
#define RGDA_COMM_F32 0
#define RGDA_COMM_BF16 1
#define RGDA_COMM_I64 2
#define RGDA_COMM_F64 3
int rgda_comm_unique_id(void* id_128_bytes);
int rgda_comm_init(const void* id_128_bytes, int rank, int world, rgda_comm_t* comm);
int rgda_comm_destroy(rgda_comm_t comm);
int rgda_comm_all_reduce(rgda_comm_t comm, void* buf, int64_t n, int dtype, rgda_stream_t stream);
int rgda_comm_all_gather(rgda_comm_t comm, const void* send, void* recv, int64_t n_per_rank, int dtype,
                         rgda_stream_t stream);
int rgda_comm_all_to_all(rgda_comm_t comm, const void* send, void* recv, int64_t n_per_rank, int dtype,
                         rgda_stream_t stream);
/* rows of K f32 -> rows of Kp bf16, zero padded (stem weights [64][147] -> [64][192]); and the
 * reverse accumulation dst[R][K] f32 += src[R][Kp] f32 for the stem weight gradient. */
int rgda_pad_cast_bf16(const float* src, void* dst, int R, int K, int Kp, rgda_stream_t stream);
int rgda_unpad_acc_f32(const float* src, float* dst, int R, int K, int Kp, rgda_stream_t stream);
/* The small chores of a step as kernels of this library (so that a step launches nothing from torch or the runtime's
 * blit kernels): clear a buffer (16-byte aligned); up to four device -> device copies in one launch (16-byte aligned,
 * sizes multiples of 16; dsts / srcs / bytes are HOST arrays); one f32 word (the learning rate the optimizer reads from
 * device memory); Dropout2d(p) keep masks, scaled by 1 / (1 - p) (regda/models/Encoder.py:39), from a counter-based
 * generator: element i depends on (seed, i) only. */
int rgda_fill_zero(void* p, size_t bytes, rgda_stream_t stream);
int rgda_copy_multi(int n, void* const* dsts, const void* const* srcs, const size_t* bytes, rgda_stream_t stream);
int rgda_set_f32(float* p, float value, rgda_stream_t stream);
int rgda_dropout_mask(float* out, int64_t n, float p, uint64_t seed, rgda_stream_t stream);
/* out = a + b (bf16, PxC) */
int rgda_add_bf16(const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t M,
                  int C, rgda_stream_t stream);

/* ------------------------------------------------------------- teacher / pseudo-label harness */

/* One view of the 8-view test-time augmentation of regda/utils/tools.py:132-152 (ttach 0.0.3:
 * Compose([HorizontalFlip(), Rotate90([0,90,180,270])]), un-vendored, restated).  With R = torch.rot90(., 1, (2,3))
 * and F = flip(3): flip_first=1 -> dst = R^k(F^f(src)) (augment_image), flip_first=0 -> dst = F^f(R^k(src))
 * (deaugment_mask with k := (4-k)%4).  dst (+)= scale * view; fp32 NCHW; output is Ws x Hs for odd k. */
int rgda_dihedral_nchw(const float* src, float* dst, int N, int C, int Hs, int Ws, int hflip, int rot_k,
                       int flip_first, float scale, int accumulate, rgda_stream_t stream);

/* Sliding-window inference of regda/utils/tools.py:61-97 (pre_slide): crop + zero-pad one window to the tile size
 * (tools.py:79-80), add a tile of predictions into the full map and bump the visit count (tools.py:91-93),
 * divide by the count (tools.py:95). */
/* pad_image exactly as written (tools.py:51-58): tnf.pad(img, (0, 0, top, bottom)) pads the ROW dimension (top by
 * rows_missing, bottom by cols_missing; negative = crop) and leaves W alone; dst has h + top + bottom rows. */
int rgda_pad_rows_nchw(const float* src, float* dst, int N, int C, int h, int w, int top, int bottom,
                       rgda_stream_t stream);
int rgda_window_crop(const float* full, float* tile, int N, int C, int Hf, int Wf, int y1, int x1, int h, int w,
                     int Th, int Tw, rgda_stream_t stream);
int rgda_window_accumulate(const float* tile, float* full, float* count, int N, int C, int Hf, int Wf, int y1,
                           int x1, int h, int w, int Th, int Tw, rgda_stream_t stream);
int rgda_window_normalise(float* full, const float* count, int N, int C, int Hf, int Wf, rgda_stream_t stream);

/* Batched sliding-window inference: the window loop of pre_slide with K windows per network forward.  A window is a row
 * (image, y1, x1) of the int32 [K][3] DEVICE table `windows`; every window has the full tile size Th x Tw and lies inside
 * its image (H >= Th, W >= Tw).  V = `views` is 1, or 8 (tta_predict's views (flip, k) = (v >> 2, v & 3), Th == Tw).
 * A table row outside the images is not read: it sets *flag (optional, device int) to 1 and contributes zeros / nothing.
 *
 * rgda_window_gather: out f32 [K*V][C][Th][Tw], row w*V + v = view v of window w, bit for bit rgda_window_crop followed
 * by rgda_dihedral_nchw(flip_first = 1).  The source is src_f32 (f32 [n][C][H][W]) or src_u8 (uint8 [n][H][W][3], HWC as
 * imread returns it, C = 3) through lut (f32 [3][256], device: the rgda_augment_tiles normalisation table); exactly one.
 *
 * rgda_window_scatter: adds pred f32 [K*V][C][Th][Tw] into full f32 [n][C][H][W] and count f32 [n][1][H][W], bit for bit
 * the sequential rgda_window_accumulate calls of the K windows in table order (with V = 8 each window's value is first
 * the mean of its de-augmented views, scale 1/8 fused into the sum, in view order, as tta_predict forms it).  One thread
 * per pixel of the flattened image rows [row0, row0 + rows) of the n*H rows, which must cover the K windows; no atomics.
 * K <= 1024.
 *
 * rgda_window_finish: full /= count (rgda_window_normalise), then the first maximum over C into labels_u8 (uint8
 * [n][H][W], C <= 256) and / or labels_i64 (int64 [n][H][W]) (rgda_argmax_nchw), and with y_true (int64 [n][H][W]) the
 * confusion matrix cm int64 [C][C] += counts of the pixels with y_true >= 0 (rgda_confusion_accumulate; flag |= 1 on a
 * label >= C; C <= 64).  Each output is optional; y_true and cm go together and need flag.
 * Errors before any launch: null pointers, sizes outside the above (RGDA_ERR_ARG). */
int rgda_window_gather(const float* src_f32, const uint8_t* src_u8, const float* lut, const int32_t* windows, int K,
                       int views, int n, int C, int H, int W, int Th, int Tw, float* out, int* flag,
                       rgda_stream_t stream);
int rgda_window_scatter(const float* pred, const int32_t* windows, int K, int views, int n, int C, int H, int W, int Th,
                        int Tw, int row0, int rows, float* full, float* count, int* flag, rgda_stream_t stream);
int rgda_window_finish(float* full, const float* count, int n, int C, int H, int W, uint8_t* labels_u8,
                       int64_t* labels_i64, const int64_t* y_true, int64_t* cm, int* flag, rgda_stream_t stream);

/* tnf.interpolate(mode='bilinear', align_corners=True) of the soft labels to the dataset size
 * (regda/gast/pseudo_generation.py:135). */
int rgda_resize_bilinear_ac(const float* src, float* dst, int N, int C, int h, int w, int H, int W,
                            rgda_stream_t stream);

/* Multi-scale testing (regda/utils/tools.py:108-129, predict_multiscale): the batched window loop over the image resampled
 * to Hs x Ws, and the per-scale result brought back to H x W and added to the sum over the scales.  The resampling in both
 * directions is rgda_resize_bilinear_ac's arithmetic (ndimage.zoom(order=1, prefilter=False) is align_corners=True
 * bilinear), fused so that neither the scaled image nor the normalised scaled probabilities are ever stored.
 *
 * rgda_window_gather_scaled: rgda_window_gather on the Hs x Ws image, bit for bit rgda_window_gather applied to
 * rgda_resize_bilinear_ac(normalised source, (Hs, Ws)).  Window rows (image, y1, x1) index the Hs x Ws image and are checked
 * against it (Hs >= Th, Ws >= Tw); a uint8 source goes through lut tap by tap, before the blend (normalise, then resize).
 *
 * rgda_scale_merge: acc f32 [n][C][H][W] += rgda_resize_bilinear_ac(full_s / count_s, (H, W)) and cnt f32 [n][1][H][W] += 1,
 * bit for bit rgda_window_normalise(full_s f32 [n][C][Hs][Ws], count_s f32 [n][1][Hs][Ws]), the resize and the add (NaN where
 * those give NaN: a count of 0 under a tap); full_s is only read.  rgda_window_finish(acc, cnt) then gives the mean.
 * Errors before any launch: null pointers, sizes outside the above (RGDA_ERR_ARG). */
int rgda_window_gather_scaled(const float* src_f32, const uint8_t* src_u8, const float* lut, const int32_t* windows, int K,
                              int views, int n, int C, int H, int W, int Hs, int Ws, int Th, int Tw, float* out, int* flag,
                              rgda_stream_t stream);
int rgda_scale_merge(const float* full_s, const float* count_s, int n, int C, int Hs, int Ws, int H, int W, float* acc,
                     float* cnt, rgda_stream_t stream);

/* ------------------------------------------------------------- training augmentation of raw tiles */

/* BaseData.__getitem__ + the training transforms (regda/datasets/basedata.py:68-98, regda/aug/augmentation.py; the
 * albumentations pipeline of configs/ToPotsdam.py:43-56) for a batch of N raw tiles of one domain, one launch.
 *   img       uint8 [N][Hi][Wi][3] (HWC, as imread returns it; 4-byte aligned)   -> img_out   f32 [N][3][Ho][Wo]
 *   label     uint8 [N][Hi][Wi] or NULL                                            -> label_out int64 [N][Ho][Wo]
 *   soft      f32 [N][C][Hi][Wi] or NULL (1 <= C <= 8)                             -> soft_out  f32 [N][C][Ho][Wo]
 *   regs      int32 [N][Hi][Wi] or NULL                                            -> regs_out  int64 [N][1][Ho][Wo]
 *   lut       f32 [3][256]: img_out = lut[channel][byte] -- the pipeline's normalisation (and clamp) tabulated on the host;
 *   label_lut int32 [256]:   label_out = label_lut[byte] -- the dataset offset and `mask[mask >= n_classes] = ignore`;
 *   params    int32 [N][4] (y0, x0, d, 0) per sample; lut, label_lut, params: DEVICE memory.
 * Every output of sample n is gathered through one index map: output pixel (i, j) reads input pixel (y0 + y, x0 + x)
 * with (u, v) = t ? (j, i) : (i, j), y = fr ? Ho-1-u : u, x = fc ? Wo-1-v : v, where the dihedral element
 * d = t | fr << 1 | fc << 2 (t: transpose, fr: flip rows, fc: flip columns; t requires Ho == Wo).  With
 * H = hflip (d 4), V = vflip (d 2) and R = torch.rot90(x, 1, [1, 2]) = np.rot90 on HW (R[i][j] = X[j][S-1-i], d 5):
 *   reference (mag) pipeline: crop, then H, V, R, each drawn:  d = R ? (1 | V << 1 | !H << 2) : (V << 1 | H << 2)
 *   albumentations pipeline:  crop, then at most one of H (4), V (2), R^k (k = 1: 5, 2: 6, 3: 3).
 * The kernel does no floating-point arithmetic and no atomics.  Errors before any launch: null img / params / lut /
 * img_out, N < 1, Ho > Hi or Wo > Wi, a label without label_lut / label_out, soft with C < 1 or without soft_out, regs
 * without regs_out, a misaligned input (RGDA_ERR_ARG); C > 8 (RGDA_ERR_UNSUPPORTED).  params live on the device, so a
 * sample whose crop leaves the input, whose d is outside 0..7 or odd with Ho != Wo is checked there: its outputs are
 * not written and *flag (optional, device int) is set to 1. */
int rgda_augment_tiles(const uint8_t* img, const uint8_t* label, const float* soft, const int32_t* regs,
                       const int32_t* params, int N, int Hi, int Wi, int C, int Ho, int Wo, const float* lut,
                       const int32_t* label_lut, float* img_out, int64_t* label_out, float* soft_out, int64_t* regs_out,
                       int* flag, rgda_stream_t stream);

/* Random scale and rotation of the same raw tiles: every plane of sample n is warped by ONE affine map, one launch per
 * batch of one domain.  This project's own specification (the reference has no such transform), restated in integers
 * by tests/affine_ref.py.  Inputs, outputs and tables as rgda_augment_tiles, except 1 <= C <= 16 (the soft planes are
 * gathered, not staged) and Ho, Wo may exceed Hi, Wi (zooming out fills).
 *   params int32 [N][8] (cy, cx, a00, a01, a10, a11, fill, 0) per sample, DEVICE memory; fill = r | g << 8 | b << 16.
 * With u = 2i + 1 - Ho, v = 2j + 1 - Wo, output pixel (i, j) has the source coordinate, in 1/65536 pixel and int64,
 *   Y = cy + a00 u + a01 v,  X = cx + a10 u + a11 v
 * where a_kl = round(M_kl * 32768) for the output-to-source linear map M in centred coordinates and
 * cy = round((y0 + Ho/2) * 65536) is the crop's centre in the raw tile (pixel centre k at k + 0.5; cx likewise).
 *   image:   Yp = Y - 32768, y = Yp >> 16 (arithmetic), fy = (Yp & 0xFFFF) >> 8; x, fx likewise from X;
 *            byte = ((256-fx)(256-fy) p00 + fx (256-fy) p01 + (256-fx) fy p10 + fx fy p11 + 32768) >> 16 per channel with
 *            p00 = img[y][x], p01 = img[y][x+1], p10 = img[y+1][x], p11 = img[y+1][x+1]; a tap outside the input is the
 *            channel's fill byte; img_out = lut[channel][byte].  No floating-point arithmetic.
 *   label:   label_lut[label[Y >> 16][X >> 16]]; outside the input, ignore_label (not through the table).
 *   regions: regs[Y >> 16][X >> 16] widened; outside the input, 0 ("no region", which LRH leaves alone).
 *   soft:    the image's taps and weights in f32, (w00 p00 + w01 p01 + w10 p10 + w11 p11) * 2^-16 summed in that order; a
 *            tap outside contributes 0, so an out-of-frame pixel is all zero and pseudo_selection never selects it.
 * A row whose M is a signed permutation with an integer crop has fx = fy = 0 everywhere and gives rgda_augment_tiles'
 * outputs for the matching (y0, x0, d) bit for bit.  No atomics.  Errors before any launch: null img / params / lut /
 * img_out, a size below 1, a label without label_lut / label_out, soft with C < 1 or without soft_out, regs without
 * regs_out, a misaligned input (RGDA_ERR_ARG); Hi or Wi above 16384, Ho or Wo above 8192, C > 16, N > 65535 (one grid row
 * per sample) (RGDA_ERR_UNSUPPORTED).  Checked on the device, per row: |a_kl| <= 131072 (a scale inside [1/4, 4]), cy in
 * [0, Hi * 65536], cx in [0, Wi * 65536], column 7 zero, fill below 2^24; the outputs of a row that fails are not
 * written and *flag (optional, device int) is set to 1.  Every tap is bounds-checked, so no row reads outside the
 * input. */
int rgda_augment_affine(const uint8_t* img, const uint8_t* label, const float* soft, const int32_t* regs,
                        const int32_t* params, int N, int Hi, int Wi, int C, int Ho, int Wo, const float* lut,
                        const int32_t* label_lut, int ignore_label, float* img_out, int64_t* label_out, float* soft_out,
                        int64_t* regs_out, int* flag, rgda_stream_t stream);

/* ------------------------------------------------------------- cross-domain mixing */

/* ClassMix and CutMix across the domains (regda/utils/classmix.py:17-53, regda/utils/cutmix.py:15-31): the pixels of the
 * source batch that a predicate selects are pasted over the target batch, in place, one launch for the whole batch.
 * Sample n of the source pairs with sample n of the target, as in the reference.
 *   img_s f32 [N][3][H][W], label_s int64 [N][H][W]: the source (read only)
 *   img_t f32 [N][3][H][W]; label_t int64 [N][H][W], soft_t f32 [N][C][H][W], regs_t int64 [N][H][W], each or NULL
 * Per pixel (n, y, x) with l = label_s[n][y][x]:
 *   RGDA_MIX_CLASS: cond = 0 <= l < C && (class_bits >> l) & 1        (classmix.py:42-50 with class_ids as a bit set)
 *   RGDA_MIX_BOX:   cond = y0 <= y < y1 && x0 <= x < x1               (cutmix.py:29-30)
 * Where cond holds: img_t[n][:][y][x] = img_s[n][:][y][x]; label_t = l; soft_t[n][c] = (l == c) ? 1 : 0 for every c (so
 * a box pixel whose source label is ignore_label gets all-zero planes); regs_t = 0, the id LRH leaves alone
 * (local_region_homog.py:149-151).  Where it does not hold nothing is written.  The reference knows hard labels only;
 * soft_t and regs_t are this library's extension to the inputs its SSL step takes.
 * A label that is neither in [0, C) nor ignore_label sets *flag (optional, device int) to 1: it is not pasted in class
 * mode and is pasted as it is, with all-zero soft planes, in box mode (where only the labels inside the box are read).
 * 16-byte accesses when W % 4 == 0 and every given pointer is 16-byte aligned, element accesses otherwise.  No
 * arithmetic, no atomics: two runs are bit-identical.
 * Errors before any launch (RGDA_ERR_ARG): null img_s / label_s / img_t; N, H or W < 1; C outside 1..32; an unknown
 * mode; in class mode a bit of class_bits at or above C; in box mode a box outside 0 <= y0 <= y1 <= H,
 * 0 <= x0 <= x1 <= W.  An empty class set or an empty box returns RGDA_OK without a launch. */
enum rgda_mix_mode { RGDA_MIX_CLASS = 0, RGDA_MIX_BOX = 1 };
int rgda_domain_mix(const float* img_s, const int64_t* label_s, float* img_t, int64_t* label_t, float* soft_t,
                    int64_t* regs_t, int N, int C, int H, int W, int mode, uint32_t class_bits, int y0, int y1, int x0,
                    int x1, int ignore_label, int* flag, rgda_stream_t stream);

/* rgda_domain_mix with the predicate of every image read from a device table, and the image written out of place: the
 * mix a training step does on its own inputs (DACS: the student sees the mixed tile, the teacher the clean one), where
 * the arguments of a recorded launch are frozen and the table is not.
 *   table int32 [N][RGDA_MIX_TABLE_COLS], 16-byte aligned: row n = {class_bits, y0, y1, x0, x1, 0, 0, 0}, the predicate
 *     of image n as rgda_domain_mix takes it; `mode` says which columns are read and stays a launch argument.
 *   img_in f32 [N][3][H][W] (read only), img_out f32 [N][3][H][W]: img_out[n] = cond ? img_s[n] : img_in[n], EVERY pixel
 *     written (img_out may be img_in: the in-place mix).  Both NULL: no image work, the call that pastes labels.
 *   label_t int64 [N][H][W], soft_t f32 [N][C][H][W], each or NULL: pasted in place, as rgda_domain_mix does.
 * cond, the pasted values, the flag, the 16-byte route (W % 4 == 0 and every given pointer 16-byte aligned) and its
 * element fallback are those of rgda_domain_mix with row n's values, image by image: a row with class_bits == 0 or an
 * empty box pastes nothing, reads no label and sets no flag.  The rows are read on the device and cannot be refused
 * before the launch: a class bit at or above C selects nothing, and a box is cut to the tile by construction (only the
 * tile's pixels are visited), so no row makes the kernel leave its tensors.
 * Errors before any launch (RGDA_ERR_ARG): null img_s / label_s; null or misaligned table; N, H or W < 1; C outside
 * 1..32; an unknown mode; img_in without img_out or img_out without img_in. */
#define RGDA_MIX_TABLE_COLS 8
int rgda_domain_mix_table(const float* img_s, const int64_t* label_s, const float* img_in, float* img_out,
                          int64_t* label_t, float* soft_t, const int32_t* table, int N, int C, int H, int W, int mode,
                          int ignore_label, int* flag, rgda_stream_t stream);

/* The DACS draw on the device (half of the classes that OCCUR in each source label map): writes table[n][0], the
 * class_bits of image n, and leaves the other columns alone.
 *   label_s int64 [N][H][W]; ranks uint8 [N][C], row n a permutation of 0..C-1 (the host's draw, rgda_mix_write_table)
 *   present(n) = the classes of [0, C) that occur in label_s[n], P = |present(n)|
 *   selected(n) = the (P + 1) / 2 (integer division) classes of present(n) with the smallest ranks[n][c]; P = 0: none.
 *     Equal ranks (not a permutation) are ordered by class id, and a rank at or above C never selects its class: a row
 *     of 255s is how a step says "no mix for this batch" without changing its launch sequence.
 *   ws: workspace of N uint32 words (4-byte aligned), the presence sets; zeroed BY the call, any contents on entry.
 * A label that is neither in [0, C) nor ignore_label sets *flag (optional, device int) to 1 and is otherwise skipped.
 * Three launches: clear ws; presence (many workgroups per image, 16-byte loads where H * W is even and label_s is
 * 16-byte aligned, an OR per wave, per workgroup, then one atomic OR per workgroup); the choice (C threads per image).
 * Presence is an OR, so the result does not depend on the order of anything: two runs are bit-identical.
 * Errors before any launch (RGDA_ERR_ARG): null label_s / ranks / ws; null or misaligned table; N, H or W < 1; C
 * outside 1..32. */
int rgda_mix_select_classes(const int64_t* label_s, const uint8_t* ranks, int32_t* table, uint32_t* ws, int N, int C,
                            int H, int W, int ignore_label, int* flag, rgda_stream_t stream);

/* The host's draw -> device, carried IN THE KERNEL ARGUMENTS of one launch (as rgda_set_f32 carries the learning rate):
 * nothing is staged in host memory that a later call could overwrite before the device has read it, so a host that runs
 * a step ahead of the device is safe.
 *   table int32 [N][RGDA_MIX_TABLE_COLS], 16-byte aligned: every row becomes {class_bits, y0, y1, x0, x1, 0, 0, 0}
 *     (all zero: the empty table, which pastes nothing in either mode)
 *   ranks uint8 [N][C] on the device and ranks_host, N * C bytes of HOST memory read during the call, both or neither:
 *     ranks = ranks_host (what rgda_mix_select_classes reads).  A recorded plan must not table this call with a host
 *     pointer; the step calls it from a host action.
 * N above RGDA_MIX_WRITE_MAX_IMAGES (the images the argument block holds): RGDA_ERR_UNSUPPORTED.  RGDA_ERR_ARG: null or
 * misaligned table; N < 1; C outside 1..32; a bit of class_bits at or above C; a box that is not 0 <= y0 <= y1,
 * 0 <= x0 <= x1; ranks without ranks_host or the reverse. */
#define RGDA_MIX_WRITE_MAX_IMAGES 16
int rgda_mix_write_table(int32_t* table, uint8_t* ranks, const uint8_t* ranks_host, int N, int C, uint32_t class_bits,
                         int y0, int y1, int x0, int x1, rgda_stream_t stream);

/* ------------------------------------------------------------- strong (photometric) augmentation of the student's tile */

/* Colour jitter and Gaussian blur of normalised tiles, image by image from a device table: the perturbation of the
 * student's view in consistency training (mean teacher, DACS).  The reference has no such pass; the semantics are this
 * library's and tests/strong_ref.py restates them in fp64.
 *   img_in  f32 [N][3][H][W] (read only): v = (raw - mean_c) / std_c with raw in 0..255, as the training step sees tiles
 *   img_out f32 [N][3][H][W], every pixel written.  OUT OF PLACE ONLY: a blurred pixel reads its neighbours' inputs, which
 *     other workgroups would already have overwritten, so img_out overlapping img_in is refused (RGDA_ERR_ARG).
 *   table   f32 [N][RGDA_STRONG_TABLE_COLS], 16-byte aligned, DEVICE memory: row n = {fb, fc, fs, theta, sigma, flags, 0, 0};
 *     flags (an integer value) bit 0: jitter on, bit 1: blur on.
 *   mean_*, std_* (r, g, b): the normalisation the tiles carry; std_* > 0.
 * An image with both bits clear is copied bit for bit (16-byte moves where the route allows): no arithmetic touches it, so
 * NaN and inf pass through.  Otherwise, per pixel, u = (v * std_c + mean_c) / 255, clamp = clamp to [0, 1], and
 *   1. brightness  u <- clamp(u * fb)
 *   2. contrast    m = the mean over the WHOLE image of grey(u) = 0.299 r + 0.587 g + 0.114 b, taken after step 1;
 *                  u <- clamp((u - m) * fc + m)
 *   3. saturation  g = grey(u) of the pixel; u <- clamp((u - g) * fs + g)
 *   4. hue         u <- clamp(M u), M = T^-1 R(theta) T, nine entries built once per image (in fp64, rounded once):
 *                  T = {{0.299, 0.587, 0.114}, {0.596, -0.274, -0.322}, {0.211, -0.523, 0.312}} (RGB -> YIQ), T^-1 its
 *                  inverse to double precision, R(theta) the rotation of (I, Q) by theta radians:
 *                  I' = cos(theta) I - sin(theta) Q, Q' = sin(theta) I + cos(theta) Q
 *   5. blur, bit 1: a separable Gaussian of standard deviation sigma and radius R = ceil(3 * sigma) (that product in fp32);
 *                  taps exp(-d^2 / (2 sigma^2)), d = -R..R, normalised to sum 1 (built in fp64, rounded once); the
 *                  horizontal pass, then the vertical one; borders by reflection without repeating the edge pixel
 *                  (x[-1] -> x[1], x[W] -> x[W-2]).  It acts on the values after step 4, or on u itself when bit 0 is clear
 *   6. v' = (255 u - mean_c) / std_c
 * Steps 1 to 4 run only with bit 0, always in this order.  Every halo pixel gets the same pointwise steps as an interior
 * pixel.  Served: 0 < sigma <= 4 (R <= RGDA_STRONG_MAX_RADIUS), H > R and W > R; rgda_strong_write_table refuses rows
 * outside that.  The rows are read on the device and cannot be refused here: a row that asks for a blur outside the served
 * range is copied unchanged and sets *flag (optional, device int) to 1; every source index is cut to the image.
 * m is order-independent: every grey value is rounded to a multiple of 2^-24 and the image's total is a 64-bit integer sum
 * (integer atomics), so two runs give identical bits.
 *   ws: rgda_strong_augment_workspace(N) bytes (128 per image), 8-byte aligned; rewritten BY the call, any contents on entry.
 * Three launches whatever the table holds: each image's constants into ws (switches, radius, M and the taps, built once
 * per image by one thread, and its cleared sum); the grey sums (workgroups of images without bit 0 leave at once); the
 * transform (a 32 x 32 tile per workgroup, tile + halo of the three channels in LDS, both blur passes there).
 * 16-byte stores where W % 4 == 0 and img_out is 16-byte aligned (the copy also needs img_in aligned), element stores otherwise.
 * Errors before any launch (RGDA_ERR_ARG): null img_in / img_out / ws; null or misaligned table; misaligned ws; N, H or
 * W < 1; a std that is not positive; overlapping img_in and img_out.  N > 65535 or H * W >= 2^31: RGDA_ERR_UNSUPPORTED. */
#define RGDA_STRONG_TABLE_COLS 8
#define RGDA_STRONG_MAX_RADIUS 12
size_t rgda_strong_augment_workspace(int N);
int rgda_strong_augment(const float* img_in, float* img_out, const float* table, void* ws, int N, int H, int W,
                        float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b, int* flag,
                        rgda_stream_t stream);

/* The host's table -> device, carried IN THE KERNEL ARGUMENTS of one launch, as rgda_mix_write_table carries its draw:
 * nothing is staged in host memory, so the call can be a host action of a recorded plan.
 *   table f32 [N][RGDA_STRONG_TABLE_COLS] on the device, 16-byte aligned <- host, N * 8 floats of HOST memory read during
 *     the call; columns 6 and 7 are written as 0.
 *   H, W: the tiles the table is for (the blur radius is checked against them).
 * RGDA_ERR_ARG: null table / host; misaligned table; N, H or W < 1; a value of fb, fc, fs, theta or sigma that is not
 * finite; fb, fc or fs below 0; flags not one of 0, 1, 2, 3.  RGDA_ERR_UNSUPPORTED: N above RGDA_MIX_WRITE_MAX_IMAGES; a
 * row with bit 1 whose sigma is outside (0, 4] or whose radius R is not below both H and W. */
int rgda_strong_write_table(float* table, const float* host, int N, int H, int W, rgda_stream_t stream);

/* ------------------------------------------------------------- Fourier style transfer of the source tile */

/* Fourier Domain Adaptation (Yang and Soatto, CVPR 2020) of normalised source tiles, image by image from a device table:
 * the low-frequency amplitude spectrum of a source image is replaced with that of a target image, the source's phase is
 * kept.  The reference has no such pass; the semantics are this library's and tests/fourier_ref.py restates them in fp64
 * through a full FFT.
 *   img_s f32 [N][3][H][W], img_t f32 [M][3][H][W] (read only), out f32 [N][3][H][W], every pixel written, OUT OF PLACE.
 *   table int32 [N][RGDA_STYLE_TABLE_COLS], 16-byte aligned, DEVICE memory: row n = {partner in [0, M), b, on, 0}.
 *   mean_s*, std_s*, mean_t*, std_t* (r, g, b): the normalisations the source and the target tiles carry; std > 0.
 * Per channel, on the raw grey scale: S = x_s std_s + mean_s, T = x_t std_t + mean_t of the row's partner.
 *   1. F_S = DFT2(S), F_T = DFT2(T).
 *   2. On every frequency pair (ky, kx) with |ky| <= b and |kx| <= b (signed frequencies, DC at (0, 0): the published
 *      window [c - b, c + b] around c = floor(size / 2) of the fft-shifted spectrum, for even and odd sizes alike) the
 *      amplitude |F_S| is replaced by |F_T| and the source's phase is kept; where |F_S(k)| is exactly 0 the phase is 0.
 *   3. The real part of the inverse transform, normalised as the source is: out = (. - mean_s) / std_s.  No clamp.
 * b = 0 swaps the channel mean; T == S with equal normalisations returns S up to rounding.  A row with on == 0 is COPIED
 * bit for bit (no arithmetic touches it; NaN and inf pass through).  b comes from the host (b = floor(min(H, W) beta)).
 * No full FFT: only (2b + 1)^2 bins change, so out_raw = S + (1 / HW) Re sum_k D(k) e^{+2 pi i (ky y / H + kx x / W)} with
 * D(k) = (|F_T(k)| - |F_S(k)|) F_S(k) / |F_S(k)|, a pruned separable DFT (kx in [0, b] suffices: the images are real).
 * Six launches whatever the table holds: the rows as served and the twiddle tables e^{2 pi i p / W}, e^{2 pi i p / H}
 * (p = (k x) mod size reduced in integers, sincospi in fp64, rounded once); the row transform of the source and the
 * needed target images; the column transform; D; the column synthesis; the row synthesis, which reads the source tile
 * once, adds the correction and writes the normalised output (or copies an off row).  fp32 arithmetic, every sum in a
 * fixed order (a fixed sequence per lane, then a fixed tree): no atomics, two runs give identical bits.
 * Served: b <= RGDA_STYLE_MAX_B, 2 b + 1 <= min(H, W), N and M in 1..RGDA_STYLE_MAX_IMAGES, H, W <= 4096.
 * rgda_fourier_style_write_table refuses rows outside that.  The rows are read on the device and cannot be refused here:
 * a row with a partner outside [0, M), b < 0, a b that does not fit, or on outside {0, 1} is copied unchanged and sets
 * *flag (optional, device int) to 1.
 *   ws: rgda_fourier_style_workspace(N, M, H, W) bytes (0 for a shape that is not served), sized for the largest b the
 *     tile admits, 16-byte aligned; rewritten BY the call, any contents on entry.
 * Errors before any launch (RGDA_ERR_ARG): null img_s / img_t / out / ws; null or misaligned table; misaligned ws; N, M,
 * H or W < 1; a std that is not positive and finite, a mean that is not finite; out overlapping img_s or img_t.  N or M
 * above RGDA_STYLE_MAX_IMAGES, H or W above 4096: RGDA_ERR_UNSUPPORTED. */
#define RGDA_STYLE_TABLE_COLS 4
#define RGDA_STYLE_MAX_B 64
#define RGDA_STYLE_MAX_IMAGES 16
size_t rgda_fourier_style_workspace(int N, int M, int H, int W);
int rgda_fourier_style(const float* img_s, const float* img_t, float* out, const int32_t* table, void* ws, int N, int M,
                       int H, int W, float mean_sr, float mean_sg, float mean_sb, float std_sr, float std_sg, float std_sb,
                       float mean_tr, float mean_tg, float mean_tb, float std_tr, float std_tg, float std_tb, int* flag,
                       rgda_stream_t stream);

/* The host's table -> device, carried IN THE KERNEL ARGUMENTS of one launch, as rgda_strong_write_table carries its draw.
 *   table int32 [N][RGDA_STYLE_TABLE_COLS] on the device, 16-byte aligned <- host, N * 4 int32 of HOST memory read during
 *     the call; column 3 is written as 0.
 *   M: the target images the partners index; H, W: the tiles the table is for.
 * RGDA_ERR_ARG: null table / host; misaligned table; N, M, H or W < 1; a partner outside [0, M); b < 0; on not 0 or 1.
 * RGDA_ERR_UNSUPPORTED: N or M above RGDA_STYLE_MAX_IMAGES; b above RGDA_STYLE_MAX_B; 2 b + 1 > min(H, W).  (b is checked
 * on rows that are switched off too: the table says what was drawn.) */
int rgda_fourier_style_write_table(int32_t* table, const int32_t* host, int N, int M, int H, int W, rgda_stream_t stream);

/* ------------------------------------------------------------- histogram matching of the source tile */

/* Per-channel histogram matching of normalised source tiles to a target tile, image by image from a device table: the
 * grey-level distribution of a source plane is mapped onto that of its partner's plane (scikit-image's
 * exposure.match_histograms, albumentations' HistogramMatching with its blend_ratio).  The reference has no such pass;
 * the semantics are this library's and tests/hist_ref.py restates them in numpy and Python integers.
 *   img_s f32 [N][3][H][W], img_t f32 [M][3][H][W] (read only), out f32 [N][3][H][W], every pixel written, OUT OF PLACE.
 *   table int32 [N][RGDA_STYLE_TABLE_COLS], 16-byte aligned, DEVICE memory: row n = {partner in [0, M), blend_q in
 *     [0, RGDA_HIST_BLEND_ONE], on, 0}.  The blend is beta = blend_q / 65536, exact.
 *   mean_s*, std_s*, mean_t*, std_t* (r, g, b): the normalisations the source and the target tiles carry; std > 0.
 * Source and target tiles have one size, so both histograms of a pair sum to HW.
 * Per source image n with on == 1, partner p, per channel c:
 *   1. Grey levels: v(x) = clamp(rintf(fmaf(x, std, mean)), 0, 255), the source's normalisation for img_s, the target's
 *      for img_t (a NaN counts as level 0).
 *   2. hs[256] of the source plane and ht[256] of the partner's plane: exact integer histograms; cs, ct their inclusive
 *      prefix sums; u_0 < ... < u_{k-1} the levels with ht > 0.
 *   3. The matched level of each v with hs[v] > 0: let j be the largest index with ct[u_j] <= cs[v].
 *        no such j:  L[v] = u_0
 *        j == k - 1: L[v] = u_{k-1}
 *        otherwise:  L[v] = u_j + ((cs[v] - ct[u_j]) * (u_{j+1} - u_j)) / (ct[u_{j+1}] - ct[u_j]), numerator and
 *                    denominator formed in integers (below 2^32 at H, W <= 4096), both converted to fp64, ONE fp64
 *                    division, then ONE fp64 addition.
 *      L[v] = v where hs[v] == 0 (never read).  This is np.interp(cs / HW, ct / HW, u) with the comparisons made exact;
 *      an image matched to itself gives L[v] == v exactly.
 *   4. D[v] = (float)(beta * (L[v] - v) / (double)std_s[c]): fp64, rounded to fp32 once.
 *   5. out = x + D[v(x)], one fp32 addition, no clamp (on the grey scale the result lies in [-0.5, 255.5]); the sub-level
 *      part of the source pixel survives.  beta == 0, and a partner identical to the source under equal normalisations,
 *      give D == 0: the source comes back (x + 0.0f: a -0.0 pixel becomes +0.0, every other value keeps its bits).
 * A row with on == 0 is COPIED bit for bit (no arithmetic touches it; NaN and inf pass through).  The rows are read on the
 * device and cannot be refused here: a row with a partner outside [0, M), blend_q outside [0, RGDA_HIST_BLEND_ONE] or on
 * outside {0, 1} is copied unchanged and sets *flag (optional, device int) to 1.
 * Four launches whatever the table holds, no host synchronisation, no runtime memset: the rows as served and the zeroed
 * counters; the histograms of all N + M images (per-wave LDS bins, integer LDS atomics, then integer global atomics of
 * the nonzero bins); L and D, one workgroup per (source image, channel); the apply pass, which reads the source tile once.
 * Integer sums only: two runs give identical bits.
 * Served: N and M in 1..RGDA_STYLE_MAX_IMAGES, H, W in 1..4096.
 *   ws: rgda_hist_style_workspace(N, M, H, W) bytes (0 for a shape that is not served), 16-byte aligned; rewritten BY the
 *     call, any contents on entry.
 *   hist (optional) uint32 [N + M][3][256], 4-byte aligned: the histograms, the source images first.
 *   lut (optional) f64 [N][3][256], 8-byte aligned: L; the identity (L[v] = v) for a row that is off or not served.
 * Errors before any launch (RGDA_ERR_ARG): null img_s / img_t / out / ws; null or misaligned table; misaligned ws, hist
 * or lut; N, M, H or W < 1; a std that is not positive and finite, a mean that is not finite; out overlapping img_s or
 * img_t.  N or M above RGDA_STYLE_MAX_IMAGES, H or W above 4096: RGDA_ERR_UNSUPPORTED. */
#define RGDA_HIST_BLEND_ONE 65536
size_t rgda_hist_style_workspace(int N, int M, int H, int W);
int rgda_hist_style(const float* img_s, const float* img_t, float* out, const int32_t* table, void* ws, int N, int M, int H,
                    int W, float mean_sr, float mean_sg, float mean_sb, float std_sr, float std_sg, float std_sb,
                    float mean_tr, float mean_tg, float mean_tb, float std_tr, float std_tg, float std_tb, uint32_t* hist,
                    double* lut, int* flag, rgda_stream_t stream);

/* The host's table -> device, carried IN THE KERNEL ARGUMENTS of one launch, as rgda_fourier_style_write_table carries its
 * draw.
 *   table int32 [N][RGDA_STYLE_TABLE_COLS] on the device, 16-byte aligned <- host, N * 4 int32 of HOST memory read during
 *     the call; column 3 is written as 0.
 *   M: the target images the partners index; H, W: the tiles the table is for.
 * RGDA_ERR_ARG: null table / host; misaligned table; N, M, H or W < 1; a partner outside [0, M); blend_q outside
 * [0, RGDA_HIST_BLEND_ONE]; on not 0 or 1 (rows that are off are checked too: the table says what was drawn).
 * RGDA_ERR_UNSUPPORTED: N or M above RGDA_STYLE_MAX_IMAGES. */
int rgda_hist_style_write_table(int32_t* table, const int32_t* host, int N, int M, int H, int W, rgda_stream_t stream);

/* ------------------------------------------------------------- region maps without SAM */

/* The region maps rgda_lrh and rgda_label_refine_sup read, generated from the raw tile.
 * NOT pinned: the superpixel algorithm.  The reference gets its superpixels from cv2.ximgproc.createSuperpixelLSC
 * (regda/gast/superpixels.py:49-83) and skimage.segmentation.slic (regda/gast/slic/superpixel.py:66-90), both third
 * party.  rgda_superpixels stands in for them and reproduces neither: it is this library's own integer SLIC, specified
 * here, restated in numpy in tests/superpixel_ref.py and bit-exact against that restatement.
 *   img uint8 [N][H][W][3] (HWC, the raw tile rgda_augment_tiles takes; 4-byte aligned); region size 4 <= S <= 64 with
 *   H % S == 0, W % S == 0, H, W <= 16384; compactness 1 <= m <= 64; iters >= 1; min_area >= 1; N <= 65535.
 *   Cell k = gy * (W / S) + gx owns one centre (cy, cx, cr, cg, cb), all int32.
 *   Update(labels): per centre the int32 sums of (y, x, r, g, b) and the count n of its pixels; each component becomes
 *     (2 * sum + n) / (2 * n) (integer division: round half up); a centre with n == 0 keeps its value.
 *   Initial centres: Update of the grid labelling (every pixel labelled with its own cell).
 *   Assign(centres): a pixel of cell (gy, gx) takes, among the existing cells (gy + a, gx + b), a, b in {-1, 0, 1}, the
 *     centre of least d = ((r-cr)^2 + (g-cg)^2 + (b-cb)^2) * S^2 + m^2 * ((y-cy)^2 + (x-cx)^2); equal d: the smaller k.
 *     d < 2^31 within the limits above (a centre stays inside the 3 x 3 cells around its own, so |y - cy| < 3 S).
 *   for it = 1..iters: labels = Assign(centres); if it < iters: centres = Update(labels).
 *   Components: the 4-connected components of equal labels inside one image; a component's root is its smallest
 *     pixel index y * W + x; components of fewer than min_area pixels become region 0 ("no region", which LRH leaves
 *     as it is: local_region_homog.py:149) -- they are NOT merged into a neighbour; the others are numbered 1..R in
 *     increasing root order.
 *   regs_out int32 [N][H][W]; count_out int32 [N] = R per image.  R <= H * W / min_area.
 * ws: rgda_superpixels_workspace bytes (0 for a shape that is not served), 16-byte aligned, cleared inside the call where
 * it has to be.  It begins with int32 centres[2][N][cells][5]; copy (iters & 1) holds the centres of the last Assign.
 * 2 + iters + 7 launches, no host synchronisation.  Errors before any launch: null pointer, N / H / W < 1, H % S or
 * W % S != 0, iters < 1, min_area < 1, misalignment (RGDA_ERR_ARG); S, m, H, W or N outside the limits
 * (RGDA_ERR_UNSUPPORTED); a short workspace (RGDA_ERR_WORKSPACE). */
size_t rgda_superpixels_workspace(int N, int H, int W, int S);
int rgda_superpixels(const uint8_t* img, int N, int H, int W, int S, int m, int iters, int min_area, int32_t* regs_out,
                     int32_t* count_out, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* edge_shrinking(label_supixl, win_size)   regda/gast/superpixels.py:129-152.  PINNED: the reference's own loop,
 * bit-exact against a golden minted from it (tests/golden/edge_shrink.npz).
 * regs, out: int32 [N][H][W] (not the same buffer).  out = regs where every pixel of the (2 * win + 1)^2 window that lies
 * inside the image holds the same id, `fill` elsewhere.  The reference calls it with win = 3 and
 * fill = int(h / region_size * w / region_size); fill = 0 ("no region") is the useful value in front of LRH.
 * 0 <= win <= 8 (beyond: RGDA_ERR_UNSUPPORTED).  One launch. */
int rgda_region_shrink(const int32_t* regs, int N, int H, int W, int win, int fill, int32_t* out, rgda_stream_t stream);

/* ------------------------------------------------------------- evaluation path */

/* cls.argmax(dim=1) of the (N,C,H,W) probabilities (regda/utils/eval.py:43): int64 (N,H,W), first maximum wins. */
int rgda_argmax_nchw(const float* probs, int64_t* out, int N, int C, int64_t HW, rgda_stream_t stream);
/* Confusion matrix of the pixels with y_true >= 0 (eval.py:45-50; what ever's PixelMetric.forward accumulates):
 * cm int64 [C][C] (row = true class, column = prediction) += counts.  flag |= 1 if a label >= C or a prediction
 * outside [0,C) was seen (those pixels are not counted).  C <= 64. */
int rgda_confusion_accumulate(const int64_t* y_true, const int64_t* y_pred, int64_t* cm, int* flag, int64_t n,
                              int C, rgda_stream_t stream);

/* ------------------------------------------------------------- stage 2, "align"  */

/* PrototypeContrastiveLoss (regda/loss.py:10-47), forward + gradient w.r.t. the features in one pass:
 *   feat f32 NCHW (b,K,h,w); labels int64 (b,h,w), `ignore_label` pixels are removed; protos f32 (C,K), 6 <= C <= 16;
 *   the normalised prototypes sit in LDS: C * K floats plus the partial sums within 160 KB (C = 16: K = 2048 fits, 4096 does
 *   not; beyond it RGDA_ERR_UNSUPPORTED).
 *   logits = normalize(feat_p) . normalize(protos)^T / temperature   (tnf.normalize: x / max(||x||, 1e-12))
 *   loss[0] += weight * mean over the kept pixels of cross_entropy(logits, label)      (NaN if none is kept, and NaN
 *   if any kept pixel's loss is not finite -- a NaN or Inf feature -- however many such pixels there are)
 *   dfeat (optional) bf16 [b*h*w][lddf], pixel-major -- the layout rgda_instnorm_bwd consumes: (+)= weight * dloss/dfeat
 * ws (rgda_pcl_loss_workspace bytes): float pn[C][K] normalised prototypes, padded to 256 bytes | int valid-pixel count |
 *   int flag | rgda_stat_t loss total.  The call clears count, flag and total first.  flag bit 2 (value 4): a label
 *   outside [0,C) that is not ignore_label (such a pixel is dropped like an ignored one); bit 3 (value 8): the loss of a
 *   32-pixel block was not finite or left the fixed-point range (|partial| >= 2^19), and loss[0] is NaN. */
size_t rgda_pcl_loss_workspace(int C, int K);
int rgda_pcl_loss(const float* feat, const int64_t* labels, const float* protos, float* loss, void* dfeat,
                  int lddf, int accumulate, int b, int K, int C, int h, int w, int ignore_label,
                  float temperature, float weight, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* CoralLoss (regda/gast/coral.py, is_sqrt=False) of Aligner.align_domain (regda/gast/alignment.py:79-84), forward +
 * gradient w.r.t. both feature maps in one call (stage 1 and stage 2 with --align-domain 1):
 *   feat_s f32 (bs, d, hws): element (image b, channel c, pixel p) at feat_s[b * ldbs + c * ldcs + p] (NCHW: ldcs = h*w,
 *   ldbs = d*h*w); its ns = bs * hws pixels are the rows of Xs (n, d).  Same for feat_t (nt rows); ns != nt allowed.
 *   mu = column means of X (fp32, fixed order);  Xc = bf16(X - mu), rounded once
 *   Cs = Xcs^T Xcs / (ns - 1), Ct = Xct^T Xct / (nt - 1)   (bf16 products, fp32 sums; tiles on and above the diagonal)
 *   D = Cs - Ct (fp32);  loss[0] += weight * sum(D * D) / (4 d^2)
 *   dfeat_s (optional) bf16 [ns][ldds], pixel-major -- the layout rgda_instnorm_bwd consumes:
 *            (+)= weight * Xcs . bf16(D) / (d^2 (ns - 1))        (accumulate != 0: added in fp32, rounded once)
 *   dfeat_t (optional) bf16 [nt][lddt]: (+)= -weight * Xct . bf16(D) / (d^2 (nt - 1))
 * (D is symmetric and the centred rows sum to zero, so the mean term of the backward vanishes.)  d % 32 == 0,
 * ns >= 2, nt >= 2, ldd % 8 == 0 (RGDA_ERR_ARG before any launch otherwise).  Deterministic: no atomics, the split-K
 * partials of the covariance product are reduced in a fixed order.  ws: rgda_coral_loss_workspace bytes (0 for
 * arguments the entry point rejects). */
size_t rgda_coral_loss_workspace(int ns, int nt, int d);
int rgda_coral_loss(const float* feat_s, int bs, int hws, int64_t ldcs, int64_t ldbs,
                    const float* feat_t, int bt, int hwt, int64_t ldct, int64_t ldbt, int d, float* loss,
                    void* dfeat_s, int ldds, void* dfeat_t, int lddt, int accumulate, float weight, void* ws,
                    size_t ws_bytes, rgda_stream_t stream);

/* MMDLoss (regda/gast/mmd.py:15-58; the commented `self.mmd = MMDLoss(kernel_type='linear')` of
 * regda/gast/alignment.py:68), forward + gradient w.r.t. both feature maps in one call.  Features are addressed as in
 * rgda_coral_loss (strided NCHW or (n, d) rows, no permuted copy); `total` = the ns source rows followed by the nt target
 * rows (mmd.py:27), n = ns + nt.
 * kernel_type RGDA_MMD_RBF (guassian_kernel, mmd.py:25-38, and the four block means of mmd.py:53-57):
 *   mu = column means of total (fp32, fixed order);  Xc = bf16(total - mu), rounded once (distances do not see the shift;
 *   centring first keeps r_i + r_j - 2 g accurate on post-ReLU features);  r_i = sum of squares of the rounded row (fp32)
 *   bw = fix_sigma when fix_sigma > 0, else the mean pairwise squared distance sum(l2) / (n^2 - n) of mmd.py:34 in closed
 *        form, (2 n sum_i r_i - 2 |sum_i Xc_i|^2) / (n^2 - n);  bw /= kernel_mul^(kernel_num / 2);  bw_q = bw kernel_mul^q,
 *        q < kernel_num.  Computed on the device (no read-back); a constant of the backward, as in the reference (`.data`).
 *   per upper 128 x 128 tile of the n x n matrix: g = Xc Xc^T (bf16 products, fp32 sums),
 *        l2_ij = max(r_i + r_j - 2 g_ij, 0), exactly 0 for i = j;  kappa_ij = sum_q exp(-l2_ij / bw_q)
 *        s_ij = a_i a_j with a = 1 / ns for a source row, -1 / nt for a target row
 *        L = sum_ij s_ij kappa_ij (tiles off the diagonal count twice; tile partials reduced in a fixed order)
 *        W_ij = bf16(s_ij sum_q exp(-l2_ij / bw_q) / bw_q), W_ii = 0, stored to both triangles;  rho_i = sum_j W_ij (fp32, of
 *        the rounded values, per-tile partial row sums reduced in a fixed order)
 *   loss[0] += weight * L
 *   dfeat_s (optional) bf16 [ns][ldds], pixel-major -- the layout rgda_instnorm_bwd consumes: row i
 *        (+)= -4 weight (rho_i Xc_i - sum_j W_ij Xc_j)            (accumulate != 0: added in fp32, rounded once)
 *   dfeat_t (optional) bf16 [nt][lddt]: the same for rows ns .. n of total.
 * kernel_type RGDA_MMD_LINEAR (forward_linear, mmd.py:41-44): loss[0] += weight * |mean_s - mean_t|^2 / d; source rows
 *   (+)= 2 weight (mean_s - mean_t) / (d ns), target rows (+)= -2 weight (mean_s - mean_t) / (d nt).
 * Before any launch: null feat / loss / ws, ws not 256-byte aligned, d % 32 != 0, ns < 2, nt < 2, kernel_num < 1,
 * kernel_mul <= 0, an unknown kernel_type, ldd % 8 != 0 or ldd < d: RGDA_ERR_ARG; kernel_num > 8 or n > 32768:
 * RGDA_ERR_UNSUPPORTED; a short workspace: RGDA_ERR_WORKSPACE.  Deterministic: no atomics.
 * ws: rgda_mmd_loss_workspace(ns, nt, d) bytes (0 for arguments the entry point rejects) =
 *   a(12 d) + 2 a(2 NP d) + 2 a(4 NP) + a(4 d) + 256 + a(4 T NP) + a(4 U) + a(2 NP^2),
 *   NP = 128 * ceil(n / 128), T = NP / 128, U = T (T + 1) / 2, a(x) = x rounded up to a multiple of 256
 * (the last term is W: 512 MB at n = 16384, 2 GB at the limit).  RGDA_MMD_LINEAR uses the means only and accepts a
 * workspace of the first term, a(12 d) bytes. */
#define RGDA_MMD_RBF 0
#define RGDA_MMD_LINEAR 1
size_t rgda_mmd_loss_workspace(int ns, int nt, int d);
int rgda_mmd_loss(const float* feat_s, int bs, int hws, int64_t ldcs, int64_t ldbs,
                  const float* feat_t, int bt, int hwt, int64_t ldct, int64_t ldbt, int d, int kernel_type,
                  float kernel_mul, int kernel_num, float fix_sigma, float* loss, void* dfeat_s, int ldds,
                  void* dfeat_t, int lddt, int accumulate, float weight, void* ws, size_t ws_bytes,
                  rgda_stream_t stream);

/* ClassWareWhitening(class_ids = range(C), groups) (regda/gast/class_ware_whiten.py:14-65) of
 * Aligner.whiten_class_ware (regda/gast/alignment.py:165-170), forward + gradient w.r.t. the feature map in one call:
 *   feat f32 (b, k, hw): element (image i, channel c, pixel p) at feat[i * ldb + c * ldc + p] (NCHW: ldc = h*w,
 *   ldb = k*h*w); labels int64 (b, hw), already at feature resolution; `ignore_label` pixels belong to no class.
 *   s = k / groups.  For every class c < C with n_c >= 2 pixels and every group g of s consecutive channels:
 *     mu = mean of the class's rows (fp32, fixed order);  Xc = bf16(X - mu), rounded once
 *     S = Xc^T Xc / (n_c - 1)   (bf16 products, fp32 sums);  D = S - I (fp32);  term = sum(D * D) / s^2
 *   a class with n_c <= 1 contributes 0 (the reference substitutes the identity).  loss[0] += weight * sum of the terms
 *   dfeat (optional) bf16 [b*hw][lddf], pixel-major -- the layout rgda_instnorm_bwd consumes: the g block of the row
 *     of a pixel of class c  (+)= 4 weight / (s^2 (n_c - 1)) * Xc[pixel][g block] . bf16(D_cg)
 *     accumulate != 0: added in fp32, rounded once; the rows of ignored pixels and of classes with n_c <= 1 are left.
 *     accumulate == 0: every row is written, those rows as zeros.
 * (D is symmetric and the centred rows sum to zero, so the mean term of the backward vanishes.)
 * 6 <= C <= 16 (a runtime value) and s in {32, 64, 96, 128}: RGDA_ERR_UNSUPPORTED otherwise.  Null pointers,
 * k % groups != 0, lddf % 8 != 0 or lddf < k, dfeat not 16-byte aligned, ws not 256-byte aligned, b * hw > 2^24:
 * RGDA_ERR_ARG.  Every check comes before any launch.  Deterministic: no floating-point atomics; the pixels are
 * sorted by class in image order and every sum over them (means, the four row shares of a covariance block) is
 * reduced in a fixed order.  The sort is one workgroup, serial in b * hw: meant for feature maps of some 10^4 pixels.
 * ws: rgda_whiten_loss_workspace(n = b * hw, k, C, groups) bytes (0 for arguments the entry point rejects) =
 *   256 + a(4 NP) + a(4 NP / 64) + a(4 C k) + 2 a(2 k NP) + a(2 C k s) + a(4 C groups),
 *   NP = 64 * ceil(n / 64) + 64 * C,  a(x) = x rounded up to a multiple of 256.
 * Its first int32 is a flag: bit 2 is set when a label outside [0, C) that is not ignore_label was seen (such a pixel
 * is treated as ignored); the next 16 are the per-class pixel counts. */
size_t rgda_whiten_loss_workspace(int n, int k, int C, int groups);
int rgda_whiten_loss(const float* feat, int b, int hw, int64_t ldc, int64_t ldb, const int64_t* labels, int k,
                     int C, int groups, int ignore_label, float* loss, void* dfeat, int lddf, int accumulate,
                     float weight, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* PixelContrastLoss (regda/gast/contrastive.py:27-162: the pixel-wise supervised contrast of Wang et al., ICCV 2021,
 * with hard-anchor sampling) in two entry points.  The host takes the reference's random draws between them
 * (regda_amd/gast/contrastive.py::plan_anchors); the device does the rest.
 *
 * rgda_pixel_contrast_select: labels int64 (b, H, W) are read at (y * H / h, x * W / w) -- what
 *   interpolate(mode='nearest') reads for integer ratios; H % h != 0 or W % w != 0: RGDA_ERR_UNSUPPORTED.
 *   predict: RGDA_PREDICT_LABELS int64 (b, h, w), or RGDA_PREDICT_LOGITS f32 (b, C, h, w) whose argmax is taken (the
 *   lowest index on ties).  A pixel with 0 <= label < C has key 2 * label + easy, easy = (predict == label); an ignored
 *   pixel and one with a label outside [0, C) have key 2 C (the latter also sets bit 2 of flag[0]).
 *   counts int32 [b][C][2]: the pixels per (class, hard / easy);  order int32 [b][h * w]: per image the pixel indices
 *   stably sorted by key, so each of the 2 C lists is in ascending pixel order and the ignored pixels come last.
 *   One workgroup per image, no atomics that could change the output.  2 <= C <= 16 and h * w <= 16384:
 *   RGDA_ERR_UNSUPPORTED otherwise; null pointers, sizes < 1, an unknown predict_kind: RGDA_ERR_ARG; before any launch.
 *
 * rgda_pixel_contrast_loss: forward + gradient w.r.t. the feature map in one call.  feat f32 (b, k, hw) is addressed as
 *   in rgda_whiten_loss (ldc, ldb, read in place).  anchors int32 [A][3] = (image, class, hard_keep), ranks int32
 *   [A][n_view]: the first hard_keep ranks of an anchor index its hard list (key 2 class of `order`), the rest its easy
 *   list.  Row r = v * A + a (view-major, contrastive.py:114) is view v of anchor a, N = A * n_view.
 *     X = bf16(feat rows), rounded once;  dot_rq = sum_c X_rc X_qc (bf16 products, fp32 sums, by upper 128 x 128 tiles;
 *     K is split into up to 8 runs of whole 32-channel groups whose partials are added in order)
 *     G_rq = dot_rq / temperature (fp32 division), stored symmetric;  m_r = max_q G_rq over all N columns
 *     l_rq = G_rq - m_r;  neg_r = sum over q of another class of exp(l_rq)
 *     for q of the same class, q != r:  d_rq = exp(l_rq) + neg_r + eps;  lp_rq = l_rq - log(d_rq)
 *     L = -(temperature / base_temperature) / N * sum_r [ sum_q lp_rq / (P_r + eps) ],  P_r = the number of such q
 *     (every row sum: 64 lane-strided fp32 partials, then a butterfly; the sum over r: 256 strided partials, a
 *     butterfly per wavefront, then (w0 + w1) + (w2 + w3));   loss[0] += weight * L
 *     c_r = -(temperature / base_temperature) / (N (P_r + eps));  W_rq = c_r (1 - exp(l_rq) / d_rq) for a positive q,
 *     -c_r exp(l_rq) sum_p 1 / d_rp for a negative q, 0 for q = r (m_r is a constant of the backward, as in the
 *     reference: `.detach()`);  M = bf16(W + W^T), rounded once
 *   dfeat (optional) bf16 [b * hw][lddf], pixel-major -- the layout rgda_instnorm_bwd consumes: the row of the pixel of
 *     r  (+)= weight / temperature * sum_q M_rq X_q  (bf16 products, fp32 sums).
 *     accumulate != 0: added in fp32 to the selected rows only, rounded once; every other row is left.
 *     accumulate == 0: every row is written (its first k columns), the unselected ones as zeros.
 *   The selected rows are distinct (ranks of one list are distinct), so there are no atomics: deterministic.
 * Before any launch: null feat / order / counts / anchors / ranks / loss / ws, ws not 256-byte aligned, k % 32 != 0,
 * temperature or base_temperature <= 0, eps < 0, b * hw > 2^24, dfeat not 16-byte aligned, lddf % 8 != 0 or lddf < k: RGDA_ERR_ARG;
 * N < 1, N > 4096 or C outside 2..16: RGDA_ERR_UNSUPPORTED; a short workspace: RGDA_ERR_WORKSPACE.
 * ws: rgda_pixel_contrast_loss_workspace(N, k) bytes (0 for arguments the entry point rejects) =
 *   2 a(4 NP) + 2 a(2 NP k) + a(20 NP) + a(4 NP^2) + a(65536 U S) + a(2 NP^2),
 *   NP = 128 * ceil(N / 128), T = NP / 128, U = T (T + 1) / 2, g = k / 32, S0 = min(g, clamp(256 / U, 1, 8)),
 *   S = ceil(g / ceil(g / S0)), a(x) = x rounded up to a multiple of 256  (fp32 G: 4 MB at N = 1024). */
#define RGDA_PREDICT_LABELS 0
#define RGDA_PREDICT_LOGITS 1
int rgda_pixel_contrast_select(const int64_t* labels, const void* predict, int predict_kind, int b, int C, int H,
                               int W, int h, int w, int ignore_label, int32_t* counts, int32_t* order, int* flag,
                               rgda_stream_t stream);
size_t rgda_pixel_contrast_loss_workspace(int N, int k);
int rgda_pixel_contrast_loss(const float* feat, int b, int hw, int64_t ldc, int64_t ldb, int k, int C,
                             const int32_t* order, const int32_t* counts, const int32_t* anchors, int A,
                             const int32_t* ranks, int n_view, float temperature, float base_temperature, float eps,
                             float* loss, void* dfeat, int lddf, int accumulate, float weight, void* ws,
                             size_t ws_bytes, rgda_stream_t stream);

/* TripletLoss (regda/gast/triple.py:13-55: batch-hard mining, Hermans et al., arXiv:1703.07737), forward + gradient
 * w.r.t. the feature map in one call.  feat f32 (b, k, hw) is addressed as in rgda_whiten_loss (ldc, ldb, read in place;
 * (n, k) rows: b = n, hw = 1, ldc = 1, ldb = k); row i = image * hw + pixel, n = b * hw; labels int64 [n].
 * Definition: d_ij = sqrt(max(|x_i - x_j|^2, 1e-12));  d_ap(i) = max over j with t_j = t_i (j = i included),
 *   d_an(i) = min over j with t_j != t_i;  L = mean_i max(0, d_ap(i) - d_an(i) + margin).
 *   has_ignore != 0: rows labelled ignore_label are neither anchors nor candidates.  m = the number of anchors that
 *   have a negative; the mean runs over them (with two or more distinct labels among the valid rows that is every valid
 *   row; with fewer, m = 0 and the loss and the gradient are 0 -- decided on the device).
 *   Labels are compared as int32 (their low 32 bits); the value -2^31 is reserved for "no label".
 * Arithmetic:
 *   rows    Xh = bf16(x), rounded once, [NP][k] (NP = n rounded up to 128, the padding zero);  s_i = sum_c Xh_ic^2 (fp32, of
 *           the rounded values: lane-strided partials, then a butterfly)
 *   mining  per 128 x 128 tile of ALL T x T tiles (one wavefront each, the full K in one run): G = Xh Xh^T (bf16 products,
 *           fp32 sums);  d2_ij = (s_i + s_j) - 2 G_ij;  per anchor the maximum over equal labels and the minimum over
 *           unequal labels with their indices, ties to the lowest index.  G and d2 stay in registers; per (tile row,
 *           anchor) one (value, index) pair of each kind goes to memory, combined with the same tie rule (the rule makes
 *           the combination independent of its order).  -> p(i), n(i)
 *   values  |x_i - x_p|^2 and |x_i - x_n|^2 again for the selected pairs only, as direct fp32 sums of squared differences
 *           of the UNROUNDED rows (64 lane-strided partials, then a butterfly); clamp, sqrt, hinge h_i.  Mining noise can
 *           pick a neighbouring candidate; it cannot perturb the distance of the chosen one.
 *   loss    loss[0] += weight * (sum_i h_i) / m  (256 strided partials, a butterfly per wavefront, (w0 + w1) + (w2 + w3))
 *   dfeat (optional) bf16 [n][lddf], pixel-major -- the layout rgda_instnorm_bwd consumes.  With c = weight / m, for
 *           every anchor i with h_i > 0:  row i += (c / d_ap)(x_i - x_p) - (c / d_an)(x_i - x_n);
 *           row p -= (c / d_ap)(x_i - x_p);  row n += (c / d_an)(x_i - x_n);  a pair whose squared distance is below the
 *           clamp contributes nothing.  Formed in fp32 from the unrounded rows, one workgroup per row r: its own anchor's
 *           two terms first, then the anchors i != r that selected r in ascending i (found by scanning the p / n tables;
 *           no floating-point atomics), rounded once.
 *           accumulate != 0: added in fp32 to the rows that receive something, rounded once; every other row is left.
 *           accumulate == 0: every row is written (its first k columns), the untouched ones as zeros.
 *   Two calls on the same inputs are bit-identical.
 * Before any launch: null feat / labels / loss / ws, ws not 256-byte aligned, k < 32 or k % 32 != 0, margin < 0 (or
 * NaN), n < 2, ldc < hw, ldb < ldc * k, dfeat not 16-byte aligned, lddf % 8 != 0 or lddf < k: RGDA_ERR_ARG; n > 16384:
 * RGDA_ERR_UNSUPPORTED; a short workspace: RGDA_ERR_WORKSPACE.
 * ws: rgda_triplet_loss_workspace(n, k) bytes (0 for arguments the entry point rejects) =
 *   256 + 9 a(4 NP) + a(16 T NP) + a(2 NP k) + a(4 NP k),   NP = 128 * ceil(n / 128), T = NP / 128,
 *   a(x) = x rounded up to a multiple of 256  (the last term is the pixel-major f32 copy of the rows that the selected
 *   distances and the gradient read: 128 MB at n = 16384, k = 2048).  Layout, in this order: the stats block (256 bytes:
 *   int32 m, int32 number of positive hinges), then nine [NP] tables -- int32 staged labels, f32 s, int32 p, int32 n,
 *   int32 p and n again with -1 where the pair carries no gradient, f32 d_ap and d_an (0 where it carries none), f32
 *   hinge --, the mining partials, Xh, the f32 rows. */
size_t rgda_triplet_loss_workspace(int n, int k);
int rgda_triplet_loss(const float* feat, int b, int hw, int64_t ldc, int64_t ldb, const int64_t* labels, int k,
                      float margin, int has_ignore, int ignore_label, float* loss, void* dfeat, int lddf,
                      int accumulate, float weight, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* Deep Covariance Alignment (regda/dca_modules.py:20-188: CategoryAlign_Module.get_context :20-34,
 * get_cross_corcoef_mat :47-57, regularize :59-76; ICR :79-105, CCR :108-133, MSE_intra :136-159, MSE_cross :162-188),
 * forward + gradient w.r.t. the feature map in one call.  A side is b images: feat f32 (b, c, hw) addressed as in
 * rgda_whiten_loss (ldc, ldb, read in place, once) and one or two prediction planes f32 (b, C, hw), contiguous.
 * Definition, per side:
 *   P (b, C, hw)  pred_kind 0: pred1 as given (probabilities);  1: softmax(pred1) over the classes;
 *                 2: (softmax(pred1) + softmax(pred2)) / 2.  P is a constant: no gradient reaches the predictions.
 *   Z[b][k] = sum_p P[b][k][p];   v[b][k][:] = sum_p feat[b][:][p] P[b][k][p] / Z[b][k]                     (:26-29)
 *   ignore_bg != 0: class 0 is dropped, n = C - 1; else n = C                                                (:31-32)
 *   u[b][k][ch] = v[b][k][ch] / max(sqrt(sum_k' v[b][k'][ch]^2), 1e-12) -- F.normalize(dim=1) runs over the CLASS axis,
 *                 per image and channel                                                                      (:33)
 *   kind 0 (cov): m_a = mean_b u_a, m_b = mean_b u_b (n, c);  R[i][j] = the Pearson coefficient of m_a[i][:] and
 *                 m_b[j][:] over the c channels;  L = -mean_i log R[i][i] - mean_{i != j} log(1 - max(R[i][j], 1e-6)).
 *                 An off-diagonal entry at or below 1e-6 carries no gradient; a non-positive diagonal entry gives a NaN
 *                 (or infinite) loss as in the reference: nothing is clamped here.
 *   kind 1 (mse): L = mean over (b, n, c) of (u_a - u_b)^2;  b_a == b_b.
 *   CCR / MSE_cross: side a = the source without dfeat, side b = the target.  ICR / MSE_intra: the two sides are the
 *   halves [:B / 2] and [B / 2:] of one batch, both with dfeat.
 * Arithmetic (fp32 throughout, from the unrounded f32 features; no bf16 operand):
 *   P       max-subtracted softmax: the hardware exp2 of (l - max) log2(e), the sum over the classes in ascending order,
 *           one hardware reciprocal per pixel and map (each about one unit in the last place); formed per pixel in
 *           registers in both passes and never written to memory
 *   context one workgroup per (image, 64 channels) walks all pixels: wavefront q adds P x feat over the pixels 128 t + 32 q
 *           + i (t ascending, four pixels per fp32 MFMA 16 x 16 x 4, fp32 operands); S = (q0 + q1) + (q2 + q3).  Z: thread
 *           t < 128 adds the pixels t + 128 j, a butterfly per wavefront, (w0 + w1) + (w2 + w3).  v = S / Z, the sum of squares
 *           over the classes in ascending order (fused), sqrt, u = v / max(., 1e-12).
 *   cov     m = (sum_b u in ascending b) / b; centred by its mean over the channels; R = <a_i, b_j> / (sqrt(|a_i|^2)
 *           sqrt(|b_j|^2)); channel sums: 256 strided partials, a butterfly per wavefront, (w0 + w1) + (w2 + w3);
 *           L the same sum over the n * n entries;  loss[0] += weight * L
 *   mse     one partial per 256 channels of an image, summed by one workgroup;  loss[0] += weight * sum / (b n c)
 *   table   dL/dv in closed form (through u, the batch mean, R or the squared difference) divided by Z ->
 *           G[b][k][ch], f32 (b, C, c) in the workspace; the row of a dropped class 0 is zero
 *   dfeat (optional, per side) bf16 [b * hw][lddf], pixel-major -- the layout rgda_instnorm_bwd consumes: row b * hw + p,
 *           channel ch = weight * sum_k P[b][k][p] G[b][k][ch] (k ascending, fused), rounded once.
 *           accumulate != 0: the old bf16 value joins the fp32 one before the one rounding.  A side without dfeat gets no
 *           gradient launch and its rows are not touched.
 *   Two calls on the same inputs are bit-identical (no floating-point atomics).
 * Before any launch: null feat / pred1 / loss / ws (pred2 with pred_kind 2; u for rgda_dca_context), ws not 256-byte
 * aligned, c < 32 or c % 32 != 0, hw < 1, b < 1 on either side, pred_kind outside 0..2, kind outside 0..1, ldc < hw,
 * ldb < ldc * c, a dfeat not 16-byte aligned, lddf % 8 != 0 or lddf < c, mse with b_a != b_b: RGDA_ERR_ARG; C outside
 * 6..16: RGDA_ERR_UNSUPPORTED; a short workspace: RGDA_ERR_WORKSPACE.
 * rgda_dca_context: one side -> u f32 (b, n, c), optionally v f32 (b, n, c) and Z f32 (b, C); ws:
 *   rgda_dca_context_workspace(b, c) = a(4 b c) bytes, the class norms (b, c) before their clamp.
 * rgda_dca_loss ws: rgda_dca_loss_workspace(b_a, b_b, c, C, ignore_bg) bytes (0 for arguments the entry point rejects) =
 *   256 + sum over the sides of [a(4 b n c) + a(4 b c) + a(4 b C) + a(4 b C c)] + 2 a(8 n c) + a(4 (2 n + 2 n^2))
 *   + a(4 ceil(c / 256) max(b_a, b_b)),   a(x) = x rounded up to a multiple of 256.  Layout, in this order: 256 spare
 *   bytes; per side (a, then b) u (b, n, c), the class norms (b, c), Z (b, C), G (b, C, c); the centred means (2, n, c);
 *   dL/dm (2, n, c); the squared norms of the centred means (2, n), R (n, n), dL/dR (n, n); the mse partials. */
size_t rgda_dca_context_workspace(int b, int c);
int rgda_dca_context(const float* feat, int b, int hw, int64_t ldc, int64_t ldb, const float* pred1, const float* pred2,
                     int pred_kind, int c, int C, int ignore_bg, float* u, float* v, float* Z, void* ws, size_t ws_bytes,
                     rgda_stream_t stream);
size_t rgda_dca_loss_workspace(int b_a, int b_b, int c, int C, int ignore_bg);
int rgda_dca_loss(const float* feat_a, int b_a, int64_t ldc_a, int64_t ldb_a, const float* pred1_a, const float* pred2_a,
                  void* dfeat_a, const float* feat_b, int b_b, int64_t ldc_b, int64_t ldb_b, const float* pred1_b,
                  const float* pred2_b, void* dfeat_b, int hw, int c, int C, int pred_kind, int ignore_bg, int kind,
                  float* loss, int lddf, int accumulate, float weight, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* Semantic-aware whitening (regda/gast/SAW.py:54-107: SAW of Peng et al., CVPR 2022), forward + gradient w.r.t. the
 * feature map in one call.  feat f32 (b, k, hw) is addressed as in rgda_whiten_loss (ldc, ldb, read in place);
 * cls_w f32 (n_cls, k) on the device, row r at cls_w + r * ldw: the classifier weight; selected int32 [C] in HOST memory:
 * the rows of cls_w that take part, distinct, each in [0, n_cls).
 * Definition:
 *   A = |cls_w|;  G = k / C (integer division).  For class j the channels are ranked by A[selected[j]] in descending
 *   order; equal values rank by the lower channel index (the reference's torch.sort leaves ties unspecified; this rule is
 *   part of the contract).  Slot (g, j), g < G: ch[g][j] = the channel of rank g, wgh[g][j] = sigmoid(A[selected[j]][ch]).
 *   Ranks >= G fill no slot; a channel fills at most one slot per class; two classes may put one channel into one group.
 *   xt[b][g][j][p] = wgh[g][j] * feat[b][ch[g][j]][p];  cov[b][g] = xt xt^T / (hw - 1) (C x C, no mean centring; the
 *   reference's eps * I lies on the diagonal, which the strict upper triangle never reads)
 *   s[b][g] = sum over j < j' of |cov_jj'|;  nod = C (C - 1) / 2;  `margin` is the caller's (the reference: 0 when
 *   relax_denom == 0, else nod // relax_denom)
 *   L = sum_g sum_b max((s[b][g] - margin) / nod, 0) / b;   loss[0] += weight * L
 *   For a (b, g) with s > margin ("active"):  dL/dxt_j[p] = sum_{j' != j} sign(cov_jj') xt_j'[p] / (b nod (hw - 1)),
 *   sign(0) = 0;  dL/dfeat[b][c][p] = the sum over the slots (g, j) of channel c of wgh[g][j] dL/dxt_j[p].  cls_w
 *   receives no gradient.
 * Arithmetic (fp32 throughout, from the unrounded f32 features; the one bf16 value is the stored gradient):
 *   plan    rank(c) = the number of channels with larger A, or equal A and lower index -- counted, not sorted, on the
 *           device.  wgh: the sigmoid evaluated in double and rounded once.  A non-finite weight sets bit 0 of the flag
 *           word and ranks as +inf; the loss and the gradient of such a call are unspecified, but nothing faults.
 *   gram    one workgroup per (b, g): xt = wgh * x (one rounding); per pair, thread t adds the products of the pixels
 *           t + 256 i in ascending i, a butterfly per wavefront, (w0 + w1) + (w2 + w3); cov = dot / (hw - 1); s adds
 *           |cov| in pair order (j, j') row-major; active = s > margin; partial = (s - margin) / nod
 *   loss    loss[0] += (weight / b) * sum of the partials (256 strided partials, a butterfly per wavefront,
 *           (w0 + w1) + (w2 + w3))
 *   slots   for an active (b, g): wgh_j coef sum_j' sign_jj' xt_j'[p] (j' ascending), coef = weight / (b nod (hw - 1)),
 *           f32 (b, G, C, hw) in the workspace
 *   dfeat (optional) bf16 [b * hw][lddf], pixel-major -- the layout rgda_instnorm_bwd consumes: channel c of row
 *           b * hw + p = the sum of the slot gradients of c in class order (a gather through the inverse table: no
 *           floating-point atomics, no scattered adds), rounded once.
 *           accumulate == 0: every row is written in its first k columns; a channel that fills no slot, or whose groups
 *           are all inactive in that image, as zeros.
 *           accumulate != 0: added in fp32 to the old bf16 value, rounded once; those channels are left untouched.
 *   Two calls on the same inputs are bit-identical.
 * Served: C in {2, 4, 6, 8, 16} (the reference asserts it), C <= k <= 4096, hw >= 2 (the division by hw - 1),
 * b * hw <= 2^24 (and b * G < 2^31): RGDA_ERR_UNSUPPORTED otherwise.  Before any launch: null feat / cls_w / selected /
 * loss / ws, b, k or n_cls < 1, ldw < k, a negative or NaN margin, a selected entry outside [0, n_cls) or repeated,
 * ldc < hw, ldb < ldc * k, dfeat not 16-byte aligned, lddf % 8 != 0 or lddf < k, ws not 256-byte aligned: RGDA_ERR_ARG;
 * a short workspace: RGDA_ERR_WORKSPACE.
 * ws: rgda_saw_loss_workspace(b, hw, k, C) bytes (0 for arguments the entry point rejects) =
 *   256 + a(TS b G) + 2 a(4 b G) + 2 a(4 G C) + a(4 k C) + a(4 b G C hw),   TS = 4 * ceil((nod + 1) / 4),
 *   a(x) = x rounded up to a multiple of 256.  A call without dfeat accepts a workspace without the last term.
 *   Layout, in this order: 256 bytes whose first int32 is the flag word; the per-(b, g) table, TS bytes each: byte 0 the
 *   active bit, bytes 1 .. nod the pair signs as int8 (-1, 0, 1), pairs (j, j'), j < j', row-major; s f32 (b, G); the
 *   partial losses f32 (b, G); ch int32 (G, C); wgh f32 (G, C); the inverse table int32 (k, C): the rank g of the slot
 *   channel c fills for class j, or -1; the slot gradients. */
size_t rgda_saw_loss_workspace(int b, int hw, int k, int C);
int rgda_saw_loss(const float* feat, int b, int hw, int64_t ldc, int64_t ldb, int k,
                  const float* cls_w, int n_cls, int64_t ldw, const int32_t* selected, int C, float margin,
                  float* loss, void* dfeat, int lddf, int accumulate, float weight,
                  void* ws, size_t ws_bytes, rgda_stream_t stream);

/* Transferable Normalization (regda/trans_norm.py:169-230: _TransNorm.forward of Wang et al., NeurIPS 2019; the two
 * F.batch_norm calls, the four reductions over permuted copies, the cat and the Python sum over the channels), forward
 * and backward, training and eval mode.
 * x f32: n samples of C channels of s values; element (i, c, p) at x[i * ldb + c * ldc + p], p < s contiguous (the
 * addressing of rgda_saw_loss; a 2-D (n, C) input is s = 1, ldc = 1, ldb >= C), read in place.  y, g and dx are f32 with
 * strides of their own and must not overlap x.  weight / bias f32 [C], both or neither (NULL: 1 and 0).  rm_s, rv_s,
 * rm_t, rv_t f32 [C]: running mean / variance of the source and target domain, all four or none (NULL: not tracked;
 * training only).  saved f32 [5][C]: mean_s, rstd_s, mean_t, rstd_t, alpha -- written by the forward, read by the backward.
 * Definition, training != 0:  samples [0, n_src) are the source domain (d = s), [n_src, n) the target domain (d = t);
 *   mean_d, varb_d (biased), varu_d (unbiased) over the n_d * s values of channel c in domain d
 *   rstd_d = 1 / sqrt(varb_d + eps);   z = (x - mean_d) * rstd_d * weight + bias
 *   running: r = (1 - momentum) * r + momentum * stat, stat = mean_d for rm_d, varu_d for rv_d (updated in place)
 *   dis = |mean_s / sqrt(varu_s + eps) - mean_t / sqrt(varu_t + eps)|;  prob = 1 / (1 + dis);
 *   alpha = C * prob / sum_c prob;   y = z * (1 + alpha)
 *   backward (alpha is a constant), a = 1 + alpha, gh = g * a * weight, xhat = (x - mean_d) * rstd_d:
 *   dx = rstd_d * (gh - mean_d(gh) - xhat * mean_d(gh * xhat));  dweight = sum of g * a * xhat;  dbias = sum of g * a
 * training == 0:  mean = rm_t, rstd = 1 / sqrt(rv_t + eps) for every sample (n_src is not read); alpha from the four
 *   running vectors by the formulae above; nothing is updated; saved holds (rm_s, 1 / sqrt(rv_s + eps), rm_t,
 *   1 / sqrt(rv_t + eps), alpha);  dx = g * a * weight * rstd_t, dweight and dbias as above with the target's xhat.
 * Arithmetic:
 *   stats    a thread keeps shifted sums about the first value x0 it reads, sum (x - x0) and sum (x - x0)^2 in fp32, and
 *            turns them into a record (count, mean, M2) in double; the records of a wavefront (a tree: lanes (l, l + 32),
 *            then 16, 8, 4, 2, 1), of the four wavefronts ((w0, w1), (w2, w3)) and of the K workgroups of a (channel,
 *            domain) (ascending) are merged by Chan's formula in double.  No sum of squares of the raw values is formed:
 *            |mean| >> std loses nothing.
 *   finalize double: varb = M2 / count, varu = M2 / (count - 1); mean and rstd rounded once to fp32; the running
 *            update evaluated in double from the old fp32 value and rounded once; prob rounded to fp32, sum_c prob in
 *            double over those (one workgroup of 1024: thread t adds the channels t + 1024 i in ascending i, the
 *            wavefront tree, the 16 wavefronts in ascending order), alpha = C * prob / sum rounded once.  Equal halves give dis = 0 and alpha = 1.0 exactly.
 *   apply    double from the fp32 constants of the saved block, each operation rounded once in the order
 *            ((x - mean) * rstd * w + b) * (1 + alpha), never contracted; y is that value rounded once to fp32.
 *   backward sum g and sum g * xhat: fp32 within a thread, the same trees in double; dweight = a * (sum_s + sum_t) and
 *            dbias likewise, rounded once; per domain A = rstd a w, B = A sum(g) / count, D = A sum(g xhat) / count
 *            (double, rounded once to fp32);  dx = (A * g - B) - xhat * D in double from those, rounded once.
 *   Two calls on the same inputs are bit-identical (no floating-point atomics).
 * Launches: training forward 3 (stats, finalize, apply; x read twice), eval forward 2, backward 3 (reduce, finalize,
 *   apply; g and x read twice each; eval without dweight / dbias: the apply alone; dx == NULL: no apply).  Nothing of
 *   the input's size is written in between.  s >= 16: threads run along the planes (16-byte loads where s % 4 == 0 and
 *   every base and stride is 16-byte aligned, 4-byte loads otherwise); s < 16: threads run along the channels.
 * Served: C <= 2^20, n * s <= 2^30; training: 1 <= n_src < n and n_src * s >= 2 and (n - n_src) * s >= 2 (the unbiased
 *   variance of each half): RGDA_ERR_UNSUPPORTED otherwise.  Before any launch: null x / y (g) / saved / ws, n, C or
 *   s < 1, eps negative or NaN, momentum outside [0, 1], one of weight / bias without the other, some but not all of the
 *   running vectors, training == 0 without them, n_src outside [0, n], ldc < s, ldb < ldc * C (of any map), ws not
 *   256-byte aligned: RGDA_ERR_ARG; a short workspace: RGDA_ERR_WORKSPACE.
 * ws: rgda_transnorm_fwd_workspace / _bwd_workspace (n, n_src, C, s, training) bytes, 0 for sizes the entry points do
 *   not serve: the records, double [C][2][K][3] (forward) or double [C][2][K][2] then the coefficients f32 [6][C]
 *   (backward), each rounded up to 256 bytes; K <= 64 is the library's split of a (channel, domain), and the query
 *   returns enough for every alignment of the maps. */
size_t rgda_transnorm_fwd_workspace(int n, int n_src, int C, int s, int training);
int rgda_transnorm_fwd(const float* x, int n, int n_src, int C, int s, int64_t ldc, int64_t ldb, const float* weight,
                       const float* bias, float* rm_s, float* rv_s, float* rm_t, float* rv_t, float eps, float momentum,
                       int training, float* y, int64_t ldc_y, int64_t ldb_y, float* saved, void* ws, size_t ws_bytes,
                       rgda_stream_t stream);
size_t rgda_transnorm_bwd_workspace(int n, int n_src, int C, int s, int training);
int rgda_transnorm_bwd(const float* g, int64_t ldc_g, int64_t ldb_g, const float* x, int n, int n_src, int C, int s,
                       int64_t ldc, int64_t ldb, const float* weight, const float* saved, int training, float* dx,
                       int64_t ldc_dx, int64_t ldb_dx, float* dweight, float* dbias, void* ws, size_t ws_bytes,
                       rgda_stream_t stream);

/* ------------------------------------------------ output-space adversarial alignment (csrc/adv_kernels.hip)
 * FCDiscriminator (regda/models/Discriminator.py:4-28: four Conv2d(4, stride 2, pad 1) + LeakyReLU(0.2) and a
 * one-channel Conv2d of the same geometry) on pixel-major bf16 rows, fed by the softmax of the upsampled logits
 * (AdaptSegNet, Tsai et al. 2018; the upsample is loss_calc's, regda/loss.py: bilinear, align_corners=True).  All
 * activations are DENSE rows (row stride = channel count).  Deterministic: fixed summation orders, no floating-point
 * atomics.  Every check comes before any launch; every row buffer must stay below 2^31 bytes (RGDA_ERR_UNSUPPORTED).
 *
 * rgda_adv_probs_fwd: x f32 (b, C, h, w) -> P bf16 [b*H*W][Cp], Cp = 16 (anything else: RGDA_ERR_UNSUPPORTED), channels
 *   C .. Cp-1 zero.  mode 0: softmax over the classes of the bilinear (align_corners=True) upsample to H x W; mode 1: x
 *   holds probabilities of size H x W (h == H, w == W) and is only packed.  6 <= C <= 16.  P 16-byte aligned.  One launch.
 * rgda_adv_probs_bwd: dx f32 (b, C, h, w) += scale * (the transpose of that map applied to dP bf16 [b*H*W][Cp]).  mode 0:
 *   the softmax backward with the probabilities recomputed from x in f32, then the transpose of the bilinear map in its
 *   gather form: one workgroup per low-resolution pixel, fixed order.  mode 1: x is not read (may be NULL).  One launch.
 *   Replaces F.softmax / F.interpolate and their autograd nodes in front of Discriminator.py:17. */
int rgda_adv_probs_fwd(const float* x, void* P, int b, int C, int h, int w, int H, int W, int Cp, int mode,
                       rgda_stream_t stream);
int rgda_adv_probs_bwd(const void* dP, const float* x, float* dx, int b, int C, int h, int w, int H, int W, int Cp,
                       int mode, float scale, rgda_stream_t stream);

/* One discriminator layer, nn.Conv2d(Cin, Cout, 4, 2, 1) + LeakyReLU(slope) (Discriminator.py:9-12, 18-25), as an implicit
 * GEMM on the bf16 MFMA:  y bf16 [N*(H/2)*(W/2)][Cout] = lrelu(conv(x bf16 [N*H*W][Cin]) + bias),  wgt bf16
 * [Cout][16][Cin] (tap = kh * 4 + kw), bias f32 [Cout] or NULL.  H, W even.  Served: Cin == 16 or Cin % 32 == 0, Cout % 32
 * == 0 (RGDA_ERR_UNSUPPORTED otherwise).  One launch.
 * rgda_disc_conv_bwd_data: the data gradient of that layer as four parity sub-convolutions in ONE launch (the output
 *   pixels of one (row parity, column parity) class read the same 2 x 2 of the 16 taps; no zero tap is multiplied):
 *   dx bf16 [N*H*W][Cin] = mask * sum dy[src][co] * wt[ci][tap][co],  dy bf16 [N*(H/2)*(W/2)][Cout], wt bf16
 *   [Cin][16][Cout] (rgda_weight_transpose_bf16 of the [Cout][16][Cin] f32 weights), mask = below > 0 ? 1 : slope read from
 *   `below` bf16 [N*H*W][Cin], the stored activation of the layer underneath (torch's LeakyReLU convention at 0; NULL: no
 *   mask, the probability rows).  dx is then the gradient of that layer's PRE-activation: what its own data gradient, its
 *   weight gradient (rgda_conv2d_wgrad_grouped, kh = kw = 4, stride 2, pad 1) and its bias gradient read.
 * rgda_disc_bias_lrelu: y bf16 [M][C] = lrelu(y + bias) in place: the epilogue pass behind rgda_conv2d where the generic
 *   kernel forms a layer's matrix product (measured faster for layers 2-4); C % 32 == 0.  One launch.
 * rgda_disc_bias_grad: db f32 [C] = the column sums of g bf16 [M][C] in a fixed order (two launches); C % 32 == 0;
 *   ws: rgda_disc_bias_grad_workspace(M, C) bytes (0: not served), 16-byte aligned. */
int rgda_disc_conv_fwd(const void* x, const void* wgt, const float* bias, void* y, int N, int H, int W, int Cin, int Cout,
                       float slope, rgda_stream_t stream);
int rgda_disc_conv_bwd_data(const void* dy, const void* wt, const void* below, void* dx, int N, int H, int W, int Cin,
                            int Cout, float slope, rgda_stream_t stream);
int rgda_disc_bias_lrelu(void* y, const float* bias, int64_t M, int C, float slope, rgda_stream_t stream);
size_t rgda_disc_bias_grad_workspace(int64_t M, int C);
int rgda_disc_bias_grad(const void* g, int64_t M, int C, float* db, void* ws, size_t ws_bytes, rgda_stream_t stream);

/* The classifier Conv2d(C, 1, 4, 2, 1) (Discriminator.py:13, 26): a K = 16 C dot product per output pixel.
 * rgda_disc_head_fwd: z f32 [N*(H/2)*(W/2)] = bias[0] + sum a4[src][c] * w[tap][c];  a4 bf16 [N*H*W][C], w f32 [16][C],
 *   C % 32 == 0, H and W even.  One wavefront per output.
 * rgda_disc_head_bwd: from dz f32 [N*(H/2)*(W/2)]: da4 bf16 [N*H*W][C] (masked by a4 > 0 ? 1 : slope: the gradient of the
 *   last layer's pre-activation; NULL: skipped), dw f32 [16][C] and db f32 [1] (both or neither; written, not
 *   accumulated).  One launch each for da4 and for (dw, db).
 * rgda_bce_logits: F.binary_cross_entropy_with_logits(z, full(label)) for a constant label in {0, 1}:
 *   loss[0] = (accumulate ? loss[0] : 0) + scale * mean(max(z, 0) - label * z + log1p(exp(-|z|))),
 *   dz (NULL: not wanted) = scale / n * (sigmoid(z) - label).  One workgroup. */
int rgda_disc_head_fwd(const void* a4, const float* w, const float* bias, float* z, int N, int H, int W, int C,
                       rgda_stream_t stream);
int rgda_disc_head_bwd(const float* dz, const void* a4, const float* w, void* da4, float* dw, float* db, int N, int H, int W,
                       int C, float slope, rgda_stream_t stream);
int rgda_bce_logits(const float* z, int n, float label, float scale, float* loss, int accumulate, float* dz,
                    rgda_stream_t stream);

/* ------------------------------------------------ category-level adversarial alignment (csrc/clan_kernels.hip)
 * CLAN (Luo et al., CVPR 2019) around the discriminator above: ONE discriminator reads softmax(up x1 + up x2) of the two
 * heads, its output is upsampled to the tile, and the BCE there is weighted per pixel by alpha + beta * wmap, wmap the
 * cosine distance of the two heads' probabilities.  `up` is loss_calc's bilinear map (align_corners=True) everywhere.
 * Deterministic: fixed summation orders, no floating-point atomics.  Every check comes before any launch; 6 <= C <= 16,
 * Cp = 16 and every row buffer below 2^31 bytes, or RGDA_ERR_UNSUPPORTED; NULL or misaligned pointers RGDA_ERR_ARG.
 *
 * rgda_clan_probs_fwd: x1, x2 f32 (b, C, h, w).  Per pixel of the H x W tile, with u_i = up(x_i), p_i = softmax(u_i):
 *     P bf16 [b*H*W][Cp] = softmax(u1 + u2), channels C .. Cp-1 zero (rgda_adv_probs_fwd's layout, 16-byte aligned);
 *     wmap f32 [b*H*W]   = 1 - <p1, p2> / (|p1|_2 |p2|_2)     (no clamp, no epsilon: |softmax|_2 >= 1 / sqrt(C)).
 *   One launch, one thread per pixel.  Replaces two F.interpolate, three F.softmax, the cosine similarity and their
 *   autograd nodes.
 * rgda_clan_probs_bwd: dx1, dx2 f32 (b, C, h, w) += scale * (the transpose of that map), from dP bf16 [b*H*W][Cp], the
 *   discriminator's gradient, and gw f32 [b*H*W], the gradient with respect to wmap (NULL: none, the weight is a
 *   constant).  Per pixel, p1, p2 and q = softmax(u1 + u2) recomputed in f32:
 *     both heads receive  q (dP - <q, dP>);
 *     head 1 adds  p1 (g1 - <p1, g1>),  g1 = -gw (p2 / (n1 n2) - s p1 / (n1^3 n2)),  s = <p1, p2>, n_i = |p_i|_2;
 *     head 2 its mirror;
 *   then the transpose of the bilinear map in gather form: one workgroup per low-resolution pixel over its footprint, 2 C
 *   accumulators, a fixed two-level sum in LDS.  One launch.
 * rgda_wbce_logits: WeightedBCEWithLogitsLoss (regda/loss.py:60-85) on an upsampled map.  z f32 [b*hz*wz], zu = up(z) to
 *   H x W (hz == H and wz == W: the identity); t = target[p] (f32 [b*H*W]) or, target NULL, the constant label in {0, 1};
 *     l = max(zu, 0) - t zu + log1p(exp(-|zu|)),    k = wmap ? alpha + beta * wmap[p] : 1      (`weighted()`, :66-79)
 *     loss[0] = (accumulate ? loss[0] : 0) + scale * r * sum_p k l,   r = mean ? 1 / n : 1,  n = b*H*W:  per-workgroup
 *       partials in ws, then one fixed-order sum;
 *     dz f32 [b*hz*wz] (NULL: not wanted) = the transpose of `up` applied to scale * r * k (sigmoid(zu) - t), in gather
 *       form, one workgroup per pixel of z: written, never scattered;
 *     gw f32 [b*H*W] (NULL: not wanted; needs wmap) = scale * r * beta * l, the gradient with respect to wmap.
 *   At most three launches.  ws: rgda_wbce_logits_workspace(b, H, W) bytes (0: not served), 16-byte aligned, or
 *   RGDA_ERR_WORKSPACE. */
int rgda_clan_probs_fwd(const float* x1, const float* x2, void* P, float* wmap, int b, int C, int h, int w, int H, int W,
                        int Cp, rgda_stream_t stream);
int rgda_clan_probs_bwd(const void* dP, const float* gw, const float* x1, const float* x2, float* dx1, float* dx2, int b,
                        int C, int h, int w, int H, int W, int Cp, float scale, rgda_stream_t stream);
size_t rgda_wbce_logits_workspace(int b, int H, int W);
int rgda_wbce_logits(const float* z, int b, int hz, int wz, int H, int W, const float* target, float label, const float* wmap,
                     float alpha, float beta, float scale, int mean, float* loss, int accumulate, float* dz, float* gw,
                     void* ws, size_t ws_bytes, rgda_stream_t stream);

/* ------------------------------------------------ feature-space adversarial alignment (csrc/fada_kernels.hip)
 * PixelDiscriminator (regda/models/Discriminator.py:60-78: D = Conv2d(input_nc, ndf, 3, 1, 1) + LeakyReLU(0.2) +
 * Conv2d(ndf, ndf/2, 3, 1, 1) + LeakyReLU(0.2), then cls1 and cls2 = Conv2d(ndf/2, num_classes, 3, 1, 1), concatenated:
 * FADA's class-level discriminator, Wang et al. 2020) on pixel-major DENSE bf16 rows.  D.0 and D.2 run on rgda_conv2d
 * (mode 0 / mode 1 on the transposed operand), rgda_disc_bias_lrelu, rgda_conv2d_wgrad_grouped and rgda_disc_bias_grad; the
 * entry points below are what those do not provide.  Stored activations are post-LeakyReLU, stored gradients are
 * gradients of pre-activations.  Deterministic: fixed summation orders, no floating-point atomics.  Every check comes
 * before any launch; every row buffer must stay below 2^31 bytes (RGDA_ERR_UNSUPPORTED).
 *
 * rgda_feat_pack_rows: x f32, image n / channel c / pixel p at x[n * ldb + c * ldc + p] (a strided NCHW view: NCHW, a
 *   channel slice, a batch slice) -> rows bf16 [b*hw][ld], columns 0 .. k-1 written (round to nearest even), the others
 *   untouched.  ld >= k, ld % 8 == 0, rows 16-byte aligned.  A 64 x 64 transpose through LDS: loads coalesced along the
 *   pixels, stores along the channels.  Replaces the permute + cast in front of Discriminator.py:72.  One launch.
 * rgda_feat_unpack_rows: the inverse, dx[n * ldb + c * ldc + p] = (accumulate ? dx : 0) + scale * rows[n * hw + p][c].
 * rgda_fada_head: the two heads (Discriminator.py:70-71, 75-77) as ONE 3 x 3 / pad 1 convolution to 32 columns on
 *   v_mfma_f32_32x32x16_bf16: a2 bf16 [N*H*W][Ch], wh bf16 [32][9][Ch] (cls1 rows 0 .. nc-1, cls2 rows nc .. 2nc-1, zero
 *   rows beyond; tap = kh * 3 + kw), bias f32 [32].  Ch % 32 == 0, 1 <= nc <= 16.  Two uses, one or both per call:
 *   z != NULL : z f32 [N*H*W][32] is stored.
 *   x2 != NULL: (z need not be stored) x2 f32 (N, nc, H, W) are logits; with a[k] = min(softmax_k(x2 / T), clip), S = sum_k
 *     a[k], logp = log_softmax(z[0 .. 2nc)), M = N*H*W and side in {0, 1}:
 *       loss[0] += scale / M * sum_p -sum_k a[k] logp[side * nc + k]   (per-workgroup partials in ws, then one fixed-order sum)
 *       dz bf16 [N*H*W][32] = scale / M * (S * softmax(z)_j - a'_j), a' = a in that side's half; columns >= 2nc zero.
 *     T > 0, clip > 0; ws: rgda_fada_head_workspace(M) bytes.  Two launches.
 * rgda_fada_head_bwd_data: da bf16 [N*H*W][Ch] = mask * sum dz[(y + 1 - kh, x + 1 - kw)][j] * wt[c][tap][j] from dz bf16
 *   [N*H*W][32] and wt bf16 [Ch][9][32] (rgda_weight_transpose_bf16 of wh); mask = below > 0 ? 1 : slope from `below` bf16
 *   [N*H*W][Ch], the stored activation.  Also D.2's data gradient where ndf / 2 == 32.  One launch.
 *   The heads' weight and bias gradients are rgda_conv2d_wgrad_grouped and rgda_disc_bias_grad with 32 columns.
 * rgda_lrelu_mask_rows: g bf16 [M][C] *= (a > 0 ? 1 : slope) in place, a bf16 [M][C]; C % 8 == 0: the pass behind the
 *   generic data gradient (rgda_conv2d mode 1) of D.2.  One launch. */
int rgda_feat_pack_rows(const float* x, int b, int hw, int64_t ldc, int64_t ldb, int k, void* rows, int ld,
                        rgda_stream_t stream);
int rgda_feat_unpack_rows(const void* rows, int ld, float* dx, int b, int hw, int64_t ldc, int64_t ldb, int k, float scale,
                          int accumulate, rgda_stream_t stream);
size_t rgda_fada_head_workspace(int64_t M);
int rgda_fada_head(const void* a2, const void* wh, const float* bias, int N, int H, int W, int Ch, int nc, float* z,
                   const float* x2, int side, float T, float clip, float scale, float* loss, void* dz, void* ws,
                   size_t ws_bytes, rgda_stream_t stream);
int rgda_fada_head_bwd_data(const void* dz, const void* wt, const void* below, void* da, int N, int H, int W, int Ch,
                            float slope, rgda_stream_t stream);
int rgda_lrelu_mask_rows(void* g, const void* a, int64_t M, int C, float slope, rgda_stream_t stream);

/* Factored form of the PPM heads' tap-shifted bilinear maps (regda/models/Encoder.py:30-51: Upsample(bilinear,
 * align_corners=False) of the s x s branches into the 3x3 / pad 1 conv_last): the map V[(y,x)][(jy,jx),(ky,kx)] =
 * Uy[y+ky-1][jy] * Ux[x+kx-1][jx] is separable, so V and V^T are applied as two short maps (csrc/mix_kernels.hip).
 *   rgda_group_mix : out[g][i][c] = sum_j W[i][j] * in[g][j][c] for G groups of J consecutive rows, W f32 [I][J]
 *                    (the x direction: one group per image row);
 *   rgda_sparse_mix: out[n][i][c] = sum_k vals[k] * ins[cols[k] >> 24][n][cols[k] & 0xffffff][c] over CSR row i
 *                    (rowptr int32 [I+1], cols int32, vals f32: DEVICE arrays; ins/ldins/Js: HOST arrays, nsrc <= 4;
 *                    the I = sum(out_rows) rows are split over ndst <= 4 image-major output tensors, out_rows[q]
 *                    rows per image each: outs/ldouts/out_rows HOST arrays)
 *                    (the y direction: the gather from the four branch tensors / the scatter back to them).
 * in/out bf16, or f32 where in_f32 / out_f32 != 0; C % 8 == 0; deterministic. */
int rgda_group_mix(const void* in, int ldin, int in_f32, const float* W, void* out, int ldout, int out_f32,
                   int G, int I, int J, int C, rgda_stream_t stream);
int rgda_sparse_mix(int nsrc, const void* const* ins, const int* ldins, const int* Js, int in_f32,
                    const int* rowptr, const int* cols, const float* vals, int ndst, void* const* outs,
                    const int* ldouts, const int* out_rows, int out_f32, int N, int C, rgda_stream_t stream);

/* ------------------------------------------------------------- ASPP head */

/* Classifier_Module (regda/models/Encoder.py:68-84): out = sum_d Conv2d(K -> C, 3x3, padding = dilation = dil[d],
 * bias)(x), for the model's two heads at once.  The 2*4 convolutions' taps are computed as ONE 1x1 convolution
 * (rgda_conv2d) Z = x @ Wstack^T, Z bf16 [N*h*w][ldz] with column ((head*4 + d)*C + c)*9 + tap -- the stacked filter
 * is the eight [C][3][3][K] weights back to back -- and these two entry points do the rest:
 *   gather : out_head f32 (N,C,h,w) = sum_d bias[head*4+d][c] + sum_{d,tap} Z[(y + dy*dil[d], x + dx*dil[d])][col]
 *   scatter: dZ (bf16 [N*h*w][lddz], zc >= 72*C columns, the pad columns zeroed) from the two logit gradients
 *            g_head f32 (N,C,h,w), and dbias[head*4+d][c] += sum g_head[:,c]   (deterministic).
 * bias / dbias: HOST arrays of eight DEVICE pointers; dil: HOST array of four dilations. */
int rgda_aspp_gather(const void* z, int ldz, const float* const* bias, float* out1, float* out2, int N, int h,
                     int w, int C, const int* dil, rgda_stream_t stream);
int rgda_aspp_scatter(const float* g1, const float* g2, void* dz, int lddz, int zc, float* const* dbias, int N,
                      int h, int w, int C, const int* dil, rgda_stream_t stream);

/* ------------------------------------------------------------------ plan replay
 * The reference drives its step from Python, one operator call at a time (tools/train_ssl_reg.py:198-241); so does
 * regda_amd in eager mode -- ~750 entry-point calls per SSL step.  The step's launch sequence is static (fixed shapes,
 * fixed buffers), so the caller may RECORD it once as a table of rows {entry point, arguments packed into 64-bit
 * slots: integers / pointers / streams by value, float and double by bit pattern} and have it replayed by one call.
 * The table, every buffer it points to (device memory and the small host arrays some entry points take) and the
 * streams are caller-owned; nothing is retained or allocated here.
 *   rgda_plan_fn_id("rgda_conv2d") -> index of that entry point in the dispatch table (-1: not replayable; only
 *     int-returning enqueue entry points are), rgda_plan_fn_count() -> table size.
 *   rgda_plan_run: calls the rows in order; stops at the first row whose entry point returns a negative status and
 *     returns that status (*failed_index = its row, when given).  A row with a bad id / argument count -> RGDA_ERR_ARG. */
#define RGDA_PLAN_MAX_ARGS 36
typedef struct rgda_plan_entry {
    int32_t fn;
    int32_t nargs;
    uint64_t args[RGDA_PLAN_MAX_ARGS];
} rgda_plan_entry;
int rgda_plan_fn_count(void);
int rgda_plan_fn_id(const char* name);
int rgda_plan_run(const rgda_plan_entry* entries, int n, int* failed_index);

#ifdef __cplusplus
}
#endif
#endif /* RGDA_HIP_H */
