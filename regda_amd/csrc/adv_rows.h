// What the kernels of the probability rows share (adv_kernels.hip, clan_kernels.hip): the row layout, the byte limit, the
// interpolated logits and the softmax of one pixel and the footprint of the gather-form bilinear transpose.
#pragma once
#include "common.h"

#define ADV_CP 16
#define ADV_BYTES_MAX 0x7fffffffLL       // row buffers are addressed below 2^31 bytes

static inline bool adv_fits(long long rows, long long cols, long long elem) { return rows * cols * elem <= ADV_BYTES_MAX; }

// one full-resolution pixel: the C interpolated logits
template <int C>
static __device__ __forceinline__ void adv_logits_at(const float* __restrict__ xb, int h, int w, const Lerp& ly, const Lerp& lx,
                                                     float (&u)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* q = xb + (size_t)c * h * w;
        const float top = q[ly.i0 * w + lx.i0] * lx.l0 + q[ly.i0 * w + lx.i1] * lx.l1;
        const float bot = q[ly.i1 * w + lx.i0] * lx.l0 + q[ly.i1 * w + lx.i1] * lx.l1;
        u[c] = top * ly.l0 + bot * ly.l1;
    }
}
// softmax over the C values, in place
template <int C>
static __device__ __forceinline__ void adv_softmax(float (&p)[C]) {
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, p[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { p[c] = expf(p[c] - mx); s += p[c]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] *= inv;
}
template <int C>
static __device__ __forceinline__ void adv_probs_at(const float* __restrict__ xb, int h, int w, const Lerp& ly, const Lerp& lx,
                                                    float (&p)[C]) {
    adv_logits_at<C>(xb, h, w, ly, lx, p);
    adv_softmax<C>(p);
}

// the source rows (columns) of an align_corners=True map that touch low-resolution index i: a conservative range, the
// exact weight is taken from lerp_ac per candidate
static __device__ __forceinline__ void adv_footprint(int i, int in, int out, int& lo, int& hi) {
    if (in <= 1 || out <= 1) { lo = 0; hi = out - 1; return; }
    const float inv = (float)(out - 1) / (float)(in - 1);
    lo = max(0, (int)floorf((float)(i - 1) * inv) - 1);
    hi = min(out - 1, (int)ceilf((float)(i + 1) * inv) + 1);
}
static __device__ __forceinline__ float adv_weight_of(const Lerp& l, int i) {
    return (l.i0 == i ? l.l0 : 0.f) + (l.i1 == i ? l.l1 : 0.f);
}
