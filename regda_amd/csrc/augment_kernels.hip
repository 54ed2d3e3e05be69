// Training augmentation of raw tiles (regda/aug/augmentation.py and the albumentations pipeline of
// configs/ToPotsdam.py): crop + one dihedral element + the normalisation / label tables, for a whole batch of one
// domain in one launch.  The geometry is a pure gather; every value goes through a per-(channel, byte) table, so the
// kernel does no floating-point arithmetic (include/rgda_hip.h: rgda_augment_tiles).  rgda_augment_affine warps the same
// planes by one affine map per sample (random scale and rotation): bilinear image taps in integers, nearest labels and
// regions, the soft planes in f32.
#include "common.h"

namespace {

constexpr int AUG_S = 32;                       // output tile edge: one workgroup writes an S x S tile of every plane
constexpr int AUG_THREADS = 256;                // S rows x S/4 quads: one thread = 4 consecutive pixels of one row
constexpr int AUG_IMG_DW = (3 * AUG_S + 3 + 3) / 4;     // dwords per staged uint8 HWC window row (with its head offset)
constexpr int AUG_LD = AUG_S + 1;               // padded LDS row (4-byte planes): the transposing reads do not collide

// dword k of a uint8 buffer of `total` bytes (base 4-byte aligned); the dword holding the buffer's last bytes is
// assembled byte by byte so no byte past the end is read
__device__ __forceinline__ uint32_t load_dword(const uint8_t* __restrict__ base, long long k, long long total) {
    if (4 * k + 4 <= total) return reinterpret_cast<const uint32_t*>(base)[k];
    uint32_t v = 0;
    for (int b = 0; b < 4 && 4 * k + b < total; ++b) v |= (uint32_t)base[4 * k + b] << (8 * b);
    return v;
}

// out[0..3] -> p[0..3]: one 16-byte store when the quad is whole (vec), else the pixels inside the tile one by one
template <typename T>
__device__ __forceinline__ void store4(T* __restrict__ p, const T (&v)[4], int cnt, bool vec) {
    if (vec && cnt == 4) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            typedef __attribute__((ext_vector_type(2))) long long i64x2;
            reinterpret_cast<i64x2*>(p)[0] = i64x2{(long long)v[0], (long long)v[1]};
            reinterpret_cast<i64x2*>(p)[1] = i64x2{(long long)v[2], (long long)v[3]};
        }
    } else {
        for (int e = 0; e < cnt; ++e) p[e] = v[e];
    }
}

// grid (tiles, N).  Sample n: crop origin (y0, x0), element d = t | fr << 1 | fc << 2 of params[n]; output pixel (i, j)
// reads crop pixel (y, x) with (u, v) = t ? (j, i) : (i, j), y = fr ? Ho-1-u : u, x = fc ? Wo-1-v : v.  The tile's
// source is an S x S window of the crop (rows / columns swapped when t): staged in LDS with row-contiguous reads, then
// every output plane is written in whole rows.
__global__ void __launch_bounds__(AUG_THREADS) augment_tiles_kernel(
    const uint8_t* __restrict__ img, const uint8_t* __restrict__ label, const float* __restrict__ soft,
    const int32_t* __restrict__ regs, const int32_t* __restrict__ params, int Hi, int Wi, int C, int Ho, int Wo,
    long long img_bytes, const float* __restrict__ lut, const int32_t* __restrict__ label_lut, float* __restrict__ img_out,
    int64_t* __restrict__ label_out, float* __restrict__ soft_out, int64_t* __restrict__ regs_out, int* __restrict__ flag,
    int vec) {
    extern __shared__ float s_soft[];                           // [C][S][AUG_LD] when soft is given
    __shared__ float s_lut[3 * 256];
    __shared__ int s_llut[256];
    __shared__ uint32_t s_img[AUG_S * AUG_IMG_DW];
    __shared__ int s_reg[AUG_S * AUG_LD];
    __shared__ uint8_t s_lab[AUG_S * (AUG_S + 4)];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int y0 = params[4 * n], x0 = params[4 * n + 1], d = params[4 * n + 2];
    const int t = d & 1, fr = (d >> 1) & 1, fc = (d >> 2) & 1;
    if (d < 0 || d > 7 || (t && Ho != Wo) || y0 < 0 || x0 < 0 || y0 > Hi - Ho || x0 > Wi - Wo) {
        if (flag && blockIdx.x == 0 && tid == 0) *flag = 1;         // the sample is skipped; every writer stores 1
        return;
    }
    const int tiles_x = (Wo + AUG_S - 1) / AUG_S;
    const int I0 = (blockIdx.x / tiles_x) * AUG_S, J0 = (blockIdx.x % tiles_x) * AUG_S;
    const int ti = min(AUG_S, Ho - I0), tj = min(AUG_S, Wo - J0);
    // the window of crop rows [ylo, ylo + wr) x columns [xlo, xlo + wc) that this tile reads
    const int ulo = t ? J0 : I0, wr = t ? tj : ti, vlo = t ? I0 : J0, wc = t ? ti : tj;
    const int ylo = fr ? Ho - ulo - wr : ulo, xlo = fc ? Wo - vlo - wc : vlo;
    const int gy = y0 + ylo, gx = x0 + xlo;

    for (int k = tid; k < 3 * 256; k += AUG_THREADS) s_lut[k] = lut[k];
    if (label)
        for (int k = tid; k < 256; k += AUG_THREADS) s_llut[k] = label_lut[k];
    for (int e = tid; e < wr * AUG_IMG_DW; e += AUG_THREADS) {
        const int r = e / AUG_IMG_DW, q = e - r * AUG_IMG_DW;
        const long long b0 = (((long long)n * Hi + gy + r) * Wi + gx) * 3;
        if ((b0 >> 2) + q <= (b0 + 3 * wc - 1) >> 2) s_img[e] = load_dword(img, (b0 >> 2) + q, img_bytes);
    }
    for (int e = tid; e < wr * AUG_S; e += AUG_THREADS) {
        const int r = e / AUG_S, c = e % AUG_S;
        if (c >= wc) continue;
        const long long p = ((long long)n * Hi + gy + r) * Wi + gx + c;
        if (label) s_lab[r * (AUG_S + 4) + c] = label[p];
        if (regs) s_reg[r * AUG_LD + c] = regs[p];
    }
    if (soft)
        for (int e = tid; e < C * wr * AUG_S; e += AUG_THREADS) {
            const int c = e % AUG_S, r = (e / AUG_S) % wr, ch = e / (AUG_S * wr);
            if (c < wc) s_soft[(ch * AUG_S + r) * AUG_LD + c] = soft[(((long long)n * C + ch) * Hi + gy + r) * Wi + gx + c];
        }
    __syncthreads();

    const int a = tid / (AUG_S / 4), b = (tid % (AUG_S / 4)) * 4;
    if (a >= ti || b >= tj) return;
    const int cnt = min(4, tj - b);
    int wy[4], wx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ul = t ? b + e : a, vl = t ? a : b + e;
        wy[e] = fr ? wr - 1 - ul : ul;
        wx[e] = fc ? wc - 1 - vl : vl;
    }
    const long long plane = (long long)Ho * Wo, o = (long long)(I0 + a) * Wo + J0 + b;
    const uint8_t* s_imgb = reinterpret_cast<const uint8_t*>(s_img);
    int ib[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int head = (int)(((((long long)n * Hi + gy + wy[e]) * Wi + gx) * 3) & 3);
        ib[e] = wy[e] * AUG_IMG_DW * 4 + head + 3 * wx[e];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = s_lut[ch * 256 + s_imgb[ib[e] + ch]];
        store4(img_out + ((long long)n * 3 + ch) * plane + o, v, cnt, vec);
    }
    if (label) {
        int64_t v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = s_llut[s_lab[wy[e] * (AUG_S + 4) + wx[e]]];
        store4(label_out + n * plane + o, v, cnt, vec);
    }
    if (regs) {
        int64_t v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = s_reg[wy[e] * AUG_LD + wx[e]];
        store4(regs_out + n * plane + o, v, cnt, vec);
    }
    if (soft)
        for (int ch = 0; ch < C; ++ch) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = s_soft[(ch * AUG_S + wy[e]) * AUG_LD + wx[e]];
            store4(soft_out + ((long long)n * C + ch) * plane + o, v, cnt, vec);
        }
}

// ---------------------------------------------------------------------------------------------- affine warp
constexpr int AFF_IMG_DW = 8192;                // LDS budget of the staged uint8 HWC window: 32 KB
constexpr int AFF_A_MAX = 131072;               // |a_kl| <= 4 * 32768: a scale inside [1/4, 4]

// One bilinear tap set of an output pixel: the top-left source pixel (y, x), the 8-bit fractions, and which of the rows
// y, y + 1 and columns x, x + 1 lie inside the input (none for a pixel past the tile's edge, `live` false: its taps are
// never read).
struct AffTap {
    int y, x, fy, fx;
    bool y0, y1, x0, x1;
};

__device__ __forceinline__ AffTap aff_tap(long long Y, long long X, int Hi, int Wi, bool live) {
    const long long Yp = Y - 32768, Xp = X - 32768;
    AffTap t;
    t.y = (int)(Yp >> 16);
    t.x = (int)(Xp >> 16);
    t.fy = (int)(Yp & 0xFFFF) >> 8;
    t.fx = (int)(Xp & 0xFFFF) >> 8;
    t.y0 = live && t.y >= 0 && t.y < Hi;
    t.y1 = live && t.y + 1 >= 0 && t.y + 1 < Hi;
    t.x0 = live && t.x >= 0 && t.x < Wi;
    t.x1 = live && t.x + 1 >= 0 && t.x + 1 < Wi;
    return t;
}

// grid (tiles, N).  Row n of params: (cy, cx, a00, a01, a10, a11, fill, 0); output pixel (i, j) has the source coordinate
// Y = cy + a00 u + a01 v, X = cx + a10 u + a11 v in 1/65536 pixel, u = 2i + 1 - Ho, v = 2j + 1 - Wo (int64).  Image:
// four taps with 8-bit weights in integers, then the table; label / regions: the nearest pixel; soft planes: the image's
// taps and weights in f32.  The tile's taps lie in the bounding box of its four corner pixels' taps (Y, X are affine in
// (i, j) and the floor is monotone); that window of the uint8 image, clipped to the input, is staged in LDS as dwords
// when it fits AFF_IMG_DW and read from global memory otherwise -- the same bytes either way.
__global__ void __launch_bounds__(AUG_THREADS) augment_affine_kernel(
    const uint8_t* __restrict__ img, const uint8_t* __restrict__ label, const float* __restrict__ soft,
    const int32_t* __restrict__ regs, const int32_t* __restrict__ params, int Hi, int Wi, int C, int Ho, int Wo,
    long long img_bytes, const float* __restrict__ lut, const int32_t* __restrict__ label_lut, int ignore_label,
    float* __restrict__ img_out, int64_t* __restrict__ label_out, float* __restrict__ soft_out,
    int64_t* __restrict__ regs_out, int* __restrict__ flag, int vec) {
    __shared__ float s_lut[3 * 256];
    __shared__ int s_llut[256];
    __shared__ uint32_t s_img[AFF_IMG_DW];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int32_t* prm = params + 8 * n;
    const int cy = prm[0], cx = prm[1], a00 = prm[2], a01 = prm[3], a10 = prm[4], a11 = prm[5], fill = prm[6];
    const int amin = min(min(a00, a01), min(a10, a11)), amax = max(max(a00, a01), max(a10, a11));
    if (amin < -AFF_A_MAX || amax > AFF_A_MAX || cy < 0 || cy > Hi * 65536 || cx < 0 || cx > Wi * 65536 || prm[7] != 0 ||
        ((uint32_t)fill >> 24) != 0) {
        if (flag && blockIdx.x == 0 && tid == 0) *flag = 1;         // the sample is skipped; every writer stores 1
        return;
    }
    const int tiles_x = (Wo + AUG_S - 1) / AUG_S;
    const int I0 = (blockIdx.x / tiles_x) * AUG_S, J0 = (blockIdx.x % tiles_x) * AUG_S;
    const int ti = min(AUG_S, Ho - I0), tj = min(AUG_S, Wo - J0);

    // the window of input rows [gy, gy + wr) x columns [gx, gx + wc) that holds every in-frame tap of this tile
    int ymin = 0x7fffffff, ymax = -0x7fffffff, xmin = 0x7fffffff, xmax = -0x7fffffff;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long u = 2 * (long long)((k & 1) ? I0 + ti - 1 : I0) + 1 - Ho;
        const long long v = 2 * (long long)((k & 2) ? J0 + tj - 1 : J0) + 1 - Wo;
        const int y = (int)((cy + a00 * u + a01 * v - 32768) >> 16), x = (int)((cx + a10 * u + a11 * v - 32768) >> 16);
        ymin = min(ymin, y), ymax = max(ymax, y), xmin = min(xmin, x), xmax = max(xmax, x);
    }
    const int gy = max(ymin, 0), gx = max(xmin, 0);
    const int wr = min(ymax + 1, Hi - 1) - gy + 1, wc = min(xmax + 1, Wi - 1) - gx + 1;
    const int rd = (3 * wc + 6) / 4;                            // dwords per staged window row (with its head offset)
    const bool staged = wr > 0 && wc > 0 && (long long)wr * rd <= AFF_IMG_DW;
    const long long base3 = (((long long)n * Hi + gy) * Wi + gx) * 3;  // byte offset of the window's first pixel

    for (int k = tid; k < 3 * 256; k += AUG_THREADS) s_lut[k] = lut[k];
    if (label)
        for (int k = tid; k < 256; k += AUG_THREADS) s_llut[k] = label_lut[k];
    if (staged)
        for (int e = tid; e < wr * rd; e += AUG_THREADS) {
            const int r = e / rd, q = e - r * rd;
            const long long b0 = base3 + (long long)r * Wi * 3;
            if ((b0 >> 2) + q <= (b0 + 3 * wc - 1) >> 2) s_img[e] = load_dword(img, (b0 >> 2) + q, img_bytes);
        }
    __syncthreads();

    const int a = tid / (AUG_S / 4), b = (tid % (AUG_S / 4)) * 4;
    if (a >= ti || b >= tj) return;
    const int cnt = min(4, tj - b);
    const long long plane = (long long)Ho * Wo, o = (long long)(I0 + a) * Wo + J0 + b;
    const long long u = 2 * (long long)(I0 + a) + 1 - Ho, v0 = 2 * (long long)(J0 + b) + 1 - Wo;
    const long long Y0 = cy + a00 * u + a01 * v0, X0 = cx + a10 * u + a11 * v0;
    const uint8_t* s_imgb = reinterpret_cast<const uint8_t*>(s_img);
    const uint8_t* img_n = img + (long long)n * Hi * Wi * 3;
    const int h0 = (int)(base3 & 3), w3 = (Wi * 3) & 3;

    AffTap tap[4];                                              // kept for the soft planes
    float iv[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        tap[e] = aff_tap(Y0 + 2LL * e * a01, X0 + 2LL * e * a11, Hi, Wi, e < cnt);
        const AffTap& t = tap[e];
        const uint32_t w00 = (256 - t.fx) * (256 - t.fy), w01 = t.fx * (256 - t.fy), w10 = (256 - t.fx) * t.fy,
                       w11 = t.fx * t.fy;
        // byte offset of the pixel (y, x) and of the one below it, in the staged window or in the sample's image (of a
        // row inside the input; the other row's offset is not used)
        long long p0, p1;
        if (staged) {
            const int r0 = t.y0 ? t.y - gy : 0, r1 = t.y1 ? t.y + 1 - gy : 0;
            p0 = r0 * rd * 4 + ((h0 + r0 * w3) & 3) + 3 * (t.x - gx);
            p1 = r1 * rd * 4 + ((h0 + r1 * w3) & 3) + 3 * (t.x - gx);
        } else {
            p0 = ((long long)t.y * Wi + t.x) * 3;
            p1 = p0 + (long long)Wi * 3;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t f = ((uint32_t)fill >> (8 * ch)) & 255;
            uint32_t q00 = f, q01 = f, q10 = f, q11 = f;
            if (staged) {
                if (t.y0 && t.x0) q00 = s_imgb[p0 + ch];
                if (t.y0 && t.x1) q01 = s_imgb[p0 + 3 + ch];
                if (t.y1 && t.x0) q10 = s_imgb[p1 + ch];
                if (t.y1 && t.x1) q11 = s_imgb[p1 + 3 + ch];
            } else {
                if (t.y0 && t.x0) q00 = img_n[p0 + ch];
                if (t.y0 && t.x1) q01 = img_n[p0 + 3 + ch];
                if (t.y1 && t.x0) q10 = img_n[p1 + ch];
                if (t.y1 && t.x1) q11 = img_n[p1 + 3 + ch];
            }
            iv[ch][e] = s_lut[ch * 256 + ((w00 * q00 + w01 * q01 + w10 * q10 + w11 * q11 + 32768) >> 16)];
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) store4(img_out + ((long long)n * 3 + ch) * plane + o, iv[ch], cnt, vec);

    if (label || regs) {
        // the nearest pixel's offset inside the batch, or -1 outside the input
        long long np[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int y = (int)((Y0 + 2LL * e * a01) >> 16), x = (int)((X0 + 2LL * e * a11) >> 16);
            const bool in = e < cnt && y >= 0 && y < Hi && x >= 0 && x < Wi;
            np[e] = in ? ((long long)n * Hi + y) * Wi + x : -1;
        }
        if (label) {
            int64_t lv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) lv[e] = np[e] >= 0 ? s_llut[label[np[e]]] : ignore_label;
            store4(label_out + n * plane + o, lv, cnt, vec);
        }
        if (regs) {
            int64_t rv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) rv[e] = np[e] >= 0 ? regs[np[e]] : 0;
            store4(regs_out + n * plane + o, rv, cnt, vec);
        }
    }
    if (soft) {
        // per pixel: the four weights, the offsets of (y, x) and its right / lower neighbours inside one plane (a tap
        // outside the input is never loaded: it contributes 0)
        float w[4][4];
        int p0[4];
        bool ok[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const AffTap& t = tap[e];
            w[e][0] = (float)((256 - t.fx) * (256 - t.fy)), w[e][1] = (float)(t.fx * (256 - t.fy));
            w[e][2] = (float)((256 - t.fx) * t.fy), w[e][3] = (float)(t.fx * t.fy);
            ok[e][0] = t.y0 && t.x0, ok[e][1] = t.y0 && t.x1, ok[e][2] = t.y1 && t.x0, ok[e][3] = t.y1 && t.x1;
            p0[e] = t.y * Wi + t.x;
        }
        for (int ch = 0; ch < C; ++ch) {
            const float* sp = soft + ((long long)n * C + ch) * Hi * Wi;
            float sv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float q00 = ok[e][0] ? sp[p0[e]] : 0.f, q01 = ok[e][1] ? sp[p0[e] + 1] : 0.f;
                const float q10 = ok[e][2] ? sp[p0[e] + Wi] : 0.f, q11 = ok[e][3] ? sp[p0[e] + Wi + 1] : 0.f;
                sv[e] = (w[e][0] * q00 + w[e][1] * q01 + w[e][2] * q10 + w[e][3] * q11) * (1.f / 65536.f);
            }
            store4(soft_out + ((long long)n * C + ch) * plane + o, sv, cnt, vec);
        }
    }
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int rgda_augment_tiles(const uint8_t* img, const uint8_t* label, const float* soft, const int32_t* regs,
                                  const int32_t* params, int N, int Hi, int Wi, int C, int Ho, int Wo, const float* lut,
                                  const int32_t* label_lut, float* img_out, int64_t* label_out, float* soft_out,
                                  int64_t* regs_out, int* flag, rgda_stream_t stream) {
    if (!img || !params || !lut || !img_out || N < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1) return RGDA_ERR_ARG;
    if (Ho > Hi || Wo > Wi) return RGDA_ERR_ARG;                         // the crop cannot lie inside the input
    if ((label && (!label_lut || !label_out)) || (soft && (C < 1 || !soft_out)) || (regs && !regs_out))
        return RGDA_ERR_ARG;
    if (soft && C > 8) return RGDA_ERR_UNSUPPORTED;                    // the soft planes of a tile are staged in LDS
    if (!aligned(img, 4) || (soft && !aligned(soft, 4)) || (regs && !aligned(regs, 4)) || !aligned(lut, 4) ||
        (label_lut && !aligned(label_lut, 4)) || !aligned(params, 4))
        return RGDA_ERR_ARG;
    const bool vec = Wo % 4 == 0 && aligned(img_out, 16) && (!label || aligned(label_out, 16)) &&
                     (!soft || aligned(soft_out, 16)) && (!regs || aligned(regs_out, 16));
    const long long tiles = (long long)((Ho + AUG_S - 1) / AUG_S) * ((Wo + AUG_S - 1) / AUG_S);
    if (tiles > 0x7fffffff || N > 65535) return RGDA_ERR_UNSUPPORTED;
    const size_t lds = soft ? (size_t)C * AUG_S * AUG_LD * sizeof(float) : 0;
    augment_tiles_kernel<<<dim3((unsigned)tiles, (unsigned)N), AUG_THREADS, lds, to_stream(stream)>>>(
        img, label, soft, regs, params, Hi, Wi, soft ? C : 0, Ho, Wo, (long long)N * Hi * Wi * 3, lut, label_lut,
        img_out, label_out, soft_out, regs_out, flag, vec ? 1 : 0);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_augment_affine(const uint8_t* img, const uint8_t* label, const float* soft, const int32_t* regs,
                                   const int32_t* params, int N, int Hi, int Wi, int C, int Ho, int Wo, const float* lut,
                                   const int32_t* label_lut, int ignore_label, float* img_out, int64_t* label_out,
                                   float* soft_out, int64_t* regs_out, int* flag, rgda_stream_t stream) {
    if (!img || !params || !lut || !img_out || N < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1) return RGDA_ERR_ARG;
    if ((label && (!label_lut || !label_out)) || (soft && (C < 1 || !soft_out)) || (regs && !regs_out))
        return RGDA_ERR_ARG;
    if (!aligned(img, 4) || (soft && !aligned(soft, 4)) || (regs && !aligned(regs, 4)) || !aligned(lut, 4) ||
        (label_lut && !aligned(label_lut, 4)) || !aligned(params, 4))
        return RGDA_ERR_ARG;
    // 16384 * 65536 is the largest centre an int32 row holds; 8192 keeps a_kl * u inside 2^31 per term
    // N is the grid's second dimension
    if (Hi > 16384 || Wi > 16384 || Ho > 8192 || Wo > 8192 || (soft && C > 16) || N > 65535) return RGDA_ERR_UNSUPPORTED;
    const bool vec = Wo % 4 == 0 && aligned(img_out, 16) && (!label || aligned(label_out, 16)) &&
                     (!soft || aligned(soft_out, 16)) && (!regs || aligned(regs_out, 16));
    const int tiles = ((Ho + AUG_S - 1) / AUG_S) * ((Wo + AUG_S - 1) / AUG_S);
    augment_affine_kernel<<<dim3((unsigned)tiles, (unsigned)N), AUG_THREADS, 0, to_stream(stream)>>>(
        img, label, soft, regs, params, Hi, Wi, soft ? C : 0, Ho, Wo, (long long)N * Hi * Wi * 3, lut, label_lut,
        ignore_label, img_out, label_out, soft_out, regs_out, flag, vec ? 1 : 0);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
