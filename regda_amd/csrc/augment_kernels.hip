// Training augmentation of raw tiles (regda/aug/augmentation.py and the albumentations pipeline of
// configs/ToPotsdam.py): crop + one dihedral element + the normalisation / label tables, for a whole batch of one
// domain in one launch.  The geometry is a pure gather; every value goes through a per-(channel, byte) table, so the
// kernel does no floating-point arithmetic (include/rgda_hip.h: rgda_augment_tiles).
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
