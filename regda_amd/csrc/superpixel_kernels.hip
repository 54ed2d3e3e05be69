// Region maps without SAM: an integer SLIC, 4-connected components with min-index roots, and the reference's
// edge_shrinking (include/rgda_hip.h: rgda_superpixels, rgda_region_shrink).
//
// NOT pinned: the superpixel algorithm.  The reference generates its superpixels with cv2.ximgproc.createSuperpixelLSC
// (regda/gast/superpixels.py:49-83) and skimage.segmentation.slic (regda/gast/slic/superpixel.py:66-90), both third
// party; this generator stands in for them and reproduces neither.  It is this project's own specification (integers
// only, ties defined), restated in numpy in tests/superpixel_ref.py and matched bit for bit.
// PINNED: edge_shrinking (regda/gast/superpixels.py:129-152), the reference's own loop; bit-exact against a golden
// minted from it.
//
// One call is 2 + iters + 7 launches and no host synchronisation:
//   fill (centres + sums) | slic_iter<INIT> | slic_iter<MID> x (iters - 1) | slic_iter<LAST> |
//   ccl_local | ccl_merge | ccl_compress | root_count | root_scan | root_number | region_write
// An iteration reads the image once: Assign(it) and the sum half of Update(it) are one pass, the division half of
// Update(it) is redone by every workgroup of iteration it + 1 for its <= 100 candidate centres, and only the last
// Assign writes the label map.  Small components are dropped to region 0, never merged into a neighbour.
#include <limits.h>

#include "common.h"

namespace {

constexpr int SPX_THREADS = 256;
constexpr int SPX_TILE = 32;                          // a workgroup covers max(1, 32 / S) x max(1, 32 / S) cells
constexpr int SPX_MAX_T = 64;                         // ... so a tile edge is at most max(32, S) = 64 pixels
constexpr int SPX_IMG_DW = (3 * SPX_MAX_T + 3 + 3) / 4;   // dwords per staged uint8 HWC row (with its head offset)
constexpr int SPX_MAX_CAND = (SPX_TILE / 4 + 2) * (SPX_TILE / 4 + 2);     // S = 4: 8 x 8 cells and their ring
constexpr int CCL_T = 32;                             // component tile edge
constexpr int SCAN_CHUNK = 1024;                      // pixels per workgroup of the root numbering passes
constexpr int SHR_T = 32, SHR_MAX_WIN = 8, SHR_LD = SHR_T + 2 * SHR_MAX_WIN + 1;

enum { SLIC_INIT = 0, SLIC_MID = 1, SLIC_LAST = 2 };

// dword k of a uint8 buffer of `total` bytes (base 4-byte aligned); the dword holding the buffer's last bytes is
// assembled byte by byte so no byte past the end is read
__device__ __forceinline__ uint32_t load_dword(const uint8_t* __restrict__ base, long long k, long long total) {
    if (4 * k + 4 <= total) return reinterpret_cast<const uint32_t*>(base)[k];
    uint32_t v = 0;
    for (int b = 0; b < 4 && 4 * k + b < total; ++b) v |= (uint32_t)base[4 * k + b] << (8 * b);
    return v;
}

// ---- SLIC.  grid (cell blocks, N).  The workgroup owns the cells [cy0, cy0 + ncy) x [cx0, cx0 + ncx) and their
// pixels; the candidate centres are those cells and the ring around them, slot (i, j) = cell (cy0 - 1 + i, cx0 - 1 + j).
//   INIT: every pixel is labelled with its own cell; the sums go to sums_out.
//   MID : centres = Update(sums_in, ctr_prev) for the candidates (the owned ones are also written to ctr_cur, and their
//         entries of sums_zero -- the buffer read one iteration ago -- are cleared for the next); Assign; sums to sums_out.
//   LAST: as MID, but the labels are written and nothing is summed.
// Sums: LDS atomics per pixel, then one global atomic per non-zero (candidate, component) of the workgroup.  Integer
// sums do not depend on the order of the additions.
template <int MODE>
__global__ void __launch_bounds__(SPX_THREADS) slic_iter_kernel(
    const uint8_t* __restrict__ img, long long img_bytes, int H, int W, int S, int bc, int Gy, int Gx, int m2,
    const int* __restrict__ sums_in, const int* __restrict__ ctr_prev, int* __restrict__ ctr_cur,
    int* __restrict__ sums_out, int* __restrict__ sums_zero, int* __restrict__ labels) {
    __shared__ uint32_t s_img[SPX_MAX_T * SPX_IMG_DW];
    __shared__ int s_ctr[SPX_MAX_CAND * 5];
    __shared__ int s_sum[SPX_MAX_CAND * 6];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int nbx = (Gx + bc - 1) / bc;
    const int cy0 = (blockIdx.x / nbx) * bc, cx0 = (blockIdx.x % nbx) * bc;
    const int ncy = min(bc, Gy - cy0), ncx = min(bc, Gx - cx0);
    const int y0 = cy0 * S, x0 = cx0 * S, th = ncy * S, tw = ncx * S;
    const int cw = bc + 2;
    const long long K = (long long)Gy * Gx;

    for (int e = tid; e < cw * cw; e += SPX_THREADS) {
        const int i = e / cw, j = e - i * cw;
        const int gy = cy0 - 1 + i, gx = cx0 - 1 + j;
        for (int c = 0; c < 6; ++c) s_sum[e * 6 + c] = 0;
        if (MODE == SLIC_INIT || i > ncy + 1 || j > ncx + 1 || gy < 0 || gy >= Gy || gx < 0 || gx >= Gx) continue;
        const long long k = n * K + (long long)gy * Gx + gx;
        const bool owned = i >= 1 && i <= ncy && j >= 1 && j <= ncx;
        const int cnt = sums_in[k * 6 + 5];
        for (int c = 0; c < 5; ++c) {
            const int v = cnt > 0 ? (2 * sums_in[k * 6 + c] + cnt) / (2 * cnt) : ctr_prev[k * 5 + c];
            s_ctr[e * 5 + c] = v;
            if (owned) ctr_cur[k * 5 + c] = v;
        }
        if (owned)
            for (int c = 0; c < 6; ++c) sums_zero[k * 6 + c] = 0;
    }
    for (int e = tid; e < th * SPX_IMG_DW; e += SPX_THREADS) {
        const int r = e / SPX_IMG_DW, q = e - r * SPX_IMG_DW;
        const long long b0 = (((long long)n * H + y0 + r) * W + x0) * 3;
        if ((b0 >> 2) + q <= (b0 + 3 * tw - 1) >> 2) s_img[e] = load_dword(img, (b0 >> 2) + q, img_bytes);
    }
    __syncthreads();

    const uint8_t* s_imgb = reinterpret_cast<const uint8_t*>(s_img);
    const int S2 = S * S;
    for (int e = tid; e < th * tw; e += SPX_THREADS) {
        const int ly = e / tw, lx = e - ly * tw;
        const int y = y0 + ly, x = x0 + lx;
        const int head = (int)(((((long long)n * H + y) * W + x0) * 3) & 3);
        const uint8_t* px = s_imgb + ly * SPX_IMG_DW * 4 + head + 3 * lx;
        const int r = px[0], g = px[1], b = px[2];
        const int li = ly / S + 1, lj = lx / S + 1;           // the pixel's own cell as a candidate slot
        int best = li * cw + lj;
        if (MODE != SLIC_INIT) {
            int bd = INT_MAX;
            for (int a = -1; a <= 1; ++a) {
                const int gy = cy0 - 1 + li + a;
                if (gy < 0 || gy >= Gy) continue;
                for (int bb = -1; bb <= 1; ++bb) {
                    const int gx = cx0 - 1 + lj + bb;
                    if (gx < 0 || gx >= Gx) continue;
                    const int* c = s_ctr + ((li + a) * cw + lj + bb) * 5;
                    const int dy = y - c[0], dx = x - c[1], dr = r - c[2], dg = g - c[3], db = b - c[4];
                    const int d = (dr * dr + dg * dg + db * db) * S2 + m2 * (dy * dy + dx * dx);
                    if (d < bd) { bd = d; best = (li + a) * cw + lj + bb; }      // ascending k: the smaller k keeps a tie
                }
            }
        }
        if (MODE == SLIC_LAST) {
            const int bi = best / cw, bj = best - bi * cw;
            labels[((long long)n * H + y) * W + x] = (cy0 - 1 + bi) * Gx + (cx0 - 1 + bj);
        } else {
            int* s = s_sum + best * 6;
            atomicAdd(s + 0, y); atomicAdd(s + 1, x); atomicAdd(s + 2, r); atomicAdd(s + 3, g); atomicAdd(s + 4, b);
            atomicAdd(s + 5, 1);
        }
    }
    if (MODE == SLIC_LAST) return;
    __syncthreads();
    for (int e = tid; e < cw * cw * 6; e += SPX_THREADS) {
        const int v = s_sum[e];
        if (v == 0) continue;                                   // also every slot outside the grid: nothing was added there
        const int slot = e / 6, c = e - slot * 6;
        const int i = slot / cw, j = slot - i * cw;
        const long long k = n * K + (long long)(cy0 - 1 + i) * Gx + (cx0 - 1 + j);
        atomicAdd(sums_out + k * 6 + c, v);
    }
}

// ---- 4-connected components of equal labels.  parent[p] <= p always, so a tree's root is its smallest pixel index.
__device__ __forceinline__ int lds_find(int* par, int a) {
    for (;;) {
        const int p = __hip_atomic_load(par + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == a) return a;
        a = p;
    }
}
__device__ __forceinline__ void lds_unite(int* par, int a, int b) {
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }           // a > b: hang a under b, unless a got a parent meanwhile
        const int old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}
// The merge pass touches `parent` through returning atomics only: they execute at the memory side, so what one workgroup
// links every other sees, whichever XCD's L2 it sits behind.
__device__ __forceinline__ int glb_find(int* par, int a) {
    for (;;) {
        const int p = atomicMin(par + a, INT_MAX);             // an atomic read
        if (p == a) return a;
        a = p;
    }
}
__device__ __forceinline__ void glb_unite(int* par, int a, int b) {
    for (;;) {
        a = glb_find(par, a);
        b = glb_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}

// grid (tiles, N): the components of one 32 x 32 tile in LDS.  parent[p] = the piece's smallest pixel (an index into
// the image), area[p] = the piece's pixel count at that pixel and 0 elsewhere (every entry is written).
__global__ void __launch_bounds__(SPX_THREADS) ccl_local_kernel(const int* __restrict__ labels, int* __restrict__ parent,
                                                                 int* __restrict__ area, int H, int W) {
    __shared__ int s_lab[CCL_T * CCL_T], s_par[CCL_T * CCL_T], s_cnt[CCL_T * CCL_T];
    const int tid = threadIdx.x;
    const int tx = (W + CCL_T - 1) / CCL_T;
    const int Y0 = (blockIdx.x / tx) * CCL_T, X0 = (blockIdx.x % tx) * CCL_T;
    const long long base = (long long)blockIdx.y * H * W;
    for (int e = tid; e < CCL_T * CCL_T; e += SPX_THREADS) {
        const int y = Y0 + e / CCL_T, x = X0 + e % CCL_T;
        s_lab[e] = (y < H && x < W) ? labels[base + (long long)y * W + x] : -1;
        s_par[e] = e;
        s_cnt[e] = 0;
    }
    __syncthreads();
    for (int e = tid; e < CCL_T * CCL_T; e += SPX_THREADS) {
        const int l = s_lab[e];
        if (l < 0) continue;
        if (e % CCL_T > 0 && s_lab[e - 1] == l) lds_unite(s_par, e, e - 1);
        if (e >= CCL_T && s_lab[e - CCL_T] == l) lds_unite(s_par, e, e - CCL_T);
    }
    __syncthreads();
    int root[CCL_T * CCL_T / SPX_THREADS];
#pragma unroll
    for (int q = 0; q < CCL_T * CCL_T / SPX_THREADS; ++q) {
        const int e = tid + q * SPX_THREADS;
        root[q] = s_lab[e] < 0 ? -1 : lds_find(s_par, e);
        if (root[q] >= 0) atomicAdd(s_cnt + root[q], 1);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CCL_T * CCL_T / SPX_THREADS; ++q) {
        const int e = tid + q * SPX_THREADS, r = root[q];
        if (r < 0) continue;
        const long long p = base + (long long)(Y0 + e / CCL_T) * W + X0 + e % CCL_T;
        parent[p] = (Y0 + r / CCL_T) * W + X0 + r % CCL_T;
        area[p] = r == e ? s_cnt[e] : 0;
    }
}

// grid (tiles, N), 64 threads: the tile's left column against the column before it, its top row against the row above
__global__ void __launch_bounds__(64) ccl_merge_kernel(const int* __restrict__ labels, int* parent, int H, int W) {
    const int t = threadIdx.x;
    const int tx = (W + CCL_T - 1) / CCL_T;
    const int Y0 = (blockIdx.x / tx) * CCL_T, X0 = (blockIdx.x % tx) * CCL_T;
    const long long base = (long long)blockIdx.y * H * W;
    int y, x, q;
    if (t < CCL_T) {
        y = Y0 + t; x = X0;
        if (X0 == 0 || y >= H) return;
        q = y * W + x - 1;
    } else {
        y = Y0; x = X0 + t - CCL_T;
        if (Y0 == 0 || x >= W) return;
        q = (y - 1) * W + x;
    }
    const int p = y * W + x;
    if (labels[base + p] == labels[base + q]) glb_unite(parent + base, p, q);
}

// grid (ceil(HW / 256), N): parent[p] = its root; the area of every tile piece is added to its root's.  Concurrent
// readers of an entry being compressed see its old or its new value, both ancestors of the pixel.
__global__ void __launch_bounds__(SPX_THREADS) ccl_compress_kernel(int* parent, int* area, int HW) {
    const int p = blockIdx.x * SPX_THREADS + threadIdx.x;
    if (p >= HW) return;
    int* par = parent + (long long)blockIdx.y * HW;
    int* ar = area + (long long)blockIdx.y * HW;
    int r = par[p];
    for (int q = par[r]; q != r; q = par[r]) r = q;
    par[p] = r;
    const int a = ar[p];
    if (a > 0 && r != p) atomicAdd(ar + r, a);
}

__device__ __forceinline__ int block_exclusive_scan(int v, int* s, int& total) {
    const int tid = threadIdx.x;
    s[tid] = v;
    for (int o = 1; o < SPX_THREADS; o <<= 1) {
        __syncthreads();
        const int t = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += t;
    }
    __syncthreads();
    total = s[SPX_THREADS - 1];
    const int ex = s[tid] - v;
    __syncthreads();
    return ex;
}

// grid (ceil(HW / 1024), N): the kept roots (area >= min_area) of each 1024-pixel chunk, counted
__global__ void __launch_bounds__(SPX_THREADS) root_count_kernel(const int* __restrict__ parent, const int* __restrict__ area,
                                                                  int* __restrict__ chunk_cnt, int HW, int min_area) {
    __shared__ int s[SPX_THREADS];
    const long long base = (long long)blockIdx.y * HW;
    int c = 0;
    for (int e = 0; e < SCAN_CHUNK / SPX_THREADS; ++e) {
        const int p = blockIdx.x * SCAN_CHUNK + threadIdx.x * (SCAN_CHUNK / SPX_THREADS) + e;
        if (p < HW && parent[base + p] == p && area[base + p] >= min_area) ++c;
    }
    int total;
    block_exclusive_scan(c, s, total);
    if (threadIdx.x == 0) chunk_cnt[(long long)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// grid (N): chunk counts -> exclusive offsets in place, and the image's region count
__global__ void __launch_bounds__(SPX_THREADS) root_scan_kernel(int* __restrict__ chunk_cnt, int* __restrict__ count_out,
                                                                 int chunks) {
    __shared__ int s[SPX_THREADS];
    int* cc = chunk_cnt + (long long)blockIdx.x * chunks;
    int running = 0;
    for (int b0 = 0; b0 < chunks; b0 += SPX_THREADS) {
        const int i = b0 + threadIdx.x;
        const int v = i < chunks ? cc[i] : 0;
        int total;
        const int ex = block_exclusive_scan(v, s, total);
        if (i < chunks) cc[i] = running + ex;
        running += total;
    }
    if (threadIdx.x == 0) count_out[blockIdx.x] = running;
}

// grid (ceil(HW / 1024), N): regs[root] = its number 1..R in increasing root order, 0 for a dropped root
__global__ void __launch_bounds__(SPX_THREADS) root_number_kernel(const int* __restrict__ parent, const int* __restrict__ area,
                                                                   const int* __restrict__ chunk_off, int* __restrict__ regs,
                                                                   int HW, int min_area) {
    __shared__ int s[SPX_THREADS];
    constexpr int E = SCAN_CHUNK / SPX_THREADS;
    const long long base = (long long)blockIdx.y * HW;
    const int p0 = blockIdx.x * SCAN_CHUNK + threadIdx.x * E;
    bool isroot[E], kept[E];
    int c = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int p = p0 + e;
        isroot[e] = p < HW && parent[base + p] == p;
        kept[e] = isroot[e] && area[base + p] >= min_area;
        c += kept[e];
    }
    int total;
    int id = chunk_off[(long long)blockIdx.y * gridDim.x + blockIdx.x] + block_exclusive_scan(c, s, total);
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (isroot[e]) regs[base + p0 + e] = kept[e] ? ++id : 0;
}

// grid (ceil(HW / 256), N): every other pixel takes its root's number (root entries are not written here)
__global__ void __launch_bounds__(SPX_THREADS) region_write_kernel(const int* __restrict__ parent, int* regs, int HW) {
    const int p = blockIdx.x * SPX_THREADS + threadIdx.x;
    if (p >= HW) return;
    const long long base = (long long)blockIdx.y * HW;
    const int r = parent[base + p];
    if (r != p) regs[base + p] = regs[base + r];
}

// ---- edge_shrinking.  grid (tiles, N): the tile and a halo of `win` in LDS; s_h = "the row's window around this pixel
// holds one id", then the column test over s_h and the centre column's ids.  Pixels outside the image do not count.
__global__ void __launch_bounds__(SPX_THREADS) region_shrink_kernel(const int* __restrict__ regs, int* __restrict__ out, int H,
                                                                     int W, int win, int fill) {
    __shared__ int s_r[(SHR_T + 2 * SHR_MAX_WIN) * SHR_LD];
    __shared__ uint8_t s_h[(SHR_T + 2 * SHR_MAX_WIN) * SHR_T];
    const int tid = threadIdx.x;
    const int tx = (W + SHR_T - 1) / SHR_T;
    const int Y0 = (blockIdx.x / tx) * SHR_T, X0 = (blockIdx.x % tx) * SHR_T;
    const long long base = (long long)blockIdx.y * H * W;
    const int ext = SHR_T + 2 * win;
    for (int e = tid; e < ext * ext; e += SPX_THREADS) {
        const int rr = e / ext, cc = e - rr * ext;
        const int y = Y0 - win + rr, x = X0 - win + cc;
        if (y >= 0 && y < H && x >= 0 && x < W) s_r[rr * SHR_LD + cc] = regs[base + (long long)y * W + x];
    }
    __syncthreads();
    for (int e = tid; e < ext * SHR_T; e += SPX_THREADS) {
        const int rr = e / SHR_T, c = e - rr * SHR_T;
        const int y = Y0 - win + rr, x = X0 + c;
        bool ok = true;
        if (y >= 0 && y < H && x < W) {
            const int v = s_r[rr * SHR_LD + c + win];
            for (int dx = -win; dx <= win; ++dx) {
                const int xx = x + dx;
                if (xx >= 0 && xx < W && s_r[rr * SHR_LD + c + win + dx] != v) ok = false;
            }
        }
        s_h[e] = ok;
    }
    __syncthreads();
    for (int e = tid; e < SHR_T * SHR_T; e += SPX_THREADS) {
        const int a = e / SHR_T, b = e - a * SHR_T;
        const int y = Y0 + a, x = X0 + b;
        if (y >= H || x >= W) continue;
        const int v = s_r[(a + win) * SHR_LD + b + win];
        bool ok = true;
        for (int dy = -win; dy <= win; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            if (s_r[(a + win + dy) * SHR_LD + b + win] != v || !s_h[(a + win + dy) * SHR_T + b]) ok = false;
        }
        out[base + (long long)y * W + x] = ok ? v : fill;
    }
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// RGDA_OK when (N, H, W, S) is a shape the generator serves
int superpixel_shape(int N, int H, int W, int S) {
    if (N < 1 || H < 1 || W < 1) return RGDA_ERR_ARG;
    if (S < 4 || S > 64 || H > 16384 || W > 16384 || N > 65535) return RGDA_ERR_UNSUPPORTED;
    if (H % S || W % S) return RGDA_ERR_ARG;
    return RGDA_OK;
}

struct SpxLayout {
    size_t centres, sums, labels, parent, area, chunks, total;      // byte offsets
    int chunk_count;
};
SpxLayout superpixel_layout(int N, int H, int W, int S) {
    SpxLayout L;
    const size_t K = (size_t)(H / S) * (W / S), HW = (size_t)H * W;
    L.chunk_count = (int)((HW + SCAN_CHUNK - 1) / SCAN_CHUNK);
    L.centres = 0;
    L.sums = round16(L.centres + (size_t)2 * N * K * 5 * 4);
    L.labels = round16(L.sums + (size_t)3 * N * K * 6 * 4);
    L.parent = round16(L.labels + N * HW * 4);
    L.area = round16(L.parent + N * HW * 4);
    L.chunks = round16(L.area + N * HW * 4);
    L.total = round16(L.chunks + (size_t)N * L.chunk_count * 4);
    return L;
}

}  // namespace

extern "C" size_t rgda_superpixels_workspace(int N, int H, int W, int S) {
    if (superpixel_shape(N, H, W, S) != RGDA_OK) return 0;
    return superpixel_layout(N, H, W, S).total;
}

extern "C" int rgda_superpixels(const uint8_t* img, int N, int H, int W, int S, int m, int iters, int min_area,
                                int32_t* regs_out, int32_t* count_out, void* ws, size_t ws_bytes, rgda_stream_t stream) {
    if (!img || !regs_out || !count_out || !ws || iters < 1 || min_area < 1) return RGDA_ERR_ARG;
    const int shape = superpixel_shape(N, H, W, S);
    if (shape != RGDA_OK) return shape;
    if (m < 1 || m > 64) return RGDA_ERR_UNSUPPORTED;
    if (!aligned(img, 4) || !aligned(regs_out, 4) || !aligned(count_out, 4) || !aligned(ws, 16)) return RGDA_ERR_ARG;
    const SpxLayout L = superpixel_layout(N, H, W, S);
    if (ws_bytes < L.total) return RGDA_ERR_WORKSPACE;
    hipStream_t st = to_stream(stream);
    char* w8 = (char*)ws;
    const int Gy = H / S, Gx = W / S, HW = H * W;
    const size_t K = (size_t)Gy * Gx;
    int* ctr[2] = {(int*)(w8 + L.centres), (int*)(w8 + L.centres) + (size_t)N * K * 5};
    int* sums[3];
    for (int i = 0; i < 3; ++i) sums[i] = (int*)(w8 + L.sums) + (size_t)i * N * K * 6;
    int* labels = (int*)(w8 + L.labels);
    int* parent = (int*)(w8 + L.parent);
    int* area = (int*)(w8 + L.area);
    int* chunks = (int*)(w8 + L.chunks);
    // the centres (read where a centre has lost every pixel) and the three rotating sum buffers start at zero
    if (zero_bytes(w8 + L.centres, L.labels - L.centres, stream) != RGDA_OK) return RGDA_ERR_LAUNCH;

    const int bc = S >= SPX_TILE ? 1 : SPX_TILE / S;
    const dim3 gs((unsigned)(cdiv(Gy, bc) * cdiv(Gx, bc)), (unsigned)N);
    const long long img_bytes = (long long)N * HW * 3;
    slic_iter_kernel<SLIC_INIT><<<gs, SPX_THREADS, 0, st>>>(img, img_bytes, H, W, S, bc, Gy, Gx, m * m, nullptr, nullptr,
                                                            nullptr, sums[0], nullptr, nullptr);
    RGDA_CHECK_LAUNCH();
    // iteration it reads the sums of it - 1, adds into buffer it % 3 and clears buffer (it + 1) % 3, read one launch ago
    for (int it = 1; it <= iters; ++it) {
        const int* sin = sums[(it - 1) % 3];
        int *sout = sums[it % 3], *szero = sums[(it + 1) % 3];
        if (it < iters)
            slic_iter_kernel<SLIC_MID><<<gs, SPX_THREADS, 0, st>>>(img, img_bytes, H, W, S, bc, Gy, Gx, m * m, sin,
                                                                   ctr[(it - 1) & 1], ctr[it & 1], sout, szero, labels);
        else
            slic_iter_kernel<SLIC_LAST><<<gs, SPX_THREADS, 0, st>>>(img, img_bytes, H, W, S, bc, Gy, Gx, m * m, sin,
                                                                    ctr[(it - 1) & 1], ctr[it & 1], sout, szero, labels);
        RGDA_CHECK_LAUNCH();
    }
    const dim3 gt((unsigned)(cdiv(H, CCL_T) * cdiv(W, CCL_T)), (unsigned)N);
    const dim3 gp((unsigned)cdiv(HW, SPX_THREADS), (unsigned)N), gc((unsigned)L.chunk_count, (unsigned)N);
    ccl_local_kernel<<<gt, SPX_THREADS, 0, st>>>(labels, parent, area, H, W);
    RGDA_CHECK_LAUNCH();
    ccl_merge_kernel<<<gt, 64, 0, st>>>(labels, parent, H, W);
    RGDA_CHECK_LAUNCH();
    ccl_compress_kernel<<<gp, SPX_THREADS, 0, st>>>(parent, area, HW);
    RGDA_CHECK_LAUNCH();
    root_count_kernel<<<gc, SPX_THREADS, 0, st>>>(parent, area, chunks, HW, min_area);
    RGDA_CHECK_LAUNCH();
    root_scan_kernel<<<N, SPX_THREADS, 0, st>>>(chunks, count_out, L.chunk_count);
    RGDA_CHECK_LAUNCH();
    root_number_kernel<<<gc, SPX_THREADS, 0, st>>>(parent, area, chunks, regs_out, HW, min_area);
    RGDA_CHECK_LAUNCH();
    region_write_kernel<<<gp, SPX_THREADS, 0, st>>>(parent, regs_out, HW);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}

extern "C" int rgda_region_shrink(const int32_t* regs, int N, int H, int W, int win, int fill, int32_t* out,
                                  rgda_stream_t stream) {
    if (!regs || !out || regs == out || N < 1 || H < 1 || W < 1 || win < 0) return RGDA_ERR_ARG;
    if (win > SHR_MAX_WIN || N > 65535 || H > 16384 || W > 16384) return RGDA_ERR_UNSUPPORTED;
    if (!aligned(regs, 4) || !aligned(out, 4)) return RGDA_ERR_ARG;
    const dim3 g((unsigned)(cdiv(H, SHR_T) * cdiv(W, SHR_T)), (unsigned)N);
    region_shrink_kernel<<<g, SPX_THREADS, 0, to_stream(stream)>>>(regs, out, H, W, win, fill);
    RGDA_CHECK_LAUNCH();
    return RGDA_OK;
}
