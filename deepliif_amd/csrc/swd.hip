// swd.hip -- the sliced Wasserstein distance of two image sets (the reference's DeepLIIF_Statistics/swd.py) on the GPU, in three stages that are
// each an entry of their own:
//   dl_swd_patches    Gaussian pyramid of a chunk of uint8 images (5 x 5 binomial kernel, stride 2, zero padding) and the RAW 7 x 7 x 3 patches of
//                     every Laplacian level at the chosen positions.  Only the chosen patches are evaluated: no Laplacian image, no up-sampled
//                     image and no unfolded window tensor is ever stored;
//   dl_swd_normalise  per-channel mean and unbiased std of one set's patch matrix [R][147], and (x - mean) / (std + 1e-8) in place;
//   dl_swd_distance   per projection direction p: mean |sort(A p) - sort(B p)|.  One pass projects both sets onto 32 directions per workgroup;
//                     up to dl_swd_lds_rows() rows a workgroup per direction then sorts both projections in LDS (bitonic network), above
//                     that hipcub's segmented radix sort does.  (Projecting straight into the sorting workgroup's LDS was measured first: it
//                     reads both sets once per direction, 10 GB of cache traffic per level at 8192 rows x 512 directions, and took 10.2 ms
//                     for six levels where this takes the time profiles/swd.json holds.)
// Everything is double, summed in a fixed order, without floating-point atomics: two calls give the same bits.  Format-independent: the same
// object code in both libraries.
#include "common.h"
#include <hipcub/hipcub.hpp>
#include <math.h>

// unfused, like stat.hip: the float64 yardstick of the tests is unfused too
#pragma clang fp contract(off)

#define SW_P 7                       // patch side (swd.py hard-codes the 6 = SW_P - 1 and the 3 * 7 * 7)
#define SW_K (3 * SW_P * SW_P)       // 147 columns of the descriptor matrix: channel, dy, dx
#define SW_MAX_PYR 15
#define SW_DT 16                     // pyramid_down: 16 x 16 outputs per workgroup ...
#define SW_DS (2 * SW_DT + 3)        // ... from a staged 35 x 35 input tile (tile + halo)
#define SW_UP (SW_P + 4)             // up-sampled rows / columns under one patch and its 5 x 5 halo: 11
#define SW_LDS_ROWS 8192             // two sets of 8-byte values, padded to a power of two: 2 x 8192 x 8 = 128 KiB of the CU's 160 KiB
#define SW_SORT_THREADS 1024
#define SW_LARGE_ELEMS ((long long)1 << 22)   // large route: projections of one set held in global memory per pass (32 MiB)

static size_t sw_align(size_t v) { return (v + 255) & ~(size_t)255; }

// [1 4 6 4 1] / 16: the 5 x 5 kernel of swd.py:9-14 is its outer product (exact in binary)
__device__ __forceinline__ double sw_tap(int k) { return k == 2 ? 0.375 : ((k == 1 || k == 3) ? 0.25 : 0.0625); }

// one pyramid level: the uint8 images themselves (level 0: v / 255, HWC with byte strides) or planar doubles [N][3][h][w]
struct SwLevel { const uint8_t *u8; size_t rs, is; const double *f; int h, w; };

__device__ __forceinline__ double sw_load(const SwLevel &s, int n, int c, int y, int x) {        // zero padding
    if ((unsigned)y >= (unsigned)s.h || (unsigned)x >= (unsigned)s.w) return 0.0;
    if (s.u8) return (double)s.u8[(size_t)n * s.is + (size_t)y * s.rs + (size_t)x * 3 + c] / 255.0;
    return s.f[(((size_t)n * 3 + c) * s.h + y) * s.w + x];
}

// fixed-order sum of one value per thread over the T threads of the workgroup (T a power of two; result in every thread)
template <int T>
__device__ __forceinline__ double sw_block_sum(double v, double *red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = T / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// ---------------------------------------------------------------------------------------------------- pyramid_down
// dst[n][c][oy][ox] = sum_ij k_i k_j src(2 oy - 2 + i, 2 ox - 2 + j), rows first; blockIdx.z = n * 3 + c.  LDS: 35 x 35 + 35 x 16 doubles = 14 280 bytes
__global__ void __launch_bounds__(256) sw_down_kernel(SwLevel src, double *dst, int ho, int wo) {
    __shared__ double tile[SW_DS][SW_DS];
    __shared__ double rowf[SW_DS][SW_DT];
    const int tid = threadIdx.x, n = blockIdx.z / 3, c = blockIdx.z - n * 3;
    const int oy0 = blockIdx.y * SW_DT, ox0 = blockIdx.x * SW_DT;
    for (int i = tid; i < SW_DS * SW_DS; i += 256) {
        const int ly = i / SW_DS, lx = i - ly * SW_DS;
        tile[ly][lx] = sw_load(src, n, c, 2 * oy0 - 2 + ly, 2 * ox0 - 2 + lx);
    }
    __syncthreads();
    for (int i = tid; i < SW_DS * SW_DT; i += 256) {
        const int ly = i / SW_DT, ox = i - ly * SW_DT;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 5; ++k) s += sw_tap(k) * tile[ly][2 * ox + k];
        rowf[ly][ox] = s;
    }
    __syncthreads();
    const int oy = tid / SW_DT, ox = tid - oy * SW_DT;
    if (oy0 + oy < ho && ox0 + ox < wo) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 5; ++k) s += sw_tap(k) * rowf[2 * oy + k][ox];
        dst[(((size_t)n * 3 + c) * ho + (oy0 + oy)) * wo + (ox0 + ox)] = s;
    }
}

// ---------------------------------------------------------------------------------------------------- Laplacian patches
// one workgroup per (descriptor, image): the patch of cur minus conv5x5(nearest_upsample_x2(next)) over the patch, both zero-padded at the
// level's border; `next` == nullptr: the last level, the Gaussian level itself.  The 11 x 11 up-sampled pixels under the patch and its halo
// are staged in LDS and filtered rows first.  out row = row0 + n * D + d (image-major, then descriptor), columns channel, dy, dx.
__global__ void __launch_bounds__(128) sw_patch_kernel(SwLevel cur, const double *next, int h2, int w2, const int *idx, int D, size_t row0, double *out) {
    __shared__ double up[3][SW_UP][SW_UP];
    __shared__ double rowf[3][SW_UP][SW_P];
    const int tid = threadIdx.x, d = blockIdx.x, n = blockIdx.y;
    double *o = out + (row0 + (size_t)n * D + d) * SW_K;
    const int wp = cur.w - (SW_P - 1), hp = cur.h - (SW_P - 1);
    const int i = idx[d];
    if (i < 0 || i >= hp * wp) {                       // an index outside the level: refuse to read there
        for (int e = tid; e < SW_K; e += 128) o[e] = NAN;
        return;
    }
    const int py = i / wp, px = i - py * wp;           // swd.py:81-85: the windows are unfolded rows first
    if (next) {
        for (int e = tid; e < 3 * SW_UP * SW_UP; e += 128) {
            const int c = e / (SW_UP * SW_UP), r = (e / SW_UP) % SW_UP, q = e % SW_UP;
            const int y = py - 2 + r, x = px - 2 + q;
            double v = 0.0;
            if ((unsigned)y < (unsigned)cur.h && (unsigned)x < (unsigned)cur.w && (y >> 1) < h2 && (x >> 1) < w2)
                v = next[(((size_t)n * 3 + c) * h2 + (y >> 1)) * w2 + (x >> 1)];
            up[c][r][q] = v;
        }
        __syncthreads();
        for (int e = tid; e < 3 * SW_UP * SW_P; e += 128) {
            const int c = e / (SW_UP * SW_P), r = (e / SW_P) % SW_UP, q = e % SW_P;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 5; ++k) s += sw_tap(k) * up[c][r][q + k];
            rowf[c][r][q] = s;
        }
        __syncthreads();
    }
    for (int e = tid; e < SW_K; e += 128) {
        const int c = e / (SW_P * SW_P), dy = (e / SW_P) % SW_P, dx = e % SW_P;
        double v = sw_load(cur, n, c, py + dy, px + dx);
        if (next) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 5; ++k) s += sw_tap(k) * rowf[c][dy + k][dx];
            v -= s;
        }
        o[e] = v;
    }
}

struct SwShapes { int n, h[SW_MAX_PYR + 1], w[SW_MAX_PYR + 1]; size_t off[SW_MAX_PYR + 2]; };   // off: bytes of level l >= 1 in the workspace

static int sw_shapes(int N, int H, int W, int n_pyramids, SwShapes *s) {
    if (N <= 0 || N > 65535 / 3 || H <= 0 || W <= 0 || n_pyramids < 0 || n_pyramids > SW_MAX_PYR) return -1;
    if ((size_t)H * W >= ((size_t)1 << 31)) return -1;
    if ((H & ((1 << n_pyramids) - 1)) || (W & ((1 << n_pyramids) - 1))) return -2;
    if ((H >> n_pyramids) < SW_P || (W >> n_pyramids) < SW_P) return -3;
    s->n = n_pyramids;
    size_t off = 0;
    for (int l = 0; l <= n_pyramids; ++l) {
        s->h[l] = H >> l;
        s->w[l] = W >> l;                 // = floor((h - 1) / 2) + 1 of the level above, which is even
        s->off[l] = off;
        if (l > 0) off += sw_align((size_t)N * 3 * s->h[l] * s->w[l] * sizeof(double));
    }
    s->off[n_pyramids + 1] = off;
    return 0;
}

extern "C" size_t dl_swd_patches_ws_bytes(int N, int H, int W, int n_pyramids) {
    SwShapes s;
    if (sw_shapes(N, H, W, n_pyramids, &s)) return 0;
    return s.off[n_pyramids + 1] + 256;
}

extern "C" int dl_swd_patches(const void *images, size_t row_stride, size_t image_stride, int N, int H, int W, int n_pyramids, const int *indices,
                              const int *counts, long long n_total, long long n0, void *ws, double *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!images || !indices || !counts || !ws || !out) DL_FAIL("dl_swd_patches: null argument");
    SwShapes s;
    const int rc = sw_shapes(N, H, W, n_pyramids, &s);
    if (rc == -2) DL_FAIL("dl_swd_patches: H=%d W=%d are not divisible by 2^n_pyramids = %d", H, W, 1 << n_pyramids);
    if (rc == -3) DL_FAIL("dl_swd_patches: the smallest level, %d x %d, is below the 7 x 7 patch", H >> n_pyramids, W >> n_pyramids);
    if (rc) DL_FAIL("dl_swd_patches: empty problem or too large (N=%d H=%d W=%d n_pyramids=%d; at most 21845 images per call)", N, H, W, n_pyramids);
    if (row_stride < (size_t)W * 3) DL_FAIL("dl_swd_patches: the row stride is shorter than a row");
    if (n0 < 0 || n_total <= 0 || n0 + N > n_total) DL_FAIL("dl_swd_patches: images %lld .. %lld of %lld", n0, n0 + N, n_total);
    for (int l = 0; l <= n_pyramids; ++l) {
        const long long positions = (long long)(s.h[l] - (SW_P - 1)) * (s.w[l] - (SW_P - 1));
        if (counts[l] <= 0 || counts[l] > positions || counts[l] > 65535)
            DL_FAIL("dl_swd_patches: %d descriptors at level %d, which has %lld positions (at most 65535)", counts[l], l, positions);
    }
    char *w = (char *)ws;
    SwLevel lev[SW_MAX_PYR + 1];
    lev[0] = SwLevel{(const uint8_t *)images, row_stride, image_stride, nullptr, H, W};
    for (int l = 1; l <= n_pyramids; ++l) {
        double *dst = (double *)(w + s.off[l]);
        const dim3 grid((s.w[l] + SW_DT - 1) / SW_DT, (s.h[l] + SW_DT - 1) / SW_DT, N * 3);
        hipLaunchKernelGGL(sw_down_kernel, grid, dim3(256), 0, stream, lev[l - 1], dst, s.h[l], s.w[l]);
        lev[l] = SwLevel{nullptr, 0, 0, dst, s.h[l], s.w[l]};
    }
    size_t rows_before = 0, idx_before = 0;
    for (int l = 0; l <= n_pyramids; ++l) {
        const int D = counts[l];
        const bool last = l == n_pyramids;
        hipLaunchKernelGGL(sw_patch_kernel, dim3(D, N), dim3(128), 0, stream, lev[l], last ? (const double *)nullptr : lev[l + 1].f, last ? 0 : s.h[l + 1],
                           last ? 0 : s.w[l + 1], indices + idx_before, D, rows_before + (size_t)n0 * D, out);
        rows_before += (size_t)n_total * D;
        idx_before += D;
    }
    DL_CHECK_LAUNCH("dl_swd_patches");
    return 0;
}

// ---------------------------------------------------------------------------------------------------- statistics + normalisation
// PASS 0: partial[block][c] = sum of x over the block's rows; PASS 1: sum of (x - mean[c])^2.  Thread t takes the elements t, t + 256, ... of
// the block's rows of one channel, then the fixed tree.
template <int PASS>
__global__ void __launch_bounds__(256) sw_moment_kernel(const double *x, long long R, long long rows_per_block, const double *stats, double *partial) {
    __shared__ double red[256];
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long rows = (R - r0 < rows_per_block) ? R - r0 : rows_per_block;
    for (int c = 0; c < 3; ++c) {
        const double mean = PASS ? stats[c] : 0.0;
        double s = 0.0;
        for (long long e = threadIdx.x; e < rows * (SW_P * SW_P); e += 256) {
            const long long r = e / (SW_P * SW_P);
            const int q = (int)(e - r * (SW_P * SW_P));
            const double v = x[(size_t)(r0 + r) * SW_K + c * (SW_P * SW_P) + q];
            s += PASS ? (v - mean) * (v - mean) : v;
        }
        s = sw_block_sum<256>(s, red);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * 3 + c] = s;
    }
}

// one workgroup: the partial sums in index order -> stats[c] = mean (PASS 0), stats[3 + c] = unbiased std (PASS 1)
template <int PASS>
__global__ void __launch_bounds__(256) sw_moment_final_kernel(const double *partial, int blocks, double count, double *stats) {
    __shared__ double red[256];
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int b = threadIdx.x; b < blocks; b += 256) s += partial[(size_t)b * 3 + c];
        s = sw_block_sum<256>(s, red);
        if (threadIdx.x == 0) stats[PASS * 3 + c] = PASS ? sqrt(s / (count - 1.0)) : s / count;
    }
}

__global__ void __launch_bounds__(256) sw_normalise_kernel(double *x, size_t total, const double *stats) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % SW_K) / (SW_P * SW_P);
    x[i] = (x[i] - stats[c]) / (stats[3 + c] + 1e-8);            // swd.py:92
}

#define SW_MOMENT_BLOCKS 1024
static bool sw_bad_rows(long long R) { return R <= 0 || R > ((long long)1 << 30); }

extern "C" size_t dl_swd_normalise_ws_bytes(long long R) {
    if (sw_bad_rows(R)) return 0;
    return sw_align((size_t)SW_MOMENT_BLOCKS * 3 * sizeof(double));
}

extern "C" int dl_swd_normalise(double *x, long long R, void *ws, double *stats, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!x || !ws || !stats) DL_FAIL("dl_swd_normalise: null argument");
    if (sw_bad_rows(R)) DL_FAIL("dl_swd_normalise: empty problem or too large (R=%lld)", R);
    long long blocks = (R + 63) / 64;
    if (blocks > SW_MOMENT_BLOCKS) blocks = SW_MOMENT_BLOCKS;
    const long long rpb = (R + blocks - 1) / blocks;
    blocks = (R + rpb - 1) / rpb;
    double *partial = (double *)ws;
    const double count = (double)R * (SW_P * SW_P);
    hipLaunchKernelGGL(sw_moment_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, stream, (const double *)x, R, rpb, (const double *)stats, partial);
    hipLaunchKernelGGL(sw_moment_final_kernel<0>, dim3(1), dim3(256), 0, stream, (const double *)partial, (int)blocks, count, stats);
    hipLaunchKernelGGL(sw_moment_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, stream, (const double *)x, R, rpb, (const double *)stats, partial);
    hipLaunchKernelGGL(sw_moment_final_kernel<1>, dim3(1), dim3(256), 0, stream, (const double *)partial, (int)blocks, count, stats);
    const size_t total = (size_t)R * SW_K;
    hipLaunchKernelGGL(sw_normalise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, total, (const double *)stats);
    DL_CHECK_LAUNCH("dl_swd_normalise");
    return 0;
}

// ---------------------------------------------------------------------------------------------------- project, sort, reduce
// Projections: keys [2 * pc][R]; segment c holds A p_(col0 + c), segment pc + c holds B p_(col0 + c).  A workgroup takes 64 rows and a tile of
// SW_PT directions (staged in LDS as doubles, zero-padded to 160); a row's 147 values are loaded ONCE, 10 per lane of a 16-lane group, and serve
// the whole tile, so each set is read P / SW_PT times per level, not P times.  Lane j adds the products j, j + 16, ... in that order, then the xor
// tree 8, 4, 2, 1: a fixed order.  Every lane of a wavefront runs the same trips (the shuffles are not divergent).
#define SW_PT 32
#define SW_PROWS 64
__global__ void __launch_bounds__(256) sw_project_kernel(const double *a, const double *b, long long R, const float *proj, int col0, int pc, double *keys) {
    __shared__ double pv[SW_PT][160];                    // 40 960 bytes
    const int tid = threadIdx.x, c0 = blockIdx.y * SW_PT;
    const int nc = pc - c0 < SW_PT ? pc - c0 : SW_PT;
    for (int e = tid; e < SW_PT * 160; e += 256) {
        const int c = e / 160, k = e - c * 160;
        pv[c][k] = (c < nc && k < SW_K) ? (double)proj[(size_t)(col0 + c0 + c) * SW_K + k] : 0.0;
    }
    __syncthreads();
    const int g = tid >> 4, j = tid & 15;
    for (int q = 0; q < SW_PROWS / 16; ++q) {
        const long long r = (long long)blockIdx.x * SW_PROWS + q * 16 + g;
        const bool valid = r < R;
        for (int set = 0; set < 2; ++set) {
            const double *row = (set ? b : a) + (size_t)(valid ? r : 0) * SW_K;
            double x[10];
#pragma unroll
            for (int i = 0; i < 10; ++i) x[i] = (valid && j + 16 * i < SW_K) ? row[j + 16 * i] : 0.0;
            for (int c = 0; c < nc; ++c) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < 10; ++i) s += x[i] * pv[c][j + 16 * i];
                for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                if (j == 0 && valid) keys[((size_t)set * pc + c0 + c) * R + r] = s;
            }
        }
    }
}

// LDS route: one workgroup per direction takes both sets' projections into LDS, padded to a power of two Rp (>= 64) with +inf, which the
// ascending bitonic network leaves behind the R values; then mean |a - b| in a fixed tree.  Dynamic LDS: sa[Rp] sb[Rp] red[1024].
__global__ void __launch_bounds__(SW_SORT_THREADS) sw_sort_lds_kernel(const double *keys, int R, int Rp, int pc, double *out) {
    extern __shared__ __attribute__((aligned(16))) char sw_smem[];
    double *sa = (double *)sw_smem, *sb = sa + Rp, *red = sb + Rp;
    const int tid = threadIdx.x, col = blockIdx.x;
    const double *ka = keys + (size_t)col * R, *kb = keys + (size_t)(pc + col) * R;
    for (int r = tid; r < Rp; r += SW_SORT_THREADS) {
        sa[r] = r < R ? ka[r] : INFINITY;
        sb[r] = r < R ? kb[r] : INFINITY;
    }
    __syncthreads();
    for (int k = 2; k <= Rp; k <<= 1) {
        for (int s = k >> 1; s > 0; s >>= 1) {
            for (int t = tid; t < (Rp >> 1); t += SW_SORT_THREADS) {
                const int lo = t & (s - 1), i = ((t - lo) << 1) + lo, p = i + s;
                const bool up = (i & k) == 0;
                const double x0 = sa[i], x1 = sa[p];
                if ((x0 > x1) == up) { sa[i] = x1; sa[p] = x0; }
                const double y0 = sb[i], y1 = sb[p];
                if ((y0 > y1) == up) { sb[i] = y1; sb[p] = y0; }
            }
            __syncthreads();
        }
    }
    double s = 0.0;
    for (int i = tid; i < R; i += SW_SORT_THREADS) s += fabs(sa[i] - sb[i]);
    s = sw_block_sum<SW_SORT_THREADS>(s, red);
    if (tid == 0) out[col] = s / (double)R;
}

__global__ void __launch_bounds__(256) sw_offsets_kernel(int *off, int n, int R) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i <= n) off[i] = i * R;
}

__global__ void __launch_bounds__(256) sw_reduce_kernel(const double *sorted, long long R, int pc, double *out) {
    __shared__ double red[256];
    const int c = blockIdx.x;
    const double *sa = sorted + (size_t)c * R, *sb = sorted + (size_t)(pc + c) * R;
    double s = 0.0;
    for (long long i = threadIdx.x; i < R; i += 256) s += fabs(sa[i] - sb[i]);
    s = sw_block_sum<256>(s, red);
    if (threadIdx.x == 0) out[c] = s / (double)R;
}

extern "C" int dl_swd_lds_rows(void) { return SW_LDS_ROWS; }

// 1 = LDS, 2 = large, 0 = refused
extern "C" int dl_swd_route(long long R, int P, int route) {
    if (sw_bad_rows(R) || P <= 0 || P > 65535 || route < 0 || route > 2) return 0;
    if (route == 1) return R <= SW_LDS_ROWS ? 1 : 0;
    if (route == 2) return 2;
    return R <= SW_LDS_ROWS ? 1 : 2;
}

// workspace: keys (both routes)  |  large route only: sorted keys, segment offsets (int32 [2 pc + 1]), hipcub's temp
struct SwLayout { int pc; size_t keys, sorted, off, temp, temp_bytes, total; };
static int sw_layout(long long R, int P, int rt, SwLayout *l) {
    long long pc = SW_LARGE_ELEMS / R;                  // directions per pass
    if (pc < 1) pc = 1;
    if (pc > P) pc = P;
    l->pc = (int)pc;
    const size_t items = (size_t)2 * pc * R;            // < 2^31: pc * R <= 2^22, or pc == 1 and R <= 2^30
    if (items >= ((size_t)1 << 31)) return -1;
    size_t off = 0;
    l->keys = off; off += sw_align(items * sizeof(double));
    l->sorted = l->off = l->temp = off; l->temp_bytes = 0;
    if (rt == 2) {
        l->sorted = off; off += sw_align(items * sizeof(double));
        l->off = off; off += sw_align(((size_t)2 * pc + 1) * sizeof(int));
        size_t tb = 0;
        if (hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, tb, (const double *)nullptr, (double *)nullptr, (int)items, (int)(2 * pc), (const int *)nullptr,
                                                       (const int *)nullptr, 0, 64) != hipSuccess) return -1;
        l->temp = off; l->temp_bytes = tb; off += sw_align(tb);
    }
    l->total = off;
    return 0;
}

extern "C" size_t dl_swd_distance_ws_bytes(long long R, int P, int route) {
    const int rt = dl_swd_route(R, P, route);
    SwLayout l;
    if (rt == 0 || sw_layout(R, P, rt, &l)) return 0;
    return l.total;
}

extern "C" int dl_swd_distance(const double *a, const double *b, long long R, const float *proj, int P, int route, void *ws, double *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!a || !b || !proj || !ws || !out) DL_FAIL("dl_swd_distance: null argument");
    if (sw_bad_rows(R) || P <= 0 || P > 65535) DL_FAIL("dl_swd_distance: empty problem or too large (R=%lld P=%d)", R, P);
    if (route < 0 || route > 2) DL_FAIL("dl_swd_distance: route=%d (0 = by size, 1 = LDS, 2 = large)", route);
    const int rt = dl_swd_route(R, P, route);
    if (rt == 0) DL_FAIL("dl_swd_distance: the LDS route holds at most %d rows, got R=%lld", SW_LDS_ROWS, R);
    SwLayout l;
    if (sw_layout(R, P, rt, &l)) DL_FAIL("dl_swd_distance: workspace query failed (R=%lld)", R);
    char *w = (char *)ws;
    double *keys = (double *)(w + l.keys), *sorted = (double *)(w + l.sorted);
    int *off = (int *)(w + l.off);
    int Rp = 64;
    size_t lds = 0;
    if (rt == 1) {
        while (Rp < R) Rp <<= 1;
        lds = ((size_t)2 * Rp + SW_SORT_THREADS) * sizeof(double);                          // at most 139 264 bytes
        // above 64 KiB the dynamic LDS of a kernel has to be granted (per device; the size varies with R: a smaller one after a larger asks nothing)
        if (lds > (size_t)64 << 10 && dl_lds_limit(reinterpret_cast<const void *>(sw_sort_lds_kernel), lds, "dl_swd_distance")) return -1;
    } else {
        hipLaunchKernelGGL(sw_offsets_kernel, dim3((2 * l.pc + 256) / 256), dim3(256), 0, stream, off, 2 * l.pc, (int)R);
    }
    for (int col0 = 0; col0 < P; col0 += l.pc) {
        const int pc = P - col0 < l.pc ? P - col0 : l.pc;       // the last pass may hold fewer directions: segments [0, 2 pc) of the same offsets
        const dim3 grid((unsigned)((R + SW_PROWS - 1) / SW_PROWS), (pc + SW_PT - 1) / SW_PT);
        hipLaunchKernelGGL(sw_project_kernel, grid, dim3(256), 0, stream, a, b, R, proj, col0, pc, keys);
        if (rt == 1) {
            hipLaunchKernelGGL(sw_sort_lds_kernel, dim3(pc), dim3(SW_SORT_THREADS), lds, stream, (const double *)keys, (int)R, Rp, pc, out + col0);
            continue;
        }
        size_t tb = l.temp_bytes;
        if (hipcub::DeviceSegmentedRadixSort::SortKeys(w + l.temp, tb, (const double *)keys, sorted, (int)((size_t)2 * pc * R), 2 * pc, (const int *)off,
                                                       (const int *)off + 1, 0, 64, stream) != hipSuccess) DL_FAIL("dl_swd_distance: sort failed");
        hipLaunchKernelGGL(sw_reduce_kernel, dim3(pc), dim3(256), 0, stream, (const double *)sorted, R, pc, out + col0);
    }
    DL_CHECK_LAUNCH("dl_swd_distance");
    return 0;
}
