// stat.hip -- the evaluation metrics of the reference's DeepLIIF_Statistics scripts (ComputeStatistics.py, Segmentation_Metrics.py) on the GPU:
//   dl_stat_similarity  MSE and Gaussian-weighted SSIM of uint8 image pairs (skimage's rgb2gray + structural_similarity), in double;
//   dl_stat_confusion   TP / FP / FN / TN of the positive (channel 0) and negative (channel 2) masks (compute_metrics_gpu's counts);
//   dl_stat_label       skimage.measure.label(plane, background=0): 8-connected components of EQUAL value, numbered in raster order of their
//                       first pixel -- the union-find of postproc.hip (unionfind.h), whose roots are smallest pixel indices;
//   dl_stat_aji         compute_aji's three sums from two label images: one key sort, a run-length encode and a greedy pass of one wavefront.
// Byte- and latency-bound work.  Everything is deterministic: integer atomics only, floating-point sums in a fixed order (per-workgroup
// partial sums in a workspace, added by one workgroup in index order).  Format-independent: the same object code in both libraries.
#include "common.h"
#include "unionfind.h"
#include <hipcub/hipcub.hpp>
#include <math.h>

// no fused multiply-add anywhere in this file: SSIM of an image with itself must be exactly 1 (numerator and denominator of S are then the
// same products and sums, and stay bit-equal only if neither side is contracted differently), and the float64 yardstick is unfused too
#pragma clang fp contract(off)

typedef unsigned long long u64;

static size_t st_align(size_t v) { return (v + 255) & ~(size_t)255; }
static bool st_bad_image(int H, int W) { return H <= 0 || W <= 0 || (size_t)H * W >= ((size_t)1 << 31); }

// ---------------------------------------------------------------------------------------------------- MSE + SSIM
#define ST_R 5                      // int(3.5 * 1.5 + 0.5): the radius of scipy's gaussian_filter at sigma 1.5, truncate 3.5
#define ST_TAPS (2 * ST_R + 1)
#define ST_TH 16                    // output tile of one workgroup: 16 rows x 32 columns (two pixels per thread)
#define ST_TW 32
#define ST_SH (ST_TH + 2 * ST_R)    // staged tile + halo: 26 x 42
#define ST_SW (ST_TW + 2 * ST_R)

struct StTaps { double w[ST_TAPS]; };

__device__ __forceinline__ double st_gray(const uint8_t *q, int channels) {
    if (channels == 1) return (double)q[0] / 255.0;
    // rgb2gray after img_as_float: the dot product of (r, g, b) / 255 with (0.2125, 0.7154, 0.0721), summed left to right
    return (0.2125 * ((double)q[0] / 255.0) + 0.7154 * ((double)q[1] / 255.0)) + 0.0721 * ((double)q[2] / 255.0);
}

// fixed-order sum of one value per thread over the 256 threads of the workgroup (result in every thread)
__device__ __forceinline__ double st_block_sum(double v, double *red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// LDS: 2 x 26 x 42 gray values + 5 x 26 x 32 row-filtered maps, all double = 50 752 bytes (two workgroups per CU)
__global__ void __launch_bounds__(256) st_similarity_kernel(const uint8_t *a, size_t a_rs, size_t a_is, const uint8_t *b, size_t b_rs, size_t b_is,
                                                            int channels, int H, int W, StTaps taps, double C1, double C2, double *partial) {
    __shared__ double ga[ST_SH][ST_SW], gb[ST_SH][ST_SW];
    __shared__ double hm[5][ST_SH][ST_TW];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int ty0 = blockIdx.y * ST_TH, tx0 = blockIdx.x * ST_TW;
    const uint8_t *ia = a + (size_t)n * a_is, *ib = b + (size_t)n * b_is;
    for (int i = tid; i < ST_SH * ST_SW; i += 256) {
        const int ly = i / ST_SW, lx = i - ly * ST_SW;
        const int gy = ty0 - ST_R + ly, gx = tx0 - ST_R + lx;
        double va = 0.0, vb = 0.0;          // outside the image: never part of an interior pixel's window, nor of the MSE
        if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
            va = st_gray(ia + (size_t)gy * a_rs + (size_t)gx * channels, channels);
            vb = st_gray(ib + (size_t)gy * b_rs + (size_t)gx * channels, channels);
        }
        ga[ly][lx] = va;
        gb[ly][lx] = vb;
    }
    __syncthreads();
    // rows: x, y, x^2, y^2, xy filtered along the row, for the tile's columns and all staged rows
    for (int i = tid; i < ST_SH * ST_TW; i += 256) {
        const int ly = i / ST_TW, lx = i - ly * ST_TW;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int k = 0; k < ST_TAPS; ++k) {
            const double x = ga[ly][lx + k], y = gb[ly][lx + k], w = taps.w[k];
            sx += w * x; sy += w * y; sxx += w * (x * x); syy += w * (y * y); sxy += w * (x * y);
        }
        hm[0][ly][lx] = sx; hm[1][ly][lx] = sy; hm[2][ly][lx] = sxx; hm[3][ly][lx] = syy; hm[4][ly][lx] = sxy;
    }
    __syncthreads();
    double ssim = 0.0, mse = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = tid + j * 256;
        const int oy = i / ST_TW, ox = i - oy * ST_TW;
        const int gy = ty0 + oy, gx = tx0 + ox;
        if (gy < H && gx < W) {
            const double d = ga[oy + ST_R][ox + ST_R] - gb[oy + ST_R][ox + ST_R];
            mse += d * d;
            if (gy >= ST_R && gy < H - ST_R && gx >= ST_R && gx < W - ST_R) {
                double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
#pragma unroll
                for (int k = 0; k < ST_TAPS; ++k) {
                    const double w = taps.w[k];
                    ux += w * hm[0][oy + k][ox]; uy += w * hm[1][oy + k][ox];
                    uxx += w * hm[2][oy + k][ox]; uyy += w * hm[3][oy + k][ox]; uxy += w * hm[4][oy + k][ox];
                }
                const double vx = uxx - ux * ux, vy = uyy - uy * uy, vxy = uxy - ux * uy;
                const double A1 = 2.0 * (ux * uy) + C1, A2 = 2.0 * vxy + C2;
                const double B1 = (ux * ux + uy * uy) + C1, B2 = (vx + vy) + C2;
                ssim += (A1 * A2) / (B1 * B2);
            }
        }
    }
    double *red = &hm[0][0][0];
    const double s1 = st_block_sum(mse, red);
    const double s2 = st_block_sum(ssim, red);
    if (tid == 0) {
        double *o = partial + ((size_t)n * gridDim.y * gridDim.x + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        o[0] = s1;
        o[1] = s2;
    }
}

// one workgroup per image: thread t adds tiles t, t + 256, ... in that order, then the fixed tree
__global__ void __launch_bounds__(256) st_similarity_final_kernel(const double *partial, int tiles, double n_all, double n_interior, double *out) {
    __shared__ double red[256];
    const double *p = partial + (size_t)blockIdx.x * tiles * 2;
    double mse = 0.0, ssim = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 256) { mse += p[(size_t)t * 2]; ssim += p[(size_t)t * 2 + 1]; }
    const double s1 = st_block_sum(mse, red);
    const double s2 = st_block_sum(ssim, red);
    if (threadIdx.x == 0) {
        out[(size_t)blockIdx.x * 2] = s1 / n_all;
        out[(size_t)blockIdx.x * 2 + 1] = s2 / n_interior;
    }
}

static int st_tiles(int H, int W) { return ((H + ST_TH - 1) / ST_TH) * ((W + ST_TW - 1) / ST_TW); }

extern "C" size_t dl_stat_similarity_ws_bytes(int N, int H, int W) {
    if (N <= 0 || N > 65535 || st_bad_image(H, W)) return 0;
    return st_align((size_t)N * st_tiles(H, W) * 2 * sizeof(double));
}

extern "C" int dl_stat_similarity(const void *a, size_t a_row_stride, size_t a_image_stride, const void *b, size_t b_row_stride, size_t b_image_stride,
                                  int channels, int N, int H, int W, double data_range, void *ws, double *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!a || !b || !ws || !out) DL_FAIL("dl_stat_similarity: null argument");
    if (N <= 0 || N > 65535 || st_bad_image(H, W)) DL_FAIL("dl_stat_similarity: empty problem or too large (N=%d H=%d W=%d)", N, H, W);
    if (H < ST_TAPS || W < ST_TAPS) DL_FAIL("dl_stat_similarity: the 11 x 11 Gaussian window needs H, W >= 11 (H=%d W=%d)", H, W);
    if (channels != 1 && channels != 3) DL_FAIL("dl_stat_similarity: channels=%d (1 = gray, 3 = RGB)", channels);
    if (a_row_stride < (size_t)W * channels || b_row_stride < (size_t)W * channels) DL_FAIL("dl_stat_similarity: a row stride is shorter than a row");
    if (!(data_range > 0.0)) DL_FAIL("dl_stat_similarity: data_range=%g", data_range);
    StTaps taps;
    double sum = 0.0;
    for (int k = 0; k < ST_TAPS; ++k) { const double x = k - ST_R; taps.w[k] = exp(-0.5 / (1.5 * 1.5) * (x * x)); sum += taps.w[k]; }
    for (int k = 0; k < ST_TAPS; ++k) taps.w[k] /= sum;
    const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
    const dim3 grid((W + ST_TW - 1) / ST_TW, (H + ST_TH - 1) / ST_TH, N);
    hipLaunchKernelGGL(st_similarity_kernel, grid, dim3(256), 0, stream, (const uint8_t *)a, a_row_stride, a_image_stride, (const uint8_t *)b, b_row_stride,
                       b_image_stride, channels, H, W, taps, C1, C2, (double *)ws);
    hipLaunchKernelGGL(st_similarity_final_kernel, dim3(N), dim3(256), 0, stream, (const double *)ws, st_tiles(H, W), (double)H * (double)W,
                       (double)(H - 2 * ST_R) * (double)(W - 2 * ST_R), out);
    DL_CHECK_LAUNCH("dl_stat_similarity");
    return 0;
}

// ---------------------------------------------------------------------------------------------------- confusion counts
__device__ __forceinline__ int st_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// out[n][c][4] = TP, FP, FN, TN of "prediction > 0" against "ground truth > 0"; c = 0: channel 0, c = 1: channel 2
__global__ void __launch_bounds__(256) st_confusion_kernel(const uint8_t *pred, size_t p_rs, size_t p_is, const uint8_t *gt, size_t g_rs, size_t g_is,
                                                           int H, int W, u64 *out) {
    const int n = blockIdx.y;
    const uint8_t *ip = pred + (size_t)n * p_is, *ig = gt + (size_t)n * g_is;
    int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int p = blockIdx.x * 256 + threadIdx.x; p < H * W; p += gridDim.x * 256) {
        const int y = p / W, x = p - y * W;
        const uint8_t *qp = ip + (size_t)y * p_rs + (size_t)x * 3, *qg = ig + (size_t)y * g_rs + (size_t)x * 3;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bool m = qp[2 * k] > 0, g = qg[2 * k] > 0;
            c[4 * k + 0] += m && g;
            c[4 * k + 1] += m && !g;
            c[4 * k + 2] += !m && g;
            c[4 * k + 3] += !m && !g;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int s = st_wave_sum(c[k]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(out + (size_t)n * 8 + k, (u64)s);
    }
}

extern "C" int dl_stat_confusion(const void *pred, size_t pred_row_stride, size_t pred_image_stride, const void *gt, size_t gt_row_stride,
                                 size_t gt_image_stride, int N, int H, int W, long long *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!pred || !gt || !out) DL_FAIL("dl_stat_confusion: null argument");
    if (N <= 0 || N > 65535 || st_bad_image(H, W)) DL_FAIL("dl_stat_confusion: empty problem or too large (N=%d H=%d W=%d)", N, H, W);
    if (pred_row_stride < (size_t)W * 3 || gt_row_stride < (size_t)W * 3) DL_FAIL("dl_stat_confusion: a row stride is shorter than a row");
    if (hipMemsetAsync(out, 0, (size_t)N * 8 * sizeof(long long), stream) != hipSuccess) DL_FAIL("dl_stat_confusion: memset");
    const int blocks = (H * W + 255) / 256;
    hipLaunchKernelGGL(st_confusion_kernel, dim3(blocks < 256 ? blocks : 256, N), dim3(256), 0, stream, (const uint8_t *)pred, pred_row_stride,
                       pred_image_stride, (const uint8_t *)gt, gt_row_stride, gt_image_stride, H, W, (u64 *)out);
    DL_CHECK_LAUNCH("dl_stat_confusion");
    return 0;
}

// ---------------------------------------------------------------------------------------------------- equal-value labelling
// the plane with values below min_value zeroed + the initial labels (head of the pixel's equal-value run inside its wavefront)
__global__ void __launch_bounds__(256) st_plane_kernel(const uint8_t *src, size_t rs, int ps, int H, int W, int min_value, int binarize, uint8_t *plane, int *label) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool in = p < H * W;
    const int y = in ? p / W : 0, x = in ? p - y * W : 1;
    int v = 0;
    if (in) {
        v = src[(size_t)y * rs + (size_t)x * ps];
        if (v < min_value) v = 0;
        if (binarize && v > 0) v = 1;
    }
    const int head = uf_value_run_head(v, p, x);
    if (!in) return;
    plane[p] = (uint8_t)v;
    label[p] = head;
}

// merge with the already-visited neighbours of the SAME value: left (only where the run was cut at a wavefront boundary), up, up-left, up-right
__global__ void __launch_bounds__(256) st_merge_kernel(const uint8_t *plane, int *label, int H, int W) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const uint8_t v = plane[p];
    if (v == 0) return;
    const int y = p / W, x = p - y * W;
    if (x > 0 && (threadIdx.x & 63) == 0 && plane[p - 1] == v) uf_union(label, p, p - 1);
    if (y > 0) {
        if (plane[p - W] == v) uf_union(label, p, p - W);
        if (x > 0 && plane[p - W - 1] == v) uf_union(label, p, p - W - 1);
        if (x + 1 < W && plane[p - W + 1] == v) uf_union(label, p, p - W + 1);
    }
}

// roots + component sizes + the number of labelled pixels
__global__ void __launch_bounds__(256) st_flatten_kernel(int *label, int n, int *cnt, int *labelled) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool active = p < n && label[p] >= 0;
    if (active) {
        const int r = uf_find(label, p);
        label[p] = r;
        atomicAdd(cnt + r, 1);
    }
    const int c = __popcll(__ballot(active));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(labelled, c);
}

struct StIsRoot {
    const int *cnt;
    __host__ __device__ bool operator()(const int &i) const { return cnt[i] > 0; }
};

// component i (root order = raster order of the first pixel): its size, and its dense id at the root
__global__ void __launch_bounds__(256) st_ids_kernel(const int *roots, const int *n_ptr, const int *cnt, int *idx, int *sizes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= *n_ptr) return;
    const int r = roots[i];
    idx[r] = i;
    sizes[i] = cnt[r];
}
__global__ void __launch_bounds__(256) st_relabel_kernel(const int *label, const int *idx, int n, int *out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int r = label[p];
    out[p] = r < 0 ? 0 : idx[r] + 1;
}

// workspace (bytes, regions 256-byte aligned): cnt | idx | root label | roots (int32[HW] each)  n (int32)  plane (u8[HW])  select temp
struct StLabelLayout { size_t cnt, idx, label, roots, n, plane, temp, temp_bytes, total; };
static int st_label_layout(int H, int W, StLabelLayout *l) {
    const size_t hw = (size_t)H * W;
    size_t off = 0;
    l->cnt = off; off += st_align(hw * 4);
    l->idx = off; off += st_align(hw * 4);
    l->label = off; off += st_align(hw * 4);
    l->roots = off; off += st_align(hw * 4);
    l->n = off; off += 256;
    l->plane = off; off += st_align(hw);
    size_t tb = 0;
    hipcub::CountingInputIterator<int> it(0);
    StIsRoot pred{nullptr};
    if (hipcub::DeviceSelect::If(nullptr, tb, it, (int *)nullptr, (int *)nullptr, (int)hw, pred) != hipSuccess) return -1;
    l->temp = off; l->temp_bytes = tb; off += st_align(tb);
    l->total = off;
    return 0;
}

extern "C" size_t dl_stat_label_ws_bytes(int H, int W) {
    StLabelLayout l;
    if (st_bad_image(H, W) || st_label_layout(H, W, &l)) return 0;
    return l.total;
}

extern "C" int dl_stat_label(const void *plane, size_t row_stride, int pixel_stride, int H, int W, int min_value, int binarize, void *ws, int *labels,
                             int *info, int *sizes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!plane || !ws || !labels || !info || !sizes) DL_FAIL("dl_stat_label: null argument");
    if (st_bad_image(H, W)) DL_FAIL("dl_stat_label: empty problem or too large (H=%d W=%d)", H, W);
    if (pixel_stride < 1 || row_stride < (size_t)(W - 1) * pixel_stride + 1) DL_FAIL("dl_stat_label: pixel stride %d, row stride %zu", pixel_stride, row_stride);
    if (min_value < 0 || min_value > 255) DL_FAIL("dl_stat_label: min_value=%d", min_value);
    StLabelLayout l;
    if (st_label_layout(H, W, &l)) DL_FAIL("dl_stat_label: workspace query failed");
    char *w = (char *)ws;
    const int n = H * W, blocks = (n + 255) / 256;
    int *cnt = (int *)(w + l.cnt), *idx = (int *)(w + l.idx), *label = (int *)(w + l.label), *roots = (int *)(w + l.roots), *n_dev = (int *)(w + l.n);
    uint8_t *pl = (uint8_t *)(w + l.plane);
    if (hipMemsetAsync(cnt, 0, (size_t)n * 4, stream) != hipSuccess || hipMemsetAsync(info, 0, 2 * sizeof(int), stream) != hipSuccess)
        DL_FAIL("dl_stat_label: memset");
    hipLaunchKernelGGL(st_plane_kernel, dim3(blocks), dim3(256), 0, stream, (const uint8_t *)plane, row_stride, pixel_stride, H, W, min_value, binarize, pl, label);
    hipLaunchKernelGGL(st_merge_kernel, dim3(blocks), dim3(256), 0, stream, pl, label, H, W);
    hipLaunchKernelGGL(st_flatten_kernel, dim3(blocks), dim3(256), 0, stream, label, n, cnt, info + 1);
    hipcub::CountingInputIterator<int> it(0);
    StIsRoot pred{cnt};
    size_t tb = l.temp_bytes;
    if (hipcub::DeviceSelect::If(w + l.temp, tb, it, roots, n_dev, n, pred, stream) != hipSuccess) DL_FAIL("dl_stat_label: select failed");
    hipLaunchKernelGGL(st_ids_kernel, dim3(blocks), dim3(256), 0, stream, roots, n_dev, cnt, idx, sizes);
    hipLaunchKernelGGL(st_relabel_kernel, dim3(blocks), dim3(256), 0, stream, label, idx, n, labels);
    if (hipMemcpyAsync(info, n_dev, sizeof(int), hipMemcpyDeviceToDevice, stream) != hipSuccess) DL_FAIL("dl_stat_label: copy");
    DL_CHECK_LAUNCH("dl_stat_label");
    return 0;
}

// ---------------------------------------------------------------------------------------------------- AJI
#define ST_NO_KEY (~0ull)

// (gt id << 32) | pred id of the pixels labelled in both images; the others sort behind every real key
__global__ void __launch_bounds__(256) st_keys_kernel(const int *gt, const int *pred, int n, u64 *keys) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int g = gt[p], q = pred[p];
    keys[p] = (g > 0 && q > 0) ? (((u64)(unsigned)g << 32) | (u64)(unsigned)q) : ST_NO_KEY;
}

// compute_aji's greedy pass over the intersection table (uniq = keys in ascending order = by gt id, then by pred id; counts = pixels).
// One wavefront: the gt components in id order; the lanes scan the component's rows 64 at a time and keep the largest intersection with a pred
// component that is still unmarked, the smallest pred id among equals (the reference's strict `>` over ascending pred ids).
__global__ void __launch_bounds__(64) st_aji_greedy_kernel(const u64 *uniq, const int *counts, const int *n_runs, const int *gt_info, const int *gt_sizes, const int *pred_info,
                                                           const int *pred_sizes, int *marked, long long *out) {
    const int lane = threadIdx.x;
    const int runs = *n_runs, n_gt = gt_info[0], n_pred = pred_info[0];
    long long ti = 0, tu = 0;
    int pos = 0;
    while (pos < runs) {
        const unsigned g = (unsigned)(uniq[pos] >> 32);              // (uniform)
        if (g == 0xFFFFFFFFu || g > (unsigned)n_gt) break;           // the run of unlabelled pixels: the table ends here (or not a label image)
        int bi = 0, bp = 0x7fffffff, end = pos;
        bool more = true;
        while (more) {
            const int i = end + lane;
            bool mine = false;
            if (i < runs) {
                const u64 k = uniq[i];
                if ((unsigned)(k >> 32) == g) {
                    mine = true;
                    const int q = (int)(unsigned)(k & 0xFFFFFFFFull), c = counts[i];
                    if (q <= n_pred && !__atomic_load_n(marked + q, __ATOMIC_RELAXED) && c > bi) { bi = c; bp = q; }       // (rows come in ascending pred id)
                }
            }
            const int rows = __popcll(__ballot(mine));               // the rows of g are contiguous: a prefix of the lanes
            end += rows;
            more = rows == 64;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int oi = __shfl_xor(bi, o, 64), op = __shfl_xor(bp, o, 64);
            if (oi > bi || (oi == bi && op < bp)) { bi = oi; bp = op; }
        }
        if (bi > 0) {
            if (lane == 0) __atomic_store_n(marked + bp, 1, __ATOMIC_RELAXED);
            __threadfence();                                          // the other lanes read the mark in the next round
            ti += bi;
            tu += (long long)gt_sizes[g - 1] + (long long)pred_sizes[bp - 1] - bi;
        }
        pos = end;
    }
    long long u = 0;
    for (int q = 1 + lane; q <= n_pred; q += 64)
        if (!__atomic_load_n(marked + q, __ATOMIC_RELAXED)) u += pred_sizes[q - 1];
    for (int o = 32; o > 0; o >>= 1) u += __shfl_xor(u, o, 64);
    if (lane == 0) { out[0] = ti; out[1] = tu; out[2] = u; }
}

// workspace: keys | sorted keys | unique keys (u64[HW] each)  counts (int32[HW])  marked (int32[HW + 1])  runs (int32)  sort / encode temp
struct StAjiLayout { size_t keys, sorted, uniq, counts, marked, runs, temp, temp_bytes, total; };
static int st_aji_layout(int H, int W, StAjiLayout *l) {
    const size_t hw = (size_t)H * W;
    size_t off = 0;
    l->keys = off; off += st_align(hw * 8);
    l->sorted = off; off += st_align(hw * 8);
    l->uniq = off; off += st_align(hw * 8);
    l->counts = off; off += st_align(hw * 4);
    l->marked = off; off += st_align((hw + 1) * 4);
    l->runs = off; off += 256;
    size_t t1 = 0, t2 = 0;
    if (hipcub::DeviceRadixSort::SortKeys(nullptr, t1, (const u64 *)nullptr, (u64 *)nullptr, (int)hw, 0, 64) != hipSuccess) return -1;
    if (hipcub::DeviceRunLengthEncode::Encode(nullptr, t2, (const u64 *)nullptr, (u64 *)nullptr, (int *)nullptr, (int *)nullptr, (int)hw) != hipSuccess) return -1;
    l->temp = off; l->temp_bytes = t1 > t2 ? t1 : t2; off += st_align(l->temp_bytes);
    l->total = off;
    return 0;
}

extern "C" size_t dl_stat_aji_ws_bytes(int H, int W) {
    StAjiLayout l;
    if (st_bad_image(H, W) || st_aji_layout(H, W, &l)) return 0;
    return l.total;
}

extern "C" int dl_stat_aji(const int *gt_labels, const int *gt_info, const int *gt_sizes, const int *pred_labels, const int *pred_info, const int *pred_sizes, int H, int W,
                           void *ws, long long *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!gt_labels || !gt_info || !gt_sizes || !pred_labels || !pred_info || !pred_sizes || !ws || !out) DL_FAIL("dl_stat_aji: null argument");
    if (st_bad_image(H, W)) DL_FAIL("dl_stat_aji: empty problem or too large (H=%d W=%d)", H, W);
    StAjiLayout l;
    if (st_aji_layout(H, W, &l)) DL_FAIL("dl_stat_aji: workspace query failed");
    char *w = (char *)ws;
    const int n = H * W, blocks = (n + 255) / 256;
    u64 *keys = (u64 *)(w + l.keys), *sorted = (u64 *)(w + l.sorted), *uniq = (u64 *)(w + l.uniq);
    int *counts = (int *)(w + l.counts), *marked = (int *)(w + l.marked), *runs = (int *)(w + l.runs);
    if (hipMemsetAsync(marked, 0, ((size_t)n + 1) * 4, stream) != hipSuccess) DL_FAIL("dl_stat_aji: memset");
    hipLaunchKernelGGL(st_keys_kernel, dim3(blocks), dim3(256), 0, stream, gt_labels, pred_labels, n, keys);
    size_t tb = l.temp_bytes;
    if (hipcub::DeviceRadixSort::SortKeys(w + l.temp, tb, (const u64 *)keys, sorted, n, 0, 64, stream) != hipSuccess) DL_FAIL("dl_stat_aji: sort failed");
    tb = l.temp_bytes;
    if (hipcub::DeviceRunLengthEncode::Encode(w + l.temp, tb, (const u64 *)sorted, uniq, counts, runs, n, stream) != hipSuccess) DL_FAIL("dl_stat_aji: encode failed");
    hipLaunchKernelGGL(st_aji_greedy_kernel, dim3(1), dim3(64), 0, stream, (const u64 *)uniq, (const int *)counts, (const int *)runs, gt_info, gt_sizes, pred_info,
                       pred_sizes, marked, out);
    DL_CHECK_LAUNCH("dl_stat_aji");
    return 0;
}
