// tiles.hip -- uint8 image <-> engine tile batches: the crop / is_empty / stitch steps either side of the generator DAG
// (deepliif/util/__init__.py:129-331 InferenceTiler, deepliif/models/__init__.py:391-396 is_empty,
// deepliif/data/__init__.py:133-138 transform, deepliif/util/util.py:117-139 tensor2im).  Byte / integer work, HBM-bound:
// one thread per pixel, 16-byte (bf16) or 2 x 16-byte (fp32) NHWC stores, no LDS.
#include "common.h"
#include <stdlib.h>

// reflect-periodic source coordinate: an image narrower than a patch is widened by appending mirrored copies
// (util/__init__.py:196-211) -> period 2*n: c, then 2n-1-c
__device__ __forceinline__ int mirror_coord(int c, int n) {
    if (c < n) return c;
    const int m = c % (2 * n);
    return m < n ? m : 2 * n - 1 - m;
}

struct TileSrc {
    const uint8_t *img[DL_TILE_MAX_SRC];
    long long row_stride[DL_TILE_MAX_SRC];
};

// fetch the RGB bytes of tile pixel (ty, tx) of tile `origin`, honouring the solid border (pad) and the mirror extension
__device__ __forceinline__ void tile_pixel(const uint8_t *img, long long row_stride, int H0, int W0, int ox, int oy, int ty, int tx, int patch,
                                           int pad, uint32_t pad_rgb, int &r, int &g, int &b) {
    const int py = ty - pad, px = tx - pad;
    if (py < 0 || px < 0 || py >= patch || px >= patch) {
        r = pad_rgb & 0xff; g = (pad_rgb >> 8) & 0xff; b = (pad_rgb >> 16) & 0xff;
        return;
    }
    const int sy = mirror_coord(oy + py, H0), sx = mirror_coord(ox + px, W0);
    const uint8_t *p = img + (long long)sy * row_stride + 3ll * sx;
    r = p[0]; g = p[1]; b = p[2];
}

template <typename T>
__global__ void tile_gather_kernel(TileSrc src, int n_src, int H0, int W0, const int32_t *__restrict__ origins, int tile, int pad, uint32_t pad_rgb,
                                   const float *__restrict__ lut, T *__restrict__ out, int out_pstride, int out_cp) {
    const int t = blockIdx.y;
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= tile * tile) return;
    const int ty = pix / tile, tx = pix - ty * tile;
    const int ox = origins[2 * t], oy = origins[2 * t + 1];
    const int patch = tile - 2 * pad;
    T *o = out + ((long long)t * tile * tile + pix) * out_pstride;
    for (int c8 = 0; c8 < out_cp; c8 += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
#pragma unroll
        for (int s = 0; s < DL_TILE_MAX_SRC; ++s) {
            const int c = 3 * s;                     // channels 3s .. 3s+2 of the concatenated input (torch.cat(dim=1), models/__init__.py:279)
            if (s < n_src && c + 2 >= c8 && c < c8 + 8) {
                int r, g, b;
                tile_pixel(src.img[s], src.row_stride[s], H0, W0, ox, oy, ty, tx, patch, pad, pad_rgb, r, g, b);
                const int rgb[3] = {r, g, b};
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int cc = c + k - c8;
                    if (cc >= 0 && cc < 8) v[cc] = lut[rgb[k]];
                }
            }
        }
        Vec8<T>::store(o + c8, v);
    }
}

// (count, sum, sum of squares) of the gray values in 1..254 of every tile: the exact integer form of image_variance_gray
// (PIL convert('L'): L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16).  Integer atomics -> order-independent, deterministic.
__global__ void tile_gray_stats_kernel(const uint8_t *__restrict__ img, long long row_stride, int H0, int W0, const int32_t *__restrict__ origins, int tile,
                                       int pad, uint32_t pad_rgb, unsigned long long *__restrict__ stats) {
    const int t = blockIdx.y;
    const int ox = origins[2 * t], oy = origins[2 * t + 1];
    const int patch = tile - 2 * pad;
    unsigned int cnt = 0, s1 = 0;
    unsigned long long s2 = 0;
    for (int pix = blockIdx.x * blockDim.x + threadIdx.x; pix < tile * tile; pix += gridDim.x * blockDim.x) {
        const int ty = pix / tile, tx = pix - ty * tile;
        int r, g, b;
        tile_pixel(img, row_stride, H0, W0, ox, oy, ty, tx, patch, pad, pad_rgb, r, g, b);
        const unsigned int L = (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16;
        if (L != 0u && L != 255u) { cnt += 1; s1 += L; s2 += (unsigned long long)(L * L); }
    }
    unsigned long long c64 = cnt, a64 = s1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c64 += __shfl_xor(c64, o, 64);
        a64 += __shfl_xor(a64, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&stats[3 * t + 0], c64);
        atomicAdd(&stats[3 * t + 1], a64);
        atomicAdd(&stats[3 * t + 2], s2);
    }
}

// rect record (8 x int32): slot (tile index in the batch, or -1 = constant colour), l, t (tile-local), w, h, px, py (image), rgb
template <typename T>
__global__ void tile_paste_kernel(const T *__restrict__ tiles, int in_pstride, int tile, const int32_t *__restrict__ rects, uint8_t *__restrict__ dst,
                                  long long dst_row_stride) {
    const int32_t *rc = rects + 8 * blockIdx.y;
    const int slot = rc[0], l = rc[1], tp = rc[2], w = rc[3], h = rc[4], px = rc[5], py = rc[6];
    const uint32_t rgb = (uint32_t)rc[7];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < w * h; i += gridDim.x * blockDim.x) {
        const int y = i / w, x = i - y * w;
        uint8_t *o = dst + (long long)(py + y) * dst_row_stride + 3ll * (px + x);
        if (slot < 0) {
            o[0] = rgb & 0xff; o[1] = (rgb >> 8) & 0xff; o[2] = (rgb >> 16) & 0xff;
            continue;
        }
        const T *p = tiles + ((long long)slot * tile * tile + (long long)(tp + y) * tile + (l + x)) * in_pstride;
        float v[8];
        Vec8<T>::load(p, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // tensor2im (util/util.py:132-135): (x + 1) / 2.0 * 255.0 in fp32, then astype(uint8) = truncation; no contraction
            const float f = __fmul_rn(__fmul_rn(__fadd_rn(v[k], 1.0f), 0.5f), 255.0f);
            o[k] = (uint8_t)(int)f;
        }
    }
}

// ---- resampled tiles (tile_size != scale_size): PIL's Image.resize (separable bicubic, 8-bit fixed point) either side of the network, bit for bit.
// The coefficient table comes from the caller (deepliif_amd/tiling.py resample_table: bounds[xx] = {xmin, n}, kk[xx][ksize]); the kernels only apply it:
// byte = clip((2^21 + sum pixel * k) >> 22), horizontal pass first, its uint8 result read by the vertical pass.  One workgroup owns one tile and a
// strip of R output rows: it runs the horizontal pass for the source rows the strip's vertical taps reach (bounds[first].xmin .. bounds[last].xmin + n)
// into an LDS byte image (one r | g << 8 | b << 16 word per pixel), barriers, and runs the vertical pass from LDS into the store.
#define DL_RS_BITS 22
#define DL_RS_LDS_BYTES 65536
#define DL_RS_MAX_STRIP 32        // upper end of R: more strips per tile than the LDS budget alone would give, so that a batch of 8 tiles fills the CUs

struct RsTable {
    const int32_t *bounds;
    const int32_t *kk;
    int ksize;
};

// taps of output coordinate xx; clamped so that a malformed table cannot turn into an out-of-range read
__device__ __forceinline__ void rs_taps(const RsTable &tb, int xx, int in, int &x0, int &n) {
    x0 = tb.bounds[2 * xx];
    n = tb.bounds[2 * xx + 1];
    x0 = x0 < 0 ? 0 : (x0 > in ? in : x0);
    const int most = tb.ksize < in - x0 ? tb.ksize : in - x0;
    n = n < 0 ? 0 : (n > most ? most : n);
}

__device__ __forceinline__ uint32_t rs_clip8(int acc) {
    const int v = acc >> DL_RS_BITS;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ uint32_t rs_pack(int a0, int a1, int a2) { return rs_clip8(a0) | (rs_clip8(a1) << 8) | (rs_clip8(a2) << 16); }

// vertical pass of output pixel (yy, xx) over the LDS image `mid` (row 0 = source row `ya`, `rows` rows of `stride` words)
__device__ __forceinline__ uint32_t rs_vertical(const RsTable &tb, const uint32_t *mid, int stride, int ya, int rows, int yy, int xx, int in) {
    int v0, n;
    rs_taps(tb, yy, in, v0, n);
    int r0 = v0 - ya;
    if (r0 < 0) r0 = 0;
    if (n > rows - r0) n = rows - r0;
    const int32_t *k = tb.kk + (long long)yy * tb.ksize;
    int a0 = 1 << (DL_RS_BITS - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
        const uint32_t m = mid[(r0 + j) * stride + xx];
        const int kj = k[j];
        a0 += (int)(m & 0xff) * kj;
        a1 += (int)((m >> 8) & 0xff) * kj;
        a2 += (int)((m >> 16) & 0xff) * kj;
    }
    return rs_pack(a0, a1, a2);
}

template <typename T>
__global__ void __launch_bounds__(256) tile_gather_resample_kernel(TileSrc src, int n_src, int H0, int W0, const int32_t *__restrict__ origins, int tile, int pad,
                                                                   uint32_t pad_rgb, int net, RsTable tb, int R, int rows_cap, const float *__restrict__ lut,
                                                                   T *__restrict__ out, int out_pstride, int out_cp) {
    extern __shared__ uint32_t rs_lds[];
    uint32_t *mid = rs_lds;                          // [rows_cap][net]: horizontally resized source rows of the current image
    uint32_t *done = rs_lds + rows_cap * net;        // [n_src - 1][R][net]: finished strips of the earlier images, until all channels of a pixel are stored together
    const int t = blockIdx.y;
    const int y0 = blockIdx.x * R, y1 = y0 + R < net ? y0 + R : net;
    if (y0 >= y1) return;
    const int ox = origins[2 * t], oy = origins[2 * t + 1];
    const int patch = tile - 2 * pad;
    int ya, na, yb, nb;
    rs_taps(tb, y0, tile, ya, na);
    rs_taps(tb, y1 - 1, tile, yb, nb);
    int rows = yb + nb - ya;
    rows = rows < 0 ? 0 : (rows > rows_cap ? rows_cap : rows);
    for (int s = 0; s < n_src; ++s) {
        const uint8_t *img = src.img[0];
        long long row_stride = src.row_stride[0];
#pragma unroll
        for (int q = 1; q < DL_TILE_MAX_SRC; ++q)
            if (q == s) { img = src.img[q]; row_stride = src.row_stride[q]; }
        if (s) __syncthreads();                      // the vertical pass of the previous image has finished reading mid
        for (int i = threadIdx.x; i < rows * net; i += blockDim.x) {
            const int row = i / net, xx = i - row * net;
            int x0, n;
            rs_taps(tb, xx, tile, x0, n);
            const int32_t *k = tb.kk + (long long)xx * tb.ksize;
            int a0 = 1 << (DL_RS_BITS - 1), a1 = a0, a2 = a0;
            for (int j = 0; j < n; ++j) {
                int r, g, b;
                tile_pixel(img, row_stride, H0, W0, ox, oy, ya + row, x0 + j, patch, pad, pad_rgb, r, g, b);
                const int kj = k[j];
                a0 += r * kj; a1 += g * kj; a2 += b * kj;
            }
            mid[i] = rs_pack(a0, a1, a2);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < (y1 - y0) * net; i += blockDim.x) {
            const int ry = i / net, xx = i - ry * net;
            const uint32_t word = rs_vertical(tb, mid, net, ya, rows, y0 + ry, xx, tile);
            if (s + 1 < n_src) {
                done[(s * R + ry) * net + xx] = word;        // read back below by this same thread
                continue;
            }
            T *o = out + (((long long)t * net + (y0 + ry)) * net + xx) * out_pstride;
            for (int c8 = 0; c8 < out_cp; c8 += 8) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = 0.f;
#pragma unroll
                for (int q = 0; q < DL_TILE_MAX_SRC; ++q) {
                    const int c = 3 * q;                      // channels 3q .. 3q+2 of the concatenated input
                    if (q < n_src && c + 2 >= c8 && c < c8 + 8) {
                        const uint32_t m = q + 1 < n_src ? done[(q * R + ry) * net + xx] : word;
#pragma unroll
                        for (int kc = 0; kc < 3; ++kc) {
                            const int cc = c + kc - c8;
                            if (cc >= 0 && cc < 8) v[cc] = lut[(m >> (8 * kc)) & 0xff];
                        }
                    }
                }
                Vec8<T>::store(o + c8, v);
            }
        }
    }
}

// tensor2im byte of one activation value, in the exact form of tile_paste_kernel
__device__ __forceinline__ int tensor2im_u8(float x) { return (int)(uint8_t)(int)__fmul_rn(__fmul_rn(__fadd_rn(x, 1.0f), 0.5f), 255.0f); }

template <typename T>
__global__ void __launch_bounds__(256) tile_paste_resample_kernel(const T *__restrict__ tiles, int in_pstride, int net, int tile, RsTable tb, int R, int rows_cap,
                                                                  const int32_t *__restrict__ rects, uint8_t *__restrict__ dst, long long dst_row_stride) {
    extern __shared__ uint32_t rs_lds[];             // [rows_cap][tile]: tensor2im bytes of the activation rows, horizontally resized (columns l .. l+w-1 used)
    const int32_t *rc = rects + 8 * blockIdx.y;
    const int slot = rc[0], l = rc[1], tp = rc[2], w = rc[3], h = rc[4], px = rc[5], py = rc[6];
    const uint32_t rgb = (uint32_t)rc[7];
    if (l < 0 || tp < 0 || w <= 0 || h <= 0 || l + w > tile || tp + h > tile) return;          // not a window of the tile
    const int y0 = tp + blockIdx.x * R, y1 = y0 + R < tp + h ? y0 + R : tp + h;
    if (y0 >= y1) return;
    if (slot < 0) {
        for (int i = threadIdx.x; i < (y1 - y0) * w; i += blockDim.x) {
            const int ry = i / w, x = i - ry * w;
            uint8_t *o = dst + (long long)(py + y0 - tp + ry) * dst_row_stride + 3ll * (px + x);
            o[0] = rgb & 0xff; o[1] = (rgb >> 8) & 0xff; o[2] = (rgb >> 16) & 0xff;
        }
        return;
    }
    int ya, na, yb, nb;
    rs_taps(tb, y0, net, ya, na);
    rs_taps(tb, y1 - 1, net, yb, nb);
    int rows = yb + nb - ya;
    rows = rows < 0 ? 0 : (rows > rows_cap ? rows_cap : rows);
    const T *base = tiles + (long long)slot * net * net * in_pstride;
    for (int i = threadIdx.x; i < rows * w; i += blockDim.x) {
        const int row = i / w, xx = l + (i - row * w);
        int x0, n;
        rs_taps(tb, xx, net, x0, n);
        const int32_t *k = tb.kk + (long long)xx * tb.ksize;
        const T *p = base + ((long long)(ya + row) * net + x0) * in_pstride;
        int a0 = 1 << (DL_RS_BITS - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < n; ++j) {
            float v[8];
            Vec8<T>::load(p + (long long)j * in_pstride, v);
            const int kj = k[j];
            a0 += tensor2im_u8(v[0]) * kj; a1 += tensor2im_u8(v[1]) * kj; a2 += tensor2im_u8(v[2]) * kj;
        }
        rs_lds[row * tile + xx] = rs_pack(a0, a1, a2);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (y1 - y0) * w; i += blockDim.x) {
        const int ry = i / w, x = i - ry * w;
        const uint32_t m = rs_vertical(tb, rs_lds, tile, ya, rows, y0 + ry, l + x, net);
        uint8_t *o = dst + (long long)(py + y0 - tp + ry) * dst_row_stride + 3ll * (px + x);
        o[0] = m & 0xff; o[1] = (m >> 8) & 0xff; o[2] = (m >> 16) & 0xff;
    }
}

// tiles / rectangles per launch (gridDim.y <= 65535); DL_TILE_GRID_Y=<n> overrides it so that the chunked path can be tested on small regions
static int tile_grid_y() {
    static const int v = [] { const char *e = DL_DEV_ENV("DL_TILE_GRID_Y"); const int n = e ? atoi(e) : 0; return (n >= 1 && n <= 65535) ? n : 32768; }();
    return v;
}
#define DL_TILE_GRID_Y (tile_grid_y())

extern "C" int dl_tile_gather_u8(const void *const *imgs, const int64_t *row_strides, int n_src, int H0, int W0, const int32_t *origins,
                                 int n_tiles, int tile, int pad, uint32_t pad_rgb, const float *lut, int out_dtype, void *out,
                                 int out_pstride, int out_cp, void *stream) {
    if (n_tiles <= 0 || tile <= 0 || H0 <= 0 || W0 <= 0) DL_FAIL("dl_tile_gather_u8: empty problem (n_tiles=%d tile=%d image %dx%d)", n_tiles, tile, W0, H0);
    if (n_src < 1 || n_src > DL_TILE_MAX_SRC) DL_FAIL("dl_tile_gather_u8: n_src=%d outside 1..%d", n_src, DL_TILE_MAX_SRC);
    if (out_cp % 8 || out_cp < 3 * n_src || out_pstride < out_cp) DL_FAIL("dl_tile_gather_u8: bad channel geometry (Cp=%d pstride=%d for %d source images)", out_cp, out_pstride, n_src);
    if (pad < 0 || 2 * pad >= tile) DL_FAIL("dl_tile_gather_u8: pad=%d does not fit tile=%d", pad, tile);
    TileSrc s;
    for (int i = 0; i < DL_TILE_MAX_SRC; ++i) {
        s.img[i] = (const uint8_t *)(i < n_src ? imgs[i] : imgs[0]);
        s.row_stride[i] = i < n_src ? row_strides[i] : row_strides[0];
    }
    // gridDim.y is limited to 65535: a region with more tiles (about 115k x 115k pixels at tile 512 / overlap 32) is launched in chunks
    for (int t0 = 0; t0 < n_tiles; t0 += DL_TILE_GRID_Y) {
        const int nt = n_tiles - t0 < DL_TILE_GRID_Y ? n_tiles - t0 : DL_TILE_GRID_Y;
        dim3 grid((tile * tile + 255) / 256, nt);
        const size_t o0 = (size_t)t0 * tile * tile * out_pstride;
        if (out_dtype == DL_BF16)
            hipLaunchKernelGGL(tile_gather_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, s, n_src, H0, W0, origins + 2 * (size_t)t0, tile, pad, pad_rgb, lut,
                               (bf16_t *)out + o0, out_pstride, out_cp);
        else
            hipLaunchKernelGGL(tile_gather_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, s, n_src, H0, W0, origins + 2 * (size_t)t0, tile, pad, pad_rgb, lut,
                               (float *)out + o0, out_pstride, out_cp);
        DL_CHECK_LAUNCH("dl_tile_gather_u8");
    }
    return 0;
}

extern "C" int dl_tile_gray_stats_u8(const void *img, int64_t row_stride, int H0, int W0, const int32_t *origins, int n_tiles, int tile, int pad,
                                     uint32_t pad_rgb, uint64_t *stats, void *stream) {
    if (n_tiles <= 0 || tile <= 0 || H0 <= 0 || W0 <= 0) DL_FAIL("dl_tile_gray_stats_u8: empty problem (n_tiles=%d tile=%d image %dx%d)", n_tiles, tile, W0, H0);
    if (pad < 0 || 2 * pad >= tile) DL_FAIL("dl_tile_gray_stats_u8: pad=%d does not fit tile=%d", pad, tile);
    hipError_t e = hipMemsetAsync(stats, 0, sizeof(uint64_t) * 3 * n_tiles, (hipStream_t)stream);
    if (e != hipSuccess) DL_FAIL("dl_tile_gray_stats_u8: memset failed: %s", hipGetErrorString(e));
    int bx = (tile * tile + 256 * 8 - 1) / (256 * 8);
    if (bx < 1) bx = 1;
    for (int t0 = 0; t0 < n_tiles; t0 += DL_TILE_GRID_Y) {
        const int nt = n_tiles - t0 < DL_TILE_GRID_Y ? n_tiles - t0 : DL_TILE_GRID_Y;
        hipLaunchKernelGGL(tile_gray_stats_kernel, dim3(bx, nt), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)img, (long long)row_stride, H0, W0,
                           origins + 2 * (size_t)t0, tile, pad, pad_rgb, (unsigned long long *)stats + 3 * (size_t)t0);
        DL_CHECK_LAUNCH("dl_tile_gray_stats_u8");
    }
    return 0;
}

extern "C" int dl_tile_paste_u8(int in_dtype, const void *tiles, int in_pstride, int tile, const int32_t *rects, int n_rects, void *dst, int64_t dst_row_stride,
                                void *stream) {
    if (n_rects <= 0 || tile <= 0) DL_FAIL("dl_tile_paste_u8: empty problem (n_rects=%d tile=%d)", n_rects, tile);
    if (in_pstride < 8) DL_FAIL("dl_tile_paste_u8: engine tiles have at least 8 padded channels (pstride=%d)", in_pstride);
    for (int r0 = 0; r0 < n_rects; r0 += DL_TILE_GRID_Y) {          // the rectangles carry their own tile index: only the list is chunked
        const int nr = n_rects - r0 < DL_TILE_GRID_Y ? n_rects - r0 : DL_TILE_GRID_Y;
        dim3 grid(64, nr);
        if (in_dtype == DL_BF16)
            hipLaunchKernelGGL(tile_paste_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t *)tiles, in_pstride, tile, rects + 8 * (size_t)r0, (uint8_t *)dst,
                               (long long)dst_row_stride);
        else
            hipLaunchKernelGGL(tile_paste_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float *)tiles, in_pstride, tile, rects + 8 * (size_t)r0, (uint8_t *)dst,
                               (long long)dst_row_stride);
        DL_CHECK_LAUNCH("dl_tile_paste_u8");
    }
    return 0;
}

// ---- host side of the resampled entries: strip height R and the LDS image it needs
static int rs_ksize(int in, int out) { return 2 * (in > out ? (int)((2ll * in + out - 1) / out) : 2) + 1; }      // 2 * ceil(support) + 1, support = 2 * max(in / out, 1)
// source rows the vertical taps of R consecutive output rows can reach: xmax(last) - xmin(first) <= (R - 1) * in / out + 2 * support + 1
static int rs_rows_cap(int in, int out, int R) {
    const long long r = ((long long)(R - 1) * in) / out + rs_ksize(in, out);
    return r < in ? (int)r : in;
}
static size_t rs_lds_bytes(int in, int out, int R, int n_src) { return 4ull * out * ((size_t)rs_rows_cap(in, out, R) + (size_t)(n_src - 1) * R); }
static int rs_strip_rows(int in, int out, int n_src) {
    for (int R = out < DL_RS_MAX_STRIP ? out : DL_RS_MAX_STRIP; R >= 1; --R)
        if (rs_lds_bytes(in, out, R, n_src) <= DL_RS_LDS_BYTES) return R;
    return 0;
}

extern "C" int dl_tile_resample_supported(int in_size, int out_size) {
    if (in_size <= 0 || out_size <= 0 || in_size == out_size) return 0;
    return rs_strip_rows(in_size, out_size, DL_TILE_MAX_SRC) >= 1 ? 1 : 0;
}

extern "C" int dl_tile_gather_resample_u8(const void *const *imgs, const int64_t *row_strides, int n_src, int H0, int W0, const int32_t *origins, int n_tiles, int tile,
                                          int pad, uint32_t pad_rgb, int net, const int32_t *bounds, const int32_t *kk, int ksize, int strip_rows, const float *lut,
                                          int out_dtype, void *out, int out_pstride, int out_cp, void *stream) {
    if (n_tiles <= 0 || tile <= 0 || net <= 0 || H0 <= 0 || W0 <= 0)
        DL_FAIL("dl_tile_gather_resample_u8: empty problem (n_tiles=%d tile=%d net=%d image %dx%d)", n_tiles, tile, net, W0, H0);
    if (tile == net) DL_FAIL("dl_tile_gather_resample_u8: tile == net == %d is dl_tile_gather_u8", net);
    if (n_src < 1 || n_src > DL_TILE_MAX_SRC) DL_FAIL("dl_tile_gather_resample_u8: n_src=%d outside 1..%d", n_src, DL_TILE_MAX_SRC);
    if (out_cp % 8 || out_cp < 3 * n_src || out_pstride < out_cp)
        DL_FAIL("dl_tile_gather_resample_u8: bad channel geometry (Cp=%d pstride=%d for %d source images)", out_cp, out_pstride, n_src);
    if (pad < 0 || 2 * pad >= tile) DL_FAIL("dl_tile_gather_resample_u8: pad=%d does not fit tile=%d", pad, tile);
    if (!bounds || !kk || !lut) DL_FAIL("dl_tile_gather_resample_u8: the coefficient table (bounds, kk) and lut are required");
    if (ksize != rs_ksize(tile, net)) DL_FAIL("dl_tile_gather_resample_u8: ksize=%d, the table of %d -> %d has %d", ksize, tile, net, rs_ksize(tile, net));
    const int R = strip_rows > 0 ? (strip_rows < net ? strip_rows : net) : rs_strip_rows(tile, net, n_src);
    if (R < 1 || rs_lds_bytes(tile, net, R, n_src) > DL_RS_LDS_BYTES)
        DL_FAIL("dl_tile_gather_resample_u8: %d -> %d with %d source images and strips of %d rows does not fit %d bytes of LDS", tile, net, n_src, R, DL_RS_LDS_BYTES);
    const int rows_cap = rs_rows_cap(tile, net, R);
    const size_t lds = rs_lds_bytes(tile, net, R, n_src);
    TileSrc s;
    for (int i = 0; i < DL_TILE_MAX_SRC; ++i) {
        s.img[i] = (const uint8_t *)(i < n_src ? imgs[i] : imgs[0]);
        s.row_stride[i] = i < n_src ? row_strides[i] : row_strides[0];
    }
    const RsTable tb = {bounds, kk, ksize};
    for (int t0 = 0; t0 < n_tiles; t0 += DL_TILE_GRID_Y) {
        const int nt = n_tiles - t0 < DL_TILE_GRID_Y ? n_tiles - t0 : DL_TILE_GRID_Y;
        dim3 grid((net + R - 1) / R, nt);
        const size_t o0 = (size_t)t0 * net * net * out_pstride;
        if (out_dtype == DL_BF16)
            hipLaunchKernelGGL(tile_gather_resample_kernel<bf16_t>, grid, dim3(256), lds, (hipStream_t)stream, s, n_src, H0, W0, origins + 2 * (size_t)t0, tile, pad, pad_rgb,
                               net, tb, R, rows_cap, lut, (bf16_t *)out + o0, out_pstride, out_cp);
        else
            hipLaunchKernelGGL(tile_gather_resample_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, s, n_src, H0, W0, origins + 2 * (size_t)t0, tile, pad, pad_rgb,
                               net, tb, R, rows_cap, lut, (float *)out + o0, out_pstride, out_cp);
        DL_CHECK_LAUNCH("dl_tile_gather_resample_u8");
    }
    return 0;
}

extern "C" int dl_tile_paste_resample_u8(int in_dtype, const void *tiles, int in_pstride, int net, int tile, const int32_t *bounds, const int32_t *kk, int ksize,
                                         int strip_rows, const int32_t *rects, int n_rects, void *dst, int64_t dst_row_stride, void *stream) {
    if (n_rects <= 0 || tile <= 0 || net <= 0) DL_FAIL("dl_tile_paste_resample_u8: empty problem (n_rects=%d tile=%d net=%d)", n_rects, tile, net);
    if (tile == net) DL_FAIL("dl_tile_paste_resample_u8: tile == net == %d is dl_tile_paste_u8", net);
    if (in_pstride < 8) DL_FAIL("dl_tile_paste_resample_u8: engine tiles have at least 8 padded channels (pstride=%d)", in_pstride);
    if (!bounds || !kk || !rects || !dst) DL_FAIL("dl_tile_paste_resample_u8: the coefficient table (bounds, kk), rects and dst are required");
    if (ksize != rs_ksize(net, tile)) DL_FAIL("dl_tile_paste_resample_u8: ksize=%d, the table of %d -> %d has %d", ksize, net, tile, rs_ksize(net, tile));
    const int R = strip_rows > 0 ? (strip_rows < tile ? strip_rows : tile) : rs_strip_rows(net, tile, 1);
    if (R < 1 || rs_lds_bytes(net, tile, R, 1) > DL_RS_LDS_BYTES)
        DL_FAIL("dl_tile_paste_resample_u8: %d -> %d with strips of %d rows does not fit %d bytes of LDS", net, tile, R, DL_RS_LDS_BYTES);
    const int rows_cap = rs_rows_cap(net, tile, R);
    const size_t lds = rs_lds_bytes(net, tile, R, 1);
    const RsTable tb = {bounds, kk, ksize};
    for (int r0 = 0; r0 < n_rects; r0 += DL_TILE_GRID_Y) {
        const int nr = n_rects - r0 < DL_TILE_GRID_Y ? n_rects - r0 : DL_TILE_GRID_Y;
        dim3 grid((tile + R - 1) / R, nr);           // strips of a window as high as the tile; the strips past a shorter window return at once
        if (in_dtype == DL_BF16)
            hipLaunchKernelGGL(tile_paste_resample_kernel<bf16_t>, grid, dim3(256), lds, (hipStream_t)stream, (const bf16_t *)tiles, in_pstride, net, tile, tb, R, rows_cap,
                               rects + 8 * (size_t)r0, (uint8_t *)dst, (long long)dst_row_stride);
        else
            hipLaunchKernelGGL(tile_paste_resample_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, (const float *)tiles, in_pstride, net, tile, tb, R, rows_cap,
                               rects + 8 * (size_t)r0, (uint8_t *)dst, (long long)dst_row_stride);
        DL_CHECK_LAUNCH("dl_tile_paste_resample_u8");
    }
    return 0;
}

// ---- training batches from 8-bit dataset rows (deepliif/data/aligned_dataset.py:36-113 AlignedDataset.__getitem__ after Image.open(...).convert('RGB'):
// panel crop, then base_dataset.py:80-114 get_transform in PIL's order -- convert('L'), Image.resize, crop, FLIP_LEFT_RIGHT -- then ToTensor + Normalize as
// lut[], then engine.to_engine).  Same integer resize as above, but one table PER AXIS (panel w2 x h -> new_w x new_h; a null table = PIL skips that pass),
// a per-sample crop window and flip read from the device, and an LDS image that only holds the crop window's columns.
#define DL_TRAIN_CHUNK 16         // samples per launch: their row pointers travel as kernel arguments

struct TrainSrc {
    const uint8_t *row[DL_TRAIN_CHUNK];
    long long row_stride[DL_TRAIN_CHUNK];
};

__device__ __forceinline__ void train_src_of(const TrainSrc &src, int s, const uint8_t *&img, long long &row_stride) {
    img = src.row[0];
    row_stride = src.row_stride[0];
#pragma unroll
    for (int q = 1; q < DL_TRAIN_CHUNK; ++q)
        if (q == s) { img = src.row[q]; row_stride = src.row_stride[q]; }
}

// the r | g << 8 | b << 16 word of panel pixel (y, x); gray: PIL's convert('L') in all three bytes
__device__ __forceinline__ uint32_t train_pixel(const uint8_t *img, long long row_stride, int x_off, int y, int x, int gray) {
    const uint8_t *p = img + (long long)y * row_stride + 3ll * (x_off + x);
    const uint32_t r = p[0], g = p[1], b = p[2];
    if (gray) {
        const uint32_t l = (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16;
        return l | (l << 8) | (l << 16);
    }
    return r | (g << 8) | (b << 16);
}

// the per-sample record {crop_x, crop_y, flip}, clamped so that a wrong record cannot turn into an out-of-range read
__device__ __forceinline__ void train_params(const int32_t *params, int s, int new_w, int new_h, int cw, int ch, int &cx, int &cy, int &flip) {
    cx = params[3 * s];
    cy = params[3 * s + 1];
    flip = params[3 * s + 2] != 0;
    cx = cx < 0 ? 0 : (cx > new_w - cw ? new_w - cw : cx);
    cy = cy < 0 ? 0 : (cy > new_h - ch ? new_h - ch : cy);
}

// channels [c0, c0 + nch) of one output pixel <- lut[] of the word's bytes, channels up to zero_to <- 0 (as nchw_to_nhwc_kernel); one 8-channel vector
// store when the call owns the whole group
template <typename T>
__device__ __forceinline__ void train_store(T *o, uint32_t word, const float *__restrict__ lut, int c0, int nch, int zero_to) {
    if ((c0 & 7) == 0 && zero_to == c0 + 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < nch) v[k] = lut[(word >> (8 * k)) & 0xff];
        Vec8<T>::store(o + c0, v);
        return;
    }
    for (int k = 0; k < nch; ++k) store1<T>(o + c0 + k, lut[(word >> (8 * k)) & 0xff]);
    for (int c = c0 + nch; c < zero_to; ++c) store1<T>(o + c, 0.f);
}

// no resize on either axis: crop + flip + lut, one thread per output pixel, no LDS
template <typename T>
__global__ void __launch_bounds__(256) train_gather_kernel(TrainSrc src, int x_off, int w2, int h, int gray, const int32_t *__restrict__ params, int ch, int cw,
                                                           const float *__restrict__ lut, T *__restrict__ out, int out_pstride, int c0, int nch, int zero_to) {
    const int s = blockIdx.y;
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= ch * cw) return;
    const int oy = pix / cw, ox = pix - oy * cw;
    int cx, cy, flip;
    train_params(params, s, w2, h, cw, ch, cx, cy, flip);
    const uint8_t *img;
    long long row_stride;
    train_src_of(src, s, img, row_stride);
    const uint32_t word = train_pixel(img, row_stride, x_off, cy + oy, cx + (flip ? cw - 1 - ox : ox), gray);
    train_store<T>(out + ((long long)s * ch * cw + pix) * out_pstride, word, lut, c0, nch, zero_to);
}

// One workgroup = one sample and a strip of R rows of its crop window.  mid[rows_cap][cw]: the panel rows the strip's vertical taps reach (tby.bounds of
// the first and the last row; without a vertical table the strip's own rows), horizontally resized, columns crop_x .. crop_x + cw - 1 only.
template <typename T>
__global__ void __launch_bounds__(256) train_gather_resample_kernel(TrainSrc src, int x_off, int w2, int h, int gray, int new_w, RsTable tbx, int new_h, RsTable tby,
                                                                    const int32_t *__restrict__ params, int ch, int cw, int R, int rows_cap,
                                                                    const float *__restrict__ lut, T *__restrict__ out, int out_pstride, int c0, int nch,
                                                                    int zero_to) {
    extern __shared__ uint32_t rs_lds[];
    uint32_t *mid = rs_lds;
    const int s = blockIdx.y;
    const int y0 = blockIdx.x * R, y1 = y0 + R < ch ? y0 + R : ch;          // rows of the crop window
    if (y0 >= y1) return;
    int cx, cy, flip;
    train_params(params, s, new_w, new_h, cw, ch, cx, cy, flip);
    const uint8_t *img;
    long long row_stride;
    train_src_of(src, s, img, row_stride);
    int ya = cy + y0, rows = y1 - y0;
    if (tby.bounds) {
        int na, yb, nb;
        rs_taps(tby, cy + y0, h, ya, na);
        rs_taps(tby, cy + y1 - 1, h, yb, nb);
        rows = yb + nb - ya;
    }
    rows = rows < 0 ? 0 : (rows > rows_cap ? rows_cap : rows);
    for (int i = threadIdx.x; i < rows * cw; i += blockDim.x) {
        const int row = i / cw, xx = cx + (i - row * cw);
        if (!tbx.bounds) {
            mid[i] = train_pixel(img, row_stride, x_off, ya + row, xx, gray);
            continue;
        }
        int x0, n;
        rs_taps(tbx, xx, w2, x0, n);
        const int32_t *k = tbx.kk + (long long)xx * tbx.ksize;
        int a0 = 1 << (DL_RS_BITS - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < n; ++j) {
            const uint32_t m = train_pixel(img, row_stride, x_off, ya + row, x0 + j, gray);
            const int kj = k[j];
            a0 += (int)(m & 0xff) * kj;
            a1 += (int)((m >> 8) & 0xff) * kj;
            a2 += (int)((m >> 16) & 0xff) * kj;
        }
        mid[i] = rs_pack(a0, a1, a2);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (y1 - y0) * cw; i += blockDim.x) {
        const int ry = i / cw, ox = i - ry * cw;
        const int col = flip ? cw - 1 - ox : ox;
        uint32_t word = 0;
        if (tby.bounds) word = rs_vertical(tby, mid, cw, ya, rows, cy + y0 + ry, col, h);
        else if (ry < rows) word = mid[ry * cw + col];
        train_store<T>(out + (((long long)s * ch + (y0 + ry)) * cw + ox) * out_pstride, word, lut, c0, nch, zero_to);
    }
}

// strip height of the crop window and the LDS image it needs: rows_cap source rows of cw words
static int train_rows_cap(int h, int new_h, int resize_y, int R) { return resize_y ? rs_rows_cap(h, new_h, R) : R; }
static size_t train_lds_bytes(int h, int new_h, int resize_y, int cw, int R) { return 4ull * cw * (size_t)train_rows_cap(h, new_h, resize_y, R); }
static int train_strip_rows(int h, int new_h, int resize_y, int ch, int cw) {
    for (int R = ch < DL_RS_MAX_STRIP ? ch : DL_RS_MAX_STRIP; R >= 1; --R)
        if (train_lds_bytes(h, new_h, resize_y, cw, R) <= DL_RS_LDS_BYTES) return R;
    return 0;
}
// the checks on the geometry that dl_train_gather_u8 and dl_train_gather_supported share; panels = panel index + 1
static int train_geometry_ok(const char *who, int w2, int h, int panels, int new_w, int new_h, int ch, int cw) {
    if (w2 <= 0 || h <= 0 || new_w <= 0 || new_h <= 0 || ch <= 0 || cw <= 0 || panels <= 0)
        DL_FAIL("%s: empty problem (panel %dx%d -> %dx%d, crop %dx%d, panel index %d)", who, w2, h, new_w, new_h, cw, ch, panels - 1);
    if (cw > new_w || ch > new_h) DL_FAIL("%s: the crop window %dx%d does not fit the resized panel %dx%d", who, cw, ch, new_w, new_h);
    if (3ll * panels * w2 > 0x7fffffffll || (long long)ch * cw > 0x7fffffffll || (long long)new_w * rs_ksize(w2, new_w) > 0x7fffffffll ||
        (long long)new_h * rs_ksize(h, new_h) > 0x7fffffffll)
        DL_FAIL("%s: panel %dx%d (index %d) -> %dx%d, crop %dx%d overflows the kernel's 32-bit offsets", who, w2, h, panels - 1, new_w, new_h, cw, ch);
    return 0;
}

extern "C" int dl_train_gather_supported(int w2, int h, int new_w, int new_h, int ch, int cw) {
    if (train_geometry_ok("dl_train_gather_supported", w2, h, 1, new_w, new_h, ch, cw)) return 0;
    if (new_w == w2 && new_h == h) return ch < DL_RS_MAX_STRIP ? ch : DL_RS_MAX_STRIP;          // plain kernel, no LDS: any strip height is accepted
    const int R = train_strip_rows(h, new_h, new_h != h, ch, cw);
    if (R < 1)
        dl_set_error("dl_train_gather_supported: %d -> %d rows at a crop width of %d needs %zu bytes of LDS for one output row, the limit is %d", h, new_h, cw,
                     train_lds_bytes(h, new_h, new_h != h, cw, 1), DL_RS_LDS_BYTES);
    return R < 1 ? 0 : R;
}

extern "C" int dl_train_gather_u8(const void *const *rows, const int64_t *row_strides, int n, int w2, int h, int panel, int gray, int new_w, const int32_t *xbounds,
                                  const int32_t *xkk, int xksize, int new_h, const int32_t *ybounds, const int32_t *ykk, int yksize, const int32_t *params, int ch,
                                  int cw, int strip_rows, const float *lut, int out_dtype, void *out, int out_pstride, int out_c0, int zero_pad_to, void *stream) {
    if (n <= 0) DL_FAIL("dl_train_gather_u8: empty problem (n=%d)", n);
    if (panel < 0) DL_FAIL("dl_train_gather_u8: panel index %d", panel);
    if (train_geometry_ok("dl_train_gather_u8", w2, h, panel + 1, new_w, new_h, ch, cw)) return -1;
    if (!rows || !row_strides || !params || !lut || !out) DL_FAIL("dl_train_gather_u8: rows, row_strides, params, lut and out are required");
    if (out_dtype != DL_F32 && out_dtype != DL_BF16) DL_FAIL("dl_train_gather_u8: dtype %d", out_dtype);
    const int nch = gray ? 1 : 3;
    if (out_c0 < 0 || out_c0 + nch > out_pstride || (zero_pad_to > out_c0 + nch && zero_pad_to > out_pstride))
        DL_FAIL("dl_train_gather_u8: bad channel geometry (%d channels at %d, zero to %d, pstride=%d)", nch, out_c0, zero_pad_to, out_pstride);
    if (out_pstride % 8) DL_FAIL("dl_train_gather_u8: engine tensors have a multiple of 8 padded channels (pstride=%d)", out_pstride);
    if ((long long)n * ch * cw * out_pstride > 0x7fffffffffffll) DL_FAIL("dl_train_gather_u8: output of %d x %d x %d x %d elements is too large", n, ch, cw, out_pstride);
    for (int i = 0; i < n; ++i)
        if (!rows[i] || row_strides[i] < 3ll * (panel + 1) * w2) DL_FAIL("dl_train_gather_u8: sample %d: null row or a row stride (%lld) shorter than %d panels of %d pixels",
                                                                         i, (long long)row_strides[i], panel + 1, w2);
    const int resize_x = new_w != w2, resize_y = new_h != h;
    if (resize_x != (xbounds != nullptr) || resize_x != (xkk != nullptr))
        DL_FAIL("dl_train_gather_u8: width %d -> %d %s (PIL skips a pass that does not change the size)", w2, new_w, resize_x ? "needs a table" : "takes no table");
    if (resize_y != (ybounds != nullptr) || resize_y != (ykk != nullptr))
        DL_FAIL("dl_train_gather_u8: height %d -> %d %s (PIL skips a pass that does not change the size)", h, new_h, resize_y ? "needs a table" : "takes no table");
    if (resize_x && xksize != rs_ksize(w2, new_w)) DL_FAIL("dl_train_gather_u8: xksize=%d, the table of %d -> %d has %d", xksize, w2, new_w, rs_ksize(w2, new_w));
    if (resize_y && yksize != rs_ksize(h, new_h)) DL_FAIL("dl_train_gather_u8: yksize=%d, the table of %d -> %d has %d", yksize, h, new_h, rs_ksize(h, new_h));
    if (strip_rows < 0) DL_FAIL("dl_train_gather_u8: strip_rows=%d", strip_rows);
    int R = 0, rows_cap = 0;
    size_t lds = 0;
    if (resize_x || resize_y) {
        if (strip_rows > ch) DL_FAIL("dl_train_gather_u8: strips of %d rows in a crop window of %d rows", strip_rows, ch);
        R = strip_rows > 0 ? strip_rows : train_strip_rows(h, new_h, resize_y, ch, cw);
        // the library's choice: shorter strips while the batch gives fewer than two workgroups per CU (each halving repeats at most ksize source rows per strip)
        while (strip_rows == 0 && R > 8 && (long long)n * ((ch + R - 1) / R) < 512) R = (R + 1) / 2;
        if (R < 1 || train_lds_bytes(h, new_h, resize_y, cw, R) > DL_RS_LDS_BYTES)
            DL_FAIL("dl_train_gather_u8: %d -> %d rows at a crop width of %d with strips of %d rows needs %zu bytes of LDS, the limit is %d", h, new_h, cw, R < 1 ? 1 : R,
                    train_lds_bytes(h, new_h, resize_y, cw, R < 1 ? 1 : R), DL_RS_LDS_BYTES);
        rows_cap = train_rows_cap(h, new_h, resize_y, R);
        lds = train_lds_bytes(h, new_h, resize_y, cw, R);
    }
    const RsTable tbx = {xbounds, xkk, xksize}, tby = {ybounds, ykk, yksize};
    const int zero_to = zero_pad_to > out_c0 + nch ? zero_pad_to : out_c0 + nch;
    for (int s0 = 0; s0 < n; s0 += DL_TRAIN_CHUNK) {
        const int ns = n - s0 < DL_TRAIN_CHUNK ? n - s0 : DL_TRAIN_CHUNK;
        TrainSrc src;
        for (int i = 0; i < DL_TRAIN_CHUNK; ++i) {
            src.row[i] = (const uint8_t *)rows[s0 + (i < ns ? i : 0)];
            src.row_stride[i] = row_strides[s0 + (i < ns ? i : 0)];
        }
        const size_t o0 = (size_t)s0 * ch * cw * out_pstride;
        const int32_t *pr = params + 3 * (size_t)s0;
        if (!resize_x && !resize_y) {
            dim3 grid((unsigned)(((long long)ch * cw + 255) / 256), ns);
            if (out_dtype == DL_BF16)
                hipLaunchKernelGGL(train_gather_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, src, panel * w2, w2, h, gray, pr, ch, cw, lut, (bf16_t *)out + o0,
                                   out_pstride, out_c0, nch, zero_to);
            else
                hipLaunchKernelGGL(train_gather_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, src, panel * w2, w2, h, gray, pr, ch, cw, lut, (float *)out + o0,
                                   out_pstride, out_c0, nch, zero_to);
        } else {
            dim3 grid((ch + R - 1) / R, ns);
            if (out_dtype == DL_BF16)
                hipLaunchKernelGGL(train_gather_resample_kernel<bf16_t>, grid, dim3(256), lds, (hipStream_t)stream, src, panel * w2, w2, h, gray, new_w, tbx, new_h, tby, pr,
                                   ch, cw, R, rows_cap, lut, (bf16_t *)out + o0, out_pstride, out_c0, nch, zero_to);
            else
                hipLaunchKernelGGL(train_gather_resample_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, src, panel * w2, w2, h, gray, new_w, tbx, new_h, tby, pr,
                                   ch, cw, R, rows_cap, lut, (float *)out + o0, out_pstride, out_c0, nch, zero_to);
        }
        DL_CHECK_LAUNCH("dl_train_gather_u8");
    }
    return 0;
}
