// spectral.hip -- spectral normalisation of conv weights (torch.nn.utils.parametrizations._SpectralNorm, networks.py:757-765 of the reference):
// one power iteration, sigma = u^T (M v), the effective weight W / sigma, and the projection of the effective-weight gradient back onto W.
// fp32 throughout.  A network's layers are batched through a device-resident table of job records (one per layer) and host-built
// workgroup tables, so the number of launches never depends on the number of layers.  See include/deepliif_hip.h.
//
// M is the [R = Cout] x [C = Cin*KH*KW] matrix view of the weight: element (r, c) of a Conv2d weight (dim 0) sits at r*C + c, of a
// ConvTranspose2d weight [Cin][Cout][KH][KW] (dim 1) at ((c / KK)*R + r)*KK + c % KK.  The effective weight and both gradients share W's layout.
//
// Work unit of the matrix passes: a tile of SP_TR rows x SP_TC columns, one workgroup of 256 threads, each thread owning 4 consecutive columns.
// Every cross-workgroup sum goes through per-tile partials in the caller's scratch that the NEXT launch adds up in index order: no atomics,
// two runs give the same bits.  Forward, iterating (7 launches):
//   1 mv      pt[ct][r]  = sum_{c in tile} M[r][c] v[c]
//   2 rowsum  t[r]       = sum_ct pt[ct][r];  tsq[rt] = sum_{r in row tile} t[r]^2
//   3 mtv     u = t / max(sqrt(sum_rt tsq), eps)  -> _u, snapshot;   ps[rt][c] = sum_{r in tile} M[r][c] u[r]
//   4 colsum  s[c]       = sum_rt ps[rt][c];  ssq[ct] = sum_{c in column tile} s[c]^2
//   5 mv      v = s / max(sqrt(sum_ct ssq), eps)  -> _v, snapshot;   pt[ct][r] = sum_c M[r][c] v[c]
//   6 rowdot  sigp[rt]   = sum_{r in row tile} u[r] * sum_ct pt[ct][r]
//   7 scale   sigma = sum_rt sigp -> sigma[job];  weff = W / sigma
// Not iterating (3 launches): pass 5 with u, v read from the buffers (and copied to the snapshots), then 6 and 7.
#include "common.h"

constexpr int SP_TR = 16;                 // rows of a tile
constexpr int SP_TC = 1024;               // columns of a tile: 256 threads x 4
constexpr float SP_EPS = 1e-12f;          // _SpectralNorm's eps

struct SpJob {
    const float *w;                       // master weight (parametrizations.weight.original)
    float *u, *v;                         // _u [R], _v [C]: updated in place when iterating
    float *weff;                          // out: W / sigma, W's shape and layout
    float *u_snap, *v_snap, *sigma;       // out: the u, v, sigma of THIS call (what its backward needs)
    const float *g;                       // backward: gradient w.r.t. weff
    float *grad;                          // backward: gradient w.r.t. w
    long long scratch_off;                // this job's region of the scratch buffer, in floats
    int R, C, KK, dim;
    int vec;                              // dim 0, C % 4 == 0 and every pointer 16-byte aligned: 16-byte accesses
    int nrt, nct;                         // row / column tiles
    int pad_;
};

// scratch region of a job, in floats
struct SpScratch {
    size_t pt, t, tsq, ps, s, ssq, sigp, dotp, total;
    __host__ __device__ SpScratch(int R, int C, int nrt, int nct) {
        size_t o = 0;
        pt = o; o += (size_t)nct * R;
        t = o; o += R;
        tsq = o; o += nrt;
        ps = o; o += (size_t)nrt * C;
        s = o; o += C;
        ssq = o; o += nct;
        sigp = o; o += nrt;
        dotp = o; o += (size_t)nrt * nct;
        total = (o + 3) / 4 * 4;
    }
};

__device__ __forceinline__ size_t sp_addr(const SpJob &j, int r, int c) {
    return j.dim == 0 ? (size_t)r * j.C + c : ((size_t)(c / j.KK) * j.R + r) * j.KK + (c % j.KK);
}

// 4 consecutive columns c .. c+3 of row r (0 beyond C)
__device__ __forceinline__ void sp_load4(const SpJob &j, const float *base, int r, int c, float (&m)[4]) {
    if (j.vec) {            // C % 4 == 0 and c % 4 == 0: all four inside or all four outside
        if (c < j.C) {
            const float4 q = *reinterpret_cast<const float4 *>(base + (size_t)r * j.C + c);
            m[0] = q.x; m[1] = q.y; m[2] = q.z; m[3] = q.w;
        } else {
            m[0] = m[1] = m[2] = m[3] = 0.f;
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = (c + e < j.C) ? base[sp_addr(j, r, c + e)] : 0.f;
}

__device__ __forceinline__ void sp_store4(const SpJob &j, float *base, int r, int c, const float (&m)[4]) {
    if (j.vec) {
        if (c < j.C) *reinterpret_cast<float4 *>(base + (size_t)r * j.C + c) = make_float4(m[0], m[1], m[2], m[3]);
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (c + e < j.C) base[sp_addr(j, r, c + e)] = m[e];
}

__device__ __forceinline__ void sp_load_job(SpJob &dst, const char *jobs, int job) {
    const int *src = reinterpret_cast<const int *>(jobs + (size_t)job * sizeof(SpJob));
    int *d = reinterpret_cast<int *>(&dst);
    for (int i = threadIdx.x; i < (int)(sizeof(SpJob) / sizeof(int)); i += blockDim.x) d[i] = src[i];
    __syncthreads();
}

// sum of n partials in index order (every thread of every workgroup that needs it computes the same bits)
__device__ __forceinline__ float sp_sum_ordered(const float *p, int n) {
    float a = 0.f;
    for (int i = 0; i < n; ++i) a += p[i];
    return a;
}

// ---- passes 1 / 5: pt[ct][r] = sum_{c in tile} M[r][c] v[c].  FROM_S: v = s / |s| (pass 5, written to _v and the snapshot by the rt == 0 tiles);
// otherwise v is read from the buffer, and with `snapshot` set (the non-iterating call) u and v are copied to the snapshots on the way.
template <bool FROM_S>
__global__ void __launch_bounds__(256) sp_mv_kernel(const char *jobs, const int2 *tab, float *scratch, int snapshot) {
    __shared__ SpJob j;
    __shared__ float red[4][SP_TR];
    const int2 bt = tab[blockIdx.x];
    sp_load_job(j, jobs, bt.x);
    const SpScratch S(j.R, j.C, j.nrt, j.nct);
    float *sc = scratch + j.scratch_off;
    const int rt = bt.y / j.nct, ct = bt.y - rt * j.nct;
    const int r0 = rt * SP_TR, c = ct * SP_TC + threadIdx.x * 4;
    float vv[4];
    if (FROM_S) {
        const float nrm = fmaxf(sqrtf(sp_sum_ordered(sc + S.ssq, j.nct)), SP_EPS);
#pragma unroll
        for (int e = 0; e < 4; ++e) vv[e] = (c + e < j.C) ? sc[S.s + c + e] / nrm : 0.f;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) vv[e] = (c + e < j.C) ? j.v[c + e] : 0.f;
    }
    if (rt == 0 && (FROM_S || snapshot)) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < j.C) {
                if (FROM_S) j.v[c + e] = vv[e];
                j.v_snap[c + e] = vv[e];
            }
    }
    if (!FROM_S && snapshot && ct == 0 && threadIdx.x < SP_TR && r0 + threadIdx.x < j.R) j.u_snap[r0 + threadIdx.x] = j.u[r0 + threadIdx.x];
    float acc[SP_TR];
#pragma unroll
    for (int i = 0; i < SP_TR; ++i) {
        float m[4] = {0.f, 0.f, 0.f, 0.f};
        if (r0 + i < j.R) sp_load4(j, j.w, r0 + i, c, m);
        acc[i] = m[0] * vv[0] + m[1] * vv[1] + m[2] * vv[2] + m[3] * vv[3];
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < SP_TR; ++i) {
        const float s = wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < SP_TR && r0 + threadIdx.x < j.R)
        sc[S.pt + (size_t)ct * j.R + r0 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- passes 2 / 6: per row tile, t[r] = sum_ct pt[ct][r]; DOT: sigp[rt] = sum_r u_snap[r] t[r], else t is stored and tsq[rt] = sum_r t[r]^2
template <bool DOT>
__global__ void __launch_bounds__(64) sp_rowsum_kernel(const char *jobs, const int2 *tab, float *scratch) {
    __shared__ SpJob j;
    __shared__ float part[SP_TR];
    const int2 bt = tab[blockIdx.x];
    sp_load_job(j, jobs, bt.x);
    const SpScratch S(j.R, j.C, j.nrt, j.nct);
    float *sc = scratch + j.scratch_off;
    const int rt = bt.y, r = rt * SP_TR + threadIdx.x;
    if (threadIdx.x < SP_TR) {
        float t = 0.f;
        if (r < j.R) {
            for (int ct = 0; ct < j.nct; ++ct) t += sc[S.pt + (size_t)ct * j.R + r];
            if (!DOT) sc[S.t + r] = t;
        }
        part[threadIdx.x] = (r < j.R) ? (DOT ? j.u_snap[r] * t : t * t) : 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f;
        for (int i = 0; i < SP_TR; ++i) a += part[i];
        sc[(DOT ? S.sigp : S.tsq) + rt] = a;
    }
}

// ---- pass 3: u = t / |t| (stored by the ct == 0 tiles); ps[rt][c] = sum_{r in tile} M[r][c] u[r]
__global__ void __launch_bounds__(256) sp_mtv_kernel(const char *jobs, const int2 *tab, float *scratch) {
    __shared__ SpJob j;
    const int2 bt = tab[blockIdx.x];
    sp_load_job(j, jobs, bt.x);
    const SpScratch S(j.R, j.C, j.nrt, j.nct);
    float *sc = scratch + j.scratch_off;
    const int rt = bt.y / j.nct, ct = bt.y - rt * j.nct;
    const int r0 = rt * SP_TR, c = ct * SP_TC + threadIdx.x * 4;
    const float nrm = fmaxf(sqrtf(sp_sum_ordered(sc + S.tsq, j.nrt)), SP_EPS);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < SP_TR; ++i) {
        if (r0 + i >= j.R) break;
        const float u = sc[S.t + r0 + i] / nrm;
        float m[4];
        sp_load4(j, j.w, r0 + i, c, m);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += m[e] * u;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (c + e < j.C) sc[S.ps + (size_t)rt * j.C + c + e] = acc[e];
    if (ct == 0 && threadIdx.x < SP_TR && r0 + threadIdx.x < j.R) {
        const float u = sc[S.t + r0 + threadIdx.x] / nrm;
        j.u[r0 + threadIdx.x] = u;
        j.u_snap[r0 + threadIdx.x] = u;
    }
}

// ---- pass 4: per column tile, s[c] = sum_rt ps[rt][c]; ssq[ct] = sum_c s[c]^2
__global__ void __launch_bounds__(256) sp_colsum_kernel(const char *jobs, const int2 *tab, float *scratch) {
    __shared__ SpJob j;
    __shared__ float red[4];
    const int2 bt = tab[blockIdx.x];
    sp_load_job(j, jobs, bt.x);
    const SpScratch S(j.R, j.C, j.nrt, j.nct);
    float *sc = scratch + j.scratch_off;
    const int ct = bt.y, c = ct * SP_TC + threadIdx.x * 4;
    float sq = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (c + e >= j.C) break;
        float s = 0.f;
        for (int rt = 0; rt < j.nrt; ++rt) s += sc[S.ps + (size_t)rt * j.C + c + e];
        sc[S.s + c + e] = s;
        sq += s * s;
    }
    sq = wave_sum(sq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) sc[S.ssq + ct] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- pass 7: weff = W / sigma
__global__ void __launch_bounds__(256) sp_scale_kernel(const char *jobs, const int2 *tab, float *scratch) {
    __shared__ SpJob j;
    const int2 bt = tab[blockIdx.x];
    sp_load_job(j, jobs, bt.x);
    const SpScratch S(j.R, j.C, j.nrt, j.nct);
    const float *sc = scratch + j.scratch_off;
    const int rt = bt.y / j.nct, ct = bt.y - rt * j.nct;
    const int r0 = rt * SP_TR, c = ct * SP_TC + threadIdx.x * 4;
    const float sigma = sp_sum_ordered(sc + S.sigp, j.nrt);
    if (bt.y == 0 && threadIdx.x == 0) *j.sigma = sigma;
#pragma unroll 4
    for (int i = 0; i < SP_TR; ++i) {
        if (r0 + i >= j.R) break;
        float m[4];
        sp_load4(j, j.w, r0 + i, c, m);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = m[e] / sigma;
        sp_store4(j, j.weff, r0 + i, c, m);
    }
}

// ---- backward 1: dotp[tile] = sum_{tile} G * Weff
__global__ void __launch_bounds__(256) sp_dot_kernel(const char *jobs, const int2 *tab, float *scratch) {
    __shared__ SpJob j;
    __shared__ float red[4];
    const int2 bt = tab[blockIdx.x];
    sp_load_job(j, jobs, bt.x);
    const SpScratch S(j.R, j.C, j.nrt, j.nct);
    float *sc = scratch + j.scratch_off;
    const int rt = bt.y / j.nct, ct = bt.y - rt * j.nct;
    const int r0 = rt * SP_TR, c = ct * SP_TC + threadIdx.x * 4;
    float a = 0.f;
#pragma unroll 4
    for (int i = 0; i < SP_TR; ++i) {
        if (r0 + i >= j.R) break;
        float g[4], m[4];
        sp_load4(j, j.g, r0 + i, c, g);
        sp_load4(j, j.weff, r0 + i, c, m);
        a += (g[0] * m[0] + g[1] * m[1]) + (g[2] * m[2] + g[3] * m[3]);
    }
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) sc[S.dotp + bt.y] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- backward 2: grad (+)= (G - <G, Weff> u v^T) / sigma
__global__ void __launch_bounds__(256) sp_project_kernel(const char *jobs, const int2 *tab, float *scratch, int accumulate) {
    __shared__ SpJob j;
    const int2 bt = tab[blockIdx.x];
    sp_load_job(j, jobs, bt.x);
    const SpScratch S(j.R, j.C, j.nrt, j.nct);
    const float *sc = scratch + j.scratch_off;
    const int rt = bt.y / j.nct, ct = bt.y - rt * j.nct;
    const int r0 = rt * SP_TR, c = ct * SP_TC + threadIdx.x * 4;
    const float d = sp_sum_ordered(sc + S.dotp, j.nrt * j.nct);
    const float sigma = *j.sigma;
    float vv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) vv[e] = (c + e < j.C) ? j.v_snap[c + e] : 0.f;
#pragma unroll 4
    for (int i = 0; i < SP_TR; ++i) {
        if (r0 + i >= j.R) break;
        const float du = d * j.u_snap[r0 + i];
        float g[4], o[4] = {0.f, 0.f, 0.f, 0.f};
        sp_load4(j, j.g, r0 + i, c, g);
        if (accumulate) sp_load4(j, j.grad, r0 + i, c, o);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += (g[e] - du * vv[e]) / sigma;
        sp_store4(j, j.grad, r0 + i, c, o);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
static inline int sp_nrt(int R) { return (R + SP_TR - 1) / SP_TR; }
static inline int sp_nct(int C) { return (C + SP_TC - 1) / SP_TC; }

extern "C" size_t dl_spectral_job_bytes(void) { return sizeof(SpJob); }

extern "C" size_t dl_spectral_scratch_floats(int rows, int cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return SpScratch(rows, cols, sp_nrt(rows), sp_nct(cols)).total;
}

extern "C" int dl_spectral_job_fill(const float *w, int rows, int cols, int kk, int dim, float *u, float *v, float *weff, float *u_snap, float *v_snap,
                                    float *sigma, const float *g, float *grad, int64_t scratch_off, void *job_host) {
    static_assert(sizeof(SpJob) % 16 == 0, "job records are copied to LDS as ints and sit back to back");
    if (!job_host) DL_FAIL("dl_spectral_job_fill: null job record");
    if (!w || !u || !v || !weff || !u_snap || !v_snap || !sigma) DL_FAIL("dl_spectral_job_fill: null argument");
    if ((g == nullptr) != (grad == nullptr)) DL_FAIL("dl_spectral_job_fill: g and grad go together");
    if (rows <= 0 || cols <= 0 || kk <= 0 || cols % kk) DL_FAIL("dl_spectral_job_fill: bad matrix %d x %d (kernel %d)", rows, cols, kk);
    if (dim != 0 && dim != 1) DL_FAIL("dl_spectral_job_fill: dim %d (0: Conv2d, 1: ConvTranspose2d)", dim);
    if (scratch_off < 0 || scratch_off % 4) DL_FAIL("dl_spectral_job_fill: scratch offset %lld", (long long)scratch_off);
    SpJob j;
    memset(&j, 0, sizeof(j));
    j.w = w; j.u = u; j.v = v; j.weff = weff; j.u_snap = u_snap; j.v_snap = v_snap; j.sigma = sigma; j.g = g; j.grad = grad;
    j.scratch_off = scratch_off;
    j.R = rows; j.C = cols; j.KK = kk; j.dim = dim;
    j.nrt = sp_nrt(rows); j.nct = sp_nct(cols);
    if ((long long)j.nrt * j.nct > 0x3fffffffLL) DL_FAIL("dl_spectral_job_fill: matrix too large");
    const uintptr_t al = (uintptr_t)w | (uintptr_t)weff | (uintptr_t)g | (uintptr_t)grad;
    j.vec = (dim == 0 && cols % 4 == 0 && al % 16 == 0) ? 1 : 0;
    memcpy(job_host, &j, sizeof(j));
    return 0;
}

// Workgroup table of one grid shape over `count` back-to-back host records: int32 pairs {job, index}; kind 0: one entry per tile (index = rt * nct + ct),
// 1: per row tile, 2: per column tile.  tab_host = NULL returns the entry count.
extern "C" int dl_spectral_blocks(const void *jobs_host, int count, int kind, int32_t *tab_host) {
    if (!jobs_host || count < 0 || kind < 0 || kind > 2) DL_FAIL("dl_spectral_blocks: bad arguments");
    long n = 0;
    for (int i = 0; i < count; ++i) {
        SpJob j;
        memcpy(&j, (const char *)jobs_host + (size_t)i * sizeof(SpJob), sizeof(j));
        const long m = kind == 0 ? (long)j.nrt * j.nct : (kind == 1 ? j.nrt : j.nct);
        for (long t = 0; t < m; ++t, ++n)
            if (tab_host) { tab_host[2 * n] = i; tab_host[2 * n + 1] = (int32_t)t; }
    }
    if (n > 0x7fffffffL) DL_FAIL("dl_spectral_blocks: too many workgroups");
    return (int)n;
}

extern "C" int dl_spectral_forward(const void *jobs_dev, int count, const int32_t *tiles_dev, int ntiles, const int32_t *rows_dev, int nrows,
                                   const int32_t *cols_dev, int ncols, float *scratch, int do_power_iteration, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (count <= 0) return 0;
    if (!jobs_dev || !tiles_dev || !rows_dev || !cols_dev || !scratch || ntiles <= 0 || nrows <= 0 || ncols <= 0) DL_FAIL("dl_spectral_forward: bad arguments");
    const char *jobs = reinterpret_cast<const char *>(jobs_dev);
    const int2 *tiles = reinterpret_cast<const int2 *>(tiles_dev), *rows = reinterpret_cast<const int2 *>(rows_dev), *cols = reinterpret_cast<const int2 *>(cols_dev);
    if (do_power_iteration) {
        hipLaunchKernelGGL(sp_mv_kernel<false>, dim3(ntiles), dim3(256), 0, stream, jobs, tiles, scratch, 0);
        hipLaunchKernelGGL(sp_rowsum_kernel<false>, dim3(nrows), dim3(64), 0, stream, jobs, rows, scratch);
        hipLaunchKernelGGL(sp_mtv_kernel, dim3(ntiles), dim3(256), 0, stream, jobs, tiles, scratch);
        hipLaunchKernelGGL(sp_colsum_kernel, dim3(ncols), dim3(256), 0, stream, jobs, cols, scratch);
        hipLaunchKernelGGL(sp_mv_kernel<true>, dim3(ntiles), dim3(256), 0, stream, jobs, tiles, scratch, 0);
    } else {
        hipLaunchKernelGGL(sp_mv_kernel<false>, dim3(ntiles), dim3(256), 0, stream, jobs, tiles, scratch, 1);
    }
    hipLaunchKernelGGL(sp_rowsum_kernel<true>, dim3(nrows), dim3(64), 0, stream, jobs, rows, scratch);
    hipLaunchKernelGGL(sp_scale_kernel, dim3(ntiles), dim3(256), 0, stream, jobs, tiles, scratch);
    DL_CHECK_LAUNCH("dl_spectral_forward");
    return 0;
}

extern "C" int dl_spectral_backward(const void *jobs_dev, int count, const int32_t *tiles_dev, int ntiles, float *scratch, int accumulate, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (count <= 0 || ntiles <= 0) return 0;
    if (!jobs_dev || !tiles_dev || !scratch) DL_FAIL("dl_spectral_backward: bad arguments");
    const char *jobs = reinterpret_cast<const char *>(jobs_dev);
    const int2 *tiles = reinterpret_cast<const int2 *>(tiles_dev);
    hipLaunchKernelGGL(sp_dot_kernel, dim3(ntiles), dim3(256), 0, stream, jobs, tiles, scratch);
    hipLaunchKernelGGL(sp_project_kernel, dim3(ntiles), dim3(256), 0, stream, jobs, tiles, scratch, accumulate ? 1 : 0);
    DL_CHECK_LAUNCH("dl_spectral_backward");
    return 0;
}
