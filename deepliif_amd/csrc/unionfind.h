// unionfind.h -- the lock-free union-find of the connected-component labellings (postproc.hip: background and cell passes; stat.hip: the
// equal-value labelling of the evaluation metrics).  Links go from the larger root to the smaller one (atomicMin), so a component's root is
// its SMALLEST pixel index = its first pixel in raster order, whatever the order the links were made in.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int uf_find(const int *L, int a) {
    int b = __atomic_load_n(L + a, __ATOMIC_RELAXED);
    while (b != a) { a = b; b = __atomic_load_n(L + a, __ATOMIC_RELAXED); }
    return a;
}
__device__ __forceinline__ void uf_union(int *L, int a, int b) {
    bool done;
    do {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a < b) { const int old = atomicMin(L + b, a); done = (old == b); b = old; }
        else if (b < a) { const int old = atomicMin(L + a, b); done = (old == a); a = old; }
        else done = true;
    } while (!done);
}

// Initial label of an active pixel: the first pixel of its horizontal run INSIDE this wavefront (64 consecutive pixel indices, cut at row
// starts).  A run of n pixels then needs n/64 horizontal links instead of n, and every find() starts one hop from a run head: the image
// border's UNKNOWN region (usually one giant component) made the plain "label = own index" start 12x slower on a 2048 x 2048 image.
// Every lane of the wavefront must call it (ballots).
__device__ __forceinline__ int pp_run_head(bool active, int p, int x) {
    const unsigned long long act = __ballot(active);
    const unsigned long long brk = ~act | __ballot(x == 0);        // lanes that cannot be continued INTO: inactive, or first of a row
    const int lane = threadIdx.x & 63;
    if (!active) return -1;
    // highest lane l <= lane that starts a run: l is active and (l == 0 or lane l-1 inactive or x(l) == 0)
    const unsigned long long starts = act & ((~act << 1) | 1ull | __ballot(x == 0));
    const unsigned long long below = starts & (lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1));
    (void)brk;
    return p - (lane - (63 - __builtin_clzll(below)));
}

// The same for runs of EQUAL value (v > 0 is active): a run is also cut where the value changes.
__device__ __forceinline__ int uf_value_run_head(int v, int p, int x) {
    const int lane = threadIdx.x & 63;
    const int left = __shfl_up(v, 1, 64);
    const bool active = v > 0;
    const unsigned long long starts = __ballot(active && (lane == 0 || x == 0 || left != v));
    if (!active) return -1;
    const unsigned long long below = starts & (lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1));
    return p - (lane - (63 - __builtin_clzll(below)));
}
