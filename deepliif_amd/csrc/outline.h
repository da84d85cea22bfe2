// outline.h -- the cell-outline trace and its encoders, shared by postproc.hip (one lane per cell: pp_outline_count_kernel,
// pp_outline_emit_kernel) and the host check outline_check.cpp (tests/test_outline_host.py runs the same two lane functions cell by cell
// on the CPU against postprocessing.get_cell_boundary / make_simple_contour / encode_cell_data_v4).
//
// get_cell_boundary (:491-581) + make_simple_contour (:584-634) + encode_cell_data_v4 (:752-848) of deepliif/postprocessing.py.  The trace is the
// reference's: Moore neighbourhood, clockwise, ring order (-1,-1) (0,-1) (1,-1) (1,0) (1,1) (0,1) (-1,1) (-1,0); the pixel that precedes
// the start is the first cell neighbour met COUNTER-clockwise from ring index 6; the search for the next pixel starts one past the
// pixel we came from (ring index of the last move + 5); the trace ends when the start is re-entered from that first predecessor, and
// that closing pair is not part of the outline.  Nothing is stored per outline point: with d(i) the move into point i and d(n) the
// closing move, point i >= 1 is kept iff d(i) != d(i+1) (the sign pairs make_simple_contour compares ARE the ring directions, the
// points being 8-neighbours), and the points dropped between two kept ones lie on one straight run, which is what the chain code
// spells: ceil(s / 10) characters for s steps.  Point 0 is always kept; the run that closes the outline is not encoded.
// Bound: (pixel, ring index of its predecessor) determines the rest of the walk and the step is invertible, so the walk is a cycle
// through the start state that visits no state twice: at most 8 * size moves.  The loop stops at 8 * size + 8 and reports OPEN.
#pragma once
#include "common.h"

#define PPO_HD __host__ __device__ __forceinline__
#define PPO_DX(k) ((int)((0x06A4u >> (2 * (k))) & 3u) - 1)
#define PPO_DY(k) ((int)((0x6A40u >> (2 * (k))) & 3u) - 1)

PPO_HD int ppo_max(int a, int b) { return a > b ? a : b; }
PPO_HD int ppo_min(int a, int b) { return a < b ? a : b; }

PPO_HD bool ppo_cell(const uint8_t *mask, int H, int W, int x, int y) {
    return (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H && mask[(size_t)y * W + x] != 0;
}

// Sink: point(x, y) = a kept point, in order; run(s, k) = the s >= 1 steps in ring direction k that led to the point just reported;
// visit(x, y) = every outline point after the first (for the bounding box)
template <class Sink>
__host__ __device__ int ppo_trace(const uint8_t *mask, int H, int W, int sx, int sy, int size, Sink &s) {
    if ((unsigned)sx >= (unsigned)W || (unsigned)sy >= (unsigned)H) return DL_PP_OUTLINE_OUTSIDE;
    if (mask[(size_t)sy * W + sx] == 0) return DL_PP_OUTLINE_BACKGROUND;
    int k0 = 6;
    while (k0 >= 0 && !ppo_cell(mask, H, W, sx + PPO_DX(k0), sy + PPO_DY(k0))) --k0;
    s.point(sx, sy);
    if (k0 < 0) return DL_PP_OUTLINE_OK;                              // the one-pixel cell
    const long long limit = 8ll * (size > 0 ? size : 0) + 8;
    int x = sx, y = sy, k = (k0 + 1) & 7, last = -1, run = 0;
    for (long long m = 0; m < limit; ++m) {
        int t = 0;
        while (t < 8 && !ppo_cell(mask, H, W, x + PPO_DX(k), y + PPO_DY(k))) { k = (k + 1) & 7; ++t; }
        if (t == 8) return DL_PP_OUTLINE_OPEN;                        // (the pixel we came from is a cell: not reached)
        const int nx = x + PPO_DX(k), ny = y + PPO_DY(k);
        if (last >= 0 && k != last) { s.point(x, y); s.run(run, last); run = 0; }
        if (nx == sx && ny == sy && ((k + 4) & 7) == k0) return DL_PP_OUTLINE_OK;
        s.visit(nx, ny);
        x = nx; y = ny; last = k; ++run;
        k = (k + 5) & 7;
    }
    return DL_PP_OUTLINE_OPEN;
}

PPO_HD int ppo_digits(int v) {                    // to_base92 (:685-727): no digit for v <= 0
    int n = 0;
    while (v > 0) { v /= 92; ++n; }
    return n;
}
// the widths of one encoded cell: size | class (>= 2) | top-left pair | the six offsets
struct PPOWidths { int size, cls, tl, off; };
PPO_HD PPOWidths ppo_widths(const int *c, int x0, int y0, int x1, int y1, int ox, int oy) {
    PPOWidths w;
    w.size = ppo_max(ppo_digits(c[2]), 1);
    w.cls = ppo_max(ppo_digits(c[4] * 2 + (c[3] != 0)), 2);
    w.tl = ppo_max(ppo_max(ppo_digits(x0 + ox), ppo_digits(y0 + oy)), 1);
    int o = ppo_max(ppo_digits(x1 - x0), ppo_digits(y1 - y0));
    o = ppo_max(o, ppo_max(ppo_digits(c[5] - x0), ppo_digits(c[6] - y0)));
    o = ppo_max(o, ppo_max(ppo_digits(c[0] - x0), ppo_digits(c[1] - y0)));
    w.off = ppo_max(o, 1);
    return w;
}

struct PPOCountSink {
    int x0, y0, x1, y1, npts, chain;
    PPO_HD void point(int x, int y) { if (npts == 0) { x0 = x1 = x; y0 = y1 = y; } ++npts; }
    PPO_HD void run(int s, int) { chain += (s + 9) / 10; }
    PPO_HD void visit(int x, int y) { x0 = ppo_min(x0, x); x1 = ppo_max(x1, x); y0 = ppo_min(y0, y); y1 = ppo_max(y1, y); }
};

// the count pass of cell i: counts[i][0..6] (include/deepliif_hip.h)
PPO_HD void ppo_count_lane(const uint8_t *mask, int H, int W, const int *cells, int i, int ox, int oy, int *counts) {
    const int *c = cells + (size_t)i * 8;
    PPOCountSink s{0, 0, 0, 0, 0, 0};
    const int st = ppo_trace(mask, H, W, c[0], c[1], c[2], s);
    int *o = counts + (size_t)i * 8;
    o[0] = st; o[7] = 0;
    if (st != DL_PP_OUTLINE_OK) { o[1] = o[2] = o[3] = o[4] = o[5] = o[6] = 0; return; }
    const PPOWidths w = ppo_widths(c, s.x0, s.y0, s.x1, s.y1, ox, oy);
    o[1] = s.x0; o[2] = s.y0; o[3] = s.x1; o[4] = s.y1; o[5] = s.npts;
    o[6] = 1 + w.size + w.cls + 2 * w.tl + 6 * w.off + s.chain;
}

struct PPOPointSink {
    int *out; long long cap; int ox, oy; long long n;                // out = this cell's first pair, cap = pairs it may store
    PPO_HD void point(int x, int y) { if (n < cap) { out[2 * n] = x + ox; out[2 * n + 1] = y + oy; } ++n; }
    PPO_HD void run(int, int) {}
    PPO_HD void visit(int, int) {}
};
struct PPOStringSink {
    char *out; long long cap, n;
    PPO_HD void put(int ch) { if (n < cap) out[n] = (char)ch; ++n; }
    PPO_HD void number(int v, int width) {                       // big-endian base 92, characters 35 .. 126, padded with the digit 0
        if (v < 0) v = 0;
        int div = 1;
        for (int j = 1; j < width; ++j) div *= 92;                   // width <= 5 for an int
        for (int j = 0; j < width; ++j) { put(35 + (v / div) % 92); div /= 92; }
    }
    PPO_HD void point(int, int) {}
    PPO_HD void run(int s, int k) {
        const int code = (3 - k) & 7;                                // ring direction -> Freeman code (1,0) = 0, counter-clockwise with y down
        while (s > 10) { put(35 + 80 + code); s -= 10; }
        put(35 + 8 * s + code);
    }
    PPO_HD void visit(int, int) {}
};

// the emit pass of cell i: stores inside [offsets[i], min(offsets[i + 1], out_items)) only; counts[i][7] = items produced
PPO_HD void ppo_emit_lane(const uint8_t *mask, int H, int W, const int *cells, int *counts, const long long *offsets, int i, int ox, int oy,
                          int mode, void *out, long long out_items) {
    const int *c = cells + (size_t)i * 8;
    int *o = counts + (size_t)i * 8;
    if (o[0] != DL_PP_OUTLINE_OK) { o[7] = 0; return; }
    const long long begin = offsets[i], end = offsets[i + 1] < out_items ? offsets[i + 1] : out_items;
    const long long cap = (begin >= 0 && end > begin) ? end - begin : 0;
    if (mode == DL_PP_OUTLINE_POINTS) {
        PPOPointSink s{(int *)out + 2 * (cap ? begin : 0), cap, ox, oy, 0};
        ppo_trace(mask, H, W, c[0], c[1], c[2], s);
        o[7] = (int)s.n;
        return;
    }
    const int x0 = o[1], y0 = o[2];
    const PPOWidths w = ppo_widths(c, x0, y0, o[3], o[4], ox, oy);
    PPOStringSink s{(char *)out + (cap ? begin : 0), cap, 0};
    s.put(35 + (w.size - 1) * 16 + (w.tl - 1) * 4 + (w.off - 1));
    s.number(c[2], w.size);
    s.number(c[4] * 2 + (c[3] != 0), w.cls);
    s.number(x0 + ox, w.tl); s.number(y0 + oy, w.tl);
    s.number(o[3] - x0, w.off); s.number(o[4] - y0, w.off);
    s.number(c[5] - x0, w.off); s.number(c[6] - y0, w.off);
    s.number(c[0] - x0, w.off); s.number(c[1] - y0, w.off);
    ppo_trace(mask, H, W, c[0], c[1], c[2], s);
    o[7] = (int)s.n;
}
