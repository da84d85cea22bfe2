// render.h -- decoding, classifying and painting a STORED cell list, shared by postproc.hip (one lane per cell: pp_render_count_kernel,
// pp_render_paint_kernel) and the host check render_check.cpp (tests/test_cells_render_host.py runs the same lane functions cell by cell
// on the CPU against the host route of postprocessing.cells_to_final_results).
//
// cells_to_final_results (:1307-1412) of deepliif/postprocessing.py: decode_cell_data_v4 (:851-920), the classification of :1371-1380,
// make_full_contour (:637-682).  A cell is a list of vertices; consecutive vertices (and the last and the first) are joined by straight
// runs in one of the eight pixel directions.  A version-4 / -6 string spells them as a first point plus one chain character per run of
// <= 11 steps (35 + 8 * steps + Freeman code); a character that repeats the direction of the one before it extends the run, which
// changes neither the pixels nor the extent of the vertices, so every character is simply one more vertex here.
// The strings come from files: every byte is checked (35 .. 126), nothing outside the cell's own range [offsets[i], offsets[i + 1]) is
// read, coordinates are 64-bit while they are decoded (a base-92 number of six digits does not fit 32 bits, and a long chain can walk
// anywhere), and the paint pass walks only cells whose every vertex the count pass found inside the image.
#pragma once
#include "common.h"

#define PPR_HD __host__ __device__ __forceinline__
typedef long long ppr_i64;

PPR_HD ppr_i64 ppr_abs(ppr_i64 v) { return v < 0 ? -v : v; }
PPR_HD ppr_i64 ppr_max(ppr_i64 a, ppr_i64 b) { return a > b ? a : b; }
PPR_HD int ppr_sat(ppr_i64 v) { return v > 2147483647ll ? 2147483647 : (v < -2147483647ll - 1 ? -2147483647 - 1 : (int)v); }
PPR_HD int ppr_sgn(ppr_i64 v) { return (v > 0) - (v < 0); }

// create-or-not and the class of one cell (:1371-1380, in that order): 0 = not counted, 1 = positive, 2 = negative
PPR_HD int ppr_class(ppr_i64 size, int positive, ppr_i64 value, const dl_pp_render_thresh &t, int v6) {
    if (!(size > t.size_lower && (!t.has_size_upper || size < t.size_upper))) return 0;
    bool pos = positive != 0;
    if (!v6 && t.has_marker && value > t.marker) pos = true;
    if (v6) {
        if (t.has_od_lower && value < t.od_lower) pos = false;
        else if (t.has_od_upper && value > t.od_upper) pos = false;
    }
    return pos ? 1 : 2;
}

// the numbers in front of the chain of one version-4 / -6 string s[b .. e): lengths byte, size, class (2 digits), top-left x y, six offsets
struct PPRHead { bool ok; ppr_i64 size, cls, fx, fy, chain; };              // chain = index of the first chain character
PPR_HD bool ppr_number(const uint8_t *s, ppr_i64 &pos, int width, ppr_i64 &out) {
    ppr_i64 v = 0;
    for (int j = 0; j < width; ++j) {
        const int c = s[pos + j];
        if (c < 35 || c > 126) return false;
        v = v * 92 + (c - 35);
    }
    pos += width;
    out = v;
    return true;
}
PPR_HD PPRHead ppr_head(const uint8_t *s, ppr_i64 b, ppr_i64 e) {
    PPRHead h{false, 0, 0, 0, 0, 0};
    if (e <= b) return h;
    const int c0 = s[b];
    if (c0 < 35 || c0 > 126) return h;
    const int n = c0 - 35, w_size = n / 16 + 1, w_tl = (n / 4) % 4 + 1, w_off = n % 4 + 1;       // <= 6, 4, 4 digits
    if (e - b < 1 + w_size + 2 + 2 * w_tl + 6 * w_off) return h;
    ppr_i64 pos = b + 1, ax, ay, off[6];
    if (!ppr_number(s, pos, w_size, h.size) || !ppr_number(s, pos, 2, h.cls) || !ppr_number(s, pos, w_tl, ax) || !ppr_number(s, pos, w_tl, ay)) return h;
    for (int j = 0; j < 6; ++j)
        if (!ppr_number(s, pos, w_off, off[j])) return h;
    h.fx = ax + off[4]; h.fy = ay + off[5]; h.chain = pos; h.ok = true;
    return h;
}

// Freeman code -> step: (1,0) (1,-1) (0,-1) (-1,-1) (-1,0) (-1,1) (0,1) (1,1)
#define PPR_FDX(c) ((int)((0x901Au >> (2 * (c))) & 3u) - 1)
#define PPR_FDY(c) ((int)((0xA901u >> (2 * (c))) & 3u) - 1)

// every vertex of cell i, in order, moved by (-ox, -oy), to v.vertex(x, y) (which returns false to stop).  -> false: malformed
template <class V>
__host__ __device__ bool ppr_vertices(int mode, const void *data, ppr_i64 data_items, const ppr_i64 *offsets, int i, int ox, int oy, V &v) {
    const ppr_i64 b = offsets[i], e = offsets[i + 1];
    if (b < 0 || e <= b || e > data_items) return false;
    if (mode == DL_PP_OUTLINE_POINTS) {
        const int *p = (const int *)data;
        for (ppr_i64 j = b; j < e; ++j)
            if (!v.vertex((ppr_i64)p[2 * j] - ox, (ppr_i64)p[2 * j + 1] - oy)) return true;
        return true;
    }
    const uint8_t *s = (const uint8_t *)data;
    const PPRHead h = ppr_head(s, b, e);
    if (!h.ok) return false;
    ppr_i64 x = h.fx - ox, y = h.fy - oy;
    if (!v.vertex(x, y)) return true;
    for (ppr_i64 j = h.chain; j < e; ++j) {
        const int c = s[j];
        if (c < 35 || c > 126) return false;
        const int steps = (c - 35) >> 3, code = (c - 35) & 7;
        x += PPR_FDX(code) * steps; y += PPR_FDY(code) * steps;
        if (!v.vertex(x, y)) return true;
    }
    return true;
}

struct PPRCountV {
    ppr_i64 fx, fy, px, py, x0, y0, x1, y1, pixels;
    int n;
    bool bad;
    PPR_HD void segment(ppr_i64 dx, ppr_i64 dy, int closing) {
        const ppr_i64 ax = ppr_abs(dx), ay = ppr_abs(dy), s = ppr_max(ax, ay);
        if (ax != 0 && ay != 0 && ax != ay) bad = true;
        pixels += closing ? ppr_max(s - 1, 0) : s;              // the closing run stops in front of the first point
    }
    PPR_HD bool vertex(ppr_i64 x, ppr_i64 y) {
        if (n == 0) { fx = x0 = x1 = x; fy = y0 = y1 = y; pixels = 1; }
        else {
            segment(x - px, y - py, 0);
            x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
        }
        px = x; py = y; ++n;
        return true;
    }
};

// the count pass of cell i: rows[i][0..7] (include/deepliif_hip.h)
PPR_HD void ppr_count_lane(int mode, int v6, const void *data, ppr_i64 data_items, const ppr_i64 *offsets, const int *table, int i,
                           const dl_pp_render_thresh &t, int ox, int oy, int H, int W, int *rows) {
    int *o = rows + (size_t)i * 8;
    o[0] = DL_PP_RENDER_MALFORMED;
    o[1] = o[2] = o[3] = o[4] = o[5] = o[6] = o[7] = 0;
    const ppr_i64 b = offsets[i], e = offsets[i + 1];
    if (b < 0 || e <= b || e > data_items) return;
    if (mode == DL_PP_OUTLINE_POINTS) {
        const int *c = table + (size_t)i * 4;
        o[1] = ppr_class(c[0], c[1], c[2], t, v6);
    } else {
        const PPRHead h = ppr_head((const uint8_t *)data, b, e);
        if (!h.ok) return;
        o[1] = ppr_class(h.size, (int)(h.cls & 1), h.cls >> 1, t, v6);
    }
    PPRCountV v{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, false};
    const bool ok = ppr_vertices(mode, data, data_items, offsets, i, ox, oy, v);
    if (!ok || v.n == 0) return;
    v.segment(v.fx - v.px, v.fy - v.py, 1);
    o[2] = ppr_sat(v.x0); o[3] = ppr_sat(v.y0); o[4] = ppr_sat(v.x1); o[5] = ppr_sat(v.y1); o[6] = ppr_sat(v.pixels);
    if (v.bad) o[0] = DL_PP_RENDER_BAD_SEGMENT;
    else if (v.x0 < 0 || v.y0 < 0 || v.x1 >= W || v.y1 >= H) o[0] = DL_PP_RENDER_OUTSIDE;
    else o[0] = DL_PP_RENDER_OK;
}

// Sink: pixel(x, y) = one pixel of the full outline (the sink checks it against the image and keeps the maximum cell index)
template <class Sink>
struct PPRPaintV {
    Sink &s;
    int H, W, fx, fy, px, py, n;
    PPR_HD void run(int dx, int dy, int steps) {
        const int sx = ppr_sgn(dx), sy = ppr_sgn(dy);
        for (int j = 0; j < steps; ++j) { px += sx; py += sy; s.pixel(px, py); }
    }
    PPR_HD bool vertex(ppr_i64 x, ppr_i64 y) {
        if (x < 0 || y < 0 || x >= W || y >= H) return false;          // (not reached for a cell the count pass found OK)
        if (n == 0) { fx = px = (int)x; fy = py = (int)y; s.pixel(px, py); }
        else {
            const int dx = (int)x - px, dy = (int)y - py;
            run(dx, dy, (int)ppr_max(ppr_abs(dx), ppr_abs(dy)));
            px = (int)x; py = (int)y;
        }
        ++n;
        return true;
    }
};

// the paint pass of cell i: make_full_contour's pixels, the closing run back to (excluding) the first point included
template <class Sink>
__host__ __device__ void ppr_paint_lane(int mode, const void *data, ppr_i64 data_items, const ppr_i64 *offsets, const int *rows, int i,
                                        int ox, int oy, int H, int W, Sink &s) {
    const int *o = rows + (size_t)i * 8;
    if (o[0] != DL_PP_RENDER_OK || o[1] == 0) return;
    PPRPaintV<Sink> v{s, H, W, 0, 0, 0, 0, 0};
    if (!ppr_vertices(mode, data, data_items, offsets, i, ox, oy, v) || v.n == 0) return;
    const int dx = v.fx - v.px, dy = v.fy - v.py;
    v.run(dx, dy, (int)ppr_max(ppr_abs(dx), ppr_abs(dy)) - 1);
}
