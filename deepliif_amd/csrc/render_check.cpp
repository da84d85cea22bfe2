// render_check.cpp -- host run of render.h (test infrastructure; built and run by tests/test_cells_render_host.py, never linked into the library).
// Input file: int32 {H, W, n, ox, oy, mode, v6, 0} | dl_pp_render_thresh | int64 data_items | int64 offsets[n + 1] | data (data_items bytes for
// mode 1, data_items int32 pairs for mode 0) | int32 table[n][4] (mode 0 only).  Runs the count lane, then the paint lane, cell by cell; every
// cell sees its own range as a separate allocation of exactly that size (an address sanitizer then reports any read beyond it) through a
// two-entry offset table.  A range that is not inside the data is handed over as an empty one.  Writes: int32 rows[n][8] | int32 owner[H * W].
#include "render.h"
#include <stdlib.h>
#include <vector>

void dl_set_error(const char *, ...) {}

struct HostSink {
    int *owner; int H, W, i;
    void pixel(int x, int y) {
        if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H && owner[(size_t)y * W + x] < i) owner[(size_t)y * W + x] = i;
    }
};

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[8];
    dl_pp_render_thresh t;
    long long data_items;
    if (fread(hdr, sizeof(int), 8, f) != 8 || fread(&t, sizeof(t), 1, f) != 1 || fread(&data_items, sizeof(data_items), 1, f) != 1) return 2;
    const int H = hdr[0], W = hdr[1], n = hdr[2], ox = hdr[3], oy = hdr[4], mode = hdr[5], v6 = hdr[6];
    if (H <= 0 || W <= 0 || n < 0 || data_items < 0 || (mode != DL_PP_OUTLINE_POINTS && mode != DL_PP_OUTLINE_STRINGS)) return 2;
    const size_t item = mode == DL_PP_OUTLINE_STRINGS ? 1 : 8;
    std::vector<long long> offsets((size_t)n + 1);
    std::vector<uint8_t> data((size_t)data_items * item);
    std::vector<int> table((size_t)n * 4), rows((size_t)n * 8), owner((size_t)H * W, -1);
    if (fread(offsets.data(), sizeof(long long), offsets.size(), f) != offsets.size()) return 2;
    if (!data.empty() && fread(data.data(), 1, data.size(), f) != data.size()) return 2;
    if (mode == DL_PP_OUTLINE_POINTS && n && fread(table.data(), sizeof(int), table.size(), f) != table.size()) return 2;
    fclose(f);
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < n; ++i) {
            long long b = offsets[i], e = offsets[i + 1];
            if (b < 0 || e < b || e > data_items) b = e = 0;
            const long long two[2] = {0, e - b};
            void *own = e > b ? malloc((size_t)(e - b) * item) : nullptr;
            if (e > b) memcpy(own, data.data() + (size_t)b * item, (size_t)(e - b) * item);
            if (pass == 0) ppr_count_lane(mode, v6, own, e - b, two, table.data() + (size_t)i * 4, 0, t, ox, oy, H, W, rows.data() + (size_t)i * 8);
            else {
                HostSink s{owner.data(), H, W, i};
                ppr_paint_lane(mode, own, e - b, two, rows.data() + (size_t)i * 8, 0, ox, oy, H, W, s);
            }
            free(own);
        }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(rows.data(), sizeof(int), rows.size(), f);
    fwrite(owner.data(), sizeof(int), owner.size(), f);
    fclose(f);
    return 0;
}
