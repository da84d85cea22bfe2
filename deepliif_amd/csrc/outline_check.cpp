// outline_check.cpp -- host run of outline.h (test infrastructure; built and run by tests/test_outline_host.py, never linked into the library).
// Input file: int32 {H, W, n, ox, oy, mode, slack} | uint8 mask[H * W] | int32 cells[n][8].  Runs the count pass cell by cell, scans the counts the way
// the caller of the library does, runs the emit pass into a buffer with `slack` guard items on either side of every cell's range (the emit pass must
// leave them alone), and writes: int32 counts[n][8] | int64 total | the items (int32 pairs for mode 0, bytes for mode 1).  Exit code 3 = a guard item
// was overwritten.
#include "outline.h"
#include <vector>

void dl_set_error(const char *, ...) {}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[7];
    if (fread(hdr, sizeof(int), 7, f) != 7) return 2;
    const int H = hdr[0], W = hdr[1], n = hdr[2], ox = hdr[3], oy = hdr[4], mode = hdr[5], slack = hdr[6];
    if (H <= 0 || W <= 0 || n < 0 || slack < 0) return 2;
    std::vector<uint8_t> mask((size_t)H * W);
    std::vector<int> cells((size_t)n * 8 + 1), counts((size_t)n * 8 + 1);
    if (fread(mask.data(), 1, mask.size(), f) != mask.size()) return 2;
    if (n && fread(cells.data(), sizeof(int), (size_t)n * 8, f) != (size_t)n * 8) return 2;
    fclose(f);
    for (int i = 0; i < n; ++i) ppo_count_lane(mask.data(), H, W, cells.data(), i, ox, oy, counts.data());
    // every cell's range is preceded and followed by `slack` guard items
    std::vector<long long> offsets(n + 1), padded(n + 1);
    long long total = 0, ptotal = slack;
    for (int i = 0; i < n; ++i) {
        const int items = counts[(size_t)i * 8 + (mode == DL_PP_OUTLINE_STRINGS ? 6 : 5)];
        offsets[i] = total; padded[i] = ptotal;
        total += items; ptotal += items + slack;
    }
    offsets[n] = total; padded[n] = ptotal;
    const size_t item = mode == DL_PP_OUTLINE_STRINGS ? 1 : 8;
    std::vector<uint8_t> buf((size_t)ptotal * item + 8, 0xA5), out((size_t)total * item + 8);
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        // the lane sees [padded[i], padded[i] + items) through a two-entry offset table of its own
        const long long items = offsets[i + 1] - offsets[i];
        const long long two[2] = {padded[i], padded[i] + items};
        ppo_emit_lane(mask.data(), H, W, cells.data() + (size_t)i * 8, counts.data() + (size_t)i * 8, two, 0, ox, oy, mode, buf.data(), ptotal);
        memcpy(out.data() + (size_t)offsets[i] * item, buf.data() + (size_t)padded[i] * item, (size_t)items * item);
        memset(buf.data() + (size_t)padded[i] * item, 0xA5, (size_t)items * item);
    }
    for (size_t j = 0; j < buf.size(); ++j) bad += buf[j] != 0xA5;
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(counts.data(), sizeof(int), (size_t)n * 8, f);
    fwrite(&total, sizeof(total), 1, f);
    fwrite(out.data(), item, (size_t)total, f);
    fclose(f);
    return bad ? 3 : 0;
}
