"""Hand-made masks for the cell-outline path, shared by tests/golden/make_golden_cells_wsi.py, test_outline_host.py and
test_gpu_outline.py.  Every mask holds ONE 8-connected cell (uint8, 100 = cell, 0 = background) and is the smallest picture of one
thing the trace, the simplification or the encoder can get wrong."""
import numpy as np

# region offsets (start_x, start_y): none; 91 / 92 = the last one-digit and the first two-digit base-92 number; 8463 / 8464 the same
# for two and three digits; a slide-sized one
OFFSETS = [(0, 0), (91, 0), (92, 5), (8463, 8464), (20000, 40000)]


def _blank(h, w):
    return np.zeros((h, w), dtype=np.uint8)


def _spiral():
    """a 1-pixel-wide rectangular spiral of three turns: on the way out every pixel of the way in is visited again"""
    m = _blank(15, 15)
    x, y, dx, dy, leg = 7, 7, 1, 0, 2
    m[y, x] = 100
    for i in range(12):                                   # 4 legs per turn
        for _ in range(leg):
            x, y = x + dx, y + dy
            m[y, x] = 100
        dx, dy = -dy, dx
        if i % 2 == 1:
            leg += 2
    return m


def hand_masks():
    """name -> mask"""
    out = {}
    m = _blank(5, 6); m[2, 3] = 100
    out['single_pixel'] = m
    m = _blank(5, 12); m[2, 1:10] = 100
    out['line_horizontal'] = m
    m = _blank(12, 5); m[2:11, 3] = 100
    out['line_vertical'] = m
    m = _blank(9, 9)
    for i in range(1, 8):
        m[i, i] = 100
    out['line_diagonal'] = m
    m = _blank(9, 9)
    for i in range(1, 8):
        m[i, 8 - i] = 100
    out['line_antidiagonal'] = m
    m = _blank(8, 8); m[1:4, 1:4] = 100; m[4:7, 4:7] = 100
    out['blobs_joined_diagonally'] = m
    m = _blank(11, 11); m[1:10, 1:10] = 100; m[4:7, 4:7] = 0
    out['ring'] = m
    m = _blank(9, 9); m[1:8, 1] = 100; m[1:8, 7] = 100; m[7, 1:8] = 100
    out['u_shape'] = m
    out['spiral'] = _spiral()
    m = _blank(7, 9); m[3, :] = 100; m[:, 4] = 100
    out['touches_four_borders'] = m
    out['fills_the_image'] = np.full((4, 6), 100, dtype=np.uint8)
    m = _blank(1, 37); m[0, 5:30] = 100
    out['image_1x37'] = m
    out['image_1x37_full'] = np.full((1, 37), 100, dtype=np.uint8)
    m = _blank(61, 1); m[7:50, 0] = 100
    out['image_61x1'] = m
    for w in (11, 21, 25, 45):                            # top edge = one run of 10, 20, 24, 44 steps
        m = _blank(5, w + 2); m[1:4, 1:w + 1] = 100
        out[f'bar_{w}x3'] = m
    m = _blank(27, 5); m[1:26, 1:4] = 100
    out['bar_3x25'] = m
    m = _blank(102, 103); m[1:101, 2:102] = 100           # size 10 000: three digits; offsets 99: two
    out['square_100'] = m
    m = _blank(12, 200); m[2:9, 95:110] = 100; m[9, 100] = 100
    out['starts_at_x_95'] = m
    return out


def single_cell(mask, positive=True, value=77):
    """the row get_cells_info would list for the one cell of `mask`: (size, positive, value, first x, first y, centre x, centre y)"""
    ys, xs = np.nonzero(mask)                              # raster order
    n = len(xs)
    return (n, positive, value, int(xs[0]), int(ys[0]), int(np.rint(xs.sum() / n)), int(np.rint(ys.sum() / n)))


def seg_from_mask(mask):
    """a segmentation image whose cell mapping gives `mask` back when the mask has no enclosed hole: cells positive, the rest unknown"""
    seg = np.zeros(mask.shape + (3,), dtype=np.uint8)
    seg[mask != 0] = (230, 10, 20)
    return seg
