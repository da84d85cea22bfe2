"""Segmentation post-processing on the GPU -- the seam of deepliif/postprocessing.py.

`compute_final_results(orig, seg, marker, resolution, ...)` keeps the reference's signature and return value
(deepliif/postprocessing.py:1223-1304: overlay image, refined segmentation image, scoring dictionary) and its byte-exact results; the
per-pixel work, the two connected-component labellings and the per-cell reductions run in csrc/postproc.hip (dl_pp_cells,
dl_pp_finish).  What stays on the host is the arithmetic over the CELL LIST (hundreds to thousands of rows): noise thresholds, centroid
rounding, the default size threshold (a 500-bin KDE of sqrt(size), :365-447, repeated expression by expression so that its float64
comparisons agree) and the default marker threshold (:450-488, from a 256-bin histogram the GPU produces instead of np.percentile over
the image).  There is no CPU fallback: without the HIP library this module raises.

`compute_cell_results(seg, marker, resolution, version, ..., route=None, offset=(0, 0))` (:1136-1220) is the per-cell export: on top of the cell
mapping, every cell's bounding box and simplified outline, as dicts (data versions 3 / 5) or base-92 + Freeman-chain strings (4 / 6).  The outlines are
traced and encoded on the GPU (dl_pp_outline_count / dl_pp_outline_emit, one lane per cell; outline_cells below); the per-cell Python code the
reference's functions translate to is kept as route='host', the yardstick.  `offset` places the image inside a slide (wsi.infer_slide_cells).

`cells_to_final_results(data, orig, ...thresholds..., route='gpu', offset=(0, 0), outside='raise')` (:1307-1412) renders such a stored cell list
back into overlay, refined image and scoring under new thresholds (dl_pp_render_count / _paint / _finish); `pack_cells` uploads a list once for
repeated calls; route='host' is the numpy restatement the kernels are held to.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import ops

DEFAULT_SEG_THRESH = 120          # postprocessing.py:83
DEFAULT_NOISE_THRESH = 4          # postprocessing.py:84
_OD_LUT = [math.log10(255 / max(i, 1)) for i in range(256)]          # create_od_image's table (:123-130): entry 0 takes entry 1's value


def _to_u8_cuda(img, device) -> torch.Tensor:
    """PIL image / ndarray / tensor -> uint8 [H][W][3] CUDA tensor (to_array, :98-120: non-RGB PIL images are converted to RGB)"""
    if isinstance(img, torch.Tensor):
        t = img
    else:
        try:
            from PIL import Image
            if isinstance(img, Image.Image):
                img = np.asarray(img if img.mode == 'RGB' else img.convert('RGB'))
        except ImportError:
            pass
        t = torch.from_numpy(np.array(img, copy=True))            # (PIL-backed arrays are read-only)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f'expected a uint8 H x W x 3 image, got {tuple(t.shape)} {t.dtype}')
    t = t.to(device)
    return t if t.stride(2) == 1 and t.stride(1) == 3 else t.contiguous()


def calculate_large_noise_thresh(large_noise_thresh, resolution):
    """postprocessing.py:1125-1133"""
    if large_noise_thresh != 'default':
        return large_noise_thresh
    return {'10x': 1000, '20x': 4000}.get(resolution, 16000)


def calculate_default_size_threshold(cell_sizes, resolution='40x') -> int:
    """postprocessing.py:406-447 (+ create_kde :365-403): first local minimum of a Gaussian KDE (500 bins, bandwidth 1) of sqrt(size),
    clamped to the resolution's allowed range.  Same float64 expressions in the same order as the reference's loops."""
    sizes = np.asarray(cell_sizes, dtype=np.int64)
    if sizes.shape[0] <= 1:
        return 0
    values = np.ascontiguousarray(np.sqrt(sizes), dtype=np.float64)
    # the KDE loop itself (n x 500 exp calls in the reference's summation order) is host code inside the library: dl_pp_kde_first_minimum
    step = C.c_double(0.0)
    idx = int(L.load().dl_pp_kde_first_minimum(values.ctypes.data_as(C.c_void_p), int(values.shape[0]), 500, C.byref(step), None))
    if idx < 0:
        L.check(idx, 'dl_pp_kde_first_minimum')
    step = step.value
    t = (idx - 1) * step
    lo, dflt, hi = {'20x': (3, 4, 6), '10x': (2, 2, 3)}.get(resolution, (4, 7, 10))
    if t < lo:
        t = lo
    elif t > hi:
        t = dflt
    return round(t * t)


def percentile_from_histogram(hist, q: float) -> float:
    """np.percentile(values, q) (default 'linear' method) of the multiset {v repeated hist[v] times}, computed from the histogram the way
    numpy computes it from the sorted array (numpy/lib/_function_base_impl.py: _quantile, _get_indexes, _lerp): virtual index
    (n - 1) * (q / 100), neighbours at floor and floor + 1 (both the last element at or beyond the end), weight g = virtual - floor,
    a + (b - a) * g, taken from the far end (b - (b - a) * (1 - g)) when g >= 0.5."""
    hist = np.asarray(hist, dtype=np.int64)
    n = int(hist.sum())
    virtual = (n - 1) * np.true_divide(q, 100)
    prev = int(math.floor(virtual))
    nxt = prev + 1
    if virtual >= n - 1:
        prev = nxt = n - 1
    if virtual < 0:
        prev = nxt = 0
    gamma = virtual - (prev if virtual < n - 1 else -1)
    cum = np.cumsum(hist)
    a = float(np.searchsorted(cum, prev, side='right'))
    b = float(np.searchsorted(cum, nxt, side='right'))
    diff = b - a
    out = a + diff * gamma
    if gamma >= 0.5:
        out = b - diff * (1 - gamma)
    return float(out)


def calculate_default_marker_threshold(hist) -> int:
    """postprocessing.py:450-488 on the histogram of the gray marker image: 90 % of the 0.1 .. 99.9 percentile range of its non-zero pixels"""
    h = np.asarray(hist, dtype=np.int64).copy()
    h[0] = 0
    if int(h.sum()) == 0:
        lo = hi = 0
    else:
        lo, hi = round(percentile_from_histogram(h, 0.1)), round(percentile_from_histogram(h, 99.9))
    return round((hi - lo) * 0.9) + lo


class CellMap:
    """Device-side result of the cell mapping (get_cells_info, :311-362) plus the host-side cell list."""

    def __init__(self, mask, label, ws, rows, keep, cells, defaults, shape, table=None):
        self.mask, self.label, self.ws = mask, label, ws          # uint8 [H][W], int32 [H][W], workspace shared with dl_pp_finish
        self.rows, self.keep = rows, keep                         # every component's reductions (int64 [n][8]); which of them are cells
        self.cells, self.defaults, self.shape = cells, defaults, shape
        self.table = table                                        # `cells` as the int32 [n][8] rows of dl_pp_outline_* (outline_table)


def get_cells_info(seg, marker, resolution, noise_thresh, seg_thresh, large_noise_thresh, use_od=False, device=None) -> CellMap:
    """postprocessing.py:311-362.  `cells` = [(size, positive, marker value, first x, first y, centre x, centre y)] like the reference's."""
    be = ops.impl()
    lib = be.lib
    dev = torch.device(device) if device is not None else (seg.device if isinstance(seg, torch.Tensor) and seg.is_cuda else torch.device('cuda', torch.cuda.current_device()))
    seg_t = _to_u8_cuda(seg, dev)
    mk_t = _to_u8_cuda(marker, dev) if marker is not None else None
    H, W = int(seg_t.shape[0]), int(seg_t.shape[1])
    if mk_t is not None and tuple(mk_t.shape) != tuple(seg_t.shape):
        raise ValueError('seg and marker images differ in size')
    ops._need_cuda(seg_t, mk_t)
    nbytes = int(lib.dl_pp_ws_bytes(H, W))
    if nbytes == 0:
        raise RuntimeError('dl_pp_ws_bytes failed (empty or too large image)')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    label = torch.empty((H, W), dtype=torch.int32, device=dev)
    max_cells = min(H * W // 4 + 8, 1 << 22)                      # 8-connected components are at least two pixels apart
    rows_d = torch.empty((max_cells, 8), dtype=torch.int64, device=dev)
    n_d = torch.zeros(1, dtype=torch.int32, device=dev)
    hist_d = torch.zeros(256, dtype=torch.int64, device=dev) if (mk_t is not None and not use_od) else None
    lut_d = torch.tensor(_OD_LUT, dtype=torch.float64, device=dev) if (use_od and mk_t is not None) else None
    p = ops._ptr
    L.check(lib.dl_pp_cells(p(seg_t), seg_t.stride(0), p(mk_t), mk_t.stride(0) if mk_t is not None else 0, p(lut_d), H, W, int(seg_thresh),
                            p(mask), p(label), p(ws), p(rows_d), max_cells, p(n_d), p(hist_d), ops._stream()), 'dl_pp_cells')
    n = int(n_d.item())
    if n > max_cells:
        raise RuntimeError(f'{n} connected components exceed the cell table ({max_cells})')
    rows = rows_d[:n].cpu().numpy()
    count = rows[:, 0]
    keep = count > noise_thresh
    if large_noise_thresh is not None:
        keep &= count < large_noise_thresh
    k = rows[keep]
    kc = k[:, 0]
    # int(round(sum / count)): Python's round of the float64 quotient, i.e. round-half-even = np.rint of the same quotient
    cx, cy = np.rint(k[:, 6] / kc).astype(np.int64), np.rint(k[:, 7] / kc).astype(np.int64)
    if mk_t is None:
        mval = np.zeros(len(k), dtype=np.int64)
    elif use_od:
        mval = np.rint(k[:, 3] / kc).astype(np.int64)
    else:
        mval = k[:, 3]
    pos = k[:, 1] >= k[:, 2]
    cells = [(int(a), bool(b), int(c), int(d), int(e), int(f), int(g)) for a, b, c, d, e, f, g in zip(kc, pos, mval, k[:, 4], k[:, 5], cx, cy)]
    defaults = {'size_thresh': calculate_default_size_threshold([c[0] for c in cells], resolution)}
    if hist_d is not None:
        defaults['marker_thresh'] = calculate_default_marker_threshold(hist_d.cpu().numpy())
    table = np.zeros((len(k), 8), dtype=np.int32)
    for j, col in enumerate((k[:, 4], k[:, 5], kc, pos, mval, cx, cy)):
        table[:, j] = col
    return CellMap(mask, label, ws, rows, keep, cells, defaults, (H, W), table)


def create_cell_classification(cm: CellMap, size_thresh=0, marker_thresh=None, size_thresh_upper=None, od_thresh_lower=None, od_thresh_upper=None):
    """The per-cell decisions of postprocessing.py:923-1000 -> (code per component for dl_pp_finish, counts)"""
    code = np.zeros(len(cm.keep), dtype=np.uint8)
    num_pos = num_neg = 0
    it = iter(cm.cells)
    for i, kept in enumerate(cm.keep):
        if not kept:
            continue
        cell = next(it)
        if not (cell[0] > size_thresh and (size_thresh_upper is None or cell[0] < size_thresh_upper)):
            continue
        pos = cell[1]
        if marker_thresh is not None and cell[2] > marker_thresh:
            pos = True
        if od_thresh_lower is not None and cell[2] < od_thresh_lower:
            pos = False
        elif od_thresh_upper is not None and cell[2] > od_thresh_upper:
            pos = False
        code[i] = 1 if pos else 2
        num_pos, num_neg = num_pos + (1 if pos else 0), num_neg + (0 if pos else 1)
    return code, {'num_total': num_pos + num_neg, 'num_pos': num_pos, 'num_neg': num_neg}


def compute_final_results(orig, seg, marker, resolution, size_thresh='default', marker_thresh=None, size_thresh_upper=None,
                          seg_thresh=DEFAULT_SEG_THRESH, noise_thresh=DEFAULT_NOISE_THRESH, large_noise_thresh=None,
                          od_thresh_lower=None, od_thresh_upper=None, return_tensors: bool = False, device=None):
    """deepliif/postprocessing.py:1223-1304 -> (overlay, refined, scoring).  Images may be PIL images, uint8 ndarrays or uint8 CUDA
    tensors (H x W x 3); the results are ndarrays like the reference's unless return_tensors (then CUDA tensors, no device->host copy)."""
    large = calculate_large_noise_thresh(large_noise_thresh, resolution)
    use_od = od_thresh_lower is not None or od_thresh_upper is not None
    cm = get_cells_info(seg, orig if use_od else marker, resolution, noise_thresh, seg_thresh, large, use_od=use_od, device=device)
    if size_thresh is None:
        size_thresh = 0
    elif size_thresh == 'default':
        size_thresh = cm.defaults['size_thresh']
    if marker_thresh == 'default':
        marker_thresh = cm.defaults['marker_thresh']
    code, counts = create_cell_classification(cm, size_thresh, marker_thresh, size_thresh_upper, od_thresh_lower, od_thresh_upper)
    dev = cm.mask.device
    H, W = cm.shape
    orig_t = _to_u8_cuda(orig, dev)
    if tuple(orig_t.shape[:2]) != (H, W):
        raise ValueError('orig and seg images differ in size')
    overlay = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    refined = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    code_d = torch.from_numpy(code).to(dev) if len(code) else None
    p = ops._ptr
    L.check(ops.impl().lib.dl_pp_finish(p(orig_t), orig_t.stride(0), p(cm.mask), p(cm.label), p(cm.ws), p(code_d), len(code), H, W,
                                        p(overlay), overlay.stride(0), p(refined), refined.stride(0), ops._stream()), 'dl_pp_finish')
    scoring = {
        'num_total': counts['num_total'], 'num_pos': counts['num_pos'], 'num_neg': counts['num_neg'],
        'percent_pos': round(counts['num_pos'] / counts['num_total'] * 100, 1) if counts['num_pos'] > 0 else 0,
        'seg_thresh': seg_thresh, 'size_thresh': size_thresh, 'size_thresh_upper': size_thresh_upper,
        'marker_thresh': marker_thresh if marker is not None else None,
    }
    if return_tensors:
        return overlay, refined, scoring
    return overlay.cpu().numpy(), refined.cpu().numpy(), scoring


# ---------------------------------------------------------------------------------------------------------------
# Per-cell export (compute_cell_results, postprocessing.py:1136-1220).  The "v4" strings are DeepLIIF's wire format for cell lists
# (base-92 numbers + Freeman chain code), so their layout below is a contract, not a choice.  The functions from here to
# cell_results_from_mapping are the HOST route: pure Python over a host copy of the label mask, a few hundred microseconds per cell --
# the yardstick the outline kernels (dl_pp_outline_count / dl_pp_outline_emit, route 'gpu' of compute_cell_results) are held to, byte
# for byte, and not what a slide runs through.
# ---------------------------------------------------------------------------------------------------------------
_RING = ((-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0))        # (dx, dy), clockwise from the upper-left neighbour
_RING_INDEX = {d: i for i, d in enumerate(_RING)}


def get_cell_boundary(mask, x, y):
    """postprocessing.py:491-581: Moore-neighbour trace of the cell whose first pixel (raster order) is (x, y), clockwise, ending when the
    start pixel is re-entered from the pixel that precedes it on the outline.  mask: 2-D array, 0 = background.
    -> ([(min x, min y), (max x, max y)], [(x, y), ...])"""
    h, w = mask.shape
    if not (0 <= y < h and 0 <= x < w) or mask[y, x] == 0:
        return None, None

    def cell(px, py):
        return 0 <= px < w and 0 <= py < h and mask[py, px] != 0

    # the pixel that precedes the start on a clockwise outline: first cell neighbour met going COUNTER-clockwise from the lower-left one
    k = 6
    while k >= 0 and not cell(x + _RING[k][0], y + _RING[k][1]):
        k -= 1
    if k < 0:
        return [(x, y), (x, y)], [(x, y)]
    first_prev = (x + _RING[k][0], y + _RING[k][1])
    start = (x, y)
    prev, cur = first_prev, start
    outline = [start]
    x0 = x1 = x
    y0 = y1 = y
    while True:
        k = (_RING_INDEX[(prev[0] - cur[0], prev[1] - cur[1])] + 1) % 8          # continue clockwise just past where we came from
        while not cell(cur[0] + _RING[k][0], cur[1] + _RING[k][1]):
            k = (k + 1) % 8
        prev, cur = cur, (cur[0] + _RING[k][0], cur[1] + _RING[k][1])
        if prev == first_prev and cur == start:          # closed: the reference's list ends here too (it drops this closing pair)
            break
        outline.append(cur)
        x0, x1 = min(x0, cur[0]), max(x1, cur[0])
        y0, y1 = min(y0, cur[1]), max(y1, cur[1])
    return [(x0, y0), (x1, y1)], outline


def make_simple_contour(points):
    """postprocessing.py:584-634: drop the interior points of straight runs (the direction signs before and after a point agree); the last
    point is compared against the wrap-around to the first"""
    pts = [(int(p[0]), int(p[1])) for p in points]
    if len(pts) == 1:
        return pts[:]
    sgn = lambda v: (v > 0) - (v < 0)
    keep = [pts[0]]
    n = len(pts)
    for i in range(1, n):
        a, b, c = pts[i - 1], pts[i], pts[(i + 1) % n]
        if (sgn(b[0] - a[0]), sgn(b[1] - a[1])) != (sgn(c[0] - b[0]), sgn(c[1] - b[1])):
            keep.append(b)
    return keep


def to_base92(values, min_len=1):
    """postprocessing.py:685-727: big-endian base-92 digits as characters 35..126; several values share one width (>= min_len, padded with
    chr(35) = the digit 0)"""
    single = not isinstance(values, (list, tuple))
    vals = [values] if single else list(values)
    digits = []
    for v in vals:
        v = int(v)
        d = ''
        while v > 0:
            d = chr(v % 92 + 35) + d
            v //= 92
        digits.append(d)
    width = max(max(len(d) for d in digits), min_len)
    out = [d.rjust(width, chr(35)) for d in digits]
    return out[0] if single else out


def from_base92(val):
    """postprocessing.py:730-749"""
    res = 0
    for ch in val:
        res = res * 92 + (ord(ch) - 35)
    return res


_FREEMAN = {(1, 0): 0, (1, -1): 1, (0, -1): 2, (-1, -1): 3, (-1, 0): 4, (-1, 1): 5, (0, 1): 6, (1, 1): 7}      # (sign dx, sign dy) -> code


def encode_cell_data_v4(data, v6=False):
    """postprocessing.py:752-848.  Layout: [lengths byte] size | classification (2 digits: marker * 2 + positive) | bbox top-left x, y |
    offsets from it of: bbox bottom-right, centroid, first boundary point (6 numbers, one width) | Freeman chain of the remaining boundary
    points, one character per run of <= 10 steps: chr(35 + 8 * steps + direction).  lengths byte = chr(35 + 16 (|size| - 1) + 4 (|top-left| - 1)
    + (|offsets| - 1))."""
    size = to_base92(data['size'])
    marker = data['od'] if v6 else data['marker']
    body = size + to_base92(int(marker) * 2 + int(data['positive']), 2)
    (ax, ay), (bx, by) = data['bbox']
    topleft = to_base92([ax, ay])
    body += topleft[0] + topleft[1]
    cx, cy = data['centroid']
    fx, fy = data['boundary'][0]
    offs = to_base92([bx - ax, by - ay, cx - ax, cy - ay, fx - ax, fy - ay])
    body += ''.join(offs)
    head = chr(35 + (len(size) - 1) * 16 + (len(topleft[0]) - 1) * 4 + (len(offs[0]) - 1))
    chain = []
    pts = data['boundary']
    for j in range(1, len(pts)):
        dx, dy = pts[j][0] - pts[j - 1][0], pts[j][1] - pts[j - 1][1]
        steps = max(abs(dx), abs(dy))
        if steps == 0:
            continue
        code = _FREEMAN[((dx > 0) - (dx < 0), (dy > 0) - (dy < 0))]
        while steps > 10:
            chain.append(chr(35 + 80 + code))
            steps -= 10
        chain.append(chr(35 + steps * 8 + code))
    return head + body + ''.join(chain)


_FREEMAN_STEP = {code: step for step, code in _FREEMAN.items()}


def decode_cell_data_v4(cell, v6=False):
    """postprocessing.py:851-920, the inverse of encode_cell_data_v4: the lengths byte gives the three widths, the numbers follow in the
    order of the layout above, then every chain character moves `steps` pixels in its direction from the last point.  A character that
    repeats the direction of the one before it (a run longer than 10 steps) extends that point instead of adding one."""
    n = ord(cell[0]) - 35
    w_size, w_tl, w_off = n // 16 + 1, (n // 4) % 4 + 1, n % 4 + 1
    pos = 1

    def take(width):
        nonlocal pos
        pos += width
        return from_base92(cell[pos - width:pos])

    size = take(w_size)
    cls = take(2)
    ax, ay = take(w_tl), take(w_tl)
    offs = [take(w_off) for _ in range(6)]
    pts = [(ax + offs[4], ay + offs[5])]
    last = None
    for ch in cell[pos:]:
        steps, code = divmod(ord(ch) - 35, 8)
        dx, dy = _FREEMAN_STEP[code]
        nxt = (pts[-1][0] + dx * steps, pts[-1][1] + dy * steps)
        if code == last:
            pts[-1] = nxt
        else:
            pts.append(nxt)
        last = code
    return {'size': size, 'positive': bool(cls % 2), ('od' if v6 else 'marker'): cls // 2, 'bbox': [(ax, ay), (ax + offs[0], ay + offs[1])],
            'centroid': (ax + offs[2], ay + offs[3]), 'boundary': pts}


def shift_cell(data, offset):
    """models/__init__.py:892-896: a decoded cell moved by the offset of its region inside the slide"""
    ox, oy = offset
    out = dict(data)
    out['bbox'] = [(x + ox, y + oy) for x, y in data['bbox']]
    out['centroid'] = (data['centroid'][0] + ox, data['centroid'][1] + oy)
    out['boundary'] = [(x + ox, y + oy) for x, y in data['boundary']]
    return out


def _cell_settings(defaults, version, seg_thresh, noise_thresh, large_noise_thresh):
    settings = {'default_size_thresh': defaults['size_thresh'], 'noise_thresh': noise_thresh, 'large_noise_thresh': large_noise_thresh,
                'seg_thresh': seg_thresh}
    if version not in (5, 6):
        settings['default_marker_thresh'] = defaults['marker_thresh'] if 'marker_thresh' in defaults else None
    return settings


def cell_results_from_mapping(mask, cells, defaults, version, seg_thresh, noise_thresh, large_noise_thresh, offset=(0, 0)):
    """The host half of compute_cell_results (:1170-1220): per-cell boundary, bbox and (for versions 4 / 6) the encoded string.
    mask: 2-D uint8 ndarray after the cell mapping (0 = background), cells / defaults as get_cells_info returns them.  With an offset
    every cell is moved before it is encoded (what models/__init__.py:883-903 reaches by decode -> shift -> encode)."""
    od = version in (5, 6)
    out = []
    for c in cells:
        bbox, boundary = get_cell_boundary(mask, c[3], c[4])
        data = {'size': c[0], 'positive': c[1], ('od' if od else 'marker'): c[2], 'bbox': bbox, 'centroid': (c[5], c[6]),
                'boundary': make_simple_contour(boundary)}
        if tuple(offset) != (0, 0):
            data = shift_cell(data, offset)
        out.append(encode_cell_data_v4(data, v6=(version == 6)) if version in (4, 6) else data)
    return {'cells': out, 'settings': _cell_settings(defaults, version, seg_thresh, noise_thresh, large_noise_thresh), 'dataVersion': version}


OUTLINE_STATUS = {1: 'its first pixel lies outside the image', 2: 'its first pixel is background',
                  3: 'the outline did not close within 8 * size + 8 moves (the size is not that of the cell at the first pixel)'}


def outline_table(cells) -> np.ndarray:
    """get_cells_info's cell list [(size, positive, value, first x, first y, centre x, centre y)] -> the int32 [n][8] rows of
    dl_pp_outline_*: {first x, first y, size, positive, value, centre x, centre y, 0}"""
    t = np.zeros((len(cells), 8), dtype=np.int32)
    if len(cells):
        a = np.asarray(cells, dtype=np.int64).reshape(len(cells), 7)
        t[:, :7] = a[:, [3, 4, 0, 1, 2, 5, 6]]
    return t


def outline_cells(mask, cells, version, offset=(0, 0), timings=None, lib=None):
    """The cells of compute_cell_results (:1170-1220) from the DEVICE mask: dl_pp_outline_count (bbox, kept points, string length per
    cell), an exclusive scan of those on the host (numpy), dl_pp_outline_emit (the kept points, or the complete strings in one byte
    buffer).  mask: uint8 [H][W] CUDA tensor, 0 = background; cells: get_cells_info's list or an outline_table().  -> list of dicts
    (versions 3 / 5) or strings (4 / 6), moved by `offset`.  A cell the kernel refuses (OUTLINE_STATUS) raises.
    timings (dict, optional): seconds spent after the last device->host copy, i.e. building the Python objects ('python');
    lib: the library to call (default: the one of the current 16-bit format; the kernels are the same in both builds)."""
    import time
    lib = lib if lib is not None else ops.impl().lib
    if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.uint8 and mask.dim() == 2 and mask.is_contiguous()):
        raise ValueError('outline_cells: the mask must be a contiguous uint8 [H][W] CUDA tensor')
    table = cells if isinstance(cells, np.ndarray) else outline_table(cells)
    if table.dtype != np.int32 or table.ndim != 2 or table.shape[1] != 8:
        raise ValueError('outline_cells: the cell table must be int32 [n][8]')
    n = int(table.shape[0])
    if n == 0:
        return []
    H, W = int(mask.shape[0]), int(mask.shape[1])
    ox, oy = int(offset[0]), int(offset[1])
    strings = version in (4, 6)
    dev = mask.device
    p, stream = ops._ptr, ops._stream(mask)
    table_d = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    counts_d = torch.empty((n, 8), dtype=torch.int32, device=dev)
    L.check(lib.dl_pp_outline_count(p(mask), H, W, p(table_d), n, ox, oy, p(counts_d), stream), 'dl_pp_outline_count', lib)
    counts = counts_d.cpu().numpy()
    bad = np.flatnonzero(counts[:, 0])
    if len(bad):
        i = int(bad[0])
        raise RuntimeError(f'dl_pp_outline_count: status {int(counts[i, 0])} for cell {i} (first pixel ({int(table[i, 0])}, {int(table[i, 1])}), size '
                           f'{int(table[i, 2])}) of {n}: {OUTLINE_STATUS.get(int(counts[i, 0]), "unknown status")}; {len(bad)} cells refused')
    items = counts[:, 6 if strings else 5].astype(np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(items, out=offsets[1:])
    total = int(offsets[-1])
    out_d = torch.empty(total, dtype=torch.uint8, device=dev) if strings else torch.empty((total, 2), dtype=torch.int32, device=dev)
    offsets_d = torch.from_numpy(offsets).to(dev)
    L.check(lib.dl_pp_outline_emit(p(mask), H, W, p(table_d), p(counts_d), p(offsets_d), n, ox, oy, 1 if strings else 0, p(out_d), total, stream),
            'dl_pp_outline_emit', lib)
    stored = counts_d[:, 7].cpu().numpy()
    if not np.array_equal(stored, items):
        i = int(np.flatnonzero(stored != items)[0])
        raise RuntimeError(f'dl_pp_outline_emit: cell {i} produced {int(stored[i])} items, the count pass {int(items[i])} (the mask changed between the passes?)')
    out = out_d.cpu().numpy()
    t0 = time.perf_counter()
    if strings:
        blob = out.tobytes().decode('ascii')
        offs = offsets.tolist()
        res = [blob[a:b] for a, b in zip(offs[:-1], offs[1:])]
    else:
        # two bulk conversions: the per-cell rows (moved by the offset in numpy) and every kept point of every cell
        rows = np.empty((n, 11), dtype=np.int64)
        rows[:, 0], rows[:, 1], rows[:, 2] = table[:, 2], table[:, 3], table[:, 4]
        rows[:, 3:7] = counts[:, 1:5].astype(np.int64) + np.array([ox, oy, ox, oy], dtype=np.int64)
        rows[:, 7], rows[:, 8] = table[:, 5].astype(np.int64) + ox, table[:, 6].astype(np.int64) + oy
        rows[:, 9], rows[:, 10] = offsets[:-1], offsets[1:]
        # (a million small tuples and lists: the cyclic collector, which would rescan them again and again while they are made, waits)
        import gc
        pause = gc.isenabled()
        if pause:
            gc.disable()
        try:
            flat = out.ravel().tolist()
            pts = list(zip(flat[0::2], flat[1::2]))
            key = 'od' if version in (5, 6) else 'marker'
            res = [{'size': size, 'positive': bool(positive), key: value, 'bbox': [(x0, y0), (x1, y1)], 'centroid': (cx, cy), 'boundary': pts[a:b]}
                   for size, positive, value, x0, y0, x1, y1, cx, cy, a, b in rows.tolist()]
        finally:
            if pause:
                gc.enable()
    if timings is not None:
        timings['python'] = timings.get('python', 0.0) + (time.perf_counter() - t0)
    return res


def compute_cell_results(seg, marker, resolution, version=3, seg_thresh=DEFAULT_SEG_THRESH, noise_thresh=DEFAULT_NOISE_THRESH,
                         large_noise_thresh=None, device=None, route=None, offset=(0, 0)):
    """deepliif/postprocessing.py:1136-1220: individual cell data.  Versions 3 / 4 take the inferred marker image, 5 / 6 the ORIGINAL image
    (optical density); 4 / 6 return every cell as one encoded ASCII string.
    route: 'gpu' = outline_cells (the label mask stays on the device), 'host' = cell_results_from_mapping on a host copy of the mask (the
    yardstick), None = 'gpu' when the library exports the outline kernels, else 'host'.  offset: position of this image inside a slide
    (infer_cells_for_wsi, models/__init__.py:883-903), added to every coordinate; (0, 0) is the reference's compute_cell_results."""
    import warnings
    if version not in (3, 4, 5, 6):
        warnings.warn('Invalid cell data version provided, defaulting to version 3.')
        version = 3
    if route is None:
        route = 'gpu' if hasattr(ops.impl().lib, 'dl_pp_outline_emit') else 'host'
    if route not in ('gpu', 'host'):
        raise ValueError(f"unknown route {route!r} ('gpu' | 'host')")
    large = calculate_large_noise_thresh(large_noise_thresh, resolution)
    cm = get_cells_info(seg, marker, resolution, noise_thresh, seg_thresh, large, use_od=version in (5, 6), device=device)
    if route == 'host':
        return cell_results_from_mapping(cm.mask.cpu().numpy(), cm.cells, cm.defaults, version, seg_thresh, noise_thresh, large, offset=offset)
    cells = outline_cells(cm.mask, cm.table, version, offset)
    return {'cells': cells, 'settings': _cell_settings(cm.defaults, version, seg_thresh, noise_thresh, large), 'dataVersion': version}


# ---------------------------------------------------------------------------------------------------------------
# Rendering a STORED cell list (cells_to_final_results, postprocessing.py:1307-1412): overlay, refined image and scoring from the output of
# compute_cell_results under new thresholds, without a network or the segmentation post-processing.  route 'gpu' = dl_pp_render_count /
# _paint / _finish; route 'host' = the numpy restatement below (no numba), the yardstick the GPU route is held to.  Both start from the
# flattened form of the list (PackedCells) and share the per-cell contract of include/deepliif_hip.h: a row {status, class, extent of the
# vertices, pixels of the full outline} per cell, and "the last counted cell in list order owns an outline pixel".
# ---------------------------------------------------------------------------------------------------------------
RENDER_OK, RENDER_MALFORMED, RENDER_BAD_SEGMENT, RENDER_OUTSIDE = 0, 1, 2, 3
RENDER_STATUS = {RENDER_MALFORMED: 'the stored cell is malformed (no outline point; or its string ends before its header or its numbers, or holds a character outside 35 .. 126)',
                 RENDER_BAD_SEGMENT: 'two consecutive outline points (or the last and the first) are not joined by one of the eight pixel directions',
                 RENDER_OUTSIDE: 'an outline point lies outside the image'}
_MODE_POINTS, _MODE_STRINGS = 0, 1
_LABEL_UNKNOWN, _LABEL_POSITIVE, _LABEL_NEGATIVE, _LABEL_BACKGROUND, _LABEL_BORDER_POS, _LABEL_BORDER_NEG = 50, 200, 150, 0, 220, 170


class PackedCells:
    """A cell list flattened once (pack_cells): versions 4 / 6 as one byte buffer + int64 offsets, versions 3 / 5 as int32 points + int64
    offsets + an int32 [n][4] table {size, positive, marker or optical-density value, 0}.  `host` holds the numpy arrays, `dev` the same
    arrays on `device` (None for a list packed for the host route)."""

    def __init__(self, version, settings, mode, data, offsets, table, device=None):
        self.version, self.settings, self.mode, self.n = version, dict(settings), mode, int(len(offsets) - 1)
        self.host = (data, offsets, table)
        self.device = device
        self.dev = None
        if device is not None:
            up = lambda a: None if a is None else torch.from_numpy(a).to(device)
            self.dev = (up(data), up(offsets), up(table))

    @property
    def items(self):
        return int(self.host[0].shape[0])


def pack_cells(data, device=None, upload=True) -> PackedCells:
    """The dict compute_cell_results returns (or a stored copy of it: {'cells', 'settings', 'dataVersion'}) -> PackedCells on `device`
    (default: the current CUDA device).  A second cells_to_final_results call on the result costs kernels only.  upload=False keeps the
    arrays on the host (all that route='host' needs)."""
    version = data['dataVersion']
    if version not in (3, 4, 5, 6):
        raise ValueError(f'unknown cell data version {version!r} (3 .. 6)')
    cells = data['cells']
    n = len(cells)
    offsets = np.zeros(n + 1, dtype=np.int64)
    table = None
    if version in (4, 6):
        try:
            raw = [c.encode('latin-1') for c in cells]
        except (UnicodeEncodeError, AttributeError):
            i = next(j for j, c in enumerate(cells) if not isinstance(c, str) or any(ord(ch) > 255 for ch in c))
            raise ValueError(f'cell {i} of {n}: not a version-{version} string of characters 35 .. 126') from None
        np.cumsum([len(r) for r in raw], out=offsets[1:])
        flat = np.frombuffer(b''.join(raw), dtype=np.uint8).copy()
        mode = _MODE_STRINGS
    else:
        from itertools import chain
        key = 'od' if version == 5 else 'marker'
        np.cumsum([len(c['boundary']) for c in cells], out=offsets[1:])
        pts = np.fromiter(chain.from_iterable(chain.from_iterable(c['boundary'] for c in cells)), dtype=np.int64).reshape(-1, 2)
        tab = np.zeros((n, 4), dtype=np.int64)
        if n:
            tab[:, 0] = [c['size'] for c in cells]
            tab[:, 1] = [bool(c['positive']) for c in cells]
            tab[:, 2] = [c.get(key, 0) for c in cells]
        lim = 2 ** 31 - 1
        if (len(pts) and (pts.min() < -lim or pts.max() > lim)) or (n and (tab.min() < -lim or tab.max() > lim)):
            raise ValueError('a coordinate, size or marker value of the cell list does not fit 32 bits')
        flat, table, mode = np.ascontiguousarray(pts, dtype=np.int32), tab.astype(np.int32), _MODE_POINTS
    dev = None
    if upload:
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    return PackedCells(version, data['settings'], mode, flat, offsets, table, dev)


def _render_thresholds(version, settings, size_thresh, marker_thresh, size_thresh_upper, od_thresh_lower, od_thresh_upper):
    """:1346-1361 -> (the thresholds as the scoring reports them, the same as dl_pp_render_thresh: integer bounds that decide like the given
    numbers do on integer sizes and values -- x > t iff x > floor(t), x < t iff x < ceil(t))"""
    if version in (3, 4):
        od_thresh_lower = od_thresh_upper = None
    else:
        marker_thresh = None
    if size_thresh is None:
        size_thresh = 0
    elif isinstance(size_thresh, str) and size_thresh == 'default':
        size_thresh = settings['default_size_thresh']
    if isinstance(marker_thresh, str) and marker_thresh == 'default':
        marker_thresh = settings['default_marker_thresh']
    big = 1 << 62

    def bound(v, up):
        if v is None:
            return 0, 0
        if v != v:
            raise ValueError('a threshold is not a number')
        v = max(-big, min(big, v))
        return int(math.ceil(v) if up else math.floor(v)), 1

    th = L.RenderThresh()
    th.size_lower = bound(size_thresh, False)[0]
    th.size_upper, th.has_size_upper = bound(size_thresh_upper, True)
    th.marker, th.has_marker = bound(marker_thresh, False)
    th.od_lower, th.has_od_lower = bound(od_thresh_lower, True)
    th.od_upper, th.has_od_upper = bound(od_thresh_upper, False)
    return {'size_thresh': size_thresh, 'size_thresh_upper': size_thresh_upper, 'marker_thresh': marker_thresh}, th


def _render_class(size, positive, value, th, v6) -> int:
    """:1371-1380 -> 0 not counted / 1 positive / 2 negative"""
    if not (size > th.size_lower and (not th.has_size_upper or size < th.size_upper)):
        return 0
    pos = bool(positive)
    if not v6 and th.has_marker and value > th.marker:
        pos = True
    if v6:
        if th.has_od_lower and value < th.od_lower:
            pos = False
        elif th.has_od_upper and value > th.od_upper:
            pos = False
    return 1 if pos else 2


def _render_vertices(packed, i):
    """cell i of a host-side PackedCells -> (size, positive, value, [(x, y), ...]); None when not even the numbers can be read, and no
    point list when only the chain is malformed.  Strings are decoded like decode_cell_data_v4 does, with every byte checked; every chain
    character is one vertex (a repeated direction changes no pixel)."""
    data, offsets, table = packed.host
    b, e = int(offsets[i]), int(offsets[i + 1])
    if b < 0 or e <= b or e > len(data):
        return None
    if packed.mode == _MODE_POINTS:
        return int(table[i, 0]), int(table[i, 1]), int(table[i, 2]), [(int(x), int(y)) for x, y in data[b:e].tolist()]
    s = data[b:e].tolist()
    bad = lambda part: any(c < 35 or c > 126 for c in part)
    if bad(s[:1]):
        return None
    n = s[0] - 35
    w_size, w_tl, w_off = n // 16 + 1, (n // 4) % 4 + 1, n % 4 + 1
    head = 1 + w_size + 2 + 2 * w_tl + 6 * w_off
    if len(s) < head or bad(s[:head]):
        return None
    pos = 1
    nums = []
    for w in (w_size, 2, w_tl, w_tl) + (w_off,) * 6:
        v = 0
        for c in s[pos:pos + w]:
            v = v * 92 + (c - 35)
        nums.append(v)
        pos += w
    size, cls, ax, ay = nums[:4]
    if bad(s[head:]):
        return size, cls % 2, cls // 2, None
    x, y = ax + nums[8], ay + nums[9]
    pts = [(x, y)]
    for c in s[head:]:
        steps, code = divmod(c - 35, 8)
        dx, dy = _FREEMAN_STEP[code]
        x, y = x + dx * steps, y + dy * steps
        pts.append((x, y))
    return size, cls % 2, cls // 2, pts


def render_rows_host(packed, th, offset, H, W, paint=True):
    """The host statement of dl_pp_render_count (+ _paint): -> (rows int32 [n][8], owner int32 [H][W] or None).  Sequential, in list order:
    a later cell overwrites an earlier one (= the maximum index the kernel keeps)."""
    v6 = packed.version in (5, 6)
    ox, oy = int(offset[0]), int(offset[1])
    sat = lambda v: max(-2 ** 31, min(2 ** 31 - 1, v))
    rows = np.zeros((packed.n, 8), dtype=np.int32)
    outlines = []
    for i in range(packed.n):
        c = _render_vertices(packed, i)
        rows[i, 0] = RENDER_MALFORMED
        if c is None:
            outlines.append(None)
            continue
        size, positive, value, pts = c
        rows[i, 1] = _render_class(size, positive, value, th, v6)
        if pts is None:
            outlines.append(None)
            continue
        pts = [(x - ox, y - oy) for x, y in pts]
        bad, pixels = False, 1
        for (ax, ay), (bx, by) in zip(pts, pts[1:] + pts[:1]):
            dx, dy = abs(bx - ax), abs(by - ay)
            bad |= dx != 0 and dy != 0 and dx != dy
            pixels += max(dx, dy)
        dx, dy = abs(pts[0][0] - pts[-1][0]), abs(pts[0][1] - pts[-1][1])
        pixels -= min(max(dx, dy), 1)                                  # the closing run stops in front of the first point
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        rows[i, 2:7] = [sat(min(xs)), sat(min(ys)), sat(max(xs)), sat(max(ys)), sat(pixels)]
        rows[i, 0] = RENDER_BAD_SEGMENT if bad else (RENDER_OUTSIDE if min(xs) < 0 or min(ys) < 0 or max(xs) >= W or max(ys) >= H else RENDER_OK)
        outlines.append(pts if rows[i, 0] == RENDER_OK and rows[i, 1] != 0 else None)
    if not paint:
        return rows, None
    owner = np.full((H, W), -1, dtype=np.int32)
    sgn = lambda v: (v > 0) - (v < 0)
    for i, pts in enumerate(outlines):
        if pts is None:
            continue
        full = [pts[0]]                                                # make_full_contour (:637-682)
        for p in pts[1:] + pts[:1]:
            x, y = full[-1]
            dx, dy = sgn(p[0] - x), sgn(p[1] - y)
            for _ in range(max(abs(p[0] - x), abs(p[1] - y))):
                x, y = x + dx, y + dy
                full.append((x, y))
        if len(full) > 1 and full[-1] == full[0]:
            full.pop()
        a = np.asarray(full, dtype=np.int64)
        owner[a[:, 1], a[:, 0]] = i
    return rows, owner


def render_mask_host(owner, rows):
    """owner map + classes -> the final label mask: mark_background (:194-232), fill_cells (:1075-1099), create_outer_boundary (:1103-1122),
    enlarge_cell_boundaries (:1003-1030) twice, as whole-array numpy statements of the five order-free rules"""
    H, W = owner.shape
    cls = np.concatenate([rows[:, 1].astype(np.int64), [0]])          # owner -1 -> the appended 0
    oc = cls[owner]
    mask = np.where(owner < 0, _LABEL_UNKNOWN, np.where(oc == 1, _LABEL_BORDER_POS, _LABEL_BORDER_NEG)).astype(np.uint8)
    # background: flood fill of the UNKNOWN pixels from the image border, 4-connected (a frame of a non-UNKNOWN value stops the walk)
    pad = np.full((H + 2, W + 2), 255, dtype=np.uint8)
    pad[1:-1, 1:-1] = mask
    flat = bytearray(pad.tobytes())
    S = W + 2
    border = np.zeros((H, W), dtype=bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    ys, xs = np.nonzero(border & (mask == _LABEL_UNKNOWN))
    stack = ((ys + 1) * S + xs + 1).tolist()
    for p in stack:
        flat[p] = _LABEL_BACKGROUND
    while stack:
        p = stack.pop()
        for q in (p - S, p - 1, p + 1, p + S):
            if flat[q] == _LABEL_UNKNOWN:
                flat[q] = _LABEL_BACKGROUND
                stack.append(q)
    mask = np.frombuffer(bytes(flat), dtype=np.uint8).reshape(H + 2, S)[1:-1, 1:-1].copy()
    # fill: an UNKNOWN pixel takes the class of the nearest pixel to its left that is not UNKNOWN
    known = mask != _LABEL_UNKNOWN
    src = np.maximum.accumulate(np.where(known, np.arange(W)[None, :], -1), axis=1)
    left = np.take_along_axis(mask, np.maximum(src, 0), axis=1)
    fill = np.where((src >= 0) & (left == _LABEL_BORDER_POS), _LABEL_POSITIVE, _LABEL_NEGATIVE).astype(np.uint8)
    mask = np.where(known, mask, fill)
    mask[mask == _LABEL_BORDER_POS] = _LABEL_POSITIVE
    mask[mask == _LABEL_BORDER_NEG] = _LABEL_NEGATIVE

    def shifted(m, dy, dx):
        """m[y + dy, x + dx], 0 outside"""
        out = np.zeros_like(m)
        out[max(-dy, 0):H - max(dy, 0), max(-dx, 0):W - max(dx, 0)] = m[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)]
        return out

    # outer boundary: the first POSITIVE / NEGATIVE neighbour among up, left, right, down
    out = mask.copy()
    todo = mask == _LABEL_BACKGROUND
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
        nb = shifted(mask, dy, dx)
        for lab, border_lab in ((_LABEL_POSITIVE, _LABEL_BORDER_POS), (_LABEL_NEGATIVE, _LABEL_BORDER_NEG)):
            hit = todo & (nb == lab)
            out[hit] = border_lab
            todo &= ~hit
    mask = out
    for _ in range(2):                                                 # enlarge: the first border neighbour of the 8, in raster order
        out = mask.copy()
        todo = mask == _LABEL_BACKGROUND
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy == 0 and dx == 0:
                    continue
                nb = shifted(mask, dy, dx)
                hit = todo & ((nb == _LABEL_BORDER_POS) | (nb == _LABEL_BORDER_NEG))
                out[hit] = nb[hit]
                todo &= ~hit
        mask = out
    return mask


def _final_images_host(orig, mask):
    """create_final_images (:1033-1071)"""
    overlay, refined = orig.copy(), np.zeros_like(orig)
    overlay[mask == _LABEL_BORDER_POS] = (255, 0, 0)
    overlay[mask == _LABEL_BORDER_NEG] = (0, 0, 255)
    refined[..., 1][(mask == _LABEL_BORDER_POS) | (mask == _LABEL_BORDER_NEG)] = 255
    refined[..., 0][mask == _LABEL_POSITIVE] = 255
    refined[..., 2][mask == _LABEL_NEGATIVE] = 255
    return overlay, refined


def _render_refusals(rows, n, outside):
    """raises for the first cell the count pass refused: a malformed cell always (the reference decodes every cell), a bad segment or
    (outside='raise') a vertex outside the image only for a COUNTED cell (the reference never rasterises the others)"""
    st, cl = rows[:, 0], rows[:, 1]
    bad = (st == RENDER_MALFORMED) | ((cl != 0) & ((st == RENDER_BAD_SEGMENT) | ((st == RENDER_OUTSIDE) & (outside == 'raise'))))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        hint = "; outside='skip' leaves such cells out" if st[i] == RENDER_OUTSIDE else ''
        raise ValueError(f'cells_to_final_results: cell {i} of {n}: {RENDER_STATUS[int(st[i])]} (vertices span x {int(rows[i, 2])} .. {int(rows[i, 4])}, '
                         f'y {int(rows[i, 3])} .. {int(rows[i, 5])}){hint}')


def cells_to_final_results(data, orig, size_thresh='default', marker_thresh=None, size_thresh_upper=None, od_thresh_lower=None, od_thresh_upper=None,
                           *, route='gpu', offset=(0, 0), outside='raise', return_tensors: bool = False, device=None):
    """deepliif/postprocessing.py:1307-1412 -> (overlay, refined, scoring) from stored cell data.  data: the dict of compute_cell_results (any
    data version) or a PackedCells; orig: PIL image, uint8 ndarray or uint8 CUDA tensor (H x W x 3).  Versions 3 / 4 ignore the optical-density
    thresholds, 5 / 6 the marker threshold.
    route: 'gpu' (dl_pp_render_*) or 'host' (numpy, the yardstick).  offset: subtracted from every coordinate (slide-level lists);
    outside: 'raise' = ValueError for the first counted cell with an outline point outside the image, 'skip' = such cells are neither painted
    nor counted.  return_tensors / device as compute_final_results."""
    if route not in ('gpu', 'host'):
        raise ValueError(f"unknown route {route!r} ('gpu' | 'host')")
    if outside not in ('raise', 'skip'):
        raise ValueError(f"unknown outside {outside!r} ('raise' | 'skip')")
    ox, oy = int(offset[0]), int(offset[1])
    if isinstance(data, PackedCells):
        packed = data
    else:
        packed = pack_cells(data, device, upload=(route == 'gpu'))
    shown, th = _render_thresholds(packed.version, packed.settings, size_thresh, marker_thresh, size_thresh_upper, od_thresh_lower, od_thresh_upper)
    n = packed.n
    if route == 'host':
        if isinstance(orig, torch.Tensor):
            orig_np = orig.cpu().numpy()
        else:
            orig_np = _to_u8_cuda(orig, 'cpu').numpy()
        H, W = orig_np.shape[:2]
        rows, owner = render_rows_host(packed, th, (ox, oy), H, W)          # (paints the cells it found in order only)
        _render_refusals(rows, n, outside)
        overlay, refined = _final_images_host(orig_np, render_mask_host(owner, rows))
        if return_tensors:
            overlay, refined = torch.from_numpy(overlay), torch.from_numpy(refined)
    else:
        lib = ops.impl().lib
        dev = torch.device(device) if device is not None else (packed.device or (orig.device if isinstance(orig, torch.Tensor) and orig.is_cuda
                                                                                   else torch.device('cuda', torch.cuda.current_device())))
        if packed.dev is None or packed.device != dev:
            packed = PackedCells(packed.version, packed.settings, packed.mode, *packed.host, device=dev)
        orig_t = _to_u8_cuda(orig, dev)
        H, W = int(orig_t.shape[0]), int(orig_t.shape[1])
        ops._need_cuda(orig_t)
        nbytes = int(lib.dl_pp_render_ws_bytes(H, W))
        if nbytes == 0:
            raise RuntimeError('dl_pp_render_ws_bytes failed (empty or too large image)')
        data_d, offsets_d, table_d = packed.dev
        p, stream = ops._ptr, ops._stream(orig_t)
        rows_d = torch.empty((max(n, 1), 8), dtype=torch.int32, device=dev)
        L.check(lib.dl_pp_render_count(packed.mode, 1 if packed.version in (5, 6) else 0, p(data_d), packed.items, p(offsets_d), p(table_d), n,
                                       C.byref(th), ox, oy, H, W, p(rows_d), stream), 'dl_pp_render_count', lib)
        rows = rows_d[:n].cpu().numpy()
        _render_refusals(rows, n, outside)
        owner = torch.empty((H, W), dtype=torch.int32, device=dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        overlay = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        refined = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        L.check(lib.dl_pp_render_paint(packed.mode, p(data_d), packed.items, p(offsets_d), n, p(rows_d), ox, oy, H, W, p(owner), stream),
                'dl_pp_render_paint', lib)
        L.check(lib.dl_pp_render_finish(p(orig_t), orig_t.stride(0), p(owner), p(rows_d), n, p(ws), H, W, p(overlay), overlay.stride(0),
                                        p(refined), refined.stride(0), stream), 'dl_pp_render_finish', lib)
        if not return_tensors:
            overlay, refined = overlay.cpu().numpy(), refined.cpu().numpy()
    counted = rows[:, 0] == RENDER_OK
    num_pos, num_neg = int((counted & (rows[:, 1] == 1)).sum()), int((counted & (rows[:, 1] == 2)).sum())
    num_total = num_pos + num_neg
    scoring = {'num_total': num_total, 'num_pos': num_pos, 'num_neg': num_neg,
               'percent_pos': round(num_pos / num_total * 100, 1) if num_pos > 0 else 0,
               'seg_thresh': packed.settings['seg_thresh'], 'size_thresh': shown['size_thresh'], 'size_thresh_upper': shown['size_thresh_upper'],
               'marker_thresh': shown['marker_thresh']}
    return overlay, refined, scoring
