"""Cases for rendering stored cell data (cells_to_final_results), shared by tests/golden/make_golden_cells_render.py,
test_cells_render_host.py and test_gpu_cells_render.py.  The cell lists are those of tests/golden/cells_wsi_cases.npz (read at offset
0_0, not stored twice) plus a few hand-written version-3 lists; tests/golden/cells_render_cases.npz holds what the REFERENCE renders."""
import os

import numpy as np

from golden_util import load_npz

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
N_SETS = 5
RENDER_OFFSETS = [(92, 5), (8463, 8464)]          # two non-zero entries of outline_cases.OFFSETS
SKIP_CASE, SKIP_OFFSET, SKIP_WINDOW = 'synth_40x', (92, 5), (60, 60)          # the shifted list rendered into the top-left H x W window


def cell_lists():
    return load_npz(os.path.join(GOLDEN, 'cells_wsi_cases.npz'))


def expected():
    return load_npz(os.path.join(GOLDEN, 'cells_render_cases.npz'))


def stored(Z, name, version, offset=(0, 0)):
    """the dict compute_cell_results returned for one case, as the fixture recorded it"""
    cells = eval(str(Z[f'{name}/cells_v{version}/{offset[0]}_{offset[1]}']), {'np': np})
    return {'cells': cells, 'settings': eval(str(Z[f'{name}/settings_v{version}']), {'np': np}), 'dataVersion': version}


def threshold_sets(sizes):
    """the five threshold sets of every case; sizes = the cell sizes of the list"""
    s = sorted(int(v) for v in sizes)
    median, largest = (s[len(s) // 2], s[-1]) if s else (0, 0)
    return [{},
            dict(size_thresh=None),
            dict(size_thresh=median, size_thresh_upper=largest),          # cuts cells out from both sides
            dict(size_thresh=None, marker_thresh='default', od_thresh_lower=20, od_thresh_upper=60),
            dict(size_thresh=None, marker_thresh=0, od_thresh_lower=0)]


def pair(version):
    """versions 3 / 4 and 5 / 6 give identical pictures and scoring: one stored result per pair"""
    return 'marker' if version in (3, 4) else 'od'


def _cell(size, positive, marker, pts):
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    return {'size': size, 'positive': positive, 'marker': marker, 'bbox': [(min(xs), min(ys)), (max(xs), max(ys))],
            'centroid': (sum(xs) // len(xs), sum(ys) // len(ys)), 'boundary': pts}


def _square(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


HAND_SHAPE = (24, 24)
_SETTINGS = {'default_size_thresh': 0, 'noise_thresh': 4, 'large_noise_thresh': None, 'seg_thresh': 120, 'default_marker_thresh': 100}
_A = _cell(81, True, 150, _square(2, 2, 10, 10))
_B = _cell(81, False, 30, _square(6, 6, 14, 14))          # its outline crosses _A's at (10, 6) and (6, 10)


def hand_lists():
    """name -> (version-3 data, keyword arguments)"""
    lists = {
        'squares_pos_then_neg': ([_A, _B], {}),          # the later cell owns the shared outline pixels
        'squares_neg_then_pos': ([_B, _A], {}),
        'one_point': ([_cell(1, True, 10, [(18, 3)])], {}),
        'two_points': ([_cell(5, False, 10, [(16, 8), (20, 8)])], {}),
        'two_points_diagonal': ([_cell(5, True, 10, [(3, 20), (6, 17)])], {}),
        'along_all_four_borders': ([_cell(576, True, 10, _square(0, 0, 23, 23))], {}),
        'counted_next_to_uncounted': ([_cell(5, True, 200, _square(3, 15, 7, 19)), _cell(25, False, 20, _square(8, 15, 12, 19))], dict(size_thresh=10)),
        'everything': ([_A, _cell(1, True, 10, [(18, 3)]), _B, _cell(5, False, 10, [(16, 8), (20, 8)]), _cell(25, True, 20, _square(8, 15, 12, 19)),
                        _cell(30, False, 120, _square(14, 16, 21, 22))], dict(marker_thresh='default')),
    }
    return {k: ({'cells': c, 'settings': dict(_SETTINGS), 'dataVersion': 3}, kw) for k, (c, kw) in lists.items()}


def hand_orig():
    rng = np.random.RandomState(7)
    return rng.randint(1, 255, size=HAND_SHAPE + (3,)).astype(np.uint8)


# one byte per pixel: 0 nothing, 1 positive fill, 2 negative fill, 3 positive border, 4 negative border
def code_from_images(orig, overlay, refined):
    code = np.zeros(orig.shape[:2], dtype=np.uint8)
    code[refined[..., 0] == 255] = 1
    code[refined[..., 2] == 255] = 2
    border = refined[..., 1] == 255
    code[border & (overlay == (255, 0, 0)).all(axis=2)] = 3
    code[border & (overlay == (0, 0, 255)).all(axis=2)] = 4
    return code


def images_from_code(orig, code):
    overlay, refined = np.array(orig, copy=True), np.zeros_like(orig)
    overlay[code == 3] = (255, 0, 0)
    overlay[code == 4] = (0, 0, 255)
    refined[..., 0][code == 1] = 255
    refined[..., 2][code == 2] = 255
    refined[..., 1][code >= 3] = 255
    return overlay, refined
