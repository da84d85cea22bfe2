"""Fixtures for the slide-level cell data (deepliif.models.infer_cells_for_wsi, models/__init__.py:785-947): what the REFERENCE makes of a
region's cells when the region does not start at (0, 0).

  python tests/golden/make_golden_cells_wsi.py        ->  tests/golden/cells_wsi_cases.npz

Per case (a few golden_util.synth_cells images and the hand-made shapes of tests/outline_cases.py as segmentation images) and data version
3 - 6: the reference's compute_cell_results (postprocessing.py:1136-1220; same stubs and the same int64 widening as make_golden_post.py),
then, for every offset of outline_cases.OFFSETS, its cells after the loop of :883-903 -- decode_cell_data_v4 (versions 4 / 6), add the
offset to bbox, centroid and boundary, encode_cell_data_v4 -- carried out with the reference's own decode and encode functions.  Like the
reference, the loop is skipped for the offset (0, 0).  Stored as repr() strings, next to the input images and options, and the reference's
decode of every version-4 / -6 string."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_import import install_stubs          # noqa: E402
from golden_util import save_npz, synth_cells  # noqa: E402
import outline_cases as OC                     # noqa: E402

SYNTH = [
    # name, (H, W), seed, n_cells, resolution, options of compute_cell_results
    ('synth_40x', (64, 80), 21, 10, '40x', {}),
    ('synth_wide_20x', (40, 210), 22, 16, '20x', {}),                 # cells that start at x >= 92: two-digit top-left numbers without an offset
    ('synth_noise_10x', (50, 60), 23, 8, '10x', dict(noise_thresh=1, large_noise_thresh='default')),
]
HAND = [('single_pixel', dict(noise_thresh=0)), ('line_horizontal', {}), ('line_vertical', {}), ('line_diagonal', dict(noise_thresh=0)),
        ('blobs_joined_diagonally', {}), ('u_shape', {}), ('spiral', {}), ('touches_four_borders', {}), ('fills_the_image', {}),
        ('image_1x37', {}), ('image_61x1', {}), ('bar_11x3', {}), ('bar_21x3', {}), ('bar_25x3', {}), ('bar_45x3', {}), ('bar_3x25', {}),
        ('square_100', dict(large_noise_thresh=None)), ('starts_at_x_95', {})]


def moved(P, cells, version, offset):
    """models/__init__.py:883-903 with start_x, start_y = offset"""
    if tuple(offset) == (0, 0):
        return cells
    ox, oy = offset
    out = []
    for c in cells:
        cell = P.decode_cell_data_v4(c, v6=(version == 6)) if version in (4, 6) else copy.deepcopy(c)
        cell['bbox'] = [(px + ox, py + oy) for px, py in cell['bbox']]
        cell['centroid'] = (cell['centroid'][0] + ox, cell['centroid'][1] + oy)
        cell['boundary'] = [(px + ox, py + oy) for px, py in cell['boundary']]
        out.append(P.encode_cell_data_v4(cell, v6=(version == 6)) if version in (4, 6) else cell)
    return out


def main():
    install_stubs()
    import importlib.util
    spec = importlib.util.spec_from_file_location('ref_postprocessing', '/root/reference/deepliif/postprocessing.py')
    P = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(P)
    _od = P.create_od_image
    P.create_od_image = lambda o: _od(o).astype(np.int64)          # numba: uint16 + uint16 -> int64 (make_golden_post.py)
    wide = lambda a: a.astype(np.int64)
    cases = [(n, synth_cells(h, w, k, seed), res, kw) for n, (h, w), seed, k, res, kw in SYNTH]
    masks = OC.hand_masks()
    for n, kw in HAND:
        m = masks[n]
        orig = np.full(m.shape + (3,), 215, dtype=np.uint8)
        orig[m != 0] = (130, 90, 60)
        cases.append(('hand_' + n, (orig, OC.seg_from_mask(m), np.full(m.shape + (3,), 60, dtype=np.uint8)), '40x', kw))
    out = {'names': np.array([c[0] for c in cases]), 'offsets': np.array(OC.OFFSETS, dtype=np.int64)}
    for name, (orig, seg, marker), res, kw in cases:
        out[f'{name}/orig'], out[f'{name}/seg'], out[f'{name}/marker'] = orig, seg, marker
        out[f'{name}/resolution'], out[f'{name}/kwargs'] = np.array(res), np.array(repr(kw))
        for version in (3, 4, 5, 6):
            r = P.compute_cell_results(wide(seg), orig.copy() if version >= 5 else wide(marker), res, version=version, **kw)
            out[f'{name}/settings_v{version}'] = np.array(repr(r['settings']))
            if version in (4, 6):
                out[f'{name}/decoded_v{version}'] = np.array(repr([P.decode_cell_data_v4(c, v6=(version == 6)) for c in r['cells']]))
            for ox, oy in OC.OFFSETS:
                out[f'{name}/cells_v{version}/{ox}_{oy}'] = np.array(repr(moved(P, r['cells'], version, (ox, oy))))
        print(name, len(r['cells']), 'cells')
    save_npz(os.path.join(HERE, 'cells_wsi_cases.npz'), out)


if __name__ == '__main__':
    main()
