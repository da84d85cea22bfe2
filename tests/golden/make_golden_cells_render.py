"""Fixtures for rendering stored cell data: what the REFERENCE's cells_to_final_results (deepliif/postprocessing.py:1307-1412) makes of the
cell lists of cells_wsi_cases.npz under five threshold sets.

  python tests/golden/make_golden_cells_render.py        ->  tests/golden/cells_render_cases.npz

The cell lists are read from cells_wsi_cases.npz (offset 0_0) and not stored again.  Per case, version pair (3 / 4 and 5 / 6 give identical
results, asserted here) and threshold set (tests/cells_render_cases.py): the reference's pictures as one uint8 code per pixel (0 nothing,
1 positive fill, 2 negative fill, 3 positive border, 4 negative border; asserted here to give both images back exactly, together with
orig) and its scoring as a repr() string.  The lists at a non-zero offset, rendered with offset=, must give the result of the unshifted
list, so nothing is stored for them.  'skip/...': the list shifted by SKIP_OFFSET rendered into a window that cuts cells off = the
reference on the unshifted list without those cells.  'hand/...': hand-written version-3 lists on a 24 x 24 image.  Same stubs and the
same create_od_image widening as make_golden_cells_wsi.py (the widening does not matter here: no image is converted)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_import import install_stubs          # noqa: E402
from golden_util import save_npz               # noqa: E402
import cells_render_cases as RC                # noqa: E402


def main():
    install_stubs()
    import importlib.util
    spec = importlib.util.spec_from_file_location('ref_postprocessing', '/root/reference/deepliif/postprocessing.py')
    P = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(P)
    _od = P.create_od_image
    P.create_od_image = lambda o: _od(o).astype(np.int64)

    def render(data, orig, kw):
        overlay, refined, scoring = P.cells_to_final_results(data, orig.copy(), **kw)
        code = RC.code_from_images(orig, overlay, refined)
        ov, rf = RC.images_from_code(orig, code)
        assert np.array_equal(ov, overlay) and np.array_equal(rf, refined), 'the code does not give the images back'
        return code, scoring

    Z = RC.cell_lists()
    out = {'names': np.array([str(n) for n in Z['names']])}
    for name in out['names']:
        orig = Z[f'{name}/orig']
        sizes = [c['size'] for c in RC.stored(Z, name, 3)['cells']]
        sets = RC.threshold_sets(sizes)
        for k, kw in enumerate(sets):
            got = {v: render(RC.stored(Z, name, v), orig, kw) for v in (3, 4, 5, 6)}
            for a, b in ((3, 4), (5, 6)):
                assert np.array_equal(got[a][0], got[b][0]) and got[a][1] == got[b][1], (name, k, a, b)
                out[f'{name}/{RC.pair(a)}/{k}/code'] = got[a][0]
                out[f'{name}/{RC.pair(a)}/{k}/scoring'] = np.array(repr(got[a][1]))
        print(name, len(sizes), 'cells', [eval(str(out[f'{name}/marker/{k}/scoring']))['num_total'] for k in range(len(sets))])
    # the shifted list in a window: the cells with a vertex outside the window are left out
    (ox, oy), (h, w) = RC.SKIP_OFFSET, RC.SKIP_WINDOW
    orig = np.ascontiguousarray(Z[f'{RC.SKIP_CASE}/orig'][:h, :w])
    for v in (3, 4, 5, 6):
        data = RC.stored(Z, RC.SKIP_CASE, v)
        decoded = [P.decode_cell_data_v4(c, v6=(v == 6)) if v in (4, 6) else c for c in data['cells']]
        keep = [i for i, c in enumerate(decoded) if all(0 <= x < w and 0 <= y < h for x, y in c['boundary'])]
        assert 0 < len(keep) < len(decoded)
        data['cells'] = [data['cells'][i] for i in keep]
        code, scoring = render(data, orig, dict(size_thresh=None))
        out[f'skip/v{v}/code'], out[f'skip/v{v}/scoring'], out[f'skip/v{v}/kept'] = code, np.array(repr(scoring)), np.array(keep, dtype=np.int64)
        print('skip', v, len(keep), 'of', len(decoded), 'cells kept')
    horig = RC.hand_orig()
    for name, (data, kw) in RC.hand_lists().items():
        code, scoring = render(data, horig, kw)
        out[f'hand/{name}/code'], out[f'hand/{name}/scoring'] = code, np.array(repr(scoring))
        print('hand', name, scoring)
    path = os.path.join(HERE, 'cells_render_cases.npz')
    save_npz(path, out)
    assert not os.path.exists(path[:-4] + '.1.npz'), 'the fixture must stay one file'
    print(os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
