"""Host side of the slide-level cell data (wsi.infer_slide_cells / merge_cell_results, postprocessing.decode_cell_data_v4 and the region
offset) against tests/golden/cells_wsi_cases.npz: the reference's compute_cell_results on small images, and its cells after the decode ->
shift -> encode loop of infer_cells_for_wsi (models/__init__.py:883-903) for five offsets.  No GPU: the cell mapping comes from the pinned
oracle, inference and the cell mapping of the slide driver are stubbed."""
import os

import numpy as np
import pytest

from deepliif_amd import postprocessing as PP
from deepliif_amd import wsi
from golden_util import load_npz

Z = load_npz(os.path.join(os.path.dirname(__file__), 'golden', 'cells_wsi_cases.npz'))
NAMES = [str(n) for n in Z['names']]
OFFSETS = [tuple(int(v) for v in o) for o in Z['offsets']]


def stored(name, version, offset):
    return eval(str(Z[f'{name}/cells_v{version}/{offset[0]}_{offset[1]}']))


def test_the_fixture_covers_what_it_is_for():
    import outline_cases as OC
    assert OFFSETS == OC.OFFSETS == [(0, 0), (91, 0), (92, 5), (8463, 8464), (20000, 40000)]
    assert len(NAMES) >= 20 and sum(len(stored(n, 4, (0, 0))) for n in NAMES) >= 40
    heads = {ord(s[0]) - 35 for n in NAMES for o in OFFSETS for s in stored(n, 4, o)}
    assert {h // 16 for h in heads} >= {0, 1, 2} and {(h // 4) % 4 for h in heads} == {0, 1, 2} and {h % 4 for h in heads} == {0, 1}


@pytest.mark.parametrize('v6', [False, True])
@pytest.mark.parametrize('name', NAMES)
def test_decode_inverts_encode(name, v6):
    version = 6 if v6 else 4
    for offset in OFFSETS:
        strings, dicts = stored(name, version, offset), stored(name, version - 1, offset)
        assert len(strings) == len(dicts)
        for s, d in zip(strings, dicts):
            got = PP.decode_cell_data_v4(s, v6=v6)
            assert got == d                                           # the version-3 / -5 dict of the same cell, boundary runs merged
            assert PP.encode_cell_data_v4(got, v6=v6) == s
    assert [PP.decode_cell_data_v4(s, v6=v6) for s in stored(name, version, (0, 0))] == eval(str(Z[f'{name}/decoded_v{version}']))


def test_decode_merges_consecutive_equal_directions():
    """a run of 24 steps is spelled as three characters of one direction and decodes to ONE point"""
    cell = {'size': 75, 'positive': True, 'marker': 60, 'bbox': [(1, 1), (25, 3)], 'centroid': (13, 2), 'boundary': [(1, 1), (25, 1), (25, 3), (1, 3)]}
    s = PP.encode_cell_data_v4(cell)
    assert len(s) == 1 + 1 + 2 + 2 + 6 + 3 + 1 + 3
    assert PP.decode_cell_data_v4(s) == cell


@pytest.mark.parametrize('name', NAMES)
def test_encoding_the_shifted_cell_is_the_references_decode_shift_encode(name):
    """what lets the kernel add the offset while it encodes: encode(shift(cell)) == encode(shift(decode(encode(cell))))"""
    for version in (3, 4, 5, 6):
        base = stored(name, 3 if version in (3, 4) else 5, (0, 0))
        for offset in OFFSETS:
            moved = [PP.shift_cell(d, offset) for d in base]
            if version in (4, 6):
                moved = [PP.encode_cell_data_v4(d, v6=(version == 6)) for d in moved]
            assert moved == stored(name, version, offset), (version, offset)


@pytest.mark.parametrize('version', [3, 4, 5, 6])
@pytest.mark.parametrize('name', NAMES)
def test_host_route_with_an_offset(name, version):
    from oracle import postprocess_oracle as PO
    kw = eval(str(Z[f'{name}/kwargs']))
    res = str(Z[f'{name}/resolution'])
    large = PO.large_noise_threshold(kw.get('large_noise_thresh'), res)
    od = version >= 5
    mask, cells, defaults, _, _ = PO.cells_info(Z[f'{name}/seg'], Z[f'{name}/orig'] if od else Z[f'{name}/marker'], res, kw.get('noise_thresh', 4),
                                                kw.get('seg_thresh', 120), large, od)
    for offset in OFFSETS:
        got = PP.cell_results_from_mapping(mask, cells, defaults, version, kw.get('seg_thresh', 120), kw.get('noise_thresh', 4), large, offset=offset)
        assert got['cells'] == stored(name, version, offset)
        assert got['settings'] == eval(str(Z[f'{name}/settings_v{version}'])) and got['dataVersion'] == version


# ---------------------------------------------------------------------------------------------------------------- the slide driver
def test_cell_region_grid():
    # 45 000 x 21 000 at 20 000: 3 x 2 regions of stride ceil(45000 / 3) x ceil(21000 / 2), rows first
    assert wsi.cell_region_grid(45000, 21000, 20000) == [(0, 0, 15000, 10500), (15000, 0, 15000, 10500), (30000, 0, 15000, 10500),
                                                         (0, 10500, 15000, 10500), (15000, 10500, 15000, 10500), (30000, 10500, 15000, 10500)]
    assert wsi.region_grid(45000, 21000, 20000)[1] == (0, 20000, 20000, 1000)          # ... which is not infer_slide's grid
    assert wsi.cell_region_grid(40000, 20000, 20000) == [(0, 0, 20000, 20000), (20000, 0, 20000, 20000)]          # an exact multiple
    assert wsi.cell_region_grid(300, 200, 20000) == [(0, 0, 300, 200)]                                               # smaller than one region
    # a stride that does not divide the size: 100 at 30 -> 4 regions of stride 25; 10 at 3 -> 4 regions of stride ceil(10 / 4) = 3, the last 1 wide
    assert [r[0] for r in wsi.cell_region_grid(100, 10, 30)] == [0, 25, 50, 75]
    assert wsi.cell_region_grid(10, 1, 3) == [(0, 0, 3, 1), (3, 0, 3, 1), (6, 0, 3, 1), (9, 0, 1, 1)]
    with pytest.raises(ValueError):
        wsi.cell_region_grid(0, 5, 3)


def _part(cells, size, marker='absent', version=3):
    st = {'default_size_thresh': size, 'noise_thresh': 4, 'large_noise_thresh': None, 'seg_thresh': 120}
    if marker != 'absent':
        st['default_marker_thresh'] = marker
    return {'cells': list(cells), 'settings': st, 'dataVersion': version}


def test_merge_cell_results_averages_like_the_reference():
    parts = [_part(['a'], 49, 100), _part([], 0, None), _part(['b', 'c'], 50, 0), _part(['d'], 0, 105)]
    m = wsi.merge_cell_results(parts, 512, 20000, [0.25, 0.15, 0.25, 0.1, 0.25], '/models/DeepLIIF_Latest_Model')
    assert m['cells'] == ['a', 'b', 'c', 'd'] and m['dataVersion'] == 3
    # size: (49 + 50) / 2 = 49.5 -> 50 (half to even); marker: (100 + 105) / 2 = 102.5 -> 102 (half to even); None and 0 do not count
    assert m['settings'] == {'default_size_thresh': 50, 'noise_thresh': 4, 'large_noise_thresh': None, 'seg_thresh': 120, 'default_marker_thresh': 102,
                             'tile_size': 512, 'region_size': 20000, 'seg_weights': [0.25, 0.15, 0.25, 0.1, 0.25]}
    assert m['modelVersion'] == 'DeepLIIF_Latest_Model'
    try:
        import importlib.metadata
        want = importlib.metadata.version('deepliif')
    except Exception:
        want = 'unknown'
    assert m['deepliifVersion'] == want
    assert [p['cells'] for p in parts] == [['a'], [], ['b', 'c'], ['d']]           # the parts are left alone
    # 50.5 -> 50, 51.5 -> 52
    assert wsi.merge_cell_results([_part([], 50, 1), _part([], 51, 1)], 256)['settings']['default_size_thresh'] == 50
    assert wsi.merge_cell_results([_part([], 51, 1), _part([], 52, 1)], 256)['settings']['default_size_thresh'] == 52
    # nothing counted: 0 / max(0, 1)
    z = wsi.merge_cell_results([_part([], 0, None), _part([], 0, 0)], 256, model_dir=None)
    assert z['settings']['default_size_thresh'] == 0 and z['settings']['default_marker_thresh'] == 0 and z['modelVersion'] == 'unknown'
    # versions 5 / 6 carry no marker threshold
    o = wsi.merge_cell_results([_part(['x'], 30, version=6), _part(['y'], 33, version=6)], 512, model_dir='m')
    assert 'default_marker_thresh' not in o['settings'] and o['settings']['default_size_thresh'] == 32 and o['cells'] == ['x', 'y']
    with pytest.raises(ValueError):
        wsi.merge_cell_results([], 512)


class _Stubs:
    """inference() returns images that name the region they were made from; compute_cell_results records what it was given"""

    def __init__(self, monkeypatch):
        from deepliif_amd import inference as I
        self.inference_calls, self.cell_calls = [], []
        monkeypatch.setattr(I, 'inference', self.inference)
        monkeypatch.setattr(I, 'get_opt', lambda model_dir: 'opt of ' + model_dir)
        monkeypatch.setattr(PP, 'compute_cell_results', self.compute_cell_results)

    def inference(self, img, **kw):
        self.inference_calls.append((img.size, kw))
        if kw['rank'] != 0:
            return None
        tag = tuple(int(v) for v in np.asarray(img)[0, 0])
        return {'Seg': ('Seg', tag), 'mod4-Marker': ('Marker', tag)}

    def compute_cell_results(self, seg, marker, resolution, version=3, offset=(0, 0)):
        self.cell_calls.append((seg, marker, resolution, version, offset))
        return _part([f'cell@{offset[0]},{offset[1]}'], 10 + len(self.cell_calls), 100, version)


def _reader(calls):
    def read_region(x, y, w, h):
        calls.append((x, y, w, h))
        a = np.zeros((h, w, 3), dtype=np.uint8)
        a[..., 0], a[..., 1] = x // 10, y // 10                          # the image names its region
        return a
    return read_region


def test_infer_slide_cells_regions_offsets_and_marker(monkeypatch):
    stubs = _Stubs(monkeypatch)
    reads, seen = [], []
    plan, parts = wsi.infer_slide_cells(_reader(reads), 450, 210, 128, '/m/Model', version=4, region_size=200, seg_weights=[1, 2, 3, 4, 5], batch_size=3,
                                        on_region=lambda xywh, data: seen.append((xywh, data['cells'])))
    grid = wsi.cell_region_grid(450, 210, 200)
    assert plan.regions == grid and plan.mode == 'regions' and len(grid) == 6
    assert reads == grid and [i for i, _ in parts] == list(range(6))
    assert seen == [(r, [f'cell@{r[0]},{r[1]}']) for r in grid]
    for (size, kw), r in zip(stubs.inference_calls, grid):
        assert size == (r[2], r[3])
        assert kw == dict(tile_size=128, overlap_size=8, model_path='/m/Model', eager_mode=False, color_dapi=False, color_marker=False, opt='opt of /m/Model',
                          return_seg_intermediate=False, seg_only=True, seg_weights=[1, 2, 3, 4, 5], nets=None, batch_size=3, rank=0, world=1)
    # versions 3 / 4: the Marker image of the SAME region; resolution from the tile size; the region's position as the offset
    for (seg, marker, resolution, version, offset), r in zip(stubs.cell_calls, grid):
        tag = (r[0] // 10, r[1] // 10, 0)
        assert (seg, marker, resolution, version, offset) == (('Seg', tag), ('Marker', tag), '10x', 4, (r[0], r[1]))
    merged = wsi.merge_cell_results([d for _, d in parts], 128, 200, [1, 2, 3, 4, 5], '/m/Model')
    assert merged['cells'] == [f'cell@{r[0]},{r[1]}' for r in grid] and merged['modelVersion'] == 'Model'
    assert merged['settings']['default_size_thresh'] == round(sum(range(11, 17)) / 6)


@pytest.mark.parametrize('tile_size,resolution', [(512, '40x'), (385, '40x'), (384, '20x'), (193, '20x'), (192, '10x')])
def test_infer_slide_cells_versions_5_and_6_take_the_region_itself(monkeypatch, tile_size, resolution):
    stubs = _Stubs(monkeypatch)
    wsi.infer_slide_cells(_reader([]), 300, 100, tile_size, '/m/Model', version=6, region_size=200)
    assert len(stubs.cell_calls) == 2
    for (seg, marker, res, version, offset), r in zip(stubs.cell_calls, wsi.cell_region_grid(300, 100, 200)):
        assert res == resolution and version == 6 and offset == (r[0], r[1])
        assert marker.size == (r[2], r[3]) and tuple(np.asarray(marker)[0, 0]) == (r[0] // 10, r[1] // 10, 0)


def test_infer_slide_cells_rank_assignment(monkeypatch):
    """regions go to ranks through plan_slide: whole regions (every region computed exactly once, by the rank the plan names), or bands"""
    grid = wsi.cell_region_grid(450, 210, 200)
    want = wsi.plan_slide(450, 210, 64, 4, 200, regions=grid)
    assert want.mode == 'regions' and sorted(j.index for jobs in want.jobs for j in jobs) == list(range(6))
    everything = []
    for rank in range(4):
        stubs, reads = _Stubs(monkeypatch), []
        plan, parts = wsi.infer_slide_cells(_reader(reads), 450, 210, 64, '/m/Model', version=3, region_size=200, rank=rank, world=4)
        assert plan.jobs == want.jobs
        assert reads == [j.xywh for j in want.jobs[rank]] and [i for i, _ in parts] == [j.index for j in want.jobs[rank]]
        assert all(kw['rank'] == 0 and kw['world'] == 1 for _, kw in stubs.inference_calls)
        everything += parts
    merged = wsi.merge_cell_results([d for _, d in sorted(everything, key=lambda p: p[0])], 64, 200)
    assert merged['cells'] == [f'cell@{r[0]},{r[1]}' for r in grid]
    # fewer regions than ranks: every rank infers its band of every region, rank 0 alone computes the cells
    for rank in range(3):
        stubs = _Stubs(monkeypatch)
        plan, parts = wsi.infer_slide_cells(_reader([]), 300, 100, 64, '/m/Model', version=3, region_size=200, rank=rank, world=3)
        assert plan.mode == 'bands' and [(kw['rank'], kw['world']) for _, kw in stubs.inference_calls] == [(rank, 3)] * 2
        assert [i for i, _ in parts] == ([0, 1] if rank == 0 else []) and len(stubs.cell_calls) == (2 if rank == 0 else 0)


def test_plan_slide_without_a_region_list_is_unchanged():
    a, b = wsi.plan_slide(45000, 21000, 512, 2), wsi.plan_slide(45000, 21000, 512, 2, regions=wsi.region_grid(45000, 21000))
    assert a.regions == b.regions == wsi.region_grid(45000, 21000) and a.jobs == b.jobs and a.tiles_per_rank == b.tiles_per_rank
