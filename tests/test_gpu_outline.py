"""The cell-outline kernels (dl_pp_outline_count / dl_pp_outline_emit behind postprocessing.outline_cells and compute_cell_results(route='gpu'))
against the reference's stored results (tests/golden/post_cases.npz) and the host route (get_cell_boundary -> make_simple_contour ->
encode_cell_data_v4).  Integer and byte work: every comparison is equality.  The CPU twin of the kernels' code is test_outline_host.py."""
import os

import numpy as np
import pytest
import torch

import outline_cases as OC
from deepliif_amd import ops
from deepliif_amd import postprocessing as PP
from golden_util import load_npz, synth_cells

pytestmark = pytest.mark.gpu
Z = load_npz(os.path.join(os.path.dirname(__file__), 'golden', 'post_cases.npz'))
NAMES = [str(n) for n in Z['names']]
MASKS = OC.hand_masks()


@pytest.fixture(autouse=True)
def _real_backend():
    ops._impl = None
    yield


def host(mask, cells, version, offset):
    return PP.cell_results_from_mapping(mask, cells, {'size_thresh': 0}, version, 120, 4, None, offset=offset)['cells']


@pytest.mark.parametrize('version', [3, 4, 5, 6])
@pytest.mark.parametrize('name', NAMES)
def test_gpu_route_equals_the_reference_and_the_host_route(name, version):
    kw = eval(str(Z[f'{name}/kwargs']))
    ckw = {k: kw[k] for k in ('seg_thresh', 'noise_thresh', 'large_noise_thresh') if k in kw}
    args = (Z[f'{name}/seg'], Z[f'{name}/orig'] if version >= 5 else Z[f'{name}/marker'], kw['resolution'])
    got = PP.compute_cell_results(*args, version=version, route='gpu', **ckw)
    assert got == eval(str(Z[f'{name}/cell_results_v{version}']))
    assert got == PP.compute_cell_results(*args, version=version, route='host', **ckw)
    assert got == PP.compute_cell_results(*args, version=version, **ckw)          # the default is the GPU route


@pytest.mark.parametrize('offset', OC.OFFSETS)
@pytest.mark.parametrize('name', list(MASKS))
def test_hand_made_masks_straight_through_the_kernels(name, offset):
    mask = MASKS[name]
    cells = [OC.single_cell(mask, positive=(len(name) % 2 == 0), value=len(name) * 9)]
    mask_d = torch.from_numpy(mask).cuda()
    for version in (3, 4, 5, 6):
        assert PP.outline_cells(mask_d, cells, version, offset) == host(mask, cells, version, offset), version


@pytest.mark.parametrize('offset', OC.OFFSETS)
@pytest.mark.parametrize('name,kw', [
    ('single_pixel', dict(noise_thresh=0)),
    ('square_100', dict(large_noise_thresh=None)),
    ('starts_at_x_95', {}),
    ('image_1x37', {}),
    ('image_1x37_full', {}),
    ('image_61x1', {}),
    ('touches_four_borders', {}),
    ('bar_45x3', {}),
])
def test_hand_made_images_through_compute_cell_results(name, kw, offset):
    """the same shapes as segmentation images: cell mapping and outlines on the GPU, against the host route on a host copy of the mask"""
    mask = MASKS[name]
    seg = OC.seg_from_mask(mask)
    marker = np.full(mask.shape + (3,), 60, dtype=np.uint8)
    for version in (3, 4, 5, 6):
        got = PP.compute_cell_results(seg, marker, '40x', version=version, route='gpu', offset=offset, **kw)
        assert len(got['cells']) == 1
        assert got == PP.compute_cell_results(seg, marker, '40x', version=version, route='host', offset=offset, **kw)
        if version == 4:
            assert PP.decode_cell_data_v4(got['cells'][0])['size'] == int((mask != 0).sum())


@pytest.fixture(scope='module')
def many_cells():
    """777 x 1000 with 900 blobs: more than one workgroup, a cell count that is no multiple of 64; host results computed once"""
    orig, seg, marker = synth_cells(777, 1000, 900, 12)
    cm = PP.get_cells_info(seg, marker, '40x', PP.DEFAULT_NOISE_THRESH, PP.DEFAULT_SEG_THRESH, None)
    mask = cm.mask.cpu().numpy()
    return cm, mask, {(v, off): host(mask, cm.cells, v, off) for v in (3, 4) for off in ((0, 0), (8463, 8464))}


@pytest.mark.parametrize('offset', [(0, 0), (8463, 8464)])
@pytest.mark.parametrize('version', [3, 4])
def test_many_cells(many_cells, version, offset):
    cm, mask, want = many_cells
    assert len(cm.cells) > 128 and len(cm.cells) % 64 != 0
    assert np.array_equal(cm.table, PP.outline_table(cm.cells))
    assert PP.outline_cells(cm.mask, cm.table, version, offset) == want[(version, offset)]


def test_the_fp16_build_has_the_same_kernels(many_cells):
    from deepliif_amd import _lib as L
    cm, mask, want = many_cells
    assert PP.outline_cells(cm.mask, cm.table, 4, (8463, 8464), lib=L.load('fp16')) == want[(4, (8463, 8464))]


def test_the_gpu_route_keeps_the_mask_on_the_device(monkeypatch):
    orig, seg, marker = synth_cells(120, 150, 28, 1)
    copied = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (copied.append((tuple(self.shape), self.dtype)), real(self, *a, **k))[1])
    PP.compute_cell_results(seg, marker, '40x', version=4, route='gpu')
    assert copied and ((120, 150), torch.uint8) not in copied
    copied.clear()
    PP.compute_cell_results(seg, marker, '40x', version=4, route='host')
    assert ((120, 150), torch.uint8) in copied


def test_a_bad_first_pixel_raises_with_the_status():
    """a first pixel on background, outside the image, and a size too small for the outline are reported per cell by the count pass and raised
    by the host; nothing outside the image is read, and the next call works"""
    mask = MASKS['square_100']
    mask_d = torch.from_numpy(mask).cuda()
    good = OC.single_cell(mask)
    for bad, status in (((9, True, 1, 0, 0, 0, 0), 2), ((9, True, 1, mask.shape[1], 3, 0, 0), 1), ((9, True, 1, 5, -1, 0, 0), 1),
                        ((9, True, 1, 2 ** 31 - 1, -2 ** 31, 0, 0), 1), ((40, True, 1) + good[3:], 3)):
        for version in (3, 4):
            with pytest.raises(RuntimeError, match=f'status {status} for cell 1 '):
                PP.outline_cells(mask_d, [good, bad, good], version)
    assert PP.outline_cells(mask_d, [good], 4) == host(mask, [good], 4, (0, 0))
    assert PP.outline_cells(mask_d, [], 4) == []
    with pytest.raises(ValueError):
        PP.outline_cells(torch.from_numpy(mask), [good], 4)           # a host mask is refused, not copied
