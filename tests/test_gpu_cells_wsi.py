"""wsi.infer_slide_cells + merge_cell_results end to end on the GPU: a small slide of two by two regions through the seam tests' small DeepLIIF
checkpoint directory, against the same regions put through inference() -> compute_cell_results(route='host') -> the reference's shift in
Python (models/__init__.py:883-903).  Equality.

The generators hold random weights, so their Seg image is gray noise without a single cell.  seg_weights = (4, 4, 4) -- the weights of the sum of
the three segmentation outputs are the caller's -- stretches that noise over the whole uint8 range, which makes dozens of small cells of
irregular shape per region: a better outline test than blobs.  The test insists on that (a slide without cells would compare nothing)."""
import numpy as np
import pytest
from PIL import Image

from deepliif_amd import postprocessing as PP
from deepliif_amd import wsi
from golden_util import synth_image
from seam_util import build_checkpoint_dir

pytestmark = pytest.mark.gpu
SIZE_X, SIZE_Y, REGION, TILE = 150, 130, 80, 64
SEG_WEIGHTS = [4, 4, 4]


@pytest.fixture(scope='module')
def slide(tmp_path_factory):
    from deepliif_amd import inference as I
    mdir = build_checkpoint_dir(tmp_path_factory.mktemp('cells_wsi'), 'dl_m2')
    I._NETS_CACHE.clear()
    opt = I.get_opt(mdir)
    opt.ngf, opt.precision, opt.gpu_ids = 8, 'fp32', [0]
    opt.modalities_names = ['IHC', 'Hema', 'Marker']                 # the second translation is the marker: inference(seg_only=True) returns it
    nets = I.init_nets(mdir, eager_mode=True, opt=opt)
    pixels = synth_image(SIZE_X, SIZE_Y, 41)
    grid = wsi.cell_region_grid(SIZE_X, SIZE_Y, REGION)
    assert grid == [(0, 0, 75, 65), (75, 0, 75, 65), (0, 65, 75, 65), (75, 65, 75, 65)]
    # the regions' images once, shared by the tests below
    inferred = []
    for x, y, w, h in grid:
        img = Image.fromarray(np.ascontiguousarray(pixels[y:y + h, x:x + w]))
        images = I.inference(img, TILE, TILE // 16, mdir, opt=opt, seg_only=True, seg_weights=SEG_WEIGHTS, nets=nets)
        assert list(images) == ['Seg', 'mod2-Marker']
        inferred.append((img, images))
    yield dict(mdir=mdir, opt=opt, nets=nets, read=lambda x, y, w, h: pixels[y:y + h, x:x + w], grid=grid, inferred=inferred)
    I._NETS_CACHE.clear()


def expected(slide, version):
    parts = []
    for (x, y, w, h), (img, images) in zip(slide['grid'], slide['inferred']):
        data = PP.compute_cell_results(images['Seg'], img if version >= 5 else images['mod2-Marker'], '10x', version=version, route='host')
        cells = []
        for c in data['cells']:
            if version in (4, 6):
                c = PP.encode_cell_data_v4(PP.shift_cell(PP.decode_cell_data_v4(c, v6=(version == 6)), (x, y)), v6=(version == 6))
            else:
                c = PP.shift_cell(c, (x, y))
            cells.append(c)
        parts.append({**data, 'cells': cells})
    return parts


@pytest.mark.parametrize('version', [3, 4, 6])
def test_slide_cells_equal_the_host_route_shifted_in_python(slide, version):
    want = expected(slide, version)
    assert min(len(p['cells']) for p in want) >= 8 and sum(len(p['cells']) for p in want) >= 60, [len(p['cells']) for p in want]
    seen = []
    plan, parts = wsi.infer_slide_cells(slide['read'], SIZE_X, SIZE_Y, TILE, slide['mdir'], version=version, region_size=REGION, seg_weights=SEG_WEIGHTS,
                                        nets=slide['nets'], opt=slide['opt'], on_region=lambda xywh, data: seen.append(xywh))
    assert plan.regions == slide['grid'] == seen and [i for i, _ in parts] == [0, 1, 2, 3]
    assert [d for _, d in parts] == want
    got = wsi.merge_cell_results([d for _, d in parts], TILE, REGION, SEG_WEIGHTS, slide['mdir'])
    assert got == wsi.merge_cell_results(want, TILE, REGION, SEG_WEIGHTS, slide['mdir'])
    assert got['cells'] == [c for p in want for c in p['cells']] and got['modelVersion'] == 'dl_m2' and got['dataVersion'] == version
    assert got['settings']['tile_size'] == TILE and got['settings']['region_size'] == REGION
    # cells of the lower right region lie in it
    cells = got['cells'][-len(want[3]['cells']):]
    boxes = [(PP.decode_cell_data_v4(c, v6=(version == 6)) if version != 3 else c)['bbox'] for c in cells]
    assert all(75 <= b[0][0] <= b[1][0] < 150 and 65 <= b[0][1] <= b[1][1] < 130 for b in boxes)


def test_two_ranks_compute_every_region_once(slide):
    want = expected(slide, 4)
    everything = []
    for rank in range(2):
        plan, parts = wsi.infer_slide_cells(slide['read'], SIZE_X, SIZE_Y, TILE, slide['mdir'], version=4, region_size=REGION, seg_weights=SEG_WEIGHTS,
                                            nets=slide['nets'], opt=slide['opt'], rank=rank, world=2)
        assert plan.mode == 'regions' and [i for i, _ in parts] == [j.index for j in plan.jobs[rank]] and len(parts) == 2
        everything += parts
    assert [d for _, d in sorted(everything, key=lambda p: p[0])] == want
