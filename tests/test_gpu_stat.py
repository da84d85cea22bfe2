"""Model evaluation on the GPU (deepliif_amd/stat.py -> csrc/stat.hip: dl_stat_similarity, dl_stat_confusion, dl_stat_label, dl_stat_aji) against
tests/stat_ref.py and, for AJI and the six segmentation metrics, against what the reference's own Segmentation_Metrics.py returned
(tests/golden/stat_cases.npz).

MSE and SSIM: |gpu - stat_ref| <= 1e-9, a bound derived in tests/test_stat_ref_host.py (both sides work in double; the amplification through
1 / C2 leaves about 5e-12 per pixel), not measured.  There is NO skimage-generated SSIM fixture -- skimage is not installed where the fixtures are
made -- so stat_ref, held in place by that host test, is the SSIM yardstick.  Everything else here is integers, or fractions of integers computed
by the same Python expressions: compared by equality."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import stat_cases as SC
import stat_ref as R
from deepliif_amd import ops
from deepliif_amd import stat as S
from golden_util import load_npz, synth_cells

pytestmark = pytest.mark.gpu
BOUND = 1e-9
SQUARE = [n for n in SC.NAMES if SC.planes(n)[0].shape == (64, 64)]


@pytest.fixture(autouse=True)
def _real_backend():
    ops._impl = None
    yield


def check_similarity(gt, pred, data_range=1.0):
    got = S.image_similarity(gt, pred, data_range)
    gl = [np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in (gt if isinstance(gt, list) else [gt])]
    pl = [np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in (pred if isinstance(pred, list) else [pred])]
    want = R.image_similarity(gl, pl, data_range)
    assert got['mse'].shape == got['ssim'].shape == (len(gl),) and got['mse'].dtype == np.float64
    for k in ('mse', 'ssim'):
        err = np.abs(got[k] - want[k])
        print(f'{k}: gpu {got[k]} ref {want[k]} |diff| {err}')
        assert np.all(err <= BOUND), (k, got[k], want[k])
    return got


# ---------------------------------------------------------------------------------------------------- MSE / SSIM
@pytest.mark.parametrize('data_range', [1.0, 255.0])
@pytest.mark.parametrize('channels', [3, 1], ids=['rgb', 'gray'])
@pytest.mark.parametrize('shape', [(11, 11), (12, 75), (64, 48), (97, 130)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_similarity_against_stat_ref(shape, channels, data_range):
    h, w = shape
    check_similarity(*SC.noise_pair(h, w, 1, channels), data_range)
    check_similarity(*SC.near_flat_pair(h, w, 2, channels), data_range)


def test_similarity_512_and_a_batch_of_three():
    check_similarity(*SC.smooth_pair(512, 512, 4))
    pairs = [SC.noise_pair(64, 48, 5), SC.near_flat_pair(64, 48, 6), SC.smooth_pair(64, 48, 7)]
    got = check_similarity([p[0] for p in pairs], [p[1] for p in pairs])
    assert len(set(got['ssim'].tolist())) == 3
    one = S.image_similarity(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))          # the same as one [N, H, W, 3] array
    assert np.array_equal(one['ssim'], got['ssim']) and np.array_equal(one['mse'], got['mse'])


def test_similarity_extremes_are_exact():
    a, _ = SC.noise_pair(97, 130, 8)
    got = S.image_similarity(a, a.copy())
    assert got['mse'][0] == 0.0 and got['ssim'][0] == 1.0                     # exactly
    g, _ = SC.noise_pair(64, 48, 9, channels=1)
    got = S.image_similarity(g, g.copy(), data_range=255)
    assert got['mse'][0] == 0.0 and got['ssim'][0] == 1.0
    got = check_similarity(*SC.black_white_pair(64, 48))
    assert abs(got['mse'][0] - 1.0) <= BOUND and abs(got['ssim'][0] - 1e-4 / (1 + 1e-4)) <= BOUND


def test_similarity_of_a_strided_panel_needs_no_copy():
    """panel 2 of a 64 x 320 training row: a view with the row's stride"""
    rng = np.random.RandomState(10)
    row = rng.randint(0, 256, size=(64, 320, 3)).astype(np.uint8)
    other = np.clip(row.astype(np.int64) + rng.randint(-30, 31, size=row.shape), 0, 255).astype(np.uint8)
    rt, ot = torch.from_numpy(row).cuda(), torch.from_numpy(other).cuda()
    a, b = rt[:, 128:192], ot[:, 128:192]
    assert not a.is_contiguous() and S._batch(a, a.device).data_ptr() == a.data_ptr()
    got = S.image_similarity(a, b)
    want = R.image_similarity([row[:, 128:192]], [other[:, 128:192]])
    assert abs(got['mse'][0] - want['mse'][0]) <= BOUND and abs(got['ssim'][0] - want['ssim'][0]) <= BOUND
    # a PIL image and a tensor of the same pixels
    from PIL import Image
    got2 = S.image_similarity(Image.fromarray(row[:, 128:192]), b)
    assert got2['ssim'][0] == got['ssim'][0] and got2['mse'][0] == got['mse'][0]


def test_similarity_is_bit_identical_across_runs_and_rejects_small_or_unequal_images():
    a, b = SC.smooth_pair(97, 130, 11)
    r1, r2 = S.image_similarity([a] * 3, [b] * 3), S.image_similarity([a] * 3, [b] * 3)
    assert r1['ssim'].tobytes() == r2['ssim'].tobytes() and r1['mse'].tobytes() == r2['mse'].tobytes()
    assert r1['ssim'][0] == r1['ssim'][1] == r1['ssim'][2]
    with pytest.raises(ValueError, match='>= 11'):
        S.image_similarity(np.zeros((10, 64, 3), dtype=np.uint8), np.zeros((10, 64, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match='resize'):
        S.image_similarity(np.zeros((16, 64, 3), dtype=np.uint8), np.zeros((16, 32, 3), dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------- labelling, AJI, confusion, IHC
def check_labels(plane, min_value, binarize=False):
    c = S.label_components(plane, min_value=min_value, binarize=binarize)
    src = (plane > 0).astype(np.uint8) if binarize else plane
    lab, n = R.label(src, min_value)
    info = c.info.cpu().numpy()
    assert int(info[0]) == n and int(info[1]) == int(np.count_nonzero(lab))
    assert np.array_equal(c.labels.cpu().numpy(), lab)
    assert np.array_equal(c.sizes[:n].cpu().numpy(), R.component_sizes(lab, n))


@pytest.mark.parametrize('name', SC.NAMES)
def test_labels_and_aji_against_the_reference_fixture(name):
    g, p = SC.planes(name)
    for plane in (g, p):
        check_labels(plane, 0)
        check_labels(plane, 10)
        check_labels(plane, 0, binarize=True)
    got = S.aji(g, p)
    assert got == R.compute_aji(g, p)
    assert got[0] == float(SC.Z[f'{name}/aji'])                               # the reference's own compute_aji
    assert S.aji(g, p) == got
    # the reference's compute_metrics_gpu, through the confusion counts
    gt, pred = SC.rgb_masks(name)
    info, _ = S.segmentation_metrics(gt, pred)
    six = [float(v) for v in SC.Z[f'{name}/metrics']]                         # IOU, precision, recall, f1, Dice, pixAcc
    assert [info[0][k] for k in ('IOU', 'precision', 'recall', 'f1', 'Dice', 'PixAcc')] == [v * 100 for v in six]
    assert S._confusion(*S._pair(gt, pred))[0].tolist() == [list(R.confusion(pred[..., c], gt[..., c])) for c in (0, 2)]


def test_segmentation_metrics_and_ihc_of_a_batch():
    gts, preds = (list(x) for x in zip(*[SC.rgb_masks(n) for n in SQUARE]))
    names = [n + '_SegRefined.png' for n in SQUARE]
    for with_aji in (False, True):
        info, metrics = S.segmentation_metrics(gts, preds, model_name='M', names=names, aji=with_aji)
        winfo, wmetrics = R.segmentation_metrics(gts, preds, model_name='M', names=names, aji=with_aji)
        assert info == winfo and [list(r.keys()) for r in info] == [list(r.keys()) for r in winfo]
        assert dict(metrics) == dict(wmetrics)
    assert metrics['precision'] > 1 > metrics['precision_positive'] > 0       # percent against fraction: the script's convention
    got, want = S.ihc_score_diff(gts, preds), R.ihc_score_diff(gts, preds)
    assert np.array_equal(got['diff'], want['diff']) and got['mean'] == want['mean'] and got['diff'].max() > 0
    # labels minus one: the planes of no_background have 2 and 1 components and no background pixel
    i = SQUARE.index('no_background')
    assert S._cell_counts(S._batch(gts[i], torch.device('cuda')))[0].tolist() == [1, 1]
    assert S._cell_counts(S._batch(preds[i], torch.device('cuda')))[0].tolist() == [0, 0]
    with pytest.raises(ValueError, match='resize'):
        S.segmentation_metrics(gts[0], np.zeros((32, 64, 3), dtype=np.uint8))


@pytest.fixture(scope='module')
def synth_masks():
    """golden_util.synth_cells' seg image thresholded into a red / blue mask pair (raw values kept above the threshold, so the IHC count sees
    many values); the prediction is a shifted copy"""
    out = []
    for seed in (1, 2):
        _, seg, _ = synth_cells(256, 256, 100, seed)
        gt = np.zeros_like(seg)
        gt[..., 0] = np.where(seg[..., 0] > 120, seg[..., 0], 0)
        gt[..., 2] = np.where(seg[..., 2] > 120, seg[..., 2], 0)
        out.append((gt, np.roll(np.roll(gt, 3, axis=0), -2, axis=1)))
    return out


def test_synthetic_cells_256(synth_masks):
    gts, preds = [m[0] for m in synth_masks], [m[1] for m in synth_masks]
    # channel 2 has some 50 components: the reference's slow way; channel 0 (with the speckle, some 600) would take it minutes: the table route
    assert 20 < R.label((gts[0][..., 2] > 0).astype(np.uint8))[1] < 100 and R.label((gts[0][..., 0] > 0).astype(np.uint8))[1] > 300
    assert S.aji(gts[0][..., 2].copy(), preds[0][..., 2].copy()) == R.compute_aji(gts[0][..., 2], preds[0][..., 2])
    assert S.aji(gts[0][..., 0].copy(), preds[0][..., 0].copy()) == R.compute_aji_table(gts[0][..., 0], preds[0][..., 0])
    for c in (0, 2):
        check_labels(np.ascontiguousarray(gts[0][..., c]), 10)
    info, metrics = S.segmentation_metrics(gts, preds, aji=True)
    winfo, wmetrics = R.segmentation_metrics(gts, preds, aji=True, aji_fn=R.compute_aji_table)
    assert info == winfo and dict(metrics) == dict(wmetrics) and 0 < metrics['AJI'] < 100
    got, want = S.ihc_score_diff(gts, preds), R.ihc_score_diff(gts, preds)
    assert np.array_equal(got['diff'], want['diff']) and got['mean'] == want['mean']


# ---------------------------------------------------------------------------------------------------- the directory driver
def read_csv(path):
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_compute_statistics_on_a_directory(tmp_path):
    from PIL import Image
    gt_dir, model_dir, out_dir = tmp_path / 'gt', tmp_path / 'model', tmp_path / 'out'
    gt_dir.mkdir()
    model_dir.mkdir()
    cases = ['untouched_preds', 'two_gts_one_pred', 'low_values', 'w65']       # (w65 has another size: a batch of its own)
    gts, preds, names = [], [], []
    for n in cases:
        g, p = SC.rgb_masks(n)
        Image.fromarray(g).save(gt_dir / f'{n}.png')
        Image.fromarray(p).save(model_dir / f'{n}_SegRefined.png')
        gts.append(g)
        preds.append(p)
        names.append(f'{n}_SegRefined.png')
    mods = {}
    for i, kind in enumerate(('Hema', 'DAPI')):
        for j in range(2):
            a, b = SC.smooth_pair(48, 64, 20 + 2 * i + j)
            Image.fromarray(a).save(gt_dir / f'img{j}_{kind}.png')
            Image.fromarray(b).save(model_dir / f'img{j}_{kind}.png')
            mods.setdefault(kind, []).append((a, b))
    order = np.argsort(names)
    all_info = S.compute_statistics(str(gt_dir), str(model_dir), str(out_dir), model_name='DeepLIIF', mode='All', image_types=('Hema', 'DAPI'), aji=True)
    assert sorted(os.listdir(out_dir)) == ['IHC_Scoring_info_All_DeepLIIF.csv', 'metrics_All_DeepLIIF.csv', 'segmentation_info_All_DeepLIIF_100_50.csv']
    # segmentation rows: per image (sorted listing), values of stat_ref
    want_rows = []
    for i in order:
        want_rows += R.segmentation_metrics([gts[i]], [preds[i]], 'DeepLIIF', [names[i]], aji=True)[0]
    head, rows = read_csv(out_dir / 'segmentation_info_All_DeepLIIF_100_50.csv')
    assert head == ['Model', 'image_name', 'cell_type', 'precision', 'recall', 'f1', 'Dice', 'IOU', 'PixAcc', 'AJI']
    assert len(rows) == 3 * len(cases)
    for row, want in zip(rows, want_rows):
        assert row[:3] == [want['Model'], want['image_name'], want['cell_type']]
        assert [float(v) for v in row[3:]] == [float(want[k]) for k in head[3:]]
    head, rows = read_csv(out_dir / 'IHC_Scoring_info_All_DeepLIIF.csv')
    assert head == ['Model', 'Sample', 'Diff_IHC_Score'] and [r[1] for r in rows] == sorted(f'{n}.png' for n in cases)
    assert [float(r[2]) for r in rows] == [float(R.ihc_score_diff([gts[i]], [preds[i]])['diff'][0]) for i in order]
    head, rows = read_csv(out_dir / 'metrics_All_DeepLIIF.csv')
    sim = [f'{k}_{s}' for k in ('Hema', 'DAPI') for s in ('MSE_avg', 'MSE_std', 'ssim_avg', 'ssim_std')]
    seg = [k + s for k in ('precision', 'recall', 'f1', 'Dice', 'IOU', 'PixAcc', 'AJI') for s in ('', '_positive', '_negative')]
    assert head == ['Model'] + sim + seg and len(rows) == 1 and rows[0][0] == 'DeepLIIF'
    got = dict(zip(head[1:], (float(v) for v in rows[0][1:])))
    for kind in ('Hema', 'DAPI'):
        w = R.image_similarity([m[0] for m in mods[kind]], [m[1] for m in mods[kind]])
        assert abs(got[f'{kind}_MSE_avg'] - np.mean(w['mse'])) <= BOUND and abs(got[f'{kind}_ssim_avg'] - np.mean(w['ssim'])) <= BOUND
        assert abs(got[f'{kind}_MSE_std'] - np.std(w['mse'])) <= BOUND and abs(got[f'{kind}_ssim_std'] - np.std(w['ssim'])) <= BOUND
    sums = {}
    for i in order:
        for k, v in R.segmentation_metrics([gts[i]], [preds[i]], aji=True)[1].items():
            sums[k] = sums.get(k, 0.0) + v
    assert {k: got[k] for k in seg} == {k: sums[k] / len(cases) for k in seg}
    assert all_info['precision'] == got['precision'] and all_info['Model'] == 'DeepLIIF'
    # the other modes, and what is left out
    S.compute_statistics(str(gt_dir), str(model_dir), str(tmp_path / 'seg'), model_name='X-DeepLIIF', mode='Segmentation')
    assert sorted(os.listdir(tmp_path / 'seg')) == ['IHC_Scoring_info_Segmentation_X-DeepLIIF.csv', 'segmentation_info_Segmentation_X-DeepLIIF_100_50.csv']
    assert read_csv(tmp_path / 'seg' / 'segmentation_info_Segmentation_X-DeepLIIF_100_50.csv')[0][-1] == 'PixAcc'
    S.compute_statistics(str(gt_dir), str(model_dir), str(tmp_path / 'syn'), mode='ImageSynthesis', image_types=('Hema',))
    assert os.listdir(tmp_path / 'syn') == ['metrics_ImageSynthesis_DeepLIIF.csv']
    with pytest.raises(NotImplementedError):
        S.compute_statistics(str(gt_dir), str(model_dir), str(out_dir), raw_segmentation=True)
    Image.fromarray(np.zeros((32, 32, 3), dtype=np.uint8)).save(model_dir / 'low_values_SegRefined.png')
    with pytest.raises(ValueError, match='resize'):
        S.compute_statistics(str(gt_dir), str(model_dir), str(out_dir), mode='Segmentation')


# ---------------------------------------------------------------------------------------------------- metrics.json for --with-val
def test_get_cell_count_metrics_equals_postprocess(tmp_path):
    from PIL import Image
    from deepliif_amd import inference as I
    P = load_npz(os.path.join(os.path.dirname(__file__), 'golden', 'post_cases.npz'))
    samples = [str(n) for n in P['names'] if str(n).startswith('sample_')]
    assert samples
    want = {}
    for use_marker in (False, True):
        d = tmp_path / f'rows_{int(use_marker)}'
        d.mkdir()
        for n in samples:
            orig, seg, marker = P[f'{n}/orig'], P[f'{n}/seg'], P[f'{n}/marker']
            Image.fromarray(np.concatenate([orig, orig[::-1].copy(), marker, seg], axis=1)).save(d / f'{n}.png')
            images = {'Seg': Image.fromarray(seg)}
            if use_marker:
                images['Marker'] = Image.fromarray(marker)
            want[n] = I.postprocess(Image.fromarray(orig), images, orig.shape[0], 'DeepLIIF')[1]
        got = S.get_cell_count_metrics(str(d), tile_size=P[f'{samples[0]}/orig'].shape[0], use_marker=use_marker, save_individual=True)
        assert got == want
        on_disk = json.load(open(d / 'metrics.json'))
        assert on_disk == json.loads(json.dumps(want)) and list(on_disk.keys()) == sorted(samples)
        assert set(on_disk[samples[0]]) >= {'num_total', 'num_pos', 'num_neg', 'percent_pos'}
        assert json.load(open(d / f'{samples[0]}.json')) == on_disk[samples[0]]
