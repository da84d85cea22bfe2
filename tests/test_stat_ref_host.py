"""tests/stat_ref.py, the float64 / integer yardstick of the evaluation metrics, against what the REFERENCE's own Segmentation_Metrics.py returns
(tests/golden/stat_cases.npz, made by tests/golden/make_golden_stat.py), and the derivation of the SSIM bound the GPU test uses.

There is no skimage-generated SSIM fixture (skimage is not installed where the fixtures are made): stat_ref IS the SSIM yardstick.  What holds
it in place here: two float64 evaluations in different summation orders agree far inside the bound, a float32 evaluation does not, and every
plausible misreading of the definition (radius, sigma, interior crop) moves the value by much more than the bound.

The bound, |a - b| <= 1e-9 for MSE and SSIM computed in double by two routes: each map value (a filtered mean, a variance) carries at most a
few tens of ulp (2.2e-16) of a quantity <= 1; S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) has a denominator of at least
C1 C2, and the factor that amplifies an absolute error of a variance is 1 / C2 = 1.1e3 at data_range = 1: about 5e-12 per pixel, which the mean
cannot exceed.  Single precision (ulp 6e-8) lands near 1e-6 by the same count."""
import os
import re

import numpy as np
import pytest

import stat_cases as SC
import stat_ref as R

BOUND = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ssim_pairs():
    return {'noise': SC.noise_pair(64, 48, 1), 'near_flat': SC.near_flat_pair(64, 48, 2), 'black_white': SC.black_white_pair(64, 48),
            'smooth': SC.smooth_pair(64, 48, 3)}


# ---------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize('name', SC.NAMES)
def test_aji_and_metrics_reproduce_the_reference_exactly(name):
    g, p = SC.planes(name)
    aji, ti, tu, tU = R.compute_aji(g, p)
    assert aji == float(SC.Z[f'{name}/aji'])
    assert isinstance(ti, int) and ti <= tu
    assert R.compute_aji_table(g, p) == (aji, ti, tu, tU)                     # the table route that the GPU test uses on images with hundreds of components
    got = R.metrics_from_counts(*R.confusion(p, g))
    assert [float(v) for v in got] == [float(v) for v in SC.Z[f'{name}/metrics']]


def test_the_fixture_holds_the_cases_it_is_meant_to():
    """each case shows what its name says, in numbers derived by hand"""
    g, p = SC.planes('one_gt_two_preds_tie')
    assert R.label(g)[1] == 2 and R.label(p)[1] == 2
    assert R.compute_aji(g, p)[1:] == (99, 21 * 11 + 21 * 9 - 99, 99)         # pred 1 goes to gt 1; gt 2 overlaps only pred 1 and adds nothing; U = pred 2
    g, p = SC.planes('two_gts_one_pred')
    assert R.compute_aji(g, p)[1:] == (3 * 12, 11 * 21 + 12 * 12 - 36, 0)     # the first gt takes the pred; the second adds nothing
    g, p = SC.planes('untouched_preds')
    assert R.compute_aji(g, p)[3] == 5 * 10 + 5 * 6
    g, p = SC.planes('diagonal_contact')
    assert R.label(g)[1] == 1 and R.label(g, connectivity=4)[1] == 2 and R.label(p)[1] == 2
    g, p = SC.planes('adjacent_values')
    assert R.label(g)[1] == 3 and R.label((g > 0).astype(np.uint8))[1] == 2 and R.label(p)[1] == 3
    lab, _ = R.label(g)
    assert lab[8, 8] == 1 and lab[8, 20] == 2 and lab[40, 10] == 3            # raster order of the first pixel
    assert float(SC.Z['empty_empty/aji']) == 0.0 and float(SC.Z['pred_equals_gt/aji']) == 1.0


# ---------------------------------------------------------------------------------------------------- the TP == 0 rule, labels minus one
def test_tp_zero_rule():
    assert R.metrics_from_counts(0, 0, 0, 100) == (1, 1, 1, 1, 1, 1)
    assert R.metrics_from_counts(0, 3, 0, 97) == (0, 0, 0, 0, 0, 0)
    assert R.metrics_from_counts(0, 0, 3, 97) == (0, 0, 0, 0, 0, 0)
    assert [float(v) for v in SC.Z['gt_empty/metrics']] == [0.0] * 6 and [float(v) for v in SC.Z['pred_empty/metrics']] == [0.0] * 6
    assert [float(v) for v in SC.Z['empty_empty/metrics']] == [1.0] * 6
    IOU, precision, recall, f1, Dice, pixAcc = R.metrics_from_counts(6, 2, 4, 88)
    assert (IOU, precision, recall, Dice, pixAcc) == (6 / 12, 6 / 8, 6 / 10, 12 / 18, 94 / 100)
    assert f1 == 2 * (6 / 8) * (6 / 10) / (6 / 8 + 6 / 10)


def test_cell_count_is_labels_minus_one():
    """len(np.unique(labels)) - 1: the component count, or one less when the plane has no background pixel"""
    g, p = SC.planes('no_background')
    assert R.label(g, 10)[1] == 2 and R.cell_count(g) == 1
    assert R.label(p, 10)[1] == 1 and R.cell_count(p) == 0
    g, p = SC.planes('low_values')
    assert R.label(g)[1] == 9 + 3 and R.cell_count(g) == 2                    # values 1 .. 9 are zeroed first; the 9-valued strip leaves the 255 block alone
    assert R.cell_count(p) == 1
    assert R.cell_count(np.zeros((8, 8), dtype=np.uint8)) == 0
    gt = np.zeros((64, 64, 3), dtype=np.uint8)
    gt[..., 0], gt[..., 2] = g, g.T
    assert R.ihc_score(gt) == 2 / 4
    assert R.ihc_score(np.zeros((8, 8, 3), dtype=np.uint8)) == 0


def test_segmentation_rows_keep_the_scripts_conventions():
    gts, preds = zip(*[SC.rgb_masks(n) for n in ('untouched_preds', 'two_gts_one_pred')])
    info, metrics = R.segmentation_metrics(gts, preds, model_name='M', names=['a_SegRefined.png', 'b_SegRefined.png'], aji=True)
    assert [r['cell_type'] for r in info] == ['Positive', 'Negative', 'Mean'] * 2
    assert list(info[0].keys()) == ['Model', 'image_name', 'cell_type', 'precision', 'recall', 'f1', 'Dice', 'IOU', 'PixAcc', 'AJI']
    six = [float(v) for v in SC.Z['untouched_preds/metrics']]                 # IOU, precision, recall, f1, Dice, pixAcc
    assert info[0]['precision'] == six[1] * 100 and info[0]['IOU'] == six[0] * 100 and info[0]['AJI'] == float(SC.Z['untouched_preds/aji']) * 100
    # metrics['precision'] is a mean of percents, metrics['precision_positive'] a mean of fractions
    assert metrics['precision_positive'] == (six[1] + float(SC.Z['two_gts_one_pred/metrics'][1])) / 2
    assert metrics['precision'] == (info[2]['precision'] + info[5]['precision']) / 2
    assert set(metrics) == {k + s for k in ('precision', 'recall', 'f1', 'Dice', 'IOU', 'PixAcc', 'AJI') for s in ('', '_positive', '_negative')}
    info2, metrics2 = R.segmentation_metrics(gts, preds)
    assert 'AJI' not in info2[0] and 'AJI' not in metrics2 and len(metrics2) == 18


# ---------------------------------------------------------------------------------------------------- the SSIM bound
def test_two_float64_orderings_agree_within_the_bound_and_float32_does_not():
    worst = 0.0
    for name, (a, b) in ssim_pairs().items():
        for dr in (1.0, 255.0):
            s1, s2 = R.ssim(a, b, dr), R.ssim(a, b, dr, order='direct')
            print(f'{name} data_range={dr}: separable {s1!r} direct {s2!r} diff {abs(s1 - s2):.3e}')
            worst = max(worst, abs(s1 - s2))
            assert abs(s1 - s2) <= BOUND
    assert worst <= 1e-12                                                     # (three orders inside the bound; 1.4e-13, on the near-flat pair, when this was written)
    a, b = ssim_pairs()['near_flat']
    d32 = abs(R.ssim(a, b, dtype=np.float32) - R.ssim(a, b))
    print(f'near_flat float32 against float64: {d32:.3e}')
    assert d32 > BOUND * 100                                                  # single precision is caught with two orders to spare


def test_ssim_known_values():
    a, b = ssim_pairs()['noise']
    assert R.ssim(a, a) == 1.0 and R.mse(a, a) == 0.0
    k, w = SC.black_white_pair(64, 48)
    assert R.mse(k, w) == pytest.approx(1.0, abs=1e-15)
    assert R.ssim(k, w) == pytest.approx(1e-4 / (1 + 1e-4), abs=1e-15)        # ux = 0, uy = 1, no variance: S = C1 / (1 + C1)
    assert R.gaussian_taps().shape == (11,) and abs(R.gaussian_taps().sum() - 1) < 1e-15
    assert R.gray(np.full((2, 2, 3), 255, dtype=np.uint8))[0, 0] == pytest.approx(1.0, abs=1e-15)
    with pytest.raises(ValueError):
        R.ssim(np.zeros((10, 64), dtype=np.uint8), np.zeros((10, 64), dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------- mutations
@pytest.mark.parametrize('mutation', [dict(radius=4), dict(sigma=1.0), dict(crop=False)], ids=['radius4', 'sigma1', 'nocrop'])
def test_a_misread_ssim_definition_misses_the_bound(mutation):
    moved = [name for name, (a, b) in ssim_pairs().items() if abs(R.ssim(a, b, **mutation) - R.ssim(a, b)) > BOUND]
    assert moved, f'{mutation} changes no SSIM case by more than {BOUND}'


@pytest.mark.parametrize('mutation', [dict(connectivity=4), dict(tie='large'), dict(unmatched_union=True), dict(ge=True)],
                         ids=['conn4', 'tie_large', 'unmatched_union', 'ge'])
def test_a_misread_aji_definition_misses_a_golden(mutation):
    broken = [n for n in SC.NAMES if R.compute_aji(*SC.planes(n), **mutation)[0] != float(SC.Z[f'{n}/aji'])]
    assert broken, f'{mutation} reproduces every golden AJI'


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_stat_symbols_are_declared_bound_and_exported():
    """(tests/test_cabi_exports.py checks every declared symbol; this names the ones this module needs)"""
    from deepliif_amd import _lib as L
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'deepliif_hip.h')).read(), flags=re.S)
    lib = L.load()
    for n in ('dl_stat_similarity_ws_bytes', 'dl_stat_similarity', 'dl_stat_confusion', 'dl_stat_label_ws_bytes', 'dl_stat_label', 'dl_stat_aji_ws_bytes',
              'dl_stat_aji'):
        assert re.search(r'\b%s\s*\(' % n, header) and n in L.SIGNATURES and hasattr(lib, n)
    # decided on the host, before any launch (the pointers are never dereferenced)
    import ctypes as C
    d = C.c_void_p(0x1000)
    assert lib.dl_stat_similarity(d, 30, 300, d, 30, 300, 3, 1, 10, 10, 1.0, d, d, None) != 0 and b'H, W >= 11' in lib.dl_last_error()
    assert lib.dl_stat_similarity_ws_bytes(1, 0, 16) == 0 and lib.dl_stat_similarity_ws_bytes(3, 97, 130) >= 3 * 7 * 5 * 16
    assert lib.dl_stat_confusion(d, 30, 300, d, 30, 300, 0, 10, 10, d, None) != 0 and b'empty problem' in lib.dl_last_error()
