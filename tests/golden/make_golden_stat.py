"""Fixtures for the evaluation metrics: the REFERENCE's own DeepLIIF_Statistics/Segmentation_Metrics.py (compute_aji :64-102 and
compute_metrics_gpu :13-39) run in this container on small mask pairs.

  python tests/golden/make_golden_stat.py        ->  tests/golden/stat_cases.npz

The module is imported through _ref_import.install_stubs() (cv2, numba and skimage are not installed: numba.jit becomes the identity
decorator, so compute_metrics_gpu runs as the plain Python double loop it is written as).  ONE stand-in: the reference calls
skimage.measure.label(image, background=0); here that name is bound to `measure_label` below, which labels 8-connected regions of equal
value with scipy.ndimage.label and numbers them in raster order of their first pixel -- skimage's definition and numbering.  Everything else
(the per-component masks, the pairwise logical_and, the greedy pass, the six metrics, the TP == 0 rule) is the reference's code.

Stored per case: the two uint8 planes (gt, pred; raw values -- some cases carry several non-zero values for the labelling tests), and what the
reference returns for them after its own binarisation (plane[plane > 0] = 1, Segmentation_Metrics.py:123-133): the AJI float and the six
metrics (IOU, precision, recall, f1, Dice, pixAcc).  There is no SSIM fixture: skimage is not installed here (tests/stat_ref.py is that
yardstick)."""
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import install_stubs, REF_ROOT          # noqa: E402
from golden_util import save_npz                        # noqa: E402


def measure_label(image, background=0):
    """stand-in for skimage.measure.label(image, background=0): equal value, 8-connected, raster order of the first pixel"""
    image = np.asarray(image)
    raw = np.zeros(image.shape, dtype=np.int64)
    n_all = 0
    for v in np.unique(image):
        if v == background:
            continue
        lab, n = ndimage.label(image == v, structure=np.ones((3, 3), dtype=bool))
        raw[lab > 0] = lab[lab > 0] + n_all
        n_all += n
    ids, first = np.unique(raw.ravel(), return_index=True)
    order = [i for i in ids[np.argsort(first)] if i != 0]
    lut = np.zeros(n_all + 1, dtype=np.int64)
    for new, old in enumerate(order):
        lut[old] = new + 1
    return lut[raw]


def blobs(shape, seed, thresh):
    rng = np.random.RandomState(seed)
    f = ndimage.gaussian_filter(rng.rand(*shape), 2.0)
    return ((f > np.quantile(f, thresh)) * 255).astype(np.uint8)


def cases():
    Z = lambda h=64, w=64: np.zeros((h, w), dtype=np.uint8)
    out = []
    out.append(('empty_empty', Z(), Z()))
    g = blobs((64, 64), 1, 0.8)
    out.append(('pred_equals_gt', g, g.copy()))
    # no true positive: everything 0 (the other branch of the TP == 0 rule is empty_empty)
    out.append(('gt_empty', Z(), g.copy()))
    out.append(('pred_empty', g.copy(), Z()))
    # one gt component over two preds with EQUAL intersections (11 x 9 each): the pred with the smaller label takes it, and the second gt
    # component, which overlaps only that pred, then stays unmatched (with the other choice it would be matched: the tie rule shows in the sums)
    g, p = Z(), Z()
    g[10:21, 10:31] = 255
    g[24:31, 10:19] = 255
    p[10:31, 10:19] = 255
    p[10:21, 22:31] = 255
    out.append(('one_gt_two_preds_tie', g, p))
    # two gt components competing for one pred: the first in label order takes it although the second overlaps it more and then stays unmatched
    g, p = Z(), Z()
    g[5:16, 5:26] = 255
    g[20:31, 5:26] = 255
    p[13:25, 8:20] = 255
    out.append(('two_gts_one_pred', g, p))
    # predicted components that touch no gt component: total_U
    g, p = Z(), Z()
    g[10:20, 10:20] = 255
    p[12:22, 11:21] = 255
    p[40:45, 40:50] = 255
    p[55:60, 3:9] = 255
    out.append(('untouched_preds', g, p))
    # diagonal-only contact: one component under 8-connectivity
    g, p = Z(), Z()
    g[10:20, 10:20] = 255
    g[20:30, 20:30] = 255
    p[12:28, 12:28] = 255
    p[40:50, 40:45] = 255
    p[50:55, 45:50] = 255
    out.append(('diagonal_contact', g, p))
    # two adjacent regions of different non-zero value: two components for the labelling, one for the binarised masks
    g, p = Z(), Z()
    g[8:24, 8:20] = 100
    g[8:24, 20:32] = 200
    g[40:50, 10:30] = 150
    p[10:26, 10:34] = 200
    p[41:51, 12:20] = 60
    p[41:51, 20:30] = 61
    out.append(('adjacent_values', g, p))
    # values 1 .. 9 (zeroed before the IHC count) next to values >= 10
    g, p = Z(), Z()
    for k in range(1, 10):
        g[4:8, 6 * k:6 * k + 4] = k
    g[20:30, 20:30] = 10
    g[40:50, 10:20] = 255
    g[40:50, 20:24] = 9
    p[21:31, 19:29] = 11
    p[42:52, 12:22] = 5
    p[3:9, 3:9] = 9
    out.append(('low_values', g, p))
    # planes without any background pixel
    g, p = Z(), Z()
    g[:] = 200
    g[16:32, 16:32] = 100
    p[:] = 255
    out.append(('no_background', g, p))
    # many ragged components, the prediction a shifted copy
    g = blobs((64, 64), 2, 0.7)
    out.append(('ragged_shifted', g, np.roll(np.roll(g, 2, axis=0), -3, axis=1)))
    g = blobs((64, 64), 3, 0.6)
    out.append(('ragged_independent', g, blobs((64, 64), 4, 0.65)))
    # degenerate shapes; W = 65 cuts every row's runs at a wavefront boundary of the GPU labelling
    rng = np.random.RandomState(5)
    out.append(('w1', (rng.rand(64, 1) > 0.4).astype(np.uint8) * 255, (rng.rand(64, 1) > 0.4).astype(np.uint8) * 255))
    out.append(('h1', (rng.rand(1, 64) > 0.4).astype(np.uint8) * 255, (rng.rand(1, 64) > 0.4).astype(np.uint8) * 255))
    g, p = Z(40, 65), Z(40, 65)
    g[3:12, :] = 255
    g[20:30, 30:65] = 255
    g[32:38, 0:40] = 255
    p[5:14, 2:65] = 255
    p[22:36, 28:60] = 255
    out.append(('w65', g, p))
    return out


def main():
    install_stubs()
    sys.path.insert(0, os.path.join(REF_ROOT, 'DeepLIIF_Statistics'))
    import Segmentation_Metrics as SM
    SM.measure = types.SimpleNamespace(label=measure_label)          # the one stand-in (see the module docstring)
    out = {}
    names = []
    for name, gt, pred in cases():
        names.append(name)
        gb, pb = gt.copy(), pred.copy()
        gb[gb > 0] = 1
        pb[pb > 0] = 1
        out[f'{name}/gt'], out[f'{name}/pred'] = gt, pred
        out[f'{name}/aji'] = np.float64(SM.compute_aji(gb, pb))
        out[f'{name}/metrics'] = np.array([float(v) for v in SM.compute_metrics_gpu(pb, gb, gb.shape)], dtype=np.float64)
        print(name, float(out[f'{name}/aji']), out[f'{name}/metrics'])
    out['names'] = np.array(names)
    save_npz(os.path.join(HERE, 'stat_cases.npz'), out)


if __name__ == '__main__':
    main()
