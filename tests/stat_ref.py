"""Float64 / integer restatement of the evaluation metrics (deepliif_amd/stat.py, csrc/stat.hip): the yardstick of tests/test_gpu_stat.py.

numpy + scipy.ndimage only.  What it restates, and from where:
  * gray, mse, ssim: skimage's rgb2gray after img_as_float, mean_squared_error and structural_similarity(gaussian_weights=True, sigma=1.5,
    use_sample_covariance=False, data_range=R) as DeepLIIF_Statistics/ComputeStatistics.py:72-92 calls them -- the 2-D definition (the
    script's multichannel=True on a 2-D image is not reproduced).  skimage is not installed where these tests run, so there is NO fixture of
    SSIM values produced by skimage itself: this module is the SSIM yardstick.
  * label: skimage.measure.label(plane, background=0), 8-connected components of equal value numbered in raster order of their first pixel.
  * confusion, metrics_from_counts, segmentation_metrics: Segmentation_Metrics.py compute_metrics_gpu :13-39 and compute_segmentation_metrics
    :105-232 (with the AJI rows it has commented out, on request).
  * compute_aji: Segmentation_Metrics.py:64-102 the reference's slow way -- one full-size mask per component, logical_and of every pair, the
    greedy choice in label order.  tests/golden/stat_cases.npz holds what the reference's own function returns for the same masks.
  * cell_count, ihc_score, ihc_score_diff: ComputeStatistics.py compute_IHC_scoring :150-182.

The keyword arguments that no caller of the product needs (radius, sigma, crop, connectivity, tie, unmatched_union, ge) exist for the mutation
tests of tests/test_stat_ref_host.py: each wrong setting must fail a golden or an SSIM case.
"""
import collections

import numpy as np
from scipy import ndimage

SIGMA = 1.5
TRUNCATE = 3.5


# ---------------------------------------------------------------------------------------------------- MSE / SSIM
def gray(img, dtype=np.float64):
    """uint8 H x W (v / 255) or H x W x 3 (rgb2gray of img_as_float) -> float image"""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    f = img.astype(dtype) / dtype(255.0)
    if f.ndim == 2:
        return f
    return (dtype(0.2125) * f[..., 0] + dtype(0.7154) * f[..., 1]) + dtype(0.0721) * f[..., 2]


def gaussian_taps(sigma=SIGMA, radius=None, dtype=np.float64):
    """scipy.ndimage's _gaussian_kernel1d: radius int(truncate * sigma + 0.5) = 5 at sigma 1.5, normalised"""
    if radius is None:
        radius = int(TRUNCATE * sigma + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return (w / w.sum()).astype(dtype)


def mse(a, b):
    d = gray(a) - gray(b)
    return float(np.mean(d * d))


def _filter_separable(img, w):
    """gaussian_filter's order: axis 0, then axis 1 (the border mode never reaches the interior)"""
    return ndimage.correlate1d(ndimage.correlate1d(img, w, axis=0, mode='nearest'), w, axis=1, mode='nearest')


def _filter_direct(img, w):
    """the same filter as ONE 2-D window sum over the valid region, embedded in a full-size array: another summation order"""
    r = len(w) // 2
    win = np.lib.stride_tricks.sliding_window_view(img, (len(w), len(w)))
    k2 = np.outer(w, w).astype(img.dtype)
    out = np.zeros_like(img)
    acc = np.zeros(win.shape[:2], dtype=img.dtype)
    for i in range(len(w) - 1, -1, -1):           # (bottom-right tap first)
        for j in range(len(w) - 1, -1, -1):
            acc = acc + k2[i, j] * win[:, :, i, j]
    out[r:img.shape[0] - r, r:img.shape[1] - r] = acc
    return out


def ssim(a, b, data_range=1.0, sigma=SIGMA, radius=None, crop=True, dtype=np.float64, order='separable'):
    """structural_similarity(gaussian_weights=True, sigma, use_sample_covariance=False, data_range) of two uint8 images (gray or RGB)"""
    x, y = gray(a, dtype), gray(b, dtype)
    w = gaussian_taps(sigma, radius, dtype)
    r = len(w) // 2
    if min(x.shape) < 2 * r + 1:
        raise ValueError(f'the {2 * r + 1} x {2 * r + 1} Gaussian window needs H, W >= {2 * r + 1}, got {x.shape}')
    filt = _filter_separable if order == 'separable' else _filter_direct
    ux, uy, uxx, uyy, uxy = filt(x, w), filt(y, w), filt(x * x, w), filt(y * y, w), filt(x * y, w)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    C1, C2 = dtype((0.01 * data_range) ** 2), dtype((0.03 * data_range) ** 2)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    if crop or order != 'separable':
        S = S[r:S.shape[0] - r, r:S.shape[1] - r]
    return float(np.mean(S, dtype=dtype))


def image_similarity(gt, pred, data_range=1.0):
    """lists of uint8 images -> {'mse': [N], 'ssim': [N]}"""
    return {'mse': np.array([mse(a, b) for a, b in zip(gt, pred)]),
            'ssim': np.array([ssim(a, b, data_range) for a, b in zip(gt, pred)])}


# ---------------------------------------------------------------------------------------------------- labelling
_EIGHT = np.ones((3, 3), dtype=bool)
_FOUR = ndimage.generate_binary_structure(2, 1)


def label(plane, min_value=0, connectivity=8):
    """skimage.measure.label(plane, background=0) after values < min_value are zeroed -> (label image int32, number of components)"""
    plane = np.asarray(plane).copy()
    assert plane.ndim == 2
    plane[plane < min_value] = 0
    comps = []                      # (first pixel index, boolean mask)
    flat = np.arange(plane.size).reshape(plane.shape)
    for v in np.unique(plane):
        if v == 0:
            continue
        lab, n = ndimage.label(plane == v, structure=_EIGHT if connectivity == 8 else _FOUR)
        firsts = ndimage.minimum(flat, lab, index=np.arange(1, n + 1)) if n else []
        for i in range(n):
            comps.append((int(firsts[i]), lab == i + 1))
    comps.sort(key=lambda c: c[0])
    out = np.zeros(plane.shape, dtype=np.int32)
    for i, (_, m) in enumerate(comps):
        out[m] = i + 1
    return out, len(comps)


def component_sizes(lab, n):
    return np.bincount(lab.ravel(), minlength=n + 1)[1:]


def cell_count(plane, min_value=10):
    """ComputeStatistics.py:160-164: len(np.unique(label image)) - 1 -- the component count, or ONE LESS when the plane has no background pixel"""
    lab, _ = label(plane, min_value)
    return len(np.unique(lab)) - 1


# ---------------------------------------------------------------------------------------------------- AJI
def compute_aji_table(gt_mask, pred_mask):
    """The same result from an intersection table (one np.unique over the paired labels) instead of G x P full-size logical_ands, for images with
    hundreds of components, where the slow way takes minutes.  tests/test_stat_ref_host.py holds it to compute_aji on every fixture case."""
    lg, n_gt = label((np.asarray(gt_mask) > 0).astype(np.uint8))
    lp, n_pred = label((np.asarray(pred_mask) > 0).astype(np.uint8))
    sg, sp = component_sizes(lg, n_gt), component_sizes(lp, n_pred)
    both = (lg > 0) & (lp > 0)
    keys, counts = np.unique(lg[both].astype(np.int64) * (n_pred + 1) + lp[both], return_counts=True)
    rows = collections.defaultdict(list)
    for k, c in zip(keys.tolist(), counts.tolist()):
        rows[k // (n_pred + 1)].append((k % (n_pred + 1), c))            # (ascending pred label)
    marked = [False] * (n_pred + 1)
    ti = tu = 0
    for g in range(1, n_gt + 1):
        best = (0, 0)
        for q, c in rows.get(g, []):
            if not marked[q] and c > best[1]:
                best = (q, c)
        if best[1] > 0:
            marked[best[0]] = True
            ti += best[1]
            tu += int(sg[g - 1]) + int(sp[best[0] - 1]) - best[1]
    tU = sum(int(sp[q - 1]) for q in range(1, n_pred + 1) if not marked[q])
    return (ti / (tu + tU) if (tu + tU) > 0 else 0), ti, tu, tU


def compute_aji(gt_mask, pred_mask, connectivity=8, tie='small', unmatched_union=False, ge=False):
    """Segmentation_Metrics.compute_aji the slow way -> (aji, total_intersection, total_union, total_U).  Masks are binarised with > 0."""
    gt_image = (np.asarray(gt_mask) > 0).astype(np.uint8)
    mask_image = (np.asarray(pred_mask) > 0).astype(np.uint8)
    label_image_gt, n_gt = label(gt_image, connectivity=connectivity)
    label_image_mask, n_mask = label(mask_image, connectivity=connectivity)
    mask_components = [label_image_mask == i for i in range(1, n_mask + 1)]
    mask_marked = [False] * n_mask
    total_intersection = total_union = total_U = 0
    order = range(n_mask) if tie == 'small' else range(n_mask - 1, -1, -1)
    for g in range(1, n_gt + 1):
        comp = label_image_gt == g
        best = [0, 0, 0]            # index, intersection, union
        for i in order:
            if mask_marked[i]:
                continue
            inter = int(np.sum(np.logical_and(comp, mask_components[i])))
            if (inter >= best[1]) if ge else (inter > best[1]):
                best = [i, inter, int(np.sum(np.logical_or(comp, mask_components[i])))]
        if best[1] > 0:
            mask_marked[best[0]] = True
            total_intersection += best[1]
            total_union += best[2]
        elif unmatched_union:
            total_union += int(np.sum(comp))
    for i in range(n_mask):
        if not mask_marked[i]:
            total_U += int(np.sum(mask_components[i]))
    aji = total_intersection / (total_union + total_U) if (total_union + total_U) > 0 else 0
    return aji, total_intersection, total_union, total_U


# ---------------------------------------------------------------------------------------------------- confusion + the six metrics
def confusion(pred_plane, gt_plane):
    m, g = np.asarray(pred_plane) > 0, np.asarray(gt_plane) > 0
    return int(np.sum(m & g)), int(np.sum(m & ~g)), int(np.sum(~m & g)), int(np.sum(~m & ~g))


def metrics_from_counts(TP, FP, FN, TN):
    """compute_metrics_gpu :26-39 -> IOU, precision, recall, f1, Dice, pixAcc (np.count_nonzero(gt) = TP + FN)"""
    if TP == 0:
        if TP + FN > 0 or FP > 0:
            return 0, 0, 0, 0, 0, 0
        return 1, 1, 1, 1, 1, 1
    IOU = TP / (TP + FP + FN)
    precision = TP / (TP + FP)
    recall = TP / (TP + FN)
    f1 = 2 * precision * recall / (precision + recall)
    Dice = (2 * TP) / (2 * TP + FP + FN)
    pixAcc = (TP + TN) / (TP + TN + FP + FN)
    return IOU, precision, recall, f1, Dice, pixAcc


def segmentation_rows(per_image, model_name, names, with_aji):
    """compute_segmentation_metrics :157-232 from per-image values: per_image[i] = ((six metrics of the positive mask, AJI or None), (... negative)).
    Shared with nothing in the product: deepliif_amd/stat.py has its own copy of this bookkeeping."""
    info, metrics = [], collections.defaultdict(float)
    keys = ['IOU', 'precision', 'recall', 'f1', 'Dice', 'PixAcc']
    for name, ((mp, ap), (mn, an)) in zip(names, per_image):
        vals = {'Positive': dict(zip(keys, [v * 100 for v in mp])), 'Negative': dict(zip(keys, [v * 100 for v in mn]))}
        if with_aji:
            vals['Positive']['AJI'], vals['Negative']['AJI'] = ap * 100, an * 100
        cols = ['precision', 'recall', 'f1', 'Dice', 'IOU', 'PixAcc'] + (['AJI'] if with_aji else [])
        vals['Mean'] = {k: (vals['Positive'][k] + vals['Negative'][k]) / 2 for k in cols}
        for cell_type in ('Positive', 'Negative', 'Mean'):
            row = {'Model': model_name, 'image_name': name, 'cell_type': cell_type}
            row.update({k: vals[cell_type][k] for k in cols})
            info.append(row)
        raw = dict(zip(keys, zip(mp, mn)))
        if with_aji:
            raw['AJI'] = (ap, an)
        for k in ['precision', 'recall', 'f1', 'Dice', 'IOU', 'PixAcc'] + (['AJI'] if with_aji else []):
            metrics[k] += vals['Mean'][k]
            metrics[k + '_positive'] += raw[k][0]            # (a fraction, while metrics[k] is in percent: the script's quirk)
            metrics[k + '_negative'] += raw[k][1]
    for k in metrics:
        metrics[k] /= len(names)
    return info, metrics


def segmentation_metrics(gt, pred, model_name='DeepLIIF', names=None, aji=False, aji_fn=None):
    """lists of uint8 H x W x 3 images -> (info_rows, metrics); aji_fn = compute_aji_table for images with hundreds of components"""
    aji_fn = aji_fn or compute_aji
    names = list(names) if names is not None else [f'{i}_SegRefined.png' for i in range(len(gt))]
    per_image = []
    for g, p in zip(gt, pred):
        g, p = np.asarray(g), np.asarray(p)
        entry = []
        for c in (0, 2):
            six = metrics_from_counts(*confusion(p[..., c], g[..., c]))
            entry.append((six, aji_fn(g[..., c], p[..., c])[0] if aji else None))
        per_image.append(tuple(entry))
    return segmentation_rows(per_image, model_name, names, aji)


# ---------------------------------------------------------------------------------------------------- IHC score
def ihc_score(img):
    """positive cells / all cells (0 without cells), counted on channels 0 and 2 after values < 10 are zeroed"""
    img = np.asarray(img)
    pos, neg = cell_count(img[..., 0]), cell_count(img[..., 2])
    return pos / (pos + neg) if pos + neg > 0 else 0


def ihc_score_diff(gt, pred):
    diffs = [abs(ihc_score(g) * 100 - ihc_score(p) * 100) for g, p in zip(gt, pred)]
    return {'diff': np.array(diffs, dtype=np.float64), 'mean': sum(diffs) / len(diffs)}
