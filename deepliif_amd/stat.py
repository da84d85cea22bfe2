"""Model evaluation on the GPU -- the seam of DeepLIIF_Statistics (ComputeStatistics.py, Segmentation_Metrics.py) and deepliif/stat.

  image_similarity        MSE and SSIM of modality images                   (compute_mse_ssim_scores, ComputeStatistics.py:72-92)
  segmentation_metrics    IOU / precision / recall / f1 / Dice / PixAcc (+ AJI) per cell class
                                                                            (compute_segmentation_metrics, Segmentation_Metrics.py:105-232)
  aji                     the aggregated Jaccard index                      (compute_aji, Segmentation_Metrics.py:64-102)
  ihc_score_diff          difference of the positive-cell fractions         (compute_IHC_scoring, ComputeStatistics.py:150-182)
  swd, compute_swd        the sliced Wasserstein distance of two image sets (swd.py; the <type>_swd_value column, ComputeStatistics.py:116-128)
  compute_statistics      the directory driver that writes the script's CSV files
  get_cell_count_metrics  metrics.json for --with-val training              (deepliif/stat/__init__.py)

The per-pixel work runs in csrc/stat.hip (dl_stat_similarity, dl_stat_confusion, dl_stat_label, dl_stat_aji) and csrc/swd.hip (dl_swd_patches,
dl_swd_normalise, dl_swd_distance); no label image and no per-pixel array comes back to the host, only a few numbers per image.  Images are PIL images, ndarrays or CUDA tensors, uint8: H x W x 3 (RGB), H x W
(gray), a list of them, or one [N, H, W, 3] array.  The images of a pair must have the same size: the reference scripts cv2.resize to 512 x 512,
this module raises instead.  There is no CPU fallback: without the HIP library (or with CPU tensors that cannot be uploaded) this module raises.
"""
from __future__ import annotations

import collections
import csv
import json
import os

import numpy as np
import torch

from . import _lib as L
from . import ops

IHC_MIN_VALUE = 10           # ComputeStatistics.py:160, 168: image[image < 10] = 0
_METRIC_KEYS = ('IOU', 'precision', 'recall', 'f1', 'Dice', 'PixAcc')          # the order compute_metrics_gpu returns them in
_ROW_KEYS = ('precision', 'recall', 'f1', 'Dice', 'IOU', 'PixAcc')             # the order of the CSV columns


# ---------------------------------------------------------------------------------------------------- inputs
def _device(*xs) -> torch.device:
    for x in xs:
        for t in (x if isinstance(x, (list, tuple)) else [x]):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                return t.device
    return torch.device('cuda', torch.cuda.current_device())


def _one(img) -> torch.Tensor:
    if isinstance(img, torch.Tensor):
        return img
    try:
        from PIL import Image
        if isinstance(img, Image.Image):
            img = np.asarray(img if img.mode in ('RGB', 'L') else img.convert('RGB'))
    except ImportError:
        pass
    return torch.from_numpy(np.array(img, copy=True))            # (PIL-backed arrays are read-only)


def _batch(x, device) -> torch.Tensor:
    """-> uint8 CUDA tensor [N, H, W, C], C = 3 (RGB) or 1 (gray), unit channel stride and pixel stride C; row and image strides are kept,
    so a panel cut from a wider row is not copied"""
    if isinstance(x, (list, tuple)):
        if not x:
            raise ValueError('an empty list of images')
        ts = [_batch(i, device) for i in x]
        if any(t.shape[0] != 1 for t in ts):
            raise ValueError('a list holds single images (H x W x 3 or H x W)')
        if any(t.shape != ts[0].shape for t in ts):
            raise ValueError(f'the images of one call must have one size and kind, got {sorted(set(tuple(t.shape[1:]) for t in ts))} '
                             f'(the reference resizes; this module does not)')
        return ts[0] if len(ts) == 1 else torch.cat(ts, 0)
    t = _one(x)
    if t.dtype != torch.uint8:
        raise ValueError(f'expected uint8 images, got {t.dtype}')
    if t.dim() == 2:
        t = t[None, :, :, None]
    elif t.dim() == 3 and t.shape[2] == 3:
        t = t[None]
    elif not (t.dim() == 4 and t.shape[3] == 3):
        raise ValueError(f'expected H x W x 3, H x W, a list of them or [N, H, W, 3], got {tuple(t.shape)}')
    t = t.to(device)
    C_ = t.shape[3]
    ok = t.stride(2) == C_ and (C_ == 1 or t.stride(3) == 1) and t.stride(1) >= t.shape[2] * C_ and (t.shape[0] == 1 or t.stride(0) >= 1)
    return t if ok else t.contiguous()


def _pair(gt, pred, rgb_only=False):
    dev = _device(gt, pred)
    a, b = _batch(gt, dev), _batch(pred, dev)
    if a.shape != b.shape:
        raise ValueError(f'ground truth {tuple(a.shape)} and prediction {tuple(b.shape)} differ in number, size or kind; the reference scripts '
                         f'cv2.resize both to 512 x 512, this module does not resize: bring the pairs to one size first')
    if rgb_only and a.shape[3] != 3:
        raise ValueError('expected RGB images (channel 0 = positive cells, channel 2 = negative cells)')
    ops._need_cuda(a, b)
    return a, b


def _lib():
    return ops.impl().lib


# ---------------------------------------------------------------------------------------------------- MSE / SSIM
def image_similarity(gt, pred, data_range=1.0):
    """MSE and SSIM of N image pairs -> {'mse': ndarray[N], 'ssim': ndarray[N]} (float64).

    The images become gray floats in [0, 1] the way the script makes them (skimage rgb2gray after img_as_float; gray input is v / 255); MSE is
    skimage's mean_squared_error, SSIM is structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range):
    an 11 x 11 Gaussian window, the mean over the interior [5:H-5, 5:W-5], so H, W >= 11.  All arithmetic is float64 on the GPU, summed in
    a fixed order: repeated calls return the same bits.

    Two deviations from ComputeStatistics.py:84, on purpose:
      * the script passes data_range=255 although its images are floats in [0, 1], which makes C1 and C2 65 025 times too large and every
        SSIM close to 1.  The default here is the data range the images have, 1.0; pass data_range=255 for the script's numbers.
      * the script passes multichannel=True on a 2-D image.  skimage of its time turned that into a 1-D SSIM per image column, current
        skimage rejects the argument.  This is the 2-D definition.
    """
    a, b = _pair(gt, pred)
    N, H, W, ch = (int(v) for v in a.shape)
    if H < 11 or W < 11:
        raise ValueError(f'SSIM with the 11 x 11 Gaussian window needs H, W >= 11, got {H} x {W}')
    lib = _lib()
    out = np.empty((N, 2), dtype=np.float64)
    for n0 in range(0, N, 65535):
        n = min(65535, N - n0)
        ws = torch.empty(int(lib.dl_stat_similarity_ws_bytes(n, H, W)), dtype=torch.uint8, device=a.device)
        res = torch.empty((n, 2), dtype=torch.float64, device=a.device)
        p = ops._ptr
        L.check(lib.dl_stat_similarity(p(a[n0:]), a.stride(1), a.stride(0), p(b[n0:]), b.stride(1), b.stride(0), ch, n, H, W, float(data_range),
                                       p(ws), p(res), ops._stream(a)), 'dl_stat_similarity', lib)
        out[n0:n0 + n] = res.cpu().numpy()
    return {'mse': out[:, 0].copy(), 'ssim': out[:, 1].copy()}


# ---------------------------------------------------------------------------------------------------- labelling
class Components:
    """One labelled plane, on the device: labels int32 [H][W] (skimage.measure.label's numbering, 0 = background), info int32 [2] =
    (number of components, labelled pixels), sizes int32 [H * W] of which the first `number of components` are valid."""

    def __init__(self, labels, info, sizes):
        self.labels, self.info, self.sizes = labels, info, sizes


def _label_plane(t: torch.Tensor, n: int, c: int, min_value: int, binarize: bool, ws=None) -> Components:
    """channel c of image n of a _batch tensor"""
    lib = _lib()
    _, H, W, ch = (int(v) for v in t.shape)
    nbytes = int(lib.dl_stat_label_ws_bytes(H, W))
    if nbytes == 0:
        raise RuntimeError('dl_stat_label_ws_bytes failed (empty or too large image)')
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
    labels = torch.empty((H, W), dtype=torch.int32, device=t.device)
    info = torch.empty(2, dtype=torch.int32, device=t.device)
    sizes = torch.empty(H * W, dtype=torch.int32, device=t.device)
    p = ops._ptr
    L.check(lib.dl_stat_label(L.C.c_void_p(t.data_ptr() + n * t.stride(0) + c), t.stride(1), ch, H, W, int(min_value), int(bool(binarize)),
                              p(ws), p(labels), p(info), p(sizes), ops._stream(t)), 'dl_stat_label', lib)
    return Components(labels, info, sizes)


def label_components(plane, min_value=0, binarize=False) -> Components:
    """skimage.measure.label(plane, background=0) of an H x W uint8 plane (after values < min_value are zeroed; binarize: of plane > 0):
    8-connected components of equal value, numbered in raster order of their first pixel.  The result stays on the device."""
    t = _batch(plane, _device(plane))
    if t.shape[0] != 1 or t.shape[3] != 1:
        raise ValueError('expected one H x W plane')
    ops._need_cuda(t)
    return _label_plane(t, 0, 0, min_value, binarize)


# ---------------------------------------------------------------------------------------------------- AJI
def _aji_device(g: Components, q: Components, ws=None) -> torch.Tensor:
    lib = _lib()
    H, W = (int(v) for v in g.labels.shape)
    nbytes = int(lib.dl_stat_aji_ws_bytes(H, W))
    if nbytes == 0:
        raise RuntimeError('dl_stat_aji_ws_bytes failed (empty or too large image)')
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=g.labels.device)
    out = torch.empty(3, dtype=torch.int64, device=g.labels.device)
    p = ops._ptr
    L.check(lib.dl_stat_aji(p(g.labels), p(g.info), p(g.sizes), p(q.labels), p(q.info), p(q.sizes), H, W, p(ws), p(out), ops._stream(g.labels)),
            'dl_stat_aji', lib)
    return out


def _aji_value(ti: int, tu: int, tU: int):
    return ti / (tu + tU) if tu + tU > 0 else 0


def _aji_planes(a, b, channels):
    """a = ground truth, b = prediction (_batch tensors) -> int64 ndarray [N][len(channels)][3]; one device-to-host copy"""
    outs = []
    for n in range(a.shape[0]):
        for c in channels:
            outs.append(_aji_device(_label_plane(a, n, c, 0, True), _label_plane(b, n, c, 0, True)))
    return torch.stack(outs).cpu().numpy().reshape(a.shape[0], len(channels), 3)


def aji(gt_mask, pred_mask):
    """compute_aji(gt_mask, pred_mask) -> (aji, total_intersection, total_union, total_U).  Masks are H x W planes, binarised with > 0;
    their 8-connected components are matched greedily in the ground truth's label order (the largest intersection among the predicted
    components not taken yet, the first of equals); a ground-truth component without a match adds nothing, as in the reference."""
    a, b = _pair(gt_mask, pred_mask)
    if a.shape[0] != 1 or a.shape[3] != 1:
        raise ValueError('expected one pair of H x W masks')
    ti, tu, tU = (int(v) for v in _aji_planes(a, b, (0,))[0, 0])
    return _aji_value(ti, tu, tU), ti, tu, tU


# ---------------------------------------------------------------------------------------------------- segmentation metrics
def _confusion(a, b) -> np.ndarray:
    """a = ground truth, b = prediction -> int64 [N][2][4] = TP, FP, FN, TN of channel 0 and channel 2"""
    lib = _lib()
    N, H, W, _ = (int(v) for v in a.shape)
    out = np.empty((N, 2, 4), dtype=np.int64)
    p = ops._ptr
    for n0 in range(0, N, 65535):
        n = min(65535, N - n0)
        res = torch.empty((n, 2, 4), dtype=torch.int64, device=a.device)
        L.check(lib.dl_stat_confusion(p(b[n0:]), b.stride(1), b.stride(0), p(a[n0:]), a.stride(1), a.stride(0), n, H, W, p(res), ops._stream(a)),
                'dl_stat_confusion', lib)
        out[n0:n0 + n] = res.cpu().numpy()
    return out


def _six_metrics(TP, FP, FN, TN):
    """compute_metrics_gpu, Segmentation_Metrics.py:26-39 -> IOU, precision, recall, f1, Dice, pixAcc"""
    if TP == 0:
        if TP + FN > 0 or FP > 0:            # np.count_nonzero(gt_img) = TP + FN
            return 0, 0, 0, 0, 0, 0
        return 1, 1, 1, 1, 1, 1
    IOU = TP / (TP + FP + FN)
    precision = TP / (TP + FP)
    recall = TP / (TP + FN)
    f1 = 2 * precision * recall / (precision + recall)
    Dice = (2 * TP) / (2 * TP + FP + FN)
    pixAcc = (TP + TN) / (TP + TN + FP + FN)
    return IOU, precision, recall, f1, Dice, pixAcc


def _segmentation_values(a, b, with_aji):
    """per image: {'Positive': {key: fraction}, 'Negative': {...}}"""
    conf = _confusion(a, b)
    sums = _aji_planes(a, b, (0, 2)) if with_aji else None
    vals = []
    for n in range(a.shape[0]):
        entry = {}
        for k, cell_type in enumerate(('Positive', 'Negative')):
            d = dict(zip(_METRIC_KEYS, _six_metrics(*(int(v) for v in conf[n, k]))))
            if with_aji:
                d['AJI'] = _aji_value(*(int(v) for v in sums[n, k]))
            entry[cell_type] = d
        vals.append(entry)
    return vals


def _segmentation_rows(vals, model_name, names, with_aji):
    """the bookkeeping of compute_segmentation_metrics :157-232"""
    cols = list(_ROW_KEYS) + (['AJI'] if with_aji else [])
    info, metrics = [], collections.defaultdict(float)
    for name, v in zip(names, vals):
        pos = {k: v['Positive'][k] * 100 for k in cols}
        neg = {k: v['Negative'][k] * 100 for k in cols}
        mean = {k: (pos[k] + neg[k]) / 2 for k in cols}
        for cell_type, d in (('Positive', pos), ('Negative', neg), ('Mean', mean)):
            row = {'Model': model_name, 'image_name': name, 'cell_type': cell_type}
            row.update(d)
            info.append(row)
        for k in cols:
            metrics[k] += mean[k]                                   # in percent ...
            metrics[k + '_positive'] += v['Positive'][k]            # ... while these two are fractions: the script's own convention
            metrics[k + '_negative'] += v['Negative'][k]
    for k in metrics:
        metrics[k] /= len(vals)
    return info, metrics


def segmentation_metrics(gt, pred, model_name='DeepLIIF', names=None, aji=False):
    """compute_segmentation_metrics on images instead of directories -> (info_rows, metrics).

    gt / pred: N pairs of RGB masks (ground truth and `*_SegRefined.png`): channel 0 > 0 are the positive cells, channel 2 > 0 the negative
    ones.  info_rows holds three dicts per image (cell_type Positive, Negative, Mean) with the keys Model, image_name, cell_type, precision,
    recall, f1, Dice, IOU, PixAcc in percent; metrics holds the means over the images, with the script's conventions: metrics['precision']
    is in percent while metrics['precision_positive'] and metrics['precision_negative'] are fractions.  An image without true positives gets
    0 everywhere if the ground truth has pixels or the prediction has false positives, and 1 everywhere otherwise.  aji=True adds the AJI
    column and the AJI, AJI_positive, AJI_negative keys that the script has commented out."""
    a, b = _pair(gt, pred, rgb_only=True)
    names = list(names) if names is not None else [f'{i}_SegRefined.png' for i in range(a.shape[0])]
    if len(names) != a.shape[0]:
        raise ValueError(f'{len(names)} names for {a.shape[0]} image pairs')
    return _segmentation_rows(_segmentation_values(a, b, aji), model_name, names, aji)


# ---------------------------------------------------------------------------------------------------- IHC score
def _cell_counts(t) -> np.ndarray:
    """-> int64 [N][2]: cells on channel 0 and channel 2, counted as compute_IHC_scoring does: len(np.unique(label image)) - 1, which is the
    number of components, or one less when the plane has no background pixel (then 0 is not among the labels)"""
    N, H, W, _ = (int(v) for v in t.shape)
    infos = torch.stack([_label_plane(t, n, c, IHC_MIN_VALUE, False).info for n in range(N) for c in (0, 2)]).cpu().numpy().astype(np.int64)
    counts = infos[:, 0] - (infos[:, 1] == H * W)
    return counts.reshape(N, 2)


def _ihc_scores(t):
    return [int(p) / int(p + q) if p + q > 0 else 0 for p, q in _cell_counts(t)]


def ihc_score_diff(gt, pred):
    """compute_IHC_scoring on images -> {'diff': ndarray[N], 'mean': float}: |100 * pos_gt / all_gt - 100 * pos_pred / all_pred| per pair, where
    pos and all - pos are the numbers of 8-connected components of equal value on channel 0 and channel 2 after values < 10 are zeroed, and a
    score without cells is 0."""
    a, b = _pair(gt, pred, rgb_only=True)
    diffs = [abs(g * 100 - m * 100) for g, m in zip(_ihc_scores(a), _ihc_scores(b))]
    return {'diff': np.array(diffs, dtype=np.float64), 'mean': sum(diffs) / len(diffs)}


# ---------------------------------------------------------------------------------------------------- sliced Wasserstein distance
SWD_PATCH = 7                # swd.py hard-codes the 6 = 7 - 1 of the window count and the 3 * 7 * 7 of the descriptor
SWD_COLUMNS = 3 * SWD_PATCH * SWD_PATCH
SWD_CHUNK = 16               # images whose pyramid is held at once: the pyramid workspace does not grow with the set


def swd_level_shapes(H, W, n_pyramids):
    """(h, w) of the n_pyramids + 1 levels: pyramid_down gives floor((h - 1) / 2) + 1"""
    shapes = [(int(H), int(W))]
    for _ in range(int(n_pyramids)):
        h, w = shapes[-1]
        shapes.append(((h - 1) // 2 + 1, (w - 1) // 2 + 1))
    return shapes


class SwdDraws:
    """The random draws of one swd() call: per level the patch positions (int64 ndarray, at most n_descriptors of them) and the projection
    directions (float32 ndarray [n_repeat_projection][147][proj_per_repeat], every column divided by its unbiased std)."""

    def __init__(self, level_shapes, n_descriptors, n_repeat_projection, proj_per_repeat, indices, projections):
        self.level_shapes = [tuple(int(v) for v in s) for s in level_shapes]
        self.n_descriptors, self.n_repeat_projection, self.proj_per_repeat = int(n_descriptors), int(n_repeat_projection), int(proj_per_repeat)
        self.indices, self.projections = indices, projections


def swd_draws(level_shapes, n_descriptors=128, n_repeat_projection=128, proj_per_repeat=4, generator=None) -> SwdDraws:
    """The draws of swd.py:115-133, on the host, in the reference's order: per level torch.randperm((h - 6) * (w - 6))[:n_descriptors], then
    n_repeat_projection times torch.randn(147, proj_per_repeat) divided by its columns' unbiased std, in float32.  generator=None draws from
    torch's global CPU generator, so after torch.manual_seed(s) these are the draws of the reference's swd(..., device='cpu') after the same
    call.  Needs neither the GPU nor the HIP library."""
    if n_descriptors < 1 or n_repeat_projection < 1 or proj_per_repeat < 2:
        raise ValueError('n_descriptors, n_repeat_projection >= 1 and proj_per_repeat >= 2 (the unbiased std of one value does not exist)')
    indices, projections = [], []
    for h, w in level_shapes:
        if h < SWD_PATCH or w < SWD_PATCH:
            raise ValueError(f'a level of {h} x {w} is below the {SWD_PATCH} x {SWD_PATCH} patch')
        n = (int(h) - (SWD_PATCH - 1)) * (int(w) - (SWD_PATCH - 1))
        indices.append(torch.randperm(n, generator=generator)[:n_descriptors].numpy().astype(np.int64))
        mats = []
        for _ in range(n_repeat_projection):
            r = torch.randn(SWD_COLUMNS, proj_per_repeat, generator=generator)
            mats.append((r / torch.std(r, dim=0, keepdim=True)).numpy())
        projections.append(np.stack(mats).astype(np.float32))
    return SwdDraws(level_shapes, n_descriptors, n_repeat_projection, proj_per_repeat, indices, projections)


def _swd_patches(t: torch.Tensor, n_pyramids: int, indices) -> list:
    """stage 1 (dl_swd_patches): a _batch RGB tensor -> per level the RAW patch matrix, float64 [N * D_l][147] on the device"""
    lib = _lib()
    N, H, W, _ = (int(v) for v in t.shape)
    counts = [int(len(i)) for i in indices]
    idx = torch.from_numpy(np.concatenate([np.asarray(i) for i in indices]).astype(np.int32)).to(t.device)
    out = torch.empty(N * sum(counts) * SWD_COLUMNS, dtype=torch.float64, device=t.device)
    chunk = min(N, SWD_CHUNK)
    nbytes = int(lib.dl_swd_patches_ws_bytes(chunk, H, W, n_pyramids))
    if nbytes == 0:
        raise RuntimeError(f'dl_swd_patches_ws_bytes refused N={chunk} H={H} W={W} n_pyramids={n_pyramids}')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
    c_counts = (L.C.c_int * len(counts))(*counts)
    p = ops._ptr
    for n0 in range(0, N, chunk):
        n = min(chunk, N - n0)
        L.check(lib.dl_swd_patches(p(t[n0:]), t.stride(1), t.stride(0), n, H, W, n_pyramids, p(idx), c_counts, N, n0, p(ws), p(out), ops._stream(t)),
                'dl_swd_patches', lib)
    mats, off = [], 0
    for d in counts:
        mats.append(out[off:off + N * d * SWD_COLUMNS].view(N * d, SWD_COLUMNS))
        off += N * d * SWD_COLUMNS
    return mats


def _swd_normalise(x: torch.Tensor) -> torch.Tensor:
    """stage 2 (dl_swd_normalise): x float64 [R][147] is normalised in place -> stats float64 [6] = mean, unbiased std per channel (device)"""
    lib = _lib()
    R = int(x.shape[0])
    ws = torch.empty(int(lib.dl_swd_normalise_ws_bytes(R)), dtype=torch.uint8, device=x.device)
    stats = torch.empty(6, dtype=torch.float64, device=x.device)
    L.check(lib.dl_swd_normalise(ops._ptr(x), R, ops._ptr(ws), ops._ptr(stats), ops._stream(x)), 'dl_swd_normalise', lib)
    return stats


def _swd_distances(a: torch.Tensor, b: torch.Tensor, proj: torch.Tensor, route: int = 0) -> torch.Tensor:
    """stage 3 (dl_swd_distance): normalised sets a, b float64 [R][147], directions proj float32 [P][147] -> float64 [P] (device)"""
    lib = _lib()
    R, P = int(a.shape[0]), int(proj.shape[0])
    nbytes = int(lib.dl_swd_distance_ws_bytes(R, P, int(route)))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=a.device)
    out = torch.empty(P, dtype=torch.float64, device=a.device)
    L.check(lib.dl_swd_distance(ops._ptr(a), ops._ptr(b), R, ops._ptr(proj), P, int(route), ops._ptr(ws), ops._ptr(out), ops._stream(a)),
            'dl_swd_distance', lib)
    return out


def swd_lds_rows() -> int:
    """the most rows (images x descriptors) whose projections a workgroup sorts in LDS; above, hipcub sorts them in global memory"""
    return int(_lib().dl_swd_lds_rows())


def _swd_directions(projections: np.ndarray, device) -> torch.Tensor:
    """[n_repeat][147][proj_per_repeat] -> float32 [n_repeat * proj_per_repeat][147] on the device"""
    return torch.from_numpy(np.ascontiguousarray(projections.transpose(0, 2, 1).reshape(-1, SWD_COLUMNS), dtype=np.float32)).to(device)


def swd(gt, pred, n_pyramids=None, slice_size=7, n_descriptors=128, n_repeat_projection=128, proj_per_repeat=4, return_by_resolution=False,
        generator=None, draws=None, route=0):
    """The sliced Wasserstein distance of two image SETS, swd() of DeepLIIF_Statistics/swd.py -> float, or with return_by_resolution a float64
    ndarray [n_pyramids + 1] (finest level first).

    Images as image_similarity takes them, RGB only, both sets of one shape.  Per level of a Laplacian pyramid (5 x 5 binomial kernel, zero
    padding, nearest up-sampling; n_pyramids defaults to round(log2(H // 16))) the same n_descriptors random 7 x 7 x 3 patches are taken from
    every image of both sets (all positions where a level has fewer), normalised per channel with the mean and unbiased std of their own set,
    projected onto n_repeat_projection x proj_per_repeat random directions and sorted; the level's value is the mean absolute difference of
    the sorted projections, the result the levels' mean times 1e3.  It needs no network weights.

    The random draws are made on the host by swd_draws (generator=None: torch's global CPU generator, as the reference with device='cpu'),
    or passed as draws= to reuse them.  Everything else runs on the GPU in float64 in a fixed order: with the same draws two calls return
    the same bits, and swd(x, x) is exactly 0.  The reference computes in float32, so its numbers agree to about 1e-6 relative, not
    bit for bit.  route: 0 chooses the sort by size, 1 / 2 force the LDS / global-memory sort (dl_swd_distance)."""
    if slice_size != SWD_PATCH:
        raise ValueError(f'slice_size={slice_size}: the reference hard-codes 7 (the 6 of its window count and the 3 * 7 * 7 of its projections)')
    a, b = _pair(gt, pred)
    if a.shape[3] != 3:
        raise ValueError('expected RGB images, got gray ones')
    N, H, W, _ = (int(v) for v in a.shape)
    if n_pyramids is None:
        if H < 16:
            raise ValueError(f'n_pyramids defaults to round(log2(H // 16)), which does not exist for H={H}: pass n_pyramids')
        n_pyramids = int(np.rint(np.log2(H // 16)))
    n_pyramids = int(n_pyramids)
    if n_pyramids < 0 or n_pyramids > 15:
        raise ValueError(f'n_pyramids={n_pyramids}')
    if H % (1 << n_pyramids) or W % (1 << n_pyramids):
        raise ValueError(f'H={H} and W={W} must be divisible by 2**n_pyramids = {1 << n_pyramids} (the reference fails there with a shape mismatch)')
    shapes = swd_level_shapes(H, W, n_pyramids)
    if shapes[-1][0] < SWD_PATCH or shapes[-1][1] < SWD_PATCH:
        raise ValueError(f'the smallest level, {shapes[-1][0]} x {shapes[-1][1]}, is below the 7 x 7 patch: fewer pyramids or larger images')
    if draws is None:
        draws = swd_draws(shapes, n_descriptors, n_repeat_projection, proj_per_repeat, generator)
    elif draws.level_shapes != shapes:
        raise ValueError(f'draws were made for the levels {draws.level_shapes}, the images have {shapes}')
    pa, pb = _swd_patches(a, n_pyramids, draws.indices), _swd_patches(b, n_pyramids, draws.indices)
    per_column = []
    for l in range(n_pyramids + 1):
        _swd_normalise(pa[l])
        _swd_normalise(pb[l])
        per_column.append(_swd_distances(pa[l], pb[l], _swd_directions(draws.projections[l], a.device), route))
    cols = torch.stack(per_column).cpu().numpy()                               # one device-to-host copy: [levels][n_repeat * proj_per_repeat]
    levels = np.array([row.reshape(draws.n_repeat_projection, draws.proj_per_repeat).mean(axis=1).mean() for row in cols], dtype=np.float64) * 1e3
    return levels if return_by_resolution else float(levels.mean())


_swd = swd                   # (compute_statistics has a flag of that name)


def compute_swd(orig_images, mask_images, device=None):
    """compute_swd of swd.py:153-158: two [N, H, W, 3] uint8 arrays -> swd() with the defaults.  device (the reference's 'cpu' / 'cuda') only
    says where the tensors are put: a torch.device or None for the current GPU."""
    if device is not None and torch.device(device).type == 'cuda':
        orig_images, mask_images = (x.to(device) if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(device)
                                    for x in (orig_images, mask_images))
    return swd(orig_images, mask_images)


# ---------------------------------------------------------------------------------------------------- the directory driver
def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im if im.mode in ('RGB', 'L') else im.convert('RGB'))


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))


def _by_shape(items):
    """indices of `items` (arrays) grouped by shape, so that every group goes through the kernels as one batch"""
    groups = collections.OrderedDict()
    for i, x in enumerate(items):
        groups.setdefault(x.shape, []).append(i)
    return list(groups.values())


def _write_rows(path, rows, columns):
    with open(path, 'w', newline='') as f:
        w = csv.DictWriter(f, fieldnames=list(columns))
        w.writeheader()
        for r in rows:
            w.writerow(r)


def compute_statistics(gt_path, model_path, output_path, model_name='DeepLIIF', mode='Segmentation', image_types=('Hema', 'DAPI', 'Lap2', 'Marker'),
                       aji=False, raw_segmentation=False, swd=False):
    """DeepLIIF_Statistics/ComputeStatistics.py on two directories of PNG files -> the dict the script calls all_info; writes into output_path:

      mode 'Segmentation':   segmentation_info_<mode>_<model>_100_50.csv (Model, image_name, cell_type, precision, recall, f1, Dice, IOU, PixAcc
                             [, AJI]), IHC_Scoring_info_<mode>_<model>.csv (Model, Sample, Diff_IHC_Score)
      mode 'ImageSynthesis': metrics_<mode>_<model>.csv (Model, <type>_MSE_avg, <type>_MSE_std, <type>_ssim_avg, <type>_ssim_std per image type;
                             and with swd=True <type>_swd_value after them; the script computes these in this mode and writes nothing)
      mode 'All':            all three, the metrics file with the segmentation means (precision, precision_positive, ...) after the similarity columns.

    Files are paired by name as the script pairs them: every `<name>_SegRefined.png` of model_path with `<name>.png` of gt_path; every file of
    model_path whose name contains an image type with the file of the same name in gt_path; for the IHC score every file of gt_path with
    `<name>_SegRefined.png` of model_path if 'DeepLIIF' is in model_name, else with the file of the same name (files of gt_path without such a
    partner are skipped, where the script would stop).  Directory listings are sorted.  Pairs of one size go through the kernels as one batch;
    the images of a pair must have the same size (the script resizes to 512 x 512, this does not).

    swd=True adds the script's <type>_swd_value column (compute_swd, ComputeStatistics.py:116-128): ONE sliced Wasserstein distance per image
    type over all pairs of that type (see swd(); the draws come from torch's global CPU generator, so seed it for a repeatable value).  It is a
    distance of two sets, so the pairs of a type must all have one size.  The default leaves every file as it is without it.

    Left out: the FID and inception-score columns (they need Inception weights and TensorFlow, which this package does not ship; SWD needs
    neither) and raw_segmentation=True (the `_Seg.png` route through positive_negative_masks): it raises NotImplementedError.  SSIM uses
    data_range=1.0 and the 2-D definition (see image_similarity)."""
    if raw_segmentation:
        raise NotImplementedError('raw_segmentation=True (positive_negative_masks on *_Seg.png) is not implemented; evaluate the *_SegRefined.png images')
    if mode not in ('Segmentation', 'ImageSynthesis', 'All'):
        raise ValueError(f"mode {mode!r} (Segmentation | ImageSynthesis | All)")
    os.makedirs(output_path, exist_ok=True)
    all_info = {'Model': model_name}
    listing = sorted(os.listdir(model_path))

    if mode in ('ImageSynthesis', 'All'):
        for img_type in image_types:
            names = [n for n in listing if img_type in n]
            if not names:
                raise FileNotFoundError(f'no file of {model_path} has {img_type!r} in its name')
            gts, preds = [_read(os.path.join(gt_path, n)) for n in names], [_read(os.path.join(model_path, n)) for n in names]
            mse, ssim = np.empty(len(names)), np.empty(len(names))
            for idx in _by_shape(preds):
                r = image_similarity([gts[i] for i in idx], [preds[i] for i in idx])
                mse[idx], ssim[idx] = r['mse'], r['ssim']
            all_info[img_type + '_MSE_avg'], all_info[img_type + '_MSE_std'] = np.mean(mse), np.std(mse)
            all_info[img_type + '_ssim_avg'], all_info[img_type + '_ssim_std'] = np.mean(ssim), np.std(ssim)
            if swd:
                if len(_by_shape(preds)) != 1:
                    raise ValueError(f'swd=True: the {img_type} images have the sizes {sorted(set(x.shape for x in preds))}; the sliced Wasserstein '
                                     f'distance is taken over one set of one size (the script resizes to 512 x 512, this does not)')
                rgb = lambda x: x if x.ndim == 3 else np.repeat(x[:, :, None], 3, axis=2)          # (the script's cv2.imread gives three channels)
                all_info[img_type + '_swd_value'] = _swd([rgb(x) for x in gts], [rgb(x) for x in preds])

    if mode in ('Segmentation', 'All'):
        postfix = '_SegRefined.png'
        names = [n for n in listing if postfix in n]
        if not names:
            raise FileNotFoundError(f'no *{postfix} file in {model_path}')
        gts = [_read_rgb(os.path.join(gt_path, n.replace(postfix, '.png'))) for n in names]
        preds = [_read_rgb(os.path.join(model_path, n)) for n in names]
        vals = [None] * len(names)
        for idx in _by_shape(preds):
            a, b = _pair([gts[i] for i in idx], [preds[i] for i in idx], rgb_only=True)
            for i, v in zip(idx, _segmentation_values(a, b, aji)):
                vals[i] = v
        info, metrics = _segmentation_rows(vals, model_name, names, aji)
        _write_rows(os.path.join(output_path, f'segmentation_info_{mode}_{model_name}_100_50.csv'), info, info[0].keys())
        all_info.update(metrics)

        samples, pairs = [], []
        for n in sorted(os.listdir(gt_path)):
            partner = os.path.join(model_path, n.replace('.png', postfix) if 'DeepLIIF' in model_name else n)
            if os.path.isfile(partner):
                samples.append(n)
                pairs.append((_read_rgb(os.path.join(gt_path, n)), _read_rgb(partner)))
        if not samples:
            raise FileNotFoundError(f'no file of {gt_path} has a prediction in {model_path}')
        diffs = np.empty(len(samples))
        for idx in _by_shape([p[1] for p in pairs]):
            diffs[idx] = ihc_score_diff([pairs[i][0] for i in idx], [pairs[i][1] for i in idx])['diff']
        _write_rows(os.path.join(output_path, f'IHC_Scoring_info_{mode}_{model_name}.csv'),
                    [{'Model': model_name, 'Sample': s, 'Diff_IHC_Score': d} for s, d in zip(samples, diffs.tolist())], ['Model', 'Sample', 'Diff_IHC_Score'])
        all_info['Diff_IHC_Score'] = sum(diffs.tolist()) / len(samples)

    if mode in ('ImageSynthesis', 'All'):
        cols = [k for k in all_info if k != 'Diff_IHC_Score']
        _write_rows(os.path.join(output_path, f'metrics_{mode}_{model_name}.csv'), [{k: all_info[k] for k in cols}], cols)
    return all_info


# ---------------------------------------------------------------------------------------------------- cell counts for --with-val
def get_cell_count_metrics(dir_seg, dir_input=None, dir_save=None, model='DeepLIIF', tile_size=512, single_tile=False, use_marker=False,
                           suffix_seg='5', suffix_marker='4', save_individual=False):
    """deepliif.stat.get_cell_count_metrics: the cell counts of ground-truth tiles through inference.postprocess (the GPU post-processing),
    written as <dir_save>/metrics.json = {image name: scoring dict}, the file --with-val training reads.  Returns the same dict.

    single_tile=False: every .png of dir_seg is a row of square tiles, the first is the input, the last the segmentation, the one before it
    the marker.  single_tile=True: <name>_<suffix_seg>.png, <name>_<suffix_marker>.png in dir_seg and <name>.png in dir_input.
    dir_input and dir_save default to dir_seg, as the reference documents them."""
    from PIL import Image
    from .inference import postprocess
    dir_save = dir_seg if dir_save is None else dir_save
    dir_input = dir_seg if dir_input is None else dir_input
    if single_tile:
        fns = [x for x in os.listdir(dir_seg) if x.endswith(f'_{suffix_seg}.png') or x.endswith(f'_{suffix_marker}.png')]
        fns = sorted(set('_'.join(x.split('_')[:-1]) for x in fns))
    else:
        fns = sorted(x for x in os.listdir(dir_seg) if x.endswith('.png'))
    d_metrics = {}
    for fn in fns:
        if single_tile:
            img_gt = Image.open(os.path.join(dir_seg, fn + f'_{suffix_seg}.png'))
            img_marker = Image.open(os.path.join(dir_seg, fn + f'_{suffix_marker}.png')) if use_marker else None
            img_input = Image.open(os.path.join(dir_input, fn + '.png'))
            k = fn
        else:
            img = Image.open(os.path.join(dir_seg, fn))
            w, h = img.size
            img_input = img.crop((0, 0, h, h))
            img_gt = img.crop((w - h, 0, w, h))
            img_marker = img.crop((w - h * 2, 0, w - h, h))
            k = os.path.splitext(fn)[0]
        images = {'Seg': img_gt}
        if use_marker:
            images['Marker'] = img_marker
        _, scoring = postprocess(img_input, images, tile_size, model)
        d_metrics[k] = scoring
        if save_individual:
            with open(os.path.join(dir_save, k + '.json'), 'w') as f:
                json.dump(scoring, f, indent=2)
    with open(os.path.join(dir_save, 'metrics.json'), 'w') as f:
        json.dump(d_metrics, f, indent=2)
    return d_metrics
