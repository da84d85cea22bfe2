"""A float64 numpy restatement of the sliced Wasserstein distance of DeepLIIF_Statistics/swd.py, with explicit draws, staged as the kernels of
csrc/swd.hip are: levels -> raw patches -> normalised descriptors -> per-direction distances -> result.  It is the yardstick of the GPU test;
tests/test_swd_ref_host.py holds it to what the reference's own swd() returned (tests/golden/swd_cases.npz).

The keyword arguments of the stages select DELIBERATE MISREADINGS of the reference (biased std, transposed index, ...): the host test shows
that each of them is caught.  error_bounds() is the derivation of the bounds that the GPU test applies (see its docstring)."""
import numpy as np

PATCH = 7
COLUMNS = 3 * PATCH * PATCH
K1 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
K5 = np.outer(K1, K1) / 256.0                    # swd.py:9-14


# ---------------------------------------------------------------------------------------------------- draws
class Draws:
    def __init__(self, level_shapes, indices, projections):
        self.level_shapes, self.indices, self.projections = [tuple(s) for s in level_shapes], indices, projections
        self.n_repeat_projection, self.proj_per_repeat = projections[0].shape[0], projections[0].shape[2]


def draws(level_shapes, n_descriptors=128, n_repeat_projection=128, proj_per_repeat=4, generator=None, renormalise=True, permutation_first=True):
    """swd.py:115-133 with torch's CPU generator (generator=None: the global one), in the reference's order"""
    import torch
    indices, projections = [], []
    for h, w in level_shapes:
        n = (h - 6) * (w - 6)
        if permutation_first:
            idx = torch.randperm(n, generator=generator)[:n_descriptors]
        mats = []
        for _ in range(n_repeat_projection):
            r = torch.randn(COLUMNS, proj_per_repeat, generator=generator)
            if renormalise:
                r = r / torch.std(r, dim=0, keepdim=True)
            mats.append(r.numpy())
        if not permutation_first:
            idx = torch.randperm(n, generator=generator)[:n_descriptors]
        indices.append(idx.numpy().astype(np.int64))
        projections.append(np.stack(mats).astype(np.float32))
    return Draws(level_shapes, indices, projections)


def directions(projections):
    """[n_repeat][147][proj_per_repeat] float32 -> float64 [n_repeat * proj_per_repeat][147]"""
    return np.ascontiguousarray(projections.transpose(0, 2, 1).reshape(-1, COLUMNS)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- pyramid
def to_float(images):
    """uint8 [N, H, W, 3] -> float64 [N, 3, H, W] in [0, 1] (swd.py:153-155)"""
    return np.ascontiguousarray(np.asarray(images).transpose(0, 3, 1, 2)).astype(np.float64) / 255.0


def conv5(x, stride=1, padding='zero'):
    """the 5 x 5 kernel per channel, padding 2: the 25 taps added directly"""
    xp = np.pad(x, ((0, 0), (0, 0), (2, 2), (2, 2)), mode='constant' if padding == 'zero' else 'edge')
    h, w = x.shape[2], x.shape[3]
    out = np.zeros(x.shape[:2] + ((h - 1) // stride + 1, (w - 1) // stride + 1), dtype=np.float64)
    for i in range(5):
        for j in range(5):
            out += K5[i, j] * xp[:, :, i:i + h:stride, j:j + w:stride]
    return out


def upsample2(x, mode='nearest'):
    if mode == 'nearest':
        return np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)
    for axis in (2, 3):                          # bilinear, align_corners=False: 0.75 / 0.25 of the two nearest, clamped at the border
        n = x.shape[axis]
        prev = np.take(x, np.maximum(np.arange(n) - 1, 0), axis=axis)
        nxt = np.take(x, np.minimum(np.arange(n) + 1, n - 1), axis=axis)
        even, odd = 0.75 * x + 0.25 * prev, 0.75 * x + 0.25 * nxt
        shape = list(x.shape)
        shape[axis] = 2 * n
        y = np.empty(shape, dtype=np.float64)
        sl = [slice(None)] * 4
        sl[axis] = slice(0, None, 2)
        y[tuple(sl)] = even
        sl[axis] = slice(1, None, 2)
        y[tuple(sl)] = odd
        x = y
    return x


def levels(images, n_pyramids, padding='zero', upsample='nearest'):
    """the Laplacian pyramid (swd.py:18-52): n_pyramids + 1 arrays [N, 3, h_l, w_l]"""
    g = [to_float(images)]
    for _ in range(n_pyramids):
        g.append(conv5(g[-1], stride=2, padding=padding))
    return [g[l] - conv5(upsample2(g[l + 1], upsample), padding=padding) for l in range(n_pyramids)] + [g[-1]]


# ---------------------------------------------------------------------------------------------------- descriptors
def raw_patches(level, indices, index_order='row'):
    """[N, 3, h, w] -> [N * D][147]: rows image-major then descriptor, columns channel, dy, dx (swd.py:81-94)"""
    n, _, h, w = level.shape
    hp, wp = h - 6, w - 6
    out = np.empty((n, len(indices), 3, PATCH, PATCH), dtype=np.float64)
    for d, i in enumerate(indices):
        py, px = (int(i) // wp, int(i) % wp) if index_order == 'row' else (int(i) % hp, int(i) // hp)
        out[:, d] = level[:, :, py:py + PATCH, px:px + PATCH]
    return out.reshape(n * len(indices), COLUMNS)


def channel_stats(x, biased=False):
    """mean and std per channel over all rows and the channel's 49 columns -> ([3], [3])"""
    v = x.reshape(-1, 3, PATCH * PATCH)
    return v.mean(axis=(0, 2)), v.std(axis=(0, 2), ddof=0 if biased else 1)


def normalise(x, stats=None, biased=False):
    mean, std = stats if stats is not None else channel_stats(x, biased)
    v = x.reshape(-1, 3, PATCH * PATCH)
    return ((v - mean[None, :, None]) / (std[None, :, None] + 1e-8)).reshape(x.shape)


def column_distances(a, b, dirs):
    """normalised [R][147] x 2, directions [P][147] -> [P]: mean |sort(a p) - sort(b p)| (swd.py:135-140)"""
    pa, pb = np.sort(a @ dirs.T, axis=0), np.sort(b @ dirs.T, axis=0)
    return np.abs(pa - pb).mean(axis=0)


def level_value(cols, n_repeat_projection, proj_per_repeat):
    return cols.reshape(n_repeat_projection, proj_per_repeat).mean(axis=1).mean() * 1e3


# ---------------------------------------------------------------------------------------------------- the whole
def stages(gt, pred, dr, n_pyramids, padding='zero', upsample='nearest', index_order='row', biased=False, joint_stats=False):
    """-> per level a dict: raw_a, raw_b, stats_a, stats_b, norm_a, norm_b, dirs, cols, value"""
    la, lb = levels(gt, n_pyramids, padding, upsample), levels(pred, n_pyramids, padding, upsample)
    out = []
    for l in range(n_pyramids + 1):
        ra, rb = raw_patches(la[l], dr.indices[l], index_order), raw_patches(lb[l], dr.indices[l], index_order)
        if joint_stats:
            sa = sb = channel_stats(np.concatenate([ra, rb]), biased)
        else:
            sa, sb = channel_stats(ra, biased), channel_stats(rb, biased)
        na, nb = normalise(ra, sa), normalise(rb, sb)
        dirs = directions(dr.projections[l])
        cols = column_distances(na, nb, dirs)
        out.append(dict(raw_a=ra, raw_b=rb, stats_a=sa, stats_b=sb, norm_a=na, norm_b=nb, dirs=dirs, cols=cols,
                        value=level_value(cols, dr.n_repeat_projection, dr.proj_per_repeat)))
    return out


def swd(gt, pred, dr, n_pyramids, **misreading):
    """-> float64 [n_pyramids + 1], what the reference returns with return_by_resolution=True"""
    return np.array([s['value'] for s in stages(gt, pred, dr, n_pyramids, **misreading)], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------- the bounds of the GPU test
U = 2.0 ** -53                                   # unit round-off of float64


def error_bounds(st, n_pyramids):
    """How far may two CORRECT float64 evaluations of the stages lie apart -- this restatement and the kernels, which add in other orders
    (separable 5 + 5 taps against 25 direct ones, per-thread and tree sums against numpy's pairwise ones, 16-lane dot products)?
    st = stages(...); -> dict(raw, stats, norm, cols, value), absolute bounds over all levels, from the data:

      raw    every Gaussian level is a convex combination of values in [0, 1]; a sum of T products carries at most (T + 1) u of its absolute
             sum, so one 25-tap (or 5 + 5-tap) pass adds at most 27 u and level l carries 27 l u.  A Laplacian value takes one more pass and a
             subtraction: 27 (n + 1) u + 2 u per side, twice that between two sides.
      stats  a mean or a variance summed over M values in chains of at most C terms (C <= 64 here: at most 1024 blocks x 256 threads, then
             8- and 10-step trees; numpy's pairwise sums are shorter) carries C u of the mean absolute value.  The mean moves by at most
             raw + C u max|x|; the std, which is 1-Lipschitz in the RMS of its data, by at most raw + (C + 4) u std + the mean's share.
      norm   (x - m) / (s + 1e-8): |d| <= (d_x + d_m) / s + |xhat| d_s / s + 3 u |xhat|, with the smallest s and the largest |xhat| of the data.
      cols   a projection is a 147-term dot product: |d_y| <= |p|_1 d_norm + 148 u |p|_1 max|xhat|.  Sorting is 1-Lipschitz in the sup norm
             and a mean of |a - b| cannot move more than its terms: |d_col| <= d_ya + d_yb (+ the mean's own 64 u of its value).
      value  1e3 times a mean of columns: 1e3 d_col."""
    side = 27.0 * (n_pyramids + 1) * U + 2.0 * U
    raw = 2.0 * side
    C = 64.0
    stats = norm = d_y = cols_max = 0.0
    for s in st:
        d_ys = []
        for k in ('a', 'b'):
            x, (mean, std), xh = s['raw_' + k], s['stats_' + k], s['norm_' + k]
            xmax, hmax, smin = np.abs(x).max(), np.abs(xh).max(), std.min()
            d_m = raw + C * U * xmax
            d_s = raw + (C + 4.0) * U * std.max() + d_m
            d_n = (raw + d_m) / smin + hmax * d_s / smin + 3.0 * U * hmax
            p1 = np.abs(s['dirs']).sum(axis=1).max()
            d_ys.append(p1 * d_n + 148.0 * U * p1 * hmax)
            stats, norm = max(stats, d_s), max(norm, d_n)
        cols_max = max(cols_max, d_ys[0] + d_ys[1] + C * U * s['cols'].max())
    return dict(raw=raw, stats=stats, norm=norm, cols=cols_max, value=1e3 * cols_max)
