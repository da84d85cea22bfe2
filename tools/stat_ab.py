"""What does model evaluation (deepliif_amd/stat.py) cost on the GPU, and what does the host yardstick (tests/stat_ref.py) cost for the same
answers?  In ONE process, after a warm-up, `--rounds` windows with a device synchronise either side (wall clock), medians reported:
    image_similarity        64 pairs of 512 x 512 RGB images: host arrays in (upload included) and device tensors in
    segmentation_metrics    aji=True on one 512 x 512 mask pair with about 400 synthetic cells (discs of both classes, the prediction a shifted
                            copy): host arrays in and device tensors in
    stat_ref                the same two calls on the host, numpy / scipy in float64; the AJI the reference's slow way (one mask per component,
                            a logical_and per pair), so it runs ONCE -- that run is also the equality check of the GPU results
Writes <out> (default profiles/stat.json).

    python tools/stat_ab.py [--rounds 7] [--pairs 64] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def image_pairs(n, size, seed=0):
    """blurred blob images against noisy copies: SSIM values spread between 0.5 and 1"""
    import numpy as np
    from scipy import ndimage
    rng = np.random.RandomState(seed)
    gts, preds = [], []
    for i in range(n):
        f = ndimage.gaussian_filter(rng.rand(size, size, 3), (4.0, 4.0, 0))
        f = (f - f.min()) / (f.max() - f.min())
        a = (f * 255).astype(np.uint8)
        amp = 2 + 3 * (i % 8)
        gts.append(a)
        preds.append(np.clip(a.astype(np.int64) + rng.randint(-amp, amp + 1, size=a.shape), 0, 255).astype(np.uint8))
    return gts, preds


def cell_masks(size, n_cells, seed=0):
    """RGB mask pair: discs of radius 4 .. 9, red (positive) or blue (negative), some touching; the prediction is the ground truth moved by (3, -2)"""
    import numpy as np
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    gt = np.zeros((size, size, 3), dtype=np.uint8)
    for _ in range(n_cells):
        cy, cx, r = rng.randint(0, size), rng.randint(0, size), rng.uniform(4.0, 9.0)
        inside = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        c = 0 if rng.rand() < 0.45 else 2
        gt[..., c][inside] = 255
        gt[..., 2 - c][inside] = 0
    return gt, np.roll(np.roll(gt, 3, axis=0), -2, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--cells', type=int, default=400)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stat.json'))
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    import stat_ref as R
    from deepliif_amd import stat as S

    res = {'tool': 'tools/stat_ab.py', 'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'what': 'wall-clock seconds, medians over the rounds'}

    gts, preds = image_pairs(a.pairs, a.size)
    gd, pd = torch.from_numpy(np.stack(gts)).cuda(), torch.from_numpy(np.stack(preds)).cuda()
    got = S.image_similarity(gd, pd)                                          # warm-up
    t_host, want = timed(lambda: R.image_similarity(gts, preds))
    err = max(float(np.abs(got[k] - want[k]).max()) for k in ('mse', 'ssim'))
    assert err <= 1e-9, f'image_similarity differs from stat_ref by {err:.3e}'
    from_host = [timed(lambda: S.image_similarity(gts, preds))[0] for _ in range(a.rounds)]
    from_dev = [timed(lambda: S.image_similarity(gd, pd))[0] for _ in range(a.rounds)]
    again = S.image_similarity(gd, pd)
    res['image_similarity'] = {'pairs': a.pairs, 'size': [a.size, a.size, 3], 'gpu_from_host_arrays_s': statistics.median(from_host),
                               'gpu_from_device_tensors_s': statistics.median(from_dev), 'stat_ref_host_s': t_host, 'stat_ref_runs': 1,
                               'host_over_gpu_from_device': t_host / statistics.median(from_dev), 'max_abs_difference': err,
                               'bit_identical_repeat': bool(again['ssim'].tobytes() == got['ssim'].tobytes() and again['mse'].tobytes() == got['mse'].tobytes()),
                               'ssim_range': [float(got['ssim'].min()), float(got['ssim'].max())], 'all_from_host_s': from_host, 'all_from_device_s': from_dev}
    print(json.dumps(res['image_similarity']), flush=True)

    gt, pred = cell_masks(a.size, a.cells)
    gt_d, pred_d = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
    got = S.segmentation_metrics(gt_d, pred_d, aji=True)                      # warm-up
    t_host, want = timed(lambda: R.segmentation_metrics([gt], [pred], aji=True))
    assert got[0] == want[0] and dict(got[1]) == dict(want[1]), 'segmentation_metrics differs from stat_ref'
    from_host = [timed(lambda: S.segmentation_metrics(gt, pred, aji=True))[0] for _ in range(a.rounds)]
    from_dev = [timed(lambda: S.segmentation_metrics(gt_d, pred_d, aji=True))[0] for _ in range(a.rounds)]
    no_aji = [timed(lambda: S.segmentation_metrics(gt_d, pred_d))[0] for _ in range(a.rounds)]
    comps = {c: [int(R.label((m[..., c] > 0).astype(np.uint8))[1]) for m in (gt, pred)] for c in (0, 2)}
    res['segmentation_metrics_aji'] = {'size': [a.size, a.size, 3], 'discs': a.cells, 'components_gt_pred': {'positive': comps[0], 'negative': comps[2]},
                                       'gpu_from_host_arrays_s': statistics.median(from_host), 'gpu_from_device_tensors_s': statistics.median(from_dev),
                                       'gpu_without_aji_from_device_s': statistics.median(no_aji), 'stat_ref_host_s': t_host, 'stat_ref_runs': 1,
                                       'host_over_gpu_from_device': t_host / statistics.median(from_dev), 'equal_to_stat_ref': True,
                                       'AJI': got[1]['AJI'], 'Dice': got[1]['Dice'], 'all_from_host_s': from_host, 'all_from_device_s': from_dev}
    print(json.dumps(res['segmentation_metrics_aji']), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({'written': a.out}))


if __name__ == '__main__':
    main()
