"""What does the sliced Wasserstein distance (deepliif_amd/stat.py swd) cost on the GPU, where does the time go, and what does the host
yardstick (tests/swd_ref.py) cost for the same answer?  In ONE process, after a warm-up, `--rounds` windows with a device synchronise either
side (wall clock), medians reported:
    swd                     64 pairs of 512 x 512 RGB images with the defaults (6 levels, 128 x 4 = 512 directions, 128 descriptors): host arrays
                            in (upload included) and device tensors in, with the draws made once (swd_draws costs host time of its own, reported)
    stages                  the same call taken apart: dl_swd_patches of both sets, dl_swd_normalise of the 12 matrices, dl_swd_distance of the
                            6 levels (with the route the sort took), and the forced other route for comparison
    swd_ref                 the float64 numpy restatement on the host, ONCE -- that run is also the check of the GPU result against its bound
Writes <out> (default profiles/swd.json).

    python tools/swd_ab.py [--rounds 7] [--pairs 64] [--size 512] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--no-host', action='store_true', help='skip the swd_ref run (and with it the check)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'swd.json'))
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    import swd_cases as SC
    import swd_ref as R
    from deepliif_amd import stat as S

    med = statistics.median
    res = {'tool': 'tools/swd_ab.py', 'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'what': 'wall-clock seconds, medians over the rounds'}
    gt, pred = SC.image_sets(n=a.pairs, h=a.size, w=a.size, kind='mixed', seed=1)
    gd, pd = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
    n_pyramids = SC.default_pyramids(a.size)
    shapes = S.swd_level_shapes(a.size, a.size, n_pyramids)
    t_draws, dr = timed(lambda: S.swd_draws(shapes, generator=torch.Generator().manual_seed(1)))
    P = dr.n_repeat_projection * dr.proj_per_repeat
    got = S.swd(gd, pd, draws=dr, return_by_resolution=True)                  # warm-up
    from_host = [timed(lambda: S.swd(gt, pred, draws=dr))[0] for _ in range(a.rounds)]
    from_dev = [timed(lambda: S.swd(gd, pd, draws=dr))[0] for _ in range(a.rounds)]
    with_draws = [timed(lambda: S.swd(gd, pd))[0] for _ in range(a.rounds)]
    again = S.swd(gd, pd, draws=dr, return_by_resolution=True)

    # the stages of that call
    lib = S._lib()
    ta, tb = S._batch(gd, gd.device), S._batch(pd, pd.device)
    dirs = [S._swd_directions(p, gd.device) for p in dr.projections]
    t_patch, t_norm, t_dist, t_other = [], [], [], []
    rows = routes = None
    for _ in range(a.rounds):
        t, (pa, pb) = timed(lambda: (S._swd_patches(ta, n_pyramids, dr.indices), S._swd_patches(tb, n_pyramids, dr.indices)))
        t_patch.append(t)
        t_norm.append(timed(lambda: [S._swd_normalise(x) for x in pa + pb])[0])
        rows = [int(x.shape[0]) for x in pa]
        routes = [int(lib.dl_swd_route(r, P, 0)) for r in rows]
        t_dist.append(timed(lambda: [S._swd_distances(pa[l], pb[l], dirs[l]) for l in range(n_pyramids + 1)])[0])
        t_other.append(timed(lambda: [S._swd_distances(pa[l], pb[l], dirs[l], 3 - routes[l]) for l in range(n_pyramids + 1)
                                      if lib.dl_swd_route(rows[l], P, 3 - routes[l])])[0])
    names = {1: 'lds_bitonic', 2: 'global_hipcub_segmented_radix'}
    res['swd'] = {'pairs': a.pairs, 'size': [a.size, a.size, 3], 'levels': n_pyramids + 1, 'directions': P, 'rows_per_level': rows,
                  'sort_route_per_level': [names[r] for r in routes], 'lds_rows_limit': S.swd_lds_rows(),
                  'gpu_from_host_arrays_s': med(from_host), 'gpu_from_device_tensors_s': med(from_dev),
                  'gpu_from_device_tensors_with_draws_s': med(with_draws), 'swd_draws_host_s': t_draws,
                  'stage_patches_both_sets_s': med(t_patch), 'stage_normalise_all_s': med(t_norm), 'stage_project_sort_reduce_s': med(t_dist),
                  'stage_project_sort_reduce_other_route_s': med(t_other),
                  'bit_identical_repeat': bool(again.tobytes() == got.tobytes()), 'per_level': got.tolist(), 'value': float(got.mean()),
                  'all_from_host_s': from_host, 'all_from_device_s': from_dev}
    print(json.dumps(res['swd']), flush=True)

    if not a.no_host:
        t_host, st = timed(lambda: R.stages(gt, pred, dr, n_pyramids))
        want = np.array([s['value'] for s in st])
        bound = R.error_bounds(st, n_pyramids)['value']
        err = float(np.abs(got - want).max())
        assert err <= bound, f'swd differs from swd_ref by {err:.3e} (bound {bound:.3e})'
        res['swd'].update({'swd_ref_host_s': t_host, 'swd_ref_runs': 1, 'host_over_gpu_from_device': t_host / med(from_dev),
                           'max_abs_difference': err, 'derived_bound': bound})
        print(json.dumps({k: res['swd'][k] for k in ('swd_ref_host_s', 'host_over_gpu_from_device', 'max_abs_difference', 'derived_bound')}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({'written': a.out}))


if __name__ == '__main__':
    main()
