"""The sliced Wasserstein distance on the GPU (deepliif_amd/stat.py swd -> csrc/swd.hip: dl_swd_patches, dl_swd_normalise, dl_swd_distance) against
tests/swd_ref.py, stage by stage and as a whole, and against what the reference's own swd.py returned (tests/golden/swd_cases.npz).

Bounds between the kernels and swd_ref: swd_ref.error_bounds, derived in its docstring and pinned in tests/test_swd_ref_host.py (both sides work
in double; sorting is 1-Lipschitz, so a level's value moves by at most 1e3 (max|d_a| + max|d_b|)) -- evaluated on each case's own data, never
on what the kernels return.  Against the golden results: the host test's tolerance, 10 x observed_rel."""
import csv

import numpy as np
import pytest
import torch

import swd_cases as SC
import swd_ref as R
from deepliif_amd import ops
from deepliif_amd import stat as S
from golden_util import load_npz

pytestmark = pytest.mark.gpu
Z = load_npz(SC.GOLDEN)
TOL = 10.0 * float(Z['observed_rel'])
_memo = {}


@pytest.fixture(autouse=True)
def _real_backend():
    ops._impl = None
    yield


def prepared(key, gt, pred, n_pyramids, n_repeat, seed):
    """(gt, pred, draws, n_pyramids, swd_ref's stages, bounds): computed once per key and left unchanged"""
    if key not in _memo:
        dr = S.swd_draws(S.swd_level_shapes(gt.shape[1], gt.shape[2], n_pyramids), SC.N_DESCRIPTORS, n_repeat, SC.PROJ_PER_REPEAT,
                         generator=torch.Generator().manual_seed(seed))
        st = R.stages(gt, pred, dr, n_pyramids)
        _memo[key] = (gt, pred, dr, n_pyramids, st, R.error_bounds(st, n_pyramids))
    return _memo[key]


def case(name):
    n, h, w, n_pyramids, n_desc, n_rep, ppr, seed = (int(v) for v in Z[f'{name}/params'])
    if name not in _memo:
        gt, pred = SC.image_sets(name)
        torch.manual_seed(seed)                                               # the global generator, as the reference drew
        dr = S.swd_draws(S.swd_level_shapes(h, w, n_pyramids), n_desc, n_rep, ppr)
        st = R.stages(gt, pred, dr, n_pyramids)
        _memo[name] = (gt, pred, dr, n_pyramids, st, R.error_bounds(st, n_pyramids))
    return _memo[name]


def worst(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max())


def check_stages(gt, pred, dr, n_pyramids, st, b, route=0):
    """every stage of both sets against swd_ref, element by element -> the per-level values"""
    dev = torch.device('cuda')
    ta, tb = S._batch(gt, dev), S._batch(pred, dev)
    pa, pb = S._swd_patches(ta, n_pyramids, dr.indices), S._swd_patches(tb, n_pyramids, dr.indices)
    values = []
    for l, s in enumerate(st):
        for k, x in (('a', pa[l]), ('b', pb[l])):
            assert tuple(x.shape) == s['raw_' + k].shape and x.dtype == torch.float64
            e_raw = worst(x.cpu().numpy(), s['raw_' + k])
            stats = S._swd_normalise(x).cpu().numpy()
            e_stats = max(worst(stats[:3], s['stats_' + k][0]), worst(stats[3:], s['stats_' + k][1]))
            e_norm = worst(x.cpu().numpy(), s['norm_' + k])
            print(f'level {l} set {k}: raw {e_raw:.2e} (bound {b["raw"]:.2e}) stats {e_stats:.2e} ({b["stats"]:.2e}) norm {e_norm:.2e} ({b["norm"]:.2e})')
            assert e_raw <= b['raw'] and e_stats <= b['stats'] and e_norm <= b['norm']
        dirs = S._swd_directions(dr.projections[l], dev)
        cols = S._swd_distances(pa[l], pb[l], dirs, route).cpu().numpy()
        e_cols = worst(cols, s['cols'])
        print(f'level {l}: R {pa[l].shape[0]} route {S._lib().dl_swd_route(pa[l].shape[0], dirs.shape[0], route)} cols {e_cols:.2e} (bound {b["cols"]:.2e})')
        assert cols.shape == s['cols'].shape and e_cols <= b['cols']
        values.append(R.level_value(cols, dr.n_repeat_projection, dr.proj_per_repeat))
    return np.array(values)


# ---------------------------------------------------------------------------------------------------- stages and the whole, per case
@pytest.mark.parametrize('name', SC.NAMES)
def test_stages_and_result_against_swd_ref_and_the_reference(name):
    gt, pred, dr, n_pyramids, st, b = case(name)
    want = np.array([s['value'] for s in st])
    values = check_stages(gt, pred, dr, n_pyramids, st, b)
    assert worst(values, want) <= b['value']
    got = S.swd(gt, pred, n_pyramids=n_pyramids, draws=dr, return_by_resolution=True)
    golden = Z[f'{name}/reference']
    print(f'{name}: gpu {got} swd_ref {want} |diff| {np.abs(got - want)} (bound {b["value"]:.2e}) reference {golden}')
    assert got.dtype == np.float64 and got.shape == (n_pyramids + 1,)
    assert worst(got, want) <= b['value']
    assert float(np.max(np.abs(got - golden) / np.abs(golden))) <= TOL
    one = S.swd(gt, pred, draws=dr)                                           # n_pyramids by default, the mean over the levels
    assert isinstance(one, float) and one == float(got.mean())


def test_both_sort_routes_forced():
    gt, pred, dr, n_pyramids, st, b = case('3x48x80')
    assert [s['raw_a'].shape[0] for s in st] == [384, 384, 252]               # none a power of two
    want = np.array([s['value'] for s in st])
    for route in (1, 2):
        assert worst(check_stages(gt, pred, dr, n_pyramids, st, b, route), want) <= b['value']
        assert worst(S.swd(gt, pred, draws=dr, return_by_resolution=True, route=route), want) <= b['value']


def test_the_route_is_taken_by_size():
    lib = S._lib()
    rows = S.swd_lds_rows()
    n = rows // 128 + 1
    assert n == SC.CASES['65x32x32']['n']                                     # the fixture's large case is this one
    gt, pred, dr, n_pyramids, st, b = case('65x32x32')
    assert [s['raw_a'].shape[0] for s in st] == [n * 128, n * 100]
    assert lib.dl_swd_route(n * 128, 8, 0) == 2 and lib.dl_swd_route(n * 100, 8, 0) == 1
    assert lib.dl_swd_distance_ws_bytes(n * 128, 8, 0) >= 4 * n * 128 * 8 * 8 and lib.dl_swd_distance_ws_bytes(n * 128, 8, 1) == 0
    want = np.array([s['value'] for s in st])
    assert worst(S.swd(gt, pred, draws=dr, return_by_resolution=True), want) <= b['value']
    x = torch.zeros((n * 128, 147), dtype=torch.float64, device='cuda')
    with pytest.raises(Exception, match='LDS route'):
        S._swd_distances(x, x, torch.zeros((8, 147), device='cuda'), route=1)
    # the LDS route at exactly its limit: 64 of those images, 8192 rows at level 0
    g64, p64, dr64, _, st64, b64 = prepared('64x32x32', gt[:n - 1], pred[:n - 1], 1, 2, 64)
    assert st64[0]['raw_a'].shape[0] == rows and lib.dl_swd_route(rows, 8, 0) == 1
    check_stages(g64, p64, dr64, 1, st64, b64)


def test_identical_sets_give_exactly_zero_and_repeats_give_the_same_bits():
    gt, pred, dr, n_pyramids, _, _ = case('3x48x80')
    for route in (0, 2):
        z = S.swd(gt, gt.copy(), draws=dr, return_by_resolution=True, route=route)
        assert z.tolist() == [0.0] * (n_pyramids + 1)
    big, _, drb, _, _, _ = case('65x32x32')
    assert S.swd(big, big.copy(), draws=drb) == 0.0
    for g, p, d in ((gt, pred, dr), case('65x32x32')[:3]):
        r1, r2 = (S.swd(g, p, draws=d, return_by_resolution=True) for _ in range(2))
        assert r1.tobytes() == r2.tobytes() and r1.min() > 0


def test_a_seeded_default_call_equals_the_call_with_its_draws():
    gt, pred = SC.image_sets('2x64x64')
    torch.manual_seed(7)
    v1 = S.swd(gt, pred, n_repeat_projection=4, return_by_resolution=True)
    torch.manual_seed(7)
    dr = S.swd_draws(S.swd_level_shapes(64, 64, 2), 128, 4, 4)
    v2 = S.swd(gt, pred, draws=dr, return_by_resolution=True)
    v3 = S.swd(gt, pred, n_repeat_projection=4, return_by_resolution=True, generator=torch.Generator().manual_seed(7))
    assert v1.tobytes() == v2.tobytes() == v3.tobytes()
    assert S.swd(gt, pred, n_repeat_projection=4, return_by_resolution=True).tobytes() != v1.tobytes()      # the generator moved on
    with pytest.raises(ValueError, match='draws were made'):
        S.swd(gt, pred, n_pyramids=1, draws=dr)


def test_input_forms_agree():
    from PIL import Image
    gt, pred, dr, _, _, _ = case('3x48x80')
    want = S.swd(gt, pred, draws=dr, return_by_resolution=True)
    forms = {
        'lists': (list(gt), list(pred)),
        'pil': ([Image.fromarray(x) for x in gt], [Image.fromarray(x) for x in pred]),
        'cuda': (torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()),
        'mixed': (torch.from_numpy(gt).cuda(), pred),
    }
    for k, (a, b) in forms.items():
        assert S.swd(a, b, draws=dr, return_by_resolution=True).tobytes() == want.tobytes(), k
    # panel 1 of rows of three panels: views with the row's stride, not copied
    rng = np.random.RandomState(3)
    rows_a, rows_b = (torch.from_numpy(np.concatenate([rng.randint(0, 256, size=x.shape).astype(np.uint8), x, x[:, :, ::-1]], axis=2)).cuda()
                      for x in (gt, pred))
    a, b = rows_a[:, :, 80:160], rows_b[:, :, 80:160]
    assert not a.is_contiguous() and S._batch(a, a.device).data_ptr() == a.data_ptr()
    assert S.swd(a, b, draws=dr, return_by_resolution=True).tobytes() == want.tobytes()
    assert S.compute_swd(gt, pred) > 0


def test_512_with_the_default_five_pyramids():
    gt, pred = SC.image_sets(n=2, h=512, w=512, kind='mixed', seed=21)
    gt, pred, dr, n_pyramids, st, b = prepared('2x512x512', gt, pred, SC.default_pyramids(512), 4, 512)
    assert n_pyramids == 5 and [s['raw_a'].shape[0] for s in st] == [256] * 5 + [200]
    want = np.array([s['value'] for s in st])
    got = S.swd(gt, pred, n_repeat_projection=4, return_by_resolution=True, generator=torch.Generator().manual_seed(512))
    print(f'2x512x512: gpu {got} swd_ref {want} |diff| {np.abs(got - want)} (bound {b["value"]:.2e})')
    assert got.shape == (6,) and worst(got, want) <= b['value']
    check_stages(gt, pred, dr, n_pyramids, st, b)


def test_what_swd_refuses():
    z = np.zeros((2, 48, 80, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match='differ'):
        S.swd(z, z[:1])
    with pytest.raises(ValueError, match='differ'):
        S.swd(z, np.zeros((2, 48, 64, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match='gray'):
        S.swd([z[0, :, :, 0]], [z[1, :, :, 0]])
    with pytest.raises(ValueError, match='slice_size'):
        S.swd(z, z, slice_size=5)
    with pytest.raises(ValueError, match='divisible'):
        S.swd(z, z, n_pyramids=5)
    with pytest.raises(ValueError, match='below the 7 x 7'):
        S.swd(z[:, :32, :32], z[:, :32, :32], n_pyramids=3)
    with pytest.raises(ValueError, match='n_pyramids'):
        S.swd(z[:, :8, :8], z[:, :8, :8])


# ---------------------------------------------------------------------------------------------------- the directory driver
def read_csv(path):
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_compute_statistics_writes_the_swd_column(tmp_path):
    from PIL import Image
    gt_dir, model_dir = tmp_path / 'gt', tmp_path / 'model'
    gt_dir.mkdir()
    model_dir.mkdir()
    gt, pred = SC.image_sets('3x48x80')
    for i in range(3):
        Image.fromarray(gt[i]).save(gt_dir / f'img{i}_Hema.png')
        Image.fromarray(pred[i]).save(model_dir / f'img{i}_Hema.png')
    torch.manual_seed(9)
    info = S.compute_statistics(str(gt_dir), str(model_dir), str(tmp_path / 'with'), mode='ImageSynthesis', image_types=('Hema',), swd=True)
    torch.manual_seed(9)
    want = S.swd(list(gt), list(pred))
    head, rows = read_csv(tmp_path / 'with' / 'metrics_ImageSynthesis_DeepLIIF.csv')
    assert head == ['Model', 'Hema_MSE_avg', 'Hema_MSE_std', 'Hema_ssim_avg', 'Hema_ssim_std', 'Hema_swd_value']
    assert float(rows[0][5]) == want == info['Hema_swd_value'] and want > 0
    S.compute_statistics(str(gt_dir), str(model_dir), str(tmp_path / 'without'), mode='ImageSynthesis', image_types=('Hema',))
    head0, rows0 = read_csv(tmp_path / 'without' / 'metrics_ImageSynthesis_DeepLIIF.csv')
    assert head0 == head[:5] and rows0[0] == rows[0][:5]
    Image.fromarray(gt[0, :32, :32].copy()).save(gt_dir / 'img9_Hema.png')
    Image.fromarray(pred[0, :32, :32].copy()).save(model_dir / 'img9_Hema.png')
    with pytest.raises(ValueError, match='one set of one size'):
        S.compute_statistics(str(gt_dir), str(model_dir), str(tmp_path / 'mixed'), mode='ImageSynthesis', image_types=('Hema',), swd=True)
