"""tests/swd_ref.py, the float64 restatement of the sliced Wasserstein distance, against what the REFERENCE's own swd.py returned
(tests/golden/swd_cases.npz, made by tests/golden/make_golden_swd.py), with the draws of deepliif_amd.stat.swd_draws under the recorded seed;
and the derivation of the bounds that tests/test_gpu_swd.py applies between the kernels and the restatement.

Tolerance against the reference: 10 x observed_rel, the largest relative difference seen when the fixture was made (1.6e-6).  The reference
computes in float32 and the order of its sums depends on the torch build and its thread count; a factor of ten covers that, and every
misreading below moves a result by more.  Were observed_rel above 1e-5, the restatement would be wrong, not the tolerance.

The GPU bounds (swd_ref.error_bounds, derived in its docstring from the data: sorting is 1-Lipschitz in the sup norm, so a result moves by at
most 1e3 (max|d_a| + max|d_b|), and the per-element terms are the 25-tap filters, the division by the std and the 147-term dot product)
come to, at most over the six cases: raw patches 2.5e-14, normalised descriptors 1e-11, per-direction distances 2.5e-9, a level's value
2.5e-6 (of values between 180 and 1900: 1.4e-8 relative at most).  test_the_derived_bounds prints and pins them; the GPU test evaluates the
same function on each of its cases."""
import os
import re

import numpy as np
import pytest
import torch

import swd_cases as SC
import swd_ref as R
from golden_util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = load_npz(SC.GOLDEN)
TOL = 10.0 * float(Z['observed_rel'])
_memo = {}


def case(name):
    """(gt, pred, draws of stat.swd_draws under the recorded seed, n_pyramids, the reference's per-level results); computed once"""
    if name not in _memo:
        from deepliif_amd import stat as S
        n, h, w, n_pyramids, n_desc, n_rep, ppr, seed = (int(v) for v in Z[f'{name}/params'])
        gt, pred = SC.image_sets(name)
        torch.manual_seed(seed)
        dr = S.swd_draws(S.swd_level_shapes(h, w, n_pyramids), n_desc, n_rep, ppr)
        _memo[name] = (gt, pred, dr, n_pyramids, Z[f'{name}/reference'])
    return _memo[name]


def rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


# ---------------------------------------------------------------------------------------------------- the fixture
def test_the_fixture_is_what_it_says():
    assert [str(n) for n in Z['names']] == SC.NAMES and 0 < float(Z['observed_rel']) < 1e-5
    for name in SC.NAMES:
        c = SC.CASES[name]
        gt, pred = SC.image_sets(name)
        assert gt.shape == pred.shape == (c['n'], c['h'], c['w'], 3) and gt.dtype == np.uint8
        assert SC.checksum(gt, pred) == str(Z[f'{name}/sha256']), f'{name}: the regenerated images are not the ones the reference saw'
        p = [int(v) for v in Z[f'{name}/params']]
        assert p[:3] == [c['n'], c['h'], c['w']] and p[3] == SC.default_pyramids(c['h']) and 2 <= p[5] <= 8
        assert Z[f'{name}/reference'].shape == (p[3] + 1,)
        # no near-constant channel at any level of either set
        for imgs in (gt, pred):
            for lev in R.levels(imgs, p[3]):
                assert lev.std(axis=(0, 2, 3)).min() > 1e-3
    assert [int(v) for v in Z['1x16x16/params']][3] == 0 and [int(v) for v in Z['3x48x80/params']][3] == 2
    dr = case('3x48x80')[2]
    assert [len(i) for i in dr.indices] == [128, 128, 84]                      # the last level has 6 x 14 positions: all of them
    assert sorted(dr.indices[2].tolist()) == list(range(84))


# ---------------------------------------------------------------------------------------------------- draws
def test_swd_draws_are_the_references_draws_and_need_no_library():
    from deepliif_amd import stat as S
    shapes = S.swd_level_shapes(48, 80, 2)
    assert shapes == [(48, 80), (24, 40), (12, 20)] == SC.level_shapes(48, 80, 2)
    torch.manual_seed(5)
    a = S.swd_draws(shapes, 128, 3, 4)
    torch.manual_seed(5)
    b = R.draws(shapes, 128, 3, 4)
    g = torch.Generator().manual_seed(5)
    c = S.swd_draws(shapes, 128, 3, 4, generator=g)
    for l in range(3):
        assert a.indices[l].dtype == np.int64 and a.projections[l].dtype == np.float32 and a.projections[l].shape == (3, 147, 4)
        assert np.array_equal(a.indices[l], b.indices[l]) and np.array_equal(a.projections[l], b.projections[l])
        assert np.array_equal(a.indices[l], c.indices[l]) and np.array_equal(a.projections[l], c.projections[l])
        std = a.projections[l].astype(np.float64).std(axis=1, ddof=1)
        assert np.abs(std - 1).max() < 1e-6                                    # every direction renormalised, unbiased
    with pytest.raises(ValueError):
        S.swd_draws([(6, 20)])
    with pytest.raises(ValueError):
        S.swd_draws(shapes, proj_per_repeat=1)


# ---------------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize('name', SC.NAMES)
def test_swd_ref_reproduces_the_reference(name):
    gt, pred, dr, n_pyramids, want = case(name)
    got = R.swd(gt, pred, dr, n_pyramids)
    print(f'{name}: swd_ref {got} reference {want} rel {rel(got, want):.3e} (tolerance {TOL:.3e})')
    assert got.shape == want.shape and rel(got, want) <= TOL


MISREADINGS = {
    'biased_std': dict(biased=True),
    'index_column_row': dict(index_order='column'),
    'replicate_padding': dict(padding='replicate'),
    'bilinear_upsampling': dict(upsample='bilinear'),
    'joint_statistics': dict(joint_stats=True),
}


@pytest.mark.parametrize('which', list(MISREADINGS))
def test_a_misread_stage_leaves_the_tolerance(which):
    caught = []
    for name in SC.NAMES:
        gt, pred, dr, n_pyramids, want = case(name)
        r = rel(R.swd(gt, pred, dr, n_pyramids, **MISREADINGS[which]), want)
        print(f'{which} on {name}: rel {r:.3e}')
        if r > TOL:
            caught.append(name)
    assert caught, f'{which} reproduces every golden result within {TOL:.3e}'


@pytest.mark.parametrize('which', ['projections_not_renormalised', 'permutation_after_projections'])
def test_misread_draws_leave_the_tolerance(which):
    caught = []
    for name in SC.NAMES:
        gt, pred, dr, n_pyramids, want = case(name)
        n, h, w, _, n_desc, n_rep, ppr, seed = (int(v) for v in Z[f'{name}/params'])
        torch.manual_seed(seed)
        bad = R.draws(dr.level_shapes, n_desc, n_rep, ppr, renormalise=which != 'projections_not_renormalised',
                      permutation_first=which != 'permutation_after_projections')
        r = rel(R.swd(gt, pred, bad, n_pyramids), want)
        print(f'{which} on {name}: rel {r:.3e}')
        if r > TOL:
            caught.append(name)
    assert caught, f'{which} reproduces every golden result within {TOL:.3e}'


# ---------------------------------------------------------------------------------------------------- the bounds of the GPU test
def test_the_derived_bounds():
    """swd_ref.error_bounds on every case: the numbers of this module's docstring, far below the tolerance against the reference and far below what
    any misreading moves; a float32 evaluation of the descriptors leaves them"""
    worst = dict(raw=0.0, stats=0.0, norm=0.0, cols=0.0, value=0.0)
    for name in SC.NAMES:
        gt, pred, dr, n_pyramids, want = case(name)
        st = R.stages(gt, pred, dr, n_pyramids)
        b = R.error_bounds(st, n_pyramids)
        print(f'{name}: ' + ' '.join(f'{k} {v:.3e}' for k, v in b.items()) + f' smallest value {want.min():.1f}')
        for k in worst:
            worst[k] = max(worst[k], b[k])
        assert b['value'] / want.min() < TOL / 10                              # two orders inside the tolerance against the reference
        # the same stages from float32 descriptors: outside the bound, so the bound tells double from single precision
        l0 = st[0]
        c32 = R.column_distances(l0['norm_a'].astype(np.float32).astype(np.float64), l0['norm_b'].astype(np.float32).astype(np.float64), l0['dirs'])
        assert np.abs(c32 - l0['cols']).max() > b['cols']
    print('worst: ' + ' '.join(f'{k} {v:.3e}' for k, v in worst.items()))
    assert worst['raw'] <= 2.5e-14 and worst['norm'] <= 1e-11 and worst['cols'] <= 2.5e-9 and worst['value'] <= 2.5e-6
    assert worst['value'] >= 1e-9                                             # (and not vacuous the other way: the derivation did produce numbers)


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_swd_symbols_are_declared_bound_and_exported():
    from deepliif_amd import _lib as L
    import ctypes as C
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'deepliif_hip.h')).read(), flags=re.S)
    for half in ('bf16', 'fp16'):
        lib = L.load(half)
        for n in ('dl_swd_patches_ws_bytes', 'dl_swd_patches', 'dl_swd_normalise_ws_bytes', 'dl_swd_normalise', 'dl_swd_lds_rows', 'dl_swd_route',
                  'dl_swd_distance_ws_bytes', 'dl_swd_distance'):
            assert re.search(r'\b%s\s*\(' % n, header) and n in L.SIGNATURES and hasattr(lib, n)
    lib = L.load()
    rows = lib.dl_swd_lds_rows()
    assert rows >= 128 and rows & (rows - 1) == 0 and 2 * rows * 8 <= 160 * 1024                  # both sets at 8 bytes per value fit the CU's LDS
    assert lib.dl_swd_route(rows, 512, 0) == 1 and lib.dl_swd_route(rows + 1, 512, 0) == 2
    assert lib.dl_swd_route(rows + 1, 512, 1) == 0 and lib.dl_swd_route(100, 512, 2) == 2
    # decided on the host, before any launch (the pointers are never dereferenced)
    d = C.c_void_p(0x1000)
    counts = (C.c_int * 3)(128, 128, 84)
    assert lib.dl_swd_patches_ws_bytes(16, 512, 512, 5) >= 16 * 3 * 8 * (256 * 256 + 128 * 128) and lib.dl_swd_patches_ws_bytes(1, 48, 80, 5) == 0
    assert lib.dl_swd_patches_ws_bytes(32, 512, 512, 5) > lib.dl_swd_patches_ws_bytes(16, 512, 512, 5)
    assert lib.dl_swd_patches(d, 240, 11520, 3, 48, 80, 5, d, counts, 3, 0, d, d, None) != 0 and b'not divisible' in lib.dl_last_error()
    assert lib.dl_swd_patches(d, 240, 11520, 3, 48, 80, 3, d, counts, 3, 0, d, d, None) != 0 and b'below the 7 x 7' in lib.dl_last_error()
    counts[2] = 85
    assert lib.dl_swd_patches(d, 240, 11520, 3, 48, 80, 2, d, counts, 3, 0, d, d, None) != 0 and b'84 positions' in lib.dl_last_error()
    assert lib.dl_swd_distance(d, d, rows + 1, d, 8, 1, d, d, None) == -1 and b'LDS route' in lib.dl_last_error()
    assert lib.dl_swd_distance_ws_bytes(rows + 1, 8, 1) == 0 and lib.dl_swd_distance_ws_bytes(rows, 8, 1) > 0      # (the large route asks hipcub, on a GPU)
    assert lib.dl_swd_normalise(d, 0, d, d, None) != 0 and b'empty problem' in lib.dl_last_error()


def test_the_documents_no_longer_leave_swd_out():
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md', os.path.join('deepliif_amd', 'stat.py')):
        text = open(os.path.join(ROOT, doc)).read()
        assert not re.search(r'inception[- ]score,? and SWD|inception score, SWD|FID / inception / SWD', text), doc
        assert 'swd' in text.lower()
