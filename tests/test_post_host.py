"""Host-side arithmetic of deepliif_amd/postprocessing.py (no GPU): the default thresholds computed from the cell list / the marker
histogram must equal the reference's values (fixtures) and numpy's percentile."""
import os

import numpy as np
import pytest

from deepliif_amd import postprocessing as PP
from golden_util import load_npz

Z = load_npz(os.path.join(os.path.dirname(__file__), 'golden', 'post_cases.npz'))
NAMES = [str(n) for n in Z['names']]


@pytest.mark.parametrize('name', NAMES)
def test_default_thresholds_from_reference_cell_lists(name):
    kw = eval(str(Z[f'{name}/kwargs']))
    cells = Z[f'{name}/cells']
    assert PP.calculate_default_size_threshold(cells[:, 0], kw['resolution']) == int(Z[f'{name}/default_size_thresh'])
    want = int(Z[f'{name}/default_marker_thresh'])
    if want >= 0:
        gray = Z[f'{name}/marker'].max(axis=-1)
        hist = np.bincount(gray.ravel(), minlength=256)
        assert PP.calculate_default_marker_threshold(hist) == want


def test_percentile_from_histogram_is_numpys_percentile():
    rng = np.random.RandomState(0)
    for trial in range(300):
        n = int(rng.choice([1, 2, 3, 7, 100, 1001, 5000]))
        lo, hi = sorted(rng.randint(1, 256, size=2))
        v = rng.randint(lo, hi + 1, size=n).astype(np.uint8)
        hist = np.bincount(v, minlength=256)
        for q in (0.1, 99.9, 50.0, 25.0, 0.0, 100.0):
            assert PP.percentile_from_histogram(hist, q) == float(np.percentile(v, q)), (n, q)


def test_large_noise_threshold_table():
    assert [PP.calculate_large_noise_thresh('default', r) for r in ('10x', '20x', '40x')] == [1000, 4000, 16000]
    assert PP.calculate_large_noise_thresh(None, '40x') is None and PP.calculate_large_noise_thresh(123, '10x') == 123


def test_library_kde_is_the_reference_loop_bit_for_bit():
    """dl_pp_kde_first_minimum (host code in the library, libm exp) against the expression-by-expression Python loop of the pinned oracle:
    same threshold for random cell lists, and the float32 KDE itself identical in every bin."""
    import ctypes as C
    import math
    from deepliif_amd import _lib as L
    from oracle import postprocess_oracle as PO
    rng = np.random.RandomState(3)
    for trial in range(12):
        n = int(rng.choice([2, 3, 17, 200, 1500]))
        sizes = np.maximum(1, (rng.gamma(2.0, 40.0, size=n)).astype(np.int64))
        for res in ('40x', '20x', '10x'):
            assert PP.calculate_default_size_threshold(sizes, res) == PO.default_size_threshold(sizes, res)
    sizes = np.maximum(1, (rng.gamma(2.0, 40.0, size=300)).astype(np.int64))
    values = np.ascontiguousarray(np.sqrt(sizes), dtype=np.float64)
    kde = np.zeros(500, dtype=np.float32)
    step = C.c_double(0.0)
    L.load().dl_pp_kde_first_minimum(values.ctypes.data_as(C.c_void_p), 300, 500, C.byref(step), kde.ctypes.data_as(C.c_void_p))
    inv = 1 / math.sqrt(2 * math.pi)
    want = np.zeros(500, dtype=np.float32)
    st = (float(values.max()) + 1) / 500
    for i in range(500):
        x, total = i * st, 0
        for v in values:
            val = (x - v) * 1.0
            total += math.exp(-(val * val / 2)) * inv
        want[i] = total / (300 * 1.0)
    assert step.value == st and np.array_equal(kde.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('version', [3, 4, 5, 6])
@pytest.mark.parametrize('name', NAMES)
def test_cell_results_host_half_against_reference(name, version):
    """compute_cell_results (postprocessing.py:1136-1220) = GPU cell mapping + host-side boundary tracing / contour simplification / v4
    base-92 encoding.  The host half, fed with the pinned oracle's mapping, must reproduce what the reference returned (dicts for versions 3 / 5,
    encoded strings for 4 / 6) exactly."""
    from oracle import postprocess_oracle as PO
    kw = eval(str(Z[f'{name}/kwargs']))
    ckw = {k: kw[k] for k in ('seg_thresh', 'noise_thresh', 'large_noise_thresh') if k in kw}
    large = PO.large_noise_threshold(ckw.get('large_noise_thresh'), kw['resolution'])
    use_od = version >= 5
    mask, cells, defaults, _, _ = PO.cells_info(Z[f'{name}/seg'], Z[f'{name}/orig'] if use_od else Z[f'{name}/marker'], kw['resolution'],
                                                ckw.get('noise_thresh', 4), ckw.get('seg_thresh', 120), large, use_od)
    got = PP.cell_results_from_mapping(mask, cells, defaults, version, ckw.get('seg_thresh', 120), ckw.get('noise_thresh', 4), large)
    assert got == eval(str(Z[f'{name}/cell_results_v{version}']))


def test_base92_round_trip_and_padding():
    assert PP.to_base92(0) == '#' and PP.to_base92(91) == '~' and PP.to_base92(92) == '$#' and PP.to_base92(5, 2) == '#(' 
    assert PP.to_base92([1, 92 * 92]) == ['##$', '$##']
    for v in (0, 1, 91, 92, 8463, 778687, 12345678):
        assert PP.from_base92(PP.to_base92(v)) == v
