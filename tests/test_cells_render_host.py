"""Rendering stored cell data on the host: route='host' of postprocessing.cells_to_final_results against what the reference renders
(tests/golden/cells_render_cases.npz, bytes and scoring), and the lane functions of csrc/render.h (the kernels of dl_pp_render_count /
dl_pp_render_paint call them), run cell by cell on the CPU by csrc/render_check.cpp, against the rows and the owner map of the host route.
The GPU twin is test_gpu_cells_render.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cells_render_cases as RC
from deepliif_amd import _lib as L
from deepliif_amd import postprocessing as PP

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'deepliif_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
Z, E = RC.cell_lists(), RC.expected()
NAMES = [str(n) for n in E['names']]
HAND = RC.hand_lists()


def check_against(orig, got, code, scoring):
    overlay, refined = RC.images_from_code(orig, code)
    assert got[2] == scoring
    assert np.array_equal(got[0], overlay), 'overlay'
    assert np.array_equal(got[1], refined), 'refined'
    assert got[0].dtype == got[1].dtype == np.uint8


@pytest.mark.parametrize('version', [3, 4, 5, 6])
@pytest.mark.parametrize('name', NAMES)
def test_host_route_renders_what_the_reference_renders(name, version):
    orig = Z[f'{name}/orig']
    data = RC.stored(Z, name, version)
    sets = RC.threshold_sets([c['size'] for c in RC.stored(Z, name, 3)['cells']])
    assert len(sets) == RC.N_SETS
    for k, kw in enumerate(sets):
        want = E[f'{name}/{RC.pair(version)}/{k}/code'], eval(str(E[f'{name}/{RC.pair(version)}/{k}/scoring']))
        check_against(orig, PP.cells_to_final_results(data, orig, route='host', **kw), *want)
    # a slide-level list: the same picture with offset=
    want = E[f'{name}/{RC.pair(version)}/0/code'], eval(str(E[f'{name}/{RC.pair(version)}/0/scoring']))
    for off in RC.RENDER_OFFSETS:
        check_against(orig, PP.cells_to_final_results(RC.stored(Z, name, version, off), orig, route='host', offset=off), *want)


@pytest.mark.parametrize('version', [3, 4, 5, 6])
def test_host_route_skips_the_cells_the_window_cuts_off(version):
    h, w = RC.SKIP_WINDOW
    orig = np.ascontiguousarray(Z[f'{RC.SKIP_CASE}/orig'][:h, :w])
    data = RC.stored(Z, RC.SKIP_CASE, version, RC.SKIP_OFFSET)
    got = PP.cells_to_final_results(data, orig, size_thresh=None, route='host', offset=RC.SKIP_OFFSET, outside='skip')
    check_against(orig, got, E[f'skip/v{version}/code'], eval(str(E[f'skip/v{version}/scoring'])))
    with pytest.raises(ValueError, match=r'cell 0 of 8: an outline point lies outside the image'):
        PP.cells_to_final_results(data, orig, size_thresh=None, route='host', offset=RC.SKIP_OFFSET)


@pytest.mark.parametrize('name', list(HAND))
def test_host_route_on_the_hand_written_lists(name):
    data, kw = HAND[name]
    orig = RC.hand_orig()
    check_against(orig, PP.cells_to_final_results(data, orig, route='host', **kw), E[f'hand/{name}/code'], eval(str(E[f'hand/{name}/scoring'])))


def test_the_later_square_owns_the_shared_pixels():
    """what the two square lists are for: the outlines cross at (10, 6) and (6, 10); outline pixels end as fill (1 positive, 2 negative)"""
    for name, last in (('squares_pos_then_neg', 2), ('squares_neg_then_pos', 1)):
        assert E[f'hand/{name}/code'][6, 10] == E[f'hand/{name}/code'][10, 6] == last


# ------------------------------------------------------------------------------------------------ the lane functions on the CPU
def _build(tmp_path_factory, flags, what):
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not found')
    exe = str(tmp_path_factory.mktemp(what) / what)
    r = subprocess.run([HIPCC, '--cuda-host-only', '-O1', '-g', '-std=c++17', *flags, '-x', 'hip', os.path.join(CSRC, 'render_check.cpp'), '-o', exe],
                       capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    exe, r = _build(tmp_path_factory, [], 'render_check')
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope='module')
def sanitized_checker(tmp_path_factory):
    """the same program with the address and undefined-behaviour sanitizers in its HOST code; every cell's data is a separate allocation of
    exactly its size there, so a read past the end of a string is reported"""
    exe, r = _build(tmp_path_factory, ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all'], 'render_check_asan')
    if r.returncode != 0:
        # only a missing sanitizer RUNTIME is a reason to skip: the linker cannot find libclang_rt.asan / ubsan; anything else is a failure
        missing = [ln for ln in r.stderr.splitlines() if 'clang_rt' in ln and any(w in ln for w in ('cannot find', 'no such file', 'No such file', 'unable to find'))]
        if missing:
            pytest.skip('this toolchain cannot link the sanitizer runtime into a host program: ' + missing[0][:200])
        pytest.fail('render_check.cpp does not build under the sanitizers:\n' + r.stderr[-3000:])
    return exe


def thresholds(version, settings, **kw):
    args = dict(size_thresh='default', marker_thresh=None, size_thresh_upper=None, od_thresh_lower=None, od_thresh_upper=None)
    args.update(kw)
    return PP._render_thresholds(version, settings, **args)[1]


def run_lanes(exe, tmp_path, packed, th, offset, H, W):
    """-> (rows int32 [n][8], owner int32 [H][W]) from the count and paint lanes"""
    data, offsets, table = packed.host
    n = packed.n
    src, dst = tmp_path / 'in.bin', tmp_path / 'out.bin'
    hdr = np.array([H, W, n, offset[0], offset[1], packed.mode, 1 if packed.version in (5, 6) else 0, 0], dtype=np.int32)
    blob = hdr.tobytes() + bytes(th) + np.int64(data.shape[0]).tobytes() + offsets.astype(np.int64).tobytes() + np.ascontiguousarray(data).tobytes()
    if table is not None:
        blob += np.ascontiguousarray(table).tobytes()
    src.write_bytes(blob)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f'render_check exit {r.returncode}\n{r.stderr[-3000:]}'
    raw = dst.read_bytes()
    assert len(raw) == n * 32 + H * W * 4
    return np.frombuffer(raw[:n * 32], dtype=np.int32).reshape(n, 8), np.frombuffer(raw[n * 32:], dtype=np.int32).reshape(H, W)


@pytest.mark.parametrize('version', [3, 4, 5, 6])
@pytest.mark.parametrize('name', NAMES)
def test_lanes_equal_the_host_route(checker, tmp_path, name, version):
    """rows (status, class, extent, pixel count) and the owner map, both modes, thresholds that count every cell and that cut some out;
    without and with an offset"""
    H, W = Z[f'{name}/orig'].shape[:2]
    sets = RC.threshold_sets([c['size'] for c in RC.stored(Z, name, 3)['cells']])
    for off in [(0, 0)] + RC.RENDER_OFFSETS[:1]:
        packed = PP.pack_cells(RC.stored(Z, name, version, off), upload=False)
        for kw in sets[1:4]:
            th = thresholds(version, packed.settings, **kw)
            rows, owner = run_lanes(checker, tmp_path, packed, th, off, H, W)
            want_rows, want_owner = PP.render_rows_host(packed, th, off, H, W)
            assert np.array_equal(rows, want_rows) and np.array_equal(owner, want_owner)
            assert not rows[:, 0].any() and rows[:, 6].min() >= 1


def test_lanes_equal_the_host_route_on_the_hand_written_lists(checker, tmp_path):
    for name, (data, kw) in HAND.items():
        packed = PP.pack_cells(data, upload=False)
        th = thresholds(3, packed.settings, **kw)
        rows, owner = run_lanes(checker, tmp_path, packed, th, (0, 0), *RC.HAND_SHAPE)
        want_rows, want_owner = PP.render_rows_host(packed, th, (0, 0), *RC.HAND_SHAPE)
        assert np.array_equal(rows, want_rows) and np.array_equal(owner, want_owner), name
    assert rows[:, 6].tolist() == [32, 1, 32, 8, 16, 26]          # 'everything': 4 * 8 pixels, 1, 2 * 4, 4 * 4, 2 * 7 + 2 * 6


def test_versions_3_and_4_of_the_same_cells_pack_to_the_same_classification():
    for name in NAMES[:3]:
        H, W = Z[f'{name}/orig'].shape[:2]
        for a, b in ((3, 4), (5, 6)):
            pa, pb = PP.pack_cells(RC.stored(Z, name, a), upload=False), PP.pack_cells(RC.stored(Z, name, b), upload=False)
            assert (pa.mode, pb.mode, pa.n) == (0, 1, pb.n) and pa.host[2].shape == (pa.n, 4) and pb.host[2] is None
            assert pa.host[0].dtype == np.int32 and pb.host[0].dtype == np.uint8 and pa.host[1].dtype == pb.host[1].dtype == np.int64
            for kw in RC.threshold_sets([c['size'] for c in RC.stored(Z, name, 3)['cells']]):
                ra = PP.render_rows_host(pa, thresholds(a, pa.settings, **kw), (0, 0), H, W, paint=False)[0]
                rb = PP.render_rows_host(pb, thresholds(b, pb.settings, **kw), (0, 0), H, W, paint=False)[0]
                assert np.array_equal(ra, rb)


# ------------------------------------------------------------------------------------------------ refusals
W24 = 24
GOOD_V3 = RC.hand_lists()['squares_pos_then_neg'][0]['cells'][0]
GOOD_V4 = PP.encode_cell_data_v4(GOOD_V3)
HEAD_V4 = 1 + 1 + 2 + 2 * 1 + 6 * 1          # lengths byte, size 81 (1 digit), class, top-left pair, six one-digit offsets
SETTINGS = RC.hand_lists()['squares_pos_then_neg'][0]['settings']


def refusal_lists():
    """(name, version-3 or -4 data, expected statuses)"""
    prefixes = [GOOD_V4[:k] for k in range(len(GOOD_V4))]
    bad_cell = dict(GOOD_V3, boundary=[(0, 0), (1, 2)])
    out_cell = dict(GOOD_V3, boundary=[(20, 2), (W24, 2), (W24, 6), (20, 6)])
    small_bad, small_out = dict(bad_cell, size=0), dict(out_cell, size=0)          # not counted: size > 0 fails
    return [
        ('prefixes', {'cells': prefixes + [GOOD_V4], 'settings': SETTINGS, 'dataVersion': 4}, None),
        ('bytes', {'cells': [GOOD_V4[:-1] + chr(34), GOOD_V4[:3] + chr(127) + GOOD_V4[4:], chr(34) + GOOD_V4[1:], GOOD_V4 + chr(200), GOOD_V4],
                   'settings': SETTINGS, 'dataVersion': 4}, [1, 1, 1, 1, 0]),
        ('points', {'cells': [GOOD_V3, bad_cell, out_cell, small_bad, small_out, dict(GOOD_V3, boundary=[(-1, 5)]), dict(GOOD_V3, boundary=[(3, W24)])],
                    'settings': SETTINGS, 'dataVersion': 3}, [0, 2, 3, 2, 3, 3, 3]),
    ]


@pytest.mark.parametrize('which', ['render_check', 'render_check_asan'])
def test_refused_cells_have_a_status_and_are_not_painted(which, request, tmp_path):
    exe = request.getfixturevalue('checker' if which == 'render_check' else 'sanitized_checker')
    for name, data, statuses in refusal_lists():
        packed = PP.pack_cells(data, upload=False)
        th = thresholds(data['dataVersion'], SETTINGS)
        rows, owner = run_lanes(exe, tmp_path, packed, th, (0, 0), W24, W24)
        want_rows, want_owner = PP.render_rows_host(packed, th, (0, 0), W24, W24)
        assert np.array_equal(rows, want_rows) and np.array_equal(owner, want_owner), name
        if statuses is not None:
            assert rows[:, 0].tolist() == statuses, name
        else:
            # a proper prefix is malformed while its numbers are incomplete; after that it is a shorter legal cell (its closing vector may
            # be no pixel direction: BAD_SEGMENT, never a read past its end)
            lens = np.diff(packed.host[1])
            assert ((rows[:, 0] == PP.RENDER_MALFORMED) == (lens < HEAD_V4)).all()
            assert rows[-1].tolist() == [0, 1, 2, 2, 10, 10, 32, 0]
            assert set(rows[lens >= HEAD_V4, 0].tolist()) <= {PP.RENDER_OK, PP.RENDER_BAD_SEGMENT}
        painted = set(np.unique(owner).tolist()) - {-1}          # (a later cell may cover an earlier one completely)
        allowed = np.flatnonzero((rows[:, 0] == 0) & (rows[:, 1] != 0)).tolist()
        assert painted <= set(allowed) and allowed[-1] in painted, name


def test_an_empty_outline_and_a_range_outside_the_data_are_malformed(checker, tmp_path):
    packed = PP.pack_cells({'cells': [GOOD_V3, dict(GOOD_V3, boundary=[]), GOOD_V3], 'settings': SETTINGS, 'dataVersion': 3}, upload=False)
    th = thresholds(3, SETTINGS)
    assert run_lanes(checker, tmp_path, packed, th, (0, 0), W24, W24)[0][:, 0].tolist() == [0, 1, 0]
    packed.host[1][-1] += 5          # the last cell claims five vertices more than there are
    assert run_lanes(checker, tmp_path, packed, th, (0, 0), W24, W24)[0][:, 0].tolist() == [0, 1, 1]


def test_python_layer_raises_for_counted_cells_only():
    orig = RC.hand_orig()
    _, bytes_data, _ = refusal_lists()[1]
    with pytest.raises(ValueError, match=r'cell 0 of 5: the stored cell is malformed'):
        PP.cells_to_final_results(bytes_data, orig, route='host')
    cells = refusal_lists()[2][1]['cells']
    good, bad_cell, out_cell, small_bad, small_out = cells[:5]
    mk = lambda *c: {'cells': list(c), 'settings': SETTINGS, 'dataVersion': 3}
    with pytest.raises(ValueError, match=r'cell 1 of 2: two consecutive outline points'):
        PP.cells_to_final_results(mk(good, bad_cell), orig, route='host')
    with pytest.raises(ValueError, match=r'cell 2 of 3: an outline point lies outside the image'):
        PP.cells_to_final_results(mk(good, small_out, out_cell), orig, route='host')
    with pytest.raises(ValueError, match=r'cell 1 of 2: two consecutive outline points'):
        PP.cells_to_final_results(mk(good, bad_cell), orig, route='host', outside='skip')          # 'skip' is about the window only
    # uncounted cells are never rasterised: the picture and the counts are those of the good cell alone
    want = PP.cells_to_final_results(mk(good), orig, route='host')
    got = PP.cells_to_final_results(mk(small_bad, good, small_out), orig, route='host')
    assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = PP.cells_to_final_results(mk(good, out_cell), orig, route='host', outside='skip')
    assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError):
        PP.cells_to_final_results(mk(good), orig, route='cpu')
    with pytest.raises(ValueError):
        PP.cells_to_final_results(mk(good), orig, route='host', outside='clip')
    with pytest.raises(ValueError, match='cell 1 of 2'):
        PP.pack_cells({'cells': [GOOD_V4, GOOD_V4 + chr(300)], 'settings': SETTINGS, 'dataVersion': 4}, upload=False)


def test_no_cells_and_no_counted_cells():
    orig = RC.hand_orig()
    for data, kw in (({'cells': [], 'settings': SETTINGS, 'dataVersion': 3}, {}), ({'cells': [], 'settings': SETTINGS, 'dataVersion': 4}, {}),
                     (HAND['everything'][0], dict(size_thresh=50, size_thresh_upper=60))):
        overlay, refined, scoring = PP.cells_to_final_results(data, orig, route='host', **kw)
        assert np.array_equal(overlay, orig) and not refined.any()
        assert (scoring['num_total'], scoring['num_pos'], scoring['num_neg'], scoring['percent_pos']) == (0, 0, 0, 0)


def test_the_abi_carries_the_render_entries(monkeypatch):
    lib = L.load()
    for name in ('dl_pp_render_count', 'dl_pp_render_paint', 'dl_pp_render_ws_bytes', 'dl_pp_render_finish'):
        assert name in L.SIGNATURES and hasattr(lib, name)
    import ctypes
    assert ctypes.sizeof(L.RenderThresh) == 56
    # the workspace of the finish: two int32 maps and two byte masks, rounded up to 256 bytes each (10 bytes per pixel)
    for H, W in ((1, 37), (300, 300), (8192, 8192)):
        up = lambda v: (v + 255) // 256 * 256
        assert lib.dl_pp_render_ws_bytes(H, W) == 2 * up(4 * H * W) + 2 * up(H * W)
    assert lib.dl_pp_render_ws_bytes(0, 5) == 0 and lib.dl_pp_render_ws_bytes(1 << 16, 1 << 16) == 0
    # a library built before an entry existed is refused by name, not with a bare AttributeError
    monkeypatch.setattr(L, '_libs', {})
    monkeypatch.setitem(L.SIGNATURES, 'dl_pp_not_there_yet', (None, []))
    with pytest.raises(L.HipLibraryError, match='does not export dl_pp_not_there_yet'):
        L.load()
