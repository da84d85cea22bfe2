"""The host side of the weight-gradient dispatch against a recorded snapshot (the library loads without a GPU; nothing here launches anything).

wgrad_route() in csrc/wgrad.hip is the one place that chooses among the kernels of dl_conv_wgrad; dl_wgrad_plan, dl_conv_wgrad_deferrable and
dl_wgrad_route_info report that choice and ops.HipBackend.conv_wgrad / wgrad_takes_split / wgrad_c4_applies act on it.  tests/golden/wgrad_routing.json holds
the library's answers and what conv_wgrad does with them over the grid of tests/wgrad_routing_cases.py, and over a thinner grid under each documented runtime
switch that steers the weight gradient.  The snapshot is recorded from the commit BEFORE a change to the dispatch (see the case module), so a change that
means to keep the routing must reproduce every row.  While it collects a row the case module also asserts that dl_wgrad_route_info agrees with dl_wgrad_plan
and dl_conv_wgrad_deferrable, and that conv_wgrad asks the library no more than three questions in front of a launch."""
import os
import re

import pytest

import wgrad_routing_cases as R
from deepliif_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = ('names / return values / entry points', 'tiles, K steps, slab sizes, split-K', 'descriptor bytes')


def route_table_names():
    """the names of g_wgrad_routes, the table of the WgradRoute enum (csrc/wgrad.hip); the dev-only variants are leaves of their kernel's row and report its name"""
    with open(os.path.join(ROOT, 'deepliif_amd', 'csrc', 'wgrad.hip')) as f:
        src = f.read()
    table = src[src.index('g_wgrad_routes[] = {'):]
    table = table[:table.index('};')]
    return re.findall(r'^\s*\{"([^"]+)",', table, flags=re.M)


@pytest.fixture(scope='module')
def fixture():
    return R.load_fixture()


def _mismatches(fx, encoded, got):
    want = R.decode(fx, encoded)
    assert len(want) == len(got), f'the grid has {len(got)} rows, the fixture {len(want)}: the grid changed -- record the fixture again from the parent commit'
    bad = []
    for (key, *now), rec in zip(got, want):
        for part, a, b in zip(PARTS, now, rec):
            if a != b:
                bad.append(f'{R.describe(key)}: {part}: {a}, recorded {b}')
    return bad


def test_every_row_of_the_grid_routes_as_recorded(fixture):
    assert L.DL_VERSION == fixture['library_version']
    bad = _mismatches(fixture, fixture['main'], R.answers(L.load(), R.main_rows()))
    assert not bad, f'{len(bad)} differences from the snapshot, the first of them:\n' + '\n'.join(bad[:20])


@pytest.mark.parametrize('setting', R.SWITCH_SETTINGS)
def test_every_row_routes_as_recorded_under_the_switch(fixture, setting):
    lib = L.load()
    with R.switch_setting(lib, setting):
        got = R.answers(lib, R.switch_rows())
    assert setting.split('=')[0] not in os.environ          # (the setting is gone again)
    bad = _mismatches(fixture, fixture['switches'][setting], got)
    assert not bad, f'{setting}: {len(bad)} differences from the snapshot, the first of them:\n' + '\n'.join(bad[:20])


def test_the_switches_change_something(fixture):
    """each setting moves at least one row of the thinner grid off its default answer: the switch rows are not a second copy of the main ones"""
    default = [tuple(g[1:]) for g in R.answers(L.load(), R.switch_rows())]
    for setting in R.SWITCH_SETTINGS:
        rec = R.decode(fixture, fixture['switches'][setting])
        assert len(rec) == len(default) and rec != default, setting


def test_the_fixture_reaches_every_route_entry_point_and_answer(fixture):
    names = route_table_names()
    assert len(names) == 8 and len(set(names)) == 7, names          # (the two 7x7 forms, bf16 and strict, report one name)
    rows = list(zip((k for k, _ in R.main_rows()), R.decode(fixture, fixture['main'])))
    assert len(rows) > 30000
    reached = {cat[3 * i + 1] for _, (cat, _, _) in rows for i in range(len(R.PLAN_SPLITKS))}
    assert reached == set(names), f'never reached: {sorted(set(names) - reached)}; not in the table: {sorted(reached - set(names))}'
    # both 7x7 forms (stem: P wide, head: P small) of both kernels (bf16, strict)
    c4 = {(key[0], key[2]) for key, (cat, _, _) in rows if cat[3 * R.PLAN_SPLITKS.index(512) + 1] == 'wgrad_c4'}
    assert c4 == {(layer, pol) for layer in ('resnet.stem[zero]', 'resnet.head[zero]', 'resnet.head.narrow[zero]/c4') for pol in ('bf16', 'strict')}, sorted(c4)
    # ... and conv_wgrad hands them the split-K they need: the immediate entry point even inside a pass, with 512 parts
    auto_in_pass = R.CALLS.index((None, True))
    assert all(cat[R.COL_ENTRY0 + auto_in_pass] == 'dl_conv_wgrad' and num[3 * len(R.PLAN_SPLITKS) + 2 * auto_in_pass] == L.WGRAD_C4_PARTS
               for key, (cat, num, _) in rows if (key[0], key[2]) in c4 and cat[R.COL_C4] and cat[R.COL_ENTRY0] != 'error')
    entries = {cat[R.COL_ENTRY0 + i] for _, (cat, _, _) in rows for i in range(len(R.CALLS))}
    assert entries == {'dl_conv_wgrad', 'dl_conv_wgrad_slabs', 'dl_conv_wgrad_multi', 'error'}, entries
    assert {cat[R.COL_TAKES_SPLIT] for _, (cat, _, _) in rows} == {False, True} and {cat[R.COL_C4] for _, (cat, _, _) in rows} == {False, True}
    assert sum(1 for _, (cat, num, _) in rows if num[R.COL_TILES] > 0) >= 16 and sum(1 for _, (cat, _, _) in rows if cat[0] == 1) >= 16      # tiles; a batched form
