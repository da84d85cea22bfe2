"""The weight-gradient kernels (csrc/wgrad.hip, wgrad_x3.h, wgrad_c4.h, wgrad_w4.h) against a float64 reference, PER ELEMENT, under the derived bound of
tests/wgrad_ref.py at slack 1.  The rows are tests/wgrad_cases.py: the smallest shapes that still reach each kernel and each edge (a per-element bound is only
sharp at small K: its summation term grows like K^2 against one pixel's contribution); tests/test_wgrad_ref_host.py proves on the CPU that the bound rejects
the faults this file exists for.

Every launch goes through ops.impl().conv_wgrad (the narrow head through shift_stack + stack_kw, the c4 rows through the automatic path); the batched form of the
direct-to-LDS kernels through ctypes (dl_conv_wgrad_multi + dl_wgrad_reduce_batch, pointer arrays and entries as ops.HipBackend._launch_queued builds them: ops.py
queues only w4 layers, so nothing else reaches blockIdx.z of those kernels).  The kernel name dl_wgrad_plan gives for the launched descriptor is asserted against the
table.  Every launch runs with accumulate = False (onto a buffer of 7.0: the store overwrites) and True (onto g0 ~ N(0, 1), which is in the bound).

The worst err / bound of every launch is printed and written to parity_errors_wgrad.json in the directory $DL_PARITY_DIR names (default parity_out/); a copy of
the MI355X run is kept as profiles/wgrad_parity/parity_errors_wgrad.json.  DL_TEST_DRYRUN=1 runs the file on the CPU with wgrad_ref.emulate in the kernel's place."""
import ctypes as C
import json
import os

import pytest
import torch

import wgrad_cases as WC
import wgrad_ref as WR
from deepliif_amd import _lib as L
from deepliif_amd import ops
from deepliif_amd._lib import WGRAD_C4_PARTS

from test_gpu_kernels import DEV, DRY, _split_copy, hip, sync

pytestmark = pytest.mark.gpu
ERRLOG = {}
ERRLOG_DIR = os.environ.get('DL_PARITY_DIR', 'parity_out')
_CACHE = {}


@pytest.fixture(autouse=True)
def _real_backend_again():
    yield
    ops._impl = None


@pytest.fixture(autouse=True, scope='module')
def _errlog():
    yield
    os.makedirs(ERRLOG_DIR, exist_ok=True)
    with open(os.path.join(ERRLOG_DIR, 'parity_errors_wgrad.json'), 'w') as f:
        json.dump(ERRLOG, f, indent=1, sort_keys=True)


def _case(row, policy):
    """(inputs, (ref, S, K)) of a (row, policy): computed once, shared, never modified"""
    key = (row.id, policy)
    if key not in _CACHE:
        data = WR.inputs(row, policy)
        _CACHE[key] = (data, WR.reference(row, data[0], data[1], policy))
    return _CACHE[key]


def _lib():
    try:
        return L.load('bf16')
    except L.HipLibraryError:
        assert DRY, 'the library is not built'
        return None


def _dev(t, policy):
    return t.to(WR.storage_dtype(policy)).to(DEV)


def _operands(be, row, policy, x, dy):
    """(P, Q) on the device in the policy's storage type, as engine.conv()'s backward builds them (the stacked head through the backend's shift_stack)"""
    d = WR.descriptor_of(row)
    t = {'x': _dev(x, policy), 'dy': _dev(dy, policy)}
    P, Q = t[d.p_role], t[d.q_role]
    if d.stack_kw:
        D = torch.empty(P.shape[:3] + (WR.cpad(row.cout * d.stack_kw),), dtype=P.dtype, device=P.device)
        be.shift_stack(P, row.cout, d.stack_kw, d.pad, D)
        P = D
    return P, Q


def _assert_name(row, policy, splitk, P, Q, tag, **kw):
    lib = _lib()
    if lib is None:
        return
    sk = WGRAD_C4_PARTS if row.form == 'c4' else WR.effective_splitk(row, policy, splitk, P, Q)
    w = WR.wgrad_desc(row, policy, sk, tuple(P.shape), tuple(Q.shape), p_pstride=P.stride(2), q_pstride=Q.stride(2), **kw)
    rc, _, _, name = WR.plan(lib, w)
    assert rc >= 0 and name == row.kernel, f'{tag}: dl_wgrad_plan routes to {name}, the table says {row.kernel}'
    return rc


def _launch(be, row, policy, splitk, P, Q, grad, accumulate, data, **kw):
    d = WR.descriptor_of(row)
    if DRY:
        got = WR.emulate(row, policy, splitk, accumulate, None, (data[0], data[1], grad.clone()))
        grad.copy_(got)
        return
    be.conv_wgrad(P, Q, grad, d.k, d.step, d.pad, d.pad_mode, d.p_act, d.q_act, WR.prec_of(policy), accumulate, splitk=splitk, stack_kw=d.stack_kw, **kw)


def _start(g0, accumulate):
    return g0.clone().to(DEV) if accumulate else torch.full_like(g0, 7.0).to(DEV)


def _check(tag, row, policy, grad, g0, accumulate, cbp):
    _, (ref, S, K) = _case(row, policy)
    want = ref + g0.double() if accumulate else ref
    worst, report = WR.compare(grad, want, WR.bound(ref, S, K, policy, g0 if accumulate else None), WR.descriptor_of(row), cbp)
    ERRLOG[tag] = worst
    print(f'{tag}: worst err/bound {worst:.4f}')
    assert worst <= 1.0 and not report, f'{tag}\n{report}'


@pytest.mark.parametrize('launch', WC.ALL_LAUNCHES, ids=WC.launch_id)
def test_bf16_library(launch):
    row, policy, splitk = launch
    be = hip()
    data, _ = _case(row, policy)
    x, dy, g0 = data
    P, Q = _operands(be, row, policy, x, dy)
    twice = 'twice' in row.extras and (policy, splitk) == WC.launches(row)[0]
    for accumulate in (False, True):
        tag = f'{WC.launch_id(launch)}/{"acc" if accumulate else "store"}'
        _assert_name(row, policy, splitk, P, Q, tag)
        grad = _start(g0, accumulate)
        _launch(be, row, policy, splitk, P, Q, grad, accumulate, data)
        sync()
        _check(tag, row, policy, grad, g0, accumulate, Q.shape[3])
        if twice:
            again = _start(g0, accumulate)
            _launch(be, row, policy, splitk, P, Q, again, accumulate, data)
            sync()
            assert torch.equal(grad, again), f'{tag}: run-to-run difference'


def test_one_row_per_kernel_runs_twice():
    assert {r.kernel.split('<')[0] for r in WC.ROWS if 'twice' in r.extras} == {r.kernel.split('<')[0] for r in WC.ROWS}


SLICE = [(r, pol, sk) for r in WC.ROWS if 'slice' in r.extras for pol, sk in WC.launches(r)]


@pytest.mark.parametrize('launch', SLICE, ids=WC.launch_id)
def test_channel_slice_operands(launch):
    """P and Q are channel slices of buffers twice as wide (p_pstride = 2 CAp, q_pstride = 2 CBp); the other half holds 7.0.  Same arithmetic in the same order: in
    bound, and the bits of the dense launch"""
    row, policy, splitk = launch
    be = hip()
    data, _ = _case(row, policy)
    x, dy, g0 = data
    P, Q = _operands(be, row, policy, x, dy)
    Pw = torch.full(P.shape[:3] + (2 * P.shape[3],), 7.0, dtype=P.dtype, device=P.device)
    Qw = torch.full(Q.shape[:3] + (2 * Q.shape[3],), 7.0, dtype=Q.dtype, device=Q.device)
    Ps, Qs = Pw[..., P.shape[3]:], Qw[..., :Q.shape[3]]
    Ps.copy_(P)
    Qs.copy_(Q)
    assert Ps.stride(2) == 2 * P.shape[3] and Qs.stride(2) == 2 * Q.shape[3]
    for accumulate in (False, True):
        tag = f'{WC.launch_id(launch)}/slice/{"acc" if accumulate else "store"}'
        _assert_name(row, policy, splitk, Ps, Qs, tag)
        grad, dense = _start(g0, accumulate), _start(g0, accumulate)
        _launch(be, row, policy, splitk, Ps, Qs, grad, accumulate, data)
        _launch(be, row, policy, splitk, P, Q, dense, accumulate, data)
        sync()
        _check(tag, row, policy, grad, g0, accumulate, Q.shape[3])
        assert torch.equal(grad, dense), f'{tag}: differs from the dense launch'


SPLIT = [(r, pol, sk) for r in WC.ROWS if 'split' in r.extras for pol, sk in WC.launches(r)]


@pytest.mark.parametrize('launch', SPLIT, ids=WC.launch_id)
def test_split_copy_operands(launch):
    """strict direct-to-LDS kernel: a producer-written split copy ([8 hi | 8 lo] per group of 8 channels) of P, of Q and of both gives the bits of the in-kernel split"""
    row, policy, splitk = launch
    be = hip()
    data, _ = _case(row, policy)
    x, dy, g0 = data
    P, Q = _operands(be, row, policy, x, dy)
    plain = _start(g0, True)
    _launch(be, row, policy, splitk, P, Q, plain, True, data)
    sync()
    _check(f'{WC.launch_id(launch)}/unsplit/acc', row, policy, plain, g0, True, Q.shape[3])
    Pc, Qc = (P, Q) if DRY else (_split_copy(P), _split_copy(Q))
    for ps, qs in ((True, False), (False, True), (True, True)):
        tag = f'{WC.launch_id(launch)}/split-{"p" if ps else ""}{"q" if qs else ""}'
        _assert_name(row, policy, splitk, P, Q, tag, p_split=ps, q_split=qs)
        grad = _start(g0, True)
        _launch(be, row, policy, splitk, Pc if ps else P, Qc if qs else Q, grad, True, data, **({} if DRY else {'p_split': ps, 'q_split': qs}))
        sync()
        assert torch.equal(grad, plain), f'{tag}: differs from the unsplit launch by {float((grad - plain).abs().max())}'


MULTI = [(r, pol, sk) for r in WC.ROWS if 'multi' in r.extras for pol, sk in WC.launches(r)]


def _multi(be, row, policy, splitk, ops_list, grads, accumulate):
    """dl_conv_wgrad_multi + dl_wgrad_reduce_batch as ops.HipBackend._launch_queued / _reduce_pending call them"""
    n = len(ops_list)
    P0, Q0 = ops_list[0]
    d = WR.wgrad_desc(row, policy, splitk, tuple(P0.shape), tuple(Q0.shape), accumulate)
    per_layer = int(be.lib.dl_wgrad_slab_floats(C.byref(d)))
    slab = torch.empty((n * per_layer + 63) // 64 * 64, dtype=torch.float32, device=DEV)
    arr = C.c_void_p * n
    Ps, Qs, Gs = arr(*[p.data_ptr() for p, _ in ops_list]), arr(*[q.data_ptr() for _, q in ops_list]), arr(*[g.data_ptr() for g in grads])
    ents = (L.WgradReduceEntry * n)()
    ops._LAUNCH.dev = P0.device
    be.check(be.lib.dl_conv_wgrad_multi(C.byref(d), n, Ps, Qs, Gs, ops._ptr(slab), ents, ops._stream()), 'dl_conv_wgrad_multi')
    pend, blocks = [], 0
    for l in range(n):
        e = L.WgradReduceEntry.from_buffer_copy(ents[l])
        assert e.slab == slab.data_ptr() + 4 * l * per_layer and e.grad == grads[l].data_ptr() and e.splitk == splitk
        e.block0 = blocks
        blocks += e.nblocks
        pend.append(e)
    tab = (L.WgradReduceEntry * n)(*pend)
    dev_tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    be.check(be.lib.dl_wgrad_reduce_batch(ops._ptr(dev_tab), n, blocks, ops._stream()), 'dl_wgrad_reduce_batch')
    sync()
    return slab, dev_tab


@pytest.mark.parametrize('launch', MULTI, ids=WC.launch_id)
def test_batched_form_of_the_direct_to_lds_kernels(launch):
    """three layers with different data in ONE split-K launch (the layer comes from blockIdx.z), reduced by one dl_wgrad_reduce_batch: in bound, and bit-identical to
    three single launches at the same split-K"""
    row, policy, splitk = launch
    be = hip()
    layers = [row._replace(id=f'{row.id}#{l}') for l in range(3)]
    datas = [_case(r, policy)[0] for r in layers]
    ops_list = [_operands(be, r, policy, dt[0], dt[1]) for r, dt in zip(layers, datas)]
    for accumulate in (False, True):
        tag = f'{WC.launch_id(launch)}/multi/{"acc" if accumulate else "store"}'
        assert _assert_name(row, policy, splitk, *ops_list[0], tag) in (1, None), f'{tag}: dl_wgrad_plan reports no batched form'
        single = [_start(dt[2], accumulate) for dt in datas]
        for r, (P, Q), g, dt in zip(layers, ops_list, single, datas):
            _launch(be, r, policy, splitk, P, Q, g, accumulate, dt)
        sync()
        batch = [_start(dt[2], accumulate) for dt in datas]
        if DRY:
            for r, (P, Q), g, dt in zip(layers, ops_list, batch, datas):
                _launch(be, r, policy, splitk, P, Q, g, accumulate, dt)
        else:
            keep = _multi(be, row, policy, splitk, ops_list, batch, accumulate)
            del keep
        for l, (r, g, s, dt) in enumerate(zip(layers, batch, single, datas)):
            _check(f'{tag}/layer{l}', r, policy, g, dt[2], accumulate, ops_list[l][1].shape[3])
            assert torch.equal(g, s), f'{tag}: layer {l} differs from its single launch by {float((g - s).abs().max())}'
