"""Dropout applied inside the norm kernels (dl_norm_forward_dropout / dl_norm_backward_dropout), the device-seed route (dl_dropout_desc.seed_dev,
dl_dropout_dev) and the captured training step with dropout active (models.StepGraph(capture_dropout=True)).

p = 0.5: the fused call must equal the unfused pair (dl_norm_forward then dl_dropout; dl_dropout then dl_norm_backward) BIT FOR BIT -- the scale 2 is
exact in every format, so no tolerance exists.  p = 0.25: the float64 reference of tests/norm_ref.py with the keep mask read off a dl_dropout run over
ones; bound = norm_ref's bound of z divided by 0.75, plus half an ulp of the output type at |want|; no element may be out of bound.  (norm_ref's bound
of z carries one storage rounding of z, us |z|; the fused kernel never rounds z itself, only z / 0.75 -- that is the added half ulp -- so the unused
us |z| / 0.75 = us |want| is what covers the two fp32 roundings of the scale: the fp32 value of 1 / 0.75 and the product.)

The geometry rows are those of norm_ref.SWEEP below test_gpu_norm.BIG that reach: the 4-pixel unrolled loop of the apply kernels plus its tail, a
channel count that is no power of two with C < Cp, more than one apply block, the second trip of the channel loop, a ragged last chunk; plus one
tiny row (N 2, 5 x 7, C 20)."""
import argparse

import pytest
import torch

import bench
import norm_ref as R
from deepliif_amd import _lib as L
from deepliif_amd import engine as E
from deepliif_amd import models as M
from deepliif_amd import networks as N
from deepliif_amd import ops
from deepliif_amd.engine import Precision

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCOPE_NAME = {L.NORM_INSTANCE: 'instance', L.NORM_BATCH: 'batch'}
ACT_NAME = {L.ACT_RELU: 'relu', L.ACT_NONE: 'none'}
SEED = 0x1234_5678_9abc_def1 & (2 ** 63 - 1)          # both halves of the 64-bit seed are in use

TINY = ((2, 5, 7, 24), 20)
# SWEEP[1]: 16 chunks, the last one short.  SWEEP[2]: 9216 pixels over 5 blocks of 128 rows -- three trips of the 4-pixel loop, then the tail.
# SWEEP[4]: Cp 24, C 20, ragged last chunk, 2 blocks of 85 rows (two unrolled trips + tail).  SWEEP[6]: C 100 < Cp 128, 8 blocks.  SWEEP[10]: Cp 4096.
ROWS = [R.SWEEP[1], R.SWEEP[2], R.SWEEP[4], R.SWEEP[6], R.SWEEP[10], TINY]
BIG = 2 ** 21


@pytest.fixture(autouse=True)
def _real_backend_again():
    ops._impl = None
    yield
    ops._impl = None


def test_the_rows_reach_what_they_are_there_for():
    R.check_sweep_geometry()
    for (n, h, w, cp), c in ROWS:
        assert n * h * w * cp <= BIG
    ge = {R.case_id(c): R.geometry(c[0][0], c[0][1] * c[0][2], c[0][3]) for c in ROWS}
    unrolled = lambda g: g['HW'] // (g['blocks'] * g['col_rows'][0])          # pixels per thread: >= 4 reaches the unrolled loop, a remainder its tail
    g = ge[R.case_id(R.SWEEP[2])]
    assert unrolled(g) >= 4 and g['HW'] % (4 * g['blocks'] * g['col_rows'][0]) != 0 and g['blocks'] > 1
    g = ge[R.case_id(R.SWEEP[4])]
    assert R.SWEEP[4][0][3] == 24 and R.SWEEP[4][1] == 20 and unrolled(g) >= 4 and g['HW'] - (g['nchunks'] - 1) * g['ppc'] < g['ppc']
    assert ge[R.case_id(R.SWEEP[6])]['blocks'] > 1 and R.SWEEP[6][1] < R.SWEEP[6][0][3]
    assert len(ge[R.case_id(R.SWEEP[10])]['col_tpp']) > 256
    g = ge[R.case_id(R.SWEEP[1])]
    assert g['HW'] - (g['nchunks'] - 1) * g['ppc'] < g['ppc']
    assert unrolled(ge[R.case_id(TINY)]) == 0


def _be():
    return ops.impl()


def _dev(t, dtype=None):
    return None if t is None else (t.to(dtype) if dtype is not None else t).to(DEV, copy=True)


def _inputs(case, scope, dtype):
    t = R.make_inputs(case, scope, dtype, repair=False)
    g = torch.Generator().manual_seed(6)
    c = case[1]
    pre = {k: torch.randn(c, generator=g) for k in ('dgamma', 'dbeta', 'chansum')}
    pre['rm'], pre['rv'] = 0.1 * torch.randn(c, generator=g), 1 + 0.1 * torch.rand(c, generator=g)
    return t, pre


def _fwd(be, t, pre, case, scope, dtype, act, z, dropout=None, **kw):
    batch = scope == L.NORM_BATCH
    rm, rv = (_dev(pre['rm']), _dev(pre['rv'])) if batch else (None, None)
    st = be.norm_forward(_dev(t['y'], dtype), z, case[1], scope, act, _dev(t['gamma']), _dev(t['beta']), rm, rv, 0.1 if batch else -1.0, None,
                         **({'dropout': dropout} if dropout is not None else {}), **kw)
    return st, rm, rv


CASES_FWD = [(case, scope, prec, act) for case in ROWS for scope in (L.NORM_INSTANCE, L.NORM_BATCH) for prec in ('bf16', 'fp32')
             for act in (L.ACT_RELU, L.ACT_NONE)]
_fwd_id = lambda v: f'{R.case_id(v[0])}-{SCOPE_NAME[v[1]]}-{v[2]}-{ACT_NAME[v[3]]}'


# ------------------------------------------------------------------------------------------------ 1. forward, p = 0.5
@pytest.mark.parametrize('cfg', CASES_FWD, ids=_fwd_id)
def test_forward_equals_norm_then_dropout(cfg):
    case, scope, precname, act = cfg
    dtype = Precision.get(precname).dtype
    shape, c = case
    t, pre = _inputs(case, scope, dtype)
    be = _be()
    z0 = torch.full(shape, 7.0, dtype=dtype, device=DEV)
    st0, rm0, rv0 = _fwd(be, t, pre, case, scope, dtype, act, z0)
    want = torch.empty_like(z0)
    be.dropout(z0, want, 0.5, SEED)
    z1 = torch.full(shape, 7.0, dtype=dtype, device=DEV)
    st1, rm1, rv1 = _fwd(be, t, pre, case, scope, dtype, act, z1, dropout=(0.5, SEED, None, 0))
    torch.cuda.synchronize()
    assert torch.equal(st0, st1), 'the statistics arrays differ'
    if scope == L.NORM_BATCH:
        assert torch.equal(rm0, rm1) and torch.equal(rv0, rv1), 'the running statistics differ'
    assert torch.equal(z1, want), f'{int((z1 != want).sum())} of {want.numel()} elements differ from dropout(norm_forward(y))'
    if shape[3] > c:
        assert float(z1[..., c:].float().abs().max()) == 0.0, 'the padding channels of z must stay exactly zero'
    kept = (z1[..., :c] != 0).float().mean().item()
    assert 0.0 < kept < 1.0


# ------------------------------------------------------------------------------------------------ 2. z a channel slice (the UNet concat buffer)
@pytest.mark.parametrize('precname', ['bf16', 'fp32'])
@pytest.mark.parametrize('case', [R.SWEEP[4], R.SWEEP[6], TINY], ids=R.case_id)
def test_forward_into_a_channel_slice_draws_the_same_mask(case, precname):
    dtype = Precision.get(precname).dtype
    (n, h, w, cp), c = case
    scope, act = L.NORM_BATCH, L.ACT_NONE
    t, pre = _inputs(case, scope, dtype)
    be = _be()
    z0 = torch.empty((n, h, w, cp), dtype=dtype, device=DEV)
    _fwd(be, t, pre, case, scope, dtype, act, z0)
    dense = torch.empty_like(z0)
    be.dropout(z0, dense, 0.5, SEED)                      # the unfused pair on dense tensors
    lo, width = cp, 2 * cp + 16                          # second half of a concat buffer, and a tail behind it
    buf = torch.full((n, h, w, width), -3.0, dtype=dtype, device=DEV)
    view = buf[..., lo:lo + cp]
    _fwd(be, t, pre, case, scope, dtype, act, view, dropout=(0.5, SEED, None, 0))
    torch.cuda.synchronize()
    assert torch.equal(view, dense), 'the mask moved with the stride of the output'
    keep = torch.ones(width, dtype=torch.bool, device=DEV)
    keep[lo:lo + cp] = False
    assert bool((buf[..., keep] == -3.0).all()), 'channels next to the slice were written'


# ------------------------------------------------------------------------------------------------ 3. strict policy: z_split
@pytest.mark.parametrize('store', [True, False], ids=['stored', 'split-only'])
@pytest.mark.parametrize('case', [R.SWEEP[2], R.SWEEP[4], TINY], ids=R.case_id)
def test_split_copy_holds_the_dropped_values(case, store):
    dtype, scope, act = torch.float32, L.NORM_BATCH, L.ACT_RELU
    shape, c = case
    t, pre = _inputs(case, scope, dtype)
    be = _be()
    z0 = torch.empty(shape, device=DEV)
    _fwd(be, t, pre, case, scope, dtype, act, z0)
    want = torch.empty_like(z0)
    be.dropout(z0, want, 0.5, SEED)
    z1 = torch.full(shape, 77.0, device=DEV)
    zs = torch.full(shape, 77.0, device=DEV)
    _fwd(be, t, pre, case, scope, dtype, act, z1, dropout=(0.5, SEED, None, 0), z_split=zs, store_z=store)
    torch.cuda.synchronize()
    if store:
        assert torch.equal(z1, want)
    else:
        assert bool((z1 == 77.0).all()), 'the fp32 buffer was written although only the split copy was asked for'
    hi, lo = R.split_decode(zs)
    w64 = want.double().cpu()
    assert torch.equal(hi, w64.float().bfloat16().double()), 'hi is not the bfloat16 rounding of the dropped value'
    assert torch.equal(lo, (w64 - hi).float().bfloat16().double()), 'lo is not the bfloat16 of the remainder of the dropped value'


# ------------------------------------------------------------------------------------------------ 4. backward, p = 0.5
@pytest.mark.parametrize('precname', ['bf16', 'fp32'])
@pytest.mark.parametrize('scope', [L.NORM_INSTANCE, L.NORM_BATCH], ids=SCOPE_NAME.get)
@pytest.mark.parametrize('case', ROWS, ids=R.case_id)
def test_backward_equals_dropout_then_norm_backward(case, scope, precname):
    dtype = Precision.get(precname).dtype
    shape, c = case
    t, pre = _inputs(case, scope, dtype)
    affine = t['gamma'] is not None
    be = _be()
    yd, dzd = _dev(t['y'], dtype), _dev(t['dz'], dtype)
    for act in (L.ACT_RELU, L.ACT_NONE):
        st, _, _ = _fwd(be, t, pre, case, scope, dtype, act, torch.empty(shape, dtype=dtype, device=DEV))
        outs = []
        for fused in (False, True):
            dy = torch.full(shape, 5.0, dtype=dtype, device=DEV)
            dg, db = (_dev(pre['dgamma']), _dev(pre['dbeta'])) if affine else (None, None)
            cs = _dev(pre['chansum'])
            if fused:
                be.norm_backward(dzd, yd, dy, st, c, scope, act, _dev(t['gamma']), dg, db, cs, dropout=(0.5, SEED, None, 0))
            else:
                dzm = torch.empty_like(dzd)
                be.dropout(dzd, dzm, 0.5, SEED)
                be.norm_backward(dzm, yd, dy, st, c, scope, act, _dev(t['gamma']), dg, db, cs)
            outs.append((dy, dg, db, cs))
        torch.cuda.synchronize()
        for name, a, b in zip(('dy', 'dgamma', 'dbeta', 'dy_chansum'), *outs):
            if a is not None:
                assert torch.equal(a, b), f'{name} ({ACT_NAME[act]}): {int((a != b).sum())} of {a.numel()} elements differ'
        assert not torch.equal(outs[0][3], _dev(pre['chansum']))
        assert torch.equal(dzd.cpu(), t['dz'].to(dtype)), 'dz was written to'


def test_backward_reads_a_channel_slice_and_writes_the_split_copy():
    """the UNet's concat gradient (dz a channel slice) and the strict policy's dy_split, together"""
    case, scope, act, dtype = R.SWEEP[4], L.NORM_BATCH, L.ACT_NONE, torch.float32
    (n, h, w, cp), c = case
    t, pre = _inputs(case, scope, dtype)
    be = _be()
    yd = _dev(t['y'])
    st, _, _ = _fwd(be, t, pre, case, scope, dtype, act, torch.empty((n, h, w, cp), device=DEV))
    buf = torch.full((n, h, w, 2 * cp), 9.0, device=DEV)
    dzv = buf[..., cp:]
    dzv.copy_(t['dz'])
    dzm = torch.empty((n, h, w, cp), device=DEV)
    be.dropout(dzv, dzm, 0.5, SEED)
    outs = []
    for fused in (False, True):
        dy = torch.empty((n, h, w, cp), device=DEV)
        dys = torch.empty((n, h, w, cp), device=DEV)
        dg, db = _dev(pre['dgamma']), _dev(pre['dbeta'])
        be.norm_backward(dzv if fused else dzm, yd, dy, st, c, scope, act, _dev(t['gamma']), dg, db, None, dy_split=dys,
                         **({'dropout': (0.5, SEED, None, 0)} if fused else {}))
        outs.append((dy, dys, dg, db))
    torch.cuda.synchronize()
    for name, a, b in zip(('dy', 'dy_split', 'dgamma', 'dbeta'), *outs):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ 5. p = 0.25 against the float64 reference
def _half_ulp(x, dtype):
    """half the spacing of `dtype` at |x| (float64 tensor): |x| in [2^(e-1), 2^e) -> 2^(e - P) / 2 with P significand bits; 0 at 0"""
    _, e = torch.frexp(x.abs())
    h = torch.ldexp(torch.full_like(x, 0.5 * R.U_STORE[dtype]), e)
    return torch.where(x == 0, torch.zeros_like(x), h)


def test_half_ulp_helper():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0, -3.0], dtype=torch.float64)
    assert _half_ulp(x, torch.bfloat16).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 0.0, 2.0 ** -7]
    assert _half_ulp(x, torch.float32).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 2.0 ** -25, 0.0, 2.0 ** -23]


@pytest.mark.parametrize('precname', ['bf16', 'fp32'])
@pytest.mark.parametrize('scope', [L.NORM_INSTANCE, L.NORM_BATCH], ids=SCOPE_NAME.get)
@pytest.mark.parametrize('case', ROWS, ids=R.case_id)
def test_forward_quarter_against_the_float64_reference(case, scope, precname):
    dtype = Precision.get(precname).dtype
    shape, c = case
    p = 0.25
    t, pre = _inputs(case, scope, dtype)
    ref = R.Reference(t['y'], c, scope, t['gamma'], t['beta'], slack=1)
    be = _be()
    ones = torch.ones(shape, dtype=torch.float32, device=DEV)
    km = torch.empty_like(ones)
    be.dropout(ones, km, p, SEED)
    torch.cuda.synchronize()
    keep = (km != 0).double().cpu()
    assert torch.equal(km.double().cpu(), keep * float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))))
    for act in (L.ACT_RELU, L.ACT_NONE):
        z = torch.empty(shape, dtype=dtype, device=DEV)
        _fwd(be, t, pre, case, scope, dtype, act, z, dropout=(p, SEED, None, 0))
        torch.cuda.synchronize()
        z64, b_z = ref.forward(act, None, dtype)
        want = z64 * keep / 0.75
        bnd = keep * (b_z / 0.75 + _half_ulp(want, dtype))
        worst, report = R.compare(z, want, bnd, ref.ge)
        print(f'{precname}/{R.case_id(case)}/{SCOPE_NAME[scope]}/{ACT_NAME[act]}: worst err/bound {worst:.4f}')
        assert worst <= 1.0 and not report, report
        assert bool((z.cpu()[keep == 0] == 0).all()), 'a dropped element is not exactly zero'


# ------------------------------------------------------------------------------------------------ 6. seeds
def _mask_of(be, shape, dropout, entry='norm'):
    """the keep mask a site draws, read off the kernels: 'plain' through dl_dropout_dev over ones, 'norm' through dl_norm_forward_dropout with
    gamma = 0, beta = 1 (scale = 0, shift = 1: z = 1 exactly before the mask)"""
    ones = torch.ones(shape, dtype=torch.float32, device=DEV)
    out = torch.empty_like(ones)
    if entry == 'plain':
        be.dropout_dev(ones, out, dropout)
    else:
        c = shape[3]
        be.norm_forward(ones, out, c, L.NORM_BATCH, L.ACT_NONE, torch.zeros(c, device=DEV), torch.ones(c, device=DEV), None, None, -1.0, None, dropout=dropout)
    torch.cuda.synchronize()
    assert bool(((out == 0) | (out == 2)).all())
    return out != 0


@pytest.mark.parametrize('entry', ['norm', 'plain'])
def test_device_seed_plus_call_index_is_the_host_seed(entry):
    be = _be()
    shape = (2, 40, 36, 24)
    base = (2 ** 63 - 2) if entry == 'plain' else SEED      # the plain entry also crosses the 2^63 wrap
    sd = torch.tensor([base], dtype=torch.int64, device=DEV)
    masks = {}
    for j in (1, 2, 5):
        dev = _mask_of(be, shape, (0.5, 0, sd, j), entry)
        host = _mask_of(be, shape, (0.5, (base + j) & (2 ** 63 - 1), None, 0), entry)
        assert torch.equal(dev, host), f'call index {j}: the device-seed mask is not the host-seed mask of base + {j}'
        # the stand-alone pass with a host seed is today's dl_dropout
        ones = torch.ones(shape, device=DEV)
        ref = torch.empty_like(ones)
        be.dropout(ones, ref, 0.5, (base + j) & (2 ** 63 - 1))
        assert torch.equal(ref != 0, host)
        masks[j] = dev
        n = dev.numel()
        frac = dev.float().mean().item()
        assert abs(frac - 0.5) <= 5 * 0.5 / n ** 0.5, f'kept fraction {frac} over {n} elements'
    assert not torch.equal(masks[1], masks[2]) and not torch.equal(masks[2], masks[5])
    assert abs((masks[1] ^ masks[2]).float().mean().item() - 0.5) <= 5 * 0.5 / masks[1].numel() ** 0.5          # independent, not shifted copies
    # the seed is read when the kernel RUNS: a new value in the same device word gives the next step's masks
    sd.fill_((base + 3) & (2 ** 63 - 1))
    assert torch.equal(_mask_of(be, shape, (0.5, 0, sd, 2), entry), masks[5])


def test_backward_with_a_device_seed():
    case, scope, act, dtype = R.SWEEP[4], L.NORM_INSTANCE, L.ACT_RELU, torch.bfloat16
    shape, c = case
    t, pre = _inputs(case, scope, dtype)
    be = _be()
    yd, dzd = _dev(t['y'], dtype), _dev(t['dz'], dtype)
    st, _, _ = _fwd(be, t, pre, case, scope, dtype, act, torch.empty(shape, dtype=dtype, device=DEV))
    sd = torch.tensor([SEED - 4], dtype=torch.int64, device=DEV)
    outs = []
    for drop in ((0.5, SEED, None, 0), (0.5, 0, sd, 4)):
        dy = torch.empty(shape, dtype=dtype, device=DEV)
        cs = _dev(pre['chansum'])
        be.norm_backward(dzd, yd, dy, st, c, scope, act, None, None, None, cs, dropout=drop)
        outs.append((dy, cs))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ 7. error paths
def test_residual_and_external_partials_are_rejected_before_any_launch():
    case, scope, act, dtype = TINY, L.NORM_BATCH, L.ACT_RELU, torch.bfloat16
    shape, c = case
    t, pre = _inputs(case, scope, dtype)
    be = _be()
    yd, dzd, res = _dev(t['y'], dtype), _dev(t['dz'], dtype), _dev(t['res'], dtype)
    z = torch.full(shape, 7.0, dtype=dtype, device=DEV)
    with pytest.raises(L.HipLibraryError, match='residual'):
        be.norm_forward(yd, z, c, scope, act, _dev(t['gamma']), _dev(t['beta']), None, None, -1.0, res, dropout=(0.5, SEED, None, 0))
    st, _, _ = _fwd(be, t, pre, case, scope, dtype, act, torch.empty(shape, dtype=dtype, device=DEV))
    dy = torch.full(shape, 7.0, dtype=dtype, device=DEV)
    dg, db, cs = _dev(pre['dgamma']), _dev(pre['dbeta']), _dev(pre['chansum'])
    with pytest.raises(L.HipLibraryError, match='ext_nchunks'):
        be.norm_backward(dzd, yd, dy, st, c, scope, act, _dev(t['gamma']), dg, db, cs, ext_nchunks=1, dropout=(0.5, SEED, None, 0))
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((dy == 7.0).all()), 'a rejected call wrote its output'
    assert torch.equal(dg.cpu(), pre['dgamma']) and torch.equal(db.cpu(), pre['dbeta']) and torch.equal(cs.cpu(), pre['chansum'])


# ------------------------------------------------------------------------------------------------ 8. network level
def _net_run(arch, size, precname):
    torch.manual_seed(11)
    E._DROPOUT_COUNTER[0] = 0
    net = N.define_G(3, 3, 8, arch, 'batch', True, 'normal', 0.02, [0], 'zero')
    net.train()
    prec = Precision.get(precname)
    tape = E.Tape()
    ctx = E.Ctx(prec, tape, training=True)
    g = torch.Generator().manual_seed(6)
    xa = E.to_engine((torch.rand(2, 3, size, size, generator=g) * 2 - 1).to(DEV), prec)
    xa.needs_grad = True
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    ya = net.run(ctx, xa)
    ya.grad = E.to_engine(torch.randn(2, 3, size, size, generator=g).to(DEV), prec).t
    tape.backward()
    torch.cuda.synchronize()
    return E.from_engine(ya).clone(), {k: p.grad.clone() for k, p in net.named_parameters()}, E._DROPOUT_COUNTER[0]


# unet_32 has no ngf*8 block besides its innermost one, hence no Dropout module: it pins that nothing changes there; unet_64 has one dropout site
@pytest.mark.parametrize('precname', ['bf16', 'fp32'])
@pytest.mark.parametrize('arch,size,sites', [('resnet_2blocks', 32, 2), ('unet_32', 32, 0), ('unet_64', 64, 1)])
def test_networks_fused_equals_unfused(arch, size, sites, precname, monkeypatch):
    calls = {'fused': 0, 'plain': 0}
    orig_fwd, orig_drop = ops.HipBackend.norm_forward, ops.HipBackend.dropout

    def count_fwd(self, *a, **kw):
        calls['fused'] += kw.get('dropout') is not None
        return orig_fwd(self, *a, **kw)

    def count_drop(self, *a, **kw):
        calls['plain'] += 1
        return orig_drop(self, *a, **kw)
    monkeypatch.setattr(ops.HipBackend, 'norm_forward', count_fwd)
    monkeypatch.setattr(ops.HipBackend, 'dropout', count_drop)
    y1, g1, n1 = _net_run(arch, size, precname)
    assert calls == {'fused': sites, 'plain': 0}
    monkeypatch.setattr(ops.HipBackend, 'supports_fused_dropout', False)
    y0, g0, n0 = _net_run(arch, size, precname)
    assert calls == {'fused': sites, 'plain': 2 * sites}
    assert n0 == n1 == sites
    assert torch.equal(y0, y1), f'outputs differ in {int((y0 != y1).sum())} elements'
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())


# ------------------------------------------------------------------------------------------------ 9. the captured step
@pytest.fixture
def _one_stream(monkeypatch):
    monkeypatch.setattr(M, '_N_STREAMS', 1)


def _batches(n, size, count, m):
    g = torch.Generator().manual_seed(77)
    return [{'A': (torch.rand(n, 3, size, size, generator=g) * 2 - 1).to(DEV), 'B': [(torch.rand(n, 3, size, size, generator=g) * 2 - 1).to(DEV) for _ in range(m)],
             'A_paths': ['x']} for _ in range(count)]


def _build(kind, precision):
    """tests/test_gpu_graph.py's _build with Dropout(0.5) active; the dropout seed sequence starts over"""
    args = argparse.Namespace(ngf=8, norm='instance', precision=precision, batch=2, size=64)
    torch.manual_seed(0)
    E._DROPOUT_COUNTER[0] = 0
    if kind == 'train':
        opt = bench.make_opt(args, 0)
    else:
        opt = bench.make_opt(args, 0, M=4, seg_gen=True)
        opt.net_gs, opt.norm = 'unet_64', 'batch'
    opt.no_dropout = False
    model = M.create_model(opt)
    model.setup(opt)
    return model


def _flat(model):
    return torch.cat([o.flat.data.clone() for o in model.optimizers])


@pytest.mark.parametrize('kind', ['train', 'train18'])
def test_captured_step_with_dropout_is_bit_identical_to_the_eager_step(kind, _one_stream):
    batches = _batches(2, 64, 6, 5)
    eager = _build(kind, 'bf16')
    losses = []
    for b in batches:
        eager.set_input(b)
        eager.optimize_parameters()
        torch.cuda.synchronize()
        losses.append(eager.get_current_losses())
    want, ticks = _flat(eager), E._DROPOUT_COUNTER[0]
    assert ticks > 0 and ticks % 6 == 0
    graphed = _build(kind, 'bf16')
    sg = M.StepGraph(graphed, warmup=2, capture_dropout=True)
    assert sg.why_eager is None
    for i, b in enumerate(batches):
        sg.step(b)
        torch.cuda.synchronize()
        lg = graphed.get_current_losses()
        assert lg.keys() == losses[i].keys() and all(lg[k] == losses[i][k] for k in lg), (i, {k: (losses[i][k], lg[k]) for k in lg if lg[k] != losses[i][k]})
    assert sg.why_eager is None and sg.graph is not None and sg.calls == 6
    assert sg.sites == ticks // 6 and E._DROPOUT_COUNTER[0] == ticks
    assert torch.equal(_flat(graphed), want)
    # the masks advance: the same batch through two consecutive replays
    fakes = []
    for _ in range(2):
        sg.step(batches[0])
        torch.cuda.synchronize()
        fakes.append(graphed.fake_B_1.clone())
    assert not torch.equal(fakes[0], fakes[1])


def test_replays_with_dropout_without_a_synchronize_in_between(_one_stream):
    """the seed of step N is staged in pinned memory and copied asynchronously: the ring of engine.DropoutSeeds must keep the host, which runs ahead,
    from rewriting a slot before its copy ran.  Ten steps back to back, ONE synchronize at the end, against the eager run"""
    batches = _batches(2, 64, 10, 5)
    graphed = _build('train', 'bf16')
    sg = M.StepGraph(graphed, warmup=2, capture_dropout=True)
    torch.cuda.synchronize()
    for b in batches:
        sg.step(b)
    torch.cuda.synchronize()
    got = _flat(graphed)
    assert sg.graph is not None and sg.calls == 10
    eager = _build('train', 'bf16')
    for b in batches:
        eager.set_input(b)
        eager.optimize_parameters()
    torch.cuda.synchronize()
    assert torch.equal(_flat(eager), got)


def test_default_still_declines_dropout(_one_stream):
    model = _build('train', 'bf16')
    sg = M.StepGraph(model)
    assert sg.why_eager == 'dropout is active (its seed is a kernel argument)' and sg.seeds is None
