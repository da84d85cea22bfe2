"""The normalisation kernels (csrc/norm.hip: norm_partial_kernel, norm_chunk_sum_kernel<0|1|2>, both finalizers, norm_apply_kernel, norm_bwd_apply_kernel,
norm_bias_final_kernel) through ops.impl(), element by element against the float64 reference under the derived bound of tests/norm_ref.py -- no element
may be out of bound, slack = 1.  The geometry rows (norm_ref.SWEEP) reach the unrolled chunk loop, a channel count that is no power of two, the second trip
of the channel loop, ragged last chunks and the 256 bias partials; further cases run channel-slice views of wider buffers, instance scope with an affine,
the strict policy's split copies and run-to-run identity; a conditioning tier measures (and bounds) channels whose mean is large against their spread.
tests/test_norm_ref_host.py holds the reference and the bound themselves to torch and to an emulation of the kernels' summation order.

The backward takes the reference's statistics rounded to fp32 on both sides (see norm_ref).  The worst err / bound of every case goes to
parity_errors_norm.json in the directory $DL_PARITY_DIR names (default parity_out/).

DL_TEST_DRYRUN=1 runs the file on the CPU with the formula emulation in the kernels' place (a check of the test code only)."""
import json
import os

import pytest
import torch

import norm_ref as R
from deepliif_amd import _lib as L
from deepliif_amd import ops
from deepliif_amd.engine import Precision
from deepliif_amd.geometry import ConvSpec, cpad

from test_gpu_kernels import DEV, DRY, hip, sync

pytestmark = pytest.mark.gpu
ERRLOG = {}
ERRLOG_DIR = os.environ.get('DL_PARITY_DIR', 'parity_out')
SLACK = 1                # multiplier of the summation lengths of the bound; 1 = as derived
BIG = 2 ** 21            # elements above which a row runs one activation per scope instead of three
MOMENTUM = 0.1
SCOPE_NAME = {L.NORM_INSTANCE: 'instance', L.NORM_BATCH: 'batch'}
COMBOS = ((L.ACT_RELU, True), (L.ACT_LRELU, False), (L.ACT_NONE, True))          # every activation, with and without a residual


@pytest.fixture(autouse=True)
def _real_backend_again():
    yield
    ops._impl = None


@pytest.fixture(autouse=True, scope='module')
def _errlog():
    yield
    os.makedirs(ERRLOG_DIR, exist_ok=True)
    with open(os.path.join(ERRLOG_DIR, 'parity_errors_norm.json'), 'w') as f:
        json.dump(ERRLOG, f, indent=1, sort_keys=True)


class Checker:
    """collects err / bound per output of one case; done() asserts"""

    def __init__(self, tag, ge):
        self.tag, self.ge, self.ratios, self.reports = tag, ge, {}, []

    def __call__(self, key, got, want, bnd):
        worst, report = R.compare(got, want, bnd, self.ge if got.dim() == 4 else None)
        self.ratios[key] = max(worst, self.ratios.get(key, 0.0))
        if report:
            self.reports.append(f'{key}: {report}')

    def done(self):
        worst = max(self.ratios, key=self.ratios.get)
        ERRLOG[self.tag] = {k: round(v, 4) for k, v in self.ratios.items()}
        print(f'{self.tag}: worst err/bound {self.ratios[worst]:.4f} ({worst}); ' + ' '.join(f'{k} {v:.3f}' for k, v in self.ratios.items()))
        assert self.ratios[worst] <= 1.0 and not self.reports, f'{self.tag}\n' + '\n'.join(self.reports)
        return self.ratios[worst]


def _preloads(c):
    gen = torch.Generator().manual_seed(6)
    pre = {k: torch.randn(c, generator=gen) for k in ('dgamma', 'dbeta', 'chansum')}
    pre['rm'], pre['rv'] = 0.1 * torch.randn(c, generator=gen), 1 + 0.1 * torch.rand(c, generator=gen)
    return pre


def _dev(t, dtype=None):
    return None if t is None else (t.to(dtype) if dtype is not None else t).to(DEV, copy=True)          # (a copy in the dry run too: the kernels accumulate in place)


def _forward(be, ref, chk, t, dtype, act, with_res, pre, yd=None, zd=None, resd=None, tag=''):
    """one dl_norm_forward against the reference: the four statistics arrays, the running statistics, z"""
    c, scope = ref.C, ref.scope
    batch = scope == L.NORM_BATCH
    yd = _dev(t['y'], dtype) if yd is None else yd
    zd = torch.empty(tuple(ref.y.shape), dtype=dtype, device=DEV) if zd is None else zd
    if with_res and resd is None:
        resd = _dev(t['res'], dtype)
    rm, rv = (_dev(pre['rm']), _dev(pre['rv'])) if batch else (None, None)
    st = be.norm_forward(yd, zd, c, scope, act, _dev(t['gamma']), _dev(t['beta']), rm, rv, MOMENTUM if batch else -1.0, resd if with_res else None)
    sync()
    sb = ref.stat_bounds()
    for i, k in enumerate(('mean', 'rstd', 'scale', 'shift')):
        chk(tag + k, st[i], ref.stats()[k], sb[k])
    if batch:
        (rm_ref, rv_ref), (b_rm, b_rv) = ref.running(pre['rm'], pre['rv'], MOMENTUM)
        chk(tag + 'running_mean', rm, rm_ref, b_rm)
        chk(tag + 'running_var', rv, rv_ref, b_rv)
    z, b_z = ref.forward(act, t['res'] if with_res else None, dtype)
    chk(tag + 'z', zd, z, b_z)
    if ref.Cp > c:
        assert float(zd[..., c:].float().abs().max()) == 0.0, 'the padding channels of z must stay exactly zero'
    return st, zd


def _backward(be, ref, chk, t, dtype, act, pre, yd=None, dzd=None, dyd=None, tag=''):
    """one dl_norm_backward (statistics: the reference's, in fp32) against the reference: dy, dgamma / dbeta and the channel sums onto preloaded values"""
    c, scope = ref.C, ref.scope
    affine = t['gamma'] is not None
    yd = _dev(t['y'], dtype) if yd is None else yd
    dzd = _dev(t['dz'], dtype) if dzd is None else dzd
    dyd = torch.empty(tuple(ref.y.shape), dtype=dtype, device=DEV) if dyd is None else dyd
    dg, db = (_dev(pre['dgamma']), _dev(pre['dbeta'])) if affine else (None, None)
    cs = _dev(pre['chansum'])
    be.norm_backward(dzd, yd, dyd, ref.stats32.to(DEV), c, scope, act, _dev(t['gamma']), dg, db, cs)
    sync()
    val, bnd = ref.backward(act, t['dz'], dtype, pre['dgamma'] if affine else None, pre['dbeta'] if affine else None, pre['chansum'])
    chk(tag + 'dy', dyd, val['dy'], bnd['dy'])
    chk(tag + 'chansum', cs, val['chansum'], bnd['chansum'])
    if affine:
        chk(tag + 'dgamma', dg, val['dgamma'], bnd['dgamma'])
        chk(tag + 'dbeta', db, val['dbeta'], bnd['dbeta'])
    if ref.Cp > c:
        assert float(dyd[..., c:].float().abs().max()) == 0.0, 'the padding channels of dy must stay exactly zero'
    return dyd, dg, db, cs


def _combos(case, scope):
    if case[0][0] * case[0][1] * case[0][2] * case[0][3] <= BIG:
        return COMBOS
    return COMBOS[:1] if scope == L.NORM_INSTANCE else COMBOS[1:2]


def test_the_table_reaches_what_it_is_there_for():
    R.check_sweep_geometry()


# ------------------------------------------------------------------------------------------------ the geometry sweep
@pytest.mark.parametrize('precname', ['fp32', 'bf16'])
@pytest.mark.parametrize('scope', [L.NORM_INSTANCE, L.NORM_BATCH], ids=SCOPE_NAME.get)
@pytest.mark.parametrize('case', R.SWEEP, ids=R.case_id)
def test_sweep(case, scope, precname):
    """both scopes (batch: affine, running statistics, dgamma / dbeta), the three activations, with and without a residual, backward onto preloaded
    dgamma / dbeta / channel sums.  The reference's statistics are computed once per case and shared by the activations."""
    dtype = Precision.get(precname).dtype
    t = R.make_inputs(case, scope, dtype)
    assert t['near_kink'] == 0, 'elements are left near the activation kink'
    ref = R.Reference(t['y'], case[1], scope, t['gamma'], t['beta'], slack=SLACK)
    chk = Checker(f'{precname}/{R.case_id(case)}/{SCOPE_NAME[scope]}', ref.ge)
    pre = _preloads(case[1])
    be = hip()
    yd, dzd = _dev(t['y'], dtype), _dev(t['dz'], dtype)
    for act, with_res in _combos(case, scope):
        _forward(be, ref, chk, t, dtype, act, with_res, pre, yd=yd)
        _backward(be, ref, chk, t, dtype, act, pre, yd=yd, dzd=dzd)
    chk.done()


@pytest.mark.parametrize('scope', [L.NORM_INSTANCE, L.NORM_BATCH], ids=SCOPE_NAME.get)
@pytest.mark.parametrize('case', R.SWEEP, ids=R.case_id)
def test_sweep_f16_library_forward(case, scope):
    """the inference policy's library (the same sources, IEEE half as the 16-bit type): forward only"""
    dtype = torch.float16
    t = R.make_inputs(case, scope, dtype, repair=False)          # no backward: the forward is continuous at the kink
    ref = R.Reference(t['y'], case[1], scope, t['gamma'], t['beta'], slack=SLACK)
    chk = Checker(f'fp16/{R.case_id(case)}/{SCOPE_NAME[scope]}', ref.ge)
    pre = _preloads(case[1])
    with ops.half_mode('fp16'):
        be = hip()
        assert DRY or be.half == 'fp16'
        yd = _dev(t['y'], dtype)
        for act, with_res in _combos(case, scope):
            _forward(be, ref, chk, t, dtype, act, with_res, pre, yd=yd)
    chk.done()


# ------------------------------------------------------------------------------------------------ further cases on one mid-sized shape
MID = ((3, 24, 20, 64), 50)          # 8 chunks of 60 pixels, rows = 32, C < Cp


def _wide(shape, width, lo, fill, dtype, src=None):
    """a [N, H, W, width] buffer of `fill` and its channel slice lo : lo + Cp (holding src)"""
    n, h, w, cp = shape
    buf = torch.full((n, h, w, width), fill, dtype=dtype, device=DEV)
    view = buf[..., lo:lo + cp]
    if src is not None:
        view.copy_(src.to(dtype))
    return buf, view


def _untouched(buf, lo, cp, fill):
    keep = torch.ones(buf.shape[3], dtype=torch.bool, device=buf.device)
    keep[lo:lo + cp] = False
    return bool((buf[..., keep] == fill).all())


@pytest.mark.parametrize('precname', ['fp32', 'bf16'])
def test_channel_slices_of_wider_buffers(precname):
    """y, z, the residual, dz and dy each a slice of a wider buffer with its own width and offset (UNet's zero-copy concat): every pixel stride of the
    descriptor differs from Cp and from the others.  Every element outside the slices keeps its sentinel."""
    case, scope, act = MID, L.NORM_BATCH, L.ACT_RELU
    dtype = Precision.get(precname).dtype
    shape, c = case
    cp = shape[3]
    t = R.make_inputs(case, scope, dtype)
    assert t['near_kink'] == 0
    ref = R.Reference(t['y'], c, scope, t['gamma'], t['beta'], slack=SLACK)
    chk = Checker(f'{precname}/slices/{R.case_id(case)}', ref.ge)
    pre = _preloads(c)
    be = hip()
    ybuf, yv = _wide(shape, 192, 64, 7.0, dtype, t['y'])
    zbuf, zv = _wide(shape, 128, 0, -3.0, dtype)
    rbuf, rv_ = _wide(shape, 256, 192, 5.0, dtype, t['res'])
    dzbuf, dzv = _wide(shape, 160, 96, 9.0, dtype, t['dz'])
    dybuf, dyv = _wide(shape, 72, 8, -11.0, dtype)
    _forward(be, ref, chk, t, dtype, act, True, pre, yd=yv, zd=zv, resd=rv_)
    _backward(be, ref, chk, t, dtype, act, pre, yd=yv, dzd=dzv, dyd=dyv)
    chk.done()
    for name, buf, lo, fill in (('y', ybuf, 64, 7.0), ('z', zbuf, 0, -3.0), ('residual', rbuf, 192, 5.0), ('dz', dzbuf, 96, 9.0), ('dy', dybuf, 8, -11.0)):
        assert _untouched(buf, lo, cp, fill), f'the {name} buffer changed outside its slice'
    for name, view, src in (('y', yv, t['y']), ('residual', rv_, t['res']), ('dz', dzv, t['dz'])):
        assert torch.equal(view.cpu(), src.to(dtype)), f'the {name} operand was written to'


@pytest.mark.parametrize('precname', ['fp32', 'bf16'])
def test_instance_scope_with_an_affine(precname):
    """per-image statistics under BatchNorm's affine (batched inference on per-tile statistics): the fused finalizer with gamma / beta; the backward with a
    dgamma takes the unfused pair (norm_chunk_sum_kernel<0> + norm_bwd_finalize_kernel) and accumulates onto preloaded gradients"""
    case, scope = MID, L.NORM_INSTANCE
    dtype = Precision.get(precname).dtype
    t = R.make_inputs(case, scope, dtype, affine=True)
    assert t['near_kink'] == 0
    ref = R.Reference(t['y'], case[1], scope, t['gamma'], t['beta'], slack=SLACK)
    chk = Checker(f'{precname}/instance-affine/{R.case_id(case)}', ref.ge)
    pre = _preloads(case[1])
    be = hip()
    for act, with_res in COMBOS:
        _forward(be, ref, chk, t, dtype, act, with_res, pre)
        _backward(be, ref, chk, t, dtype, act, pre)
    chk.done()


@pytest.mark.parametrize('precname', ['fp32', 'bf16'])
def test_run_to_run_bit_identity(precname):
    case, scope, act = MID, L.NORM_BATCH, L.ACT_LRELU
    dtype = Precision.get(precname).dtype
    t = R.make_inputs(case, scope, dtype)
    ref = R.Reference(t['y'], case[1], scope, t['gamma'], t['beta'], slack=SLACK)
    pre = _preloads(case[1])
    be = hip()
    runs = []
    for _ in range(2):
        chk = Checker(f'{precname}/twice/{R.case_id(case)}', ref.ge)
        st, z = _forward(be, ref, chk, t, dtype, act, True, pre)
        dy, dg, db, cs = _backward(be, ref, chk, t, dtype, act, pre)
        chk.done()
        runs.append((st, z, dy, dg, db, cs))
    for name, a, b in zip(('statistics', 'z', 'dy', 'dgamma', 'dbeta', 'channel sums'), *runs):
        assert torch.equal(a, b), f'{name}: run-to-run difference'


@pytest.mark.skipif(DRY, reason='the split copies are a storage detail of the GPU side (FakeBackend.supports_split is False)')
@pytest.mark.parametrize('store', [True, False], ids=['stored', 'split-only'])
def test_strict_split_copies(store):
    """z_split / dy_split (fp32 policy): [8 bf16 hi | 8 bf16 lo] per eight channels next to the fp32 value; hi is the value rounded to bfloat16, hi + lo gives
    it back to 2^-16 relative (lo is the bfloat16 of an exactly representable remainder of at most 2^-8 |value|).  store_z / store_dy False: only the split
    copy is written, the fp32 buffer keeps its sentinel; hi + lo is then held to the reference directly, with 2^-16 |value| on top of the bound."""
    case, scope, act, dtype = MID, L.NORM_BATCH, L.ACT_RELU, torch.float32
    shape, c = case
    t = R.make_inputs(case, scope, dtype)
    ref = R.Reference(t['y'], c, scope, t['gamma'], t['beta'], slack=SLACK)
    chk = Checker(f'fp32/split-{"stored" if store else "only"}/{R.case_id(case)}', ref.ge)
    pre = _preloads(c)
    be = hip()
    yd, dzd, resd = _dev(t['y']), _dev(t['dz']), _dev(t['res'])
    z = torch.full(shape, 77.0, device=DEV)
    zs = torch.full(shape, 77.0, device=DEV)
    be.norm_forward(yd, z, c, scope, act, _dev(t['gamma']), _dev(t['beta']), None, None, -1.0, resd, z_split=zs, store_z=store)
    dy = torch.full(shape, 77.0, device=DEV)
    dys = torch.full(shape, 77.0, device=DEV)
    be.norm_backward(dzd, yd, dy, ref.stats32.to(DEV), c, scope, act, _dev(t['gamma']), _dev(pre['dgamma']), _dev(pre['dbeta']), None, dy_split=dys,
                     store_dy=store)
    sync()
    z_ref, b_z = ref.forward(act, t['res'], dtype)
    val, bnd = ref.backward(act, t['dz'], dtype, pre['dgamma'], pre['dbeta'], None)
    for name, full, split, want, b in (('z', z, zs, z_ref, b_z), ('dy', dy, dys, val['dy'], bnd['dy'])):
        hi, lo = R.split_decode(split)
        if store:
            chk(name, full, want, b)
            v = full.double().cpu()
            assert torch.equal(hi, v.float().bfloat16().double()), f'{name}: hi is not the bfloat16 rounding of the stored value'
            assert bool(((hi + lo - v).abs() <= 2.0 ** -16 * v.abs()).all()), f'{name}: hi + lo does not give the stored value back to 2^-16'
        else:
            assert bool((full == 77.0).all()), f'{name}: the fp32 buffer was written although only the split copy was asked for'
            chk(name + '(hi+lo)', hi + lo, want, b + 2.0 ** -16 * (want.abs() + b))
    chk.done()


@pytest.mark.skipif(DRY, reason='reads the workspace the kernels wrote')
def test_the_apply_grid_is_the_restated_one():
    """norm_ref.geometry restates apply_grid, and the workspace contract (tests/test_norm_ref_host.py) rests on it: the backward writes one row of bias
    partials per block, so after a call into a NaN-filled workspace exactly blocks x N rows of that region hold numbers"""
    for case in (R.SWEEP[5], R.SWEEP[7], MID):          # 17 x 3, 32 x 8, 2 x 3 blocks
        (n, h, w, cp), c = case
        t = R.make_inputs(case, L.NORM_INSTANCE, torch.bfloat16, repair=False)
        ref = R.Reference(t['y'], c, L.NORM_INSTANCE)
        be = hip()
        yd, dzd = _dev(t['y'], torch.bfloat16), _dev(t['dz'], torch.bfloat16)
        dy = torch.empty_like(yd)
        cs = torch.zeros(c, device=DEV)
        be.norm_backward(dzd, yd, dy, ref.stats32.to(DEV), c, L.NORM_INSTANCE, L.ACT_NONE, None, None, None, cs)          # sizes the workspace
        sync()
        ws = ops.WS.get('norm_ws', 0, yd.device)
        ws.fill_(float('nan'))
        be.norm_backward(dzd, yd, dy, ref.stats32.to(DEV), c, L.NORM_INSTANCE, L.ACT_NONE, None, None, None, cs)
        sync()
        ge = ref.ge
        lo = n * ge['nchunks'] * 2 * cp + 4 * n * cp
        rows = ws[lo:lo + R.BIAS_PART_ROWS * cp].view(R.BIAS_PART_ROWS, cp)
        written = ~torch.isnan(rows).all(dim=1)
        assert int(written.sum()) == ge['blocks'] * n and bool(written[:ge['blocks'] * n].all()), (R.case_id(case), int(written.sum()), ge['blocks'], n)


# ------------------------------------------------------------------------------------------------ conditioning tier
COND = [(1.0, 0.01), (4.0, 0.01), (32.0, 1.0), (100.0, 1.0)]
COND_SHAPES = [((1, 64, 64, 8), 8), ((2, 128, 128, 64), 64)]


def _record(record_property, tag, zd, z_ref, b_z, rstd, ref):
    zerr = float((zd.double().cpu() - z_ref).abs().max())
    rerr = float(((rstd.double().cpu() - ref.rstd) / ref.rstd).abs()[:, :ref.C].max())
    cond = float(ref.conditioning[:, :ref.C].max())
    ERRLOG[tag].update({'max_abs_z_err': zerr, 'max_rel_rstd_err': rerr, 'conditioning': cond, 'max_z_bound': float(b_z.max())})
    for k in ('max_abs_z_err', 'max_rel_rstd_err', 'conditioning'):
        record_property(k, ERRLOG[tag][k])
    print(f'{tag}: max |z - ref| {zerr:.3e} (bound {float(b_z.max()):.3e}), max relative error of rstd {rerr:.3e}, E y^2 / (var + eps) {cond:.3e}')


@pytest.mark.parametrize('precname', ['fp32', 'bf16'])
@pytest.mark.parametrize('scope', [L.NORM_INSTANCE, L.NORM_BATCH], ids=SCOPE_NAME.get)
@pytest.mark.parametrize('ms', COND, ids=lambda ms: f'mean{ms[0]:g}-spread{ms[1]:g}')
@pytest.mark.parametrize('case', COND_SHAPES, ids=R.case_id)
def test_conditioning(case, ms, scope, precname, record_property):
    """Channels whose mean is large against their spread.  The kernels take the variance as E y^2 - mean^2 from fp32 partial sums, so the error of rstd
    grows with E y^2 / (var + eps); the bound carries that factor and is the ONLY tolerance here.  Recorded per case: max |z - ref|, the largest relative
    error of rstd, the factor.  DESIGN.md (4.3 - 4.6) holds the table and what it means for the strict policy's 1e-3.  Forward only: where the bound on the
    normalised value passes the kink margin, act' is not comparable element by element."""
    dtype = Precision.get(precname).dtype
    t = R.make_inputs(case, scope, dtype, mean=ms[0], spread=ms[1], repair=False)
    ref = R.Reference(t['y'], case[1], scope, t['gamma'], t['beta'], slack=SLACK)
    tag = f'{precname}/conditioning/{R.case_id(case)}/{SCOPE_NAME[scope]}/mean{ms[0]:g}-spread{ms[1]:g}'
    chk = Checker(tag, ref.ge)
    st, zd = _forward(hip(), ref, chk, t, dtype, L.ACT_NONE, False, _preloads(case[1]))
    chk.done()
    z_ref, b_z = ref.forward(L.ACT_NONE, None, dtype)
    _record(record_property, tag, zd, z_ref, b_z, st[1], ref)


@pytest.mark.skipif(DRY, reason='the emulation reports no fused statistics')
@pytest.mark.parametrize('precname', ['fp32', 'bf16'])
def test_conditioning_of_the_fused_statistics(precname, record_property):
    """the same sum / sum of squares in fp32, produced by a convolution's epilogue (dl_conv_forward(stats_part) + dl_norm_forward(ext_nchunks)): a small conv
    with a bias near 1 and weights near 0.01 (the case and the calls of test_conv_fused_norm_statistics), so the conv output itself has the offset.  The
    reference is the float64 normalisation of the STORED conv output.  The producer's order inside a chunk is not restated here: its path is bounded by
    the chunk's pixel count (any order of P values has at most P - 1 additions on a path), then the chunk lanes."""
    prec = Precision.get(precname)
    cin, cout, k, N, H, W_ = 64, 8, 3, 1, 32, 32
    spec = ConvSpec('conv', cin, cout, k, 1, 1, L.PAD_ZERO, 0)
    gen = torch.Generator().manual_seed(21)
    w = (0.01 * torch.randn(cout, cin, k, k, generator=gen)).to(prec.dtype).float().to(DEV)
    bias = (1 + 0.01 * torch.randn(cout, generator=gen)).to(DEV)
    x = torch.zeros(N, H, W_, cpad(cin))
    x[..., :cin] = torch.randn(N, H, W_, cin, generator=gen).to(prec.dtype).float()
    be = hip()
    packed = ops.PackedWeights(spec.forward_plan(), DEV, prec.prec == L.PREC_BF16X3)
    be.pack_weights(packed, w)
    y = torch.empty((N, H, W_, cpad(cout)), dtype=prec.dtype, device=DEV)
    nch = be.conv_forward(packed, x.to(prec.dtype).to(DEV), y, H, W_, bias, L.ACT_NONE, L.ACT_NONE, prec.prec, splitk=1, want_stats=True)
    assert nch > 0, 'this case is expected to take the fused-statistics path'
    z = torch.empty_like(y)
    st = be.norm_forward(y, z, cout, L.NORM_INSTANCE, L.ACT_NONE, None, None, None, None, -1.0, None, ext_nchunks=nch)
    sync()
    sum_len = R.cdiv(H * W_, nch) + R.cdiv(R.cdiv(nch, 32), 4) + 2
    ref = R.Reference(y.float().cpu(), cout, L.NORM_INSTANCE, slack=SLACK, sum_len=sum_len)
    tag = f'{precname}/conditioning/fused-statistics'
    chk = Checker(tag, ref.ge)
    sb = ref.stat_bounds()
    for i, key in enumerate(('mean', 'rstd', 'scale', 'shift')):
        chk(key, st[i], ref.stats()[key], sb[key])
    z_ref, b_z = ref.forward(L.ACT_NONE, None, prec.dtype)
    chk('z', z, z_ref, b_z)
    chk.done()
    _record(record_property, tag, z, z_ref, b_z, st[1], ref)
