"""The elementwise family (csrc/elementwise.hip: act_fwd / act_bwd, gate_fwd / gate_bwd, axpby, copy_channels, upsample2, channel_sum_partial / _final, loss and
loss_final, the three kldiv kernels, adam and adam_dev) through ops.impl(), element by element against the float64 reference under the derived bounds of
tests/elementwise_ref.py -- no element may be out of bound, SLACK = 1; what the kernels compute exactly is compared bit for bit.  The cases (elementwise_ref's
tables) reach the second trip of every grid-stride loop, channel-slice views whose pixel strides differ per operand, the tpp / rows splits of the channel sum,
partly dead last waves of the gate's butterfly, and the branches random data does not: x == target, |d| next to 1, logits of +-30 and 0, y == 0 after a ReLU,
g = 0 on m = v = 0, a KL divergence near 1e-6.  tests/test_elementwise_ref_host.py holds reference and bounds to torch and to an emulation of the kernels' arithmetic.

The test_math_* sweeps MEASURE the device math functions (their error cannot be derived from the source) and record the worst error in fp32 ulps; the constants of
elementwise_ref are twice the recorded values, rounded up to a power of two.  The worst err / bound of every case goes to parity_errors_elementwise.json in the
directory $DL_PARITY_DIR names (default parity_out/); a copy of the MI355X run is kept as profiles/elementwise_parity/parity_errors_elementwise.json.  DL_TEST_DRYRUN=1 runs the file on the CPU with the formula emulation in the kernels' place.

Out of scope: maxpool (already bit-exact against torch), the dropout masks (test_gpu_dropout_fused.py), the folds (pad_ref), shift_sum / shift_stack /
convt4_gather (covered through the narrow-conv and wgrad references) and the probes."""
import json
import os

import pytest
import torch

import elementwise_ref as R
from deepliif_amd import _lib as L
from deepliif_amd import ops
from deepliif_amd.engine import Precision

from test_gpu_kernels import DEV, DRY, hip, sync

pytestmark = pytest.mark.gpu
ERRLOG = {}
ERRLOG_DIR = os.environ.get('DL_PARITY_DIR', 'parity_out')
SLACK = 1                # the bounds are used as derived (elementwise_ref.SLACK multiplies their rounding counts)
assert R.SLACK == SLACK
PRECS = ['fp32', 'bf16']


@pytest.fixture(autouse=True)
def _real_backend_again():
    yield
    ops._impl = None


@pytest.fixture(autouse=True, scope='module')
def _errlog():
    yield
    os.makedirs(ERRLOG_DIR, exist_ok=True)
    with open(os.path.join(ERRLOG_DIR, 'parity_errors_elementwise.json'), 'w') as f:
        json.dump(ERRLOG, f, indent=1, sort_keys=True)


def _dtype(precname):
    return Precision.get(precname).dtype


def _sid(shape):
    return 'x'.join(str(s) for s in shape)


def _checker(tag):
    return R.Checker(tag, ERRLOG)


# ------------------------------------------------------------------------------------------------ the device math functions, measured
def _record(tag, err, unit, const):
    ulps = float((err / unit).max())
    ERRLOG[tag] = {'worst_ulps': round(ulps, 4), 'constant': const}
    print(f'{tag}: worst error {ulps:.4f} fp32 ulps (constant {const:g})')
    assert ulps <= const, (tag, ulps, const)


@pytest.mark.parametrize('act,lim', [(L.ACT_TANH, 10.0), (L.ACT_SIGMOID, 30.0)], ids=['tanh', 'sigmoid'])
def test_math_activation(act, lim):
    """tanhf, and 1 / (1 + __expf(-v)) as a whole: act_forward in fp32 over a dense sweep of the argument"""
    n = 1 << 20
    x = torch.cat([torch.linspace(-lim, lim, n - 4096), torch.randn(4096, generator=R.gen(1)) * 2.0 ** -6]).view(1, n // 512, 1, 512)
    y = torch.empty(x.shape, device=DEV)
    hip().act_forward(act, x.to(DEV), y)
    sync()
    ref = R.act64(act, x.double())
    _record('math/' + R.ACT_NAME[act], (y.double().cpu() - ref).abs(), R.ulp32(ref), R.TANH_ULPS if act == L.ACT_TANH else R.SIGMOID_ULPS)


def test_math_expf():
    """expf over [-30, 1] through kldiv's gradient: element 0 holds the whole teacher mass (t = 80 against -80), so every other element reads
    gscale (expf(x) izx - 0) with izx the fp32 value the kernel left in its workspace: expf and one product rounding"""
    n = 1 << 18
    x = torch.zeros(1, n // 8, 1, 8)
    x.view(-1)[:] = torch.linspace(-30.0, 1.0, n)
    t = torch.full_like(x, -80.0)
    t.view(-1)[0] = 80.0
    out, grad = torch.zeros(1, device=DEV), torch.empty(x.shape, device=DEV)
    be = hip()
    be.kldiv(x.to(DEV), t.to(DEV), 8, out, grad, 1.0)
    sync()
    ex = torch.exp(x.double())
    if DRY:
        izx = float((1.0 / ex.sum()).float())
    else:
        izx = float(ops.WS.get('kldiv_ws', 0, grad.device)[3 * R.LOSS_THREADS // 256].cpu())          # stats[0] = 1 / Zx behind the 3 x LOSS_BLOCKS partials
        assert abs(izx * float(ex.sum()) - 1) < 1e-3
    ref = (ex * izx).view(-1)[1:]
    _record('math/expf', (grad.double().cpu().view(-1)[1:] - ref).abs(), R.ulp32(ref), R.EXP_ULPS)


def test_math_softplus():
    """log1pf(expf(-|v|)) over [-30, 0]: the BCE loss of single-element tensors with target 0 (the mean of one element is the element, every other term is 0)"""
    n = 2048
    v = torch.linspace(-30.0, 0.0, n)
    x = torch.zeros(n, 1, 1, 8)
    x[:, 0, 0, 0] = v
    xd, out = x.to(DEV), torch.zeros(n, device=DEV)
    be = hip()
    for i in range(n):
        be.loss(L.LOSS_BCE_LOGITS, xd[i:i + 1], None, 0.0, 1, out[i:i + 1], None, 1.0)
    sync()
    ref = torch.log1p(torch.exp(v.double()))
    _record('math/softplus', (out.double().cpu() - ref).abs(), R.ulp32(ref), R.SOFTPLUS_ULPS)


def test_math_sqrt():
    """sqrtf and one quotient: adam_step with step_size = 1 (lr = 1/2, beta1 = 1/2, step 1), bc2_sqrt = 1/2 (beta2 = 3/4), eps = 0, g = 0, p = 0 leaves
    p = -(m' / (sqrtf(v') / 0.5f)) with m', v' the stored moments -- read back, so only the square root and the quotient are between them and p"""
    n = 1 << 20
    ge = R.gen(2)
    v = torch.exp2(torch.rand(n, generator=ge) * 110 - 100)
    m = torch.randn(n, generator=ge)
    p, gr = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    md, vd = m.to(DEV), v.to(DEV)
    hip().adam_step(p, gr, md, vd, 0.5, 0.5, 0.75, 0.0, 1, 1.0)
    sync()
    ref = -(md.double().cpu() / (vd.double().cpu().sqrt() / 0.5))
    _record('math/sqrt', (p.double().cpu() - ref).abs(), R.ulp32(ref), R.SQRT_ULPS)


def test_math_powf():
    """1.f - powf(beta, step) as dl_adam_hyper (and dl_adam_step) compute it on the host, steps 1 .. 100 000"""
    be = hip()
    steps = sorted(set(range(1, 3000)) | {min(int(round(1.003 ** k)), 100000) for k in range(2300, 3845)})
    hyper = torch.zeros(8)
    err, unit = [], []
    for b in (R.f32(0.9), R.f32(0.999), R.f32(0.99)):
        for s in steps:
            be.adam_hyper(2e-4, b, b, 1e-8, s, 1.0, hyper)
            pw = b ** s
            err.append(abs(float(hyper[4]) - (1.0 - pw)))
            unit.append(R.pow_unit(pw, 1.0 - pw))
    _record('math/powf', torch.tensor(err, dtype=torch.float64), torch.tensor(unit, dtype=torch.float64), R.POW_ULPS)


# ------------------------------------------------------------------------------------------------ the vector kernels
def _vector_family(be, chk, shape, dtype, view, forward_only=False):
    for act in R.ACTS:
        R.run_act_forward(be, DEV, chk, shape, dtype, act, view, sync)
        if not forward_only:
            R.run_act_backward(be, DEV, chk, shape, dtype, act, view, sync)
    R.run_gate_forward(be, DEV, chk, shape, dtype, view, sync)
    for with_b in (True, False):
        R.run_axpby(be, DEV, chk, shape, dtype, with_b, view, sync)
    R.run_upsample2(be, DEV, chk, shape, dtype, False, view, sync)
    if not forward_only:
        R.run_upsample2(be, DEV, chk, shape, dtype, True, view, sync)


@pytest.mark.parametrize('precname', PRECS)
@pytest.mark.parametrize('shape', R.VEC_SHAPES, ids=_sid)
def test_vector_kernels(shape, precname):
    chk = _checker(f'{precname}/vector/{_sid(shape)}')
    _vector_family(hip(), chk, shape, _dtype(precname), False)
    chk.done()


@pytest.mark.parametrize('precname', PRECS)
def test_vector_kernels_on_channel_slices(precname):
    """every operand a channel slice of a wider buffer, each with its own width: what lies outside the slices keeps its sentinel"""
    chk = _checker(f'{precname}/vector-views/{_sid(R.VIEW_SHAPE)}')
    _vector_family(hip(), chk, R.VIEW_SHAPE, _dtype(precname), True)
    chk.done()


BIG_RUNS = {
    'act_fwd': lambda be, chk, dt: R.run_act_forward(be, DEV, chk, R.BIG_SHAPE, dt, R.BIG_ACT, False, sync),
    'act_bwd': lambda be, chk, dt: R.run_act_backward(be, DEV, chk, R.BIG_SHAPE, dt, R.BIG_ACT, False, sync),
    'gate_fwd': lambda be, chk, dt: R.run_gate_forward(be, DEV, chk, R.BIG_SHAPE, dt, False, sync),
    'axpby': lambda be, chk, dt: R.run_axpby(be, DEV, chk, R.BIG_SHAPE, dt, True, False, sync),
    'upsample2_fwd': lambda be, chk, dt: R.run_upsample2(be, DEV, chk, R.BIG_SHAPE, dt, False, False, sync),
    'upsample2_bwd': lambda be, chk, dt: R.run_upsample2(be, DEV, chk, R.BIG_SHAPE, dt, True, False, sync),
}


@pytest.mark.parametrize('precname', PRECS)
@pytest.mark.parametrize('kernel', list(BIG_RUNS))
def test_vector_kernels_second_trip(kernel, precname):
    """2 099 200 vectors against 8192 x 256 threads: the last 2 048 take the second trip of the grid-stride loop (one activation only)"""
    chk = _checker(f'{precname}/second-trip/{kernel}')
    BIG_RUNS[kernel](hip(), chk, _dtype(precname))
    chk.done()


@pytest.mark.parametrize('shape', R.VEC_SHAPES + [R.VIEW_SHAPE], ids=_sid)
def test_forward_kernels_of_the_f16_library(shape):
    """the inference policy's library (the same sources, IEEE half as the 16-bit type): the forward kernels inference reaches"""
    chk = _checker(f'fp16/vector/{_sid(shape)}')
    with ops.half_mode('fp16'):
        be = hip()
        assert DRY or be.half == 'fp16'
        _vector_family(be, chk, shape, torch.float16, shape == R.VIEW_SHAPE, forward_only=True)
        for case in R.COPY_CASES[:3]:
            for acc in (False, True):
                R.run_copy_channels(be, DEV, chk, case, torch.float16, acc, sync)
    chk.done()


@pytest.mark.parametrize('precname', PRECS)
@pytest.mark.parametrize('accumulate', [False, True], ids=['copy', 'accumulate'])
@pytest.mark.parametrize('case', R.COPY_CASES, ids=lambda c: f'{_sid(c[0])}-s{c[1]}+{c[2]}-d{c[3]}+{c[4]}-c{c[5]}')
def test_copy_channels(case, accumulate, precname):
    """offsets and widths that are no multiple of 8 on both sides; the rest of the destination and the source stay as they were"""
    chk = _checker(f'{precname}/copy/{_sid(case[0])}-c{case[5]}-{"acc" if accumulate else "copy"}')
    R.run_copy_channels(hip(), DEV, chk, case, _dtype(precname), accumulate, sync)
    chk.done()


# ------------------------------------------------------------------------------------------------ gate_backward
@pytest.mark.parametrize('precname', PRECS)
@pytest.mark.parametrize('case', R.GATE_BWD_CASES, ids=lambda c: f'{_sid(c[0])}x{c[1]}')
def test_gate_backward(case, precname):
    """Cp 8 .. 512 (1 .. 64 lanes per pixel); 1, 7 and 63 pixels of one lane each leave the last wave partly dead; 4 097 pixels x 64 lanes; 32 800 pixels x
    64 lanes take the second trip of the `rounded` loop; dpsi channel 0 under the reduction bound, channels 1 .. 7 exactly zero"""
    pix, cp = case
    chk = _checker(f'{precname}/gate-bwd/{_sid(pix)}x{cp}')
    R.run_gate_backward(hip(), DEV, chk, pix + (cp,), _dtype(precname), False, True, sync)
    chk.done()


@pytest.mark.parametrize('precname', PRECS)
@pytest.mark.parametrize('cp', [8, 64])
def test_gate_backward_without_dx_and_on_channel_slices(cp, precname):
    chk = _checker(f'{precname}/gate-bwd-variants/{cp}')
    be, dtype = hip(), _dtype(precname)
    R.run_gate_backward(be, DEV, chk, (2, 9, 7, cp), dtype, False, False, sync)          # dx = None
    R.run_gate_backward(be, DEV, chk, (2, 9, 7, cp), dtype, True, True, sync)            # strided g, x, psi, dx, dpsi
    R.run_gate_backward(be, DEV, chk, (2, 9, 7, cp), dtype, True, False, sync)
    chk.done()


# ------------------------------------------------------------------------------------------------ channel_sum
@pytest.mark.parametrize('precname', PRECS)
@pytest.mark.parametrize('case', R.CSUM_CASES, ids=lambda c: f'cp{c[0]}-{_sid(c[1])}-c{c[2]}{"-view" if c[3] else ""}')
def test_channel_sum(case, precname):
    """tpp = 1 / rows = 256 with a second trip, 4 / 64, 64 / 4 with a second trip, fewer pixels than rows, a strided view of nine trips; onto and over
    preloaded values.  The pixels past the first trip of the grid carry a same-signed weight that outweighs the bound (run_channel_sum), so a trip that is
    dropped is out of bound: tests/test_elementwise_ref_host.py, 'csum-first-trip-only' and 'csum-last-trip-dropped'"""
    chk = _checker(f'{precname}/csum/cp{case[0]}-{_sid(case[1])}-c{case[2]}')
    for acc in (False, True):
        R.run_channel_sum(hip(), DEV, chk, case, _dtype(precname), acc, sync=sync)
    chk.done()


@pytest.mark.parametrize('precname', PRECS)
def test_channel_sum_conditioning(precname):
    """channel mean 100 against a spread of 1: the sum's magnitude is the sum of the magnitudes, the bound is met where a centred sum would cancel"""
    chk = _checker(f'{precname}/csum/conditioning')
    R.run_channel_sum(hip(), DEV, chk, R.CSUM_CASES[2], _dtype(precname), True, mean=100.0, spread=1.0, sync=sync)
    R.run_channel_sum(hip(), DEV, chk, R.CSUM_CASES[0], _dtype(precname), False, mean=100.0, spread=1.0, sync=sync)
    chk.done()


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize('precname', PRECS)
@pytest.mark.parametrize('case', R.LOSS_SHAPES, ids=lambda c: f'{_sid(c[0])}-c{c[1]}')
@pytest.mark.parametrize('kind', R.LOSS_KINDS, ids=R.LOSS_NAME.get)
def test_loss(kind, case, precname):
    """the five kinds with a target tensor and with a constant: the gradient per element, the scalar under the reduction bound, the padding channels exactly 0"""
    pix, C = case
    chk = _checker(f'{precname}/loss/{R.LOSS_NAME[kind]}/{_sid(pix)}-c{C}')
    for with_target in (True, False):
        R.run_loss(hip(), DEV, chk, kind, pix, C, _dtype(precname), with_target, sync=sync)
    chk.done()


@pytest.mark.parametrize('precname', PRECS)
@pytest.mark.parametrize('kind', R.LOSS_KINDS, ids=R.LOSS_NAME.get)
def test_loss_variants(kind, precname):
    """strided x, target and gradient; no gradient; out_scale with accumulate; grad_scale != 1"""
    chk = _checker(f'{precname}/loss-variants/{R.LOSS_NAME[kind]}')
    be, dtype, pix = hip(), _dtype(precname), (2, 30, 30)
    R.run_loss(be, DEV, chk, kind, pix, 3, dtype, True, view=True, gscale=1.0 / 1024, sync=sync)
    R.run_loss(be, DEV, chk, kind, pix, 3, dtype, True, with_grad=False, out_scale=0.3, accumulate=True, sync=sync)
    R.run_loss(be, DEV, chk, kind, pix, 1, dtype, False, view=True, gscale=10.0, out_scale=-2.5, sync=sync)
    chk.done()


# ------------------------------------------------------------------------------------------------ KL divergence
@pytest.mark.parametrize('precname', PRECS)
@pytest.mark.parametrize('near', [False, True], ids=['independent', 'near-zero'])
@pytest.mark.parametrize('case', R.KL_SHAPES, ids=lambda c: f'{_sid(c[0])}-c{c[1]}')
def test_kldiv(case, near, precname):
    """independent student and teacher (KL about 0.3), and t = x + delta with 0 <= delta <= 2^-7, where the loss is about 1e-6 while log Zx and log Zt
    are about log N: the scalar is held to the ABSOLUTE bound propagated through A / Zt - log Zt + log Zx.  The three sums are bounded along the kernel's
    fixed tree (elementwise_ref.sum_len: trips + 9 roundings, not one per addend), so the bound stays near 1e-6 at every shape and a dropped second trip is
    out of bound in the near-zero scalar as well as in the independent case's gradient (tests/test_elementwise_ref_host.py, 'kl-first-trip-only')"""
    pix, C = case
    chk = _checker(f'{precname}/kl/{_sid(pix)}-c{C}-{"near" if near else "independent"}')
    val, e_val = R.run_kldiv(hip(), DEV, chk, pix, C, _dtype(precname), near, gscale=10.0, sync=sync)
    ERRLOG[chk.tag + '/value'] = {'kl': val, 'bound': e_val}
    chk.done()


@pytest.mark.parametrize('precname', PRECS)
def test_kldiv_variants(precname):
    chk = _checker(f'{precname}/kl-variants')
    be, dtype = hip(), _dtype(precname)
    R.run_kldiv(be, DEV, chk, (1, 37, 53), 3, dtype, True, view=True, gscale=1.0 / 1024, sync=sync)
    R.run_kldiv(be, DEV, chk, (1, 37, 53), 3, dtype, True, with_grad=False, out_scale=0.5, accumulate=True, sync=sync)
    R.run_kldiv(be, DEV, chk, (1, 16, 16), 8, dtype, False, view=True, out_scale=-2.0, sync=sync)
    chk.done()


# ------------------------------------------------------------------------------------------------ Adam
ADAM_COMBOS = [(gs, b) for gs in R.ADAM_GSCALE for b in R.ADAM_BETAS]


@pytest.mark.parametrize('step', R.ADAM_STEPS)
@pytest.mark.parametrize('n', R.ADAM_N)
def test_adam_step(n, step):
    """one step from a given fp32 state against the float64 update of that state; g = 0 on m = v = 0 leaves p bit for bit; v near the smallest normal;
    adam_step_dev with adam_hyper is bit-identical (a statement about the two KERNELS: in the dry run the emulation calls one function for both, and
    only the hyper tensor's slot layout is exercised).  Up to 257 elements every (grad_scale, betas) pair runs, above that one pair per (n, step)."""
    chk = _checker(f'fp32/adam/n{n}-step{step}')
    k = R.ADAM_N.index(n) + R.ADAM_STEPS.index(step)
    for gs, betas in (ADAM_COMBOS if n <= 257 else [ADAM_COMBOS[k % 4]]):
        R.run_adam_step(hip(), DEV, chk, n, step, gs, betas, sync=sync)
    chk.done()


@pytest.mark.parametrize('betas', R.ADAM_BETAS, ids=lambda b: f'b{b[0]}')
def test_adam_trajectory(betas):
    chk = _checker(f'fp32/adam-trajectory/b{betas[0]}')
    for n, gs in ((257, 1.0), (100003, 1.0 / 1024)):
        R.run_adam_trajectory(hip(), DEV, chk, n, betas, gs, sync=sync)
    chk.done()
