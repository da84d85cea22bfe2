"""tests/elementwise_ref.py held to account on the CPU (no GPU, not marked gpu):
  * its float64 reference agrees with torch's own float64 functionals and with torch.optim.Adam on float64 parameters over 5 steps, to float64 round-off;
  * its bounds hold for Emu, an fp32 emulation of each kernel's arithmetic written here from csrc/elementwise.hip -- operation by operation, with the
    summation order of the two-stage reductions (per-thread grid-stride sums, the wave butterfly, the LDS rows, the 8 lanes / 64 slices of the final kernels).
    It runs the case tables of tests/test_gpu_elementwise.py (all but the rows whose reference takes more than about a second here): the check that the chosen
    INPUTS keep the reference side inside the bound.  The worst err / bound of every case is recorded and must be <= 1;
  * the bounds are not vacuous: a named one-line perturbation of the emulation per operation is rejected by the comparer.  All of them are arithmetic changes
    on the CPU; none touches an index on a device."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R
from deepliif_amd import _lib as L

ERRLOG = {}
F32 = torch.float32
LANES = torch.arange(64)


def c32(v):
    return torch.tensor(v, dtype=F32)


def wave_sum(v, first=32):
    """__shfl_xor butterfly over the last axis (64 lanes), offsets first, first / 2 .. 1; every lane ends with the sum"""
    o = first
    while o > 0:
        v = v + v[..., LANES ^ o]
        o >>= 1
    return v


def thread_sums(vals, threads, max_trips=None):
    """grid-stride accumulation: thread i adds elements i, i + threads, ... in that order (missing elements are skipped: adding 0.f is the same)"""
    n = vals.numel()
    trips = -(-n // threads)
    if max_trips is not None:          # (a perturbation: the loop stops early)
        vals = vals.reshape(-1)[:max_trips * threads]
        n, trips = vals.numel(), min(trips, max_trips)
    pad = torch.zeros(trips * threads, dtype=F32)
    pad[:n] = vals.reshape(-1)
    acc = torch.zeros(threads, dtype=F32)
    for k in range(trips):
        acc = acc + pad[k * threads:(k + 1) * threads]
    return acc


def block_partials(vals, max_trips=None):
    """loss_kernel / kldiv_partial_kernel: 512 blocks x 256 threads -> wave_sum -> red[0] + red[1] + red[2] + red[3]"""
    acc = wave_sum(thread_sums(vals, R.LOSS_THREADS, max_trips).view(512, 4, 64))[..., 0]
    return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]


class Emu:
    """the kernels' fp32 arithmetic on CPU tensors (tanhf / expf / log1pf / sqrtf / powf are torch's fp32 functions).  `perturb` names ONE deliberate error."""

    def __init__(self, perturb=None):
        self.perturb = perturb

    # ---- activations (common.h apply_act / act_grad_from_output)
    def act_forward(self, act, x, y):
        v = x.float()
        if act == L.ACT_RELU:
            v = torch.where(v > 0, v, torch.zeros_like(v))
        elif act == L.ACT_LRELU:
            v = torch.where(v > 0, v, c32(0.25 if self.perturb == 'lrelu-slope' else 0.2) * v)
        elif act == L.ACT_TANH:
            v = torch.tanh(v)
        elif act == L.ACT_SIGMOID:
            v = c32(1.0) / (c32(1.0) + torch.exp(-v))
        y.copy_(v.to(y.dtype))

    def act_backward(self, act, dy, y, dx):
        g, o = dy.float(), y.float()
        if act == L.ACT_RELU:
            f = (o > 0).float()
        elif act == L.ACT_LRELU:
            f = torch.where(o > 0, c32(1.0), c32(0.25 if self.perturb == 'lrelu-slope' else 0.2))
        elif act == L.ACT_TANH:
            f = c32(1.0) - o * o
        elif act == L.ACT_SIGMOID:
            f = o * (c32(1.0) - o)
        else:
            f = torch.ones_like(o)
        dx.copy_((g * f).to(dx.dtype))

    # ---- attention gate
    def gate_forward(self, x, psi, out):
        out.copy_((x.float() * psi.float()[..., :1]).to(out.dtype))

    def gate_backward(self, g, x, psi, dx, dpsi):
        gv, xv = g.float(), x.float()
        cp = gv.shape[-1]
        cvec = cp // 8
        if dx is not None:
            dx.copy_((gv * psi.float()[..., :1]).to(dx.dtype))
        prod = (gv * xv).reshape(-1, cvec, 8)
        part = torch.zeros(prod.shape[:2], dtype=F32)
        for k in range(8):
            part = part + prod[..., k]
        lanes = torch.zeros(part.shape[0], 64, dtype=F32)
        lanes[:, :cvec] = part          # the cvec lanes of one pixel (aligned to cvec inside the wave: the xor offsets stay below cvec)
        first = cvec >> 1
        if self.perturb == 'dpsi-half-lanes':
            first >>= 1
        if first:
            lanes = wave_sum(lanes, first)
        d = torch.zeros(dpsi.shape, dtype=F32)
        d[..., 0] = lanes[:, 0].reshape(dpsi.shape[:-1])
        dpsi.copy_(d.to(dpsi.dtype))

    def axpby(self, alpha, a, beta, b, out):
        v = c32(alpha) * a.float()
        if b is not None:
            v = v + c32(beta) * b.float()
        out.copy_(v.to(out.dtype))

    def copy_channels(self, src, s_c0, dst, d_c0, nch, accumulate=False):
        v = src[..., s_c0:s_c0 + nch].float()
        if accumulate:
            v = v + dst[..., d_c0:d_c0 + nch].float()
        dst[..., d_c0:d_c0 + nch] = v.to(dst.dtype)

    def upsample2(self, src, dst, backward=False):
        if not backward:
            dst.copy_(src.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))
            return
        s = src.float()
        v = torch.zeros(dst.shape, dtype=F32)
        for q in range(4):
            v = v + s[:, (q >> 1)::2, (q & 1)::2]
        dst.copy_(v.to(dst.dtype))

    # ---- channel sums: channel_sum_partial_kernel (256 blocks; tpp threads per pixel, rows pixels per trip), channel_sum_final_kernel (8 lanes, double)
    def channel_sum(self, x, C_real, out, accumulate):
        cp = x.shape[-1]
        xv = x.float().reshape(-1, cp)
        npix, cvec = xv.shape[0], cp // 8
        assert cvec <= 256
        rows = 256 // cvec
        stride = R.CS_BLOCKS * rows
        trips = -(-npix // stride)
        if self.perturb == 'csum-first-trip-only':
            xv, npix, trips = xv[:stride], min(npix, stride), 1
        if self.perturb == 'csum-last-trip-dropped':
            trips -= 1
            xv, npix = xv[:trips * stride], trips * stride
        pad = torch.zeros(trips * stride, cp, dtype=F32)
        pad[:npix] = xv
        pad = pad.view(trips, R.CS_BLOCKS, rows, cp)
        s = torch.zeros(R.CS_BLOCKS, rows, cp, dtype=F32)
        for k in range(trips):
            s = s + pad[k]
        part = torch.zeros(R.CS_BLOCKS, cp, dtype=F32)
        for r in range(rows):
            if self.perturb == 'csum-skip-row' and r == 1:
                continue
            part = part + s[:, r]
        lane = torch.zeros(8, cp, dtype=F32)
        for j in range(R.CS_BLOCKS // 8):
            lane = lane + part.view(R.CS_BLOCKS // 8, 8, cp)[j]
        a = torch.zeros(cp, dtype=torch.float64)
        for r in range(8):
            a = a + lane[r].double()
        out.copy_(((out if accumulate else torch.zeros_like(out)) + a.float()[:C_real]))

    # ---- losses
    def loss(self, kind, x, target, target_const, C_real, loss_out, grad, grad_scale, out_scale=1.0, accumulate=False):
        v = x[..., :C_real].float()
        t = target[..., :C_real].float() if target is not None else torch.full_like(v, target_const)
        one, zero = c32(1.0), torch.zeros_like(v)
        if kind == L.LOSS_BCE_LOGITS:
            e = torch.exp(-v.abs())
            l = torch.maximum(v, zero) - v * t + torch.log1p(e)
            sig = torch.where(v >= 0, one / (one + e), e / (one + e))
            if self.perturb == 'bce-one-sigmoid-formula':
                sig = one / (one + e)
            g = sig - t
        elif kind == L.LOSS_MSE:
            d = v - t
            l, g = d * d, c32(2.0) * d
        elif kind == L.LOSS_LINEAR:
            l, g = t * v, t
        elif kind == L.LOSS_L1:
            d = v - t
            l, g = d.abs(), torch.sign(d)
        else:
            d = v - t
            ad = d.abs()
            inner = ad < (0.9 if self.perturb == 'smoothl1-threshold' else 1.0)
            l = torch.where(inner, c32(0.5) * d * d, ad - c32(0.5))
            g = torch.where(inner, d, torch.sign(d))
        inv = one / c32(float(v.numel()))
        part = block_partials(l).double()
        sl = torch.zeros(64, dtype=torch.float64)
        for i in range(8):          # 64 lanes, each the double sum of a contiguous slice of 8 partials
            sl = sl + part.view(64, 8)[:, i]
        tot = torch.zeros((), dtype=torch.float64)
        for i in range(64):
            if self.perturb == 'loss-drop-slice' and i == 63:
                continue
            tot = tot + sl[i]
        val = (tot * inv.double()).float() * c32(out_scale)
        loss_out[0] = loss_out[0] + val if accumulate else val
        if grad is not None:
            grad[..., :C_real] = (g * c32(grad_scale) * inv).to(grad.dtype)
            grad[..., C_real:] = 0

    def kldiv(self, x, t, C_real, loss_out, grad, grad_scale, out_scale=1.0, accumulate=False):
        xv, tv = x[..., :C_real].float(), t[..., :C_real].float()
        et, ex = torch.exp(tv), torch.exp(xv)
        one_trip = 1 if self.perturb == 'kl-first-trip-only' else None
        zx, zt, a = (block_partials(s, one_trip).double() for s in (ex, et, et * (tv - xv)))
        sums = []
        for part in (zx, zt, a):
            s = torch.zeros((), dtype=torch.float64)
            for i in range(512):
                s = s + part[i]
            sums.append(s)
        zx, zt, a = sums
        if self.perturb == 'kl-sign-of-A':
            a = -a
        val = (a / zt - torch.log(zt) + torch.log(zx)).float() * c32(out_scale)
        loss_out[0] = loss_out[0] + val if accumulate else val
        if grad is not None:
            izx, izt = (1.0 / zx).float(), (1.0 / zt).float()
            grad[..., :C_real] = (c32(grad_scale) * (ex * izx - et * izt)).to(grad.dtype)
            grad[..., C_real:] = 0

    # ---- Adam (adam_update, contraction off; the bias corrections as dl_adam_step / dl_adam_hyper compute them on the host)
    def adam_step(self, p, g, m, v, lr, b1, b2, eps, step, gscale):
        lr, b1, b2, eps, gscale, one = c32(lr), c32(b1), c32(b2), c32(eps), c32(gscale), c32(1.0)
        bc1 = one - torch.pow(b1, c32(float(step)))
        bc2_sqrt = torch.sqrt(one - torch.pow(b2, c32(float(step))))
        step_size = lr / bc1
        gi = g * gscale
        mi = b1 * m + (one - b1) * gi
        vi = b2 * v + (one - b2) * gi * gi
        m.copy_(mi)
        v.copy_(vi)
        denom = (torch.sqrt(vi) + eps) / bc2_sqrt if self.perturb == 'adam-eps-before-division' else torch.sqrt(vi) / bc2_sqrt + eps
        p.copy_(p - step_size * (mi / denom))

    def adam_hyper(self, lr, b1, b2, eps, step, gscale, hyper_host):
        self._hyper = (lr, b1, b2, eps, step, gscale)

    def adam_step_dev(self, p, g, m, v, hyper_dev):
        self.adam_step(p, g, m, v, *self._hyper)


# ------------------------------------------------------------------------------------------------ the reference against torch
def test_restated_enum_values_are_the_library_s():
    for name in dir(R.L):
        if name.startswith(('ACT_', 'LOSS_')):
            assert getattr(R.L, name) == getattr(L, name), name


def test_reference_agrees_with_torch_functionals():
    tol = 1e-13
    x = torch.randn(2, 5, 7, 8, generator=R.gen(1)).double() * 3
    t = torch.rand(2, 5, 7, 8, generator=R.gen(2)).double()
    C, n = 3, 2 * 5 * 7 * 3
    xc, tc = x[..., :C], t[..., :C]
    for kind, fn in ((L.LOSS_BCE_LOGITS, lambda: (xc.clamp_min(0) - xc * tc + torch.log1p(torch.exp(-xc.abs()))).mean()),
                     (L.LOSS_MSE, lambda: F.mse_loss(xc, tc)), (L.LOSS_LINEAR, lambda: (xc * tc).mean()), (L.LOSS_L1, lambda: F.l1_loss(xc, tc)),
                     (L.LOSS_SMOOTH_L1, lambda: F.smooth_l1_loss(xc, tc))):
        val, e_val, grad, b_grad = R.loss_ref(kind, x, t, 0.0, C, torch.float32, gscale=2.0, out_scale=0.5)
        assert abs(val - 0.5 * float(fn())) <= tol * max(1.0, abs(val)), kind
        manual = {L.LOSS_BCE_LOGITS: torch.sigmoid(xc) - tc, L.LOSS_MSE: 2 * (xc - tc), L.LOSS_LINEAR: tc, L.LOSS_L1: torch.sign(xc - tc),
                  L.LOSS_SMOOTH_L1: (xc - tc).clamp(-1, 1)}[kind]
        assert float((grad - 2.0 * manual / n).abs().max()) <= tol, kind
        assert e_val > 0 and float(b_grad.min()) >= 0
    xs, ts = torch.tanh(x), torch.tanh(t - 0.5)
    val, e_val, grad, _ = R.kldiv_ref(xs, ts, C, torch.float32, gscale=3.0)
    q, p = torch.softmax(xs[..., :C].reshape(-1), 0), torch.softmax(ts[..., :C].reshape(-1), 0)
    assert abs(val - float((p * (p.log() - q.log())).sum())) <= tol
    assert float((grad.reshape(-1) - 3.0 * (q - p)).abs().max()) <= tol
    for act, fn in ((L.ACT_RELU, F.relu), (L.ACT_LRELU, lambda v: F.leaky_relu(v, 0.2)), (L.ACT_TANH, torch.tanh), (L.ACT_SIGMOID, torch.sigmoid)):
        ref, _ = R.act_forward_ref(act, x)
        assert float((ref - fn(x)).abs().max()) <= tol
        xa = x.clone().requires_grad_(True)
        fn(xa).backward(t)
        y = fn(x)
        back, _ = R.act_backward_ref(act, t, y, torch.float32)
        assert float((back - xa.grad).abs().max()) <= 1e-12, act
    up, _ = R.upsample2_ref(x, False)
    assert torch.equal(up, F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode='nearest').permute(0, 2, 3, 1))
    xa = x.clone().requires_grad_(True)
    F.interpolate(xa.permute(0, 3, 1, 2), scale_factor=2, mode='nearest').permute(0, 2, 3, 1).backward(up)
    down, _ = R.upsample2_ref(up, True)
    assert float((down - xa.grad).abs().max()) <= tol


def test_reference_adam_agrees_with_torch_optim_over_five_steps():
    n = 1000
    p, _, m, v, _ = R.adam_state(n, tiny_v=False)
    for betas in R.ADAM_BETAS:
        lr, b1, b2, eps = R.f32(2e-4), R.f32(betas[0]), R.f32(betas[1]), R.f32(1e-8)
        pt = torch.nn.Parameter(p.double().clone())
        opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps)
        state = {'p': p.double(), 'm': torch.zeros(n, dtype=torch.float64), 'v': torch.zeros(n, dtype=torch.float64)}
        for step in range(1, 6):
            gr = torch.randn(n, generator=R.gen(step)).double()
            pt.grad = gr.clone()
            opt.step()
            state, _ = R.adam_ref(state['p'], gr * 4, state['m'], state['v'], lr, b1, b2, eps, step, 0.25)
            assert float((state['p'] - pt.detach()).abs().max()) <= 1e-15 + 1e-13 * float(pt.detach().abs().max()), (betas, step)


# ------------------------------------------------------------------------------------------------ the bounds hold for the emulation, on the GPU file's cases
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
NAME = {torch.float32: 'fp32', torch.bfloat16: 'bf16', torch.float16: 'fp16'}


def _chk(tag):
    return R.Checker(tag, ERRLOG)


def _vector_family(be, chk, shape, dtype, view):
    for act in R.ACTS:
        R.run_act_forward(be, 'cpu', chk, shape, dtype, act, view)
        R.run_act_backward(be, 'cpu', chk, shape, dtype, act, view)
    R.run_gate_forward(be, 'cpu', chk, shape, dtype, view)
    for with_b in (True, False):
        R.run_axpby(be, 'cpu', chk, shape, dtype, with_b, view)
    for bwd in (False, True):
        R.run_upsample2(be, 'cpu', chk, shape, dtype, bwd, view)


@pytest.mark.parametrize('dtype', DTYPES, ids=NAME.get)
def test_bounds_hold_for_the_emulation_vector_kernels(dtype):
    chk = _chk(f'{NAME[dtype]}/vector')
    for shape in R.VEC_SHAPES:
        _vector_family(Emu(), chk, shape, dtype, False)
    _vector_family(Emu(), chk, R.VIEW_SHAPE, dtype, True)
    for case in R.COPY_CASES[:3]:          # (the second-trip row is a plain copy at three million elements: nothing the small rows do not compute)
        for acc in (False, True):
            R.run_copy_channels(Emu(), 'cpu', chk, case, dtype, acc)
    assert chk.done() <= 1.0


@pytest.mark.parametrize('dtype', DTYPES[:2], ids=NAME.get)
def test_bounds_hold_for_the_emulation_gate_backward(dtype):
    chk = _chk(f'{NAME[dtype]}/gate-bwd')
    for pix, cp in R.GATE_BWD_CASES[:-1]:          # (without the 16.8 million elements of the second-trip row)
        R.run_gate_backward(Emu(), 'cpu', chk, pix + (cp,), dtype, False, True)
    R.run_gate_backward(Emu(), 'cpu', chk, (2, 9, 7, 64), dtype, True, False)
    assert chk.done() <= 1.0


@pytest.mark.parametrize('dtype', DTYPES[:2], ids=NAME.get)
def test_bounds_hold_for_the_emulation_channel_sum(dtype):
    chk = _chk(f'{NAME[dtype]}/csum')
    for case in R.CSUM_CASES:
        for acc in (False, True):
            R.run_channel_sum(Emu(), 'cpu', chk, case, dtype, acc)
    R.run_channel_sum(Emu(), 'cpu', chk, R.CSUM_CASES[2], dtype, True, mean=100.0, spread=1.0)
    R.run_channel_sum(Emu(), 'cpu', chk, R.CSUM_CASES[0], dtype, False, mean=100.0, spread=1.0)
    assert chk.done() <= 1.0


@pytest.mark.parametrize('dtype', DTYPES[:2], ids=NAME.get)
@pytest.mark.parametrize('kind', R.LOSS_KINDS, ids=R.LOSS_NAME.get)
def test_bounds_hold_for_the_emulation_losses(kind, dtype):
    chk = _chk(f'{NAME[dtype]}/loss/{R.LOSS_NAME[kind]}')
    for pix, C in R.LOSS_SHAPES:
        for with_target in (True, False):
            R.run_loss(Emu(), 'cpu', chk, kind, pix, C, dtype, with_target)
    R.run_loss(Emu(), 'cpu', chk, kind, (2, 30, 30), 3, dtype, True, view=True, gscale=1.0 / 1024)
    R.run_loss(Emu(), 'cpu', chk, kind, (2, 30, 30), 3, dtype, True, with_grad=False, out_scale=0.3, accumulate=True)
    R.run_loss(Emu(), 'cpu', chk, kind, (2, 30, 30), 1, dtype, False, view=True, gscale=10.0, out_scale=-2.5)
    assert chk.done() <= 1.0


@pytest.mark.parametrize('dtype', DTYPES[:2], ids=NAME.get)
def test_bounds_hold_for_the_emulation_kldiv(dtype):
    """with the near-zero case: the reference side of t = x + delta stays inside the absolute bound"""
    chk = _chk(f'{NAME[dtype]}/kl')
    for pix, C in R.KL_SHAPES[:4]:          # (without the 6.3 million elements of (8, 512, 512, 3))
        for near in (False, True):
            val, e_val = R.run_kldiv(Emu(), 'cpu', chk, pix, C, dtype, near, gscale=10.0)
            ERRLOG[f'{chk.tag}/{pix}-{near}'] = {'kl': val, 'bound': e_val}
            assert (1e-7 < val < 1e-4) if near else val > 0.05, (pix, near, val)
    R.run_kldiv(Emu(), 'cpu', chk, (1, 37, 53), 3, dtype, True, view=True, gscale=1.0 / 1024)
    R.run_kldiv(Emu(), 'cpu', chk, (1, 37, 53), 3, dtype, True, with_grad=False, out_scale=0.5, accumulate=True)
    assert chk.done() <= 1.0


def test_bounds_hold_for_the_emulation_adam():
    chk = _chk('fp32/adam')
    for n in R.ADAM_N[:5]:
        for step in R.ADAM_STEPS:
            for gs in R.ADAM_GSCALE:
                for betas in R.ADAM_BETAS:
                    if n <= 257 or (step, gs, betas) in ((1, 1.0, R.ADAM_BETAS[0]), (100000, R.ADAM_GSCALE[1], R.ADAM_BETAS[1])):
                        R.run_adam_step(Emu(), 'cpu', chk, n, step, gs, betas)
    for betas in R.ADAM_BETAS:
        R.run_adam_trajectory(Emu(), 'cpu', chk, 257, betas, 1.0 / 1024)
    assert chk.done() <= 1.0


# ------------------------------------------------------------------------------------------------ the bounds are not vacuous
PERTURBATIONS = {
    'lrelu-slope': lambda be, chk: R.run_act_forward(be, 'cpu', chk, R.VEC_SHAPES[0], torch.float32, L.ACT_LRELU),
    'bce-one-sigmoid-formula': lambda be, chk: R.run_loss(be, 'cpu', chk, L.LOSS_BCE_LOGITS, (2, 30, 30), 3, torch.float32, True),
    'smoothl1-threshold': lambda be, chk: R.run_loss(be, 'cpu', chk, L.LOSS_SMOOTH_L1, (2, 30, 30), 3, torch.float32, True),
    # at the second-trip shape, where all 64 slices hold data: the last slice (blocks 504 .. 511, one element per thread) is 1 / 97 of the mean
    'loss-drop-slice': lambda be, chk: R.run_loss(be, 'cpu', chk, L.LOSS_BCE_LOGITS, (2, 181, 182), 3, torch.float32, True),
    'kl-first-trip-only': lambda be, chk: R.run_kldiv(be, 'cpu', chk, (2, 181, 182), 3, torch.float32, True),
    'csum-first-trip-only': lambda be, chk: R.run_channel_sum(be, 'cpu', chk, R.CSUM_CASES[0], torch.float32, False),
    'csum-first-trip-only-mean100': lambda be, chk: R.run_channel_sum(be, 'cpu', chk, R.CSUM_CASES[0], torch.float32, True, mean=100.0, spread=1.0),
    'csum-last-trip-dropped': lambda be, chk: R.run_channel_sum(be, 'cpu', chk, R.CSUM_CASES[5], torch.bfloat16, True),
    'kl-sign-of-A': lambda be, chk: R.run_kldiv(be, 'cpu', chk, (1, 37, 53), 3, torch.float32, True),
    'adam-eps-before-division': lambda be, chk: R.run_adam_step(be, 'cpu', chk, 257, 2, 1.0, R.ADAM_BETAS[0], dev_variant=False),
    'csum-skip-row': lambda be, chk: R.run_channel_sum(be, 'cpu', chk, R.CSUM_CASES[2], torch.float32, False),
    'dpsi-half-lanes': lambda be, chk: R.run_gate_backward(be, 'cpu', chk, (2, 9, 11, 64), torch.float32),
}


@pytest.mark.parametrize('name', list(PERTURBATIONS))
def test_a_one_line_perturbation_is_rejected(name):
    """the same case passes with the emulation as it is, and has elements out of bound with the one arithmetic change"""
    good = R.Checker(name + '/unperturbed', {})
    PERTURBATIONS[name](Emu(), good)
    assert good.done() <= 1.0
    bad = R.Checker(name, {})
    PERTURBATIONS[name](Emu(name.replace('-mean100', '')), bad)
    assert max(bad.ratios.values()) > 1.0 and bad.reports, f'{name}: the perturbed emulation stayed inside the bound'
