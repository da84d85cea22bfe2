"""Replicate padding on the MI355X, kernel by kernel, against the float64 reference of tests/pad_ref.py (F.conv2d(F.pad(x, mode='replicate'), w) and
torch.autograd on it) at the derived per-element bound of tests/conv_ref.py -- sum_slack 1, operands pre-rounded to the 16-bit format:
  * the forward on conv_gemm_w4_kernel<.., DL_PAD_REPLICATE> (border inside the kernel: clamped slab rows, one redirected fragment lane per outer tap), with the
    zero-padding launch of the same data on conv_gemm_w4_kernel as control and as the bit-exact twin of every interior output;
  * the forward on the generic kernels (widths / channel counts the w4 kernel does not serve, H = 1, the strict policy);
  * dl_replicate_fold and the data gradient (pad-0 plan over the padded extent, fp32 accumulators, fold);
  * the weight gradient on wgrad_w4_kernel<DL_PAD_REPLICATE> (no skipped rows, clamped x row, edge pieces), single, split and batched, and on the generic kernel.
Control rule: if the zero-padding launch of a w4 / wgrad_w4 case exceeded the bound, that would be a finding about the existing kernel and the replicate case
would be held to twice the control's ratio.  Every control is asserted to be inside the bound, so the replicate cases hold the bound itself; each test prints
its worst err / bound ratios (DESIGN 4.9 quotes them)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import pad_ref as PR
import replicate_cases as RC
from deepliif_amd import _lib as L
from deepliif_amd import ops
from deepliif_amd.geometry import ConvSpec, choose_wgrad_batch_splitk, cpad

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DT = {'bf16': torch.bfloat16, 'fp16': torch.float16}
U32 = 2.0 ** -24


def rnd(shape, seed, dtype, scale=1.0):
    """N(0, scale) values exactly representable in `dtype` (fp32 master copy)"""
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    return t.to(dtype).float()


class Lib:
    """the backend of one 16-bit format for the duration of a test"""

    def __init__(self, half):
        self.half, self.cm = half, ops.half_mode(half)

    def __enter__(self):
        self.cm.__enter__()
        if self.half == 'bf16':
            ops._impl = None
        return ops.impl()

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        return self.cm.__exit__(*exc)


def launch(be, mode, x, w, bias, act, prec, hw, want_stats=False):
    """dl_conv_forward of the 3x3 stride-1 layer with the given border on x (NHWC device tensor, possibly a channel slice) -> (y, kernel name, stats chunks)"""
    cout, cin = w.shape[0], w.shape[1]
    plan = ConvSpec('conv', cin, cout, 3, 1, 1, RC.PAD[mode]).forward_plan()
    packed = ops.PackedWeights(plan, DEV, prec == L.PREC_BF16X3)
    be.pack_weights(packed, w.to(DEV))
    y = torch.empty((x.shape[0], hw[0], hw[1], cpad(cout)), dtype=x.dtype, device=DEV)
    nch = be.conv_forward(packed, x, y, hw[0], hw[1], None if bias is None else bias.to(DEV), act, L.ACT_NONE, prec, splitk=1, want_stats=want_stats)
    return y, be.last_conv_kernel, nch


# ------------------------------------------------------------------------------------------------ forward on the w4 kernel
# N, H, W, Ci, Co, width of the buffer x is a channel slice of (None: dense), bias + ReLU, fused statistics
W4_CASES = [
    (1, 2, 128, 64, 256, None, False),       # one tile, both rows are border rows
    (2, 4, 128, 128, 256, 192, False),       # tiles meet at an image boundary (the clamp must stay inside the image); two K chunks; channel-slice view
    (1, 6, 128, 64, 512, None, True),        # two N-tiles; bias + ReLU; fused statistics against float64 sums
]


def _w4_inputs(case, dtype):
    n, h, w_, ci, co, wide, extras = case
    x = rnd((n, h, w_, ci), 21, dtype)
    wt = rnd((co, ci, 3, 3), 22, dtype, 0.05)
    bias = rnd((co,), 23, torch.bfloat16, 0.5) if extras else None
    return x, wt, bias


def _as_view(x, wide, dtype):
    if wide is None:
        return x.to(dtype).to(DEV)
    buf = torch.full(x.shape[:3] + (wide,), 7.0, dtype=dtype, device=DEV)          # whatever surrounds the slice must not be read
    off = wide - x.shape[3]
    buf[..., off:] = x.to(dtype).to(DEV)
    return buf[..., off:]


def _zero_on_w4(be, case, x, wt, bias, act, dtype):
    """the zero-padding launch of the same data ON conv_gemm_w4_kernel: the dispatch gives zero padding that kernel only from 224 tiles on, so the case's images
    lead a batch that is filled up with copies of themselves (tiles are computed independently of each other); returns the case's own images"""
    n, h, w_, ci, co, wide, _ = case
    per_image = (h * w_ // 256) * (co // 256)
    reps = -(-224 // (n * per_image))
    xb = x.repeat(reps, 1, 1, 1)
    y, name, _ = launch(be, 'zero', _as_view(xb, wide, dtype), wt, bias, act, L.PREC_BF16, (h, w_))
    assert name == RC.W4, name
    return y[:n]


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('case', W4_CASES, ids=lambda c: 'n%d-%dx%d-ci%d-co%d' % c[:5])
def test_forward_on_the_w4_kernel(case, half):
    n, h, w_, ci, co, wide, extras = case
    dtype = DT[half]
    x, wt, bias = _w4_inputs(case, dtype)
    act = L.ACT_RELU if extras else L.ACT_NONE
    with Lib(half) as be:
        got, name, _ = launch(be, 'replicate', _as_view(x, wide, dtype), wt, bias, act, L.PREC_BF16, (h, w_))
        assert name == RC.W4, name
        ctl = _zero_on_w4(be, case, x, wt, bias, act, dtype)
        torch.cuda.synchronize()
        # control: the existing zero-padding instantiation through the same comparer
        ref0, S0, K0 = PR.forward(x, wt, bias, relu=extras, mode='zero')
        # (conv_ref's K counts the taps that fall into the zero padding as exact zeros; 9 * Ci (+ 1) bounds it from above at the border and equals it inside)
        worst0, rep0 = PR.compare(ctl, ref0, PR.bound(ref0, S0, K0, dtype))
        ref, S, K = PR.forward(x, wt, bias, relu=extras, mode='replicate')
        assert K == 9 * ci + (1 if extras else 0)
        worst, rep = PR.compare(got, ref, PR.bound(ref, S, K, dtype))
        print(f'w4 forward {case[:5]} {half}: replicate err/bound {worst:.3f}, zero-padding control {worst0:.3f}')
        limit = 1.0 if worst0 <= 1.0 else 2.0 * worst0
        assert worst <= limit, f'control {worst0:.3f}\n{rep}'
        assert worst0 <= 1.0, 'the zero-padding control itself is out of bound (a finding about the existing kernel):\n' + rep0
        # interior bit-identity: away from the border the two instantiations run the same arithmetic on the same slab
        if h > 2:
            assert torch.equal(got[:, 1:h - 1, 1:w_ - 1], ctl[:, 1:h - 1, 1:w_ - 1])
        assert not torch.equal(got[:, 0], ctl[:, 0]) and not torch.equal(got[:, :, 0], ctl[:, :, 0]) and not torch.equal(got[:, :, -1], ctl[:, :, -1])
        if not extras:
            return
        # fused statistics (no activation in front of a norm): per-(image, channel) sums of exactly the stored values against float64 sums
        y, name, nch = launch(be, 'replicate', _as_view(x, wide, dtype), wt, bias, L.ACT_NONE, L.PREC_BF16, (h, w_), want_stats=True)
        assert name == RC.W4 and nch == h * w_ // 256
        z = torch.empty_like(y)
        st = be.norm_forward(y, z, co, L.NORM_INSTANCE, L.ACT_NONE, None, None, None, None, -1.0, None, ext_nchunks=nch)
        torch.cuda.synchronize()
        y64 = y.double().cpu()
        npix = h * w_
        mean64, sq64 = y64.mean(dim=(1, 2)), (y64 * y64).mean(dim=(1, 2))
        # fp32 sums of npix stored values in any order: |err| <= npix * 2^-24 * mean|y| for the mean; the variance E[y^2] - mean^2 inherits the same relative
        # error of both sums, amplified by (E[y^2] + mean^2) / var (<= 3 for these N(0, ~1.7) outputs with |bias| ~ 0.5): 1e-4 relative on rstd is 10 x that
        tol_mean = npix * U32 * y64.abs().mean(dim=(1, 2)) + U32
        assert bool(((st[0].double().cpu() - mean64).abs() <= tol_mean).all())
        rstd64 = 1.0 / torch.sqrt(sq64 - mean64 * mean64 + 1e-5)
        assert float(((st[1].double().cpu() - rstd64).abs() / rstd64).max()) < 1e-4


# ------------------------------------------------------------------------------------------------ forward on the generic kernels
GENERIC = [(2, 40, 24, 32, 32), (1, 1, 5, 8, 8), (1, 8, 128, 32, 64)]      # widths the w4 kernel does not serve; H = 1: all three rows clamp to row 0; eligible width, ineligible Ci


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('shape', GENERIC, ids=lambda s: 'n%d-%dx%d-ci%d-co%d' % s)
def test_forward_on_the_generic_kernels(shape, half):
    n, h, w_, ci, co = shape
    dtype = DT[half]
    x = torch.zeros(n, h, w_, cpad(ci))
    x[..., :ci] = rnd((n, h, w_, ci), 31, dtype)
    wt, bias = rnd((co, ci, 3, 3), 32, dtype, 0.1), rnd((co,), 33, torch.bfloat16, 0.5)
    with Lib(half) as be:
        for b, act in ((None, L.ACT_NONE), (bias, L.ACT_RELU)):
            got, name, _ = launch(be, 'replicate', x.to(dtype).to(DEV), wt, b, act, L.PREC_BF16, (h, w_))
            torch.cuda.synchronize()
            assert name != RC.W4 and name.startswith('conv_gemm'), name
            ref, S, K = PR.forward(x, wt, b, relu=act == L.ACT_RELU)
            worst, rep = PR.compare(got, ref, PR.bound(ref, S, K, dtype))
            print(f'generic forward {shape} {half} {name}: err/bound {worst:.3f}')
            assert worst <= 1.0, rep


def test_forward_under_the_strict_policy():
    """fp32 storage, split-bf16 x3 products: operands that are exact in bf16 have a zero low part, so every product is exact and what remains is the fp32
    summation: K * 2^-24 * S + 2^-24 * |ref| (no 16-bit store)"""
    n, h, w_, ci, co = 2, 40, 24, 32, 32
    x, wt = rnd((n, h, w_, ci), 41, torch.bfloat16), rnd((co, ci, 3, 3), 42, torch.bfloat16, 0.1)
    with Lib('bf16') as be:
        got, name, _ = launch(be, 'replicate', x.to(DEV), wt, None, L.ACT_NONE, L.PREC_BF16X3, (h, w_))
        torch.cuda.synchronize()
        assert 'x3' in name or name == 'conv_gemm_kernel<f32>', name
        ref, S, K = PR.forward(x, wt)
        worst, rep = PR.compare(got, ref, S.mul_(K * U32).add_(ref.abs(), alpha=U32).add_(U32))
        print(f'strict forward {name}: err/bound {worst:.3f}')
        assert worst <= 1.0, rep


# ------------------------------------------------------------------------------------------------ fold and data gradient
@pytest.mark.parametrize('kind', ['bf16', 'fp16', 'fp32', 'bf16<-fp32', 'fp16<-fp32'])
@pytest.mark.parametrize('shape,pad', [((1, 1, 1, 8), 1), ((2, 3, 5, 16), 1), ((1, 4, 4, 8), 3)], ids=['9-to-1', 'ragged', 'pad>=H-1'])
def test_replicate_fold(shape, pad, kind):
    """dl_replicate_fold against autograd of F.pad(mode='replicate') in float64.  Up to (pad + 1)^2 (or (2 pad + 1)^2 on a one-pixel map) source values are
    summed in fp32 and stored once: T * 2^-24 * sum |src| + u * |ref| + 2^-24"""
    n, h, w_, c = shape
    dst_kind, _, src_kind = kind.partition('<-')
    half = dst_kind if dst_kind in DT else 'bf16'
    ddt = DT.get(dst_kind, torch.float32)
    sdt = torch.float32 if (src_kind or dst_kind == 'fp32') else ddt
    src = torch.randn((n, h + 2 * pad, w_ + 2 * pad, c), generator=torch.Generator().manual_seed(51)).to(sdt)
    x = torch.zeros(n, c, h, w_, dtype=torch.float64, requires_grad=True)
    s64 = src.double().permute(0, 3, 1, 2)
    ref = torch.autograd.grad(F.pad(x, (pad,) * 4, mode='replicate'), x, s64)[0].permute(0, 2, 3, 1).contiguous()
    S = torch.autograd.grad(F.pad(x, (pad,) * 4, mode='replicate'), x, s64.abs())[0].permute(0, 2, 3, 1).contiguous()
    T = (2 * pad + 1) ** 2
    u = PR.U32 if ddt == torch.float32 else {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[ddt]
    bnd = S * (T * U32) + ref.abs() * u + U32
    with Lib(half) as be:
        dst = torch.full(shape, 3.0, dtype=ddt, device=DEV)
        be.replicate_fold(src.to(DEV), dst, pad)
        torch.cuda.synchronize()
        worst, rep = PR.compare(dst, ref, bnd)
        assert worst <= 1.0, rep


def _dgrad(be, dy, wt, hw, dtype, prec):
    """the data gradient as engine.conv launches it: pad-0 plan over the padded extent (16-bit policies: raw fp32 accumulators), then the fold"""
    cout, cin = wt.shape[0], wt.shape[1]
    h, w_ = hw
    plan = ConvSpec('conv', cin, cout, 3, 1, 1, L.PAD_REPLICATE).dgrad_plan()
    packed = ops.PackedWeights(plan, DEV, prec == L.PREC_BF16X3)
    be.pack_weights(packed, wt.to(DEV))
    raw = dtype != torch.float32
    dxp = torch.empty((dy.shape[0], h + 2, w_ + 2, cpad(cin)), dtype=torch.float32 if raw else dtype, device=DEV)
    be.conv_forward(packed, dy, dxp, h + 2, w_ + 2, None, L.ACT_NONE, L.ACT_NONE, prec, raw_out=raw)
    dx = torch.empty((dy.shape[0], h, w_, cpad(cin)), dtype=dtype, device=DEV)
    be.replicate_fold(dxp, dx, 1)
    return dx


@pytest.mark.parametrize('half', ['bf16', 'fp16', 'strict'])
@pytest.mark.parametrize('shape', [(2, 40, 24, 32), (1, 4, 128, 256)], ids=lambda s: 'n%d-%dx%d-c%d' % s)
def test_data_gradient_plan_and_fold(shape, half):
    n, h, w_, c = shape
    strict = half == 'strict'
    dtype = torch.float32 if strict else DT[half]
    rdt = torch.bfloat16 if strict else dtype
    dy, wt = rnd((n, h, w_, c), 61, rdt), rnd((c, c, 3, 3), 62, rdt, 0.05)
    with Lib('bf16' if strict else half) as be:
        dx = _dgrad(be, dy.to(dtype).to(DEV), wt, (h, w_), dtype, L.PREC_BF16X3 if strict else L.PREC_BF16)
        torch.cuda.synchronize()
        ref, S, K = PR.dgrad(dy, wt, (h, w_))
        assert float(K.min()) == float(K.max()) == 9 * c
        bnd = S.mul_(K * U32).add_(ref.abs(), alpha=U32).add_(U32) if strict else PR.bound(ref, S, K, dtype)
        worst, rep = PR.compare(dx, ref, bnd)
        print(f'data gradient {shape} {half}: err/bound {worst:.3f}')
        assert worst <= 1.0, rep


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad(be, mode, P, Q, ca, cb, prec=L.PREC_BF16, splitk=None):
    g = torch.full((ca, cb, 3, 3), 5.0, device=DEV)
    be.conv_wgrad(P, Q, g, 3, 1, 1, RC.PAD[mode], L.ACT_NONE, L.ACT_NONE, prec, False, splitk=splitk)
    return g


def _plan_name(be, mode, P, Q, ca, cb, policy='bf16'):
    d = RC.wgrad_desc(mode, P.shape[0], P.shape[1], P.shape[2], ca, cb, policy=policy, p_pstride=P.stride(2), q_pstride=Q.stride(2))
    return RC.wgrad_plan(be.lib, d)[3]


# N, H, CA (dL/dy channels), CB (input channels), width of the buffer Q is a slice of
W4W_CASES = [(1, 2, 128, 128, None),         # every row a border row
             (2, 3, 256, 128, 192)]          # odd H: row ranges start and end mid-image; channel-slice x


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('case', W4W_CASES, ids=lambda c: 'n%d-h%d-ca%d-cb%d' % c[:4])
def test_weight_gradient_on_the_w4_kernel(case, half):
    n, h, ca, cb, wide = case
    dtype = DT[half]
    dy, x = rnd((n, h, 128, ca), 71, dtype), rnd((n, h, 128, cb), 72, dtype)
    with Lib(half) as be:
        P = dy.to(dtype).to(DEV)
        Q = _as_view(x, wide, dtype)
        ref, S, K = PR.wgrad(dy, x, ca, cb, mode='replicate')
        bnd = PR.wgrad_bound(ref, S, K)
        ref0, S0, K0 = PR.wgrad(dy, x, ca, cb, mode='zero')
        bnd0 = PR.wgrad_bound(ref0, S0, K0)
        assert _plan_name(be, 'replicate', P, Q, ca, cb) == RC.W4W and _plan_name(be, 'zero', P, Q, ca, cb) == RC.W4W
        for sk in (1, 2, n * h):
            got = _wgrad(be, 'replicate', P, Q, ca, cb, splitk=sk)
            ctl = _wgrad(be, 'zero', P, Q, ca, cb, splitk=sk)
            torch.cuda.synchronize()
            worst0 = float(((ctl.double().cpu() - ref0).abs() / bnd0).max())
            worst = float(((got.double().cpu() - ref).abs() / bnd).max())
            print(f'wgrad_w4 {case[:4]} {half} splitk {sk}: replicate err/bound {worst:.3f}, zero-padding control {worst0:.3f}')
            assert worst <= (1.0 if worst0 <= 1.0 else 2.0 * worst0), (sk, worst, worst0)
            assert worst0 <= 1.0, 'the zero-padding control itself is out of bound (a finding about the existing kernel)'
            # the centre tap never touches the border: bit-identical to the zero-padding instantiation
            assert torch.equal(got[:, :, 1, 1], ctl[:, :, 1, 1]) and not torch.equal(got[:, :, 0, 0], ctl[:, :, 0, 0])
            again = _wgrad(be, 'replicate', P, Q, ca, cb, splitk=sk)
            assert torch.equal(again, got)                                      # fixed-order combine


def test_batched_weight_gradient_of_two_replicate_layers(monkeypatch):
    """dl_conv_wgrad_multi with the replicate instantiation: two same-shaped layers queued inside a pass are computed by one launch, bit-identical to single
    launches at the batch's split-K and within the bound"""
    n, h, ca, cb = 2, 3, 128, 128
    data = [(rnd((n, h, 128, ca), 80 + i, torch.bfloat16), rnd((n, h, 128, cb), 90 + i, torch.bfloat16)) for i in range(2)]
    with Lib('bf16') as be:
        dev = [(a.bfloat16().to(DEV), b.bfloat16().to(DEV)) for a, b in data]
        rc, tiles, ksteps, name = RC.wgrad_plan(be.lib, RC.wgrad_desc('replicate', n, h, 128, ca, cb))
        assert (rc, name) == (1, RC.W4W)
        sk = choose_wgrad_batch_splitk(tiles, ksteps)
        single = [_wgrad(be, 'replicate', P, Q, ca, cb, splitk=sk) for P, Q in dev]
        monkeypatch.setattr(ops, '_WGRAD_BATCH', True)
        monkeypatch.setattr(ops, '_WGRAD_DEFER', True)
        got = [torch.full((ca, cb, 3, 3), 5.0, device=DEV) for _ in dev]
        be.wgrad_defer_begin()
        for (P, Q), g in zip(dev, got):
            be.conv_wgrad(P, Q, g, 3, 1, 1, L.PAD_REPLICATE, L.ACT_NONE, L.ACT_NONE, L.PREC_BF16, False)
        st = ops.WS._state()
        assert len(st['defer_queue']) == 2 and float(got[0][0, 0, 0, 0]) == 5.0          # queued, nothing has run
        be.wgrad_defer_end()
        torch.cuda.synchronize()
        for (dy, x), g, s in zip(data, got, single):
            assert torch.equal(g, s)
            ref, S, K = PR.wgrad(dy, x, ca, cb)
            assert float(((g.double().cpu() - ref).abs() / PR.wgrad_bound(ref, S, K)).max()) <= 1.0


@pytest.mark.parametrize('policy', ['bf16', 'fp16', 'strict'])
def test_weight_gradient_on_the_generic_kernel(policy):
    n, h, w_, c = 2, 40, 24, 32
    strict = policy == 'strict'
    dtype = torch.float32 if strict else DT[policy]
    rdt = torch.bfloat16 if strict else dtype
    dy, x = rnd((n, h, w_, c), 101, rdt), rnd((n, h, w_, c), 102, rdt)
    with Lib('bf16' if strict else policy) as be:
        P, Q = dy.to(dtype).to(DEV), x.to(dtype).to(DEV)
        assert _plan_name(be, 'replicate', P, Q, c, c, 'strict' if strict else 'bf16') == 'wgrad_kernel'
        got = _wgrad(be, 'replicate', P, Q, c, c, L.PREC_BF16X3 if strict else L.PREC_BF16)
        torch.cuda.synchronize()
        ref, S, K = PR.wgrad(dy, x, c, c)
        worst = float(((got.double().cpu() - ref).abs() / PR.wgrad_bound(ref, S, K)).max())
        print(f'generic wgrad {policy}: err/bound {worst:.3f}')
        assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ paths only the C ABI reaches
@pytest.mark.parametrize('policy', ['bf16', 'strict'])
def test_c4_patch_kernels_with_a_replicate_border(policy):
    """7 x 7, 3 -> 64 channels with replicate padding 3: the product never asks for it (stem and head of a replicate net are zero-padded, as in the reference),
    but dl_conv_forward accepts it and sends it to conv_c4_patch_kernel<DL_PAD_REPLICATE, .> / its strict twin"""
    n, h, w_, ci, co = 1, 8, 64, 3, 64
    strict = policy == 'strict'
    dtype = torch.float32 if strict else torch.bfloat16
    x = torch.zeros(n, h, w_, 8)
    x[..., :ci] = rnd((n, h, w_, ci), 111, torch.bfloat16)
    wt = rnd((co, ci, 7, 7), 112, torch.bfloat16, 0.1)
    with Lib('bf16') as be:
        prec = L.PREC_BF16X3 if strict else L.PREC_BF16
        plan = ConvSpec('conv', ci, co, 7, 1, 3, L.PAD_REPLICATE).forward_plan()
        packed = ops.PackedWeights(plan, DEV, strict)
        be.pack_weights(packed, wt.to(DEV))
        y = torch.empty((n, h, w_, co), dtype=dtype, device=DEV)
        be.conv_forward(packed, x.to(dtype).to(DEV), y, h, w_, None, L.ACT_NONE, L.ACT_NONE, prec, splitk=1)
        torch.cuda.synchronize()
        assert be.last_conv_kernel == ('conv_c4_patch_x3_kernel' if strict else 'conv_c4_patch_kernel'), be.last_conv_kernel
        ref, S, K = PR.forward(x, wt, pad=3)
        assert K == 49 * ci
        bnd = S.mul_(K * U32).add_(ref.abs(), alpha=U32).add_(U32) if strict else PR.bound(ref, S, K, dtype)
        worst, rep = PR.compare(y, ref, bnd)
        print(f'c4 patch replicate {policy}: err/bound {worst:.3f}')
        assert worst <= 1.0, rep
        other = PR.forward(x, wt, mode='zero', pad=3)[0]
        assert float(((other - ref).abs() > bnd).float().mean()) > 0.1          # (3 of 8 rows and 6 of 64 columns are border: zero padding would miss there)


def test_shift_sum_with_a_replicate_border():
    """dl_shift_sum (second half of the narrow-Cout route) with pad_mode replicate: the kernel-column sum reads the clamped column"""
    n, h, w_, cout, kw, pad = 2, 3, 37, 3, 7, 3
    tc = 24
    T = torch.randn(n, h, w_, tc, generator=torch.Generator().manual_seed(121))
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(122))
    with Lib('bf16') as be:
        out = torch.empty((n, h, w_, 8), dtype=torch.float32, device=DEV)
        be.shift_sum(T.to(DEV), cout, kw, pad, L.PAD_REPLICATE, bias.to(DEV), L.ACT_NONE, out)
        torch.cuda.synchronize()
    idx = (torch.arange(w_)[:, None] + torch.arange(kw)[None, :] - pad).clamp_(0, w_ - 1)          # [w, kw]
    T64 = T.double()
    ref = torch.zeros(n, h, w_, 8, dtype=torch.float64)
    for c in range(cout):
        for k in range(kw):
            ref[..., c] += T64[:, :, idx[:, k], c * kw + k]
        ref[..., c] += float(bias[c])
    S = 8 * U32 * (T64.abs().amax() * kw + bias.abs().max())          # eight fp32 additions of values up to max|T|
    assert float((out.double().cpu() - ref).abs().max()) <= float(S)


def test_raw_accumulators_on_the_big_tile_route():
    """the replicate data gradient of a full-size block asks the pad-0 plan for raw fp32 accumulators on a launch of >= 224 tiles (conv_gemm_8ph_kernel): same
    kernel, same summation as the 16-bit store of that launch -- rounding the raw values must reproduce the stored ones bit for bit"""
    n, h, w_, c = 4, 126, 126, 256
    dy, wt = rnd((n, h, w_, c), 131, torch.bfloat16), rnd((c, c, 3, 3), 132, torch.bfloat16, 0.05)
    with Lib('bf16') as be:
        plan = ConvSpec('conv', c, c, 3, 1, 1, L.PAD_REPLICATE).dgrad_plan()
        packed = ops.PackedWeights(plan, DEV, False)
        be.pack_weights(packed, wt.to(DEV))
        g = dy.bfloat16().to(DEV)
        stored = torch.empty((n, h + 2, w_ + 2, c), dtype=torch.bfloat16, device=DEV)
        be.conv_forward(packed, g, stored, h + 2, w_ + 2, None, L.ACT_NONE, L.ACT_NONE, L.PREC_BF16)
        assert be.last_conv_kernel == 'conv_gemm_8ph_kernel', be.last_conv_kernel
        raw = torch.empty((n, h + 2, w_ + 2, c), dtype=torch.float32, device=DEV)
        be.conv_forward(packed, g, raw, h + 2, w_ + 2, None, L.ACT_NONE, L.ACT_NONE, L.PREC_BF16, raw_out=True)
        torch.cuda.synchronize()
        assert torch.equal(raw.bfloat16(), stored)
        dx = torch.empty((n, h, w_, c), dtype=torch.bfloat16, device=DEV)
        be.replicate_fold(raw, dx, 1)
        torch.cuda.synchronize()
        # the fold of the fp32 values, restated with torch on the device: interior = the one padded position, edges = the sums of their copies
        def fold64(t):
            t = t.clone()
            t[:, 1] += t[:, 0]; t[:, -2] += t[:, -1]
            t = t[:, 1:-1]
            t[:, :, 1] += t[:, :, 0]; t[:, :, -2] += t[:, :, -1]
            return t[:, :, 1:-1]
        exp, mag = fold64(raw.double()), fold64(raw.double().abs())
        # up to four fp32 values summed in fp32, one bf16 store
        assert float(((dx.double() - exp).abs() / (exp.abs() * 2.0 ** -8 + 4 * U32 * mag + U32)).max()) <= 1.0

