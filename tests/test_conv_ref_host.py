"""The float64 reference / per-element bound / comparer of tests/conv_ref.py, checked on the CPU against a stand-in for a correct kernel (fp32 accumulation in
another summation order, result rounded to the 16-bit format) and against four subtly wrong variants of it.  The bound has to accept the first and reject
every one of the others -- in particular a store that truncates instead of rounding to nearest, which the suite's older metric (max|err| / max|expected| <
6e-3) lets through."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref
from deepliif_amd import _lib as L
from deepliif_amd.geometry import ConvSpec, cpad

SHAPES = {
    # name: (cin, cout, k, N, H, W): ResnetGenerator down1 and the PatchGAN's first conv, both stride 2, padding 1
    'down1': (64, 128, 3, 1, 32, 32),
    'c1': (6, 64, 4, 2, 32, 64),
}


def _round_to(v, dtype, trunc=False):
    if not trunc:
        return v.to(dtype)
    drop = 16 if dtype == torch.bfloat16 else 13          # mantissa bits of fp32 the format does not keep (values in the normal range of half here)
    return (v.contiguous().view(torch.int32) & ~((1 << drop) - 1)).view(torch.float32).to(dtype)


def _inputs(name, dtype):
    cin, cout, k, N, H, W_ = SHAPES[name]
    g = torch.Generator().manual_seed(11)
    x = torch.zeros(N, H, W_, cpad(cin))
    x[..., :cin] = torch.randn(N, H, W_, cin, generator=g).to(dtype).float()
    w = (torch.randn(cout, cin, k, k, generator=g) * 0.05).to(dtype).float()
    bias = torch.randn(cout, generator=g) * 0.1
    return x, w, bias


def standin(name, dtype, x, w, bias, act=L.ACT_NONE, drop=None, trunc=False, nobias_group=None, zero_halo_row=None):
    """a correct kernel's arithmetic (exact products, fp32 sums, one rounding at the store) -- taps last to first, channels inside a tap by a matrix
    product -- or one of the wrong variants:
      drop = (row, kh, kw, ci): input channel ci of tap (kh, kw) is missing on output row `row`
      trunc: the store truncates
      nobias_group = g: output channels 32 g .. 32 g + 31 miss the bias
      zero_halo_row = row: output row `row` (the first of a strip) sees zeros instead of input row 2 row - 1 (a halo row that was not staged)"""
    cin, cout, k, N, H, W_ = SHAPES[name]
    ho, wo = H // 2, W_ // 2
    xp = F.pad(x[..., :cin], (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(N, ho, wo, cout)
    for kh in reversed(range(k)):
        for kw in reversed(range(k)):
            g = xp[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2, :]
            t = g @ w[:, :, kh, kw].t()
            if drop is not None and drop[1:3] == (kh, kw):
                t[:, drop[0]] -= g[:, drop[0], :, drop[3], None] * w[:, drop[3], kh, kw]
            if zero_halo_row is not None and kh == 0:
                t[:, zero_halo_row] = 0
            acc += t
    acc += bias
    if nobias_group is not None:
        acc[..., 32 * nobias_group:32 * nobias_group + 32] -= bias[32 * nobias_group:32 * nobias_group + 32]
    if act == L.ACT_RELU:
        acc = torch.relu(acc)
    elif act == L.ACT_LRELU:
        acc = torch.where(acc > 0, acc, 0.2 * acc)
    return _round_to(acc, dtype, trunc)


def _judge(name, dtype, got, x, w, bias, act=L.ACT_NONE):
    cin, cout, k, N, H, W_ = SHAPES[name]
    spec = ConvSpec('conv', cin, cout, k, 2, 1, L.PAD_ZERO, 0)
    ref, S, K = conv_ref.reference(spec, 'fwd', x, w, bias, act)
    bnd = conv_ref.bound(ref, S, K, dtype)
    return conv_ref.compare(got, ref, bnd, {'kernel': 's2d' if name == 'down1' else 'd1', 'R': 4, 'row_div': 1}), ref


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'half'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_the_bound_accepts_a_correct_kernel(name, dtype):
    x, w, bias = _inputs(name, dtype)
    for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU):
        (worst, report), _ = _judge(name, dtype, standin(name, dtype, x, w, bias, act), x, w, bias, act)
        print(f'{name} {dtype} act {act}: worst err/bound {worst:.3f}')
        assert report == '' and worst <= 1.0, report
        assert worst > 0.5, 'a bound the rounding of the store alone does not come near to is not a tight bound'


MUTATIONS = {
    'tap_channel_dropped_on_one_row': dict(drop=(5, 1, 2, 3)),
    'truncating_store': dict(trunc=True),
    'bias_dropped_on_a_channel_group': dict(nobias_group=1),
    'strip_first_row_from_a_zeroed_halo': dict(zero_halo_row=4),
}


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'half'])
@pytest.mark.parametrize('mutation', list(MUTATIONS))
@pytest.mark.parametrize('name', list(SHAPES))
def test_the_bound_rejects_a_subtly_wrong_kernel(name, mutation, dtype):
    x, w, bias = _inputs(name, dtype)
    got = standin(name, dtype, x, w, bias, **MUTATIONS[mutation])
    (worst, report), ref = _judge(name, dtype, got, x, w, bias)
    old_metric = float((got.double()[..., :ref.shape[3]] - ref).abs().max() / ref.abs().max())
    print(f'{name} {mutation} {dtype}: worst err/bound {worst:.3g}, the older metric {old_metric:.3g}\n{report}')
    assert worst > 1.0 and report, 'the comparer let a wrong kernel through'
    if mutation == 'tap_channel_dropped_on_one_row':
        assert 'by output row   {5: ' in report and 'by row mod R    {1: ' in report and 'by strip index  {1: ' in report, report
    if mutation == 'strip_first_row_from_a_zeroed_halo':
        assert 'by output row   {4: ' in report and 'by row mod R    {0: ' in report, report
    if mutation == 'bias_dropped_on_a_channel_group':
        assert 'by wave*100' in report or name != 'down1'


def test_truncation_passes_the_older_metric():
    """why the sweep does not use max|err| / max|expected| < 6e-3: on bf16 a truncating store stays under it"""
    for name in SHAPES:
        x, w, bias = _inputs(name, torch.bfloat16)
        got = standin(name, torch.bfloat16, x, w, bias, trunc=True)
        (worst, _), ref = _judge(name, torch.bfloat16, got, x, w, bias)
        assert float((got.double() - ref).abs().max() / ref.abs().max()) < 6e-3 and worst > 1.0


def test_a_nan_is_out_of_bound():
    x, w, bias = _inputs('c1', torch.bfloat16)
    got = standin('c1', torch.bfloat16, x, w, bias)
    got[1, 3, 7, 9] = float('nan')
    (worst, report), _ = _judge('c1', torch.bfloat16, got, x, w, bias)
    assert worst == float('inf') and '(1, 3, 7, 9)' in report


def test_data_gradients_are_the_transposed_operation():
    """reference(..., 'dgrad') against autograd of the float64 forward, for the four layer forms of the sweep"""
    for kind, cin, cout, k, op, hw in (('conv', 64, 128, 3, 0, (12, 16)), ('convT', 128, 64, 3, 1, (6, 8)), ('conv', 6, 64, 4, 0, (8, 12)), ('conv', 512, 1, 4, 0, (7, 6))):
        s = 1 if cin == 512 else 2
        spec = ConvSpec(kind, cin, cout, k, s, 1, L.PAD_ZERO, op)
        g = torch.Generator().manual_seed(3)
        w = torch.randn((cout, cin, k, k) if kind == 'conv' else (cin, cout, k, k), generator=g, dtype=torch.float64)
        x = torch.randn(2, cin, *hw, generator=g, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, w, None, s, 1) if kind == 'conv' else F.conv_transpose2d(x, w, None, s, 1, op)
        assert tuple(y.shape[2:]) == spec.out_hw(*hw)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(dy)
        ref, S, K = conv_ref.reference(spec, 'dgrad', dy.permute(0, 2, 3, 1), w, None, L.ACT_NONE, in_hw=hw)
        assert ref.shape == (2, hw[0], hw[1], cpad(cin))
        assert float((ref[..., :cin] - x.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-10
        assert float(ref[..., cin:].abs().max()) == 0.0 if cpad(cin) > cin else True
        assert float((S - ref.abs()).min()) > -1e-9 and int(K.max()) <= k * k * cout


def test_strip_rows_restates_the_documented_choices():
    # (kernel, n, rows, width, co) -> R: down1 / up2 / PatchGAN c1 at the benched batch (csrc/conv_s2d.hip header: 16 rows)
    assert conv_ref.strip_rows('s2d', 8, 256, 256, 128) == (16, 16, 2)
    assert conv_ref.strip_rows('s2d', 1, 256, 256, 128) == (2, 128, 2)
    assert conv_ref.strip_rows('s2u', 8, 256, 256, 64) == (32, 8, 4)
    assert conv_ref.strip_rows('d1', 16, 256, 256, 64) == (8, 32, 1)
    assert conv_ref.strip_rows('d1g', 16, 256, 256, 8) == (16, 16, 2)
    assert conv_ref.strip_rows('s2u', 2, 7, 192, 64) == (1, 7, 3)
