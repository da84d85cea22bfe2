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


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# The tile family (tests/tileconv_cases.py, tests/test_gpu_tileconv.py): the bounds of the fp32-storing policies, the reflect border, the data gradient over
# the padded extent, and the faults of a tile kernel's geometry edges -- judged on the CPU before any GPU run.
import pad_ref  # noqa: E402
from tileconv_cases import conv as _row  # noqa: E402
import tileconv_cases as TC  # noqa: E402

Z, RF, RP = L.PAD_ZERO, L.PAD_REFLECT, L.PAD_REPLICATE
TILE_ROWS = {
    # two small stride-1 layers of the GPU table's kind: 270 pixels = 2.1 tiles of 128, one tile straddles both images; 240 pixels behind a reflect border
    'zero': _row(64, 64, 3, 1, 1, (2, 9, 15), 'stand-in'),
    'reflect': _row(32, 32, 3, 1, 1, (2, 10, 12), 'stand-in', pm=RF),
    # one product per element: the shape at which a truncating hi part of the strict split shows (see MUT_TILE)
    'k1': _row(1, 64, 1, 1, 0, (2, 9, 15), 'stand-in', bias=False),
}
BM_STANDIN = 128


def _trunc_bf16(v):
    return (v.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)


def _split(v, trunc_hi=False):
    """hi = bf16(v), lo = bf16(v - hi): store_split8 (csrc/common.h) / raw_to_planes (csrc/conv_gemm.hip)"""
    hi = _trunc_bf16(v) if trunc_hi else v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


def _tile_inputs(row, policy, seed=11):
    spec = TC.spec_of(row)
    g = torch.Generator().manual_seed(seed)
    _, n, hi, wi, cip, _, _, _, _, _ = TC.geometry(row)
    c = spec.cin if row.direction == 'fwd' else spec.cout
    x = torch.zeros(n, hi, wi, cip)
    x[..., :c] = torch.randn(n, hi, wi, c, generator=g)
    w = torch.randn(spec.cout, spec.cin, spec.k, spec.k, generator=g) * 0.05
    bias = torch.randn(spec.cout, generator=g) * 0.1
    if policy == 'bf16':
        x = x.bfloat16().float()
    if not policy.startswith('strict'):
        w = w.bfloat16().float()
    return x, w, bias


def tile_standin(row, policy, x, w, bias, mut=None):
    """a correct tile kernel's arithmetic for a stride-1 Conv2d, forward or data gradient, in float32 and in another summation order than the reference's
    (taps last to first, the channels of a tap by a matrix product, split-K partials reduced at the end):
      'strict'     hi / lo split of activations and weights by the formula of store_split8 / raw_to_planes, lo hi + hi lo + hi hi per tap, fp32 store
      'fp32+bf16'  activations rounded to bf16 while staging, one product, fp32 store
      'bf16'       stored 16-bit operands, one product, bf16 store
    or one of the faults of MUT_TILE."""
    mut = mut or {}
    spec = TC.spec_of(row)
    k, p = spec.k, spec.pad
    strict = policy.startswith('strict')
    trunc = mut.get('trunc_hi', False)
    c = spec.cin if row.direction == 'fwd' else spec.cout
    xv = x[..., :c]
    if strict:
        xh, xl = _split(xv, trunc)
        wh, wl = _split(w, trunc)
    else:
        xh = (_trunc_bf16(xv) if trunc else xv.bfloat16().float()) if policy == 'fp32+bf16' else xv
        xl, wh, wl = None, w, None

    def padded(t):
        if t is None:
            return None
        t = t.permute(0, 3, 1, 2)
        if row.direction == 'dgrad':
            q = k - 1 - (p if spec.pad_mode == Z else 0)          # the padded extent of a reflect / replicate layer: a pad-0 conv's gradient
            return F.pad(t, (q,) * 4).permute(0, 2, 3, 1)
        mode = {Z: 'constant', RF: 'reflect', RP: 'replicate'}[mut.get('border', spec.pad_mode)]
        return F.pad(t, (p,) * 4, mode=mode).permute(0, 2, 3, 1)
    xh, xl = padded(xh), padded(xl)
    _, n, _, _, _, ho, wo, _, _, _ = TC.geometry(row)
    co = spec.cout if row.direction == 'fwd' else spec.cin
    taps = [(kh, kw) for kh in reversed(range(k)) for kw in reversed(range(k))]
    nsplit = mut.get('splitk', 1)
    parts = [torch.zeros(n, ho, wo, co) for _ in range(nsplit)]
    for i, (kh, kw) in enumerate(taps):
        if row.direction == 'fwd':
            sl = (slice(None), slice(kh, kh + ho), slice(kw, kw + wo))
            wsel = lambda t: t[:, :, kh, kw].t()                                        # noqa: E731  [ci, co]
        else:
            sl = (slice(None), slice(k - 1 - kh, k - 1 - kh + ho), slice(k - 1 - kw, k - 1 - kw + wo))
            kws = (k - 1 - kw) if mut.get('unreversed_kw') else kw
            wsel = lambda t: t[:, :, kh, kws]                                           # noqa: E731  [co, ci]
        acc = parts[i * nsplit // len(taps)]
        if strict:
            lohi = xl[sl] @ wsel(wh)
            if 'drop_lohi_row' in mut:
                lohi[:, mut['drop_lohi_row']] = 0
            acc += lohi
            acc += xh[sl] @ wsel(wl)
        acc += xh[sl] @ wsel(wh)
    if 'skip_partial' in mut:            # (partial, tile): that tile's pixels of one split-K slab never reach the reduce
        part, tile = mut['skip_partial']
        parts[part].view(-1, co)[tile * BM_STANDIN:(tile + 1) * BM_STANDIN] = 0
    acc = parts[0]
    for q in parts[1:]:
        acc = acc + q
    if row.bias:
        acc = acc + bias
    if mut.get('masked_rows_written'):
        # tiles that end with the image: the last tile of image 0 writes its masked rows too (accumulators of nothing: the bias), onto the first pixels of image 1
        over = BM_STANDIN - (ho * wo) % BM_STANDIN
        acc.view(n, ho * wo, co)[1, :over] = bias if row.bias else 0.0
    out = torch.zeros(n, ho, wo, cpad(co))
    out[..., :co] = acc
    return out.bfloat16() if policy == 'bf16' else out


def _judge_tile(row, policy, got, x, w, bias):
    st = torch.bfloat16 if policy == 'bf16' else torch.float32
    ref, S, K = conv_ref.Reference(TC.spec_of(row), row.direction, x, w, in_hw=(row.H, row.W), policy=policy).variant(bias if row.bias else None, row.act)
    bnd = conv_ref.bound(ref, S, K, st, 1, policy, row.act)
    return conv_ref.compare(got, ref, bnd, {'bm': BM_STANDIN, 'step': 1})


@pytest.mark.parametrize('policy', ['strict', 'fp32+bf16'])
@pytest.mark.parametrize('name', ['zero', 'reflect'])
def test_the_fp32_bounds_accept_a_correct_kernel(name, policy):
    row = TILE_ROWS[name]
    x, w, bias = _tile_inputs(row, policy)
    worst, report = _judge_tile(row, policy, tile_standin(row, policy, x, w, bias), x, w, bias)
    print(f'{name} {policy}: worst err/bound {worst:.3f}')
    assert report == '' and worst <= 1.0, report
    # split-K partials are additions of the same sum: the bound does not move
    worst, report = _judge_tile(row, policy, tile_standin(row, policy, x, w, bias, {'splitk': 3}), x, w, bias)
    assert report == '' and worst <= 1.0, report


def test_the_strict_bound_accepts_the_split_at_one_product_per_element():
    row = TILE_ROWS['k1']
    x, w, bias = _tile_inputs(row, 'strict')
    worst, report = _judge_tile(row, 'strict', tile_standin(row, 'strict', x, w, bias), x, w, bias)
    print(f'k1 strict: worst err/bound {worst:.3f}')
    assert report == '' and worst <= 1.0, report


# fault: (row, direction, policy, edits of the stand-in, what the report has to say)
MUT_TILE = {
    # the lo x hi product is missing on output row 5 (strict): 576 terms of ~2^-9 |x w| against a bound of ~3 * 2^-16 S
    'lo_hi_dropped_on_one_row': ('zero', 'fwd', 'strict', {'drop_lohi_row': 5}, ['by output row   {5: ']),
    # the staged 16-bit value truncates: under fp32 storage with bf16 products every second activation is one bf16 ulp off the model's x.bfloat16() ...
    'hi_truncates/fp32+bf16': ('zero', 'fwd', 'fp32+bf16', {'trunc_hi': True}, ['by image        {']),
    # ... under strict, lo = bf16(v - hi) still picks up what a truncated hi leaves, and only the dropped lo lo product doubles to 2^-14 |x w| at worst; behind a
    # K = 576 sum that stays inside the worst-case bound (not a shape for this fault), at one product per element it does not
    'hi_truncates/strict': ('k1', 'fwd', 'strict', {'trunc_hi': True}, ['by image        {']),
    'reflect_border_replicates': ('reflect', 'fwd', 'strict', {'border': RP}, ['first: (n, h, w, c) = (0, 0, 0, ', 'by pixel mod 32  {0: ']),
    # 135 pixels per image: the last tile of image 0 has 121 masked rows, which land on image 1
    'masked_rows_of_a_ragged_tile_written': ('zero', 'fwd', 'fp32+bf16', {'masked_rows_written': True}, ['by image        {1: ', 'first: (n, h, w, c) = (1, 0, 0, ']),
    'split_k_partial_left_out_of_the_reduce': ('zero', 'fwd', 'strict', {'splitk': 3, 'skip_partial': (1, 1)}, ['by tile index   {1: ']),
    'kernel_columns_not_reversed_in_a_data_gradient': ('zero', 'dgrad', 'bf16', {'unreversed_kw': True}, ['by image        {']),
}


@pytest.mark.parametrize('mutation', list(MUT_TILE))
def test_the_bounds_reject_the_faults_of_a_tile_kernel(mutation):
    name, direction, policy, mut, where = MUT_TILE[mutation]
    row = TILE_ROWS[name]._replace(direction=direction, bias=TILE_ROWS[name].bias and direction == 'fwd')
    x, w, bias = _tile_inputs(row, policy)
    good, rep0 = _judge_tile(row, policy, tile_standin(row, policy, x, w, bias, {k: v for k, v in mut.items() if k == 'splitk'}), x, w, bias)
    assert rep0 == '' and good <= 1.0, f'the unmutated stand-in must pass first\n{rep0}'
    worst, report = _judge_tile(row, policy, tile_standin(row, policy, x, w, bias, mut), x, w, bias)
    print(f'{mutation}: worst err/bound {worst:.3g} (unmutated {good:.3f})\n{report}')
    assert worst > 1.0 and report, 'the comparer let a wrong kernel through'
    for text in where:
        assert text in report, (text, report)
    if mutation == 'masked_rows_of_a_ragged_tile_written':
        assert 'by image        {1: ' in report and ', 0: ' not in report.split('by image')[1].split('\n')[0]
    if mutation == 'reflect_border_replicates':
        # only border pixels differ: rows 0 and H - 1 whole, columns 0 and W - 1 elsewhere
        rows_line = report.split('by output row   ')[1].split('\n')[0]
        assert rows_line.startswith('{0: ') or rows_line.startswith('{9: '), rows_line


def test_the_reflect_and_replicate_references_are_pad_ref_and_autograd():
    """forward: pad_ref.forward itself; data gradient: autograd of the padded float64 conv with respect to the EXPLICITLY PADDED input, extent (H + 2p) x (W + 2p)"""
    for pm, mode in ((RF, 'reflect'), (RP, 'replicate')):
        row = _row(16, 24, 3, 1, 1, (2, 6, 7), 'ref', pm=pm)
        x, w, bias = _tile_inputs(row, 'bf16')
        ref, S, K = conv_ref.reference(TC.spec_of(row), 'fwd', x, w, bias, L.ACT_NONE)
        r2, S2, K2 = pad_ref.forward(x, w, bias, False, mode, 1)
        assert torch.equal(ref, r2) and torch.equal(S, S2) and float(K.min()) == float(K.max()) == K2
        drow = row._replace(direction='dgrad', bias=False)
        dy, _, _ = _tile_inputs(drow, 'bf16')
        ref, S, K = conv_ref.reference(TC.spec_of(drow), 'dgrad', dy, w, None, L.ACT_NONE, in_hw=(6, 7))
        xp = torch.zeros(2, 16, 8, 9, dtype=torch.float64, requires_grad=True)
        F.conv2d(xp, w.double()).backward(dy[..., :24].double().permute(0, 3, 1, 2).contiguous())
        assert ref.shape == (2, 8, 9, 16) and float((ref - xp.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12
        assert int(K.max()) == 9 * 24 and int(K.min()) == 24          # the corner of the padded extent sees one tap


def test_the_operand_model():
    v = torch.randn(4, 5, 6, 8, generator=torch.Generator().manual_seed(5))
    assert torch.equal(conv_ref.model_values(v, L.ACT_NONE, 'strict'), v.double())
    assert torch.equal(conv_ref.model_values(v, L.ACT_NONE, 'fp32+bf16'), v.bfloat16().double())
    assert torch.equal(conv_ref.model_values(v.half().float(), L.ACT_NONE, 'bf16'), v.half().double())          # stored values of either 16-bit format
    lr = torch.where(v > 0, v, v * 0.2)
    assert torch.equal(conv_ref.model_values(v, L.ACT_LRELU, 'strict+split'), lr.double())
    assert torch.equal(conv_ref.model_values(v.bfloat16().float(), L.ACT_LRELU, 'bf16'), torch.where(v.bfloat16().float() > 0, v.bfloat16().float(),
                                                                                                   v.bfloat16().float() * 0.2).bfloat16().double())
    assert torch.equal(conv_ref.model_values(v, L.ACT_RELU, 'bf16', torch.float16), torch.relu(v).half().double())
    import wgrad_ref
    assert wgrad_ref.model_values is conv_ref.model_values and wgrad_ref.STRICT_REPR == conv_ref.STRICT_REPR == 3 * 2.0 ** -16 * (1 + 2.0 ** -8)


def test_the_bounds_by_policy():
    ref, S, K = torch.tensor([[[[2.0, -1.0]]]], dtype=torch.float64), torch.tensor([[[[3.0, 1.5]]]], dtype=torch.float64), 10.0
    u = 2.0 ** -24
    assert torch.allclose(conv_ref.bound(ref, S.clone(), K, torch.float32, 1, 'fp32+bf16'), 10 * u * S + u * ref.abs(), rtol=1e-15)
    assert torch.allclose(conv_ref.bound(ref, S.clone(), K, torch.float32, 1, 'strict'), (conv_ref.STRICT_REPR + 30 * u) * S + u * ref.abs(), rtol=1e-15)
    assert torch.allclose(conv_ref.bound(ref, S.clone(), K, torch.float32, 1, 'strict+split', L.ACT_TANH), (conv_ref.STRICT_REPR + 30 * u) * S + 5 * u * ref.abs(),
                          rtol=1e-15)
    assert torch.allclose(conv_ref.bound(ref, S.clone(), K, torch.bfloat16), 2.0 ** -8 * ref.abs() + 10 * u * S + u, rtol=1e-15)
    assert torch.allclose(conv_ref.bound(ref, S.clone(), K, torch.float16, 1, 'bf16', L.ACT_TANH), (2.0 ** -11 + 4 * u) * ref.abs() + 10 * u * S + u, rtol=1e-15)
