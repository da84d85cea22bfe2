"""Float64 reference, per-element error bound and a locating comparer for the convolution kernels -- TEST INFRASTRUCTURE ONLY.

reference(): torch.nn.functional.conv2d / conv_transpose2d in float64 on the CPU (NCHW inside, NHWC in and out).  The data gradient is the transposed
operation of the same call; nothing here uses the project's GatherPlan tap tables, so an error in them cannot cancel between kernel and reference.

bound(): the kernels multiply operands that are exactly representable in the 16-bit format (the tests pre-round them), so every product is exact in fp32.
What remains is (a) the fp32 summation of K = taps x contracted channels products plus the bias, in whatever order, and (b) the rounding of the stored
value to the 16-bit format.  With S = conv(|x|, |w|) + |bias| (the sum of the magnitudes of everything that is added):

    |got - ref| <= u * |ref| + K * 2^-24 * S + 2^-24          u = 2^-8 (bfloat16: 8 significant bits, round to nearest), 2^-11 (IEEE half)

K * 2^-24 * S is the classical worst case of a length-K fp32 summation in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, 4.2,
gamma_{K} ~ K * 2^-24); K is counted per output element (taps that fall into the zero padding add exact zeros).  ReLU / LeakyReLU are 1-Lipschitz and are
applied to both sides, so they do not enlarge (a); the final 2^-24 covers the subnormal range of the half format (spacing 2^-24) and a result of exactly 0.
`sum_slack` multiplies term (a) only (1 = the derived bound).

compare(): worst err / bound and, when an element is out of bound, a report of WHERE: by image, by strip and row inside the strip, by pixel mod 32 / 64 / 128,
by channel mod 32 and -- for conv_s2d_kernel, whose accumulator layout is written down in csrc/conv_s2d.hip (the epilogue's comment: acc[j][q*4 + e] = channel
wave*32 + q*8 + lh*4 + e of pixel j*32 + lr) -- by (wave, lane >= 16, accumulator mod 8).  The other MFMA kernels (conv_s2u, conv_d1, conv_d1g) do not write their
accumulator-to-(pixel, channel) map down as one formula and this file does not guess it: their lane groups show up in the pixel-mod-32 and channel-mod-32
residues, which are reported for every kernel; conv_dot uses no MFMA.

Policies and borders (the tile-family rows of tests/tileconv_cases.py; the register kernels above are policy 'bf16', zero padding).

model_values(): the reference sees the values the kernel's documented arithmetic multiplies --
    'bf16'                     16-bit storage, 16-bit products   the stored values (the tests pre-round them)
    'fp32+bf16' ('f32b')       fp32 storage, 16-bit products     x.bfloat16(): raw_to_planes (csrc/conv_gemm.hip:41-59) rounds once while staging
    'strict' / 'strict+split'  fp32 storage, BF16X3 products     the fp32 values themselves (the split copy holds hi = bf16(v), lo = bf16(v - hi) of the same v)
    a staged input activation is act32(v) in float32 (common.h apply_act: `v > 0.f ? v : 0.2f * v`, the same float32 product here) and, under the two 16-bit
    product precisions, rounded ONCE more to the 16-bit format (raw_to_planes: apply_act, then f32_to_bf16); under strict it stays fp32.
    Weights: pre-rounded by the tests under the 16-bit precisions (packing is exact), full mantissas under strict (dl_pack_weights splits them by the formula
    of the activations).
Borders: reflect / replicate go through tests/pad_ref.py (F.pad in front of a padding-0 float64 conv).  The data gradient of such a layer is the gradient
    with respect to the EXPLICITLY PADDED input, extent (H + 2p) x (W + 2p): the transposed padding-0 convolution, which is what the kernel computes before
    the engine folds the border back (geometry.ConvSpec.dgrad_plan).
bound(), by store and products (S, K as above; sum_slack stays 1; nothing is fitted):
    16-bit store                  u |ref| + K 2^-24 S + 2^-24                          as derived above
    fp32 store, 16-bit products   K 2^-24 S + 2^-24 |ref|
        the products are exact as above; a length-K fp32 summation in any order is within (K - 1) 2^-24 S, the K-th 2^-24 and the |ref| term (the bias add is
        counted in K already) are generous by one rounding each.  Same form as tests/wgrad_ref.py's.
    strict (BF16X3)               (STRICT_REPR + 3K 2^-24) S + 2^-24 |ref|,            STRICT_REPR = 3 * 2^-16 * (1 + 2^-8)
        bfloat16 keeps 8 significant bits: hi = bf16(v) leaves |v - hi| <= 2^-8 |v|; v - hi is exact in fp32; lo = bf16(v - hi) leaves
        |v - hi - lo| <= 2^-16 |v| and |lo| <= 2^-8 (1 + 2^-8) |v|.  The kernels add lo_x hi_w + hi_x lo_w + hi_x hi_w = (hi_x + lo_x)(hi_w + lo_w) - lo_x lo_w, so
        per product |x w - (three terms)| <= (2 * 2^-16 + 2^-32) |x w| + 2^-16 (1 + 2^-8)^2 |x w| <= 3 * 2^-16 (1 + 2^-8) |x w|.  Each of the three terms is a
        product of two bf16 values (exact in fp32): what is left is one fp32 summation of 3K terms, 3K 2^-24 S to first order.  (tests/wgrad_ref.py carries
        the longer write-up, with why u16 is 2^-8 and not 2^-9; it imports the constant from here.)
    split-K adds nothing: the partials and their reduce are additions of the same sum, covered by "any order".
    TANH output                   + TANH_ULPS 2^-24 |ref|   tanh is 1-Lipschitz, so the error of its argument passes at most unchanged; tanhf itself is within
                                  elementwise_ref.TANH_ULPS ulps (measured on the MI355X and recorded there)
    LRELU output, fp32 store      + 2 * 2^-24 |ref|         `0.2f * v` (common.h:218): 0.2f is not 0.2 (relative 2^-26) and the product rounds once -- the r = 2
                                  of tests/elementwise_ref.py; under a 16-bit store the rounding of the store (2^-8, 2^-11) hides it, as it always did

strip_rows(): a restatement of strip_rows() of csrc/conv_args.h as csrc/conv_{s2d,s2u,d1,d1g}.hip call it; used as a coverage guard only (the sweep asserts which strip
heights its table exercises) and cross-checked against the library through dl_conv_stats_chunks (tests/test_dispatch_host.py)."""
import torch
import torch.nn.functional as F

from deepliif_amd import _lib as L
from deepliif_amd.geometry import cpad

U_STORE = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U32 = 2.0 ** -24
U16 = 2.0 ** -8          # bfloat16: 8 significant bits, round to nearest
STRICT_REPR = 3 * U16 * U16 * (1 + 2.0 ** -8)
_MODE = {L.PAD_REFLECT: 'reflect', L.PAD_REPLICATE: 'replicate'}


def _act64(act, v):
    if act == L.ACT_RELU:
        return torch.relu(v)
    if act == L.ACT_LRELU:
        return torch.where(v > 0, v, 0.2 * v)
    if act == L.ACT_TANH:
        return torch.tanh(v)
    assert act == L.ACT_NONE, act
    return v


def act32(act, v):
    """the staged activation as the kernels compute it: float32"""
    assert v.dtype == torch.float32
    if act == L.ACT_RELU:
        return torch.relu(v)
    if act == L.ACT_LRELU:
        return torch.where(v > 0, v, v * 0.2)
    assert act == L.ACT_NONE, act
    return v


def model_values(v, act, policy, h16=torch.bfloat16):
    """float64 values the kernel's documented arithmetic multiplies for the stored fp32 / 16-bit tensor v (h16: the library's 16-bit format)"""
    if policy == 'bf16' and act == L.ACT_NONE:
        return v.double()          # the stored values, of either 16-bit format: nothing is staged through fp32
    a = act32(act, v.float())
    return a.double() if policy.startswith('strict') else a.to(h16).double()


def _op(spec, direction, x, w, in_hw):
    """the layer (direction 'fwd') or its transpose (direction 'dgrad') on NCHW float64 tensors"""
    s, p = spec.stride, spec.pad
    transposed = (spec.kind == 'convT') == (direction == 'fwd')
    if spec.pad_mode != L.PAD_ZERO:
        assert spec.kind == 'conv' and s == 1, 'explicitly padded layers are stride-1 Conv2d'
        if direction == 'fwd':
            import pad_ref          # (pad_ref imports this module: not at the top)
            return pad_ref.conv64(x, w, None, _MODE[spec.pad_mode], p)
        return F.conv_transpose2d(x, w, None, 1, 0)          # the gradient with respect to the explicitly padded input: (H + 2p) x (W + 2p)
    if not transposed:
        return F.conv2d(x, w, None, s, p)
    if direction == 'fwd':
        return F.conv_transpose2d(x, w, None, s, p, spec.out_pad)
    # gradient of Conv2d with respect to its input: the output padding is whatever restores the layer-input size
    h, w_ = in_hw
    oph = h - ((x.shape[2] - 1) * s - 2 * p + spec.k)
    opw = w_ - ((x.shape[3] - 1) * s - 2 * p + spec.k)
    assert 0 <= oph < s and 0 <= opw < s, (oph, opw)
    return F.conv_transpose2d(x, w, None, s, p, (oph, opw))


class Reference:
    """the float64 convolution of one (x, w) pair, computed once; variant(bias, act) derives each bias / activation variant from it"""

    def __init__(self, spec, direction, x, w, in_hw=None, policy='bf16', in_act=L.ACT_NONE, h16=torch.bfloat16):
        """x holds the STORED values (fp32, or exactly representable in the 16-bit format h16); policy / in_act: the operand model (model_values)"""
        c_in = spec.cin if direction == 'fwd' else spec.cout
        self.c_out = spec.cout if direction == 'fwd' else spec.cin
        xv = model_values(x[..., :c_in], in_act, policy, h16).permute(0, 3, 1, 2).contiguous()
        wv = w.double()
        self.raw = _op(spec, direction, xv, wv, in_hw)
        self.S0 = _op(spec, direction, xv.abs_(), wv.abs(), in_hw)
        ones = torch.ones((1, 1) + tuple(xv.shape[2:]), dtype=torch.float64)
        w1 = torch.ones((1, 1, spec.k, spec.k), dtype=torch.float64)
        self.K0 = (_op(spec, direction, ones, w1, in_hw) * c_in).permute(0, 2, 3, 1).contiguous()          # [1, Ho, Wo, 1]: products summed per element

    def _nhwc(self, t):
        c = self.c_out
        out = torch.zeros(t.shape[0], t.shape[2], t.shape[3], cpad(c), dtype=torch.float64)
        out[..., :c] = t.permute(0, 2, 3, 1)
        return out

    def variant(self, bias, act):
        """(ref, S, K) for one bias / activation: NHWC float64, padded to the engine's channel count (padding channels 0); S and ref are fresh tensors"""
        if bias is None:
            return self._nhwc(_act64(act, self.raw)), self._nhwc(self.S0), self.K0
        b = bias.double().view(1, -1, 1, 1)
        return self._nhwc(_act64(act, self.raw + b)), self._nhwc(self.S0 + b.abs()), self.K0 + 1


def reference(spec, direction, x, w, bias, act, in_hw=None):
    """x: NHWC (layer input for 'fwd', dL/dy for 'dgrad'; padding channels ignored); w: the layer's weight in its torch layout; bias: [C] or None.
    in_hw: (H, W) of the layer input, needed for the data gradient of a strided Conv2d.
    Returns (ref, S, K): NHWC float64 tensors padded to the engine's channel count (padding channels 0) and the per-element summation length
    [1, Ho, Wo, 1]."""
    return Reference(spec, direction, x, w, in_hw).variant(bias, act)


def bound(ref, S, K, dtype, sum_slack=1, policy='bf16', act=L.ACT_NONE):
    """the per-element bound of the module docstring; dtype: the storage type of the result (bfloat16 / float16 / float32), policy: which products an fp32
    result was summed from.  S is consumed (overwritten in place: the tensors of the large cases are ~1 GB each)"""
    extra = 0.0
    if act == L.ACT_TANH:
        from elementwise_ref import TANH_ULPS          # (elementwise_ref imports pad_ref, which imports this module: not at the top)
        extra = TANH_ULPS * U32
    if dtype in U_STORE:
        assert not policy.startswith('strict')
        return S.mul_(K).mul_(sum_slack * U32).add_(ref.abs(), alpha=U_STORE[dtype] + extra).add_(U32)
    assert dtype == torch.float32, dtype
    if act == L.ACT_LRELU:
        extra = 2 * U32
    if policy.startswith('strict'):
        return S.mul_((3 * sum_slack * U32) * K + STRICT_REPR).add_(ref.abs(), alpha=U32 + extra)
    return S.mul_(K).mul_(sum_slack * U32).add_(ref.abs(), alpha=U32 + extra)


# ---- strip heights (csrc/conv_args.h strip_rows(per_img, rows, step, want); the four rows: how s2d_ / s2u_ / d1_ / d1g_strip_rows of csrc/conv_*.hip call it)
_STRIP_RULE = {
    # kernel: (pixels per row segment (0 = whole rows), output channels per tile (0 = one tile), first R and step, workgroups wanted)
    's2d': (128, 128, 2, 240),
    's2u': (64, 64, 1, 240),
    'd1': (0, 64, 2, 480),
    'd1g': (128, 0, 1, 480),
}


def strip_rows(kernel, n, rows, width, co):
    """(R, strips, segments) for `rows` x `width` = the kernel's row grid: OUTPUT rows / pixels for s2d and d1, the phase grid (= INPUT rows / pixels) for s2u
    and d1g.  R = the tallest divisor of `rows` (even for s2d / d1) that still gives the wanted number of workgroups, else the smallest one."""
    seg_px, co_tile, step, want = _STRIP_RULE[kernel]
    segs = width // seg_px if seg_px else 1
    per_img = n * segs * (co // co_tile if co_tile else 1)
    best = 0
    for R in range(step, rows + 1, step):
        if rows % R:
            continue
        wgs = per_img * (rows // R)
        if best == 0 or wgs >= want:
            best = R
        if wgs < want:
            break
    return best, (rows // best if best else 0), segs


# ---- the comparer
def _hist(idx, n_show=8):
    v, c = torch.unique(idx, return_counts=True)
    order = torch.argsort(c, descending=True)[:n_show]
    more = '' if v.numel() <= n_show else f' (+{v.numel() - n_show} more values)'
    return '{' + ', '.join(f'{int(v[i])}: {int(c[i])}' for i in order) + '}' + more


def compare(got, ref, bnd, geom=None):
    """got: NHWC tensor of any dtype / device; ref, bnd: NHWC float64.  Returns (worst err / bound, report); report is '' when every element is in bound.
    geom (optional, for the report): {'kernel': 's2d' | 's2u' | 'd1' | 'd1g', 'R': strip height, 'row_div': output rows per strip row (2 for the
    phase kernels, whose strips count input rows)}, or {'bm': pixels per tile, 'step': output pixels per phase-grid pixel along each axis (2 for a
    four-phase plan)} for the tile family, whose tiles run over the flat pixel index (n, h, w) of the phase grid across images"""
    g = got.detach().to('cpu', torch.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    err = (g - ref).abs_()
    del g
    bad = err > bnd          # (a NaN in `got` compares False here: caught by the ratio below)
    exact = err == 0         # (an fp32 store has no absolute term: a padding channel's bound is 0 and its 0 / 0 is no error)
    ratio = err.div_(bnd).masked_fill_(exact, 0.0)
    del exact
    worst = float(ratio.nan_to_num_(nan=float('inf')).max())
    nbad = int(bad.sum())
    if nbad == 0 and worst <= 1.0:
        return worst, ''
    if nbad == 0:
        bad = ratio > 1.0
        nbad = int(bad.sum())
    n, h, w, c = bad.nonzero(as_tuple=True)
    lines = [f'{nbad} of {bad.numel()} elements out of bound ({100.0 * nbad / bad.numel():.3g} %), worst err/bound {worst:.4g}',
             f'  first: (n, h, w, c) = ({int(n[0])}, {int(h[0])}, {int(w[0])}, {int(c[0])})',
             f'  by image        {_hist(n)}',
             f'  by output row   {_hist(h)}']
    if geom and geom.get('R'):
        srow = h // geom.get('row_div', 1)
        lines.append(f"  strip height R = {geom['R']} ({'input' if geom.get('row_div', 1) > 1 else 'output'} rows)")
        lines.append(f"  by row mod R    {_hist(srow % geom['R'])}")
        lines.append(f"  by strip index  {_hist(srow // geom['R'])}")
    if geom and geom.get('bm'):
        st = geom.get('step', 1)
        hq, wq = -(-bad.shape[1] // st), -(-bad.shape[2] // st)
        flat = (n * hq + h // st) * wq + w // st
        lines.append(f"  tile of {geom['bm']} pixels (flat index over the {'phase grid' if st > 1 else 'output'}, images included)")
        lines.append(f"  by tile index   {_hist(flat // geom['bm'])}")
        lines.append(f"  by pixel in tile mod 32 {_hist(flat % geom['bm'] % 32)}")
        if st > 1:
            lines.append(f'  by phase (2 (h mod 2) + w mod 2) {_hist((h % st) * st + w % st)}')
    for m in (32, 64, 128):
        lines.append(f'  by pixel mod {m:<3d} {_hist(w % m)}')
    lines.append(f'  by channel mod 32 {_hist(c % 32)}')
    if geom and geom.get('kernel') == 's2d':
        # csrc/conv_s2d.hip: acc[j][q*4 + e] = output channel wave*32 + q*8 + lh*4 + e of pixel j*32 + lr; lane = lr + 32 * lh
        cc = c % 128
        wave, q, lh, e = cc // 32, (cc % 32) // 8, (cc % 8) // 4, cc % 4
        key = wave * 100 + ((w % 32) >= 16).long() * 10 + (q * 4 + e) % 8
        lines.append(f'  by wave*100 + (lane mod 32 >= 16)*10 + accumulator mod 8   {_hist(key, 12)}')
        lines.append(f'  by lane half (K half lh) {_hist(lh)}   by pixel block j {_hist((w % 128) // 32)}')
    return worst, '\n'.join(lines)
