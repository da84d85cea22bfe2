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

strip_rows(): a restatement of strip_rows() of csrc/conv_args.h as csrc/conv_{s2d,s2u,d1,d1g}.hip call it; used as a coverage guard only (the sweep asserts which strip
heights its table exercises) and cross-checked against the library through dl_conv_stats_chunks (tests/test_dispatch_host.py)."""
import torch
import torch.nn.functional as F

from deepliif_amd import _lib as L
from deepliif_amd.geometry import cpad

U_STORE = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U32 = 2.0 ** -24


def _act64(act, v):
    if act == L.ACT_RELU:
        return torch.relu(v)
    if act == L.ACT_LRELU:
        return torch.where(v > 0, v, 0.2 * v)
    assert act == L.ACT_NONE, act
    return v


def _op(spec, direction, x, w, in_hw):
    """the layer (direction 'fwd') or its transpose (direction 'dgrad') on NCHW float64 tensors"""
    s, p = spec.stride, spec.pad
    transposed = (spec.kind == 'convT') == (direction == 'fwd')
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

    def __init__(self, spec, direction, x, w, in_hw=None):
        assert spec.pad_mode == L.PAD_ZERO, 'zero padding only'
        c_in = spec.cin if direction == 'fwd' else spec.cout
        self.c_out = spec.cout if direction == 'fwd' else spec.cin
        xv = x[..., :c_in].double().permute(0, 3, 1, 2).contiguous()
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


def bound(ref, S, K, dtype, sum_slack=1):
    """the per-element bound; S is consumed (overwritten in place: the tensors of the large cases are ~1 GB each)"""
    return S.mul_(K).mul_(sum_slack * U32).add_(ref.abs(), alpha=U_STORE[dtype]).add_(U32)


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
    phase kernels, whose strips count input rows)}"""
    g = got.detach().to('cpu', torch.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    err = (g - ref).abs_()
    del g
    bad = err > bnd          # (a NaN in `got` compares False here: caught by the ratio below)
    ratio = err.div_(bnd)
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
