"""Float64 reference, per-element bound, inputs and a CPU emulation (with named faults) for the weight-gradient kernels of csrc/wgrad.hip, wgrad_x3.h,
wgrad_c4.h and wgrad_w4.h -- TEST INFRASTRUCTURE ONLY (tests/test_wgrad_ref_host.py, tests/test_gpu_wgrad.py; the rows are tests/wgrad_cases.py).

descriptor_of(row)   the ONE place that says which tensor of a layer is the kernel's P and which its Q operand, with which step, padding, staged
                     activation and gradient layout: what engine.conv()'s backward passes to conv_wgrad (Conv2d: P = dL/dy, Q = x, the activation on Q;
                     ConvTranspose2d: P = x, Q = dL/dy, the activation on P; narrow 7x7 head: shift_stack(dL/dy) or the wgrad_c4 kernel).  The GPU test, the
                     emulation and the second (einsum) evaluation of the host test all take it from here.
reference()          dL/dw by torch.autograd through F.conv2d / F.conv_transpose2d in float64 (an explicitly padded layer through pad_ref.wgrad, i.e.
                     F.pad(mode=...) in front of a padding-0 conv).  It never looks at P / Q / taps: a wrong role, stride or transpose in descriptor_of cannot
                     cancel between kernel and reference.

Operand model -- the reference sees the values the kernel's documented arithmetic multiplies:
    'bf16'    bf16 storage, PREC_BF16      the stored values (inputs() pre-rounds them)
    'f32b'    fp32 storage, PREC_BF16      x.bfloat16() (raww_to_planes rounds once while staging)
    'strict'  fp32 storage, PREC_BF16X3    the fp32 values themselves
    a staged activation is act32(v) = torch.where(v > 0, v, v * 0.2) (or relu) in float32; under the two bf16 precisions it is rounded ONCE more to bf16
    (raww_to_planes / x3w_split4 apply the activation in fp32 and round to the 16-bit format), under strict it stays fp32.

bound(ref, S, K, policy, g0) -- S = the same gradient on |P| and |Q| (sum of |p||q| per element), K = products summed per element (pixels whose tap does not fall
into the zero padding; counted with a ones tensor):

    bf16 precisions   K * 2^-24 * S + 2^-24 * |ref + g0|
        every product of two bf16 values has 16 significant bits: exact in fp32.  What is left is ONE fp32 summation of K terms in some order: the MFMA's 32 (or
        64) pixels per step, the steps of a range, the split-K partials and their fixed-order reduce are all additions of the same sum, and any order of a
        length-K fp32 summation is within (K - 1) * 2^-24 * S (Higham, Accuracy and Stability of Numerical Algorithms, 4.2).  The K-th 2^-24 is generous by
        one rounding; the last term is the store, i.e. the rounding of the `accumulate` add onto g0 (g0 = 0 without: the sum is stored as it is).
    strict            (3 * 2^-16 * (1 + 2^-8) + 3K * 2^-24) * S + 2^-24 * |ref + g0|
        bfloat16 has 8 significant bits, so rounding to nearest leaves a relative error of at most u16 = 2^-8 (half an ulp of 2^-7; the 2^-9 one may expect is
        the typical size, not the worst case: v = 1 + 2^-8 rounds to 1).  hi = bf16(v) leaves |v - hi| <= 2^-8 |v|; v - hi is exact in fp32;
        lo = bf16(v - hi) leaves |v - hi - lo| <= 2^-8 |v - hi| <= 2^-16 |v|, and |lo| <= 2^-8 (1 + 2^-8) |v|.  The kernels add
        lo_p * hi_q + hi_p * lo_q + hi_p * hi_q = (hi_p + lo_p)(hi_q + lo_q) - lo_p * lo_q, so per product
            |p q - (three terms)| <= |p q - (hi_p + lo_p)(hi_q + lo_q)| + |lo_p lo_q| <= (2 * 2^-16 + 2^-32) |p q| + 2^-16 (1 + 2^-8)^2 |p q|
                                  <= 3 * 2^-16 * (1 + 2^-8) |p q|.
        (The first write-up of this bound took u16 = 2^-9, i.e. 3 * 2^-18; the emulation of the documented arithmetic itself then misses it by up to 1.7 x on
        the K = 8 and K = 35 rows -- test_wgrad_ref_host.py -- because the format's worst case is 2^-8.  The constant follows the format, not the measurement.)
        Each of the three terms is a product of two bf16 values (exact in fp32), so what is left is one fp32 summation of 3K terms in some order:
        3K * 2^-24 * S to first order (the magnitudes of the three terms sum to (1 + O(2^-7)) |p q|; like the u^2 terms of gamma_n = n u / (1 - n u) that
        2^-7 of the summation term is second order and is not carried).
    No fitted constant, no slack factor.

emulate(row, policy, splitk, ...)  torch float32 on the CPU in the documented order: staging (+ hi / lo split), K steps of 32 pixels (wgrad_kernel, the x3 kernels; the
    persistent c4 / w4 kernels are emulated in this form too: any order is inside the bound) or 64 pixels (wgrad_glds_kernel), per-range partials with pchunk as
    wgrad.hip computes it, the reduce in the order k = 0, 1, 2, ..., the scatter (stack_kw layout included) and `accumulate`.  MUTATIONS are small edits of it, each
    one fault the GPU test exists to catch; live(mutation, row, policy, splitk) says where a mutation changes anything."""
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

import pad_ref
from conv_ref import STRICT_REPR, U16, U32, _hist, act32, model_values  # noqa: F401  (the operand model and the strict constant live in conv_ref; re-exported)
from deepliif_amd import _lib as L
from deepliif_amd.geometry import ConvSpec, choose_wgrad_splitk, cpad

Desc = namedtuple('Desc', 'p_role q_role step pad pad_mode p_act q_act gshape CA CB k stack_kw')
_MODE = {L.PAD_ZERO: 'zero', L.PAD_REFLECT: 'reflect', L.PAD_REPLICATE: 'replicate'}


def spec_of(row):
    return ConvSpec(row.kind, row.cin, row.cout, row.k, row.stride, row.pad, row.pad_mode, row.out_pad)


def descriptor_of(row):
    """(layer) -> what the engine hands to conv_wgrad (engine.conv(), the `if w_needs:` branches of its backward)"""
    if row.form in ('stack', 'c4'):
        assert row.kind == 'conv' and row.pad_mode == L.PAD_ZERO and row.stride == 1
        return Desc('dy', 'x', 1, row.pad, L.PAD_ZERO, L.ACT_NONE, row.in_act, (row.cout, row.cin, row.k, row.k), row.cout, row.cin, row.k,
                    row.k if row.form == 'stack' else 0)
    if row.kind == 'conv':
        return Desc('dy', 'x', row.stride, row.pad, row.pad_mode, L.ACT_NONE, row.in_act, (row.cout, row.cin, row.k, row.k), row.cout, row.cin, row.k, 0)
    return Desc('x', 'dy', row.stride, row.pad, L.PAD_ZERO, row.in_act, L.ACT_NONE, (row.cin, row.cout, row.k, row.k), row.cin, row.cout, row.k, 0)


def storage_dtype(policy):
    return torch.bfloat16 if policy == 'bf16' else torch.float32


def prec_of(policy):
    return L.PREC_BF16X3 if policy == 'strict' else L.PREC_BF16


# ---- inputs
def _pad8(c):
    return (c + 7) // 8 * 8


def inputs(row, policy):
    """(x, dy, g0): float32 NHWC tensors holding the STORED values (exact in bf16 under 'bf16'; full mantissas otherwise), padding channels zero, N(0, 1), the
    first and the last pixel of every image scaled by 8 (a dropped or misplaced edge pixel then stands far above the summation term); g0 ~ N(0, 1) in the
    gradient's layout.  The seed depends on the row only."""
    g = torch.Generator().manual_seed(zlib.crc32(row.id.encode()))
    d = descriptor_of(row)
    ho, wo = spec_of(row).out_hw(row.H, row.W)

    def make(n, h, w, c, role):
        cp = _pad8(c) if (row.p_pad8 and d.p_role == role) else cpad(c)
        if row.form == 'stack' and role == 'dy':
            cp = cpad(c)
        t = torch.zeros(n, h, w, cp)
        v = torch.randn(n, h, w, c, generator=g)
        v[:, 0, 0] *= 8
        if h * w > 1:
            v[:, -1, -1] *= 8
        t[..., :c] = v.bfloat16().float() if policy == 'bf16' else v
        return t
    x = make(row.n, row.H, row.W, row.cin, 'x')
    dy = make(row.n, ho, wo, row.cout, 'dy')
    g0 = torch.randn(d.gshape, generator=g)
    return x, dy, g0


def shift_stack(dy, cout, kw, pad):
    """host model of dl_shift_stack: D[n, h, w, co * kw + k] = dy[n, h, w - (k - pad), co], zero outside"""
    n, h, w, _ = dy.shape
    D = torch.zeros(n, h, w, cpad(cout * kw), dtype=dy.dtype)
    idx = torch.arange(w)
    for k in range(kw):
        ws = idx - (k - pad)
        m = ((ws >= 0) & (ws < w)).to(dy.dtype)
        D[..., k:cout * kw:kw] = dy[:, :, ws.clamp(0, w - 1)][..., :cout] * m[None, None, :, None]
    return D


def operands(row, x, dy):
    """(P, Q) as the kernel takes them (host tensors; the stacked head's P is the host model of shift_stack)"""
    d = descriptor_of(row)
    t = {'x': x, 'dy': dy}
    P, Q = t[d.p_role], t[d.q_role]
    if d.stack_kw:
        P = shift_stack(P, row.cout, d.stack_kw, d.pad)
    return P, Q


# ---- reference
def _nchw(t, c):
    return t[..., :c].permute(0, 3, 1, 2).contiguous()


def _layer_wgrad(row, xv, gv):
    """dL/dw of the layer for NCHW float64 x and dL/dy, by autograd"""
    if row.kind == 'conv':
        w = torch.zeros(row.cout, row.cin, row.k, row.k, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xv, w, None, row.stride, row.pad)
    else:
        w = torch.zeros(row.cin, row.cout, row.k, row.k, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(xv, w, None, row.stride, row.pad, row.out_pad)
    assert y.shape == gv.shape, (y.shape, gv.shape)
    return torch.autograd.grad(y, w, gv)[0]


def reference(row, x, dy, policy):
    """(ref, S, K): float64 tensors in the gradient's layout ([Cout, Cin, k, k] for Conv2d, [Cin, Cout, k, k] for ConvTranspose2d); K per element (broadcastable)"""
    xe, ge = model_values(x, row.in_act, policy), model_values(dy, L.ACT_NONE, policy)
    if row.kind == 'conv' and row.pad_mode != L.PAD_ZERO:
        assert row.stride == 1
        ref, S, K = pad_ref.wgrad(ge, xe, row.cout, row.cin, row.k, _MODE[row.pad_mode], row.pad)
        return ref, S, torch.full((1, 1, row.k, row.k), float(K), dtype=torch.float64)
    xv, gv = _nchw(xe, row.cin), _nchw(ge, row.cout)
    ref = _layer_wgrad(row, xv, gv)
    S = _layer_wgrad(row, xv.abs(), gv.abs())
    one = row._replace(cin=1, cout=1)
    K = _layer_wgrad(one, torch.ones_like(xv[:, :1]), torch.ones_like(gv[:, :1]))          # [1, 1, k, k]: pixels per tap outside the zero padding
    return ref, S, K


def bound(ref, S, K, policy, g0=None):
    """the per-element bound of the module docstring (S is not modified)"""
    stored = ref if g0 is None else ref + g0.double()
    if policy == 'strict':
        return (STRICT_REPR + 3 * K * U32) * S + U32 * stored.abs()
    return K * U32 * S + U32 * stored.abs()


# ---- the comparer
def compare(got, want, bnd, d, cbp=None):
    """got: the kernel's gradient (any device), want = ref (+ g0), bnd: float64 in the gradient's layout.  Returns (worst err / bound, report); report is '' when every
    element is in bound, else it says WHERE the bad elements are: by ca mod 16, by j tile (j = tap * CBp + b; tiles of 128 and of 256), by tap, by b >= CB - 4"""
    g = got.detach().to('cpu', torch.float64)
    assert g.shape == want.shape, (g.shape, want.shape)
    err = (g - want).abs()
    ratio = (err / bnd).nan_to_num(nan=float('inf'))
    ratio[(err == 0) & (bnd == 0)] = 0.0
    worst = float(ratio.max())
    bad = ratio > 1.0
    nbad = int(bad.sum())
    if nbad == 0:
        return worst, ''
    a, b, kh, kw = bad.nonzero(as_tuple=True)
    cbp = cbp or cpad(d.CB)
    tap = kh * d.k + kw
    if d.stack_kw:          # kernel row = a * stack_kw + kw, tap = kh
        ca, j = a * d.stack_kw + kw, kh * cbp + b
    else:
        ca, j = a, tap * cbp + b
    lines = [f'{nbad} of {bad.numel()} elements out of bound ({100.0 * nbad / bad.numel():.3g} %), worst err/bound {worst:.4g}',
             f'  first: (a, b, kh, kw) = ({int(a[0])}, {int(b[0])}, {int(kh[0])}, {int(kw[0])})  got {float(g[a[0], b[0], kh[0], kw[0]]):.9g} '
             f'want {float(want[a[0], b[0], kh[0], kw[0]]):.9g} bound {float(bnd.expand_as(want)[a[0], b[0], kh[0], kw[0]]):.3g}',
             f'  by ca mod 16      {_hist(ca % 16, 16)}',
             f'  by ca // 128      {_hist(ca // 128)}',
             f'  by j tile (128)   {_hist(j // 128)}',
             f'  by j tile (256)   {_hist(j // 256)}',
             f'  by tap kh*k + kw  {_hist(tap, 16)}',
             f'  by b >= CB - 4    {_hist((b >= d.CB - 4).long())}   by b {_hist(b)}']
    return worst, '\n'.join(lines)


# ---- the emulation
MUTATIONS = ('drop_last_pixel', 'drop_range_last_pixel', 'empty_slab_junk', 'skip_last_slab', 'accumulate_ignores_g0', 'pad_reads_col0', 'last_row_step1',
             'act_not_rerounded', 'strict_drop_hi_lo', 'strict_q_lo_first_step_only', 'strict_last_pixel_lo_zero', 'pad_column_onto_last', 'stack_swaps_kh_kw',
             'ca_tail_from_tile0')


def kernel_form(row, policy):
    """(pixels per K step, pchunk rounding) of the kernel that serves the row"""
    return (64, 64) if (row.kernel.startswith('wgrad_glds_kernel') and policy == 'bf16') else (32, 32)


def effective_splitk(row, policy, splitk, P, Q):
    """the split-K the emulation runs: a forced value as it is; the automatic one as ops.HipBackend.conv_wgrad chooses it for the general-path kernels (the persistent
    c4 / w4 kernels partition their work in their own way: emulated as one range)"""
    if splitk is not None:
        return splitk
    if row.kernel in ('wgrad_c4', 'wgrad_w4_kernel'):
        return 1
    _, tiles, ksteps, name = plan(L.load(), wgrad_desc(row, policy, 1, P.shape, Q.shape))
    return choose_wgrad_splitk(name, tiles, ksteps, P.shape[0] * P.shape[1] * P.shape[2])


def ranges(ptot, splitk, round_to):
    pchunk = ((ptot + splitk - 1) // splitk + round_to - 1) // round_to * round_to
    return [(min(ptot, k * pchunk), min(ptot, (k + 1) * pchunk)) for k in range(splitk)]


def live(mutation, row, policy, splitk):
    """does `mutation` change anything on this launch?  (row, policy, EFFECTIVE splitk)"""
    d = descriptor_of(row)
    x, dy, _ = _shapes(row)
    P = {'x': x, 'dy': dy}[d.p_role]
    ptot = P[0] * P[1] * P[2]
    bp, rnd = kernel_form(row, policy)
    rg = ranges(ptot, splitk, rnd)
    act = d.p_act if d.p_act != L.ACT_NONE else d.q_act
    return {
        'drop_last_pixel': True,
        'drop_range_last_pixel': splitk >= 2 and rg[1][1] > rg[1][0],
        'empty_slab_junk': any(e == b for b, e in rg),
        'skip_last_slab': splitk >= 2 and rg[-1][1] > rg[-1][0],
        'accumulate_ignores_g0': True,           # (with accumulate = True)
        'pad_reads_col0': d.pad_mode == L.PAD_ZERO and d.pad > 0 and not d.stack_kw,
        'last_row_step1': d.step > 1 and P[1] > 1,
        'act_not_rerounded': policy != 'strict' and (act == L.ACT_LRELU or (act == L.ACT_RELU and policy == 'f32b')),
        'strict_drop_hi_lo': policy == 'strict',
        'strict_q_lo_first_step_only': policy == 'strict' and any(e - b > bp for b, e in rg),
        'strict_last_pixel_lo_zero': policy == 'strict',
        'pad_column_onto_last': cpad(d.CB) > d.CB,
        'stack_swaps_kh_kw': bool(d.stack_kw),
        'ca_tail_from_tile0': P[3] == 136,
    }[mutation]


def _shapes(row):
    d = descriptor_of(row)
    ho, wo = spec_of(row).out_hw(row.H, row.W)

    def cp(c, role):
        if d.stack_kw and role == 'dy':
            return cpad(c * d.stack_kw)
        return _pad8(c) if (row.p_pad8 and d.p_role == role) else cpad(c)
    return (row.n, row.H, row.W, cp(row.cin, 'x')), (row.n, ho, wo, cp(row.cout, 'dy')), d.gshape


def _border(mode, i, n):
    if mode == L.PAD_REFLECT:
        i = i.abs()
        return torch.where(i >= n, 2 * n - 2 - i, i)
    return i.clamp(0, n - 1)


def _split(v, policy, act, reround=True):
    """staging: (hi, lo) float32 planes of the stored tensor v (lo is None under the bf16 precisions)"""
    a = act32(act, v.float())
    if policy == 'strict':
        hi = a.bfloat16().float()
        return hi, (a - hi).bfloat16().float()
    if act != L.ACT_NONE and not reround:
        return a, None
    return a.bfloat16().float(), None


def emulate(row, policy, splitk, accumulate=False, mutation=None, data=None):
    """the gradient (float32, the layout of descriptor_of(row).gshape) as the documented arithmetic produces it; `mutation`: one of MUTATIONS"""
    assert mutation is None or mutation in MUTATIONS, mutation
    d = descriptor_of(row)
    x, dy, g0 = data if data is not None else inputs(row, policy)
    P, Q = operands(row, x, dy)
    splitk = effective_splitk(row, policy, splitk, P, Q)
    N, Hp, Wp, CAp = P.shape
    _, Hq, Wq, CBp = Q.shape
    KH, KW = d.k, (1 if d.stack_kw else d.k)
    pad_w = 0 if d.stack_kw else d.pad
    KK, J, ptot = KH * KW, KH * KW * CBp, N * Hp * Wp
    bp, rnd = kernel_form(row, policy)
    reround = mutation != 'act_not_rerounded'
    Ph, Pl = _split(P.reshape(ptot, CAp), policy, d.p_act, reround)
    Qh4, Ql4 = _split(Q, policy, d.q_act, reround)

    # the gather: pixel p = (n, h, w), tap t = (kh, kw) -> Q[n, h * step - pad + kh, w * step - pad_w + kw]
    p = torch.arange(ptot)
    n_i, h_i, w_i = p // (Hp * Wp), (p % (Hp * Wp)) // Wp, p % Wp
    t = torch.arange(KK)
    kh, kw = t // KW, t % KW
    hstep = torch.full_like(h_i, d.step)
    if mutation == 'last_row_step1':
        hstep[h_i == Hp - 1] = 1
    hq = (h_i * hstep)[:, None] - d.pad + kh[None, :]
    wq = (w_i * d.step)[:, None] - pad_w + kw[None, :]
    if d.pad_mode == L.PAD_ZERO:
        if mutation == 'pad_reads_col0':
            wq = torch.where(wq == -1, torch.zeros_like(wq), wq)
        ok = (hq >= 0) & (hq < Hq) & (wq >= 0) & (wq < Wq)
        hq, wq = hq.clamp(0, Hq - 1), wq.clamp(0, Wq - 1)
    else:
        ok = torch.ones_like(hq, dtype=torch.bool)
        hq, wq = _border(d.pad_mode, hq, Hq), _border(d.pad_mode, wq, Wq)
    okf = ok.float()[:, :, None]

    def gather(q4):
        return (q4[n_i[:, None], hq, wq] * okf).reshape(ptot, J)
    Qh = gather(Qh4)
    Ql = gather(Ql4) if Ql4 is not None else None
    if mutation == 'drop_last_pixel':
        Ph = Ph.clone()
        Ph[ptot - 1] = 0
        if Pl is not None:
            Pl = Pl.clone()
            Pl[ptot - 1] = 0
    if mutation == 'strict_last_pixel_lo_zero':
        if Pl is not None:
            Pl, Ql = Pl.clone(), Ql.clone()
            Pl[ptot - 1] = 0
            Ql[ptot - 1] = 0

    rg = ranges(ptot, splitk, rnd)
    slabs = []
    junk = torch.Generator().manual_seed(99)
    for ks, (b, e) in enumerate(rg):
        if e == b and mutation == 'empty_slab_junk':
            slabs.append(torch.randn(CAp, J, generator=junk))
            continue
        if mutation == 'drop_range_last_pixel' and ks == 0 and splitk >= 2:
            e_drop = e - 1
        else:
            e_drop = -1
        acc = torch.zeros(CAp, J)
        for step, s0 in enumerate(range(b, e, bp)):
            s1 = min(e, s0 + bp)
            ph, qh = Ph[s0:s1], Qh[s0:s1]
            if e_drop >= s0 and e_drop < s1:
                ph = ph.clone()
                ph[e_drop - s0] = 0
            if Pl is not None:
                pl, ql = Pl[s0:s1], Ql[s0:s1]
                if e_drop >= s0 and e_drop < s1:
                    pl = pl.clone()
                    pl[e_drop - s0] = 0
                if mutation == 'strict_q_lo_first_step_only' and step >= 1:
                    ql = torch.zeros_like(ql)
                acc = acc + pl.t() @ qh
                if mutation != 'strict_drop_hi_lo':
                    acc = acc + ph.t() @ ql
            acc = acc + ph.t() @ qh
        if mutation == 'ca_tail_from_tile0' and CAp > 128 and CAp % 128:
            acc[128:] = acc[:CAp - 128]
        slabs.append(acc)
    if mutation == 'skip_last_slab' and splitk >= 2:
        slabs = slabs[:-1]
    s = torch.zeros(CAp, J)
    for slab in slabs:          # k = 0, 1, 2, ...
        s = s + slab
    s = s.view(CAp, KK, CBp)
    if mutation == 'pad_column_onto_last' and CBp > d.CB:
        s = s.clone()
        s[:, :, d.CB - 1] = s[:, :, d.CB]
    if d.stack_kw:
        r = s[:d.CA * d.stack_kw, :, :d.CB].reshape(d.CA, d.stack_kw, KH, d.CB).permute(0, 3, 2, 1)          # [a][b][kh][kw]
        if mutation == 'stack_swaps_kh_kw':
            r = r.transpose(2, 3)
        r = r.contiguous()
    else:
        r = s[:d.CA, :, :d.CB].permute(0, 2, 1).reshape(d.CA, d.CB, KH, KW).contiguous()
    if accumulate and mutation != 'accumulate_ignores_g0':
        r = g0 + r
    return r


# ---- the C-ABI descriptor (as ops.HipBackend.conv_wgrad fills it) and the routing question
def wgrad_desc(row, policy, splitk, p_shape, q_shape, accumulate=False, p_pstride=None, q_pstride=None, p_split=False, q_split=False):
    d = descriptor_of(row)
    w = L.WgradDesc()
    w.N, w.Hp, w.Wp, w.CAp = p_shape
    _, w.Hq, w.Wq, w.CBp = q_shape
    w.p_pstride, w.q_pstride = p_pstride or w.CAp, q_pstride or w.CBp
    w.KH = w.KW = d.k
    w.step, w.pad, w.pad_mode = d.step, d.pad, d.pad_mode
    w.CA, w.CB = d.CA, d.CB
    w.pad_w, w.stack_kw = -1, 0
    if d.stack_kw:
        w.KW, w.pad_w, w.stack_kw, w.CA = 1, 0, d.stack_kw, d.CA * d.stack_kw
    w.dtype, w.prec = (L.DL_BF16 if policy == 'bf16' else L.DL_F32), prec_of(policy)
    w.accumulate = 1 if accumulate else 0
    w.p_act, w.q_act = d.p_act, d.q_act
    w.p_split, w.q_split = int(p_split), int(q_split)
    w.splitk = splitk
    return w


def plan(lib, w):
    """(multi, tiles, ksteps, name) of dl_wgrad_plan"""
    import ctypes as C
    t, k, nm = L.i32(), L.i32(), C.c_char_p()
    rc = int(lib.dl_wgrad_plan(C.byref(w), C.byref(t), C.byref(k), C.byref(nm)))
    return rc, t.value, k.value, (nm.value or b'').decode()
