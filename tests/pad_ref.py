"""Float64 reference for a 3x3-style convolution behind an explicit border pad -- TEST INFRASTRUCTURE ONLY (tests/test_replicate_host.py,
tests/test_gpu_replicate.py).

forward      F.conv2d(F.pad(x, (p, p, p, p), mode=...), w, bias) in float64 on the CPU -- for 'replicate' what nn.ReplicationPad2d(p) + Conv2d(padding=0) of the
             reference's ResnetBlock compute (networks.py:482-483 / 499-500)
gradients    torch.autograd on that very expression: d/dx for a given dL/dy (the data gradient) and d/dw (the weight gradient)
Nothing here uses the project's tap tables (geometry.GatherPlan) or its border map, so an error in them cannot cancel between kernel and reference.

Bounds -- the derived ones of tests/conv_ref.py (bound() and compare() are imported from there, not copied): operands are pre-rounded to the 16-bit
format, so every product is exact in fp32 and what remains is the fp32 summation and the rounding of the stored value:
    forward, data gradient   u * |ref| + K * 2^-24 * S + 2^-24      S = the same expression on |x| (replicate-padded) and |w| (+ |bias|), K = 9 * Cin (+ 1 with a
                             bias) at EVERY element: with a copied border no tap is an exact zero.  Data gradient: S = the same gradient on |dy| and |w|; every
                             padded position sums 9 * Cout products and the fold adds up to (p + 1)^2 of them, so K = 9 * Cout * (folded positions)
    weight gradient (fp32)   K * 2^-24 * S + 2^-24 * |ref|          K = N * H * W products per element, S = sum |dy| * |x padded|
NHWC in and out, channel counts padded to the engine's (cpad), padding channels zero."""
import torch
import torch.nn.functional as F

from conv_ref import U32, bound, compare  # noqa: F401  (re-exported: the tests take both from here)
from deepliif_amd.geometry import cpad

MODES = {'zero': 'constant', 'reflect': 'reflect', 'replicate': 'replicate'}


def _nchw(t, c):
    return t[..., :c].double().permute(0, 3, 1, 2).contiguous()


def _nhwc(t, c):
    out = torch.zeros(t.shape[0], t.shape[2], t.shape[3], cpad(c), dtype=torch.float64)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out


def conv64(x, w, bias=None, mode='replicate', pad=1):
    """NCHW float64: the padded convolution itself"""
    return F.conv2d(F.pad(x, (pad, pad, pad, pad), mode=MODES[mode]), w, bias)


def _relu64(v, relu):
    return torch.relu(v) if relu else v


def forward(x, w, bias=None, relu=False, mode='replicate', pad=1):
    """x NHWC (padding channels ignored), w [Cout, Cin, k, k], bias [Cout] or None -> (ref, S, K): NHWC float64 padded to cpad(Cout); K a python int"""
    cout, cin = w.shape[0], w.shape[1]
    xv, wv = _nchw(x, cin), w.double()
    bv = None if bias is None else bias.double()
    ref = _relu64(conv64(xv, wv, bv, mode, pad), relu)
    S = conv64(xv.abs(), wv.abs(), None if bv is None else bv.abs(), mode, pad)
    return _nhwc(ref, cout), _nhwc(S, cout), w.shape[2] * w.shape[3] * cin + (0 if bias is None else 1)


def dgrad(dy, w, hw, mode='replicate', pad=1):
    """dL/dx of conv64 for dL/dy = dy (NHWC), by autograd -> (ref, S, K): NHWC float64 padded to cpad(Cin); K = [1, H, W, 1] products summed per element"""
    cout, cin = w.shape[0], w.shape[1]
    n = dy.shape[0]
    g, wv = _nchw(dy, cout), w.double()

    def grad_of(gv, wq):
        xv = torch.zeros(n, cin, hw[0], hw[1], dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(conv64(xv, wq, None, mode, pad), xv, gv)[0]
    ref, S = grad_of(g, wv), grad_of(g.abs(), wv.abs())
    ones = torch.ones(1, 1, hw[0], hw[1], dtype=torch.float64, requires_grad=True)
    cnt = torch.autograd.grad(conv64(ones, torch.ones(1, 1, w.shape[2], w.shape[3], dtype=torch.float64), None, mode, pad).sum(), ones)[0]
    return _nhwc(ref, cin), _nhwc(S, cin), (cnt * cout).permute(0, 2, 3, 1).contiguous()


def wgrad(dy, x, cout, cin, k=3, mode='replicate', pad=1):
    """dL/dw of conv64 for dL/dy = dy, by autograd -> (ref, S, K): [Cout, Cin, k, k] float64; K = N * H * W"""
    g, xv = _nchw(dy, cout), _nchw(x, cin)

    def grad_of(gv, xq):
        wv = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(conv64(xq, wv, None, mode, pad), wv, gv)[0]
    return grad_of(g, xv), grad_of(g.abs(), xv.abs()), dy.shape[0] * dy.shape[1] * dy.shape[2]


def wgrad_bound(ref, S, K):
    """fp32 result: no storage rounding beyond fp32's own (2^-24 * |ref|); S is consumed"""
    return S.mul_(K * U32).add_(ref.abs(), alpha=U32)


def border_mask(h, w):
    """[h, w] bool: the border rows / columns, where the three padding modes differ"""
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m
