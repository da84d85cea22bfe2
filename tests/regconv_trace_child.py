"""Child process of tests/test_gpu_regconv_sweep.py::test_kernel_names_match_the_traced_launches -- not a test module.

Run under `rocprofv3 --kernel-trace`: one small dl_conv_forward per route of the dispatch (the six weights-in-registers kernels with and without fused
statistics, with and without a bias, one dl_conv_forward_add, a few fallbacks, then the kernels of the tile family) and, for each, one line

    ROUTE <label> <dl_conv_kernel_name of the descriptor that was launched>

in launch order.  The parent compares these names with the convolution kernels of the trace.  `--names` prints the same lines without a GPU (descriptors
only), for the host check of the table."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import regconv_cases as RC  # noqa: E402
from deepliif_amd import _lib as L  # noqa: E402
from deepliif_amd import ops  # noqa: E402
from deepliif_amd.geometry import ConvSpec  # noqa: E402

S2D = ('s2d', 'conv', 64, 128, 2, 16, 256, 'fwd', None)
S2U = ('s2u', 'convT', 128, 64, 2, 8, 64, 'fwd', None)
D1 = ('d1', 'conv', 6, 64, 2, 8, 512, 'fwd', None)
D1G = ('d1g', 'conv', 6, 64, 2, 8, 256, 'dgrad', None)
D1_BENCHED = ('d1', 'conv', 6, 64, 16, 512, 512, 'fwd', None)
D1G_BENCHED = ('d1g', 'conv', 6, 64, 16, 512, 512, 'dgrad', None)
DOTF = ('dotf', 'conv', 512, 1, 2, 8, 8, 'fwd', None)
DOTG = ('dotg', 'conv', 512, 1, 2, 8, 8, 'dgrad', None)
G128, G64, G16 = 'conv_gemm_glds_kernel<128,128,64>', 'conv_gemm_glds_kernel<128,64,64>', 'conv_gemm_glds_kernel<256,16,32>'

# label, case, keywords (act, bias, want_stats), the kernel this route is meant to reach
ROUTES = [
    ('s2d', S2D, {}, 'conv_s2d_kernel'),
    ('s2d+relu', S2D, {'act': L.ACT_RELU}, 'conv_s2d_kernel'),
    ('s2d+stats', S2D, {'want_stats': True}, 'conv_s2d_kernel'),
    ('s2d-bias', S2D, {'bias': False}, 'conv_s2d_kernel'),
    ('s2d-bias+stats', S2D, {'bias': False, 'want_stats': True}, 'conv_s2d_kernel'),
    ('s2d+tanh(fallback)', S2D, {'act': L.ACT_TANH}, G128),
    ('s2d+tanh+stats(fallback,no-chunks)', S2D, {'act': L.ACT_TANH, 'want_stats': True}, G128),
    ('s2u', S2U, {}, 'conv_s2u_kernel'),
    ('s2u+stats', S2U, {'want_stats': True}, 'conv_s2u_kernel'),
    ('s2u-bias', S2U, {'bias': False}, 'conv_s2u_kernel'),
    ('s2u-bias+stats', S2U, {'bias': False, 'want_stats': True}, 'conv_s2u_kernel'),
    ('s2u+tanh(fallback)', S2U, {'act': L.ACT_TANH}, G64),
    ('d1', D1, {'act': L.ACT_LRELU}, 'conv_d1_kernel'),
    ('d1-bias', D1, {'bias': False}, 'conv_d1_kernel'),
    ('d1+stats(no-chunks)', D1, {'want_stats': True}, 'conv_d1_kernel'),
    ('d1+tanh(fallback)', D1, {'act': L.ACT_TANH}, G64),
    ('d1g', D1G, {}, 'conv_d1g_kernel'),
    ('d1g+stats(no-chunks)', D1G, {'want_stats': True}, 'conv_d1g_kernel'),
    ('d1g+bias(fallback)', D1G, {'bias': True}, G16),
    # the benched discriminator batch: shapes where the 480-workgroup threshold of d1_strip_rows / d1g_strip_rows decides R (the parent checks the traced grids)
    ('d1@16x512x512', D1_BENCHED, {'act': L.ACT_LRELU}, 'conv_d1_kernel'),
    ('d1g@16x512x512', D1G_BENCHED, {}, 'conv_d1g_kernel'),
    ('dot_fwd', DOTF, {}, 'conv_dot_fwd_kernel'),
    ('dot_fwd+stats(no-chunks)', DOTF, {'want_stats': True}, 'conv_dot_fwd_kernel'),
    ('dot_fwd-bias(fallback)', DOTF, {'bias': False}, G16),
    ('dot_dgrad', DOTG, {}, 'conv_dot_dgrad_kernel'),
    ('dot_dgrad+bias(fallback)', DOTG, {'bias': True}, G128),
]
ADD_SPEC, ADD_SHAPE = ConvSpec('conv', 256, 256, 3, 1, 1, L.PAD_ZERO, 0), (4, 128, 128)          # the ResnetBlock shape: dl_conv_forward_add (conv_gemm_w4_kernel)


def _block(pad_mode):
    return ConvSpec('conv', 256, 256, 3, 1, 1, pad_mode, 0)


# the tile family, one forward launch per kernel at the smallest shape that reaches it: label, layer, N x H x W, strict policy?, input activation, the kernel
TILE_ROUTES = [
    ('w4@224-tiles', _block(L.PAD_ZERO), (4, 112, 128), False, L.ACT_NONE, 'conv_gemm_w4_kernel'),           # exactly the 224 tiles of the big-tile rule
    ('w4+replicate@8-tiles', _block(L.PAD_REPLICATE), (1, 16, 128), False, L.ACT_NONE, 'conv_gemm_w4_kernel'),
    ('8ph', _block(L.PAD_ZERO), (1, 256, 256), False, L.ACT_NONE, 'conv_gemm_8ph_kernel'),                    # rows not 128 pixels wide
    ('glds256+reflect', _block(L.PAD_REFLECT), (1, 256, 256), False, L.ACT_NONE, 'conv_gemm_glds_kernel<256,256,64>'),
    ('gather+lrelu-input', ConvSpec('conv', 64, 128, 3, 2, 1), (1, 16, 16), False, L.ACT_LRELU, 'conv_gemm_kernel<bf16>'),
    ('8ph_x3@224-tiles', _block(L.PAD_ZERO), (4, 112, 128), True, L.ACT_NONE, 'conv_gemm_8ph_x3_kernel'),
    ('glds_x3@8-tiles', _block(L.PAD_ZERO), (1, 16, 128), True, L.ACT_NONE, 'conv_gemm_glds_x3_kernel<128,128>'),
]


def tile_descriptor(spec, shape, strict, in_act):
    n, h, w = shape
    oh, ow = spec.out_hw(h, w)
    dtype, prec = (L.DL_F32, L.PREC_BF16X3) if strict else (L.DL_BF16, L.PREC_BF16)
    return RC.fill_conv_desc(spec.forward_plan(), n, h, w, RC.cpad(spec.cin), oh, ow, RC.cpad(spec.cout), RC.cpad(spec.cout), oh, ow, dtype, prec, L.ACT_NONE,
                             in_act, spec.cout, 1)


C_ABI_ROUTES = [('d1g+bias-pointer-without-entries', D1G, (64, 6, 4, 4)), ('dot_dgrad+bias-pointer-without-entries', DOTG, (1, 512, 4, 4))]


def route_cases():
    """label -> case of every route, in launch order (the parent derives the expected launch grids of the strip kernels from the cases)"""
    return [(label, case) for label, case, _, _ in ROUTES] + [(label, case) for label, case, _ in C_ABI_ROUTES] + [('conv_forward_add', None)] + \
        [(row[0], None) for row in TILE_ROUTES]


def workgroups(case):
    """workgroups the strip kernels launch for a case: images x row segments x strips x channel tiles, with R from the restated strip rule"""
    n, rows, width, co = RC.strip_grid(case)
    _, nstrips, segs = RC.strips(case)
    tiles_n = {'s2d': co // 128, 's2u': co // 64, 'd1': co // 64, 'd1g': 1}[case[0]]
    return n * segs * nstrips * tiles_n


def route_descriptor(case, kw):
    bias = kw.get('bias', case[7] == 'fwd')
    bias_n = (RC.geometry(case)[7] if case[7] == 'dgrad' else RC.spec_of(case).cout) if bias else 0
    return RC.descriptor(case, act=kw.get('act', L.ACT_NONE), bias_n=bias_n), bias_n


def names_only():
    lib = L.load()
    for label, case, kw, want in ROUTES:
        d, _ = route_descriptor(case, kw)
        print(f'ROUTE {label} {RC.kernel_name(lib, d)}')
        assert RC.kernel_name(lib, d) == want, (label, RC.kernel_name(lib, d), want)
    for label, case, _ in C_ABI_ROUTES:
        print(f'ROUTE {label} {RC.kernel_name(lib, RC.descriptor(case, bias_n=0))}')
    n, h, w = ADD_SHAPE
    d = RC.fill_conv_desc(ADD_SPEC.dgrad_plan(), n, h, w, 256, h, w, 256, 256, h, w, L.DL_BF16, L.PREC_BF16, L.ACT_NONE, L.ACT_NONE, 0, 1)
    assert lib.dl_conv_add_supported(C.byref(d)) and RC.kernel_name(lib, d) == 'conv_gemm_w4_kernel'
    print(f'ROUTE conv_forward_add {RC.kernel_name(lib, d)}')
    for label, spec, shape, strict, in_act, want in TILE_ROUTES:
        name = RC.kernel_name(lib, tile_descriptor(spec, shape, strict, in_act))
        print(f'ROUTE {label} {name}')
        assert name == want, (label, name, want)


def main():
    assert torch.cuda.is_available()
    be = ops.impl()
    dev = 'cuda'
    g = torch.Generator().manual_seed(0)
    for label, case, kw, want in ROUTES:
        plan, n, hi, wi, cip, ho, wo, cop, hq, wq = RC.geometry(case)
        spec = RC.spec_of(case)
        _, bias_n = route_descriptor(case, kw)
        wshape = (spec.cout, spec.cin, spec.k, spec.k) if spec.kind == 'conv' else (spec.cin, spec.cout, spec.k, spec.k)
        w = (torch.randn(wshape, generator=g) * 0.05).to(dev)
        packed = ops.PackedWeights(plan, dev, False)
        be.pack_weights(packed, w)
        x = torch.randn((n, hi, wi, cip), generator=g).bfloat16().to(dev)
        out = torch.empty((n, ho, wo, cop), dtype=torch.bfloat16, device=dev)
        bias = torch.randn(bias_n, generator=g).to(dev) if bias_n else None
        nch = be.conv_forward(packed, x, out, hq, wq, bias, kw.get('act', L.ACT_NONE), L.ACT_NONE, L.PREC_BF16, splitk=1, want_stats=kw.get('want_stats', False))
        torch.cuda.synchronize()
        name = be.last_conv_kernel
        assert name == want, (label, name, want)
        assert bool(nch) == (kw.get('want_stats', False) and case[0] in ('s2d', 's2u') and kw.get('act', L.ACT_NONE) == L.ACT_NONE), (label, nch)
        print(f'ROUTE {label} {name}', flush=True)
    # the C ABI directly: a bias POINTER with bias_n = 0 is no bias -- dl_conv_kernel_name says conv_d1g_kernel / conv_dot_dgrad_kernel, and that is what must run
    for label, case, wshape in C_ABI_ROUTES:
        plan, n, hi, wi, cip, ho, wo, cop, hq, wq = RC.geometry(case)
        d = RC.descriptor(case, bias_n=0)
        packed = ops.PackedWeights(plan, dev, False)
        be.pack_weights(packed, (torch.randn(wshape, generator=g) * 0.05).to(dev))
        x = torch.randn((n, hi, wi, cip), generator=g).bfloat16().to(dev)
        out = torch.empty((n, ho, wo, cop), dtype=torch.bfloat16, device=dev)
        unused = torch.zeros(cop, device=dev)
        be.check(be.lib.dl_conv_forward(C.byref(d), ops._ptr(x), ops._ptr(packed.hi), ops._ptr(packed.lo), ops._ptr(unused), ops._ptr(out), None, None, ops._stream()),
                 'dl_conv_forward')
        torch.cuda.synchronize()
        print(f'ROUTE {label} {RC.kernel_name(be.lib, d)}', flush=True)
    n, h, w_ = ADD_SHAPE
    plan = ADD_SPEC.dgrad_plan()
    w = (torch.randn((256, 256, 3, 3), generator=g) * 0.05).to(dev)
    packed = ops.PackedWeights(plan, dev, False)
    be.pack_weights(packed, w)
    x = torch.randn((n, h, w_, 256), generator=g).bfloat16().to(dev)
    addend = torch.randn((n, h, w_, 256), generator=g).bfloat16().to(dev)
    out = torch.empty_like(addend)
    assert be.conv_forward_add(packed, x, addend, out, h, w_, L.PREC_BF16), 'dl_conv_forward_add is not available for the ResnetBlock shape'
    torch.cuda.synchronize()
    print(f'ROUTE conv_forward_add {be.last_conv_kernel}', flush=True)
    for label, spec, (n, h, w_), strict, in_act, want in TILE_ROUTES:
        plan = spec.forward_plan()
        oh, ow = spec.out_hw(h, w_)
        packed = ops.PackedWeights(plan, dev, strict)          # (the strict policy reads a lo weight plane)
        be.pack_weights(packed, (torch.randn((spec.cout, spec.cin, spec.k, spec.k), generator=g) * 0.05).to(dev))
        x = torch.randn((n, h, w_, RC.cpad(spec.cin)), generator=g).to(torch.float32 if strict else torch.bfloat16).to(dev)
        out = torch.empty((n, oh, ow, RC.cpad(spec.cout)), dtype=x.dtype, device=dev)
        bias = torch.randn(spec.cout, generator=g).to(dev)
        be.conv_forward(packed, x, out, oh, ow, bias, L.ACT_NONE, in_act, L.PREC_BF16X3 if strict else L.PREC_BF16, splitk=1)
        torch.cuda.synchronize()
        name = be.last_conv_kernel
        assert name == want, (label, name, want)
        print(f'ROUTE {label} {name}', flush=True)
    print('CHILD DONE', flush=True)


if __name__ == '__main__':
    names_only() if '--names' in sys.argv[1:] else main()
