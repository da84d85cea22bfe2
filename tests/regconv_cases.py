"""The shapes of the weights-in-registers convolution kernels (conv_s2d, conv_s2u, conv_d1, conv_d1g, conv_dot_fwd / dgrad) that
tests/test_gpu_regconv_sweep.py runs on the GPU and tests/test_dispatch_host.py checks against the dispatch on the host -- TEST INFRASTRUCTURE ONLY.

A case is (kernel, kind, cin, cout, N, H, W, direction, R): the layer (kind / cin / cout; kernel size, stride and padding follow from the kernel family),
N x H x W of the LAYER INPUT, the direction that reaches the kernel, and the strip height the kernel's *_strip_rows rule picks for it today (None for the dot
kernels, which have no strips).  R is restated by conv_ref.strip_rows and, for s2d / s2u, checked against the library (dl_conv_stats_chunks); the coverage
guard below keeps the table from collapsing onto a few values of R when somebody changes a rule."""
import ctypes as C

import conv_ref
from deepliif_amd import _lib as L
from deepliif_amd.geometry import ConvSpec, cpad, fill_conv_desc

KERNEL_NAME = {'s2d': 'conv_s2d_kernel', 's2u': 'conv_s2u_kernel', 'd1': 'conv_d1_kernel', 'd1g': 'conv_d1g_kernel', 'dotf': 'conv_dot_fwd_kernel',
               'dotg': 'conv_dot_dgrad_kernel'}

S2D_CASES = [
    ('s2d', 'conv', 64, 128, 1, 512, 512, 'fwd', 2),          # batch-1 inference: 128 strips of 2 rows
    ('s2d', 'conv', 64, 128, 2, 512, 512, 'fwd', 4),
    ('s2d', 'conv', 64, 128, 4, 512, 512, 'fwd', 8),
    ('s2d', 'conv', 64, 128, 5, 480, 512, 'fwd', 10),
    ('s2d', 'conv', 64, 128, 8, 384, 512, 'fwd', 12),
    ('s2d', 'conv', 64, 128, 7, 420, 256, 'fwd', 6),          # 35 strips
    ('s2d', 'conv', 64, 128, 16, 256, 256, 'fwd', 8),
    ('s2d', 'conv', 64, 128, 1, 1024, 1024, 'fwd', 8),        # four row segments
    ('s2d', 'conv', 64, 128, 2, 12, 768, 'fwd', 2),           # three row segments
    ('s2d', 'conv', 64, 128, 1, 4, 256, 'fwd', 2),            # one strip = the whole image
    ('s2d', 'conv', 64, 256, 3, 512, 256, 'fwd', 4),          # two channel tiles
    ('s2d', 'convT', 128, 64, 1, 256, 256, 'dgrad', 2),       # data gradient of up2
    ('s2d', 'convT', 128, 64, 2, 256, 256, 'dgrad', 4),
    ('s2d', 'convT', 128, 64, 4, 256, 256, 'dgrad', 8),
    ('s2d', 'convT', 128, 64, 6, 180, 128, 'dgrad', 4),       # 45 strips
]
S2U_CASES = [
    ('s2u', 'convT', 128, 64, 1, 256, 256, 'fwd', 4),
    ('s2u', 'convT', 128, 64, 2, 256, 256, 'fwd', 8),
    ('s2u', 'convT', 128, 64, 4, 256, 256, 'fwd', 16),
    ('s2u', 'convT', 128, 64, 5, 240, 256, 'fwd', 20),
    ('s2u', 'convT', 128, 64, 8, 192, 256, 'fwd', 24),
    ('s2u', 'convT', 128, 64, 6, 180, 128, 'fwd', 9),
    ('s2u', 'convT', 128, 64, 7, 210, 128, 'fwd', 10),
    ('s2u', 'convT', 128, 64, 1, 512, 512, 'fwd', 16),        # eight row segments
    ('s2u', 'convT', 128, 64, 2, 7, 192, 'fwd', 1),           # odd height
    ('s2u', 'convT', 128, 64, 1, 2, 64, 'fwd', 1),
    ('s2u', 'convT', 128, 64, 1, 1, 64, 'fwd', 1),            # one strip = the whole image (a single input row: both neighbours are padding)
    ('s2u', 'convT', 128, 128, 3, 128, 128, 'fwd', 4),        # two channel tiles
    ('s2u', 'conv', 64, 128, 1, 512, 512, 'dgrad', 4),        # data gradient of down1
    ('s2u', 'conv', 64, 128, 2, 512, 512, 'dgrad', 8),
    ('s2u', 'conv', 64, 128, 4, 512, 512, 'dgrad', 16),
    ('s2u', 'conv', 64, 128, 7, 420, 256, 'dgrad', 10),
]
D1_CASES = [
    ('d1', 'conv', 6, 64, 1, 512, 512, 'fwd', 2),
    ('d1', 'conv', 6, 64, 4, 512, 512, 'fwd', 2),
    ('d1', 'conv', 6, 64, 16, 512, 512, 'fwd', 8),            # the benched discriminator update: fake + real batch
    ('d1', 'conv', 6, 64, 12, 384, 512, 'fwd', 4),
    ('d1', 'conv', 6, 64, 24, 360, 512, 'fwd', 6),
    ('d1', 'conv', 6, 64, 32, 512, 512, 'fwd', 16),
    ('d1', 'conv', 6, 64, 3, 4, 512, 'fwd', 2),               # one strip
]
D1G_CASES = [
    ('d1g', 'conv', 6, 64, 1, 512, 512, 'dgrad', 1),          # 256 strips of one row
    ('d1g', 'conv', 6, 64, 2, 512, 512, 'dgrad', 2),
    ('d1g', 'conv', 6, 64, 4, 512, 512, 'dgrad', 4),
    ('d1g', 'conv', 6, 64, 16, 512, 512, 'dgrad', 16),        # the benched discriminator update
    ('d1g', 'conv', 6, 64, 5, 480, 512, 'dgrad', 5),
    ('d1g', 'conv', 6, 64, 7, 420, 256, 'dgrad', 3),
    ('d1g', 'conv', 6, 64, 8, 384, 512, 'dgrad', 6),
    ('d1g', 'conv', 6, 64, 3, 1024, 1024, 'dgrad', 8),
    ('d1g', 'conv', 6, 64, 1, 2, 256, 'dgrad', 1),
]
DOT_SHAPES = [(16, 31, 31), (1, 31, 31), (5, 30, 33), (3, 63, 63), (1, 4, 4)]       # 16 x 31 x 31: the benched discriminator update
DOT_CASES = [(k, 'conv', 512, 1, n, h, w, d, None) for (n, h, w) in DOT_SHAPES for k, d in (('dotf', 'fwd'), ('dotg', 'dgrad'))]
ALL_CASES = S2D_CASES + S2U_CASES + D1_CASES + D1G_CASES + DOT_CASES

# the strip heights the table has to keep exercising (conv_s2d at R = 16 and conv_s2u at R = 32 stay in tests/test_gpu_s2d.py)
R_WANTED = {'s2d': {2, 4, 6, 8, 10, 12}, 's2u': {1, 4, 8, 9, 10, 16, 20, 24}, 'd1': {2, 4, 6, 8, 16}, 'd1g': {1, 2, 3, 4, 5, 6, 8, 16}}


def case_id(c):
    return f'{c[0]}-{c[1]}{c[2]}-{c[3]}n{c[4]}h{c[5]}w{c[6]}{c[7]}'


def spec_of(case):
    kernel, kind, cin, cout = case[:4]
    if kernel in ('s2d', 's2u'):
        return ConvSpec(kind, cin, cout, 3, 2, 1, L.PAD_ZERO, 1 if kind == 'convT' else 0)
    if kernel in ('d1', 'd1g'):
        return ConvSpec('conv', 6, 64, 4, 2, 1, L.PAD_ZERO, 0)
    return ConvSpec('conv', 512, 1, 4, 1, 1, L.PAD_ZERO, 0)


def geometry(case):
    """shapes of one launch, as ops.HipBackend.conv_forward sees them: (plan, n, hi, wi, ci_pad, ho, wo, co_pad, hq, wq)"""
    _, kind, _, _, n, H, W_, direction, _ = case
    spec = spec_of(case)
    oh, ow = spec.out_hw(H, W_)
    if direction == 'fwd':
        hq, wq = (oh, ow) if kind == 'conv' else (H, W_)
        return spec.forward_plan(), n, H, W_, cpad(spec.cin), oh, ow, cpad(spec.cout), hq, wq
    hq, wq = ((H + 1) // 2, (W_ + 1) // 2) if (kind == 'conv' and spec.stride == 2) else (H, W_)
    return spec.dgrad_plan(), n, oh, ow, cpad(spec.cout), H, W_, cpad(spec.cin), hq, wq


def descriptor(case, act=L.ACT_NONE, bias_n=None, splitk=1, in_pstride=None, out_pstride=None, in_act=L.ACT_NONE):
    plan, n, hi, wi, cip, ho, wo, cop, hq, wq = geometry(case)
    if bias_n is None:
        bias_n = spec_of(case).cout if case[7] == 'fwd' else 0
    return fill_conv_desc(plan, n, hi, wi, in_pstride or cip, ho, wo, cop, out_pstride or cop, hq, wq, L.DL_BF16, L.PREC_BF16, act, in_act, bias_n, splitk)


def strip_grid(case):
    """(n, rows, width, co) of the kernel's row grid: what conv_ref.strip_rows takes"""
    kernel = case[0]
    _, n, hi, wi, cip, ho, wo, cop, hq, wq = geometry(case)
    if kernel in ('s2d', 'd1'):
        return n, ho, wo, cop
    return n, hq, wq, cop


def strips(case):
    return conv_ref.strip_rows(case[0], *strip_grid(case))


def kernel_name(lib, d):
    return lib.dl_conv_kernel_name(C.byref(d)).decode()


def check_coverage():
    """the table's own strip heights: as listed, a superset of R_WANTED, and for every strip kernel one case of a single strip and one of >= 64 strips"""
    seen = {k: set() for k in R_WANTED}
    nstrips = {k: set() for k in R_WANTED}
    for c in ALL_CASES:
        if c[0] not in R_WANTED:
            continue
        R, ns, _ = strips(c)
        assert R == c[8], f'{case_id(c)}: the strip rule gives R = {R}, the table says {c[8]} -- a *_strip_rows rule changed: choose the shapes again'
        seen[c[0]].add(R)
        nstrips[c[0]].add(ns)
    for k, want in R_WANTED.items():
        assert seen[k] >= want, f'{k}: strip heights {sorted(want - seen[k])} are no longer exercised (table covers {sorted(seen[k])})'
        assert 1 in nstrips[k] and max(nstrips[k]) >= 64, f'{k}: strips per image {sorted(nstrips[k])} lack the one-strip or the >= 64-strip case'
