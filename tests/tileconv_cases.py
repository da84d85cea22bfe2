"""The rows of the tile-family convolution kernels -- the 18 routes of conv_route() (csrc/conv_gemm.hip) that are not weights-in-registers kernels -- that
tests/test_gpu_tileconv.py runs on the GPU and tests/test_tileconv_cases_host.py checks against the dispatch on the host -- TEST INFRASTRUCTURE ONLY.

A row is (layer: kind cin cout k stride pad pad_mode out_pad; N x H x W of the LAYER INPUT; direction; policy; act in_act bias splitk; an optional runtime
switch 'NAME=value'; the kernel conv_route() takes for it).  The policies are the four of tests/conv_routing_cases.py.  The shapes are the smallest that still
reach each route and each geometry edge (ragged last tiles, tiles that straddle two images, one-step K loops, zero-padded contracted channels, four-phase plans
at odd sizes, split-K slabs, in-kernel reflect / replicate borders, the reversed kernel-column order of the w4 data gradient); check_coverage() asks the
library for every row's kernel and fails when a routing rule moves a row off its kernel or leaves a route without a forward (or data-gradient) row."""
import ctypes as C
from collections import namedtuple

import conv_routing_cases as CR
from deepliif_amd import _lib as L
from deepliif_amd.geometry import ConvSpec, fill_conv_desc

Row = namedtuple('Row', 'kind cin cout k stride pad pad_mode out_pad n H W direction policy act in_act bias splitk switch kernel')
POLICY = {label: (dtype, prec, in_split) for label, dtype, prec, in_split in CR.POLICIES}
Z, RF, RP = L.PAD_ZERO, L.PAD_REFLECT, L.PAD_REPLICATE
NONE, RELU, LRELU, TANH = L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU, L.ACT_TANH

G16 = 'conv_gemm_glds_kernel<256,16,32>'
G64 = 'conv_gemm_glds_kernel<128,64,64>'
G128 = 'conv_gemm_glds_kernel<128,128,64>'
G256 = 'conv_gemm_glds_kernel<256,256,64>'
PH8 = 'conv_gemm_8ph_kernel'
W4 = 'conv_gemm_w4_kernel'
GB, GF = 'conv_gemm_kernel<bf16>', 'conv_gemm_kernel<f32>'
S2F, S2FX = 'conv_s2f_kernel', 'conv_s2f_x3_kernel'
C4, C4X = 'conv_c4_patch_kernel', 'conv_c4_patch_x3_kernel'
X16, X32 = 'conv_gemm_glds_x3_kernel<256,16>', 'conv_gemm_glds_x3_kernel<256,32>'
X64, X128 = 'conv_gemm_glds_x3_kernel<128,64>', 'conv_gemm_glds_x3_kernel<128,128>'
PH8X, W4X = 'conv_gemm_8ph_x3_kernel', 'conv_gemm_w4x3_kernel'
# every route of the tile family; the ones that serve data gradients somewhere in the networks (conv_gemm_kernel<bf16> takes the layers behind an input
# activation, which a data gradient never has; <256,32> is the head's stacked forward form; the w4x3 kernel is opt-in and its data gradient stays in
# tests/test_gpu_kernels.py test_strict_w4_kernel_on_split_copies)
ROUTES = (G16, G64, G128, G256, PH8, W4, GB, GF, S2F, S2FX, C4, C4X, X16, X32, X64, X128, PH8X, W4X)
DGRAD_ROUTES = (G16, G64, G128, G256, PH8, W4, GF, S2F, S2FX, C4, C4X, X16, X64, X128, PH8X)


def conv(cin, cout, k, s, p, shape, kernel, direction='fwd', policy='bf16', pm=Z, act=NONE, in_act=NONE, bias=None, splitk=1, switch=None):
    n, H, W_ = shape
    return Row('conv', cin, cout, k, s, p, pm, 0, n, H, W_, direction, policy, act, in_act, (direction == 'fwd') if bias is None else bias, splitk, switch, kernel)


def convT(cin, cout, k, p, op, shape, kernel, direction='fwd', policy='bf16', act=NONE, in_act=NONE, bias=None, splitk=1, switch=None):
    n, H, W_ = shape
    return Row('convT', cin, cout, k, 2, p, Z, op, n, H, W_, direction, policy, act, in_act, (direction == 'fwd') if bias is None else bias, splitk, switch, kernel)


S2F_ANY = 'DL_CONV_S2F=2'          # lifts conv_s2f's size rule (>= 65 536 phase-grid pixels), "for tests" (csrc/conv_s2f.hip s2f_eligible)
# conv_c4_patch's launcher (csrc/conv_c4.h c4_launch) caps the grid at 512 / (Co / 64) persistent workgroups per channel tile; 3 x 36 x 1216 is 3 x 9 x 19 = 513
# tiles of 4 x 64 pixels for Co = 64: workgroup 0 takes a second tile (the last one, of the third image)
C4_CAPPED = (3, 36, 1216)

BF16_ROWS = [
    # ---- conv_gemm_glds_kernel<256,16,32>: Co <= 16
    conv(64, 3, 7, 1, 3, (1, 8, 24), G16),                            # the head; the padding channels 3..7 must stay exactly zero
    conv(64, 3, 7, 1, 3, (1, 8, 24), G16, pm=RF, act=TANH),
    convT(128, 3, 4, 1, 0, (1, 6, 10), G16),                          # UNet last up: four phases
    conv(3, 64, 7, 1, 3, (1, 10, 20), G16, 'dgrad'),
    conv(9, 64, 4, 2, 1, (2, 12, 20), G16, 'dgrad'),                  # PatchGAN c1: four phases
    # ---- <128,64,64>: Co <= 64
    conv(3, 64, 7, 1, 3, (1, 10, 20), G64),                           # the stem at a width that is no multiple of 64: conv_c4_patch declines
    conv(3, 64, 7, 1, 3, (1, 10, 20), G64, pm=RF),
    conv(64, 64, 3, 1, 1, (2, 9, 15), G64, act=RELU),
    conv(64, 64, 3, 1, 1, (2, 9, 15), G64, 'dgrad'),
    conv(9, 64, 4, 2, 1, (2, 12, 20), G64, act=LRELU),
    conv(64, 128, 3, 2, 1, (2, 18, 22), G64, 'dgrad'),                # down1: four phases
    conv(64, 128, 3, 2, 1, (2, 25, 19), G64, 'dgrad'),                # odd sizes: ragged phases
    # ---- <128,128,64>
    conv(64, 128, 3, 2, 1, (2, 18, 22), G128),
    conv(256, 256, 3, 1, 1, (2, 12, 20), G128),                       # 480 pixels = 3.75 tiles: a masked last tile, one tile straddles both images
    conv(256, 256, 3, 1, 1, (2, 12, 20), G128, 'dgrad'),
    conv(128, 128, 3, 1, 1, (2, 12, 20), G128, pm=RF),
    conv(128, 128, 3, 1, 1, (2, 12, 20), G128, 'dgrad', pm=RF),       # the pad-0 plan over the padded extent 14 x 22 (a fold follows in the engine)
    convT(256, 128, 3, 1, 1, (2, 6, 10), G128),
    conv(192, 256, 3, 1, 1, (1, 12, 20), G128),                       # contracted channels padded 192 -> 256 with zeros
    conv(128, 256, 4, 2, 1, (1, 5, 5), G128, splitk=3),
    conv(128, 256, 4, 2, 1, (1, 5, 5), G128, 'dgrad', splitk=3),
    conv(512, 512, 4, 2, 1, (8, 2, 2), G128, splitk=4),
    # ---- conv_gemm_8ph_kernel: Co a multiple of 256, >= 224 workgroups, Ci >= 64, zero padding
    conv(64, 512, 3, 1, 1, (7, 64, 64), PH8),                         # exactly 112 tiles x 2 channel tiles = 224: the edge of the rule
    conv(64, 512, 3, 1, 1, (5, 60, 100), PH8),                        # 117.2 tiles: ragged, tiles straddle images
    conv(64, 512, 1, 1, 0, (7, 64, 64), PH8),                         # a single K step
    conv(64, 512, 3, 1, 1, (1, 56, 128), PH8, splitk=4),              # slabs and the reduce
    convT(64, 512, 3, 1, 1, (1, 56, 128), PH8),                       # four phases x 28 tiles
    conv(512, 64, 3, 1, 1, (7, 64, 64), PH8, 'dgrad'),
    # ---- <256,256,64>: the big tile without scalar tap decode
    conv(64, 512, 3, 1, 1, (2, 112, 128), G256, pm=RF),               # the reference's default ResnetBlock border at the tile rule's edge
    conv(32, 512, 3, 1, 1, (7, 64, 64), G256),                        # Ci < 64
    conv(512, 32, 3, 1, 1, (7, 64, 64), G256, 'dgrad'),
    # ---- conv_gemm_w4_kernel
    conv(64, 512, 3, 1, 1, (2, 112, 128), W4),
    conv(512, 64, 3, 1, 1, (2, 112, 128), W4, 'dgrad'),               # the reversed kernel-column order, which the replicate tests never reach
    # ---- conv_gemm_kernel<bf16>: the UNet layers, whose input activation is staged
    conv(64, 128, 4, 2, 1, (2, 12, 20), GB, in_act=LRELU),
    convT(256, 64, 4, 1, 0, (2, 6, 10), GB, in_act=RELU),
    convT(128, 3, 4, 1, 0, (1, 6, 10), GB, in_act=RELU, act=TANH),
    # ---- conv_s2f_kernel
    convT(64, 64, 3, 1, 1, (1, 256, 256), S2F),                       # exactly the 65 536-pixel size rule
    conv(64, 64, 4, 2, 1, (1, 512, 512), S2F, 'dgrad'),
    convT(64, 64, 3, 1, 1, (1, 20, 24), S2F, switch=S2F_ANY, act=RELU),      # 480 phase-grid pixels: 1.875 tiles
    conv(64, 64, 4, 2, 1, (2, 36, 40), S2F, 'dgrad', switch=S2F_ANY),        # 2 x 18 x 20 = 2.8 tiles, one straddles the images
    # (an odd-sized data gradient, 2 x 25 x 19, stays off the kernel under the switch too: s2f_eligible wants Ho == 2 Hq -- asserted in check_coverage)
    # ---- conv_c4_patch_kernel
    conv(3, 64, 7, 1, 3, (1, 8, 64), C4),
    conv(3, 64, 7, 1, 3, (1, 8, 64), C4, pm=RF),
    conv(3, 64, 7, 1, 3, (1, 8, 64), C4, pm=RP),
    conv(64, 3, 7, 1, 3, (1, 8, 64), C4, 'dgrad'),                    # the head's data gradient
    conv(3, 64, 7, 1, 3, C4_CAPPED, C4),
]

STRICT_ROWS = [
    conv(64, 3, 7, 1, 3, (1, 8, 24), X16, policy='strict'),
    conv(64, 3, 7, 1, 3, (1, 8, 24), X16, policy='strict', pm=RF, act=TANH),
    convT(128, 3, 4, 1, 0, (1, 6, 10), X16, policy='strict'),
    conv(9, 64, 4, 2, 1, (2, 12, 20), X16, 'dgrad', policy='strict'),
    conv(64, 32, 3, 1, 1, (2, 9, 15), X32, policy='strict'),
    conv(3, 64, 7, 1, 3, (1, 10, 20), X64, policy='strict', pm=RF),
    conv(64, 64, 3, 1, 1, (2, 9, 15), X64, policy='strict'),
    conv(64, 64, 3, 1, 1, (2, 9, 15), X64, 'dgrad', policy='strict'),
    conv(64, 128, 3, 2, 1, (2, 25, 19), X64, 'dgrad', policy='strict'),
    conv(64, 128, 3, 2, 1, (2, 18, 22), X128, policy='strict'),
    conv(256, 256, 3, 1, 1, (2, 12, 20), X128, policy='strict'),
    conv(256, 256, 3, 1, 1, (2, 12, 20), X128, 'dgrad', policy='strict'),
    conv(128, 128, 3, 1, 1, (2, 12, 20), X128, policy='strict', pm=RF),
    convT(256, 128, 3, 1, 1, (2, 6, 10), X128, policy='strict'),
    conv(192, 256, 3, 1, 1, (1, 12, 20), X128, policy='strict'),
    conv(128, 256, 4, 2, 1, (1, 5, 5), X128, policy='strict', splitk=3),
    # the UNet rows: the activation instantiations of conv_gemm_glds_x3_kernel
    conv(64, 128, 4, 2, 1, (2, 12, 20), X128, policy='strict', in_act=LRELU),
    convT(256, 64, 4, 1, 0, (2, 6, 10), X64, policy='strict', in_act=RELU),
    convT(128, 3, 4, 1, 0, (1, 6, 10), X16, policy='strict', in_act=RELU, act=TANH),
    conv(64, 512, 3, 1, 1, (7, 64, 64), PH8X, policy='strict'),
    conv(64, 512, 1, 1, 0, (7, 64, 64), PH8X, policy='strict'),
    conv(32, 512, 3, 1, 1, (7, 64, 64), PH8X, policy='strict'),       # Ci < 64: the strict big tile takes it all the same
    conv(512, 64, 3, 1, 1, (7, 64, 64), PH8X, 'dgrad', policy='strict'),
    conv(64, 512, 3, 1, 1, (1, 56, 128), PH8X, policy='strict', splitk=4),
    conv(3, 64, 7, 1, 3, (1, 8, 64), C4X, policy='strict'),
    conv(64, 3, 7, 1, 3, (1, 8, 64), C4X, 'dgrad', policy='strict'),
]

SPLIT_ROWS = [
    convT(64, 64, 3, 1, 1, (1, 256, 256), S2FX, policy='strict+split'),
    conv(64, 64, 3, 2, 1, (1, 512, 512), S2FX, 'dgrad', policy='strict+split'),
    convT(64, 64, 3, 1, 1, (1, 20, 24), S2FX, policy='strict+split', switch=S2F_ANY),
    conv(64, 64, 4, 2, 1, (2, 36, 40), S2FX, 'dgrad', policy='strict+split', switch=S2F_ANY),
    conv(64, 512, 3, 1, 1, (2, 112, 128), W4X, policy='strict+split', switch='DL_CONV_W4X3=1'),
]

F32B_ROWS = [
    conv(64, 64, 3, 1, 1, (2, 9, 15), GF, policy='fp32+bf16'),
    conv(64, 128, 3, 2, 1, (2, 25, 19), GF, 'dgrad', policy='fp32+bf16'),
    convT(128, 3, 4, 1, 0, (1, 6, 10), GF, policy='fp32+bf16', in_act=RELU, act=TANH),
]

ALL_ROWS = BF16_ROWS + STRICT_ROWS + SPLIT_ROWS + F32B_ROWS
# the IEEE-half library (the inference policy) runs the forward rows of the 16-bit policy again
F16_ROWS = [r for r in BF16_ROWS if r.direction == 'fwd']
# channel-slice views (in_pstride / out_pstride twice the channel count): one row each of three kernels the UNet's concat buffers reach
SLICE_ROWS = [
    conv(256, 256, 3, 1, 1, (2, 12, 20), G128),
    conv(64, 128, 4, 2, 1, (2, 12, 20), GB, in_act=LRELU),
    conv(64, 64, 3, 1, 1, (2, 9, 15), X64, policy='strict'),
]
# fused statistics: act NONE, no split-K, whole tiles per image (dl_conv_stats_chunks > 0), at most 1024 values per (image, channel).  112 images of one
# 256-pixel tile each keep the 224-workgroup rule of the big tiles; conv_s2f's smallest whole tile is 256 phase-grid pixels = 1024 output values
STATS_ROWS = [
    conv(128, 128, 3, 1, 1, (2, 8, 16), G128),
    conv(64, 512, 3, 1, 1, (112, 16, 16), PH8),
    conv(32, 512, 3, 1, 1, (112, 16, 16), G256),
    convT(64, 64, 3, 1, 1, (2, 16, 16), S2F, switch=S2F_ANY),
    conv(3, 64, 7, 1, 3, (1, 8, 64), C4),
    conv(64, 512, 3, 1, 1, (112, 16, 16), PH8X, policy='strict'),
    convT(64, 64, 3, 1, 1, (2, 16, 16), S2FX, policy='strict+split', switch=S2F_ANY),
]
# rows that must stay OFF a kernel: (row, the kernel it must not take)
DECLINED = [(conv(64, 64, 4, 2, 1, (2, 25, 19), G64, 'dgrad', switch=S2F_ANY), S2F)]

_PM = {Z: 'z', RF: 'rf', RP: 'rp'}


def case_id(r):
    tail = ''.join([f'-a{r.act}' if r.act else '', f'-ia{r.in_act}' if r.in_act else '', f'-sk{r.splitk}' if r.splitk > 1 else '',
                    f'-{r.switch}' if r.switch else ''])
    return f'{r.policy}-{r.kind}{r.cin}-{r.cout}k{r.k}s{r.stride}{_PM[r.pad_mode]}-n{r.n}h{r.H}w{r.W}-{r.direction}{tail}'


def spec_of(r):
    return ConvSpec(r.kind, r.cin, r.cout, r.k, r.stride, r.pad, r.pad_mode, r.out_pad)


def geometry(r):
    """shapes of one launch, as ops.HipBackend.conv_forward sees them: (plan, n, hi, wi, ci_pad, ho, wo, co_pad, hq, wq).  The data gradient of a reflect- or
    replicate-padded layer runs over the explicitly padded extent (conv_routing_cases._geometry)."""
    plan, hi, wi, cip, ho, wo, cop, hq, wq = CR._geometry(spec_of(r), False, r.direction, r.n, r.H, r.W)
    return plan, r.n, hi, wi, cip, ho, wo, cop, hq, wq


def descriptor(r, in_pstride=None, out_pstride=None):
    plan, n, hi, wi, cip, ho, wo, cop, hq, wq = geometry(r)
    dtype, prec, in_split = POLICY[r.policy]
    d = fill_conv_desc(plan, n, hi, wi, in_pstride or cip, ho, wo, cop, out_pstride or cop, hq, wq, dtype, prec, r.act, r.in_act,
                       plan.rows_real if r.bias else 0, r.splitk)
    d.in_split = in_split
    return d


class switched:
    """with switched(lib, row): the library sees the row's runtime switch (if it has one) and forgets it afterwards"""

    def __init__(self, lib, r):
        self.cm = CR.switch_setting(lib, r.switch) if r.switch else None

    def __enter__(self):
        if self.cm:
            self.cm.__enter__()

    def __exit__(self, *exc):
        if self.cm:
            self.cm.__exit__(*exc)


def kernel_name(lib, r, **kw):
    with switched(lib, r):
        return lib.dl_conv_kernel_name(C.byref(descriptor(r, **kw))).decode()


def check_coverage(lib=None):
    """every row takes the kernel its last field names; every route of the tile family has a forward row, and a data-gradient row where it serves data
    gradients; the rows listed as declined stay off the kernel they name.  Host side of the library only: no GPU."""
    lib = lib or L.load()
    fwd, dgrad = set(), set()
    for r in ALL_ROWS:
        got = kernel_name(lib, r)
        assert got == r.kernel, f'{case_id(r)}: conv_route() takes {got}, the table says {r.kernel} -- a routing rule changed: choose the shape again'
        (fwd if r.direction == 'fwd' else dgrad).add(got)
    assert len(ROUTES) == 18 and len(set(ROUTES)) == 18
    assert fwd >= set(ROUTES), f'no forward row reaches {sorted(set(ROUTES) - fwd)}'
    assert dgrad >= set(DGRAD_ROUTES), f'no data-gradient row reaches {sorted(set(DGRAD_ROUTES) - dgrad)}'
    assert (fwd | dgrad) == set(ROUTES), f'rows on kernels outside the tile family: {sorted((fwd | dgrad) - set(ROUTES))}'
    for r, never in DECLINED:
        got = kernel_name(lib, r)
        assert got != never and got == r.kernel, f'{case_id(r)}: expected to stay off {never} and on {r.kernel}, got {got}'
    ids = [case_id(r) for r in ALL_ROWS]
    assert len(set(ids)) == len(ids), 'two rows share an id'
    for r in STATS_ROWS:
        assert kernel_name(lib, r) == r.kernel, f'{case_id(r)}: conv_route() takes {kernel_name(lib, r)}, the statistics table says {r.kernel}'
        with switched(lib, r):
            assert lib.dl_conv_stats_chunks(C.byref(descriptor(r))) > 0, f'{case_id(r)}: no fused statistics for this row'
    for r in SLICE_ROWS:
        _, _, _, _, cip, _, _, cop, _, _ = geometry(r)
        got = kernel_name(lib, r, in_pstride=2 * cip, out_pstride=2 * cop)
        assert got == r.kernel and r in ALL_ROWS, f'{case_id(r)} as a channel slice: conv_route() takes {got}, the table says {r.kernel}'
    return sorted(fwd | dgrad)


def check_coverage_f16():
    """the IEEE-half library routes its rows as the bf16 library does (the same sources)"""
    lib = L.load('fp16')
    for r in F16_ROWS:
        got = kernel_name(lib, r)
        assert got == r.kernel, f'fp16 library, {case_id(r)}: conv_route() takes {got}, the table says {r.kernel}'
