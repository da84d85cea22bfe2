"""dl_conv_kernel_name / dl_conv_stats_chunks on the host (the library loads without a GPU; nothing here launches anything): the eligibility edges of the
six weights-in-registers kernels, the 32-bit offset guard of the four strip kernels on both tensors, and the strip heights of every shape of
the GPU sweep (tests/regconv_cases.py) against the library's own count of statistics chunks."""
import ctypes as C

import pytest

import regconv_cases as RC
from deepliif_amd import _lib as L

S2D, S2U, D1, D1G, DOTF, DOTG = (RC.KERNEL_NAME[k] for k in ('s2d', 's2u', 'd1', 'd1g', 'dotf', 'dotg'))
G128, G64, G16, PLAIN = 'conv_gemm_glds_kernel<128,128,64>', 'conv_gemm_glds_kernel<128,64,64>', 'conv_gemm_glds_kernel<256,16,32>', 'conv_gemm_kernel<bf16>'


def _reflect(d):
    d.pad_mode = L.PAD_REFLECT


def c(kernel, n, h, w, kind=None, cin=None, cout=None, direction=None):
    base = {'s2d': ('conv', 64, 128, 'fwd'), 's2u': ('convT', 128, 64, 'fwd'), 'd1': ('conv', 6, 64, 'fwd'), 'd1g': ('conv', 6, 64, 'dgrad'),
            'dotf': ('conv', 512, 1, 'fwd'), 'dotg': ('conv', 512, 1, 'dgrad')}[kernel]
    return (kernel, kind or base[0], cin or base[1], cout or base[2], n, h, w, direction or base[3], None)


# label, case, descriptor() keywords, expected kernel
EDGES = [
    # conv_s2d: 64 -> 128k channels, output rows of 128 k pixels, even output height, no split-K, none / ReLU only
    ('s2d', c('s2d', 2, 64, 256), {}, S2D),
    ('s2d relu', c('s2d', 2, 64, 256), {'act': L.ACT_RELU}, S2D),
    ('s2d no bias', c('s2d', 2, 64, 256), {'bias_n': 0}, S2D),
    ('s2d 192 -> 256 padded channels', c('s2d', 2, 64, 256, cout=192), {}, S2D),
    ('s2d output width 160', c('s2d', 2, 64, 320), {}, G128),
    ('s2d odd output height', c('s2d', 2, 66, 256), {}, G128),
    ('s2d odd input height', c('s2d', 2, 65, 256), {}, G128),
    ('s2d 64 output channels', c('s2d', 2, 64, 256, cout=64), {}, G64),
    ('s2d split-K', c('s2d', 2, 64, 256), {'splitk': 2}, G128),
    ('s2d input activation', c('s2d', 2, 64, 256), {'in_act': L.ACT_LRELU}, PLAIN),
    ('s2d tanh', c('s2d', 2, 64, 256), {'act': L.ACT_TANH}, G128),
    ('s2d leaky relu', c('s2d', 2, 64, 256), {'act': L.ACT_LRELU}, G128),
    ('s2d reflect', c('s2d', 2, 64, 256), {'mod': _reflect}, G128),
    ('s2d data gradient of up2', c('s2d', 2, 32, 128, 'convT', 128, 64, 'dgrad'), {}, S2D),
    # conv_s2u: 128 -> 64k channels, phase-grid rows of 64 k pixels
    ('s2u', c('s2u', 2, 16, 64), {}, S2U),
    ('s2u relu', c('s2u', 2, 16, 64), {'act': L.ACT_RELU}, S2U),
    ('s2u odd height', c('s2u', 2, 7, 64), {}, S2U),
    ('s2u width 96', c('s2u', 2, 16, 96), {}, G64),
    ('s2u 32 output channels', c('s2u', 2, 16, 64, cout=32), {}, G64),
    ('s2u split-K', c('s2u', 2, 16, 64), {'splitk': 2}, G64),
    ('s2u input activation', c('s2u', 2, 16, 64), {'in_act': L.ACT_RELU}, PLAIN),
    ('s2u tanh', c('s2u', 2, 16, 64), {'act': L.ACT_TANH}, G64),
    ('s2u data gradient of down1', c('s2u', 2, 32, 128, 'conv', 64, 128, 'dgrad'), {}, S2U),
    ('s2u data gradient, odd layer input', c('s2u', 2, 31, 128, 'conv', 64, 128, 'dgrad'), {}, G64),
    # conv_d1: 6 (8) -> 64 channels, k4 s2, output rows of exactly 256 pixels, even output height; none / ReLU / LeakyReLU
    ('d1', c('d1', 2, 8, 512), {'act': L.ACT_LRELU}, D1),
    ('d1 no activation, no bias', c('d1', 2, 8, 512), {'bias_n': 0}, D1),
    ('d1 output width 128', c('d1', 2, 8, 256), {}, G64),
    ('d1 output width 512', c('d1', 2, 8, 1024), {}, G64),
    ('d1 odd output height', c('d1', 2, 6, 512), {}, G64),
    ('d1 split-K', c('d1', 2, 8, 512), {'splitk': 2}, G64),
    ('d1 input activation', c('d1', 2, 8, 512), {'in_act': L.ACT_LRELU}, PLAIN),
    ('d1 tanh', c('d1', 2, 8, 512), {'act': L.ACT_TANH}, G64),
    # conv_d1g: its data gradient; phase-grid rows of 128 k pixels; no bias, no activation
    ('d1g', c('d1g', 2, 8, 256), {}, D1G),
    ('d1g bias', c('d1g', 2, 8, 256), {'bias_n': 6}, G16),
    ('d1g phase-grid width 64', c('d1g', 2, 8, 128), {}, G16),
    ('d1g split-K', c('d1g', 2, 8, 256), {'splitk': 2}, G16),
    ('d1g relu', c('d1g', 2, 8, 256), {'act': L.ACT_RELU}, G16),
    ('d1g input activation', c('d1g', 2, 8, 256), {'in_act': L.ACT_LRELU}, PLAIN),
    ('d1g odd layer input', c('d1g', 2, 7, 256), {}, G16),
    # conv_dot: whatever split-K the host asks for (nothing to reduce)
    ('dot fwd', c('dotf', 2, 8, 8), {}, DOTF),
    ('dot fwd split-K', c('dotf', 2, 8, 8), {'splitk': 3}, DOTF),
    ('dot fwd without bias', c('dotf', 2, 8, 8), {'bias_n': 0}, G16),
    ('dot fwd input activation', c('dotf', 2, 8, 8), {'in_act': L.ACT_LRELU}, PLAIN),
    ('dot fwd tanh', c('dotf', 2, 8, 8), {'act': L.ACT_TANH}, G16),
    ('dot dgrad', c('dotg', 2, 8, 8), {}, DOTG),
    ('dot dgrad split-K', c('dotg', 2, 8, 8), {'splitk': 3}, DOTG),
    ('dot dgrad with a bias', c('dotg', 2, 8, 8), {'bias_n': 1}, G128),
    ('dot dgrad relu', c('dotg', 2, 8, 8), {'act': L.ACT_RELU}, G128),
]


def _name(case, kw):
    kw = dict(kw)
    mod = kw.pop('mod', None)
    d = RC.descriptor(case, **kw)
    if mod:
        mod(d)
    return RC.kernel_name(L.load(), d)


@pytest.mark.parametrize('edge', EDGES, ids=lambda e: e[0].replace(' ', '_'))
def test_eligibility_edges(edge):
    label, case, kw, want = edge
    assert _name(case, kw) == want, label


# ---- the 32-bit edge.  The strip kernels address one image through a buffer resource with 32-bit offsets (r * (int)row_bytes, lane offsets): an image of
# 2^31 bytes or more, input or output, must go to a kernel with 64-bit addressing.  Where they land today: the gather GEMMs (conv_gemm_glds_kernel,
# conv_gemm_8ph_kernel) and, for the conv_s2u shapes, the fused four-phase kernel conv_s2f_kernel -- all three build per-lane 64-bit pointers from size_t
# pixel offsets (csrc/conv_gemm.hip, csrc/conv_s2f.hip: x_ptr / opix).
ADDR64 = ('conv_gemm_glds_kernel', 'conv_gemm_8ph_kernel', 'conv_s2f_kernel')
# Rows: kernel, side, how, case just under 2^31, its (in_pstride, out_pstride), case at 2^31, its (in_pstride, out_pstride).  "Just under" is the nearest
# size the kernel's geometry admits (one row, or one row pair / segment where heights must be even or widths multiples of 128), or one 16-byte step of the
# pixel stride.
EDGE32 = [
    ('s2d', 'in', 'size', c('s2d', 1, 2048, 7936), (None, None), c('s2d', 1, 2048, 8192), (None, None)),
    ('s2d', 'in', 'pstride', c('s2d', 1, 2048, 2048), (248, None), c('s2d', 1, 2048, 2048), (256, None)),
    ('s2d', 'out', 'size', c('s2d', 1, 2048, 3840, cout=512), (None, None), c('s2d', 1, 2048, 4096, cout=512), (None, None)),
    ('s2d', 'out', 'pstride', c('s2d', 1, 2048, 2048), (None, 1016), c('s2d', 1, 2048, 2048), (None, 1024)),
    ('s2u', 'in', 'size', c('s2u', 1, 1023, 2048), (512, None), c('s2u', 1, 1024, 2048), (512, None)),
    ('s2u', 'in', 'pstride', c('s2u', 1, 1024, 1024), (1016, None), c('s2u', 1, 1024, 1024), (1024, None)),
    ('s2u', 'out', 'size', c('s2u', 1, 2047, 2048), (None, None), c('s2u', 1, 2048, 2048), (None, None)),
    ('s2u', 'out', 'pstride', c('s2u', 1, 1024, 1024), (None, 248), c('s2u', 1, 1024, 1024), (None, 256)),
    ('d1', 'in', 'size', c('d1', 1, 65532, 512), (32, None), c('d1', 1, 65536, 512), (32, None)),
    ('d1', 'in', 'pstride', c('d1', 1, 8192, 512), (248, None), c('d1', 1, 8192, 512), (256, None)),
    ('d1', 'out', 'size', c('d1', 1, 131068, 512), (None, None), c('d1', 1, 131072, 512), (None, None)),
    ('d1', 'out', 'pstride', c('d1', 1, 65536, 512), (None, 120), c('d1', 1, 65536, 512), (None, 128)),
    ('d1g', 'in', 'size', c('d1g', 1, 8190, 8192), (None, None), c('d1g', 1, 8192, 8192), (None, None)),
    ('d1g', 'in', 'pstride', c('d1g', 1, 4096, 4096), (248, None), c('d1g', 1, 4096, 4096), (256, None)),
    ('d1g', 'out', 'size', c('d1g', 1, 4094, 8192), (None, 32), c('d1g', 1, 4096, 8192), (None, 32)),
    ('d1g', 'out', 'pstride', c('d1g', 1, 2048, 2048), (None, 248), c('d1g', 1, 2048, 2048), (None, 256)),
]


def _image_bytes(d):
    return d.Hi * d.Wi * d.in_pstride * 2, d.Ho * d.Wo * d.out_pstride * 2


@pytest.mark.parametrize('row', EDGE32, ids=lambda r: f'{r[0]}-{r[1]}-{r[2]}')
def test_images_of_2_to_the_31_bytes_leave_the_strip_kernels(row):
    kernel, side, how, under, ps_u, at, ps_a = row
    lib = L.load()
    fast = RC.KERNEL_NAME[kernel]
    which = 0 if side == 'in' else 1
    du = RC.descriptor(under, in_pstride=ps_u[0], out_pstride=ps_u[1])
    da = RC.descriptor(at, in_pstride=ps_a[0], out_pstride=ps_a[1])
    bu, ba = _image_bytes(du), _image_bytes(da)
    # the table itself: the tested tensor sits just under / exactly at 2^31 bytes per image, the other one stays well inside
    assert bu[which] < 2 ** 31 and bu[which] >= 2 ** 31 - 2 ** 31 // 16 and ba[which] == 2 ** 31, (bu, ba)
    assert bu[1 - which] <= 2 ** 30 and ba[1 - which] <= 2 ** 30, (bu, ba)
    assert RC.kernel_name(lib, du) == fast, f'{kernel}: {bu[which]} bytes per {side}put image is inside the 32-bit range'
    got = RC.kernel_name(lib, da)
    assert got != fast and got.split('<')[0] in ADDR64, f'{kernel}: a {side}put image of 2^31 bytes must go to a kernel with 64-bit addressing, got {got}'


# ---- the sweep's shapes
def test_the_sweep_keeps_its_strip_heights():
    RC.check_coverage()


@pytest.mark.parametrize('case', RC.ALL_CASES, ids=RC.case_id)
def test_sweep_cases_route_to_their_kernel_and_strip_counts_match_the_library(case):
    lib = L.load()
    kernel = case[0]
    for act in (L.ACT_NONE, L.ACT_RELU) if kernel in ('s2d', 's2u') else ((L.ACT_NONE, L.ACT_LRELU) if kernel in ('d1', 'dotf') else (L.ACT_NONE,)):
        assert RC.kernel_name(lib, RC.descriptor(case, act=act)) == RC.KERNEL_NAME[kernel], (RC.case_id(case), act)
    if kernel in ('s2d', 's2u', 'd1') and case[7] == 'fwd':
        assert RC.kernel_name(lib, RC.descriptor(case, bias_n=0)) == RC.KERNEL_NAME[kernel]
    chunks = lib.dl_conv_stats_chunks(C.byref(RC.descriptor(case)))
    if kernel in ('s2d', 's2u'):
        R, nstrips, segs = RC.strips(case)
        assert R == case[8] and chunks == segs * nstrips, (RC.case_id(case), R, nstrips, segs, chunks)
    else:
        assert chunks == 0, 'no fused statistics on the PatchGAN kernels'


def test_the_routes_of_the_trace_child_reach_the_kernels_they_name(capsys):
    """tests/regconv_trace_child.py (the GPU test that holds dl_conv_kernel_name against a kernel trace): its table, checked here without launching"""
    import regconv_trace_child as T
    T.names_only()
    out = capsys.readouterr().out
    for k in RC.KERNEL_NAME.values():
        assert f' {k}\n' in out
    assert out.count('ROUTE ') == len(T.route_cases())
