"""GPU sweep of the six weights-in-registers convolution kernels (conv_s2d, conv_s2u, conv_d1, conv_d1g, conv_dot_fwd / dgrad) over the strip
heights their *_strip_rows rules pick at the batch sizes and image heights of real use, on both libraries (bf16 and, for the inference kernels, IEEE half).

Every case goes through ops.impl() / dl_conv_forward with splitk = 1, asserts by name that the dispatch took the kernel under test, and is compared element by
element with a float64 convolution under the derived bound of tests/conv_ref.py (u |ref| + K 2^-24 S + 2^-24; no element may be out of bound).  A failure
prints where the bad elements are (image, strip, row inside the strip, pixel / channel residues, accumulator position).  Shapes: tests/regconv_cases.py, whose
coverage guard fails when a strip rule changes under the table.  The worst err / bound of every case goes to parity_errors_regconv.json in the directory $DL_PARITY_DIR names
(default parity_out/); a copy of the MI355X run is kept as profiles/r06/parity_errors_regconv.json.

DL_TEST_DRYRUN=1 runs the file on the CPU with the formula emulation in the kernels' place (a check of the test code only)."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import conv_ref
import regconv_cases as RC
from deepliif_amd import _lib as L
from deepliif_amd import ops
from deepliif_amd.engine import Precision
from deepliif_amd.geometry import cpad

from test_gpu_kernels import DEV, DRY, _run_conv, hip, sync

pytestmark = pytest.mark.gpu
ERRLOG = {}
ERRLOG_DIR = os.environ.get('DL_PARITY_DIR', 'parity_out')
SUM_SLACK = 1            # multiplier of the summation term of the bound (conv_ref.bound); 1 = as derived
SMALL = 2 * 512 * 512    # pixels (of the larger of the layer's input and output) up to which every bias / activation variant runs; larger shapes run one
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _real_backend_again():
    yield
    ops._impl = None


@pytest.fixture(autouse=True, scope='module')
def _errlog():
    yield
    os.makedirs(ERRLOG_DIR, exist_ok=True)
    with open(os.path.join(ERRLOG_DIR, 'parity_errors_regconv.json'), 'w') as f:
        json.dump(ERRLOG, f, indent=1, sort_keys=True)


def _rnd(shape, seed, dtype, scale=1.0):
    """normal values exactly representable in the library's 16-bit format (packing / staging them is exact: the test sees the kernel's arithmetic only)"""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).float()


def _inputs(case, dtype):
    """(x, w, bias): the tensor the kernel reads (layer input, or dL/dy for a data gradient; padding channels zero), the layer's weight, its bias"""
    _, kind, _, _, n, H, W_, direction, _ = case
    spec = RC.spec_of(case)
    w = _rnd((spec.cout, spec.cin, spec.k, spec.k) if kind == 'conv' else (spec.cin, spec.cout, spec.k, spec.k), 1, dtype, 0.05)
    bias = torch.randn((spec.cout,), generator=torch.Generator().manual_seed(2)) * 0.1
    if direction == 'fwd':
        c, h, w_ = spec.cin, H, W_
    else:
        c = spec.cout
        h, w_ = spec.out_hw(H, W_)
    x = torch.zeros(n, h, w_, cpad(c))
    x[..., :c] = _rnd((n, h, w_, c), 3 if direction == 'fwd' else 4, dtype)
    return x.to(dtype), w, bias


def _variants(case):
    kernel, _, _, _, n, H, W_, direction, _ = case
    oh, ow = RC.spec_of(case).out_hw(H, W_)
    small = n * max(H * W_, oh * ow) <= SMALL
    if direction == 'dgrad':
        return [(L.ACT_NONE, False)]
    if kernel in ('s2d', 's2u'):
        return [(L.ACT_NONE, True), (L.ACT_RELU, True), (L.ACT_NONE, False)] if small else [(L.ACT_NONE, True)]
    if kernel == 'd1':
        return [(L.ACT_LRELU, True)] + ([(L.ACT_NONE, True), (L.ACT_LRELU, False)] if (n, H) in ((1, 512), (3, 4)) else [])
    return [(L.ACT_NONE, True), (L.ACT_LRELU, True)]          # conv_dot_fwd


def _geom(case):
    if case[8] is None:
        return None
    return {'kernel': case[0], 'R': case[8], 'row_div': 2 if case[0] in ('s2u', 'd1g') else 1}


def _sweep(case, half, twice=False):
    kernel, _, _, _, n, H, W_, direction, _ = case
    prec = Precision.get(half)
    spec = RC.spec_of(case)
    want = RC.KERNEL_NAME[kernel]
    x, w, bias = _inputs(case, prec.dtype)
    reference = conv_ref.Reference(spec, direction, x, w, in_hw=(H, W_))
    with ops.half_mode(half):
        real = hip()
        assert DRY or real.half == half
        lib = L.load(half)
        xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
        for act, with_bias in _variants(case):
            tag = f'{half}/{RC.case_id(case)}/act{act}{"" if with_bias else "-nobias"}'
            assert RC.kernel_name(lib, RC.descriptor(case, act=act, bias_n=None if with_bias else 0)) == want, tag
            got = _run_conv(real, direction, spec, prec, xd, wd, bd if with_bias else None, act, L.ACT_NONE, H, W_, splitk=1)
            assert DRY or real.last_conv_kernel == want, (tag, real.last_conv_kernel)
            sync()
            ref, S, K = reference.variant(bias if with_bias else None, act)
            bnd = conv_ref.bound(ref, S, K, prec.dtype, SUM_SLACK)
            del S
            worst, report = conv_ref.compare(got, ref, bnd, _geom(case))
            del ref, bnd
            ERRLOG[tag] = worst
            print(f'{tag}: worst err/bound {worst:.4f}')
            assert worst <= 1.0 and not report, f'{tag}\n{report}'
            c_real = spec.cout if direction == 'fwd' else spec.cin
            if cpad(c_real) > c_real:
                assert float(got[..., c_real:].float().abs().max()) == 0.0, f'{tag}: the padding channels must stay exactly zero'
            if twice:
                again = _run_conv(real, direction, spec, prec, xd, wd, bd if with_bias else None, act, L.ACT_NONE, H, W_, splitk=1)
                sync()
                assert torch.equal(got, again), f'{tag}: run-to-run difference'
                twice = False
            del got


# one mid-size case per kernel also checks that two launches give the same bits (the older files repeat their own cases three times)
TWICE = {('s2d', 7, 420, 256, 'fwd'), ('s2u', 6, 180, 128, 'fwd'), ('d1', 12, 384, 512, 'fwd'), ('d1g', 7, 420, 256, 'dgrad'), ('dotf', 5, 30, 33, 'fwd'),
         ('dotg', 5, 30, 33, 'dgrad')}


def _twice(c):
    return (c[0], c[4], c[5], c[6], c[7]) in TWICE


def test_the_table_covers_the_strip_heights():
    RC.check_coverage()
    assert sum(_twice(c) for c in RC.ALL_CASES) == len(TWICE)


@pytest.mark.parametrize('case', RC.ALL_CASES, ids=RC.case_id)
def test_bf16_library(case):
    _sweep(case, 'bf16', _twice(case))


@pytest.mark.parametrize('case', [c for c in RC.S2D_CASES + RC.S2U_CASES if c[7] == 'fwd'], ids=RC.case_id)
def test_f16_library(case):
    """the inference policy's library: the same sources, another register allocation (IEEE half operands); forward kernels of the generators only"""
    _sweep(case, 'fp16', _twice(case))


# ---- fused statistics
STATS_CASES = [
    # kernel, (N, H, W) of the layer input, scope; strip heights 2, 8, 6, 2 (three segments) / 4, 16, 9, 1
    ('s2d', (1, 512, 512), L.NORM_INSTANCE), ('s2d', (4, 512, 512), L.NORM_BATCH), ('s2d', (7, 420, 256), L.NORM_INSTANCE), ('s2d', (2, 12, 768), L.NORM_BATCH),
    ('s2u', (1, 256, 256), L.NORM_INSTANCE), ('s2u', (4, 256, 256), L.NORM_BATCH), ('s2u', (6, 180, 128), L.NORM_INSTANCE), ('s2u', (2, 7, 192), L.NORM_BATCH),
]


def _case_of(kernel, shape, direction='fwd'):
    hits = [c for c in RC.ALL_CASES if c[0] == kernel and c[4:7] == shape and c[7] == direction and c[3] in (64, 128) and c[2] != c[3]]
    assert len(hits) == 1, (kernel, shape, hits)
    return hits[0]


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
@pytest.mark.parametrize('sc', STATS_CASES, ids=lambda s: f'{s[0]}-n{s[1][0]}h{s[1][1]}w{s[1][2]}-{"batch" if s[2] == L.NORM_BATCH else "instance"}')
def test_fused_statistics_against_float64_statistics_of_the_stored_tensor(sc, half):
    """want_stats=True: the kernel leaves per-(image, channel) sum and sum of squares OF THE VALUES IT STORED, one chunk per workgroup (row segment x strip);
    dl_norm_forward(ext_nchunks) turns them into mean and rstd.  Checked against float64 statistics of the stored tensor.

    Bound.  A chunk covers P = R strip rows x one row segment of output pixels (s2d: 128 R; s2u: 64 R input = 256 R output pixels); at least 16 lanes share
    the pixels of a channel, each adds its P / 16 values serially in fp32, then 6 shuffle / LDS levels join lanes and waves, then the normalisation adds the
    nch chunks of an image (and the N images of a batch).  No value passes through more than
        Lsum = P / 16 + 6 + nch * (N for batch scope, 1 for instance scope)
    additions, so  |d sum| <= Lsum 2^-24 sum|y|,  |d sumsq| <= (Lsum + 1) 2^-24 sum y^2  (one more rounding for the square), whatever the order.  With
    mean = sum / n and var = sumsq / n - mean^2 computed in fp32 (a handful of roundings, relative to E y^2 + mean^2):
        |d mean| <= (Lsum + 2) 2^-24 E|y|
        |d var|  <= (Lsum + 6) 2^-24 (E y^2 + 2 |mean| E|y|)
        |d rstd| / rstd <= |d var| / (2 (var + eps)) + 4 * 2^-24      (rstd = (var + eps)^-1/2, allowing a 2-ulp reciprocal square root)
    Both are capped at 1e-4 (of the channel's RMS for the mean): the bound may be tighter than that, never looser."""
    kernel, shape, scope = sc
    case = _case_of(kernel, shape)
    _, _, _, _, n, H, W_, _, R = case
    prec = Precision.get(half)
    spec = RC.spec_of(case)
    x, w, bias = _inputs(case, prec.dtype)
    _, _, hi, wi, _, ho, wo, cop, hq, wq = RC.geometry(case)
    with ops.half_mode(half):
        be = hip()
        packed = ops.PackedWeights(spec.forward_plan(), DEV, False)
        be.pack_weights(packed, w.to(DEV))
        y = torch.empty((n, ho, wo, cop), dtype=prec.dtype, device=DEV)
        nch = be.conv_forward(packed, x.to(DEV), y, hq, wq, bias.to(DEV), L.ACT_NONE, L.ACT_NONE, prec.prec, splitk=1, want_stats=True)
        _, nstrips, segs = RC.strips(case)
        assert DRY or (be.last_conv_kernel == RC.KERNEL_NAME[kernel] and nch == segs * nstrips), (be.last_conv_kernel, nch, segs, nstrips)
        affine = scope == L.NORM_BATCH
        g = (1 + 0.1 * torch.randn(cop, generator=torch.Generator().manual_seed(4))).to(DEV) if affine else None
        b = (0.1 * torch.randn(cop, generator=torch.Generator().manual_seed(5))).to(DEV) if affine else None
        z = torch.empty_like(y)
        st = be.norm_forward(y, z, cop, scope, L.ACT_RELU, g, b, None, None, -1.0, None, ext_nchunks=nch)
        sync()
    mean, rstd = st[0].double().cpu(), st[1].double().cpu()          # [N, C]
    yv = y.double().cpu()
    dims = (0, 1, 2) if scope == L.NORM_BATCH else (1, 2)
    m_ref = yv.mean(dim=dims, keepdim=True)
    e_abs = yv.abs().mean(dim=dims, keepdim=True).reshape(-1, cop)
    e_sq = (yv * yv).mean(dim=dims, keepdim=True).reshape(-1, cop)
    v_ref = ((yv - m_ref) ** 2).mean(dim=dims, keepdim=True).reshape(-1, cop)
    m_ref = m_ref.reshape(-1, cop)
    r_ref = 1.0 / torch.sqrt(v_ref + 1e-5)
    P = (128 if kernel == 's2d' else 256) * R
    nch_geom = segs * nstrips
    lsum = P // 16 + 6 + nch_geom * (n if scope == L.NORM_BATCH else 1)
    u = conv_ref.U32
    tol_mean = torch.minimum((lsum + 2) * u * e_abs, 1e-4 * e_sq.sqrt())
    d_var = (lsum + 6) * u * (e_sq + 2 * m_ref.abs() * e_abs)
    tol_rstd = torch.clamp(d_var / (2 * (v_ref + 1e-5)) + 4 * u, max=1e-4)
    r_mean = float(((mean - m_ref).abs() / tol_mean).max())
    r_rstd = float((((rstd - r_ref) / r_ref).abs() / tol_rstd).max())
    tag = f'{half}/stats/{RC.case_id(case)}/{"batch" if scope == L.NORM_BATCH else "instance"}'
    ERRLOG[tag + '/mean'], ERRLOG[tag + '/rstd'] = r_mean, r_rstd
    print(f'{tag}: Lsum {lsum}, worst err/bound mean {r_mean:.4f} rstd {r_rstd:.4f}; bounds mean/RMS <= {float((tol_mean / e_sq.sqrt()).max()):.2e}, '
          f'rstd rel <= {float(tol_rstd.max()):.2e}')
    assert mean.shape == (n, cop) and r_mean <= 1.0 and r_rstd <= 1.0, (tag, r_mean, r_rstd)


# ---- channel-slice views
SLICE_CASES = [('bf16', 's2d', (7, 420, 256)), ('fp16', 's2d', (2, 512, 512)), ('bf16', 's2u', (6, 180, 128)), ('fp16', 's2u', (2, 256, 256)),
               ('bf16', 'd1', (12, 384, 512))]


@pytest.mark.parametrize('sl', SLICE_CASES, ids=lambda s: f'{s[0]}-{s[1]}-n{s[2][0]}h{s[2][1]}w{s[2][2]}')
def test_channel_slices_of_wider_buffers(sl):
    """in_pstride / out_pstride twice the channel count (UNet-style concat buffers) at a strip height above 2: s2d and s2u read the upper half of one buffer and
    write the upper half of another; conv_d1 (whose 8-channel input is never a slice) writes one.  The other half must keep its bits."""
    half, kernel, shape = sl
    case = _case_of(kernel, shape)
    _, _, _, _, n, H, W_, _, R = case
    assert R > 2
    prec = Precision.get(half)
    spec = RC.spec_of(case)
    x, w, bias = _inputs(case, prec.dtype)
    _, _, hi, wi, cip, ho, wo, cop, hq, wq = RC.geometry(case)
    act = L.ACT_LRELU if kernel == 'd1' else L.ACT_NONE
    with ops.half_mode(half):
        be = hip()
        packed = ops.PackedWeights(spec.forward_plan(), DEV, False)
        be.pack_weights(packed, w.to(DEV))
        if kernel == 'd1':
            xin = x.to(DEV)
        else:
            wide_in = torch.full((n, hi, wi, 2 * cip), 7.0, dtype=prec.dtype, device=DEV)
            wide_in[..., cip:] = x.to(DEV)
            xin = wide_in[..., cip:]
        wide_out = torch.full((n, ho, wo, 2 * cop), -3.0, dtype=prec.dtype, device=DEV)
        be.conv_forward(packed, xin, wide_out[..., cop:], hq, wq, bias.to(DEV), act, L.ACT_NONE, prec.prec, 1)
        sync()
        assert DRY or be.last_conv_kernel == RC.KERNEL_NAME[kernel], be.last_conv_kernel
    ref, S, K = conv_ref.Reference(spec, 'fwd', x, w).variant(bias, act)
    bnd = conv_ref.bound(ref, S, K, prec.dtype, SUM_SLACK)
    worst, report = conv_ref.compare(wide_out[..., cop:], ref, bnd, _geom(case))
    tag = f'{half}/slice/{RC.case_id(case)}'
    ERRLOG[tag] = worst
    assert worst <= 1.0 and not report, f'{tag}\n{report}'
    assert bool((wide_out[..., :cop] == -3.0).all()), 'the other half of the output buffer must be untouched'
    if kernel != 'd1':
        assert bool((wide_in[..., :cip] == 7.0).all())


# ---- the names against the launches
_CONV_KERNEL = re.compile(r'conv_[a-z0-9_]*?kernel')


@pytest.mark.skipif(DRY, reason='needs the profiler on a GPU')
def test_kernel_names_match_the_traced_launches(tmp_path):
    """dl_conv_kernel_name reports the decision of conv_route() (csrc/conv_gemm.hip), the same one the launch of dl_conv_forward switches on; every 'the
    dispatch took the new kernel' assertion of the suite reads the name.  What only a trace can show is that each arm of the launch switch starts the kernel its
    row of the name table says: a fresh child process (tests/regconv_trace_child.py) runs one small call per route -- the special kernels and the tile family --
    under a kernel trace and prints the name the library reports for each; the convolution kernels in the trace, in launch order, must be exactly those.  Where
    the reported name carries template arguments (the tile of conv_gemm_glds_kernel, the storage type of conv_gemm_kernel) they must lead the traced kernel's;
    the launch grids of the strip kernels must be what conv_ref.strip_rows predicts."""
    prof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    assert os.path.exists(prof), 'rocprofv3 not found'
    cmd = ['timeout', '-k', '10', '300', prof, '--kernel-trace', '--output-format', 'csv', '-d', str(tmp_path), '--', sys.executable,
           os.path.join(ROOT, 'tests', 'regconv_trace_child.py')]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, f'exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}'
    routes = [ln.split(' ', 2)[1:] for ln in r.stdout.splitlines() if ln.startswith('ROUTE ')]
    assert len(routes) >= 36 and 'CHILD DONE' in r.stdout, r.stdout[-3000:]
    import csv
    rows = []
    for dirpath, _, files in os.walk(tmp_path):
        for fn in files:
            if fn.endswith('kernel_trace.csv'):
                with open(os.path.join(dirpath, fn), newline='') as f:
                    rows += list(csv.DictReader(f))
    assert rows, f'no kernel trace under {tmp_path}: {[fs for _, _, fs in os.walk(tmp_path)]}'
    rows.sort(key=lambda row: int(row['Start_Timestamp']))
    conv_rows = [row for row in rows if _CONV_KERNEL.search(row['Kernel_Name'])]
    table = '\n'.join(f'{lab:40s} {name}' for lab, name in routes)
    launched = [_CONV_KERNEL.search(row['Kernel_Name']).group(0) for row in conv_rows]
    named = [_CONV_KERNEL.search(name).group(0) for _, name in routes]
    assert launched == named, f'launched: {launched}\nnamed:\n{table}'
    for k in RC.KERNEL_NAME.values():
        assert k in launched, f'{k} was never launched'
    import regconv_trace_child as T
    cases = T.route_cases()
    assert [lab for lab, _ in cases] == [lab for lab, _ in routes]
    for row, (label, name), (_, case) in zip(conv_rows, routes, cases):
        # template arguments the library reports (conv_gemm_glds_kernel<128,64,64>: the tile) are the leading template arguments of the traced kernel
        if '<' in name:
            # (conv_gemm_kernel<bf16> / <f32>: the library names the storage type, the trace spells the C++ type of its first template argument)
            want_args = [{'bf16': 'unsigned short', 'f32': 'float'}.get(a.strip(), a.strip()) for a in name[name.index('<') + 1:name.rindex('>')].split(',')]
            traced = row['Kernel_Name']
            got_args = [a.strip() for a in traced[traced.index('<') + 1:traced.rindex('>')].split(',')]
            assert got_args[:len(want_args)] == want_args, (label, name, traced)
        # the strip kernels' launch grids: ties conv_ref.strip_rows (the sweep's coverage guard) to the *_strip_rows rules that really ran -- for conv_d1 / conv_d1g,
        # which report no statistics chunks, this is the only such tie; the 16 x 512 x 512 routes sit where the 480-workgroup threshold decides R
        if case is not None and RC.KERNEL_NAME.get(case[0]) == _CONV_KERNEL.search(name).group(0) and case[0] in RC.R_WANTED:
            wgs, wg = T.workgroups(case), int(row['Workgroup_Size_X'])
            assert int(row['Grid_Size_X']) == wgs * wg and int(row['Grid_Size_Y']) == 1, (label, row['Grid_Size_X'], wgs, wg)
