"""GPU sweep of the tile-family convolution kernels -- the 18 routes of conv_route() (csrc/conv_gemm.hip) that are not weights-in-registers kernels:
conv_gemm_8ph_kernel, the four conv_gemm_glds_kernel tiles, conv_gemm_w4_kernel, conv_gemm_kernel<bf16> / <f32>, conv_s2f_kernel, conv_c4_patch_kernel and the
strict-policy family of conv_x3.h, conv_s2f_x3.hip and conv_w4x3.hip -- over the rows of tests/tileconv_cases.py: the smallest shapes that reach each kernel
and each geometry edge (ragged last tiles, tiles that straddle two images, one-step K loops, zero-padded contracted channels, four-phase plans at odd sizes,
split-K slabs, in-kernel reflect / replicate borders, the reversed kernel-column order of the w4 data gradient), under the four precision policies.

Every row goes through ops.impl().conv_forward with the row's split-K, split-copy input and runtime switch, asserts by name (dl_conv_kernel_name before, last_conv_kernel
after the launch) that the dispatch took the kernel under test, and is compared element by element with a float64 convolution under the derived bound of
tests/conv_ref.py (no element may be out of bound; sum_slack = 1).  A failure prints where the bad elements are (image, row, tile, pixel / channel residues).
The worst err / bound of every row goes to parity_errors_tileconv.json in the directory $DL_PARITY_DIR names (default parity_out/); a copy of the MI355X run is
kept as profiles/r06/parity_errors_tileconv.json, next to the register kernels'.

DL_TEST_DRYRUN=1 runs the file on the CPU with the formula emulation in the kernels' place (a check of the test code only: the emulation knows neither split
copies nor the staged rounding nor a replicate border, so the dry run hands it the operand model's values and an explicitly padded input)."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

import conv_ref
import tileconv_cases as TC
from deepliif_amd import _lib as L
from deepliif_amd import ops
from deepliif_amd.geometry import ConvSpec, cpad

from test_gpu_kernels import DEV, DRY, _split_copy, hip, sync

pytestmark = pytest.mark.gpu
ERRLOG = {}
ERRLOG_DIR = os.environ.get('DL_PARITY_DIR', 'parity_out')
SUM_SLACK = 1            # multiplier of the summation term of the bound (conv_ref.bound); 1 = as derived
# pixels per tile of each kernel (g_routes of csrc/conv_gemm.hip; conv_s2f: 256 phase-grid pixels), for the comparer's report only
BM = {TC.G16: 256, TC.G64: 128, TC.G128: 128, TC.G256: 256, TC.PH8: 256, TC.W4: 256, TC.S2F: 256, TC.S2FX: 256, TC.X16: 256, TC.X32: 256, TC.X64: 128,
      TC.X128: 128, TC.PH8X: 256, TC.W4X: 256}


@pytest.fixture(autouse=True)
def _real_backend_again():
    yield
    ops._impl = None


@pytest.fixture(autouse=True, scope='module')
def _errlog():
    yield
    os.makedirs(ERRLOG_DIR, exist_ok=True)
    with open(os.path.join(ERRLOG_DIR, 'parity_errors_tileconv.json'), 'w') as f:
        json.dump(ERRLOG, f, indent=1, sort_keys=True)


def _storage(row, half):
    return ops.H16_DTYPE[half] if row.policy == 'bf16' else torch.float32


def _inputs(row, half):
    """(x, w, bias) as float32 host tensors holding the STORED values: the tensor the kernel reads (layer input, or dL/dy for a data gradient; padding
    channels zero), the layer's weight, its bias.  'bf16': x and w exactly representable in the library's 16-bit format; 'fp32+bf16': w pre-rounded to the
    16-bit format, x with a full mantissa (the kernel rounds it while staging); strict: full mantissas."""
    h16 = ops.H16_DTYPE[half]
    spec = TC.spec_of(row)
    g = torch.Generator().manual_seed(1)
    w = torch.randn((spec.cout, spec.cin, spec.k, spec.k) if row.kind == 'conv' else (spec.cin, spec.cout, spec.k, spec.k), generator=g) * 0.05
    if not row.policy.startswith('strict'):
        w = w.to(h16).float()
    bias = torch.randn((spec.cout,), generator=torch.Generator().manual_seed(2)) * 0.1
    _, n, hi, wi, cip, _, _, _, _, _ = TC.geometry(row)
    c = spec.cin if row.direction == 'fwd' else spec.cout
    x = torch.zeros(n, hi, wi, cip)
    v = torch.randn((n, hi, wi, c), generator=torch.Generator().manual_seed(3 if row.direction == 'fwd' else 4))
    x[..., :c] = v.to(h16).float() if row.policy == 'bf16' else v
    return x, w, bias


def _reference(row, half, x, w):
    return conv_ref.Reference(TC.spec_of(row), row.direction, x, w, in_hw=(row.H, row.W), policy=row.policy, in_act=row.in_act, h16=ops.H16_DTYPE[half])


def _launch(be, row, half, x, w, bias, out=None, xin=None, want_stats=False):
    """one dl_conv_forward of the row; x, w, bias: host tensors of the stored values.  out / xin: views to write / read instead of fresh tensors (xin already on
    the device, in the storage type).  Returns (out, chunks of fused statistics)."""
    plan, n, hi, wi, cip, ho, wo, cop, hq, wq = TC.geometry(row)
    dtype, prec, in_split = TC.POLICY[row.policy]
    st = _storage(row, half)
    in_act = row.in_act
    if DRY:
        # the emulation multiplies whatever it is given in fp32: give it the operand model's values; a replicate border: pad explicitly, padding-0 plan
        in_split = 0
        if xin is None:
            c = x.shape[3]
            xm = conv_ref.model_values(x, in_act, row.policy, ops.H16_DTYPE[half]).float()
            if row.pad_mode == L.PAD_REPLICATE:
                xm = F.pad(xm.permute(0, 3, 1, 2), (row.pad,) * 4, mode='replicate').permute(0, 2, 3, 1).contiguous()
                plan = ConvSpec(row.kind, row.cin, row.cout, row.k, row.stride, 0, L.PAD_ZERO, 0).forward_plan()
            xin = xm if st == torch.float32 else xm.to(st)
            assert xin.shape[3] == c
            in_act = L.ACT_NONE
        else:
            assert in_act == L.ACT_NONE or row.policy.startswith('strict'), 'dry run: a staged activation on a view needs the strict policy'
    if xin is None:
        xin = x.to(st).to(DEV)
        if in_split:
            xin = _split_copy(xin)
    packed = ops.PackedWeights(plan, DEV, prec == L.PREC_BF16X3)
    be.pack_weights(packed, w.to(DEV))
    if out is None:
        out = torch.empty((n, ho, wo, cop), dtype=st, device=DEV)
    nch = be.conv_forward(packed, xin, out, hq, wq, bias.to(DEV) if row.bias else None, row.act, in_act, prec, splitk=row.splitk, want_stats=want_stats,
                          in_split=bool(in_split))
    return out, nch


def _geom(row):
    bm = BM.get(row.kernel)
    return {'bm': bm, 'step': 2 if TC.geometry(row)[0].n_phase == 4 else 1} if bm else None


def _sweep(row, half, twice=False):
    st = _storage(row, half)
    spec = TC.spec_of(row)
    x, w, bias = _inputs(row, half)
    tag = f'{half}/{TC.case_id(row)}'
    with ops.half_mode(half):
        real = hip()
        assert DRY or real.half == half
        lib = L.load(half)
        with TC.switched(lib, row):
            assert TC.kernel_name(lib, row) == row.kernel, tag
            got, _ = _launch(real, row, half, x, w, bias)
            assert DRY or real.last_conv_kernel == row.kernel, (tag, real.last_conv_kernel)
            sync()
            if twice:
                again, _ = _launch(real, row, half, x, w, bias)
                sync()
                assert torch.equal(got, again), f'{tag}: run-to-run difference'
                del again
    ref, S, K = _reference(row, half, x, w).variant(bias if row.bias else None, row.act)
    bnd = conv_ref.bound(ref, S, K, st, SUM_SLACK, row.policy, row.act)
    del S
    worst, report = conv_ref.compare(got, ref, bnd, _geom(row))
    del ref, bnd
    ERRLOG[tag] = worst
    print(f'{tag}: {row.kernel} worst err/bound {worst:.4f}')
    assert worst <= 1.0 and not report, f'{tag} ({row.kernel})\n{report}'
    c_real = spec.cout if row.direction == 'fwd' else spec.cin
    if cpad(c_real) > c_real:
        assert float(got[..., c_real:].float().abs().max()) == 0.0, f'{tag}: the padding channels must stay exactly zero'


def _first_rows_per_kernel(rows):
    seen, out = set(), set()
    for r in rows:
        if r.kernel not in seen and r.direction == 'fwd':
            seen.add(r.kernel)
            out.add(r)
    return out


# one row per kernel (its first forward row) also checks that two launches give the same bits
TWICE = _first_rows_per_kernel(TC.ALL_ROWS)


def test_the_table_reaches_every_route():
    routes = TC.check_coverage()
    assert len(routes) == 18 and {r.kernel for r in TWICE} == set(routes)
    TC.check_coverage_f16()


@pytest.mark.parametrize('row', TC.ALL_ROWS, ids=TC.case_id)
def test_bf16_library(row):
    _sweep(row, 'bf16', row in TWICE)


@pytest.mark.parametrize('row', TC.F16_ROWS, ids=TC.case_id)
def test_f16_library(row):
    """the inference policy's library: the same sources with IEEE half as the 16-bit type; the forward rows of the 16-bit policy, the same bound with u = 2^-11"""
    _sweep(row, 'fp16', row in TWICE)


# ---- channel-slice views
@pytest.mark.parametrize('row', TC.SLICE_ROWS, ids=TC.case_id)
def test_channel_slices_of_wider_buffers(row):
    """in_pstride / out_pstride twice the channel count, as the UNet's concat buffers make them: the kernel reads the upper half of one buffer and writes the
    upper half of another.  The result is held to the same bound; the other halves must keep their bits."""
    half = 'bf16'
    st = _storage(row, half)
    x, w, bias = _inputs(row, half)
    _, n, hi, wi, cip, ho, wo, cop, hq, wq = TC.geometry(row)
    tag = f'{half}/slice/{TC.case_id(row)}'
    with ops.half_mode(half):
        be = hip()
        lib = L.load(half)
        assert TC.kernel_name(lib, row, in_pstride=2 * cip, out_pstride=2 * cop) == row.kernel, tag
        wide_in = torch.full((n, hi, wi, 2 * cip), 7.0, dtype=st, device=DEV)
        wide_in[..., cip:] = x.to(st).to(DEV)
        wide_out = torch.full((n, ho, wo, 2 * cop), -3.0, dtype=st, device=DEV)
        xin = wide_in[..., cip:]
        if DRY and not row.policy.startswith('strict'):
            xin = None          # (the emulation gets the operand model's values instead of the view: see _launch)
        _launch(be, row, half, x, w, bias, out=wide_out[..., cop:], xin=xin)
        assert DRY or be.last_conv_kernel == row.kernel, (tag, be.last_conv_kernel)
        sync()
    ref, S, K = _reference(row, half, x, w).variant(bias if row.bias else None, row.act)
    bnd = conv_ref.bound(ref, S, K, st, SUM_SLACK, row.policy, row.act)
    worst, report = conv_ref.compare(wide_out[..., cop:], ref, bnd, _geom(row))
    ERRLOG[tag] = worst
    assert worst <= 1.0 and not report, f'{tag}\n{report}'
    assert bool((wide_out[..., :cop] == -3.0).all()), 'the other half of the output buffer must be untouched'
    assert bool((wide_in[..., :cip] == 7.0).all()), 'the other half of the input buffer must be untouched'


# ---- fused statistics
@pytest.mark.parametrize('row', TC.STATS_ROWS, ids=TC.case_id)
def test_fused_statistics_against_float64_statistics_of_the_stored_tensor(row):
    """want_stats=True: the kernel leaves per-(image, channel) sum and sum of squares OF THE VALUES IT STORED, one chunk per tile (and phase);
    dl_norm_forward(ext_nchunks) turns them into mean and rstd (instance scope).  Checked against float64 statistics of the stored tensor.

    Bound.  A sum of the L = Ho * Wo values of one (image, channel) in fp32 passes no value through more than L - 1 additions, whatever the order and the
    grouping into lanes, tiles and chunks (Higham 4.2): |d sum| <= L 2^-24 sum|y|, |d sumsq| <= (L + 1) 2^-24 sum y^2 (one more rounding for the square).  With
    mean = sum / L and var = sumsq / L - mean^2 computed in fp32 (a handful of roundings, relative to E y^2 + mean^2), as in tests/test_gpu_regconv_sweep.py:
        |d mean| <= (L + 2) 2^-24 E|y|
        |d var|  <= (L + 6) 2^-24 (E y^2 + 2 |mean| E|y|)
        |d rstd| / rstd <= |d var| / (2 (var + eps)) + 4 * 2^-24      (rstd = (var + eps)^-1/2, allowing a 2-ulp reciprocal square root)
    Both are capped at 1e-4 (of the channel's RMS for the mean): the bound may be tighter than that, never looser.  The shapes keep L <= 1024: one dropped
    pixel moves the mean by E|y| / L, which is 2^24 / (L (L + 2)) times the bound: 16 x at L = 1024 (conv_s2f's smallest whole tile), 64 x at 512, 250 x at 256
    (the three big-tile rows) and 1000 x at 128."""
    half = 'bf16'
    st = _storage(row, half)
    x, w, bias = _inputs(row, half)
    _, n, hi, wi, cip, ho, wo, cop, hq, wq = TC.geometry(row)
    tag = f'{half}/stats/{TC.case_id(row)}'
    with ops.half_mode(half):
        be = hip()
        lib = L.load(half)
        with TC.switched(lib, row):
            assert TC.kernel_name(lib, row) == row.kernel, tag
            want = int(lib.dl_conv_stats_chunks(C.byref(TC.descriptor(row))))
            y, nch = _launch(be, row, half, x, w, bias, want_stats=True)
            assert DRY or (be.last_conv_kernel == row.kernel and nch == want and nch > 0), (tag, be.last_conv_kernel, nch, want)
        assert want > 0, tag
        z = torch.empty_like(y)
        stt = be.norm_forward(y, z, cop, L.NORM_INSTANCE, L.ACT_RELU, None, None, None, None, -1.0, None, ext_nchunks=nch)
        sync()
    mean, rstd = stt[0].double().cpu(), stt[1].double().cpu()          # [N, C]
    yv = y.double().cpu()
    m_ref = yv.mean(dim=(1, 2))
    e_abs = yv.abs().mean(dim=(1, 2))
    e_sq = (yv * yv).mean(dim=(1, 2))
    v_ref = ((yv - m_ref[:, None, None, :]) ** 2).mean(dim=(1, 2))
    r_ref = 1.0 / torch.sqrt(v_ref + 1e-5)
    lsum = ho * wo
    assert lsum <= 1024
    u = conv_ref.U32
    tol_mean = torch.minimum((lsum + 2) * u * e_abs, 1e-4 * e_sq.sqrt())
    d_var = (lsum + 6) * u * (e_sq + 2 * m_ref.abs() * e_abs)
    tol_rstd = torch.clamp(d_var / (2 * (v_ref + 1e-5)) + 4 * u, max=1e-4)
    r_mean = float(((mean - m_ref).abs() / tol_mean).max())
    r_rstd = float((((rstd - r_ref) / r_ref).abs() / tol_rstd).max())
    ERRLOG[tag + '/mean'], ERRLOG[tag + '/rstd'] = r_mean, r_rstd
    print(f'{tag}: L {lsum}, chunks {nch}, worst err/bound mean {r_mean:.4f} rstd {r_rstd:.4f}; bounds mean/RMS <= {float((tol_mean / e_sq.sqrt()).max()):.2e}, '
          f'rstd rel <= {float(tol_rstd.max()):.2e}')
    assert mean.shape == (n, cop) and r_mean <= 1.0 and r_rstd <= 1.0, (tag, r_mean, r_rstd)
