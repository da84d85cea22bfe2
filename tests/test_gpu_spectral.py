"""Spectral normalisation (`--norm spectral`) on the MI355X: the kernels of csrc/spectral.hip through the C ABI against torch in float64, the
spectrally normalised networks against torch's own forward of the deep-copied container tree (torch.nn.utils.parametrizations._SpectralNorm) in float64,
two training steps against the trajectory recorded from the reference (tests/golden/step_spectral_m2.npz) and the save -> init_nets -> run_dask path.
Companion of tests/test_spectral_host.py (same nets, same fixture, emulated backend)."""
import os

import numpy as np
import pytest
import torch

import spectral_util as SU
from deepliif_amd import engine as E
from deepliif_amd import inference as I
from deepliif_amd import models as M
from deepliif_amd import ops
from golden_util import digest_close, seeded_uniform
from test_gpu_networks import ERRLOG, GRAD_FLOOR, LAYER_NOISE, TOL_OUT, conv_noise, l2, make_opt
from test_spectral_host import SIZES, SMALL, Z, check_step, input_for

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def _real_backend():
    ops._impl = None
    yield
    ops._impl = None


def rel(a, b, floor=1e-30):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(floor))


# -----------------------------------------------------------------------------------------------------------------------------------
# kernels
# -----------------------------------------------------------------------------------------------------------------------------------
def kernel_cases():
    """seven weights: (shape, dim).  Matrix views 1 x 1024 (Cout = 1), 8 x 147 and 3 x 392 (odd widths: scalar path), 32 x 144, 16 x 288 read in place from
    a ConvTranspose2d(32, 16, 3) weight (dim 1), 256 x 2304 (16 x 3 tiles) and 512 x 4096 (32 x 4 tiles): the last two spread over many workgroups"""
    return [((1, 64, 4, 4), 0), ((8, 3, 7, 7), 0), ((3, 8, 7, 7), 0), ((32, 16, 3, 3), 0), ((32, 16, 3, 3), 1), ((256, 256, 3, 3), 0), ((512, 256, 4, 4), 0)]


def make_jobs(seed, with_grad, dtype, device):
    g = torch.Generator().manual_seed(seed)
    jobs = []
    for shape, dim in kernel_cases():
        w = (0.05 * torch.randn(shape, generator=g)).to(dtype).to(device)
        rows = shape[dim]
        cols = w.numel() // rows
        u = torch.randn(rows, generator=g)
        v = torch.randn(cols, generator=g)
        u, v = (u / u.norm()).to(dtype).to(device), (v / v.norm()).to(dtype).to(device)
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=device)
        gr = torch.randn(shape, generator=g).to(dtype).to(device) if with_grad else None
        g0 = (0.1 * torch.randn(shape, generator=g)).to(dtype).to(device) if with_grad else None
        jobs.append(ops.SpectralJob(w, dim, u, v, z(shape), z(rows), z(cols), z(1), gr, g0))
    return jobs


def reference_run(jobs, iterate, dtype):
    """torch's formulas on CPU copies of the jobs' inputs in `dtype`: [(u, v, sigma, weff)]"""
    out = []
    for j in jobs:
        out.append(SU.spectral_forward_ref(j.w.cpu().to(dtype), j.dim, j.u.cpu().to(dtype), j.v.cpu().to(dtype), iterate))
    return out


def maxabs_err(a, b):
    b = b.double()
    return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('iterate', [True, False])
def test_spectral_kernels_against_float64(iterate):
    """u, v, sigma, W / sigma of dl_spectral_forward and both accumulate modes of dl_spectral_backward, one batched call over the seven matrices.
    Bound: the error of torch's own float32 CPU evaluation of the same formulas against float64 on the same inputs, times 10 (another summation order),
    relative to each tensor's max-abs (sigma: the vector of the seven sigmas).
    Measured ratios kernel error / float32-CPU error (MI355X), worst over the seven jobs -- iterating: u 0.82, v 1.10, W/sigma 1.70, sigma 1.91, gradient 1.55
    ('=') and 1.35 ('+='); not iterating (u, v copied bit for bit): W/sigma 1.00, sigma 0.21, gradient 0.80 / 0.79.  Absolute: 6e-8 ... 2.6e-6 of max-abs.
    Every figure is printed before the assertion."""
    be = ops.impl()
    jobs = make_jobs(11, True, torch.float32, DEV)
    u0 = [j.u.clone() for j in jobs]
    v0 = [j.v.clone() for j in jobs]
    g0 = [j.grad.clone() for j in jobs]
    ref64 = reference_run(jobs, iterate, torch.float64)
    ref32 = reference_run(jobs, iterate, torch.float32)
    table = be.spectral_table(jobs)
    be.spectral_forward(table, iterate)
    torch.cuda.synchronize()
    ratios = {}

    def check(name, got, r32, r64):
        e_kernel, e_cpu = maxabs_err(got, r64), maxabs_err(r32, r64)
        ratios[name] = (e_kernel, e_cpu)
        print(f'spectral kernel iterate={iterate} {name}: kernel {e_kernel:.3e} float32-cpu {e_cpu:.3e} ratio {e_kernel / max(e_cpu, 1e-300):.2f}')
        ERRLOG[f'spectral/kernel/iter{int(iterate)}/{name}'] = [e_kernel, e_cpu]
        return e_kernel <= 10 * e_cpu

    bad = []
    for i, j in enumerate(jobs):
        for name, got, k in (('u', j.u_snap, 0), ('v', j.v_snap, 1), ('weff', j.weff, 3)):
            if not check(f'{name}{i}', got, ref32[i][k], ref64[i][k]):
                bad.append(f'{name}{i}')
        if iterate:
            assert torch.equal(j.u, j.u_snap) and torch.equal(j.v, j.v_snap)
        else:
            assert torch.equal(j.u, u0[i]) and torch.equal(j.v, v0[i]) and torch.equal(j.u_snap, u0[i]) and torch.equal(j.v_snap, v0[i])
    sig = torch.cat([j.sigma for j in jobs])
    if not check('sigma', sig, torch.stack([r[2] for r in ref32]), torch.stack([r[2] for r in ref64])):
        bad.append('sigma')
    # backward: '=' first (into a buffer of garbage), then '+=' on top of a known gradient
    for accumulate in (False, True):
        for i, j in enumerate(jobs):
            j.grad.copy_(g0[i])
        be.spectral_backward(table, accumulate)
        torch.cuda.synchronize()
        for i, j in enumerate(jobs):
            outs = []
            for dt in (torch.float32, torch.float64):
                # the gradient formula on the float64 / float32 results of the forward above (u, v are constants of the graph)
                u, v, s, weff = (ref64 if dt == torch.float64 else ref32)[i]
                d = SU.spectral_backward_ref(j.g.cpu().to(dt), weff, j.dim, u, v, s)
                outs.append(d + g0[i].cpu().to(dt) if accumulate else d)
            if not check(f'grad{i}/acc{int(accumulate)}', j.grad, outs[0], outs[1]):
                bad.append(f'grad{i}/acc{int(accumulate)}')
    assert not bad, {k: ratios[k] for k in bad}


def test_spectral_kernels_are_bit_reproducible():
    be = ops.impl()
    results = []
    for _ in range(2):
        jobs = make_jobs(12, True, torch.float32, DEV)
        table = be.spectral_table(jobs)
        be.spectral_forward(table, True)
        be.spectral_forward(table, False)
        be.spectral_backward(table, True)
        torch.cuda.synchronize()
        results.append([t.clone() for j in jobs for t in (j.u, j.v, j.u_snap, j.v_snap, j.sigma, j.weff, j.grad)])
    assert all(torch.equal(a, b) for a, b in zip(*results))


def test_spectral_backward_on_a_subset_leaves_the_other_gradients_alone():
    be = ops.impl()
    jobs = make_jobs(13, True, torch.float32, DEV)
    table = be.spectral_table(jobs)
    be.spectral_forward(table, True)
    before = [j.grad.clone() for j in jobs]
    be.spectral_backward(table, True, only=(1, 4, 6))
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        assert torch.equal(j.grad, before[i]) == (i not in (1, 4, 6)), i


# -----------------------------------------------------------------------------------------------------------------------------------
# networks
# -----------------------------------------------------------------------------------------------------------------------------------
def gpu_net(tag, precname, seed=3, settle=0):
    """settle: power iterations (torch's own, on the CPU) between the seeded fill and the copies -- u, v of a trained checkpoint are near the leading singular
    pair; the random unit vectors of fill_seeded give a sigma = u^T M v of any size, down to ~0"""
    net = SMALL[tag]()
    SU.fill_seeded(net, seed)
    if settle:
        net.model.train()
        with torch.no_grad():
            for _ in range(settle):
                SU.twin_forward(net.model, input_for(net, (16, 16), n=1))
    twin = SU.float64_twin(net.model)
    net.to(DEV)
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    return net.set_precision(precname), twin


@pytest.mark.parametrize('precname', ['fp32', 'bf16'])
@pytest.mark.parametrize('hw', SIZES)
@pytest.mark.parametrize('tag', list(SMALL))
def test_network_forward_backward_match_torch_spectral_norm(tag, hw, precname):
    net, twin = gpu_net(tag, precname)
    net.train()
    twin.train()
    x = input_for(net, hw)
    prec = E.Precision.get(precname)
    tape = E.Tape()
    ctx = E.Ctx(prec, tape, training=True)
    xa = E.to_engine(x.to(DEV), prec)
    xa.needs_grad = True
    ya = net.run(ctx, xa)
    buffers0 = [b.clone() for b in twin.buffers()]

    def reference(noise_seed=None):
        """(y, dx, {key: dw}) of torch's forward of the float64 twin from the same u, v -- clean, or with this policy's rounding noise on every conv output"""
        for b, b0 in zip(twin.buffers(), buffers0):
            b.copy_(b0)
        twin.zero_grad()
        xo = x.double().requires_grad_(True)
        if noise_seed is None:
            yo = SU.twin_forward(twin, xo)
        else:
            with conv_noise(LAYER_NOISE[precname], noise_seed):
                yo = SU.twin_forward(twin, xo)
        r = torch.randn(yo.shape, generator=torch.Generator().manual_seed(7))
        (yo * r.double()).sum().backward()
        return yo.detach(), r, xo.grad, {k: p.grad.clone() for k, p in twin.named_parameters()}

    yo, r, dxo, dwo = reference()
    key = f'spectral/{tag}-{hw[0]}x{hw[1]}-{precname}'
    e_out = ERRLOG[key + '/y'] = rel(E.from_engine(ya), yo)
    ya.grad = E.to_engine(r.to(DEV), prec).t
    tape.backward()
    e_dx = ERRLOG[key + '/dx_l2'] = l2(E.from_engine(E.Act(xa.grad, xa.C)), dxo)
    e_dw = {k: l2(p.grad, dwo[k]) for k, p in net.model.named_parameters()}
    ERRLOG[key + '/dw_l2_worst'] = max(e_dw.values())
    e_uv = max(rel(b, b2) for (_, b), (_, b2) in zip(net.model.named_buffers(), twin.named_buffers()))
    # The bound of tests/test_gpu_networks.py: GRAD_FLOOR, or 4 x the reference's OWN gradient sensitivity to rounding noise of this policy's size when that is
    # larger.  These nets have no normalisation layer, so a pre-activation near zero flips its ReLU mask under fp32-sized noise and the float64 twin's own dx
    # moves by 1.2e-2 (g_resize_conv, 48 x 40: 4 of 8 draws; 7e-7 in the others); under bf16-sized noise it moves by 0.14 - 0.16.  Measured on the MI355X:
    # fp32 dx / worst dw 1.0e-5 ... 1.5e-5 where no mask flips and 1.22e-2 / 1.25e-2 (that flip; the twin's own sensitivity there: 1.27e-2 / 1.31e-2) on
    # g_resize_conv 48 x 40; bf16 0.12 - 0.14 on the generators (sensitivity 0.16 - 0.18) and 0.06 - 0.09 on the discriminator (0.09 - 0.14).
    s_dx, s_dw = 0.0, {k: 0.0 for k in e_dw}
    for seed in range(1, 9):
        _, _, dxn, dwn = reference(seed)
        s_dx = max(s_dx, l2(dxn, dxo))
        for k in s_dw:
            s_dw[k] = max(s_dw[k], l2(dwn[k], dwo[k]))
    ERRLOG[key + '/reference_sensitivity_dx_l2'] = s_dx
    print(f'{key}: y {e_out:.3e} dx {e_dx:.3e} (reference sensitivity {s_dx:.3e}) dw worst {max(e_dw.values()):.3e} ({max(e_dw, key=e_dw.get)}, '
          f'sensitivity {s_dw[max(e_dw, key=e_dw.get)]:.3e}) u/v {e_uv:.3e}')
    assert e_out < TOL_OUT[precname]
    assert e_dx <= max(GRAD_FLOOR[precname], 4 * s_dx), (e_dx, s_dx)
    bad = {k: (v, s_dw[k]) for k, v in e_dw.items() if v > max(GRAD_FLOOR[precname], 4 * s_dw[k])}
    assert not bad, bad
    assert e_uv < 1e-5              # fp32 arithmetic whatever the policy


def test_fp16_eval_forward_is_no_worse_than_bf16():
    """the fp16 inference policy (libdeepliif_hip_f16.so) on a spectral generator: finite, and at least as near to the float64 twin as the bf16 policy on
    the same input (11 significand bits against 8).  Measured (MI355X): bf16 6.6e-3, fp16 9.2e-4 of the output's max-abs."""
    errs = {}
    for precname in ('bf16', 'fp16'):
        net, twin = gpu_net('g_convtranspose', precname, settle=10)        # (sigma of un-iterated random u, v is ~100 x too small: the activations leave half's range)
        net.eval()
        twin.eval()
        x = input_for(net, (48, 40))
        with torch.no_grad():
            y = net(x.to(DEV))
            yo = SU.twin_forward(twin, x.double())
        assert torch.isfinite(y).all()
        errs[precname] = ERRLOG[f'spectral/eval/{precname}'] = rel(y, yo)
    print(f'spectral eval forward vs float64 twin: bf16 {errs["bf16"]:.3e} fp16 {errs["fp16"]:.3e}')
    assert errs['fp16'] <= errs['bf16'] and errs['bf16'] < TOL_OUT['bf16']


# -----------------------------------------------------------------------------------------------------------------------------------
# model: the step fixture, save -> init_nets -> run_dask
# -----------------------------------------------------------------------------------------------------------------------------------
def spectral_model(precname, tmp=None):
    opt = make_opt(2, True, 'spectral', 'unet_64', 8, precname)
    if tmp is not None:
        opt.checkpoints_dir = str(tmp)
    model = M.create_model(opt)
    model.setup(opt)
    for name, seed in zip(Z['model_names'], Z['net_seeds']):
        SU.fill_seeded(getattr(model, 'net' + str(name)), int(seed))
    size, batch = int(Z['meta'][5]), int(Z['meta'][7])
    A = seeded_uniform((batch, 3, size, size), 22)
    B = [seeded_uniform((batch, 3, size, size), 23 + i) for i in range(3)]
    return model, opt, A, B


@pytest.mark.parametrize('precname', ['fp32', 'bf16'])
def test_training_steps_follow_the_reference(precname):
    model, _, A, B = spectral_model(precname)
    for s in range(int(Z['meta'][8])):
        model.set_input({'A': A, 'B': B, 'A_paths': ['x']})
        model.optimize_parameters()
        worst, ltol, otol = check_step(model, s, precname, ERRLOG)
        print(f'spectral step {s} {precname}: ' + ' '.join(f'{k}={v:.2e}' for k, v in worst.items()))
        for k, v in worst.items():
            assert v <= (otol if k.startswith('fake') else ltol), (s, k, v)
        for n in model.model_names:
            net = getattr(model, 'net' + n)
            if precname == 'fp32':
                flat = torch.cat([v.reshape(-1).float().cpu() for v in net.state_dict().values() if v.is_floating_point()])
                ok, msg = digest_close(flat, Z[f'step{s}/w_digest/{n}'], 8e-3)
                assert ok, f'step {s} weights of {n}: {msg}'
            if net.spectral_norm and precname == 'fp32':
                uv = torch.cat([v.reshape(-1).float().cpu() for k, v in net.state_dict().items() if k.endswith('._u') or k.endswith('._v')])
                ok, msg = digest_close(uv, Z[f'step{s}/uv_digest/{n}'], 1e-3)
                assert ok, f'step {s} u / v of {n}: {msg}'


def test_save_init_nets_run_dask_round_trip(tmp_path):
    """a spectral model trains a step, save_networks writes the reference's keys, init_nets loads the directory and the run_dask path serves the
    training side's eval forward"""
    model, opt, A, B = spectral_model('fp32', tmp_path)
    model.set_input({'A': A, 'B': B, 'A_paths': ['x']})
    model.optimize_parameters()
    model.save_networks('latest')
    sd = torch.load(os.path.join(model.save_dir, 'latest_net_G1.pth'), map_location='cpu')
    assert any(k.endswith('parametrizations.weight.original') for k in sd) and any(k.endswith('parametrizations.weight.0._v') for k in sd)
    model.eval()
    model.set_input({'A': A, 'B': B, 'A_paths': ['x']})
    with torch.no_grad():
        model.test()
    S = str(model.mod_id_seg)
    expected = {'G1': model.fake_B_1, 'G2': model.fake_B_2, 'G' + S: getattr(model, f'fake_B_{S}')}
    I._NETS_CACHE.clear()
    ropt = serve_opt(opt, model)
    nets = I.init_nets(model.save_dir, eager_mode=True, opt=ropt)
    assert all(not net.training for net in nets.values()) and nets['G1'].spectral_norm and not nets['G' + S + '0'].spectral_norm
    for t in range(A.shape[0]):
        res = I.run_dask(A[t:t + 1], nets=nets, opt=ropt, use_dask=False, output_tensor=True)
        for k, exp in expected.items():
            assert rel(res[k], exp[t:t + 1]) < 1e-5, (t, k)
    I._NETS_CACHE.clear()


def serve_opt(opt, model):
    import types
    o = types.SimpleNamespace(**vars(opt))
    o.is_train, o.phase, o.gpu_ids = False, 'test', [0]
    o.mod_id_seg, o.input_id = model.mod_id_seg, int(model.input_id)
    o.modalities_names = ['IHC', 'Hema', 'DAPI']
    o.scale_size = int(Z['meta'][5])
    return o
