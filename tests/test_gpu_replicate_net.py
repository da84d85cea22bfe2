"""`--padding replicate` through the product path on the MI355X: networks (training graph) against the CPU oracle at the tolerances tests/test_gpu_networks.py
uses for its reflect rows, one DeepLIIF training step against OracleDeepLIIF(padding='replicate') at the step-fixture tolerances, and a served model directory
written with `padding: replicate` on both 16-bit inference policies."""
import pytest
import torch

import replicate_cases as RC
import test_gpu_networks as TGN
from deepliif_amd import _lib as L
from deepliif_amd import engine as E
from deepliif_amd import models as M
from deepliif_amd import networks as N
from deepliif_amd import ops
from golden_util import seeded_uniform
from oracle import deepliif_oracle as O
from replicate_cases import build_replicate_dir

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def _real_backend():
    ops._impl = None
    yield
    ops._impl = None


@pytest.mark.parametrize('precname', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(1, 3, 32, 32), (2, 3, 40, 24)], ids=['1x3x32x32', '2x3x40x24'])
@pytest.mark.parametrize('norm', ['batch', 'instance'])
def test_resnet_2blocks_training_graph_against_the_oracle(norm, shape, precname):
    """forward, dx and dw of a replicate-padded generator: the case body and the tolerances are those of the reflect rows of tests/test_gpu_networks.py.
    Teeth: with the very weights and input of that case the oracle with MIRRORED block borders (same keys, stem and head as for replicate) misses the
    replicate oracle by more than the output tolerance -- an engine that took the wrong border would not pass"""
    sd = O.random_state_dict('resnet_2blocks', 3, 3, 8, norm, 'replicate', 4, generator=torch.Generator().manual_seed(5))
    x = seeded_uniform(shape, 6)
    with torch.no_grad():
        assert TGN.rel(_mirrored_blocks('resnet_2blocks', sd, x, norm), O.run_generator('resnet_2blocks', sd, x, norm, 'replicate')) > TGN.TOL_OUT[precname]
    TGN.test_network_forward_backward('resnet_2blocks', 3, 8, norm, 'replicate', shape, precname)


def _mirrored_blocks(arch, sd, x, norm):
    """the oracle forward of a replicate net with the BLOCK borders mirrored instead (stem and head stay zero-padded): what a wrong border map would compute"""
    orig = O._pad
    O._pad = lambda t, p, mode: orig(t, p, 'reflect' if (mode == 'replicate' and p == 1) else mode)
    try:
        return O.run_generator(arch, sd, x, norm, 'replicate')
    finally:
        O._pad = orig


def test_full_width_blocks_run_on_both_new_instantiations():
    """resnet_2blocks at ngf 64 on (1, 3, 8, 512): the blocks see 2 x 128 pixels x 256 channels -- the forward of all four block convs on
    conv_gemm_w4_kernel, their weight gradients on wgrad_w4_kernel, both with the replicate border (asserted from the names the library reports for the
    descriptors that were launched) -- and the outputs / gradients agree with the oracle as in the small cases"""
    arch, nf, norm, shape, precname = 'resnet_2blocks', 64, 'instance', (1, 3, 8, 512), 'bf16'
    sd = O.random_state_dict(arch, 3, 3, nf, norm, 'replicate', 4, generator=torch.Generator().manual_seed(5))
    net = N.define_G(3, 3, nf, arch, norm, False, 'normal', 0.02, [0], 'replicate')
    net.load_state_dict(sd, strict=True)
    net.train()
    be = ops.impl()
    seen = {'conv': [], 'wgrad': []}
    conv_forward, conv_wgrad = be.conv_forward, be.conv_wgrad

    def spy_conv(packed, *a, **k):
        r = conv_forward(packed, *a, **k)
        if packed.plan.pad_mode == L.PAD_REPLICATE:
            seen['conv'].append(be.last_conv_kernel)
        return r

    def spy_wgrad(P, Q, grad, k, step, pad, pad_mode, *a, **kw):
        if pad_mode == L.PAD_REPLICATE:
            d = RC.wgrad_desc('replicate', P.shape[0], P.shape[1], P.shape[2], P.shape[3], Q.shape[3], p_pstride=P.stride(2), q_pstride=Q.stride(2))
            seen['wgrad'].append(RC.wgrad_plan(be.lib, d)[3])
        return conv_wgrad(P, Q, grad, k, step, pad, pad_mode, *a, **kw)
    be.conv_forward, be.conv_wgrad = spy_conv, spy_wgrad
    try:
        prec = E.Precision.get(precname)
        tape = E.Tape()
        ctx = E.Ctx(prec, tape, training=True)
        x = seeded_uniform(shape, 6)
        xa = E.to_engine(x.to(DEV), prec)
        xa.needs_grad = True
        for p in net.parameters():
            p.grad = torch.zeros_like(p)
        ya = net.run(ctx, xa)
        y = E.from_engine(ya)
        r = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
        ya.grad = E.to_engine(r.to(DEV), prec).t
        tape.backward()
        torch.cuda.synchronize()
    finally:
        del be.conv_forward, be.conv_wgrad
    print('kernels of the replicate launches:', seen)
    assert seen['conv'] == [RC.W4] * 4, seen
    assert seen['wgrad'] == [RC.W4W] * 4, seen
    sdo = {k: v.clone() for k, v in sd.items()}
    params = {k: v.requires_grad_(True) for k, v in sdo.items() if v.is_floating_point()}
    xo = x.clone().requires_grad_(True)
    yo = O.run_generator(arch, sdo, xo, norm, 'replicate')
    grads = torch.autograd.grad((yo * r).sum(), [xo] + list(params.values()))
    assert TGN.rel(y, yo) < TGN.TOL_OUT[precname]
    with torch.no_grad():
        assert TGN.rel(_mirrored_blocks(arch, sd, x, norm), yo) > TGN.TOL_OUT[precname]          # teeth: a mirrored border would miss by more than the tolerance
    # gradients: the floor of tests/test_gpu_networks.py for this policy, or four times the oracle's own sensitivity to rounding noise of its size
    s_dx = s_dw = 0.0
    dw_oracle = torch.cat([g.reshape(-1) for g in grads[1:]])
    for seed in range(1, 9):          # eight draws below 256 x 256, as tests/test_gpu_networks.py (the sensitivity is quantised by single ReLU mask flips)
        with TGN.conv_noise(TGN.LAYER_NOISE[precname], seed):
            yn = O.run_generator(arch, sdo, xo, norm, 'replicate')
        gn = torch.autograd.grad((yn * r).sum(), [xo] + list(params.values()))
        s_dx = max(s_dx, TGN.l2(gn[0], grads[0]))
        s_dw = max(s_dw, TGN.l2(torch.cat([g.reshape(-1) for g in gn[1:]]), dw_oracle))
    named = dict(net.named_parameters())
    dw_engine = torch.cat([named[k].grad.reshape(-1).cpu() for k in params])
    e_dx, e_dw = TGN.l2(E.from_engine(E.Act(xa.grad, xa.C)), grads[0]), TGN.l2(dw_engine, dw_oracle)
    print(f'ngf 64 replicate blocks: y {TGN.rel(y, yo):.3e}, dx {e_dx:.3e} (oracle sensitivity {s_dx:.3e}), dw {e_dw:.3e} (oracle sensitivity {s_dw:.3e})')
    assert e_dx <= max(TGN.GRAD_FLOOR[precname], 4 * s_dx), (e_dx, s_dx)
    assert e_dw <= max(TGN.GRAD_FLOOR[precname], 4 * s_dw), (e_dw, s_dw)


@pytest.mark.parametrize('norm', ['batch', 'spectral'])
@pytest.mark.parametrize('precname', ['fp32', 'bf16'])
def test_one_training_step_against_the_oracle_model(precname, norm):
    """one optimize_parameters() of DeepLIIF (2 modalities + seg, ngf 8, 64 x 64, batch 2) with opt.padding = 'replicate' against OracleDeepLIIF(padding='replicate')
    from the same weights: losses, images and -- fp32 -- updated parameters at the tolerances of the step fixtures' first step.  'spectral': replicate padding
    together with --norm spectral only has to construct and run a finite step (no oracle restatement of the parametrization is involved here)"""
    opt = TGN.make_opt(2, True, norm, 'unet_64', 8, precname)
    opt.padding = 'replicate'
    torch.manual_seed(3)
    model = M.create_model(opt)
    model.setup(opt)
    A = seeded_uniform((2, 3, 64, 64), 22)
    B = [seeded_uniform((2, 3, 64, 64), 23 + i) for i in range(3)]
    if norm == 'spectral':
        model.set_input({'A': A, 'B': B, 'A_paths': ['x']})
        model.optimize_parameters()
        assert all(v == v and abs(v) < 1e4 for v in model.get_current_losses().values())
        return
    cfg = O.OracleConfig(modalities_no=2, seg_gen=True, net_g='resnet_9blocks', net_gs='unet_64', norm=norm, padding='replicate', ngf=8, ndf=8)
    S = str(model.mod_id_seg)
    g_names, gs_names, d_names, ds_names = cfg.names('S')
    nets = {}
    for j, name in enumerate(g_names + gs_names + d_names + ds_names):
        if name.startswith('D'):
            arch, pad, cin = 'n_layers', 'zero', 6
        elif name in g_names:
            arch, pad, cin = 'resnet_9blocks', 'replicate', 3
        else:
            arch, pad, cin = 'unet_64', 'reflect', 3
        nets[name] = O.random_state_dict(arch, cin, 3, 8, norm, pad, 4, generator=torch.Generator().manual_seed(2300 + j))
        mine = name.replace('S', S, 1) if len(name) > 2 else name
        getattr(model, 'net' + mine).load_state_dict({k: v.clone() for k, v in nets[name].items()})
    om = O.OracleDeepLIIF(cfg, nets)
    om.set_input({'A': A, 'B': B})
    om.optimize_parameters()
    exp = om.current_losses()
    model.set_input({'A': A, 'B': B, 'A_paths': ['x']})
    model.optimize_parameters()
    got = model.get_current_losses()
    ltol = {'fp32': 1e-3, 'bf16': 3e-2}[precname]
    otol = {'fp32': 1e-3, 'bf16': 6e-2}[precname]
    assert len(exp) == len(got)
    for name, e in exp.items():
        mine = name[:-1] + S if name.endswith('_S') else name
        err = abs(got[mine] - e) / max(abs(e), TGN.LOSS_FLOOR)
        assert err <= ltol, (name, got[mine], e)
    for i in range(2):
        assert TGN.rel(getattr(model, f'fake_B_{i + 1}'), om.fake_B[i]) < otol
    assert TGN.rel(getattr(model, f'fake_B_{S}'), om.fake_seg) < otol
    if precname == 'fp32':
        for name, sd in nets.items():
            mine = name.replace('S', S, 1) if len(name) > 2 else name
            mysd = getattr(model, 'net' + mine).state_dict()
            a = torch.cat([mysd[k].reshape(-1).float().cpu() for k, v in sd.items() if v.is_floating_point()])
            b = torch.cat([v.detach().reshape(-1).float() for v in sd.values() if v.is_floating_point()])
            # as the step fixtures: 8e-3 of |w| = 80 % of one Adam update's norm -- a wrong update direction / learning rate is >= 100 %
            assert float((a - b).norm() / b.norm()) < 8e-3, name


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_served_model_directory_with_replicate_padding(tmp_path, precision):
    """init_nets on a directory whose train_opt.txt says `padding: replicate`: the translation generators are replicate-padded and follow the oracle forward on both
    16-bit policies (bounds: tests/test_gpu_networks.TOL_OUT for bf16, the fixture-size bound of tests/test_gpu_fp16.py for fp16)"""
    from deepliif_amd import inference as I
    I._NETS_CACHE.clear()
    mdir = build_replicate_dir(tmp_path)
    opt = I.get_opt(mdir)
    assert opt.padding == 'replicate'
    opt.ngf, opt.precision, opt.gpu_ids = 8, precision, [0]
    nets = I.init_nets(mdir, eager_mode=True, opt=opt)
    assert list(nets) == ['G1', 'G2', 'GS0', 'GS1', 'GS2']
    assert nets['G1'].padding_type == 'replicate' and isinstance(nets['G1'].model[10].conv_block[0], torch.nn.ReplicationPad2d)
    x = seeded_uniform((2, 3, 64, 64), 32)
    tol = {'bf16': TGN.TOL_OUT['bf16'], 'fp16': 1e-2}[precision]
    for name in ('G1', 'G2'):
        sd = torch.load(f'{mdir}/latest_net_{name}.pth', map_location='cpu')
        with torch.no_grad():
            got = nets[name](x.to(DEV)).float().cpu()
            # served nets normalise every tile with its own statistics (the reference runs one tile per call): the oracle sees the tiles one by one
            exp = torch.cat([O.run_generator('resnet_9blocks', sd, x[i:i + 1], 'batch', 'replicate') for i in range(x.shape[0])])
            other = torch.cat([O.run_generator('resnet_9blocks', sd, x[i:i + 1], 'batch', 'reflect') for i in range(x.shape[0])])
        e = TGN.rel(got, exp)
        print(f'served {name} {precision}: {e:.3e} (reflect oracle would be {TGN.rel(got, other):.3e})')
        assert e < tol, (name, e)
        assert TGN.rel(got, other) > 2 * tol, (name, TGN.rel(got, other))          # teeth: the mirrored-border oracle is far outside the tolerance
    I._NETS_CACHE.clear()
