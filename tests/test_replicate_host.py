"""Replicate padding (`--padding replicate`: nn.ReplicationPad2d(1) in front of both ResnetBlock convs, networks.py:482-483 / 499-500) on the host: the float64
reference of the GPU tests against a hand-written clamp loop, the fold formula against autograd, the module tree against key lists recorded from the
reference, the routing and the status codes of the library (it loads without a GPU; nothing here launches anything), the oracle against a fixture the
reference produced, and `serialize` of a replicate net."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pad_ref as PR
import replicate_cases as RC
from replicate_cases import build_replicate_dir
from deepliif_amd import _lib as L
from deepliif_amd import networks as N
from oracle import deepliif_oracle as O

G = os.path.join(os.path.dirname(__file__), 'golden')
Z = np.load(os.path.join(G, 'resnet_replicate.npz'))
RTOL = 1e-4                 # tests/test_oracle_golden.py: fp32 oracle against the reference on the same torch build


def rnd16(shape, seed, dtype=torch.bfloat16, scale=1.0):
    """N(0, scale) values that are exactly representable in the 16-bit format"""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).float()


# ------------------------------------------------------------------------------------------------ the reference of the GPU tests
def test_pad_ref_against_an_index_clamp_loop():
    n, h, w, c, co = 1, 3, 4, 2, 3
    x = rnd16((n, h, w, 8), 1)
    x[..., c:] = 0
    wt = rnd16((co, c, 3, 3), 2)
    bias = rnd16((co,), 3)
    ref, S, K = PR.forward(x, wt, bias, relu=False)
    assert K == 9 * c + 1 and ref.shape == (n, h, w, 8)
    for i in range(h):
        for j in range(w):
            for o in range(co):
                acc, mag = float(bias[o]), abs(float(bias[o]))
                for kh in range(3):
                    for kw in range(3):
                        ii, jj = min(max(i + kh - 1, 0), h - 1), min(max(j + kw - 1, 0), w - 1)
                        for ci in range(c):
                            p = float(x[0, ii, jj, ci]) * float(wt[o, ci, kh, kw])
                            acc += p
                            mag += abs(p)
                assert abs(float(ref[0, i, j, o]) - acc) < 1e-12 and abs(float(S[0, i, j, o]) - mag) < 1e-12
    assert float(ref[..., co:].abs().max()) == 0.0
    # the gradients are autograd's on that expression: <dy, conv(x)> is linear in x and in w, so the inner products must agree
    dy = rnd16((n, h, w, 8), 4)
    dy[..., co:] = 0
    dx, _, Kd = PR.dgrad(dy, wt, (h, w))
    dw, _, Kw = PR.wgrad(dy, x, co, c)
    lhs = float((dy.double() * PR.forward(x, wt)[0]).sum())
    assert abs(float((dx[..., :c] * x[..., :c].double()).sum()) - lhs) < 1e-9 and abs(float((dw * wt.double()).sum()) - lhs) < 1e-9
    assert float(Kd.min()) == float(Kd.max()) == 9 * co and Kw == n * h * w          # every input pixel is read nine times per output channel, borders included


def fold_formula(src, pad):
    """dl_replicate_fold restated (csrc/elementwise.hip replicate_fold_kernel): NHWC, padded rows 0 .. pad onto row 0, H-1+pad .. H-1+2 pad onto row H-1"""
    n, hp, wp, c = src.shape
    h, w = hp - 2 * pad, wp - 2 * pad
    dst = torch.zeros(n, h, w, c, dtype=src.dtype)
    for i in range(h):
        lo_i, hi_i = (0 if i == 0 else i + pad), (hp - 1 if i == h - 1 else i + pad)
        for j in range(w):
            lo_j, hi_j = (0 if j == 0 else j + pad), (wp - 1 if j == w - 1 else j + pad)
            dst[:, i, j] = src[:, lo_i:hi_i + 1, lo_j:hi_j + 1].sum(dim=(1, 2))
    return dst


@pytest.mark.parametrize('shape,pad', [((1, 1, 1, 8), 1), ((2, 3, 5, 16), 1), ((1, 4, 4, 8), 3), ((1, 2, 7, 8), 2)])
def test_fold_formula_is_the_backward_of_replication_pad(shape, pad):
    n, h, w, c = shape
    src = torch.randn(n, h + 2 * pad, w + 2 * pad, c, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    x = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
    exp = torch.autograd.grad(F.pad(x, (pad,) * 4, mode='replicate'), x, src.permute(0, 3, 1, 2))[0].permute(0, 2, 3, 1)
    assert float((fold_formula(src, pad) - exp).abs().max()) < 1e-12


def teeth_fraction(ref_other, ref, bnd, h, w):
    """share of the border-row / border-column elements at which another mode's reference misses the replicate reference by more than the bound"""
    m = PR.border_mask(h, w)[None, :, :, None]
    miss = ((ref_other - ref).abs() > bnd) & m
    return float(miss.sum()) / float(m.expand_as(ref).sum())


@pytest.mark.parametrize('n,h,w,cin,cout', [(1, 2, 128, 64, 256), (2, 4, 128, 128, 256), (2, 40, 24, 32, 32), (1, 1, 5, 8, 8)])
def test_bound_separates_the_three_padding_modes(n, h, w, cin, cout):
    """the teeth of the GPU tests: with their N(0, 1) inputs a kernel that padded with zeros or mirrored instead of clamping would be caught at >= 90 % of
    the border elements (reflect needs two pixels per axis: not defined for the H = 1 case, where zero padding alone is tested)"""
    x, wt = rnd16((n, h, w, cin), 11), rnd16((cout, cin, 3, 3), 12, scale=0.05)
    ref, S, K = PR.forward(x, wt)
    bnd = PR.bound(ref, S, K, torch.bfloat16)
    for mode in ('zero', 'reflect'):
        if mode == 'reflect' and min(h, w) < 2:
            continue
        other = PR.forward(x, wt, mode=mode)[0]
        assert teeth_fraction(other, ref, bnd, h, w) >= 0.9, mode
        inner = ~PR.border_mask(h, w)
        assert float((other - ref)[:, inner].abs().max() if inner.any() else 0.0) == 0.0          # ... and the modes agree everywhere else


# ------------------------------------------------------------------------------------------------ module tree
@pytest.mark.parametrize('norm', ['batch', 'instance', 'spectral'])
@pytest.mark.parametrize('dropout', [False, True])
def test_state_dict_keys_equal_the_references(norm, dropout):
    torch.manual_seed(1)
    net = N.define_G(3, 3, 8, 'resnet_2blocks', norm, dropout, 'normal', 0.02, [], 'replicate')
    tag = norm + ('_dropout' if dropout else '')
    sd = net.state_dict()
    assert list(sd.keys()) == Z[f'keys/{tag}'].tolist()
    assert [str(tuple(v.shape)) for v in sd.values()] == Z[f'shapes/{tag}'].tolist()
    blk = net.model[10]
    pads = [i for i, m in enumerate(blk.conv_block) if isinstance(m, torch.nn.ReplicationPad2d)]
    assert pads == ([0, 5] if dropout else [0, 4]) and all(blk.conv_block[i].padding == (1, 1, 1, 1) for i in pads)
    assert isinstance(net.model[0], torch.nn.ZeroPad2d) and isinstance(net.model[-3], torch.nn.ZeroPad2d)       # stem / head: zero for anything but reflect
    b = net._bind()
    assert b['stem'][0].spec.pad_mode == L.PAD_ZERO and b['head'].spec.pad_mode == L.PAD_ZERO
    assert all(c.spec.pad_mode == L.PAD_REPLICATE for ent, _ in b['blocks'] for c, _ in ent)


def test_unknown_padding_is_still_refused():
    with pytest.raises(NotImplementedError, match='padding'):
        N.define_G(3, 3, 8, 'resnet_2blocks', 'batch', False, 'normal', 0.02, [], 'circular')


# ------------------------------------------------------------------------------------------------ the oracle against the reference's fixture
@pytest.mark.parametrize('norm', ['batch', 'instance'])
def test_oracle_reproduces_the_reference_fixture(norm):
    sd = {k[len(f'{norm}/sd/'):]: torch.from_numpy(Z[k].astype(np.float32) if Z[k].dtype == np.float16 else Z[k]) for k in Z.files if k.startswith(f'{norm}/sd/')}
    params = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and 'running' not in k}
    x = torch.from_numpy(Z[f'{norm}/x']).requires_grad_(True)
    y = O.run_generator('resnet_2blocks', sd, x, norm, 'replicate')
    rel = lambda a, b, floor=1e-30: float((a.double() - torch.as_tensor(b).double()).abs().max() / torch.as_tensor(b).double().abs().max().clamp_min(floor))
    assert rel(y.detach(), Z[f'{norm}/y']) < RTOL
    grads = torch.autograd.grad(y.square().mean(), [x] + list(params.values()))
    assert rel(grads[0], Z[f'{norm}/dx']) < RTOL
    gscale = max(float(g.abs().max()) for g in grads[1:])
    for (k, _), g in zip(params.items(), grads[1:]):
        assert rel(g, Z[f'{norm}/dw/{k}'], floor=0.05 * gscale) < 5 * RTOL, k
    # the fixture is about the border: mirroring in the blocks (same keys, another border) misses it by far more than the tolerance.  ('reflect' would
    # also mirror stem and head, where 'replicate' pads with zeros: the blocks alone are swapped here)
    with torch.no_grad():
        orig = O._pad
        O._pad = lambda t, p, mode: orig(t, p, 'reflect' if (mode == 'replicate' and p == 1) else mode)
        try:
            assert rel(O.run_generator('resnet_2blocks', sd, x.detach(), norm, 'replicate'), Z[f'{norm}/y']) > 100 * RTOL
        finally:
            O._pad = orig


# ------------------------------------------------------------------------------------------------ routing
W4_FWD = [(1, 2, 128, 64, 256), (2, 4, 128, 128, 256), (1, 6, 128, 64, 512), (8, 128, 128, 256, 256)]


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
def test_replicate_routes_to_the_w4_kernels_exactly_on_their_shapes(half):
    lib = L.load(half)
    for n, h, w, ci, co in W4_FWD:
        d = RC.conv_desc('replicate', n, h, w, ci, co)
        assert RC.conv_name(lib, d) == RC.W4, (n, h, w, ci, co)
        assert lib.dl_conv_add_supported(C.byref(d)) == 0                       # the fused addend belongs to the zero-padding data gradient
        assert lib.dl_conv_stats_chunks(C.byref(d)) == h * w // 256             # one chunk per 256-pixel tile, as the kernel writes them
    for why, args in (('W = 64', (2, 8, 64, 64, 256)), ('Ci = 32', (1, 8, 128, 32, 256)), ('odd Hq', (1, 3, 128, 64, 256)), ('Co = 128', (1, 2, 128, 64, 128)),
                      ('strict', (1, 2, 128, 64, 256, 3, 'strict')), ('data gradient', (8, 128, 128, 256, 256, 3, 'bf16', 'dgrad')),
                      ('ReLU + tanh only none / ReLU', (1, 2, 128, 64, 256, 3, 'bf16', 'fwd', L.ACT_TANH)), ('split-K', (1, 2, 128, 64, 256, 3, 'bf16', 'fwd', L.ACT_NONE, 0, 2))):
        assert RC.conv_name(lib, RC.conv_desc('replicate', *args)) != RC.W4, why
    assert RC.conv_name(lib, RC.conv_desc('replicate', 1, 2, 128, 64, 256, act=L.ACT_RELU, bias_n=256)) == RC.W4
    for n, h, w, ca, cb in [(1, 2, 128, 128, 128), (2, 3, 128, 256, 128), (8, 128, 128, 256, 256)]:
        rc, tiles, ksteps, name = RC.wgrad_plan(lib, RC.wgrad_desc('replicate', n, h, w, ca, cb))
        assert (rc, name, tiles, ksteps) == (1, RC.W4W, (ca // 128) * (cb // 128) * 3, n * h), (n, h, w, ca, cb)
    assert RC.wgrad_plan(lib, RC.wgrad_desc('replicate', 2, 3, 128, 256, 128, p_pstride=384, q_pstride=192))[3] == RC.W4W
    for why, args in (('W = 64', (2, 8, 64, 128, 128)), ('CB = 32', (1, 8, 128, 128, 32)), ('CA = 64', (1, 8, 128, 64, 128)), ('H = 1', (2, 1, 128, 128, 128)),
                      ('strict', (1, 2, 128, 128, 128, 3, 'strict')), ('5 x 5', (1, 8, 128, 128, 128, 5))):
        assert RC.wgrad_plan(lib, RC.wgrad_desc('replicate', *args))[3] != RC.W4W, why


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
def test_zero_and_reflect_routing_is_where_it_was(half):
    lib = L.load(half)
    assert len(RC.UNCHANGED) >= 20
    for entry, want in RC.UNCHANGED:
        assert RC.routed(lib, entry) == want, entry


# ------------------------------------------------------------------------------------------------ status codes
def test_bad_padding_modes_are_refused_before_any_launch():
    lib = L.load()
    p = C.c_void_p(0x1000)                  # never dereferenced: every check below fails on the host
    d = RC.conv_desc('zero', 1, 2, 128, 64, 256)
    d.pad_mode = 3
    assert lib.dl_conv_forward(C.byref(d), p, p, None, None, p, None, None, None) != 0 and b'pad_mode=3' in lib.dl_last_error()
    d.pad_mode = -1
    assert lib.dl_conv_forward(C.byref(d), p, p, None, None, p, None, None, None) != 0
    # replicate on a four-phase plan (a stride-2 data gradient) and on a strided input walk
    from deepliif_amd.geometry import ConvSpec, cpad, fill_conv_desc
    plan = ConvSpec('conv', 64, 128, 3, 2, 1).dgrad_plan()
    d4 = fill_conv_desc(plan, 1, 8, 8, 128, 16, 16, 64, 64, 8, 8, L.DL_BF16, L.PREC_BF16, L.ACT_NONE, L.ACT_NONE, 0, 1)
    assert d4.n_phase == 4
    d4.pad_mode = L.PAD_REPLICATE
    assert lib.dl_conv_forward(C.byref(d4), p, p, None, None, p, None, None, None) != 0 and b'replicate padding only' in lib.dl_last_error()
    d2 = fill_conv_desc(ConvSpec('conv', 64, 128, 3, 2, 1).forward_plan(), 1, 16, 16, 64, 8, 8, 128, 128, 8, 8, L.DL_BF16, L.PREC_BF16, L.ACT_NONE, L.ACT_NONE, 0, 1)
    d2.pad_mode = L.PAD_REPLICATE
    assert d2.in_step == 2 and lib.dl_conv_forward(C.byref(d2), p, p, None, None, p, None, None, None) != 0 and b'replicate padding only' in lib.dl_last_error()
    w = RC.wgrad_desc('zero', 1, 2, 128, 128, 128)
    w.pad_mode = 3
    assert lib.dl_conv_wgrad(C.byref(w), p, p, p, p, None) != 0 and b'pad_mode=3' in lib.dl_last_error()
    w.pad_mode, w.step = L.PAD_REPLICATE, 2
    assert lib.dl_conv_wgrad(C.byref(w), p, p, p, p, None) != 0 and b'replicate padding only' in lib.dl_last_error()
    f = lib.dl_replicate_fold
    assert f(L.DL_BF16, None, 8, p, 8, 1, 4, 4, 1, 8, None) != 0 and f(L.DL_BF16, p, 8, None, 8, 1, 4, 4, 1, 8, None) != 0
    assert b'dl_replicate_fold' in lib.dl_last_error()
    assert f(L.DL_BF16, p, 8, p, 8, 1, 4, 4, 1, 12, None) != 0                      # Cp % 8
    assert f(L.DL_BF16, p, 8, p, 8, 1, 4, 4, 0, 8, None) != 0 and b'pad=0' in lib.dl_last_error()
    assert f(L.DL_BF16, p, 8, p, 8, 0, 4, 4, 1, 8, None) != 0 and b'empty problem' in lib.dl_last_error()
    assert f(7, p, 8, p, 8, 1, 4, 4, 1, 8, None) != 0 and b'dtype' in lib.dl_last_error()


# ------------------------------------------------------------------------------------------------ serialize
def test_serialize_of_a_replicate_model_directory(tmp_path, monkeypatch):
    """train_opt.txt with `padding: replicate` -> init_nets builds replicate ResnetGenerators, serialize writes stock TorchScript files with the reference's keys
    whose forward pads by replication (the plain-torch twin carries the ReplicationPad2d modules), equal to the oracle"""
    import shutil
    import fake_backend
    from deepliif_amd import export as X
    from deepliif_amd import inference as I
    fake_backend.install()
    try:
        monkeypatch.setattr(I, '_device_for', lambda opt: torch.device('cpu'))
        I._NETS_CACHE.clear()
        mdir = build_replicate_dir(tmp_path)
        opt = I.get_opt(mdir)
        assert opt.padding == 'replicate'
        opt.ngf, opt.precision = 8, 'fp32'
        sdir = str(tmp_path / 'serialized')
        report = X.serialize(mdir, sdir, device='cpu', opt=opt)
        assert sorted(report) == ['G1', 'G2', 'GS0', 'GS1', 'GS2'] and max(report.values()) <= 1e-3
        for name in ('G1', 'G2'):
            ts = torch.jit.load(os.path.join(sdir, f'{name}.pt'), map_location='cpu')
            sd = torch.load(os.path.join(mdir, f'latest_net_{name}.pth'), map_location='cpu')
            assert list(ts.state_dict().keys()) == [k for k in sd if k.rsplit('.', 1)[-1] not in ('running_mean', 'running_var')]
            assert 'replicat' in str(ts.inlined_graph)                  # aten::replication_pad2d
            x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(9)) * 2 - 1
            with torch.no_grad():
                got = ts(x.clone())
                assert float((got - O.run_generator('resnet_9blocks', sd, x.clone(), 'batch', 'replicate')).abs().max()) < 1e-5
                assert float((got - O.run_generator('resnet_9blocks', sd, x.clone(), 'batch', 'reflect')).abs().max()) > 1e-4        # (same keys, another border)
    finally:
        fake_backend.uninstall()
        I._NETS_CACHE.clear()
