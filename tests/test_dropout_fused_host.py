"""Host side of the dropout that the norm kernels apply in registers (engine.norm_act(dropout=...), engine.DropoutSeeds, the dl_dropout_desc
binding), on CPU: routing through an emulated backend that takes the `dropout=` argument, the seed arithmetic of the device-seed route against the
eager sequence, the staging ring's event discipline, and the C ABI of the three new entries."""
import ctypes
import os
import subprocess

import pytest
import torch

import fake_backend
from deepliif_amd import _lib as L
from deepliif_amd import engine as E
from deepliif_amd import networks as N
from deepliif_amd import ops
from golden_util import seeded_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'deepliif_hip.h')


class FusedFake(fake_backend.FakeBackend):
    """FakeBackend plus the fused interface of ops.HipBackend: the mask of a site is the one FakeBackend.dropout draws for the site's effective seed
    (over the DENSE shape, so a channel-slice output gets the same one)."""
    supports_fused_dropout = True

    @staticmethod
    def _keep(shape, dropout):
        p, seed, seed_dev, call_index = dropout
        s = ((int(seed_dev[0]) if seed_dev is not None else int(seed)) + call_index) & (2 ** 63 - 1)
        g = torch.Generator().manual_seed(s % (2 ** 63))
        return (torch.rand(shape, generator=g) >= p).float() / (1.0 - p)

    def norm_forward(self, y, z, *a, dropout=None, **kw):
        stats = super().norm_forward(y, z, *a, **kw)
        if dropout is not None:
            self._count('fused_fwd')
            z.copy_((z.float() * self._keep(z.shape, dropout)).to(z.dtype))
        return stats

    def norm_backward(self, dz, *a, dropout=None, **kw):
        if dropout is not None:
            self._count('fused_bwd')
            dz = (dz.float() * self._keep(dz.shape, dropout)).to(dz.dtype)
        return super().norm_backward(dz, *a, **kw)

    def dropout_dev(self, x, y, dropout):
        self._count('dropout_dev')
        y.copy_((x.float() * self._keep(x.shape, dropout)).to(y.dtype))


# (arch, input size).  unet_32 has no ngf*8 block between its innermost and its ngf*4 block, hence no Dropout module at all: it pins "nothing changes";
# unet_64 is the smallest UNet with a dropout site (its one ngf*8 block)
NETS = [('resnet_2blocks', 32), ('unet_32', 32), ('unet_64', 64)]


def _run(backend, arch, size, train, seed=11):
    """one forward + backward of a use_dropout=True generator on `backend`: (output, {parameter: gradient}, call counts)"""
    ops._impl = backend
    try:
        torch.manual_seed(seed)
        E._DROPOUT_COUNTER[0] = 0
        net = N.define_G(3, 3, 8, arch, 'batch', True, 'normal', 0.02, [], 'zero')
        net.train(train)
        prec = E.Precision.get('fp32')
        tape = E.Tape()
        ctx = E.Ctx(prec, tape, training=train)
        xa = E.to_engine(seeded_uniform((2, 3, size, size), 6), prec)
        xa.needs_grad = True
        for p in net.parameters():
            p.grad = torch.zeros_like(p)
        ya = net.run(ctx, xa)
        ya.grad = E.to_engine(torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(7)), prec).t
        tape.backward()
        return E.from_engine(ya), {k: p.grad.clone() for k, p in net.named_parameters()}, dict(backend.calls), E._DROPOUT_COUNTER[0]
    finally:
        ops._impl = None


@pytest.mark.parametrize('arch,size', NETS)
def test_fused_route_makes_no_dropout_call_and_changes_nothing(arch, size):
    y0, g0, c0, n0 = _run(fake_backend.FakeBackend(), arch, size, True)
    y1, g1, c1, n1 = _run(FusedFake(), arch, size, True)
    sites = {'resnet_2blocks': 2, 'unet_32': 0, 'unet_64': 1}[arch]
    assert n0 == n1 == sites                                        # one tick of the seed sequence per site on either route
    assert c0.get('dropout', 0) == 2 * sites                        # the plain backend: a pass over the activation and one over its gradient
    assert c1.get('dropout', 0) == 0 and c1.get('dropout_dev', 0) == 0
    assert c1.get('fused_fwd', 0) == sites and c1.get('fused_bwd', 0) == sites
    assert c1['norm_fwd'] == c0['norm_fwd'] and c1['norm_bwd'] == c0['norm_bwd']
    # the UNet's placement copy (one axpby per site on the three-pass route) is gone; no other axpby appears or disappears
    assert c0.get('axpby', 0) - c1.get('axpby', 0) == (sites if arch.startswith('unet') else 0)
    assert torch.equal(y0, y1)
    assert g0.keys() == g1.keys()
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    if sites:
        assert any(float(v.abs().max()) > 0 for v in g0.values())


@pytest.mark.parametrize('arch,size', NETS)
def test_eval_mode_is_untouched(arch, size):
    y0, g0, c0, n0 = _run(fake_backend.FakeBackend(), arch, size, False)
    y1, g1, c1, n1 = _run(FusedFake(), arch, size, False)
    assert n0 == n1 == 0
    assert c0 == c1 and 'dropout' not in c1 and 'fused_fwd' not in c1
    assert torch.equal(y0, y1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_a_backend_without_the_attribute_keeps_the_two_pass_route():
    """engine.norm_act(dropout=p) on the plain emulation: norm_act followed by dropout(), the same seed as a direct call"""
    ops._impl = fb = fake_backend.FakeBackend()
    try:
        outs = []
        for fused_arg in (True, False):
            torch.manual_seed(4)
            E._DROPOUT_COUNTER[0] = 0
            ctx = E.Ctx(E.Precision.get('fp32'), None, training=True)
            y = E.Act(seeded_uniform((1, 6, 5, 8), 3), 8, False)
            norm = E.NormLayer('instance', 8, None)
            if fused_arg:
                z = E.norm_act(ctx, y, norm, L.ACT_RELU, dropout=0.5)
            else:
                z = E.dropout(ctx, E.norm_act(ctx, y, norm, L.ACT_RELU), 0.5)
            outs.append(z.t.clone())
            assert E._DROPOUT_COUNTER[0] == 1
        assert torch.equal(outs[0], outs[1])
        assert fb.calls['dropout'] == 2
    finally:
        ops._impl = None


class _Event:
    """stands in for torch.cuda.Event: remembers the order of record / synchronize calls"""
    log = []

    def __init__(self):
        self.id = len([e for e in _Event.log if e[0] == 'new'])
        _Event.log.append(('new', self.id))

    def record(self):
        _Event.log.append(('record', self.id))

    def synchronize(self):
        _Event.log.append(('sync', self.id))


def _eager_seeds(n):
    """the seeds n consecutive eager dropout sites draw"""
    return [E._dropout_site(0.5)[1] for _ in range(n)]


def test_device_seeds_walk_the_eager_sequence(monkeypatch):
    monkeypatch.setattr(E, '_rank', lambda: 3)
    torch.manual_seed(1234)
    E._DROPOUT_COUNTER[0] = 5
    per_step = [4, 4, 7]
    want = [_eager_seeds(j) for j in per_step]
    assert len({s for w in want for s in w}) == sum(per_step)
    assert want[0][0] == (1234 * 1000003 + 7919 * 3 + 6) & (2 ** 63 - 1)
    E._DROPOUT_COUNTER[0] = 5
    ds = E.DropoutSeeds('cpu')
    for step, j in enumerate(per_step):
        ds.begin_step()
        base = int(ds.dev[0])
        assert base == (1234 * 1000003 + 7919 * 3 + E._DROPOUT_COUNTER[0]) & (2 ** 63 - 1)
        got = []
        for _ in range(j):
            p, seed, seed_dev, idx = E._dropout_site(0.5)
            assert seed_dev is ds.dev and p == 0.5
            got.append((int(seed_dev[0]) + idx) & (2 ** 63 - 1))
        assert [g - base for g in got] == list(range(1, j + 1))
        assert ds.end_step() == j
        assert got == want[step]
    assert E._DROPOUT_COUNTER[0] == 5 + sum(per_step)
    assert E._DEVICE_SEEDS[0] is None
    # a replay of a captured step with J sites: the same base, the same advance
    E._DROPOUT_COUNTER[0] = 5
    for step, j in enumerate(per_step):
        ds.replay_step(j)
        assert [(int(ds.dev[0]) + i) & (2 ** 63 - 1) for i in range(1, j + 1)] == want[step]
    # eager sites after a device-seed step continue the sequence
    assert _eager_seeds(1)[0] == (1234 * 1000003 + 7919 * 3 + 5 + sum(per_step) + 1) & (2 ** 63 - 1)


def test_base_plus_index_wraps_like_the_eager_mask(monkeypatch):
    """the eager seed is (a + k) mod 2^63; base = (a + k0) mod 2^63 and the kernel's (base + j) mod 2^63 must agree across the wrap"""
    monkeypatch.setattr(E, '_seed_base', lambda: 2 ** 63 - 3)
    E._DROPOUT_COUNTER[0] = 0
    want = _eager_seeds(6)
    assert want == [2 ** 63 - 2, 2 ** 63 - 1, 0, 1, 2, 3]
    E._DROPOUT_COUNTER[0] = 0
    ds = E.DropoutSeeds('cpu')
    ds.begin_step()
    got = [(int(ds.dev[0]) + E._dropout_site(0.5)[3]) & (2 ** 63 - 1) for _ in range(6)]
    ds.end_step()
    assert got == want


def test_cancelled_step_rewinds_the_sequence():
    torch.manual_seed(9)
    E._DROPOUT_COUNTER[0] = 40
    want = _eager_seeds(3)
    E._DROPOUT_COUNTER[0] = 40
    ds = E.DropoutSeeds('cpu')
    ds.begin_step()
    for _ in range(3):
        E._dropout_site(0.5)
    ds.cancel_step()                              # a failed capture: none of these launches ran
    assert E._DROPOUT_COUNTER[0] == 40 and E._DEVICE_SEEDS[0] is None and ds.index == 0
    assert _eager_seeds(3) == want                # the eager re-run of the step draws the seeds the cancelled pass would have
    with pytest.raises(AssertionError):
        ds.end_step()                             # nothing is open
    ds.begin_step()
    with pytest.raises(AssertionError):
        E.DropoutSeeds('cpu').begin_step()        # one open step at a time
    ds.cancel_step()


def test_staging_ring_waits_for_a_slot_before_reusing_it():
    _Event.log = []
    E._DROPOUT_COUNTER[0] = 0
    ds = E.DropoutSeeds('cpu', ring=3, event_factory=_Event)
    assert [e for e in _Event.log] == [('new', 0), ('new', 1), ('new', 2)]
    hosts = [h for h, _ in ds._ring]
    assert len({h.data_ptr() for h in hosts}) == 3
    _Event.log = []
    staged = []
    for step in range(7):
        E._DROPOUT_COUNTER[0] = 10 * step
        staged.append(ds.stage())
        assert int(hosts[step % 3][0]) == staged[-1] == int(ds.dev[0])
    # the first pass over the ring only records; from then on slot k is synchronised BEFORE it is rewritten and recorded again
    assert _Event.log == [('record', 0), ('record', 1), ('record', 2),
                          ('sync', 0), ('record', 0), ('sync', 1), ('record', 1), ('sync', 2), ('record', 2), ('sync', 0), ('record', 0)]
    assert len(set(staged)) == 7


def test_ctypes_dropout_desc_matches_the_header(tmp_path):
    c = tmp_path / 'sz.hip'
    c.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(dl_dropout_desc), '
                 'offsetof(dl_dropout_desc, p), offsetof(dl_dropout_desc, seed), offsetof(dl_dropout_desc, seed_dev), '
                 'offsetof(dl_dropout_desc, call_index));return 0;}\n' % HEADER)
    exe = tmp_path / 'sz'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '--offload-arch=gfx950', str(c), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = L.DropoutDesc
    assert got == [ctypes.sizeof(D), D.p.offset, D.seed.offset, D.seed_dev.offset, D.call_index.offset]


@pytest.mark.parametrize('half', ['bf16', 'fp16'])
def test_both_libraries_export_the_three_entries(half):
    lib = L.load(half)
    for name in ('dl_norm_forward_dropout', 'dl_norm_backward_dropout', 'dl_dropout_dev'):
        assert hasattr(lib, name), f'{name} is missing from the {half} library'
        assert name in L.SIGNATURES
        assert getattr(lib, name).argtypes[-1 if name != 'dl_dropout_dev' else -2]._type_ is L.DropoutDesc
    assert ops.HipBackend.supports_fused_dropout is True


def test_dropout_arguments_are_checked_before_any_launch():
    """decided on the host before the device is touched (the pointers are never dereferenced): runs without a GPU"""
    lib = L.load()
    dummy = ctypes.c_void_p(0x1000)
    n = L.NormDesc()
    n.N, n.H, n.W, n.Cp, n.C, n.y_pstride, n.z_pstride, n.r_pstride, n.dtype = 1, 8, 8, 8, 8, 8, 8, 8, L.DL_BF16
    dd = L.DropoutDesc()
    dd.p, dd.seed = 0.5, 7
    fwd = lambda res, drop: lib.dl_norm_forward_dropout(ctypes.byref(n), dummy, None, None, None, None, dummy, dummy, dummy, dummy, res, dummy, dummy, None, None, drop)
    assert fwd(dummy, ctypes.byref(dd)) != 0 and b'residual' in lib.dl_last_error()
    assert fwd(None, None) != 0 and b'null dropout descriptor' in lib.dl_last_error()
    dd.p = 1.0
    assert fwd(None, ctypes.byref(dd)) != 0 and b'outside [0, 1)' in lib.dl_last_error()
    dd.p = 0.5
    n.ext_nchunks = 4
    rc = lib.dl_norm_backward_dropout(ctypes.byref(n), dummy, dummy, None, dummy, dummy, dummy, dummy, dummy, None, None, 1, None, dummy, None, None, ctypes.byref(dd))
    assert rc != 0 and b'ext_nchunks' in lib.dl_last_error()
    assert lib.dl_dropout_dev(L.DL_BF16, dummy, 8, dummy, 8, 64, 8, None, None) != 0 and b'dl_dropout_dev' in lib.dl_last_error()
