"""Helpers shared by the spectral-normalisation tests and tests/golden/make_golden_spectral.py.

fill_seeded           deterministic weights / biases / unit-length u, v for any net, walking state_dict() in order with ONE generator, so that an engine net
                      and a reference net with the same keys get the same numbers
SpectralFakeBackend   tests/fake_backend.FakeBackend plus the two spectral ops in plain torch (the formulas of
                      torch.nn.utils.parametrizations._SpectralNorm, evaluated in fp32), for the CPU suite
float64_twin / twin_forward   the deep-copied container tree of an engine net in float64 and torch's own forward of it: the reference of the parity tests
"""
import copy
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

import fake_backend
from deepliif_amd import ops


def fill_seeded(net, seed: int):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if not v.is_floating_point():
                continue
            r = torch.randn(v.shape, generator=g, dtype=torch.float32)
            if k.endswith('._u') or k.endswith('._v'):
                v.copy_(r / r.norm())
            elif k.endswith('bias'):
                v.copy_(0.02 * r)
            elif 'running_var' in k:
                v.copy_(1.0 + 0.1 * r.abs())
            else:
                v.copy_(0.05 * r)
    return net


def uv_digest(net) -> np.ndarray:
    """[sum, abs-sum] over every _u / _v buffer, in state_dict order"""
    out = []
    for k, v in net.state_dict().items():
        if k.endswith('._u') or k.endswith('._v'):
            out.append([float(v.double().sum()), float(v.double().abs().sum())])
    return np.array(out, dtype=np.float64).reshape(-1, 2)


def state_digest(net) -> np.ndarray:
    return np.array([[float(v.double().sum()), float(v.double().abs().sum())] for v in net.state_dict().values()], dtype=np.float64)


def keys_fingerprint(keys) -> str:
    return hashlib.sha256('\n'.join(keys).encode()).hexdigest()


def matrix_of(w: torch.Tensor, dim: int) -> torch.Tensor:
    """_SpectralNorm._reshape_weight_to_matrix"""
    if dim != 0:
        w = w.permute(dim, *(d for d in range(w.dim()) if d != dim))
    return w.flatten(1)


def spectral_forward_ref(w, dim, u, v, iterate: bool, eps=1e-12):
    """_SpectralNorm.forward on explicit tensors, in their dtype: -> (u, v, sigma, w / sigma); u, v are new tensors"""
    m = matrix_of(w, dim)
    if iterate:
        u = F.normalize(torch.mv(m, v), dim=0, eps=eps)
        v = F.normalize(torch.mv(m.t(), u), dim=0, eps=eps)
    sigma = torch.dot(u, torch.mv(m, v))
    return u.clone(), v.clone(), sigma, w / sigma


def spectral_backward_ref(g, weff, dim, u, v, sigma):
    """d(loss)/dW for W_eff = W / sigma(W), sigma = u^T M v with constant u, v:  (G - <G, W_eff> u v^T) / sigma, in W's layout"""
    d = (g * weff).sum()
    uv = torch.outer(u, v)
    if dim == 0:
        uv = uv.view(g.shape)
    else:
        uv = uv.view(g.shape[1], g.shape[0], *g.shape[2:]).permute(1, 0, 2, 3)
    return (g - d * uv) / sigma


class SpectralFakeBackend(fake_backend.FakeBackend):
    def spectral_table(self, jobs):
        self._count('spectral_table')
        t = ops.SpectralTable()
        t.jobs, t.count = list(jobs), len(jobs)
        return t

    def spectral_forward(self, table, iterate):
        self._count('spectral_forward')
        for j in table.jobs:
            u, v, sigma, weff = spectral_forward_ref(j.w.float(), j.dim, j.u, j.v, iterate)
            if iterate:
                j.u.copy_(u)
                j.v.copy_(v)
            j.u_snap.copy_(u)
            j.v_snap.copy_(v)
            j.sigma.fill_(float(sigma))
            j.weff.copy_(weff)

    def spectral_backward(self, table, accumulate, only=None):
        self._count('spectral_backward')
        for i, j in enumerate(table.jobs):
            if only is not None and i not in only:
                continue
            d = spectral_backward_ref(j.g, j.weff, j.dim, j.u_snap, j.v_snap, j.sigma[0])
            if accumulate:
                j.grad.add_(d)
            else:
                j.grad.copy_(d)


def install():
    ops._impl = SpectralFakeBackend()
    return ops._impl


def uninstall():
    fake_backend.uninstall()


def float64_twin(module):
    """deep copy of a container tree (net.model) in float64; parametrized convs stay parametrized, so running it (twin_forward) runs torch's own
    spectral norm: one power iteration per call in train() mode"""
    return copy.deepcopy(module).double()


def twin_forward(seq, x):
    """torch's forward of a container tree: the Sequential as it stands, a ResnetBlock container as x + conv_block(x) (networks.py:509-513)"""
    for m in seq:
        x = x + m.conv_block(x) if hasattr(m, 'conv_block') else m(x)
    return x
