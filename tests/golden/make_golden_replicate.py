"""Fixture of the replicate-padding tests, recorded from the REFERENCE implementation (`--padding replicate`).

Runs only where the reference checkout exists (tests/golden/_ref_import.py).  Usage:
    python tests/golden/make_golden_replicate.py
Writes tests/golden/resnet_replicate.npz -- data only:
  keys/<norm>[_dropout], shapes/...   state_dict key and shape lists of the reference's define_G(3, 3, 8, 'resnet_2blocks', norm, dropout, ..., 'replicate') for
                                      norm = batch | instance | spectral: ResnetBlock puts nn.ReplicationPad2d(1) in front of both convs (networks.py:482-483,
                                      499-500), so the convs sit at conv_block.1 / .5 (.6 behind a Dropout) and the norms at .2 / .6 (.7)
  <norm>/sd/<key>                     (float16, lossless: the values are rounded to half before use) the state_dict of ResnetGenerator(3, 3, ngf=8, n_blocks=2, padding_type='replicate') for batch and instance norm, filled
                                      with seeded N(0, 0.3)-scaled values (init_weights' N(0, 0.02) leaves the border of a 32 x 32 map within rounding of zero
                                      padding's; the test wants the three modes far apart)
  <norm>/x, y, dx, dw/<key>           an input (2 x 3 x 32 x 24), the training-mode output and the gradients of out.square().mean() with respect to the input
                                      and every parameter
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _ref_import  # noqa: E402
from golden_util import seeded_uniform  # noqa: E402

models, networks = _ref_import.import_reference()

torch.set_num_threads(8)
W_SEED, X_SEED = 2100, 2101
SHAPE = (2, 3, 32, 24)


def fill_seeded(net, seed):
    """conv weights ~ N(0, 0.3 / sqrt(fan_in / 9)), norm weights ~ N(1, 0.1), biases ~ N(0, 0.1), in state_dict order from one generator"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if not v.is_floating_point() or 'running' in k:
                continue
            if v.dim() == 4:
                v.copy_(torch.randn(v.shape, generator=g) * (0.3 / (v.shape[1] * v.shape[2] * v.shape[3] / 9.0) ** 0.5))
            elif k.endswith('.weight'):
                v.copy_(1.0 + 0.1 * torch.randn(v.shape, generator=g))
            else:
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            v.copy_(v.half().float())          # exactly representable in IEEE half: the fixture stores the state_dict as float16 without loss


def main():
    out = {}
    for norm in ('batch', 'instance', 'spectral'):
        for dropout in (False, True):
            torch.manual_seed(1)
            sd = networks.define_G(3, 3, 8, 'resnet_2blocks', norm, dropout, 'normal', 0.02, [], 'replicate').state_dict()
            tag = norm + ('_dropout' if dropout else '')
            out[f'keys/{tag}'] = np.array(list(sd.keys()))
            out[f'shapes/{tag}'] = np.array([str(tuple(v.shape)) for v in sd.values()])
    for norm in ('batch', 'instance'):
        net = networks.ResnetGenerator(3, 3, ngf=8, norm_layer=networks.get_norm_layer(norm), n_blocks=2, padding_type='replicate')
        fill_seeded(net, W_SEED)
        net.train()
        for k, v in net.state_dict().items():
            out[f'{norm}/sd/{k}'] = v.detach().clone().numpy().astype(np.float16) if v.is_floating_point() else v.detach().clone().numpy()
            assert not v.is_floating_point() or np.array_equal(out[f'{norm}/sd/{k}'].astype(np.float32), v.detach().numpy())
        x = seeded_uniform(SHAPE, X_SEED).requires_grad_(True)
        y = net(x)
        params = dict(net.named_parameters())
        grads = torch.autograd.grad(y.square().mean(), [x] + list(params.values()))
        out[f'{norm}/x'], out[f'{norm}/y'], out[f'{norm}/dx'] = x.detach().numpy(), y.detach().numpy(), grads[0].numpy()
        for (k, _), g in zip(params.items(), grads[1:]):
            out[f'{norm}/dw/{k}'] = g.numpy()
    path = os.path.join(HERE, 'resnet_replicate.npz')
    np.savez_compressed(path, **out)
    print('resnet_replicate.npz', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
