"""Fixture of the spectral-normalisation tests, recorded from the REFERENCE implementation (`--norm spectral`).

Runs only where the reference checkout exists (tests/golden/_ref_import.py).  Usage:
    python tests/golden/make_golden_spectral.py
Writes tests/golden/step_spectral_m2.npz -- data only:
  keys/<case>, shapes/<case>      state_dict key lists of the reference's resnet_9blocks (both upsample modes) and n_layers nets under norm='spectral'
  init/<case>/sums, abs_sums      per-key checksums right after torch.manual_seed(INIT_SEED); define_G / define_D(...): the RNG order of construction
                                  (the _SpectralNorm draws and 15 warm-up iterations) and of init_weights (which writes into a temporary: the weights keep
                                  PyTorch's default initialisation, the RNG is consumed and u, v advance by one iteration per conv)
  step<s>/...                     2 optimize_parameters() steps of DeepLIIFModel (2 modalities + seg, unet_64, ngf = ndf = 8, 64 x 64, batch 2, zero padding)
                                  in make_golden.make_step's layout, plus a digest of all _u / _v of every network after each step
Weights are not stored: tests/spectral_util.fill_seeded(net, seed) redraws them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import _ref_import  # noqa: E402
from golden_util import digest, seeded_uniform  # noqa: E402
import spectral_util as SU  # noqa: E402

models, networks = _ref_import.import_reference()
from deepliif.options import Options  # noqa: E402

torch.set_num_threads(8)

INIT_SEED = 11
NF_INIT = 16
CASES = {
    'resnet_9blocks_convtranspose': lambda nw: nw.define_G(3, 3, NF_INIT, 'resnet_9blocks', 'spectral', False, 'normal', 0.02, [], 'zero', 'convtranspose'),
    'resnet_9blocks_resize_conv': lambda nw: nw.define_G(3, 3, NF_INIT, 'resnet_9blocks', 'spectral', False, 'normal', 0.02, [], 'reflect', 'resize_conv'),
    'n_layers': lambda nw: nw.define_D(6, NF_INIT, 'n_layers', 4, 'spectral', 'normal', 0.02, []),
}
STEP_SEED0 = 1500


def uv_flat(net):
    parts = [v.reshape(-1).float() for k, v in net.state_dict().items() if k.endswith('._u') or k.endswith('._v')]
    return torch.cat(parts) if parts else None


def base_params():
    w = [1.0 / 3] * 3
    return dict(
        model='DeepLIIF', name='golden', checkpoints_dir='/tmp/golden_ckpt', gpu_ids=[], phase='train', preprocess='none',
        remote_transfer_cmd=None, continue_train=False, modalities_no=2, seg_gen=True,
        modalities_names=[], input_nc=3, input_no=1, output_nc=3, ngf=8, ndf=8, net_g='resnet_9blocks',
        net_gs='unet_64', net_d='n_layers', norm='spectral', no_dropout=True, init_type='normal', init_gain=0.02,
        padding='zero', upsample='convtranspose', gan_mode='vanilla', gan_mode_s='lsgan', optimizer='adam',
        lr_g=2e-4, lr_d=2e-4, beta1=0.5, lr_policy='linear', n_epochs=100, n_epochs_decay=100, epoch_count=0,
        seg_weights=w, loss_G_weights=w, loss_D_weights=w, verbose=False, epoch='latest', load_iter=0)


def main():
    out = {}
    for tag, fn in CASES.items():
        torch.manual_seed(INIT_SEED)
        sd = fn(networks).state_dict()
        out[f'keys/{tag}'] = np.array(list(sd.keys()))
        out[f'shapes/{tag}'] = np.array([str(tuple(v.shape)) for v in sd.values()])
        out[f'init/{tag}/sums'] = np.array([v.double().sum().item() for v in sd.values()])
        out[f'init/{tag}/abs_sums'] = np.array([v.double().abs().sum().item() for v in sd.values()])
    out['init_meta'] = np.array([str(INIT_SEED), str(NF_INIT)])

    os.makedirs('/tmp/golden_ckpt/golden', exist_ok=True)
    opt = Options(d_params=base_params())
    model = models.create_model(opt)
    model.setup(opt)
    size, batch, steps = 64, 2, 2
    for j, n in enumerate(model.model_names):
        SU.fill_seeded(getattr(model, 'net' + n), STEP_SEED0 + j)
    A = seeded_uniform((batch, 3, size, size), 22)
    B = [seeded_uniform((batch, 3, size, size), 23 + i) for i in range(3)]
    out['meta'] = np.array(['2', 'True', 'spectral', 'zero', 'unet_64', str(size), '8', str(batch), str(steps)])
    out['model_names'] = np.array(model.model_names)
    out['net_seeds'] = np.array([STEP_SEED0 + j for j in range(len(model.model_names))])
    out['loss_names'] = np.array(model.loss_names)
    out['mod_id_seg'] = np.array(str(model.mod_id_seg))
    out['spectral_nets'] = np.array([n for n in model.model_names if uv_flat(getattr(model, 'net' + n)) is not None])
    for s in range(steps):
        model.set_input({'A': A, 'B': B, 'A_paths': ['x']})
        model.optimize_parameters()
        losses = model.get_current_losses()
        out[f'step{s}/losses'] = np.array([losses[k] for k in model.loss_names], dtype=np.float64)
        for i in range(2):
            out[f'step{s}/fake_B_{i + 1}'] = getattr(model, f'fake_B_{i + 1}').detach().numpy()[:, :, ::2, ::2]
        out[f'step{s}/fake_B_S'] = getattr(model, f'fake_B_{model.mod_id_seg}').detach().numpy()[:, :, ::2, ::2]
        for n in model.model_names:
            net = getattr(model, 'net' + n)
            sd = net.state_dict()
            out[f'step{s}/w_digest/{n}'] = digest(torch.cat([v.reshape(-1).float() for v in sd.values() if v.is_floating_point()]))
            uv = uv_flat(net)
            if uv is not None:
                out[f'step{s}/uv_digest/{n}'] = digest(uv)
    path = os.path.join(HERE, 'step_spectral_m2.npz')
    np.savez_compressed(path, **out)
    print('step_spectral_m2.npz', os.path.getsize(path) // 1024, 'KiB;', 'spectral nets:', list(out['spectral_nets']), 'losses', out['step1/losses'])


if __name__ == '__main__':
    main()
