"""Host logic of deepliif_amd/data.py on the CPU: parameter stream, panel counts, table selection, refused crops, samplers, and the loader
end to end on the emulated backend against tests/data_ref.py (the PIL restatement of the reference's loader).  Integer work and table
lookups throughout: every comparison is equality."""
import os
import random
import types

import numpy as np
import pytest
import torch
from PIL import Image

import data_ref
import fake_backend
from deepliif_amd import data as D
from deepliif_amd import engine as E
from deepliif_amd import models as M
from golden_util import synth_image

MODES = [None, 'resize_and_crop', 'crop', 'scale_width', 'scale_width_and_crop', 'none']


class GatherBackend(fake_backend.FakeBackend):
    """FakeBackend + dl_train_gather_u8 written from the header's formula in numpy (the tables applied as include/deepliif_hip.h states)"""

    def train_gather_supported(self, w2, h, new_w, new_h, ch, cw):
        return 1 if cw <= new_w and ch <= new_h else 0

    def train_gather_limit(self):
        return 'emulation'

    @staticmethod
    def _pass(src, tb):
        """one resize pass along axis 1: byte = clip((2^21 + sum pixel * k) >> 22, 0, 255)"""
        bounds, kk = (np.asarray(t) for t in tb)
        acc = np.full((src.shape[0], bounds.shape[0], src.shape[2]), 1 << 21, dtype=np.int64)
        for xx in range(bounds.shape[0]):
            x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
            acc[:, xx] += (src[:, x0:x0 + n] * kk[xx, :n, None].astype(np.int64)).sum(axis=1)
        return np.clip(acc >> 22, 0, 255)

    def train_gather(self, rows, w2, h, panel, gray, new_size, tables, params, lut, out, c0, zero_pad_to, strip_rows=0):
        self._count('train_gather')
        ch, cw = out.shape[1], out.shape[2]
        for s, row in enumerate(rows):
            a = row.numpy()[:, panel * w2:(panel + 1) * w2, :].astype(np.int64)
            assert a.shape == (h, w2, 3)
            if gray:
                a = ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16)[..., None]
            if tables[0] is not None:
                a = self._pass(a, tables[0])
            if tables[1] is not None:
                a = self._pass(a.transpose(1, 0, 2), tables[1]).transpose(1, 0, 2)
            assert a.shape[:2] == (new_size[1], new_size[0])
            cx, cy, flip = (int(v) for v in params[s])
            a = a[cy:cy + ch, cx:cx + cw]
            if flip:
                a = a[:, ::-1]
            nch = a.shape[2]
            out[s, :, :, c0:c0 + nch] = lut[torch.from_numpy(np.ascontiguousarray(a))].to(out.dtype)
            if zero_pad_to > c0 + nch:
                out[s, :, :, c0 + nch:zero_pad_to] = 0


@pytest.fixture(autouse=True)
def _fake():
    from deepliif_amd import ops
    ops._impl = GatherBackend()
    yield
    fake_backend.uninstall()


class CpuLoader(D.CustomDatasetDataLoader):
    def _device_from_opt(self, opt):
        return torch.device('cpu')


def data_opt(root, model='DeepLIIF', preprocess='resize_and_crop', load_size=24, crop_size=16, **kw):
    o = types.SimpleNamespace(dataroot=str(root), phase='train', dataset_mode='aligned', model=model, preprocess=preprocess, load_size=load_size,
                              crop_size=crop_size, direction='AtoB', input_nc=3, output_nc=3, no_flip=False, modalities_no=2, seg_no=1, input_no=1,
                              seg_gen=True, max_dataset_size=None, serial_batches=True, num_threads=0, gpu_ids=[0], batch_size=2, precision='fp32',
                              is_train=True)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def write_rows(root, n, num_img, w2, h, seed=0, phase='train'):
    d = os.path.join(str(root), phase)
    os.makedirs(d, exist_ok=True)
    paths = []
    for i in range(n):
        p = os.path.join(d, f'row_{i:02d}.png')
        Image.fromarray(synth_image(num_img * w2, h, seed + i)).save(p)
        paths.append(p)
    return paths


def ref_batches(paths, opt, batch_size):
    samples = [data_ref.getitem(Image.open(p), opt, p) for p in paths]
    return [data_ref.collate(samples[i:i + batch_size]) for i in range(0, len(samples), batch_size)]


def as_tensor(v):
    return E.from_engine(v) if isinstance(v, E.Act) else v


def assert_batch_equal(got, exp):
    assert set(got) == set(exp)
    for k, e in exp.items():
        g = got[k]
        if isinstance(e, torch.Tensor):
            assert torch.equal(as_tensor(g), e), k
        elif e and isinstance(e[0], torch.Tensor) or (isinstance(e, list) and not e):
            assert len(g) == len(e), k
            for a, b in zip(g, e):
                assert torch.equal(as_tensor(a), b), k
        else:
            assert list(g) == list(e), k


# ---- the parameter stream
@pytest.mark.parametrize('mode', MODES)
def test_parameter_stream_equals_get_params(mode, tmp_path):
    sizes = [(20, 12), (40, 40), (16, 12), (33, 47), (24, 24), (18, 14), (64, 30)]
    opt = data_opt(tmp_path, preprocess=mode, load_size=24, crop_size=12)
    os.makedirs(os.path.join(str(tmp_path), 'train'))
    ds = D.AlignedDataset(opt)
    random.seed(1234)
    exp = [data_ref.get_params(mode, 24, 12, s) for s in sizes]
    tail = random.random()
    random.seed(1234)
    got = []
    for w2, h in sizes:
        try:
            got.append(ds.geometry((w2 * ds.num_img + 1, h))['params'])       # a row that does not divide evenly: w2 = int(w / num_img)
        except NotImplementedError:
            got.append(None)                                                  # the draws were made before the crop was refused
    assert random.random() == tail
    for g, e in zip(got, exp):
        if g is not None:
            assert (int(g['crop_pos'][0]), int(g['crop_pos'][1]), bool(g['flip'])) == (int(e['crop_pos'][0]), int(e['crop_pos'][1]), bool(e['flip']))
    assert sum(g is not None for g in got) >= 4


@pytest.mark.parametrize('mode', MODES)
def test_geometry_matches_pil_sizes(mode):
    """resized_size / crop_window against what the PIL chain actually returns"""
    for (w, h), load, crop in [((20, 12), 24, 16), ((40, 40), 16, 12), ((16, 12), 16, 16), ((18, 14), 20, 8), ((19, 14), 20, 8), ((20, 12), 16, 8),
                               ((16, 30), 16, 8), ((8, 8), 8, 8)]:
        img = Image.fromarray(synth_image(w, h, 3))
        random.seed(w * h)
        params = data_ref.get_params(mode, load, crop, (w, h))
        new = D.resized_size(mode, load, crop, (w, h))
        try:
            x, y, cw, ch = D.crop_window(mode, crop, new, params['crop_pos'])
        except NotImplementedError:
            continue
        out = data_ref.transform_pil(img, mode, load, crop, True, params)
        assert out.size == (cw, ch), (mode, w, h, load, crop)


# ---- panel counts
@pytest.mark.parametrize('model,M_,seg_no,input_no,seg_gen,num,A,B,BS', [
    ('DeepLIIF', 4, 1, 1, True, 6, [0], [1, 2, 3, 4, 5], None),
    ('DeepLIIF', 2, 0, 1, False, 3, [0], [1, 2], None),
    ('DeepLIIFKD', 4, 1, 2, True, 7, [0, 1], [2, 3, 4, 5, 6], None),
    ('DeepLIIFExt', 3, 0, 1, True, 7, [0], [1, 2, 3], [4, 5, 6]),
    ('DeepLIIFExt', 3, 0, 1, False, 4, [0], [1, 2, 3], []),
    ('SDG', 2, 1, 3, False, 6, [0, 1, 2], [3, 4, 5], None),
])
def test_panel_counts(model, M_, seg_no, input_no, seg_gen, num, A, B, BS):
    opt = types.SimpleNamespace(model=model, modalities_no=M_, seg_no=seg_no, input_no=input_no, seg_gen=seg_gen)
    n, panels = D.panel_layout(opt)
    assert n == num == data_ref.num_images(model, M_, seg_no, input_no, seg_gen)
    assert panels['A'] == A and panels['B'] == B and panels.get('BS') == BS


def test_other_models_raise_the_reference_message():
    opt = types.SimpleNamespace(model='CycleGAN', modalities_no=1, seg_no=0, input_no=1, seg_gen=False)
    with pytest.raises(Exception, match='model class CycleGAN does not have corresponding implementation in deepliif/data/aligned_dataset.py'):
        D.panel_layout(opt)


# ---- tables
def test_table_selection_per_axis():
    assert D.axis_tables((20, 12), (20, 12)) == (None, None)                       # Pillow returns a copy
    tx, ty = D.axis_tables((16, 12), (16, 16))
    assert tx is None and ty[0].shape == (16, 2)                                   # vertical pass only
    tx, ty = D.axis_tables((20, 12), (16, 12))
    assert ty is None and tx[0].shape == (16, 2) and tx[1].shape[1] == 2 * 3 + 1   # 20 -> 16: support 2.5, ksize 2 * ceil(2.5) + 1
    tx, ty = D.axis_tables((20, 12), (24, 24))
    assert tx[0].shape == (24, 2) and ty[0].shape == (24, 2) and tx[1].shape[1] == ty[1].shape[1] == 5


def test_mixed_crop_is_refused():
    new = D.resized_size('scale_width_and_crop', 24, 16, (48, 20))                 # 24 x 16? no: int(max(24 * 20 / 48, 16)) = 16 -> fits
    assert new == (24, 16)
    assert D.crop_window('scale_width_and_crop', 16, new, (5, 0)) == (5, 0, 16, 16)
    with pytest.raises(NotImplementedError, match='20x12'):                         # 'crop' of 16 from a 20 x 12 panel: wider, but shorter
        D.crop_window('crop', 16, (20, 12), (2, 0))
    assert D.crop_window('crop', 16, (12, 12), (0, 0)) == (0, 0, 12, 12)           # smaller on both axes: __crop is a no-op


# ---- samplers
def test_sampler_and_shard_with_fake_rank(tmp_path, monkeypatch):
    write_rows(tmp_path, 7, 4, 8, 8)
    opt = data_opt(tmp_path, preprocess='none', serial_batches=False)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'DEEPLIIF_SEED'):
        monkeypatch.delenv(k, raising=False)
    plain = CpuLoader(opt)
    assert plain.sampler is None and isinstance(plain.dataloader.sampler, torch.utils.data.RandomSampler) and len(plain) == 7
    opt.serial_batches = True
    serial = CpuLoader(opt)
    assert isinstance(serial.dataloader.sampler, torch.utils.data.SequentialSampler)
    assert [b for b in serial.dataloader] == [[0, 1], [2, 3], [4, 5], [6]]
    seen = []
    for rank in (0, 1):
        monkeypatch.setenv('RANK', str(rank))
        monkeypatch.setenv('WORLD_SIZE', '2')
        ld = CpuLoader(opt)
        assert isinstance(ld.sampler, torch.utils.data.distributed.DistributedSampler) and ld.sampler.rank == rank and ld.sampler.num_replicas == 2
        ld.sampler.set_epoch(3)
        ref = list(torch.utils.data.distributed.DistributedSampler(ld.dataset, num_replicas=2, rank=rank))       # epoch 0 ...
        ref_s = torch.utils.data.distributed.DistributedSampler(ld.dataset, num_replicas=2, rank=rank)
        ref_s.set_epoch(3)
        idx = [i for b in ld.dataloader for i in b]
        assert idx == list(ref_s) and len(idx) == 4 and (idx != ref or True)
        seen += idx
    assert set(seen) == set(range(7))                                               # the two shards cover the dataset (one index padded)
    monkeypatch.delenv('RANK')
    monkeypatch.setenv('DEEPLIIF_SEED', '1')
    opt.serial_batches = False
    a = [i for b in CpuLoader(opt).dataloader for i in b]
    g = torch.Generator()
    g.manual_seed(0)
    ref_dl = torch.utils.data.DataLoader(list(range(7)), batch_size=2, shuffle=True, num_workers=0, generator=g)
    assert a == [int(i) for b in ref_dl for i in b]                                 # the reference's seeded order (deepliif/data/__init__.py:102-114)
    opt.max_dataset_size = 3
    short = CpuLoader(opt)
    assert len(short.dataset) == 3 and len(list(iter(short))) == 2                  # make_dataset cut + the i * batch_size >= max_dataset_size stop


# ---- the loader end to end on the emulated backend
CASES = [
    ('DeepLIIF', 'resize_and_crop', 24, 16, (20, 12), {}),
    ('DeepLIIF', 'resize_and_crop', 16, 12, (40, 40), {}),
    ('DeepLIIF', 'crop', 16, 8, (20, 12), {}),
    ('DeepLIIF', 'scale_width', 16, 8, (20, 12), {}),
    ('DeepLIIF', 'scale_width_and_crop', 16, 8, (20, 12), {}),
    ('DeepLIIF', 'none', 16, 8, (18, 14), {}),
    ('DeepLIIF', None, 16, 8, (18, 14), {'no_flip': True}),
    ('DeepLIIF', 'resize_and_crop', 24, 16, (20, 12), {'input_nc': 1}),
    ('DeepLIIF', 'resize_and_crop', 24, 16, (20, 12), {'direction': 'BtoA', 'input_nc': 1}),
    ('DeepLIIFKD', 'resize_and_crop', 24, 16, (20, 12), {'input_no': 2}),
    ('DeepLIIFExt', 'resize_and_crop', 24, 16, (20, 12), {}),
    ('DeepLIIFExt', 'crop', 16, 8, (12, 20), {'seg_gen': False}),
    ('SDG', 'resize_and_crop', 24, 16, (20, 12), {'input_no': 3}),
]


@pytest.mark.parametrize('model,mode,load,crop,panel,extra', CASES)
@pytest.mark.parametrize('threads', [0, 2])
def test_loader_equals_reference(model, mode, load, crop, panel, extra, threads, tmp_path):
    opt = data_opt(tmp_path, model=model, preprocess=mode, load_size=load, crop_size=crop, num_threads=threads, **extra)
    num_img = D.panel_layout(opt)[0]
    paths = write_rows(tmp_path, 5, num_img, panel[0], panel[1], seed=7)
    random.seed(99)
    exp = ref_batches(sorted(paths), opt, 2)
    tail = random.random()
    random.seed(99)
    loader = CpuLoader(opt)
    got = list(loader.load_data())
    assert random.random() == tail                                                  # same number of draws, in the same order
    assert len(got) == len(exp) == 3
    for g, e in zip(got, exp):
        if isinstance(e['A'], list):                                                # several input panels: the model concatenates them (set_input)
            e = dict(e, A=torch.cat(e['A'], dim=1))
        assert isinstance(g['A'], E.Act) and all(isinstance(b, E.Act) for b in g['B'])
        assert_batch_equal(g, e)
        assert (g['A'].t[..., g['A'].C:] == 0).all()


def test_loader_bf16_rounds_like_to_engine(tmp_path):
    opt = data_opt(tmp_path, precision='bf16')
    paths = write_rows(tmp_path, 2, 4, 20, 12)
    random.seed(5)
    exp = ref_batches(sorted(paths), opt, 2)[0]
    random.seed(5)
    got = next(iter(CpuLoader(opt)))
    assert got['A'].t.dtype == torch.bfloat16
    assert torch.equal(got['A'].t, E.to_engine(exp['A'], E.Precision.get('bf16')).t)


def test_rows_of_different_sizes_in_one_batch(tmp_path):
    opt = data_opt(tmp_path, preprocess='resize_and_crop', load_size=24, crop_size=16)
    d = os.path.join(str(tmp_path), 'train')
    os.makedirs(d)
    paths = []
    for i, (w2, h) in enumerate([(20, 12), (30, 26)]):
        paths.append(os.path.join(d, f'r{i}.png'))
        Image.fromarray(synth_image(4 * w2, h, 11 + i)).save(paths[-1])
    random.seed(8)
    exp = ref_batches(paths, opt, 2)[0]
    random.seed(8)
    assert_batch_equal(next(iter(CpuLoader(opt))), exp)


def test_create_dataset_has_no_cpu_path(tmp_path):
    write_rows(tmp_path, 1, 4, 8, 8)
    opt = data_opt(tmp_path, gpu_ids=[])
    with pytest.raises(Exception, match='MI355X|GPU'):
        D.create_dataset(opt)


# ---- set_input
class CpuModel(M.DeepLIIFModel):
    def _device_from_opt(self, opt):
        return torch.device('cpu')

    def _net_gpu_ids(self):
        return []


class CpuExtModel(M.DeepLIIFExtModel):
    def _device_from_opt(self, opt):
        return torch.device('cpu')

    def _net_gpu_ids(self):
        return []


def test_set_input_takes_act_batches(tmp_path):
    from test_host_model import make_opt
    mopt = make_opt(2, True, 'batch')
    torch.manual_seed(0)
    model = CpuModel(mopt)
    model.setup(mopt)
    opt = data_opt(tmp_path, load_size=72, crop_size=64)                            # 64: the smallest side unet_64 takes
    paths = write_rows(tmp_path, 2, 4, 80, 80)
    random.seed(3)
    exp = ref_batches(sorted(paths), opt, 2)[0]
    random.seed(3)
    got = next(iter(CpuLoader(opt)))
    model.set_input(exp)
    ref = [model._A.t.clone()] + [b.t.clone() for b in model._B] + [model._Bseg.t.clone()]
    ref_real = [model.real_A.clone(), model.real_B_1.clone(), model.real_B_2.clone(), getattr(model, f'real_B_{model.mod_id_seg}').clone()]
    model.set_input(got)
    assert model._A is not got['A'] and model._A.t is got['A'].t                    # adopted: no copy, no layout pass
    new = [model._A.t] + [b.t for b in model._B] + [model._Bseg.t]
    assert len(new) == len(ref) and all(torch.equal(a, b) for a, b in zip(new, ref))
    real = [model.real_A, model.real_B_1, model.real_B_2, getattr(model, f'real_B_{model.mod_id_seg}')]
    assert all(torch.equal(a, b) for a, b in zip(real, ref_real))
    assert model.image_paths == sorted(paths)
    model.optimize_parameters()                                                     # the step runs from the adopted activations
    assert all(np.isfinite(v) for v in model.get_current_losses().values())
    bad = dict(got, A=E.Act(got['A'].t.to(torch.bfloat16), 3))
    with pytest.raises(TypeError, match='set_input'):
        model.set_input(bad)


def test_ext_set_input_takes_act_batches(tmp_path):
    from test_host_model import make_opt
    mopt = make_opt(2, True, 'batch')
    mopt.model, mopt.net_ds = 'DeepLIIFExt', 'n_layers'
    mopt.loss_G_weights = mopt.loss_D_weights = mopt.seg_weights = [0.5, 0.5]
    torch.manual_seed(0)
    model = CpuExtModel(mopt)
    opt = data_opt(tmp_path, model='DeepLIIFExt', load_size=36, crop_size=32)
    paths = write_rows(tmp_path, 2, 5, 40, 40)
    random.seed(3)
    exp = ref_batches(sorted(paths), opt, 2)[0]
    random.seed(3)
    got = next(iter(CpuLoader(opt)))
    model.set_input(exp)
    ref = [model._A.t.clone()] + [b.t.clone() for b in model._B + model._BS]
    model.set_input(got)
    new = [model._A.t] + [b.t for b in model._B + model._BS]
    assert len(new) == len(ref) == 5 and all(torch.equal(a, b) for a, b in zip(new, ref))
    assert torch.equal(model.real_A, exp['A']) and all(torch.equal(a, b) for a, b in zip(model.real_B + model.real_BS, exp['B'] + exp['BS']))
