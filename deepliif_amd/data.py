"""Training batches built on the GPU from 8-bit dataset rows: the drop-in for deepliif.data.create_dataset (dataset_mode 'aligned').

The reference's AlignedDataset.__getitem__ (deepliif/data/aligned_dataset.py:36-113) cuts one wide image into panels, runs every panel
through PIL (Grayscale, Resize bicubic, crop, flip -- base_dataset.py:80-114 get_transform), then ToTensor and Normalize, and hands fp32
NCHW host tensors to set_input(), which copies them to the device and converts the layout.  Here only the decode stays on the CPU:

  * a pool of opt.num_threads threads runs Image.open(...).convert('RGB') into pinned uint8 staging buffers (0 = in the calling thread);
  * the 8-bit rows go to the device on a side stream, one batch ahead of the batch being handed out;
  * dl_train_gather_u8 (include/deepliif_hip.h) does the rest for one panel of every sample per launch -- convert('L'), PIL's integer
    bicubic resize with one coefficient table per axis (tiling.resample_table), per-sample crop and flip, the 256-entry ToTensor +
    Normalize table, engine layout in the model's precision -- bit for bit what the reference chain followed by engine.to_engine gives.

The loader yields the reference's dict (A, B, BS for DeepLIIFExt, A_paths, B_paths) with engine.Act values; DeepLIIFModel /
DeepLIIFExtModel.set_input (and SDG / DeepLIIFKD, which inherit it) adopt them without a copy.  Sizes, crop positions and flips are
restatements of get_params / __scale_width / __make_power_2 / __crop, drawn in the calling process from Python's `random` in sample order
(randint, randint, random() per sample): the stream the reference draws with num_threads = 0.  There is no CPU path: a geometry the
kernel does not serve raises.  Unaligned data (CycleGAN) is not covered.
"""
from __future__ import annotations

import os
import random
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.utils.data
from PIL import Image
from torch.utils.data.distributed import DistributedSampler

from . import engine as E
from . import ops
from .tiling import resample_table

IMG_EXTENSIONS = ['.jpg', '.JPG', '.jpeg', '.JPEG', '.png', '.PNG', '.ppm', '.PPM', '.bmp', '.BMP', '.tif', '.TIF', '.tiff', '.TIFF']      # image_folder.py:13-17
PREPROCESS_MODES = (None, 'resize_and_crop', 'crop', 'scale_width', 'scale_width_and_crop', 'none')


def make_dataset(dir: str, max_dataset_size=None) -> List[str]:
    """deepliif/data/image_folder.py:24-34"""
    assert os.path.isdir(dir), '%s is not a valid directory' % dir
    images = []
    for root, _, fnames in sorted(os.walk(dir)):
        for fname in fnames:
            if any(fname.endswith(e) for e in IMG_EXTENSIONS):
                images.append(os.path.join(root, fname))
    return images[:max_dataset_size] if max_dataset_size else images


def panel_layout(opt) -> Tuple[int, Dict[str, List[int]]]:
    """(num_img, {'A': panels, 'B': panels, 'BS': panels}) of one dataset row (aligned_dataset.py:53-62 and :72-111)"""
    M, model = opt.modalities_no, opt.model
    if model in ('DeepLIIF', 'DeepLIIFKD', 'SDG'):
        num_img = M + opt.seg_no + opt.input_no
        if model == 'SDG':
            return num_img, {'A': list(range(opt.input_no)), 'B': list(range(opt.input_no, opt.input_no + M + 1))}
        return num_img, {'A': list(range(opt.input_no)) if opt.input_no > 1 else [0], 'B': list(range(opt.input_no, num_img))}
    if model == 'DeepLIIFExt':
        num_img = M * 2 + 1 if opt.seg_gen else M + 1
        return num_img, {'A': [0], 'B': list(range(1, M + 1)), 'BS': list(range(M + 1, 2 * M + 1)) if opt.seg_gen else []}
    raise Exception(f'model class {model} does not have corresponding implementation in deepliif/data/aligned_dataset.py')


def get_params(preprocess, load_size: int, crop_size: int, size: Tuple[int, int]) -> dict:
    """base_dataset.py:62-77, draw for draw"""
    w, h = size
    new_h, new_w = h, w
    if preprocess == 'resize_and_crop':
        new_h = new_w = load_size
    elif preprocess == 'scale_width_and_crop':
        new_w = load_size
        new_h = load_size * h // w
    x = random.randint(0, max(0, new_w - crop_size))
    y = random.randint(0, max(0, new_h - crop_size))
    flip = random.random() > 0.5
    return {'crop_pos': (x, y), 'flip': flip}


def resized_size(preprocess, load_size: int, crop_size: int, size: Tuple[int, int]) -> Tuple[int, int]:
    """(width, height) of a panel after the resize step of get_transform (base_dataset.py:85-89 Resize / __scale_width :128-134, and :97-98
    __make_power_2 :117-125 for 'none'); the input size where the reference returns the image untouched"""
    w, h = size
    p = preprocess or ''
    if 'resize' in p:
        return load_size, load_size
    if 'scale_width' in p:
        if w == load_size and h >= crop_size:
            return w, h
        return load_size, int(max(load_size * h / w, crop_size))
    if p == 'none':
        return int(round(w / 4) * 4), int(round(h / 4) * 4)
    return w, h


def crop_window(preprocess, crop_size: int, new_size: Tuple[int, int], pos: Tuple[int, int]) -> Tuple[int, int, int, int]:
    """(x, y, width, height) of the window __crop (base_dataset.py:137-143) cuts from the resized panel: the whole panel unless the mode
    crops and the panel exceeds crop_size on an axis.  A window that leaves the panel (PIL pads it with black) is refused."""
    nw, nh = new_size
    if 'crop' in (preprocess or '') and (nw > crop_size or nh > crop_size):
        x, y = pos
        if x < 0 or y < 0 or x + crop_size > nw or y + crop_size > nh:
            raise NotImplementedError(f'crop of {crop_size}x{crop_size} at ({x}, {y}) leaves the resized image of {nw}x{nh}: PIL would pad with black, '
                                      f'which deepliif_amd.data does not emulate (make load_size / the images at least crop_size on both axes)')
        return x, y, crop_size, crop_size
    return 0, 0, nw, nh


def axis_tables(size: Tuple[int, int], new_size: Tuple[int, int]):
    """(x table, y table) for Image.resize size -> new_size: None for an axis whose length does not change (Pillow skips that pass)"""
    return tuple(resample_table(a, b) if a != b else None for a, b in zip(size, new_size))


def normalize_lut() -> torch.Tensor:
    """ToTensor + Normalize(0.5, 0.5) per byte value, in torch's own float32 operations"""
    return torch.arange(256, dtype=torch.uint8).float().div(255).sub(0.5).div(0.5)


class AlignedDataset:
    """Host side of the reference's AlignedDataset (aligned_dataset.py:14-34): paths, panel layout and per-sample geometry."""

    def __init__(self, opt, phase='train'):
        self.root = opt.dataroot
        self.preprocess = opt.preprocess
        if self.preprocess not in PREPROCESS_MODES:
            raise ValueError(f'unknown preprocess {self.preprocess!r} ({" | ".join(str(m) for m in PREPROCESS_MODES)})')
        self.dir_AB = os.path.join(opt.dataroot, phase)
        self.AB_paths = sorted(make_dataset(self.dir_AB, opt.max_dataset_size))
        assert opt.load_size >= opt.crop_size
        b_to_a = getattr(opt, 'direction', 'AtoB') == 'BtoA'
        self.input_nc = opt.output_nc if b_to_a else opt.input_nc
        self.output_nc = opt.input_nc if b_to_a else opt.output_nc
        self.no_flip = opt.no_flip
        self.load_size, self.crop_size = opt.load_size, opt.crop_size
        self.model = opt.model
        self.num_img, self.panels = panel_layout(opt)
        last = max(i for panels in self.panels.values() for i in panels)
        if last >= self.num_img:          # SDG reads modalities_no + 1 targets whatever seg_no says: PIL would hand back a black panel past the row's end
            raise ValueError(f'model {self.model} reads panel {last} of rows that are cut into {self.num_img} panels (modalities_no, seg_no, input_no)')

    def __len__(self):
        return len(self.AB_paths)

    def __getitem__(self, index):          # the torch samplers only need len(); the DataLoader that batches the indices reads this
        return index

    def geometry(self, row_size: Tuple[int, int]) -> dict:
        """draws this sample's parameters (get_params) and resolves them: panel size, resized size, crop window, flip"""
        w, h = row_size
        w2 = int(w / self.num_img)
        params = get_params(self.preprocess, self.load_size, self.crop_size, (w2, h))
        new = resized_size(self.preprocess, self.load_size, self.crop_size, (w2, h))
        if w2 <= 0 or min(new) <= 0:
            raise ValueError(f'a dataset row of {w}x{h} gives {self.num_img} panels of {w2}x{h} -> {new[0]}x{new[1]}: nothing to load')
        x, y, cw, ch = crop_window(self.preprocess, self.crop_size, new, params['crop_pos'])
        return {'panel': (w2, h), 'new': new, 'crop': (x, y, cw, ch), 'flip': bool(params['flip']) and not self.no_flip, 'params': params}


class _Slot:
    """one batch in flight: pinned staging rows, their device copies, the event of the copy and the event of the kernels that read them"""

    def __init__(self):
        self.pinned: List[Optional[torch.Tensor]] = []
        self.dev: List[Optional[torch.Tensor]] = []
        self.copied = None
        self.read = None
        self.indices: List[int] = []
        self.futures = []
        self.rows: List[torch.Tensor] = []
        self.geo: List[dict] = []
        self.params: Optional[torch.Tensor] = None


class CustomDatasetDataLoader:
    """deepliif/data/__init__.py:67-130 with the transform chain on the GPU (module docstring)."""

    def __init__(self, opt, phase=None, batch_size=None):
        self.batch_size = batch_size if batch_size else opt.batch_size
        self.max_dataset_size = opt.max_dataset_size
        if opt.dataset_mode != 'aligned':
            raise NotImplementedError(f"deepliif_amd.data serves dataset_mode 'aligned' (got {opt.dataset_mode!r})")
        self.dataset = AlignedDataset(opt, phase=phase if phase else opt.phase)
        print("dataset [%s] was created" % type(self.dataset).__name__)
        self.device = self._device_from_opt(opt)
        self.precision = E.Precision.get(getattr(opt, 'precision', None) or _default_precision())
        self.num_threads = int(opt.num_threads)

        sampler = None
        if os.getenv('LOCAL_RANK') is not None or os.getenv('RANK') is not None:
            sampler = self._distributed_sampler() if len(opt.gpu_ids) > 0 else None
        generator = None
        if os.getenv('DEEPLIIF_SEED', None) is not None:
            generator = torch.Generator()
            generator.manual_seed(0)
        # torch's own DataLoader batches the INDICES (same samplers, same draws from the same generators as the reference's loader); the samples
        # themselves are decoded by this class's thread pool
        self.dataloader = torch.utils.data.DataLoader(self.dataset, sampler=sampler, batch_size=self.batch_size,
                                                      shuffle=not opt.serial_batches if sampler is None else False, num_workers=0, generator=generator,
                                                      collate_fn=lambda idx: [int(i) for i in idx])
        self.sampler = sampler
        self._cuda = self.device.type == 'cuda'
        self._lut = normalize_lut().to(self.device)
        self._tables: dict = {}
        self._slots = [_Slot() for _ in range(3)]
        self._side = torch.cuda.Stream(self.device) if self._cuda else None
        self._pool = ThreadPoolExecutor(max_workers=self.num_threads, thread_name_prefix='dl_decode') if self.num_threads > 0 else None

    def _device_from_opt(self, opt) -> torch.device:
        from .models import pick_gpu
        return torch.device('cuda:{}'.format(pick_gpu(opt.gpu_ids, getattr(opt, 'is_train', True))))

    def _distributed_sampler(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return DistributedSampler(self.dataset)
        rank = int(os.getenv('RANK') if os.getenv('RANK') is not None else os.getenv('LOCAL_RANK'))
        return DistributedSampler(self.dataset, num_replicas=int(os.getenv('WORLD_SIZE', '1')), rank=rank)

    def load_data(self):
        return self

    def __len__(self):
        return max(len(self.dataset), self.max_dataset_size or 0)

    # ---- host side: decode into pinned staging, copy one batch ahead
    def _decode(self, slot: _Slot, i: int, path: str) -> Tuple[int, int]:
        im = Image.open(path).convert('RGB')
        w, h = im.size
        need = h * w * 3
        buf = slot.pinned[i]
        if buf is None or buf.numel() < need:
            buf = slot.pinned[i] = torch.empty(need, dtype=torch.uint8, pin_memory=self._cuda)
        np.copyto(buf[:need].view(h, w, 3).numpy(), np.asarray(im))
        return w, h

    def _prepare(self, slot: _Slot, indices: Sequence[int]) -> None:
        """start decoding a batch into the slot's staging buffers"""
        if slot.copied is not None:
            slot.copied.synchronize()            # the copy that last read these staging buffers has finished
        n = len(indices)
        slot.indices = list(indices)
        slot.pinned += [None] * (n - len(slot.pinned))
        slot.dev += [None] * (n - len(slot.dev))
        paths = [self.dataset.AB_paths[i] for i in indices]
        if self._pool is None:
            sizes = [self._decode(slot, i, p) for i, p in enumerate(paths)]
            slot.futures = [_Done(s) for s in sizes]
        else:
            slot.futures = [self._pool.submit(self._decode, slot, i, p) for i, p in enumerate(paths)]

    def _upload(self, slot: _Slot) -> None:
        """wait for the decode, draw the parameters in sample order, send the rows to the device on the side stream"""
        sizes = [f.result() for f in slot.futures]
        slot.geo = [self.dataset.geometry(s) for s in sizes]
        slot.rows = []
        rec = torch.tensor([[g['crop'][0], g['crop'][1], int(g['flip'])] for g in slot.geo], dtype=torch.int32)      # the kernels' per-sample record
        if not self._cuda:
            slot.rows = [slot.pinned[i][:h * w * 3].view(h, w, 3) for i, (w, h) in enumerate(sizes)]
            slot.params = rec
            return
        if slot.read is not None:
            self._side.wait_event(slot.read)     # the kernels that last read these device rows have finished
        with torch.cuda.stream(self._side):
            for i, (w, h) in enumerate(sizes):
                need = h * w * 3
                if slot.dev[i] is None or slot.dev[i].numel() < need:
                    slot.dev[i] = torch.empty(need, dtype=torch.uint8, device=self.device)
                slot.dev[i][:need].copy_(slot.pinned[i][:need], non_blocking=True)
                slot.rows.append(slot.dev[i][:need].view(h, w, 3))
            slot.params = rec.pin_memory().to(self.device, non_blocking=True)
            slot.copied = torch.cuda.Event()
            slot.copied.record(self._side)

    def _table(self, n_in: int, n_out: int):
        key = (n_in, n_out)
        if key not in self._tables:
            self._tables[key] = tuple(torch.from_numpy(np.array(a)).to(self.device) for a in resample_table(n_in, n_out))
        return self._tables[key]

    def _gather(self, be, slot: _Slot, which: Sequence[int], panel: int, gray: bool, out: torch.Tensor, c0: int, zero_to: int) -> None:
        g = slot.geo[which[0]]
        (w2, h), new = g['panel'], g['new']
        ch, cw = out.shape[1], out.shape[2]
        if not be.train_gather_supported(w2, h, new[0], new[1], ch, cw):
            raise NotImplementedError(f'resize of a {w2}x{h} panel to {new[0]}x{new[1]} with a crop of {cw}x{ch} is not served by dl_train_gather_u8: '
                                      f'{be.train_gather_limit()}')
        tables = tuple(None if tb is None else self._table(a, b) for tb, a, b in zip(axis_tables((w2, h), new), (w2, h), new))
        params = slot.params[which[0]:which[-1] + 1]              # `which` is the whole batch or one sample
        dst = out if len(which) == out.shape[0] else out[which[0]:which[0] + 1]
        be.train_gather([slot.rows[i] for i in which], w2, h, panel, gray, new, tables, params, self._lut, dst, c0, zero_to)

    def _launch(self, slot: _Slot) -> dict:
        """the kernels of one uploaded batch, on the current stream, and the reference's dict"""
        ds, n = self.dataset, len(slot.indices)
        sizes = {(g['crop'][2], g['crop'][3]) for g in slot.geo}
        if len(sizes) != 1:
            raise ValueError(f'the samples of one batch come out in different sizes {sorted(sizes)}: they cannot be stacked (the reference fails in collate)')
        cw, ch = next(iter(sizes))
        same = all(g['panel'] == slot.geo[0]['panel'] and g['new'] == slot.geo[0]['new'] for g in slot.geo)
        groups = [list(range(n))] if same else [[i] for i in range(n)]          # one launch per panel, or per sample when the row sizes differ
        if self._cuda:
            torch.cuda.current_stream(self.device).wait_event(slot.copied)
        out: dict = {}
        with ops.half_mode(self.precision.half):
            be = ops.impl()
            for key, panels in ds.panels.items():
                gray = (ds.input_nc if key == 'A' else ds.output_nc) == 1
                nc = 1 if gray else 3
                if key == 'A':                   # several input panels: channel slices of ONE activation (set_input would torch.cat them)
                    a = E.new_act(n, ch, cw, nc * len(panels), self.precision, self.device)
                    for j, panel in enumerate(panels):
                        for which in groups:
                            self._gather(be, slot, which, panel, gray, a.t, j * nc, a.t.shape[3] if j + 1 == len(panels) else (j + 1) * nc)
                    out[key] = a
                    continue
                acts = []
                for panel in panels:
                    a = E.new_act(n, ch, cw, nc, self.precision, self.device)
                    for which in groups:
                        self._gather(be, slot, which, panel, gray, a.t, 0, a.t.shape[3])
                    acts.append(a)
                out[key] = acts
        if self._cuda:
            slot.read = torch.cuda.Event()
            slot.read.record(torch.cuda.current_stream(self.device))
        paths = [ds.AB_paths[i] for i in slot.indices]
        out['A_paths'], out['B_paths'] = paths, list(paths)
        return out

    def __iter__(self):
        """batches in the reference's order; while batch k is handed out, batch k + 1 is on its way to the device and batch k + 2 is being decoded"""
        batches = []
        for i, idx in enumerate(self.dataloader):
            if self.max_dataset_size and i * self.batch_size >= self.max_dataset_size:
                break
            batches.append(idx)
        slots = self._slots
        for k in range(min(2, len(batches))):
            self._prepare(slots[k % 3], batches[k])
        if batches:
            self._upload(slots[0])
        for k in range(len(batches)):
            data = self._launch(slots[k % 3])
            if k + 1 < len(batches):
                self._upload(slots[(k + 1) % 3])
            if k + 2 < len(batches):
                self._prepare(slots[(k + 2) % 3], batches[k + 2])
            yield data


class _Done:
    def __init__(self, value):
        self._value = value

    def result(self):
        return self._value


def _default_precision() -> str:
    from . import networks
    return networks.DEFAULT_PRECISION


def create_dataset(opt, phase=None, batch_size=None):
    """deepliif/data/__init__.py:58-64"""
    return CustomDatasetDataLoader(opt, phase=phase if phase else opt.phase, batch_size=batch_size if batch_size else opt.batch_size)
