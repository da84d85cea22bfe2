"""tile_size != scale_size on the CPU: tiling.resample_table() against PIL's Image.resize (byte for byte), and the infer_region
route of inference() for resampled tiles against the host route (_inference_resampled), on the emulated ops backend extended with
the resample entries -- implemented with PIL itself here, so that the test pins the ROUTE (geometry in tile coordinates, empty
tiles, bands over ranks, multi-input split); tests/test_gpu_resample.py pins the kernels."""
import types

import numpy as np
import pytest
import torch
from PIL import Image

import fake_backend
from deepliif_amd import inference as I
from deepliif_amd import ops
from deepliif_amd import tiling as TL
from golden_util import synth_image

SIZES = [(48, 64), (64, 48), (32, 64), (64, 32), (96, 64), (64, 96), (61, 64), (64, 61), (16, 64), (256, 64)]


def _noise(s, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (s, s, 3)).astype(np.uint8)


def _smooth_saturated(s):
    """smooth ramps and waves clipped to plateaus of 0 and 255: the negative lobes overshoot at the plateau edges, so the clip matters"""
    yy, xx = np.mgrid[0:s, 0:s].astype(np.float64)
    a = np.stack([np.sin(xx * 9.0 / s) * 260 + 128, np.cos(yy * 7.0 / s) * 300 + 100, (xx + yy) * (700.0 / (2 * s)) - 200], axis=-1)
    a[s // 4:s // 2, s // 4:s // 2] = 255                      # hard edges too
    a[s // 2:3 * s // 4, s // 8:s // 3] = 0
    return np.clip(a, 0, 255).astype(np.uint8)


def _apply_table(a, d):
    """resample_table() driven by hand: horizontal, uint8, vertical; int32 accumulator, wrap-around as the hardware's"""
    def one_pass(src, table):                                   # along axis 1
        bounds, kk = table
        out = np.empty((src.shape[0], len(bounds), src.shape[2]), dtype=np.uint8)
        s32 = src.astype(np.int32)
        for xx, (x0, n) in enumerate(bounds.tolist()):
            acc = np.full((src.shape[0], src.shape[2]), 1 << 21, dtype=np.int32)
            for k in range(n):
                acc += s32[:, x0 + k] * np.int32(kk[xx, k])
            out[:, xx] = np.clip(acc >> 22, 0, 255)
        return out
    table = TL.resample_table(a.shape[0], d)
    mid = one_pass(a, table)
    return one_pass(mid.transpose(1, 0, 2), table).transpose(1, 0, 2)


@pytest.mark.parametrize('s,d', SIZES)
def test_table_reproduces_pil_resize(s, d):
    bounds, kk = TL.resample_table(s, d)
    support = 2.0 * max(s / d, 1.0)
    assert bounds.dtype == np.int32 and kk.dtype == np.int32
    assert bounds.shape == (d, 2) and kk.shape == (d, 2 * int(np.ceil(support)) + 1)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= s).all() and (bounds[:, 1] <= kk.shape[1]).all()
    for xx in range(d):
        assert not kk[xx, bounds[xx, 1]:].any()                 # zero-filled past n
    assert 255 * int(np.abs(kk.astype(np.int64)).sum(axis=1).max()) + (1 << 21) < 2 ** 31        # the 32-bit accumulator cannot overflow
    assert TL.resample_table(s, d)[1] is kk                     # cached per pair
    for name, a in (('noise', _noise(s)), ('smooth', _smooth_saturated(s))):
        ref = np.asarray(Image.fromarray(a).resize((d, d)))
        got = _apply_table(a, d)
        assert np.array_equal(got, ref), (name, int((got != ref).sum()))
        assert np.array_equal(TL.resample_apply(a, d), ref), name


def test_table_tap_counts():
    """n <= 4 when enlarging, 8 at 2 : 1, 16 at 4 : 1"""
    assert TL.resample_table(32, 64)[0][:, 1].max() <= 4 and TL.resample_table(48, 64)[0][:, 1].max() <= 4
    assert TL.resample_table(64, 32)[0][:, 1].max() == 8
    assert TL.resample_table(256, 64)[0][:, 1].max() == 16


# ---- the route -------------------------------------------------------------------------------------------------------------
class PilResampleBackend(fake_backend.FakeBackend):
    """the emulated backend plus the three resample entries, the resize done by PIL itself"""

    def tile_resample_supported(self, in_size, out_size):
        return in_size != out_size and max(in_size, out_size) <= 4 * min(in_size, out_size)

    def tile_gather_resampled(self, images, H0, W0, origins, tile, pad, pad_rgb, net, table, lut, out, strip_rows=0):
        self._count('tile_gather_resampled')
        assert tuple(table[0].shape) == (net, 2)
        out.zero_()
        for t, (ox, oy) in enumerate(origins.tolist()):
            for s, im in enumerate(images):
                px = np.asarray(Image.fromarray(self._tile_pixels(im, H0, W0, ox, oy, tile, pad, pad_rgb)).resize((net, net)))
                out[t, :, :, 3 * s:3 * s + 3] = lut[torch.from_numpy(px.astype('int64'))].to(out.dtype)

    def tile_paste_resampled(self, tiles, net, tile, table, rects, dst, strip_rows=0):
        self._count('tile_paste_resampled')
        assert tuple(table[0].shape) == (tile, 2) and tuple(tiles.shape[1:3]) == (net, net)
        for slot, l, t, w, h, px, py, rgb in rects.tolist():
            if slot < 0:
                dst[py:py + h, px:px + w] = torch.tensor([rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255], dtype=torch.uint8)
                continue
            u8 = (((tiles[slot, :, :, :3].float() + 1.0) * 0.5) * 255.0).to(torch.int32).to(torch.uint8).numpy()
            small = np.asarray(Image.fromarray(u8).resize((tile, tile)))
            dst[py:py + h, px:px + w] = torch.from_numpy(small[t:t + h, l:l + w].copy())


@pytest.fixture
def pil_backend():
    be = PilResampleBackend()
    ops._impl = be
    yield be
    fake_backend.uninstall()


def _opt(model='DeepLIIF', M=1, seg_gen=True, input_no=1):
    return types.SimpleNamespace(model=model, modalities_no=M, seg_gen=seg_gen, mod_id_seg='S', input_id=0, input_nc=3, output_nc=3, ngf=8,
                                 norm='batch', padding='zero', net_g='resnet_9blocks', net_gs='unet_32', input_no=input_no, scale_size=64,
                                 modalities_names=['IHC', 'Marker'], background_colors=[(201, 211, 208)], gpu_ids=[])


_NETS = {}


def _nets(opt):
    key = (opt.model, opt.input_no)
    if key not in _NETS:                                        # built once, shared, never modified
        torch.manual_seed(3)
        _NETS[key] = I.build_generators(opt, torch.device('cpu'), 'fp32')
    return _NETS[key]


def _host_route(img, tile, overlap, opt, nets, be, **kw):
    """inference() as the parent commit runs it: the backend without the resample entries -> _inference_resampled"""
    fake_backend.install()
    try:
        assert not I.region_resample_supported(tile, opt.scale_size)
        return I.inference(img, tile, overlap, None, opt=opt, nets=nets, batch_size=3, **kw)
    finally:
        ops._impl = be


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].size == b[k].size and np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


IMAGES = {'ragged': (150, 130), 'small': (40, 30)}               # ragged sides / smaller than one tile (mirror extension)


@pytest.mark.parametrize('tile', [48, 96])
@pytest.mark.parametrize('shape', sorted(IMAGES))
def test_region_route_equals_host_route(pil_backend, tile, shape):
    w, h = IMAGES[shape]
    a = synth_image(w, h, 11)
    if shape == 'ragged':
        a[:tile] = 250                                          # a row of empty tiles: constant colours through the resampled tiler
    img = Image.fromarray(a)
    opt = _opt()
    nets = _nets(opt)
    expect = _host_route(img, tile, tile // 16, opt, nets, pil_backend, return_seg_intermediate=True)
    n0 = dict(pil_backend.calls)
    got = I.inference(img, tile, tile // 16, None, opt=opt, nets=nets, batch_size=3, return_seg_intermediate=True)
    assert pil_backend.calls.get('tile_gather_resampled', 0) > n0.get('tile_gather_resampled', 0)
    assert pil_backend.calls.get('tile_paste_resampled', 0) > n0.get('tile_paste_resampled', 0)
    _same(got, expect)


def test_region_route_seg_only(pil_backend):
    img = Image.fromarray(synth_image(150, 130, 12))
    opt = _opt()
    nets = _nets(opt)
    expect = _host_route(img, 48, 3, opt, nets, pil_backend, seg_only=True)
    got = I.inference(img, 48, 3, None, opt=opt, nets=nets, batch_size=3, seg_only=True)
    assert 'Seg' in got
    _same(got, expect)


def test_region_route_two_inputs(pil_backend):
    """input_no = 2: the image is two modalities side by side, both cropped, resized and concatenated on the channel axis"""
    img = Image.fromarray(synth_image(2 * 110, 90, 13))
    opt = _opt('SDG', M=1, seg_gen=False, input_no=2)
    nets = _nets(opt)
    for tile in (48, 96):
        expect = _host_route(img, tile, tile // 16, opt, nets, pil_backend)
        got = I.inference(img, tile, tile // 16, None, opt=opt, nets=nets, batch_size=3)
        assert all(v.size == (110, 90) for v in got.values())
        _same(got, expect)


@pytest.mark.parametrize('world', [2, 3])
def test_region_route_bands_concatenate(pil_backend, world):
    a = synth_image(150, 130, 14)
    opt = _opt()
    nets = _nets(opt)
    full, band = I.infer_region([torch.from_numpy(a)], 48, 3, nets, opt, batch_size=3)
    assert band == (0, 130)
    parts = [I.infer_region([torch.from_numpy(a)], 48, 3, nets, opt, batch_size=3, rank=r, world=world) for r in range(world)]
    assert [p[1][0] for p in parts][1:] == [p[1][1] for p in parts][:-1] and parts[0][1][0] == 0 and parts[-1][1][1] == 130
    for k, v in full.items():
        cat = torch.cat([p[0][k] for p in parts if k in p[0]], dim=0)
        assert torch.equal(cat, v), k
    expect = _host_route(Image.fromarray(a), 48, 3, opt, nets, pil_backend, return_seg_intermediate=True)
    names = I._result_names(opt, full, False, False, True)
    for n, k in names.items():
        assert np.array_equal(full[k].numpy(), np.asarray(expect[n])), n


def test_unsupported_pair_keeps_the_host_route(pil_backend):
    """a ratio the backend declines (here > 4 : 1): infer_region raises as before, inference() falls back to the host route"""
    a = synth_image(20, 12, 15)
    opt = _opt()
    nets = _nets(opt)
    assert not I.region_resample_supported(8, 64)
    with pytest.raises(NotImplementedError):
        I.infer_region([torch.from_numpy(a)], 8, 0, nets, opt)
    n0 = pil_backend.calls.get('tile_gather_resampled', 0)
    got = I.inference(Image.fromarray(a), 8, 0, None, opt=opt, nets=nets, batch_size=3, mod_only=True)
    assert pil_backend.calls.get('tile_gather_resampled', 0) == n0
    _same(got, _host_route(Image.fromarray(a), 8, 0, opt, nets, pil_backend, mod_only=True))


def test_emulated_backend_keeps_the_host_route():
    """tests/fake_backend.py has no resample entries: every existing CPU test stays on its present route"""
    fake_backend.install()
    try:
        assert not I.region_resample_supported(48, 64)
        with pytest.raises(NotImplementedError):
            I.infer_region([torch.from_numpy(synth_image(60, 50, 1))], 48, 3, _nets(_opt()), _opt())
    finally:
        fake_backend.uninstall()
