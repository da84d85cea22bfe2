"""GPU parity of the resampled tile kernels (dl_tile_gather_resample_u8 / dl_tile_paste_resample_u8 / dl_tile_resample_supported,
through the C ABI of both libraries) and of inference() with tile_size != scale_size on top of them.  PIL's Image.resize is the oracle
of the resize, _inference_resampled (the host route) the oracle of the route.  Integer work throughout: every comparison is equality.

Strip heights: the library's own choice at net 64 is 32 rows (two strips per tile); the explicit heights 7, 5 and 24 give strip counts
that do not divide the height, so the last strip is short and every strip boundary lands on different vertical taps."""
import types

import numpy as np
import pytest
import torch
from PIL import Image

from fake_backend import FakeBackend
from golden_util import synth_image

pytestmark = pytest.mark.gpu
NET = 64
TILES = [48, 96, 61, 16, 32, 256]
HALVES = ['bf16', 'fp16']
PAD_RGB = 10 | (200 << 8) | (90 << 16)


def _resize(a, d):
    return np.asarray(Image.fromarray(a).resize((d, d)))


def _tensor2im(v):
    """deepliif/util/util.py:132-135 on float32 values"""
    return ((v.astype(np.float32) + 1) / 2.0 * 255.0).astype(np.uint8)


def _tables(TL, a, b, dev='cuda'):
    return tuple(torch.from_numpy(np.array(t)).to(dev) for t in TL.resample_table(a, b))


_GATHER_REF = {}


def _gather_case(tile, pad):
    """two source images, five origins (the four corners of the mirror-extended image and one inside) and the PIL reference, computed
    once per (tile, pad) and shared by both libraries"""
    if (tile, pad) not in _GATHER_REF:
        patch = tile - 2 * pad
        w, h = 2 * patch + 17, 2 * patch + 9
        imgs = [synth_image(w, h, 31 + tile), synth_image(w, h, 57 + tile)]
        origins = np.array([(0, 0), (w - patch, 0), (0, h - patch), (w - patch, h - patch), (patch // 2 + 3, patch // 3 + 1)], dtype=np.int32)
        ref = np.stack([np.concatenate([_resize(FakeBackend._tile_pixels(torch.from_numpy(im), h, w, int(ox), int(oy), tile, pad, PAD_RGB), NET) for im in imgs], axis=-1)
                        for ox, oy in origins])                                      # [5, NET, NET, 6] uint8
        _GATHER_REF[(tile, pad)] = (imgs, origins, ref)
    return _GATHER_REF[(tile, pad)]


def _check_gather(be, TL, imgs_dev, h, w, origins, tile, pad, ref, dtype, strip_rows):
    n_src = len(imgs_dev)
    cp = 8
    lut = torch.from_numpy(TL.transform_lut())
    out = torch.full((len(origins), NET, NET, cp), 7.0, dtype=dtype, device='cuda')
    be.tile_gather_resampled(imgs_dev, h, w, torch.from_numpy(origins).cuda(), tile, pad, PAD_RGB, NET, _tables(TL, tile, NET), lut.cuda(), out, strip_rows=strip_rows)
    got = out.cpu()
    exp = lut[torch.from_numpy(ref[..., :3 * n_src].astype(np.int64))].to(dtype)      # fp32: the lut value itself; 16-bit: lut[ref] cast to that type
    assert torch.equal(got[..., :3 * n_src], exp), (tile, pad, n_src, dtype, strip_rows, int((got[..., :3 * n_src] != exp).sum()))
    assert (got[..., 3 * n_src:] == 0).all()


@pytest.mark.parametrize('half', HALVES)
@pytest.mark.parametrize('tile', TILES)
def test_gather_resample_matches_pil(tile, half):
    from deepliif_amd import ops
    from deepliif_amd import tiling as TL
    h16 = ops.H16_DTYPE[half]
    with ops.half_mode(half):
        be = ops.impl()
        for pad in (0, 3):
            imgs, origins, ref = _gather_case(tile, pad)
            h, w = imgs[0].shape[:2]
            dev = [torch.from_numpy(im).cuda() for im in imgs]
            for n_src in (1, 2):
                _check_gather(be, TL, dev[:n_src], h, w, origins, tile, pad, ref, torch.float32, 7)       # 10 strips, the last of 1 row
                _check_gather(be, TL, dev[:n_src], h, w, origins, tile, pad, ref, h16, 24)               # 3 strips, the last of 16 rows
            _check_gather(be, TL, dev, h, w, origins, tile, pad, ref, h16, 0)                            # the library's strips (2 x 32 rows)
        torch.cuda.synchronize()


@pytest.mark.parametrize('half', HALVES)
def test_gather_resample_image_smaller_than_a_patch(half):
    """an image narrower and lower than the patch: the mirror extension is read through the resize"""
    from deepliif_amd import ops
    from deepliif_amd import tiling as TL
    img = synth_image(20, 15, 77)
    with ops.half_mode(half):
        be = ops.impl()
        for tile, pad in ((48, 0), (48, 3), (96, 0)):
            origins = np.zeros((1, 2), dtype=np.int32)
            ref = _resize(FakeBackend._tile_pixels(torch.from_numpy(img), 15, 20, 0, 0, tile, pad, PAD_RGB), NET)[None]
            for dtype, strips in ((torch.float32, 5), (ops.H16_DTYPE[half], 0)):
                _check_gather(be, TL, [torch.from_numpy(img).cuda()], 15, 20, origins, tile, pad, ref, dtype, strips)


def _ulp_neighbours(x):
    """x and its two neighbours in x's own number format"""
    it = torch.int32 if x.dtype == torch.float32 else torch.int16
    iv = x.contiguous().view(it)
    return torch.stack([(iv - 1).view(x.dtype), x, (iv + 1).view(x.dtype)])


def _paste_inputs(dtype):
    """[3, NET, NET, 8]: random activations in [-1, 1]; exact +-1; values one ulp either side of the byte boundaries of tensor2im"""
    g = torch.Generator().manual_seed(5)
    x = torch.zeros(3, NET, NET, 8, dtype=torch.float32)
    x[0, :, :, :3] = torch.rand(NET, NET, 3, generator=g) * 2 - 1
    x[1, :, :, :3] = (torch.rand(NET, NET, 3, generator=g) < 0.5).float() * 2 - 1
    x = x.to(dtype)
    b = torch.arange(1, 256, dtype=torch.float32)
    edge = _ulp_neighbours((b * 2 / 255 - 1).to(dtype)).reshape(-1)                 # (x + 1) / 2 * 255 == b, and a step to either side
    edge = edge[torch.randperm(edge.numel(), generator=g)]
    flat = edge.repeat(NET * NET * 3 // edge.numel() + 1)[:NET * NET * 3]
    x[2, :, :, :3] = flat.reshape(NET, NET, 3)
    return x


@pytest.mark.parametrize('half', HALVES)
@pytest.mark.parametrize('tile', TILES)
def test_paste_resample_matches_pil(tile, half):
    from deepliif_amd import ops
    from deepliif_amd import tiling as TL
    for dtype, strips in ((torch.float32, 5), (ops.H16_DTYPE[half], 24), (torch.float32, 0)):
        x = _paste_inputs(dtype)
        small = [_resize(_tensor2im(x[i, :, :, :3].float().numpy()), tile) for i in range(3)]
        a, b = max(tile // 3, 1), max(tile // 4, 1)
        # {slot, l, t, w, h, px, py, rgb}: the whole tile (every edge), a constant colour, the top-left corner, the bottom-right corner,
        # an inner window, windows along the right and the bottom edge
        recs = [(0, 0, 0, tile, tile, 3, 2, 0),
                (-1, 0, 0, a, b, tile + 5, 1, PAD_RGB),
                (1, 0, 0, a, b, tile + 5, b + 3, 0),
                (2, tile - a, tile - b, a, b, tile + 5, 2 * b + 5, 0),
                (1, 1, 2, tile - 3, 1, 3, tile + 4, 0),
                (2, tile - 1, 0, 1, tile, 0, 2, 0),
                (2, 0, tile - 1, tile, 1, 3, tile + 6, 0)]
        H, W = tile + 8, 2 * tile + 8
        exp = np.zeros((H, W, 3), dtype=np.uint8)
        for slot, l, t, w, h, px, py, rgb in recs:
            exp[py:py + h, px:px + w] = [rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255] if slot < 0 else small[slot][t:t + h, l:l + w]
        wide = torch.zeros((H, W + 5, 3), dtype=torch.uint8, device='cuda')
        dst = wide[:, :W]                                                             # row stride != 3 * width
        with ops.half_mode(half):
            ops.impl().tile_paste_resampled(x.cuda(), NET, tile, _tables(TL, NET, tile), torch.tensor(recs, dtype=torch.int32).cuda(), dst, strip_rows=strips)
        got = wide.cpu().numpy()
        assert np.array_equal(got[:, :W], exp), (tile, dtype, strips, int((got[:, :W] != exp).sum()))
        assert not got[:, W:].any()


@pytest.mark.parametrize('half', HALVES)
@pytest.mark.parametrize('tile,net,n_src', [(256, 512, 1), (1024, 512, 1), (2048, 1024, 2)])
def test_full_size_round_trip(tile, net, n_src, half):
    """the LDS budget at the real widths, with the strips the library chooses: one tile up / down to the network and back"""
    from deepliif_amd import ops
    from deepliif_amd import tiling as TL
    rng = np.random.RandomState(tile)
    imgs = [rng.randint(0, 256, (tile, tile, 3)).astype(np.uint8) for _ in range(n_src)]
    lut = torch.from_numpy(TL.transform_lut())
    dtype = torch.float32 if n_src == 1 else ops.H16_DTYPE[half]
    with ops.half_mode(half):
        be = ops.impl()
        assert be.tile_resample_supported(tile, net) and be.tile_resample_supported(net, tile)
        out = torch.empty((1, net, net, 8), dtype=dtype, device='cuda')
        be.tile_gather_resampled([torch.from_numpy(a).cuda() for a in imgs], tile, tile, torch.zeros((1, 2), dtype=torch.int32, device='cuda'), tile, 0, 0, net,
                                 _tables(TL, tile, net), lut.cuda(), out)
        ref = np.concatenate([_resize(a, net) for a in imgs], axis=-1)
        assert torch.equal(out[0, :, :, :3 * n_src].cpu(), lut[torch.from_numpy(ref.astype(np.int64))].to(dtype))
        if n_src > 1:
            return
        x = torch.zeros((1, net, net, 8), dtype=torch.float32)
        x[0, :, :, :3] = torch.from_numpy(rng.uniform(-1, 1, (net, net, 3)).astype(np.float32))
        dst = torch.zeros((tile, tile, 3), dtype=torch.uint8, device='cuda')
        be.tile_paste_resampled(x.cuda(), net, tile, _tables(TL, net, tile), torch.tensor([(0, 0, 0, tile, tile, 0, 0, 0)], dtype=torch.int32).cuda(), dst)
        assert np.array_equal(dst.cpu().numpy(), _resize(_tensor2im(x[0, :, :, :3].numpy()), tile))


@pytest.mark.parametrize('half', HALVES)
def test_resample_supported(half):
    from deepliif_amd import ops
    with ops.half_mode(half):
        be = ops.impl()
        for tile in (128, 256, 384, 640, 1024):
            assert be.tile_resample_supported(tile, 512) and be.tile_resample_supported(512, tile), tile
        for tile in (512, 2048):
            assert be.tile_resample_supported(tile, 1024) and be.tile_resample_supported(1024, tile), tile
        assert not be.tile_resample_supported(8192, 512)
        assert not be.tile_resample_supported(512, 512)


def test_bad_arguments_are_refused():
    from deepliif_amd import _lib as L
    from deepliif_amd import ops
    from deepliif_amd import tiling as TL
    be = ops.impl()
    img = torch.zeros((64, 64, 3), dtype=torch.uint8, device='cuda')
    org = torch.zeros((1, 2), dtype=torch.int32, device='cuda')
    lut = torch.from_numpy(TL.transform_lut()).cuda()
    out = torch.zeros((1, NET, NET, 8), device='cuda')
    good = _tables(TL, 48, NET)
    other = _tables(TL, 96, NET)                                                     # ksize 7: not the table of 48 -> 64
    with pytest.raises(L.HipLibraryError, match='ksize'):
        be.tile_gather_resampled([img], 64, 64, org, 48, 0, 0, NET, other, lut, out)
    with pytest.raises(L.HipLibraryError, match='pad'):
        be.tile_gather_resampled([img], 64, 64, org, 48, 24, 0, NET, good, lut, out)
    with pytest.raises(L.HipLibraryError, match='channel geometry'):
        be.tile_gather_resampled([img, img, img], 64, 64, org, 48, 0, 0, NET, good, lut, out)            # 9 channels into Cp = 8
    with pytest.raises(L.HipLibraryError, match='LDS'):
        big = torch.zeros((1, 512, 512, 8), device='cuda')
        be.tile_gather_resampled([img], 64, 64, org, 256, 0, 0, 512, _tables(TL, 256, 512), lut, big, strip_rows=512)
    torch.cuda.synchronize()


# ---- the route -------------------------------------------------------------------------------------------------------------
def _opt():
    return types.SimpleNamespace(model='DeepLIIF', modalities_no=2, seg_gen=True, mod_id_seg='S', input_id=0, input_nc=3, output_nc=3, ngf=8,
                                 norm='batch', padding='zero', net_g='resnet_9blocks', net_gs='unet_64', input_no=1, scale_size=64,
                                 modalities_names=['input1', 'mod1', 'mod2'], background_colors=[(201, 211, 208), (10, 10, 10)], gpu_ids=[0])


_NETS = {}


def _nets(precision):
    from deepliif_amd import inference as I
    if precision not in _NETS:                                                        # built once per precision, shared, never modified
        torch.manual_seed(6)
        _NETS[precision] = I.build_generators(_opt(), torch.device('cuda', 0), precision)
    return _NETS[precision]


def _images(tile):
    ragged = synth_image(150, 130, 41)
    blank = synth_image(150, 130, 42)
    blank[:tile + 4] = 246                                                            # the first tile row sees background only: empty tiles are pasted
    return {'ragged': ragged, 'blank': blank, 'small': synth_image(40, 30, 43)}


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
@pytest.mark.parametrize('tile', [48, 96])
def test_inference_gpu_route_equals_host_route(tile, precision, monkeypatch):
    from deepliif_amd import inference as I
    opt, nets = _opt(), _nets(precision)
    assert I.region_resample_supported(tile, NET)
    for name, a in _images(tile).items():
        img = Image.fromarray(a)
        got = I.inference(img, tile, tile // 16, None, opt=opt, nets=nets, return_seg_intermediate=True, batch_size=4)
        with monkeypatch.context() as m:
            m.setattr(I, 'region_resample_supported', lambda a_, b_: False)           # the parent commit's route: _inference_resampled
            expect = I.inference(img, tile, tile // 16, None, opt=opt, nets=nets, return_seg_intermediate=True, batch_size=4)
        assert list(got) == list(expect) and len(got) == 6
        for k in got:
            assert got[k].size == img.size
            assert np.array_equal(np.asarray(got[k]), np.asarray(expect[k])), (name, k, int((np.asarray(got[k]) != np.asarray(expect[k])).sum()))


def test_infer_region_accepts_resampled_tiles_and_bands_concatenate():
    from deepliif_amd import inference as I
    opt, nets = _opt(), _nets('fp32')
    a = _images(48)['blank']
    full, band = I.infer_region([torch.from_numpy(a).cuda()], 48, 3, nets, opt, batch_size=4)
    assert band == (0, 130) and all(tuple(v.shape) == (130, 150, 3) for v in full.values())
    parts = [I.infer_region([torch.from_numpy(a).cuda()], 48, 3, nets, opt, batch_size=4, rank=r, world=3) for r in range(3)]
    for k, v in full.items():
        assert torch.equal(torch.cat([p[0][k] for p in parts], dim=0), v), k


def test_unsupported_pair_falls_back_to_the_host_route(monkeypatch):
    """64 -> 2100 does not fit the LDS budget: inference() takes the host route, infer_region raises as before"""
    from deepliif_amd import inference as I
    from deepliif_amd import ops
    opt, nets = _opt(), _nets('fp32')
    assert not I.region_resample_supported(2100, NET)
    img = Image.fromarray(synth_image(40, 30, 44))
    with pytest.raises(NotImplementedError):
        I.infer_region([torch.from_numpy(np.asarray(img)).cuda()], 2100, 0, nets, opt)
    called = []
    monkeypatch.setattr(type(ops.impl()), 'tile_gather_resampled', lambda self, *a, **k: called.append(1))
    got = I.inference(img, 2100, 0, None, opt=opt, nets=nets, mod_only=True)
    assert not called
    expect = I._inference_resampled([img], 2100, 0, nets, opt, False, True, None, 8, NET)
    names = I._result_names(opt, expect, False, True, False)
    assert list(got) == list(names)
    for n, k in names.items():
        assert np.array_equal(np.asarray(got[n]), np.asarray(expect[k])), n
