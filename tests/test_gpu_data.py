"""GPU parity of dl_train_gather_u8 / dl_train_gather_supported (through the C ABI of both libraries, fp32 and both 16-bit output types) and
of the loader + set_input on top of them, against tests/data_ref.py: PIL's own convert / resize / crop / transpose followed by the float32
normalisation.  Integer arithmetic and a table lookup throughout: every comparison is equality, there is no tolerance.

Shapes: the smallest at which each path of the kernels is taken -- both resize passes with different tables, one pass only, none (the
plain kernel), a crop window inside / at the far corner of / equal to the resized panel, flips mixed within a batch, strips of one row and
strips that do not divide the window, a second panel at channel offset 3, a row stride wider than the row."""
import os
import random
import types

import numpy as np
import pytest
import torch
from PIL import Image

import data_ref
from golden_util import synth_image

pytestmark = pytest.mark.gpu
HALVES = ['bf16', 'fp16']


def _backend(half):
    from deepliif_amd import ops
    return ops, ops.H16_DTYPE[half]


_ROWS = {}


def _row(num_img, w2, h, seed):
    key = (num_img, w2, h, seed)
    if key not in _ROWS:
        _ROWS[key] = synth_image(num_img * w2, h, seed)
    return _ROWS[key]


_REF = {}


def _reference(rows_key, rows, w2, panel, gray, mode, load, crop, params):
    """uint8 [n, ch, cw, nch]: the PIL chain of data_ref on panel `panel` of every row; computed once per case and shared by libraries and dtypes"""
    key = (rows_key, w2, panel, gray, mode, load, crop, tuple(params))
    if key not in _REF:
        out = []
        for a, (x, y, flip) in zip(rows, params):
            img = Image.fromarray(a).crop((w2 * panel, 0, w2 * (panel + 1), a.shape[0]))
            r = np.asarray(data_ref.transform_pil(img, mode, load, crop, False, {'crop_pos': (x, y), 'flip': flip}, grayscale=gray))
            out.append(r[:, :, None] if r.ndim == 2 else r)
        _REF[key] = np.stack(out)
    return _REF[key]


def _run(be, dtype, rows, w2, panel, gray, mode, load, crop, params, strip_rows=0, cp=8, c0=0, zero_to=None, out=None, row_pad=0, rows_key=None):
    """one dl_train_gather_u8 call for a reference configuration; returns (out on the host, expected values of its channels)"""
    from deepliif_amd import data as D
    h = rows[0].shape[0]
    ref = _reference(rows_key, rows, w2, panel, gray, mode, load, crop, params)
    n, ch, cw, nch = ref.shape
    new = D.resized_size(mode, load, crop, (w2, h))
    win = [D.crop_window(mode, crop, new, (x, y)) for x, y, _ in params]
    assert all(w[2:] == (cw, ch) for w in win), (win, ref.shape)
    tables = tuple(None if tb is None else tuple(torch.from_numpy(np.array(a)).cuda() for a in tb) for tb in D.axis_tables((w2, h), new))
    dev = []
    for a in rows:
        wide = torch.zeros((h, a.shape[1] + row_pad, 3), dtype=torch.uint8, device='cuda')
        wide[:, :a.shape[1]] = torch.from_numpy(a).cuda()
        dev.append(wide[:, :a.shape[1]])                                             # row stride 3 * (w + row_pad)
    rec = torch.tensor([[w[0], w[1], int(p[2])] for w, p in zip(win, params)], dtype=torch.int32).cuda()
    lut = D.normalize_lut()
    if out is None:
        out = torch.full((n, ch, cw, cp), 7.0, dtype=dtype, device='cuda')
    assert be.train_gather_supported(w2, h, new[0], new[1], ch, cw) > 0
    be.train_gather(dev, w2, h, panel, gray, new, tables, rec, lut.cuda(), out, c0, cp if zero_to is None else zero_to, strip_rows=strip_rows)
    torch.cuda.synchronize()
    exp = lut[torch.from_numpy(ref.astype(np.int64))].to(dtype)
    return out, exp


def _check(be, dtype, rows, w2, panel, gray, mode, load, crop, params, rows_key, **kw):
    out, exp = _run(be, dtype, rows, w2, panel, gray, mode, load, crop, params, rows_key=rows_key, **kw)
    got = out.cpu()
    nch = exp.shape[3]
    assert torch.equal(got[..., :nch], exp), (mode, w2, dtype, kw, int((got[..., :nch] != exp).sum()))
    assert (got[..., nch:] == 0).all()


def _rows3(w2, h, seed):
    return [_row(4, w2, h, seed + i) for i in range(3)], ('r3', w2, h, seed)


# (mode, load, crop, panel size, per-sample (crop_x, crop_y, flip))
CASES = {
    'upscale_nonsquare': ('resize_and_crop', 24, 16, (20, 12), [(0, 0, False), (8, 8, True), (3, 5, False)]),
    'upscale_nonsquare_flipped': ('resize_and_crop', 24, 16, (20, 12), [(0, 0, True), (8, 8, False), (3, 5, True)]),
    'downscale_ksize11': ('resize_and_crop', 16, 12, (40, 40), [(0, 0, False), (4, 4, True), (1, 3, True)]),
    'vertical_pass_only': ('resize_and_crop', 16, 16, (16, 12), [(0, 0, False), (0, 0, True), (0, 0, False)]),
    'horizontal_pass_only': ('resize_and_crop', 16, 12, (20, 16), [(0, 0, False), (4, 4, True), (2, 1, True)]),
    'crop_far_corner': ('crop', 16, 8, (20, 12), [(12, 4, False), (12, 4, True), (0, 0, True)]),
    'crop_is_the_image': ('crop', 8, 8, (8, 8), [(0, 0, False), (0, 0, True), (0, 0, False)]),
    'no_preprocess': (None, 16, 8, (18, 14), [(0, 0, True), (0, 0, False), (0, 0, True)]),
    # 'none' rounds to a multiple of 4 with Python's round (half to even): 18 x 14 -> 16 x 16 (4.5 -> 4, 3.5 -> 4); 19 x 14 -> 20 x 16
    'none_18x14': ('none', 16, 8, (18, 14), [(0, 0, False), (0, 0, True), (0, 0, True)]),
    'none_19x14': ('none', 16, 8, (19, 14), [(0, 0, True), (0, 0, False), (0, 0, True)]),
    'scale_width': ('scale_width', 16, 8, (20, 12), [(0, 0, False), (0, 0, True), (0, 0, True)]),
    'scale_width_and_crop': ('scale_width_and_crop', 16, 8, (20, 12), [(0, 0, False), (8, 0, True), (5, 0, True)]),
}


@pytest.mark.parametrize('half', HALVES)
@pytest.mark.parametrize('name', sorted(CASES))
def test_gather_matches_pil(name, half):
    ops, h16 = _backend(half)
    mode, load, crop, (w2, h), params = CASES[name]
    rows, key = _rows3(w2, h, 40)
    with ops.half_mode(half):
        be = ops.impl()
        for dtype in (torch.float32, h16):
            for panel in (0, 2):
                _check(be, dtype, rows, w2, panel, False, mode, load, crop, params, key)


@pytest.mark.parametrize('half', HALVES)
@pytest.mark.parametrize('name', ['upscale_nonsquare', 'downscale_ksize11', 'crop_far_corner', 'vertical_pass_only'])
def test_gray_output(name, half):
    """input_nc = 1: convert('L') BEFORE the resize, one channel out, seven zeroed"""
    ops, h16 = _backend(half)
    mode, load, crop, (w2, h), params = CASES[name]
    rows, key = _rows3(w2, h, 40)
    with ops.half_mode(half):
        be = ops.impl()
        for dtype in (torch.float32, h16):
            _check(be, dtype, rows, w2, 1, True, mode, load, crop, params, key)


@pytest.mark.parametrize('half', HALVES)
@pytest.mark.parametrize('name', ['upscale_nonsquare', 'crop_far_corner'])
def test_two_input_panels_in_one_activation(name, half):
    """panels 0 and 1 at channel offsets 0 and 3 of a Cp = 8 activation: the second call zeroes the pad channels, neither touches the other's slice"""
    ops, h16 = _backend(half)
    mode, load, crop, (w2, h), params = CASES[name]
    rows, key = _rows3(w2, h, 40)
    with ops.half_mode(half):
        be = ops.impl()
        for dtype in (torch.float32, h16):
            out, e0 = _run(be, dtype, rows, w2, 0, False, mode, load, crop, params, c0=0, zero_to=3, rows_key=key)
            assert (out.cpu()[..., 3:] == 7.0).all()                                 # nothing past its three channels yet
            out, e1 = _run(be, dtype, rows, w2, 1, False, mode, load, crop, params, c0=3, zero_to=8, out=out, rows_key=key)
            got = out.cpu()
            assert torch.equal(got[..., 0:3], e0) and torch.equal(got[..., 3:6], e1) and (got[..., 6:] == 0).all()
            # gray panels: channels 0 and 1, the rest of the group zeroed by the second call
            out, g0 = _run(be, dtype, rows, w2, 0, True, mode, load, crop, params, c0=0, zero_to=1, rows_key=key)
            out, g1 = _run(be, dtype, rows, w2, 1, True, mode, load, crop, params, c0=1, zero_to=8, out=out, rows_key=key)
            got = out.cpu()
            assert torch.equal(got[..., 0:1], g0) and torch.equal(got[..., 1:2], g1) and (got[..., 2:] == 0).all()


@pytest.mark.parametrize('half', HALVES)
@pytest.mark.parametrize('name', ['upscale_nonsquare', 'downscale_ksize11', 'crop_far_corner'])
def test_source_row_stride(name, half):
    ops, h16 = _backend(half)
    mode, load, crop, (w2, h), params = CASES[name]
    rows, key = _rows3(w2, h, 40)
    with ops.half_mode(half):
        _check(ops.impl(), h16, rows, w2, 3, False, mode, load, crop, params, key, row_pad=5)


@pytest.mark.parametrize('half', HALVES)
@pytest.mark.parametrize('name', ['upscale_nonsquare', 'downscale_ksize11', 'vertical_pass_only', 'horizontal_pass_only', 'scale_width'])
def test_strip_rows(name, half):
    """strips of one row, and strips that do not divide the window (16 = 3 * 5 + 1, 12 = 2 * 5 + 2, 9 = 5 + 4): every strip boundary lands on other taps"""
    ops, h16 = _backend(half)
    mode, load, crop, (w2, h), params = CASES[name]
    rows, key = _rows3(w2, h, 40)
    with ops.half_mode(half):
        be = ops.impl()
        _check(be, torch.float32, rows, w2, 1, False, mode, load, crop, params, key, strip_rows=1)
        _check(be, h16, rows, w2, 1, False, mode, load, crop, params, key, strip_rows=5)


@pytest.mark.parametrize('half', HALVES)
def test_more_samples_than_one_launch(half):
    """17 samples: the row pointers travel as kernel arguments, 16 per launch"""
    ops, h16 = _backend(half)
    mode, load, crop, (w2, h), _ = CASES['upscale_nonsquare']
    rows = [_row(4, w2, h, 60 + i) for i in range(17)]
    params = [((3 * i) % 9, (5 * i) % 9, bool(i % 2)) for i in range(17)]
    with ops.half_mode(half):
        _check(ops.impl(), h16, rows, w2, 1, False, mode, load, crop, params, ('r17', w2, h))
        _check(ops.impl(), h16, rows, w2, 1, False, 'crop', 16, 8, [(x, y // 2, f) for x, y, f in params], ('r17', w2, h))


def _wide_case():
    """a 1030 x 40 panel resized to 1024 x 40 (horizontal pass only): strips of R rows need 4096 * R bytes of LDS -- 16 rows are exactly the 64 KB"""
    a = synth_image(1030, 40, 77)
    ref = np.asarray(Image.fromarray(a).resize((1024, 40), Image.BICUBIC))
    return a, ref


@pytest.mark.parametrize('half', HALVES)
def test_strip_rows_too_large_fails_cleanly(half):
    from deepliif_amd import _lib as L
    from deepliif_amd import data as D
    ops, h16 = _backend(half)
    a, ref = _wide_case()
    with ops.half_mode(half):
        be = ops.impl()
        tables = (tuple(torch.from_numpy(np.array(t)).cuda() for t in D.axis_tables((1030, 40), (1024, 40))[0]), None)
        rec = torch.zeros((1, 3), dtype=torch.int32, device='cuda')
        lut = D.normalize_lut()
        out = torch.full((1, 40, 1024, 8), 7.0, dtype=h16, device='cuda')
        args = ([torch.from_numpy(a).cuda()], 1030, 40, 0, False, (1024, 40), tables, rec, lut.cuda(), out, 0, 8)
        with pytest.raises(L.HipLibraryError, match='LDS'):
            be.train_gather(*args, strip_rows=17)
        with pytest.raises(L.HipLibraryError, match='strips of 41 rows'):
            be.train_gather(*args, strip_rows=41)
        torch.cuda.synchronize()
        assert (out == 7.0).all()                                                    # nothing was launched
        assert be.train_gather_supported(1030, 40, 1024, 40, 40, 1024) == 16        # the library's own choice stops at the budget
        for strip in (16, 0):
            out.fill_(7.0)
            be.train_gather(*args, strip_rows=strip)
            got = out.cpu()
            assert torch.equal(got[0, :, :, :3], lut[torch.from_numpy(ref.astype(np.int64))].to(h16)) and (got[..., 3:] == 0).all()


@pytest.mark.parametrize('half', HALVES)
def test_supported_is_zero_exactly_where_the_call_fails(half):
    from deepliif_amd import _lib as L
    from deepliif_amd import data as D
    ops, h16 = _backend(half)
    # (panel w2 x h, new size, crop window ch x cw, supported?)
    geos = [((40, 4000), (40, 16), (16, 32), False),          # 4000 -> 16 rows: ksize 1001 source rows of 32 words = 128 128 bytes for ONE output row
            ((40, 1500), (40, 16), (16, 40), True),           # ksize 377 rows of 40 words = 60 320 bytes: fits with one row per strip
            ((20, 12), (24, 24), (25, 16), False),            # window higher than the resized panel
            ((20, 12), (24, 24), (16, 25), False),            # ... wider
            ((20, 12), (24, 24), (24, 24), True),
            ((20, 12), (20, 12), (12, 20), True),             # no resize
            ((20, 12), (20, 12), (13, 20), False),
            ((20, 12), (24, 0), (1, 1), False)]               # empty
    with ops.half_mode(half):
        be = ops.impl()
        lut = D.normalize_lut().cuda()
        rec = torch.zeros((1, 3), dtype=torch.int32, device='cuda')
        for (w2, h), new, (ch, cw), ok in geos:
            sup = be.train_gather_supported(w2, h, new[0], new[1], ch, cw)
            assert (sup > 0) == ok, ((w2, h), new, (ch, cw), sup)
            if not ok:
                assert be.train_gather_limit()                                       # says why
            tables = tuple(None if tb is None else tuple(torch.from_numpy(np.array(a)).cuda() for a in tb)
                           for tb in (D.axis_tables((w2, h), new) if min(new) > 0 else (None, None)))
            row = torch.from_numpy(synth_image(w2, h, 5)).cuda()
            out = torch.full((1, ch, cw, 8), 7.0, dtype=h16, device='cuda')
            if ok:
                be.train_gather([row], w2, h, 0, False, new, tables, rec, lut, out, 0, 8)
                torch.cuda.synchronize()
                ref = np.asarray(Image.fromarray(synth_image(w2, h, 5)).resize(new, Image.BICUBIC))[:ch, :cw]
                assert torch.equal(out.cpu()[0, :, :, :3], lut.cpu()[torch.from_numpy(ref.astype(np.int64))].to(h16))
            else:
                with pytest.raises(L.HipLibraryError):
                    be.train_gather([row], w2, h, 0, False, new, tables, rec, lut, out, 0, 8)
                torch.cuda.synchronize()
                assert (out == 7.0).all()


def test_table_for_an_unchanged_axis_is_refused():
    from deepliif_amd import _lib as L
    from deepliif_amd import data as D
    from deepliif_amd import ops
    be = ops.impl()
    from deepliif_amd.tiling import resample_table
    tb = tuple(torch.from_numpy(np.array(a)).cuda() for a in resample_table(20, 20))        # a well-formed table of a pass Pillow would skip
    ty = tuple(torch.from_numpy(np.array(a)).cuda() for a in D.axis_tables((20, 12), (24, 24))[1])
    row = torch.from_numpy(synth_image(20, 12, 5)).cuda()
    rec = torch.zeros((1, 3), dtype=torch.int32, device='cuda')
    out = torch.zeros((1, 24, 24, 8), device='cuda')
    with pytest.raises(L.HipLibraryError, match='needs a table'):
        be.train_gather([row], 20, 12, 0, False, (24, 24), (None, ty), rec, D.normalize_lut().cuda(), out, 0, 8)
    out = torch.zeros((1, 12, 20, 8), device='cuda')
    with pytest.raises(L.HipLibraryError, match='takes no table'):
        be.train_gather([row], 20, 12, 0, False, (20, 12), (tb, None), rec, D.normalize_lut().cuda(), out, 0, 8)


# ---- model level: a loader batch against the same images through data_ref -> tensors -> set_input
def _model_opt(precision, root):
    return types.SimpleNamespace(
        model='DeepLIIF', name='data', checkpoints_dir=os.path.join(str(root), 'ckpt'), gpu_ids=[0], is_train=True, phase='train', continue_train=False,
        modalities_no=1, seg_gen=True, modalities_names=[], input_nc=3, input_no=1, output_nc=3, ngf=8, ndf=8, net_g='resnet_9blocks',
        net_gs='resnet_9blocks', net_d='n_layers', n_layers_D=2, norm='batch', no_dropout=True, init_type='normal', init_gain=0.02, padding='zero',
        upsample='convtranspose', gan_mode='vanilla', gan_mode_s='lsgan', optimizer='adam', lr_g=2e-4, lr_d=2e-4, beta1=0.5, lr_policy='linear',
        n_epochs=100, n_epochs_decay=100, epoch_count=0, seg_weights=[0.5, 0.5], loss_G_weights=[0.5, 0.5], loss_D_weights=[0.5, 0.5],
        lambda_L1=100.0, verbose=False, epoch='latest', load_iter=0, precision=precision,
        # the loader's options
        dataroot=str(root), dataset_mode='aligned', preprocess='resize_and_crop', load_size=36, crop_size=32, direction='AtoB', no_flip=False,
        seg_no=1, max_dataset_size=None, serial_batches=True, num_threads=2, batch_size=2)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_loader_batch_equals_tensor_batch_in_the_model(precision, tmp_path):
    from deepliif_amd import data as D
    from deepliif_amd import models as M
    opt = _model_opt(precision, tmp_path)
    d = os.path.join(str(tmp_path), 'train')
    os.makedirs(d)
    paths = []
    for i in range(4):
        paths.append(os.path.join(d, f'row_{i}.png'))
        Image.fromarray(synth_image(3 * 40, 40, 90 + i)).save(paths[-1])
    random.seed(17)
    samples = [data_ref.getitem(Image.open(p), opt, p) for p in paths]
    exp = [data_ref.collate(samples[i:i + 2]) for i in (0, 2)]
    random.seed(17)
    loader = D.create_dataset(opt)
    got = list(loader.load_data())
    assert len(got) == 2 and got[1]['A_paths'] == paths[2:]

    def fresh():
        torch.manual_seed(0)
        m = M.create_model(opt)
        m.setup(opt)
        return m
    ma, mb = fresh(), fresh()
    for k in range(2):
        ma.set_input(got[k])
        mb.set_input({'A': exp[k]['A'].cuda(), 'B': [b.cuda() for b in exp[k]['B']], 'A_paths': exp[k]['A_paths']})
        assert ma._A.t.dtype == mb._A.t.dtype and torch.equal(ma._A.t, mb._A.t)
        assert len(ma._B) == len(mb._B) == 1 and torch.equal(ma._B[0].t, mb._B[0].t) and torch.equal(ma._Bseg.t, mb._Bseg.t)
        if precision == 'fp32':
            assert torch.equal(ma.real_A, mb.real_A) and torch.equal(ma.real_B_1, mb.real_B_1)
    ma.optimize_parameters()
    mb.optimize_parameters()
    torch.cuda.synchronize()
    la, lb = ma.get_current_losses(), mb.get_current_losses()
    assert la == lb and all(np.isfinite(v) for v in la.values()), (la, lb)
