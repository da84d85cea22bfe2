"""tile_size != scale_size: what inference() costs on a 20x slide.  A synthetic 4096 x 4096 image (noise: no tile is_empty) through the
full-size DeepLIIF (4 x Resnet-9block + 5 x UNet-512, ngf 64) in three configurations, each timed with events after a warm-up on a
smaller image:
    host   tile 256 / scale 512 through _inference_resampled (PIL on the host, one tile at a time: the only route before the GPU kernels)
    gpu    tile 256 / scale 512 through infer_region (dl_tile_gather_resample_u8 / dl_tile_paste_resample_u8)
    base   tile 512 / scale 512 (no resampling)
plus the two new kernels alone on a batch of 8 tiles, next to the plain gather / paste at 512.

    python tools/resample_time.py [--precision bf16] [--size 4096] [--out profiles/resample/resample_time.txt]
"""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def timed(fn):
    """(event ms, wall ms) of fn(), the device idle before and after"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def kernel_ms(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precision', default='bf16')
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--out', default=os.path.join('profiles', 'resample', 'resample_time.txt'))
    args = ap.parse_args()
    from PIL import Image
    from deepliif_amd import engine as E
    from deepliif_amd import inference as I
    from deepliif_amd import ops
    from deepliif_amd import tiling as TL
    dev = torch.device('cuda', 0)
    opt = types.SimpleNamespace(model='DeepLIIF', modalities_no=4, seg_gen=True, mod_id_seg='S', input_id=0, input_nc=3, output_nc=3, ngf=64,
                                norm='batch', padding='zero', net_g='resnet_9blocks', net_gs='unet_512', input_no=1, scale_size=512,
                                modalities_names=['IHC', 'Hema', 'DAPI', 'Lap2', 'Marker'], gpu_ids=[0])
    torch.manual_seed(0)
    nets = I.build_generators(opt, dev, args.precision)
    rng = np.random.RandomState(7)
    big = Image.fromarray(rng.randint(0, 256, (args.size, args.size, 3)).astype(np.uint8))
    small = Image.fromarray(rng.randint(0, 256, (1024, 1024, 3)).astype(np.uint8))
    gpu_supported = I.region_resample_supported
    lines = [f'resample_time: {args.size} x {args.size} noise image, DeepLIIF 4 x Resnet-9block + 5 x UNet-512 (ngf 64), precision {args.precision}, '
             f'batches of {args.batch} tiles, {torch.cuda.get_device_name(0)}', '']
    results = {}
    for tag, tile, route in (('host', 256, False), ('gpu', 256, True), ('base', 512, True)):
        I.region_resample_supported = gpu_supported if route else (lambda a, b: False)
        try:
            run = lambda img: I.inference(img, tile, tile // 16, None, opt=opt, nets=nets, batch_size=args.batch)
            run(small)                                               # warm-up: weight packing, allocator, table upload
            out, ev, wall = timed(lambda: run(big))
        finally:
            I.region_resample_supported = gpu_supported
        n = len(TL.TilePlan(args.size, args.size, tile, tile // 16))
        results[tag] = out
        lines.append(f'{tag:5s} tile {tile} / scale 512: {n:4d} tiles  events {ev:9.1f} ms  wall {wall:9.1f} ms  {n / (wall / 1e3):7.1f} tiles/s (wall)  '
                     f'{n / (ev / 1e3):7.1f} tiles/s (events)')
    same = all(np.array_equal(np.asarray(results['host'][k]), np.asarray(results['gpu'][k])) for k in results['host'])
    lines.append(f'host and gpu route return identical images: {same}')
    lines.append('')

    # the kernels alone: 8 tiles of a 4096 x 4096 image resident in HBM
    prec = E.Precision.get(args.precision)
    img = torch.from_numpy(np.asarray(big)).to(dev)
    with ops.half_mode(prec.half):
        for tile, net in ((256, 512), (512, 512)):
            rt = TL.RegionTiler([img], tile, tile // 16, net_size=net)
            ids = rt.tile_ids[:args.batch]
            be, pl = ops.impl(), rt.plan
            org = rt._origins_of(ids)
            x = torch.empty((len(ids), net, net, 8), dtype=prec.dtype, device=dev)
            rec = np.zeros((len(ids), 8), dtype=np.int32)
            rec[:, 0], rec[:, 1:7] = np.arange(len(ids)), rt._rects[ids]
            rects, dst = torch.from_numpy(rec).to(dev), rt.result('k')
            if tile != net:                      # the launches alone: every operand already on the device
                g = kernel_ms(lambda: be.tile_gather_resampled([img], pl.orig_height, pl.orig_width, org, tile, 0, rt.pad_rgb, net, rt._table_in, rt.lut, x))
                p = kernel_ms(lambda: be.tile_paste_resampled(x, net, tile, rt._table_out, rects, dst))
            else:
                g = kernel_ms(lambda: be.tile_gather([img], pl.orig_height, pl.orig_width, org, tile, 0, rt.pad_rgb, rt.lut, x))
                p = kernel_ms(lambda: be.tile_paste(x, tile, rects, dst))
            kind = 'dl_tile_gather_resample_u8 / dl_tile_paste_resample_u8' if tile != net else 'dl_tile_gather_u8 / dl_tile_paste_u8'
            lines.append(f'tile {tile} net {net} ({kind}), {len(ids)} tiles per call, {prec.dtype}: gather {g * 1e3 / len(ids):7.1f} us/tile  '
                         f'paste {p * 1e3 / len(ids):7.1f} us/tile  (one result image; a DeepLIIF tile pastes 10)')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
