"""What does building the training batch on the GPU cost against handing set_input() the reference loader's tensors?  At batch 8, 1 + 5 panels, 512 x 512,
alternated `--rounds` times in ONE process after warm-up, a device synchronise either side of every window (wall clock: the host's share is the point):
    (A) the parent path: pageable fp32 NCHW tensors -> set_input (host-to-device copies + one dl_nchw_to_nhwc per tensor)
    (B) pinned uint8 rows -> host-to-device copy on the side stream -> dl_train_gather_u8 per panel -> set_input(engine.Act batch);
        the loader's own code (deepliif_amd.data: _upload + _launch), decode excluded (the rows are decoded once, before the windows)
plus the device time of (B)'s six kernel launches against their byte bound (bytes read + written, from shapes, over the measured HBM copy rate of an
MI355X, 6.29 TB/s) for the plain path and for a resize (572 -> 512 on both axes, then a 512 crop: `--preprocess resize_and_crop`), and the single-thread
CPU time of the PIL chain per sample (tests/data_ref.py) for context.  Writes <out> (default profiles/data_pipeline.json) and prints it.

The GPU work runs in a child process under its own time limit (--timeout seconds).

    python tools/data_pipeline_ab.py [--rounds 5] [--iters 10] [--timeout 600] [--out FILE]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

HBM_BYTES_PER_S = 6.29e12


def write_rows(root, n, num_img, w2, h):
    import numpy as np
    from PIL import Image
    d = os.path.join(root, 'train')
    os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(0)
    for i in range(n):
        Image.fromarray(rng.randint(0, 256, (h, num_img * w2, 3)).astype(np.uint8)).save(os.path.join(d, f'row_{i:02d}.png'), compress_level=1)


def window(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters          # ms per batch


def kernel_us(loader, slot, rounds, iters):
    """device time of the six launches of one batch: issued from Python they are host-bound (about 28 us per call), so they are captured once into a
    graph (one stream, no branches) and the replays are timed with device events; returns (us per batch per round, us per batch as issued eagerly)"""
    import torch
    from deepliif_amd import engine as E
    from deepliif_amd import ops
    ds, n = loader.dataset, len(slot.indices)
    cw, ch = slot.geo[0]['crop'][2], slot.geo[0]['crop'][3]
    acts = [E.new_act(n, ch, cw, 3, loader.precision, loader.device) for _ in range(6)]
    be = ops.impl()

    def gathers():
        for a, panel in zip(acts, ds.panels['A'] + ds.panels['B']):
            loader._gather(be, slot, list(range(n)), panel, False, a.t, 0, a.t.shape[3])

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k

    gathers()
    torch.cuda.synchronize()
    eager = timed(gathers, iters)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gathers()
    g.replay()
    torch.cuda.synchronize()
    return [timed(g.replay, iters) for _ in range(rounds)], eager


def child(args):
    import torch
    import bench
    import data_ref
    from PIL import Image
    from deepliif_amd import data as D
    from deepliif_amd import models as M
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    n, size, panels = args.batch, args.size, 6
    a = argparse.Namespace(batch=n, size=size, ngf=8, norm='instance', precision='bf16')
    torch.manual_seed(0)
    opt = bench.make_opt(a, 0)
    so, sys.stdout = sys.stdout, open(os.devnull, 'w')
    try:
        model = M.create_model(opt)
        model.setup(opt)
    finally:
        sys.stdout = so
    res = {'timing': f'wall clock per batch, device synchronise around each window of {args.iters} batches, after warm-up; {args.rounds} alternations',
           'device': torch.cuda.get_device_name(0), 'workload': f'batch {n}, 1 + 5 panels, {size} x {size}, bf16 activations'}
    with tempfile.TemporaryDirectory() as root:
        for k, v in dict(dataroot=root, dataset_mode='aligned', preprocess='resize_and_crop', load_size=size, crop_size=size, direction='AtoB', no_flip=False,
                         seg_no=0, max_dataset_size=None, serial_batches=True, num_threads=0, batch_size=n, phase='train').items():
            setattr(opt, k, v)
        write_rows(root, n, panels, size, size)
        random.seed(0)
        loader = D.create_dataset(opt)
        slot = loader._slots[0]
        loader._prepare(slot, list(range(n)))                 # decode once: pinned uint8 rows
        # (A)'s input: what the reference's loader would hand over for the same rows
        random.seed(0)
        paths = loader.dataset.AB_paths
        t0 = time.perf_counter()
        samples = [data_ref.getitem(Image.open(p), opt, p) for p in paths]
        res['cpu_reference_chain_ms_per_sample'] = round((time.perf_counter() - t0) * 1e3 / n, 2)
        batch_a = data_ref.collate(samples)
        assert not batch_a['A'].is_pinned() and batch_a['A'].dtype == torch.float32

        def path_a():
            model.set_input(batch_a)

        def path_b():
            loader._upload(slot)
            model.set_input(loader._launch(slot))

        random.seed(0)
        path_b()
        got = [model._A.t.clone()] + [b.t.clone() for b in model._B]
        path_a()
        torch.cuda.synchronize()
        want = [model._A.t] + [b.t for b in model._B]
        assert all(torch.equal(x, y) for x, y in zip(got, want)), '(B) does not produce the activations of (A)'
        for _ in range(10):
            path_a()
            path_b()
        times = {'A': [], 'B': []}
        for _ in range(args.rounds):
            times['A'].append(window(path_a, args.iters))
            times['B'].append(window(path_b, args.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        res['ms_per_batch'] = {k: round(v, 3) for k, v in med.items()}
        res['alternations_ms'] = {k: [round(x, 3) for x in v] for k, v in times.items()}
        res['spread_ms'] = round(max(max(v) - min(v) for v in times.values()), 3)
        res['B_not_above_A'] = bool(med['B'] <= med['A'])
        res['host_link_bytes_per_batch'] = {'A': panels * n * 3 * size * size * 4, 'B': panels * n * 3 * size * size}
        # the kernels against their byte bound: per launch 3 bytes read and Cp * 2 bytes written per pixel
        bound_us = panels * n * size * size * (3 + 8 * 2) / HBM_BYTES_PER_S * 1e6
        loader._upload(slot)
        torch.cuda.current_stream().wait_event(slot.copied)
        ks, eager = kernel_us(loader, slot, args.rounds, args.iters)
        res['kernels_plain'] = {'us_per_batch': round(statistics.median(ks), 1), 'alternations_us': [round(x, 1) for x in ks], 'byte_bound_us': round(bound_us, 1),
                                'over_bound': round(statistics.median(ks) / bound_us, 2), 'us_per_batch_issued_from_python': round(eager, 1)}
    with tempfile.TemporaryDirectory() as root:
        src = size + 60
        opt.dataroot, opt.load_size, opt.crop_size = root, size + 30, size
        write_rows(root, n, panels, src, src)
        random.seed(0)
        loader = D.create_dataset(opt)
        slot = loader._slots[0]
        loader._prepare(slot, list(range(n)))
        loader._upload(slot)
        bound_us = panels * n * (src * src * 3 + size * size * 8 * 2) / HBM_BYTES_PER_S * 1e6
        torch.cuda.current_stream().wait_event(slot.copied)
        ks, eager = kernel_us(loader, slot, args.rounds, args.iters)
        res['kernels_resize'] = {'geometry': f'{src} x {src} -> {size + 30} x {size + 30}, crop {size}', 'us_per_batch': round(statistics.median(ks), 1),
                                 'alternations_us': [round(x, 1) for x in ks], 'byte_bound_us': round(bound_us, 1),
                                 'over_bound': round(statistics.median(ks) / bound_us, 2), 'us_per_batch_issued_from_python': round(eager, 1)}
    print('RESULT ' + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--timeout', type=int, default=600)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'data_pipeline.json'))
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--rounds', str(args.rounds), '--iters', str(args.iters), '--batch', str(args.batch),
           '--size', str(args.size)]
    p = subprocess.run(cmd, timeout=args.timeout, stdout=subprocess.PIPE, text=True)          # the GPU step, under its own time limit
    if p.returncode != 0:
        sys.exit(f'the measurement ended with status {p.returncode}')
    line = [x for x in p.stdout.splitlines() if x.startswith('RESULT ')][-1]
    res = json.loads(line[len('RESULT '):])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
