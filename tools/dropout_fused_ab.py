"""What does applying Dropout(0.5) inside the norm kernels buy?  Event timings after warm-up, three ways, alternated `--rounds` times in ONE process:
    (a) norm_forward alone                                            (the bytes the fused pass moves)
    (b) the unfused pair: norm_forward + dropout (+ axpby into the concat slice for the UNet shapes)
    (c) the fused call: norm_forward(dropout=...)
and the same three for the backward (dropout on the gradient, then norm_backward | norm_backward(dropout=...)), at the ResnetBlock tensor
[8,128,128,256] bf16 and at the UNet ngf*8 shapes of unet_512 at batch 8 ([8,s,s,512], s = 32, 16, 8, 4, written into the second half of a 1024-wide
concat buffer).  The large tensors are cycled over a pool so that nothing is served from the Infinity Cache, as in the training step.
Then the one-stream 5 G + 5 D training step (ngf 64, 512 x 512, batch 8, no_dropout=False): unfused eager, fused eager, fused captured
(models.StepGraph(capture_dropout=True)), in alternating blocks.  Writes <out> (default profiles/dropout_fused.json) and prints it.

    python tools/dropout_fused_ab.py [--rounds 3] [--steps 8] [--no-step] [--out FILE] [--ngf 64 --size 512 --batch 8]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from deepliif_amd import _lib as L  # noqa: E402
from deepliif_amd import models as M  # noqa: E402
from deepliif_amd import ops  # noqa: E402

DEV = 'cuda'
SEED = 123456789


def timeit(fn, n, pool):
    for i in range(min(5, n)):
        fn(i % pool)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i % pool)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n           # us per call


def summarize(times):
    """median per label, the spread between the alternations, and whether (c) < (b) by more than that spread"""
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(max(v) - min(v) for v in times.values())
    return {'us': {k: round(v, 2) for k, v in med.items()}, 'alternations_us': {k: [round(x, 2) for x in v] for k, v in times.items()},
            'spread_us': round(spread, 2), 'saved_us': round(med['b'] - med['c'], 2), 'fused_over_norm_alone': round(med['c'] / med['a'], 3),
            'fused_wins': bool(med['b'] - med['c'] > spread)}


def kernel_ab(be, shape, act, scope, slice_out, rounds, calls):
    n, h, w, c = shape
    dt = torch.bfloat16
    pool = max(1, min(10, (1 << 30) // (n * h * w * c * 2)))            # ~1 GB per operand: no tensor comes back out of the Infinity Cache
    ys = [torch.randn(shape, device=DEV).to(dt) for _ in range(pool)]
    dzbuf = [torch.randn((n, h, w, 2 * c) if slice_out else shape, device=DEV).to(dt) for _ in range(pool)]
    dzs = [b[..., c:] for b in dzbuf] if slice_out else dzbuf           # the UNet's gradient arrives as a slice of the concat gradient
    tmp = [torch.empty(shape, dtype=dt, device=DEV) for _ in range(pool)]
    tmp2 = [torch.empty(shape, dtype=dt, device=DEV) for _ in range(pool)]
    cat = [torch.empty((n, h, w, 2 * c), dtype=dt, device=DEV) for _ in range(pool)] if slice_out else None
    outs = [b[..., c:] for b in cat] if slice_out else [torch.empty(shape, dtype=dt, device=DEV) for _ in range(pool)]
    g, b_ = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    dg, db = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    affine = scope == L.NORM_BATCH
    ga, be_ = (g, b_) if affine else (None, None)
    drop = (0.5, SEED, None, 0)
    st = be.norm_forward(ys[0], tmp[0], c, scope, act, ga, be_, None, None, -1.0, None)

    def fwd_a(i):
        be.norm_forward(ys[i], outs[i], c, scope, act, ga, be_, None, None, -1.0, None)

    def fwd_b(i):
        if slice_out:                               # networks.UnetGenerator._run's three passes
            be.norm_forward(ys[i], tmp[i], c, scope, act, ga, be_, None, None, -1.0, None)
            be.dropout(tmp[i], tmp2[i], 0.5, SEED)
            be.axpby(1.0, tmp2[i], 0.0, None, outs[i])
        else:
            be.norm_forward(ys[i], tmp[i], c, scope, act, ga, be_, None, None, -1.0, None)
            be.dropout(tmp[i], outs[i], 0.5, SEED)

    def fwd_c(i):
        be.norm_forward(ys[i], outs[i], c, scope, act, ga, be_, None, None, -1.0, None, dropout=drop)

    def bwd_a(i):
        be.norm_backward(dzs[i], ys[i], tmp[i], st, c, scope, act, ga, dg if affine else None, db if affine else None)

    def bwd_b(i):
        be.dropout(dzs[i], tmp2[i], 0.5, SEED)
        be.norm_backward(tmp2[i], ys[i], tmp[i], st, c, scope, act, ga, dg if affine else None, db if affine else None)

    def bwd_c(i):
        be.norm_backward(dzs[i], ys[i], tmp[i], st, c, scope, act, ga, dg if affine else None, db if affine else None, dropout=drop)

    # the fused call must give what the pair gives before its time means anything
    fwd_b(0)
    want = outs[0].clone()
    fwd_c(0)
    bwd_b(0)
    want_dy = tmp[0].clone()
    bwd_c(0)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], want) and torch.equal(tmp[0], want_dy), 'the fused call differs from the unfused pair'
    res = {}
    for name, fns in (('forward', (fwd_a, fwd_b, fwd_c)), ('backward', (bwd_a, bwd_b, bwd_c))):
        times = {'a': [], 'b': [], 'c': []}
        for _ in range(rounds):
            for k, fn in zip('abc', fns):
                times[k].append(timeit(fn, calls, pool))
        res[name] = summarize(times)
    res['bytes_of_one_tensor'] = n * h * w * c * 2
    return res


def build(args):
    a = argparse.Namespace(batch=args.batch, size=args.size, ngf=args.ngf, norm='instance', precision='bf16')
    torch.manual_seed(0)
    opt = bench.make_opt(a, 0)
    opt.no_dropout = False
    so, sys.stdout = sys.stdout, open(os.devnull, 'w')
    try:
        model = M.create_model(opt)
        model.setup(opt)
    finally:
        sys.stdout = so
    return model


def step_ab(args):
    M._N_STREAMS = 1
    g = torch.Generator().manual_seed(1)
    synth = lambda: (torch.rand(args.batch, 3, args.size, args.size, generator=g) * 2 - 1).to(DEV)
    batch = {'A': synth(), 'B': [synth() for _ in range(5)], 'A_paths': ['synthetic']}
    eager, graphed = build(args), build(args)
    sg = M.StepGraph(graphed, warmup=2, capture_dropout=True)

    def run(kind, n):
        ops.HipBackend.supports_fused_dropout = kind != 'unfused_eager'
        try:
            for _ in range(n):
                if kind == 'fused_captured':
                    sg.step(batch)
                else:
                    eager.set_input(batch)
                    eager.optimize_parameters()
        finally:
            ops.HipBackend.supports_fused_dropout = True

    kinds = ('unfused_eager', 'fused_eager', 'fused_captured')
    for k in kinds:
        run(k, 4)                                    # warm-up: code objects, pack tables, workspaces; the capture
    torch.cuda.synchronize()
    assert sg.graph is not None and sg.why_eager is None, sg.why_eager
    times = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k in kinds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(k, args.steps)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.steps)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {'workload': f'DeepLIIF 5 G + 5 D training step, one stream, ngf {args.ngf}, {args.size} x {args.size}, batch {args.batch}, bf16, norm instance, no_dropout=False',
            'dropout_sites_per_step': sg.sites, 'ms_per_step': {k: round(v, 3) for k, v in med.items()},
            'alternations_ms': {k: [round(x, 3) for x in v] for k, v in times.items()},
            'spread_ms': round(max(max(v) - min(v) for v in times.values()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--ngf', type=int, default=64)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dropout_fused.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    be = ops.impl()
    res = {'timing': f'device events around blocks of calls after warm-up; (a) norm alone, (b) unfused pair, (c) fused; {args.rounds} alternations, medians',
           'device': torch.cuda.get_device_name(0), 'kernels': {}}
    res['kernels']['resnet_block [8,128,128,256] instance relu'] = kernel_ab(be, (args.batch, 128, 128, 256), L.ACT_RELU, L.NORM_INSTANCE, False, args.rounds, 40)
    for s in (32, 16, 8, 4):
        res['kernels'][f'unet ngf*8 [8,{s},{s},512] batch norm -> concat slice'] = kernel_ab(be, (args.batch, s, s, 512), L.ACT_NONE, L.NORM_BATCH, True, args.rounds, 200)
    if not args.no_step:
        res['step'] = step_ab(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
