"""What does `--norm spectral` cost?  The 5 G + 5 D training step (ngf 64, 512 x 512, batch 8) with norm='spectral' and with norm='none' -- the same
convolutions, the same launches apart from the spectral ones -- built in ONE process and timed in alternating blocks with device events after warm-up;
then one `rocprofv3 --kernel-trace --stats` run of the spectral step in a fresh child process for the count and summed time of the spectral kernels
(csrc/spectral.hip: sp_*).  Writes <out>/step_ab.json (default out: profiles/spectral) and the child's trace under <out>/trace.

    python tools/spectral_step.py [--precision bf16] [--steps 10] [--rounds 3] [--no-trace] [--out DIR] [--ngf 64 --size 512 --batch 8]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args, norm):
    import torch
    import bench
    from deepliif_amd import models as M
    a = argparse.Namespace(batch=args.batch, size=args.size, ngf=args.ngf, norm=norm, precision=args.precision)
    torch.manual_seed(0)
    opt = bench.make_opt(a, 0)
    so, sys.stdout = sys.stdout, open(os.devnull, 'w')
    try:
        model = M.create_model(opt)
        model.setup(opt)
    finally:
        sys.stdout = so
    return model


def batch_of(args):
    import torch
    dev = torch.device('cuda', 0)

    def synth(seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.rand(args.batch, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
    return {'A': synth(1234), 'B': [synth(1235 + i) for i in range(5)], 'A_paths': ['synthetic']}


def run_steps(model, batch, n):
    for _ in range(n):
        model.set_input(batch)
        model.optimize_parameters()


def timed_block(model, batch, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run_steps(model, batch, n)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def trace_child(args):
    """the program rocprofv3 traces: warm-up + `steps` spectral steps"""
    import torch
    model = build(args, 'spectral')
    batch = batch_of(args)
    run_steps(model, batch, 1 + args.steps)
    torch.cuda.synchronize()


def trace(args, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'spectral', '--', sys.executable, os.path.abspath(__file__),
           '--trace-child', '--precision', args.precision, '--steps', str(args.trace_steps), '--ngf', str(args.ngf), '--size', str(args.size), '--batch', str(args.batch)]
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
    if r.returncode != 0:
        return {'error': f'rocprofv3 exited with {r.returncode}: {r.stderr[-400:]}'}
    files = glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        return {'error': 'rocprofv3 wrote no kernel_stats.csv'}
    rows = list(csv.DictReader(open(files[0])))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    sp = [r for r in rows if r['Name'].startswith('sp_') or ' sp_' in r['Name']]
    nsteps = 1 + args.trace_steps
    return {'traced_steps': nsteps, 'kernels': {r['Name'].split('(')[0]: {'calls': int(r['Calls']), 'total_us': float(r['TotalDurationNs']) / 1e3} for r in sp},
            'spectral_launches_per_step': sum(int(r['Calls']) for r in sp) / nsteps,
            'spectral_kernel_ms_per_step': sum(float(r['TotalDurationNs']) for r in sp) / 1e6 / nsteps,
            'all_kernel_ms_per_step': total / 1e6 / nsteps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precision', default='bf16')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--trace-steps', type=int, default=3)
    ap.add_argument('--ngf', type=int, default=64)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spectral'))
    ap.add_argument('--trace-child', action='store_true')
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args)
        return
    import torch
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    batch = batch_of(args)
    models = {norm: build(args, norm) for norm in ('spectral', 'none')}
    for m in models.values():
        run_steps(m, batch, 3)                      # warm-up: code objects, pack tables, generations, workspaces
    torch.cuda.synchronize()
    times = {norm: [] for norm in models}
    for _ in range(args.rounds):                    # alternating blocks: drift of the box hits both alike
        for norm, m in models.items():
            times[norm].append(timed_block(m, batch, args.steps))
    med = {norm: statistics.median(t) for norm, t in times.items()}
    nparams = sum(l.weight.numel() for _, net in models['spectral']._nets() if net._spectral is not None for l in net._spectral.layers)
    res = {'workload': f'DeepLIIF 5 G + 5 D training step, ngf {args.ngf}, {args.size} x {args.size}, batch {args.batch}, {args.precision}',
           'timing': f'device events around blocks of {args.steps} steps, {args.rounds} alternating blocks per norm after 3 warm-up steps, median',
           'ms_per_step': med, 'blocks_ms_per_step': times, 'difference_ms': med['spectral'] - med['none'],
           'difference_frac_of_none': (med['spectral'] - med['none']) / med['none'],
           'spectral_weights': nparams}
    del models
    torch.cuda.empty_cache()
    out = os.path.abspath(args.out)
    if not args.no_trace:
        res['rocprofv3'] = trace(args, os.path.join(out, 'trace'))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'step_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
