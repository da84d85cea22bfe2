#!/usr/bin/env python
"""bench.py -- DeepLIIF training-step throughput on MI355X (BASELINE.json metric: 512x512 tiles/s, train step 5G+5D).

  python bench.py --gpus N --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = model.set_input(batch) + model.optimize_parameters() of the DeepLIIF model
(modalities_no=5, seg_gen=False -> 5 x ResnetGenerator-9block + 5 x NLayerDiscriminator(n=4), GAN + SmoothL1, Adam) on a
batch of 8 synthetic 512x512x3 tiles per GPU that is already resident in HBM (BASELINE.json configs[2] per GPU; weak
scaling).  `--workload infer` times the 9-generator inference DAG of configs[1] instead (4 Resnet-9 + 5 UNet-512, batch 8);
`--workload wsi` the tile-parallel whole-slide loop of configs[4] (synthetic uint8 region in HBM -> crop / is_empty / 9 generators
on batches of 8 tiles / uint8 stitch; one "step" = one batch of 8 tiles per GPU, every rank owns a band of tile rows).
Without torchrun, `--gpus N` (N > 1) re-executes itself under `python -m torch.distributed.run --nproc-per-node N`.
Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times --steps steps, writes the
outputs of the last timed step if --dump-outputs DIR is given, and prints the line: `value`, `ms_per_step` and the other headline keys.
`--dump-outputs DIR` writes what the timed path computed in its last step as DIR/<name>.npy (float32, float64 for scalars): the losses,
the generated images and a sample of every network's parameters after the update (train workloads), the result images (infer / wsi);
an output larger than DUMP_SAMPLE elements is kept as a fixed, seeded sample of its elements (the same positions in every run).
`--full` adds everything else the benchmark measures:
  strict_parity: the SAME workload timed on the strict policy (fp32 storage, split-bf16 x3 MFMA: the one the GPU tests assert at 1e-3
                 against the oracle) plus the measured distance of the headline (bf16) policy from it on this very batch
  roofline     : dominant layer shape = the 3x3, 256->256 ch conv at 8x128x128 pixels (the 18 ResnetBlock convs of every Resnet-9
                 and, when training, their data-gradients); the kernel NAME is whatever the library dispatches for that
                 descriptor (dl_conv_kernel_name), per-launch time from events recorded on the launch stream around the host call
                 inside the timed region (every 8th launch of that shape: event pairs around all 180 per step cost 6 % of the step;
                 `timer_overhead` = the same steps timed once more without any events, same process); `traffic` only when the committed
                 PMC summary was collected on that same kernel
  cpu_baseline : the CPU oracle (oracle/deepliif_oracle.py, a port of the reference's PyTorch step) timed on this box's host
                 cores for a bounded sample of whole steps at batch 1 (10-30 s of CPU work; rank 0, N=1 only).
  and graph_replay, exchange, policy_vs_strict, whole_slide, other_workloads (below).  With --full the timed steps carry the roofline's
  per-launch events, as `value` / `ms_per_step` of the --full line say.
"""
import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GF_PER_TILE_TRAIN_5R5D = 6817.0      # BASELINE.md / SURVEY 8(d): conv MACs only, FLOP = 2*MAC
GF_PER_TILE_INFER = 1828.0
GF_PER_TILE_TRAIN_18NETS = 7051.0     # real DeepLIIF (4 Resnet-9 + 5 UNet-512 generators, 9 NLayerD) step
PEAK_BF16_TFLOPS = 2500.0            # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0
STRICT_PMC_FILE = os.path.join('r03', 'pmc_strict_conv256.json')     # the same passes over the strict ResnetBlock kernel (tools/gpu_r03_pmc_strict.sh)
N8_FULL_FILE = os.path.join('r06', 'cpu_baseline_n8_full.json')     # bench.py --cpu-baseline-n8-full: the oracle at batch 8, 512 x 512 (SURVEY 8d on-spec)
TRAJECTORY_FILE = os.path.join('r06', 'trajectory_r06.json')  # tests/test_gpu_trajectory.py: 100-step loss curves of both policies vs the oracle
PMC_FILE = os.path.join('r06', 'pmc_dominant_conv256.json')     # dominant-kernel HBM traffic from separate --pmc passes (re-collected when the kernel changes)
DUMP_SAMPLE = 1 << 19           # --dump-outputs: elements kept of a larger output (2 MB in float32), at fixed seeded positions
DUMP_PARAM_SAMPLE = 1 << 16     # --dump-outputs: elements kept of each network's flattened parameters after the step
DUMP_LIMIT_BYTES = 64 << 20


def _dump_sample(t, k):
    """t flattened to float32: all of it up to k elements, else k elements at positions drawn from a fixed seed (same shape -> same positions)"""
    flat = t.detach().reshape(-1).float()
    if flat.numel() > k:
        idx = torch.randint(flat.numel(), (k,), generator=torch.Generator().manual_seed(20240611)).sort().values
        flat = flat[idx.to(flat.device)]
    return flat.cpu().numpy()


def step_outputs(model, result):
    """what a caller of the timed path holds after its last step -> {name: ndarray}: the losses (float64), the generated images and a sample of every
    network's parameters (train workloads, `model`), or the result images (infer: {key: tensor}, wsi: (band images {key: uint8 tensor}, rows))"""
    import numpy as np
    out = {}
    if model is not None:
        for k, v in model.get_current_losses().items():
            out[f'loss_{k}'] = np.array(v, dtype=np.float64)
        for k, v in model.get_current_visuals().items():
            if k.startswith('fake'):
                out[k] = _dump_sample(v, DUMP_SAMPLE)
        for name in model.model_names:
            params = [p.detach().reshape(-1).float() for p in getattr(model, 'net' + name).parameters()]
            out[f'param_{name}'] = _dump_sample(torch.cat(params), DUMP_PARAM_SAMPLE)
    elif isinstance(result, tuple):
        out.update({k: _dump_sample(v, DUMP_SAMPLE) for k, v in (result[0] or {}).items()})
    elif result is not None:
        out.update({k: _dump_sample(v, DUMP_SAMPLE) for k, v in result.items()})
    return out


def dump_outputs(path, arrays):
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f'--dump-outputs: {total} bytes of outputs, more than {DUMP_LIMIT_BYTES}'
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, f'{k}.npy'), a)


def make_opt(args, device_index, M=5, seg_gen=False):
    w = [1.0 / (M + 1)] * (M + 1)      # cli.py:349-371 defaults for modalities_no != 4
    lw = w
    if M == 4:                         # the real DeepLIIF defaults (cli.py:349-371)
        w, lw = [0.25, 0.15, 0.25, 0.1, 0.25], [0.2] * 5
    return types.SimpleNamespace(
        model='DeepLIIF', name='bench', checkpoints_dir='/tmp/dl_amd_bench', gpu_ids=[device_index], is_train=True, phase='train',
        continue_train=False, modalities_no=M, seg_gen=seg_gen, modalities_names=[], input_nc=3, input_no=1, output_nc=3, ngf=args.ngf, ndf=args.ngf,
        net_g='resnet_9blocks', net_gs='unet_512', net_d='n_layers', n_layers_D=4, norm=args.norm, no_dropout=True, init_type='normal',
        init_gain=0.02, padding='zero', upsample='convtranspose', gan_mode='vanilla', gan_mode_s='lsgan', optimizer='adam', lr_g=2e-4,
        lr_d=2e-4, beta1=0.5, lr_policy='linear', n_epochs=100, n_epochs_decay=100, epoch_count=0, seg_weights=w, loss_G_weights=lw,
        loss_D_weights=lw, lambda_L1=100.0, verbose=False, epoch='latest', load_iter=0, precision=args.precision)


class KernelTimer:
    """Records HIP events around every launch of the dominant conv kernel (on the stream the kernel is launched on)."""

    EVERY = 8          # event pairs around every 8th matching launch: 3600 pairs in a 20-step run cost 6 % of the step (measured r03: 111.8 vs 105.4 ms),
                       # the subsample < 1 % (roofline.timer_overhead reports the same-process A/B of every run)

    def __init__(self, backend, shape):
        self.backend, self.shape, self.pairs, self.enabled = backend, tuple(shape), [], False
        self.pairs_add = []           # launches that also add the skip-connection gradient in their store pass (dl_conv_forward_add): +67 MB of algorithmic reads
        self.kernel = '?'
        self.seen = 0
        self._orig = backend.conv_forward
        backend.conv_forward = self._wrapped
        # the block's first conv's data gradient goes through conv_forward_add since r06 (the skip gradient is added in its store pass): the same kernel,
        # the same shape, 45 of the 180 launches per step -- they belong in the average (they are the slower ones)
        self._orig_add = getattr(backend, 'conv_forward_add', None)
        if self._orig_add is not None:
            backend.conv_forward_add = self._wrapped_add

    def _wrapped(self, packed, x, out, *args, **kwargs):
        hit = self.enabled and tuple(x.shape) == self.shape and tuple(out.shape) == self.shape and packed.plan.n_phase == 1
        if hit:
            self.seen += 1
            hit = self.seen % self.EVERY == 0
        if hit:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
        ret = self._orig(packed, x, out, *args, **kwargs)
        if hit:
            e.record()
            self.pairs.append((s, e))
            self.kernel = getattr(self.backend, 'last_conv_kernel', '') or self.kernel      # what the library dispatched
        return ret

    def _wrapped_add(self, packed, x, addend, out, *args, **kwargs):
        hit = self.enabled and tuple(x.shape) == self.shape and tuple(out.shape) == self.shape and packed.plan.n_phase == 1
        if hit:
            self.seen += 1
            hit = self.seen % self.EVERY == 0
        if hit:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
        ret = self._orig_add(packed, x, addend, out, *args, **kwargs)
        if hit and ret:
            e.record()
            self.pairs_add.append((s, e))
            self.kernel = getattr(self.backend, 'last_conv_kernel', '') or self.kernel
        return ret

    def mean_seconds(self):
        if not self.pairs:
            return None
        return sum(s.elapsed_time(e) for s, e in self.pairs) / len(self.pairs) * 1e-3

    def mean_seconds_add(self):
        if not self.pairs_add:
            return None
        return sum(s.elapsed_time(e) for s, e in self.pairs_add) / len(self.pairs_add) * 1e-3

    def median_seconds(self):
        if not self.pairs:
            return None
        v = sorted(s.elapsed_time(e) for s, e in self.pairs)
        return v[len(v) // 2] * 1e-3


def mfma_sustained(dev, launches=12, iters=240):
    """What the matrix cores of THIS box sustain on v_mfma_f32_32x32x16_bf16 with nothing else in the way (dl_probe_mfma_sustained: 256 workgroups x 4
    waves, 16 accumulators + 16 operand fragments per wave, register-resident), on random N(0,1) operand bits and on zeros: the chip clocks to
    its power budget, so the denominator of `frac` is data-dependent.  -> {'random_tflops', 'zero_tflops'} (event-timed)."""
    import ctypes as C
    from deepliif_amd import _lib as L
    lib = L.load()
    blocks = 256
    n = int(lib.dl_probe_mfma_sustained_elems(blocks))
    sink = torch.zeros(4, device=dev)
    out = {}
    for tag in ('random', 'zero'):
        data = (torch.randn(n, device=dev) if tag == 'random' else torch.zeros(n, device=dev)).to(torch.bfloat16)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(3):
            L.check(lib.dl_probe_mfma_sustained(C.c_void_p(data.data_ptr()), blocks, iters, C.c_void_p(sink.data_ptr()), st), 'dl_probe_mfma_sustained')
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            L.check(lib.dl_probe_mfma_sustained(C.c_void_p(data.data_ptr()), blocks, iters, C.c_void_p(sink.data_ptr()), st), 'dl_probe_mfma_sustained')
        e1.record()
        torch.cuda.synchronize()
        out[f'{tag}_tflops'] = round(blocks * 4 * iters * 64 * 32768.0 * launches / (e0.elapsed_time(e1) * 1e-3) / 1e12, 1)
    return out


def usable_cores():
    """Cores this process may really use: scheduler affinity capped by the cgroup CPU quota (containers)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        q, p = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if q != 'max':
            n = min(n, max(1, int(float(q) / float(p))))
    except Exception:
        pass
    return max(1, n)


def cpu_baseline_child(norm, size, batch=1, budget=45.0):
    """(child process) optimize_parameters() steps of the CPU oracle at batch `batch` (default 1), same model family, random init."""
    from oracle import deepliif_oracle as O
    cores = min(usable_cores(), 64)
    torch.set_num_threads(cores)
    cfg = O.OracleConfig(modalities_no=5, seg_gen=False, norm=norm, padding='zero', ngf=64, ndf=64)
    g = torch.Generator().manual_seed(0)
    nets = {}
    for i in range(1, 6):
        nets[f'G{i}'] = O.random_state_dict('resnet_9blocks', 3, 3, 64, norm, 'zero', generator=g)
        nets[f'D{i}'] = O.random_state_dict('n_layers', 6, 3, 64, norm, 'zero', 4, generator=g)
    om = O.OracleDeepLIIF(cfg, nets)
    A = torch.rand(batch, 3, size, size, generator=g) * 2 - 1
    B = [torch.rand(batch, 3, size, size, generator=g) * 2 - 1 for _ in range(5)]
    om.set_input({'A': A, 'B': B})
    # bounded sample of ~10-30 s of CPU work (1 warm-up + >= 3 timed steps): whole steps at batch 1, the warm-up step is
    # not counted; stops early only if the host is so slow that 3 steps would exceed ~45 s
    om.optimize_parameters()
    times = []
    while len(times) < 3 and (sum(times) < budget or not times):
        t0 = time.time()
        om.optimize_parameters()
        times.append(time.time() - t0)
    print(json.dumps({'seconds': sum(times) / len(times), 'steps': len(times), 'total_seconds': sum(times), 'cores': cores, 'size': size, 'batch': batch}), flush=True)


def cpu_infer_child(size, budget=30.0):
    """(child process) the inference DAG of BASELINE configs[1] on the CPU oracle, one tile per forward like the reference (deepliif/models/__init__.py:293-361):
    4 x resnet_9blocks on the tile, 5 x unet_512 on the tile / the four translated images, weighted seg sum; BatchNorm on the tile's own statistics"""
    from oracle import deepliif_oracle as O
    cores = min(usable_cores(), 64)
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(0)
    G = [O.random_state_dict('resnet_9blocks', 3, 3, 64, 'batch', 'zero', generator=g) for _ in range(4)]
    S = [O.random_state_dict('unet_512', 3, 3, 64, 'batch', 'zero', generator=g) for _ in range(5)]
    x = torch.rand(1, 3, size, size, generator=g) * 2 - 1
    w = [0.25, 0.15, 0.25, 0.1, 0.25]

    def tile():
        with torch.no_grad():
            mods = [O.run_generator('resnet_9blocks', sd, x, 'batch', 'zero') for sd in G]
            segs = [O.run_generator('unet_512', sd, src, 'batch', 'zero') for sd, src in zip(S, [x] + mods)]
            return sum(wi * si for wi, si in zip(w, segs))
    tile()
    times = []
    while len(times) < 3 and (sum(times) < budget or not times):
        t0 = time.time()
        tile()
        times.append(time.time() - t0)
    print(json.dumps({'seconds': sum(times) / len(times), 'steps': len(times), 'total_seconds': sum(times), 'cores': cores, 'size': size, 'batch': 1}), flush=True)


def cpu_baseline_infer(args):
    """cpu_baseline of the inference workload: the oracle's 9-generator DAG on one 512 x 512 tile at a time (the reference infers one tile per forward), a bounded
    sample in a child process"""
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--cpu-infer-child', '--size', str(args.size)], capture_output=True, text=True, timeout=240,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES=''))
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    except Exception as e:
        return {'value': None, 'unit': 'tiles/s', 'cores': usable_cores(), 'kind': 'port', 'sample': f'CPU oracle inference did not finish ({type(e).__name__})'}
    return {'value': round(1.0 / d['seconds'], 5), 'unit': 'tiles/s', 'cores': d['cores'], 'kind': 'port',
            'sample': f"1 warm-up + {d['steps']} timed tiles through the fp32 CPU oracle's inference DAG (4 Resnet-9 + 5 UNet-512 + weighted seg sum, one {args.size}x{args.size} tile per "
                      f"forward as the reference does), {d['total_seconds']:.1f} s of CPU work, {d['seconds']:.1f} s per tile"}


def other_workloads(args):
    """The driver only ever runs `bench.py --gpus 1`: so that BASELINE configs[1] / [3] / [4] and the real 18-network step get driver-timed numbers too, the
    default run appends a SHORT measurement of each (5 steps, 2 warm-up; a child process per workload, so nothing of it touches the contract line's model or
    clock).  Each entry is that child's own JSON line reduced to the figures that matter."""
    import subprocess
    out = {}
    for wl in ('infer', 'infer_fp16', 'train18', 'ext', 'wsi', 'wsi_fp16'):
        cmd = [sys.executable, os.path.abspath(__file__), '--workload', wl.split('_')[0], '--precision', 'fp16' if wl.endswith('_fp16') else args.precision, '--steps', '5', '--warmup', '2', '--full', '--no-strict', '--no-graph', '--no-timer-check', '--no-other-workloads',
               '--batch', str(args.batch), '--size', str(args.size), '--ngf', str(args.ngf)]
        if wl != 'infer':
            cmd.append('--no-cpu-baseline')
        t0 = time.time()
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
        except Exception as e:
            out[wl] = {'error': f'{type(e).__name__}: {str(e)[:160]}'}
            continue
        rf = d.get('roofline') or {}
        out[wl] = {'metric': d['metric'], 'value': d['value'], 'unit': d['unit'], 'ms_per_step': d['ms_per_step'], 'steps': d['steps'], 'warmup': d['warmup'], 'dtype': d['dtype'],
                   'model_tflops': d.get('model_tflops'), 'model_frac_of_bf16_peak': d.get('model_frac_of_bf16_peak'), 'streams': d['config'].get('streams'),
                   'workload': d['config']['workload'],
                   'roofline': ({k: rf.get(k) for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'kernel', 'launches_timed', 'avg_launch_us', 'launch_times_from')} if rf else None),
                   'wall_s': round(time.time() - t0, 1)}
        for k in ('whole_slide', 'cpu_baseline', 'policy_vs_strict'):
            if d.get(k):
                out[wl][k] = d[k]
    return out


def cpu_baseline(args, batch=None, budget=45.0, half_tile=False):
    """The CPU oracle (a port of the reference's PyTorch training step) timed on this box's host cores: a bounded sample of whole steps at batch
    `batch` (default args.cpu_batch = 1, the reference's default batch size, cli.py:110; SURVEY 8d also asks for the GPU line's per-GPU batch 8 ->
    cpu_baseline_n8).  Runs in a child process with a time limit so that a slow / oversubscribed host cannot stall the benchmark; falls back
    to a 256x256 tile (reported in 512x512-tile equivalents) if 512x512 does not finish in time."""
    import subprocess
    batch = args.cpu_batch if batch is None else batch
    last = 'not run'
    for size, limit in (((args.size, 240 * batch),) if not half_tile else ()) + ((args.size // 2, 180 if half_tile else 180 * batch),):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--cpu-baseline-child', '--norm', args.norm, '--size', str(size), '--cpu-batch', str(batch),
                                '--cpu-budget', str(budget)], capture_output=True, text=True, timeout=limit, env=dict(os.environ, HIP_VISIBLE_DEVICES=''))
            line = [l for l in r.stdout.splitlines() if l.startswith('{')][-1]
            d = json.loads(line)
        except Exception as e:            # timeout / crash: try the smaller sample, else report nothing
            last = f'{type(e).__name__}'
            continue
        scale = (size * size) / float(args.size * args.size)
        return {'value': round(scale * batch / d['seconds'], 5), 'unit': 'tiles/s', 'cores': d['cores'], 'kind': 'port',
                'sample': f"1 warm-up + {d.get('steps', 1)} timed optimize_parameters() step(s) of the fp32 CPU oracle (5 Resnet-9 G + 5 NLayer D, GAN+SmoothL1+Adam), batch {batch}, "
                          f"{size}x{size} tile, {d.get('total_seconds', d['seconds']):.1f} s of CPU work, {d['seconds']:.1f} s per step" + ('' if size == args.size else f' (scaled to {args.size}x{args.size}-tile units by pixel count)')}
    return {'value': None, 'unit': 'tiles/s', 'cores': usable_cores(), 'kind': 'port', 'sample': f'CPU oracle step did not finish within the time limit ({last})'}


def backend_of(precision):
    """the ops backend a precision policy launches through: 'fp16' -> libdeepliif_hip_f16.so, everything else -> libdeepliif_hip.so"""
    from deepliif_amd import ops
    with ops.half_mode('fp16' if precision == 'fp16' else 'bf16'):
        return ops.impl()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=8, help='tiles per GPU per step')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--ngf', type=int, default=64, help='generator / discriminator width; the contract line uses 64 (smaller values only for launch-path tests)')
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'fp32', 'fp32_bf16mma', 'fp16'],
                    help="'fp16' (IEEE half storage + MFMA operands, libdeepliif_hip_f16.so) is an INFERENCE policy: --workload infer / wsi only")
    ap.add_argument('--norm', default='instance', choices=['instance', 'batch'])
    ap.add_argument('--workload', default='train', choices=['train', 'train18', 'ext', 'infer', 'wsi'],
                    help="train = BASELINE's 5G+5D step (the contract line); train18 = the real DeepLIIF configuration (modalities_no=4, seg_gen: "
                         '4 Resnet-9 + 5 UNet-512 generators + 9 discriminators, SURVEY 8d); ext = BASELINE configs[3], DeepLIIFExt with 2 modalities: '
                         '2 Resnet-9 + 2 UNet-512 (9-channel input) generators, 2 + 2 discriminators (6 / 12 channels); infer = configs[1]; '
                         'wsi = configs[4], tile-parallel whole-slide inference (synthetic uint8 region, 512 tiles, overlap 32)')
    ap.add_argument('--region', type=int, default=20000, help='wsi workload: side of the synthetic square region in pixels')
    ap.add_argument('--full', action='store_true', help='after the headline, everything else the benchmark measures: per-launch roofline events in the timed steps '
                    '(+ the one-stream and no-events passes, the MFMA probe), the strict-parity leg, hipGraph replay, the exchange profile, policy_vs_strict, '
                    'the whole-slide pass, the CPU baselines and other_workloads; the --no-* options below switch single legs off')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help='write what the timed path computed in its last step to DIR/<name>.npy '
                    f'(float32 / float64; outputs larger than {DUMP_SAMPLE} elements as a fixed, seeded sample; at most {DUMP_LIMIT_BYTES >> 20} MB)')
    ap.add_argument('--no-timer-check', action='store_true', help='skip the second pass that times the same steps WITHOUT the per-launch events '
                    '(roofline.timer_overhead)')
    ap.add_argument('--no-strict', action='store_true', help='skip the strict-parity (fp32 policy) leg')
    ap.add_argument('--no-graph', action='store_true', help='skip the hipGraph-replay leg (the same steps replayed from a captured graph, models.StepGraph)')
    ap.add_argument('--strict', action='store_true', help='time the strict-parity leg also when WORLD_SIZE > 1 (by default a multi-GPU run only carries the '
                    'headline policy: the scaling curve should not pay for a second model and 8 more steps per rank)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--cpu-batch', type=int, default=1, help='batch size of the cpu_baseline leg: 1 = the reference default (cli.py:110) and a ~15 s sample; '
                    '8 = the per-GPU batch of the GPU line (SURVEY 8d asks for both), ~2 minutes of CPU work')
    ap.add_argument('--no-cpu-baseline-n8', action='store_true', help='skip the second CPU leg at the per-GPU batch of the GPU line (batch 8: 1 warm-up + up to 3 '
                    'steps inside a 100 s budget, about 2 minutes of CPU work)')
    ap.add_argument('--cpu-baseline-n8-full', action='store_true', help='time the second CPU leg ON SPEC: batch 8 at 512x512, 1 warm-up + 1 step (~100-200 s, ~105 GB of host '
                    'memory) instead of the scaled 256x256 sample; writes gpurun_out/cpu_baseline_n8_full.json')
    ap.add_argument('--no-other-workloads', action='store_true', help='the default train run appends short measurements of the infer / train18 / ext / wsi workloads '
                    '(other_workloads); this skips them')
    ap.add_argument('--no-wsi-whole', action='store_true', help='wsi workload: skip the end-to-end pass over the WHOLE region (all tiles + gather of the bands + stitch)')
    ap.add_argument('--cpu-baseline-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--cpu-infer-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--cpu-budget', type=float, default=45.0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.precision == 'fp16' and args.workload not in ('infer', 'wsi'):
        ap.error("--precision fp16 is an inference policy (gradients of this model underflow IEEE half): use it with --workload infer or wsi")
    if args.cpu_baseline_child:
        return cpu_baseline_child(args.norm, args.size, args.cpu_batch, args.cpu_budget)
    if args.cpu_infer_child:
        return cpu_infer_child(args.size)

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # not under torchrun: become `python -m torch.distributed.run --nproc-per-node N bench.py <same arguments>` (one process per
        # GPU over RCCL); rank 0 of that job prints the one JSON line
        # --standalone: torchrun's own c10d rendezvous picks (and keeps) a free port itself -- binding port 0 here, closing the socket and
        # handing the number over would leave a window in which another process can take it
        os.execv(sys.executable, [sys.executable, '-m', 'torch.distributed.run', '--standalone', '--local-addr', '127.0.0.1', '--nnodes=1',
                                  f'--nproc-per-node={args.gpus}', os.path.abspath(__file__)] + sys.argv[1:])

    # The contract is ONE JSON line on stdout.  Libraries write there too -- RCCL prints a version banner through C stdio, which is flushed at
    # exit, i.e. AFTER a Python-level print (seen on the one-rank RCCL run: the last line of stdout was "Librccl path : ...") -- so for the
    # whole run descriptor 1 points at stderr (every rank) and rank 0 writes the line to the saved descriptor at the end.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    from deepliif_amd import distributed as D
    from deepliif_amd import models as M
    from deepliif_amd import ops
    backend = os.environ.get('DL_BENCH_BACKEND', 'nccl')         # 'gloo' + DL_BENCH_DRYRUN=1: launch-path test without GPUs (tests/test_bench_launch.py)
    rank, world, local_rank = D.init_process_group_from_env(backend)
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}'
    dry = os.environ.get('DL_BENCH_DRYRUN') == '1'
    if dry:
        # launch-path test on a GPU-less machine: CPU tensors through the test-suite's emulated backend (tests/fake_backend.py); the numbers
        # mean nothing and the line says so
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import fake_backend
        fake_backend.install()
        dev = torch.device('cpu')
        M.BaseModel._device_from_opt = lambda self, opt: torch.device('cpu')
        M.BaseModel._net_gpu_ids = lambda self: []
    else:
        torch.cuda.set_device(local_rank)
        dev = torch.device('cuda', local_rank)
    sys.stdout = open(os.devnull, 'w')      # the model classes print like the reference does; the contract is ONE JSON line
    n, s = args.batch, args.size

    def synth(seed):
        g = torch.Generator().manual_seed(seed + 1000 * rank)       # distinct tiles per rank (data-parallel shards)
        return (torch.rand(n, 3, s, s, generator=g) * 2 - 1).to(dev)

    def sync():
        if not dry:
            torch.cuda.synchronize()

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        sync()

    last_batch = {}
    wsi_state = {'bands': None}
    whole_slide = None

    infer_state = {}

    def build(precision):
        """-> (step function, model or None, GF per tile, dominant conv shape, workload description) for args.workload on `precision`"""
        torch.manual_seed(0)
        a = argparse.Namespace(**vars(args))
        a.precision = precision
        dom = (n, s // 4, s // 4, 4 * args.ngf)
        if args.workload == 'train':
            opt = make_opt(a, local_rank)
            model = M.create_model(opt)
            model.setup(opt)
            batch = {'A': synth(1234), 'B': [synth(1235 + i) for i in range(5)], 'A_paths': ['synthetic']}
            last_batch[precision] = batch
            return (lambda: (model.set_input(batch), model.optimize_parameters())), model, GF_PER_TILE_TRAIN_5R5D, dom, \
                'DeepLIIF train step, 5x Resnet-9block G + 5x NLayerD(n=4), GAN+SmoothL1+Adam (BASELINE configs[2] per GPU)'
        if args.workload == 'ext':
            opt = make_opt(a, local_rank, M=2, seg_gen=True)
            opt.model, opt.net_ds = 'DeepLIIFExt', 'n_layers'
            opt.loss_G_weights = opt.loss_D_weights = opt.seg_weights = [0.5, 0.5]
            model = M.create_model(opt)
            model.setup(opt)
            batch = {'A': synth(1234), 'B': [synth(1235 + i) for i in range(2)], 'BS': [synth(1255 + i) for i in range(2)], 'A_paths': ['synthetic']}
            # per tile: generators forward + 2x backward; every discriminator: 2 forwards + 2x2 backward in backward_D, 1 forward + 1 dgrad
            # in backward_G = 8 forward-equivalents (the accounting SURVEY 8d uses for the 5G+5D figure: 40 x 21.8 for 5 D)
            last_batch[precision] = batch
            return (lambda: (model.set_input(batch), model.optimize_parameters())), model, 3 * (2 * 396.4 + 2 * 49.2) + 8 * (2 * 21.8 + 2 * 22.6), dom, \
                ('DeepLIIFExt train step, modalities_no=2: 2x Resnet-9block + 2x UNet-512 (9-ch in) generators, 2x NLayerD (6 ch) + 2x NLayerD '
                 '(12 ch), GAN/LSGAN+SmoothL1+Adam (BASELINE configs[3])')
        if args.workload == 'train18':
            opt = make_opt(a, local_rank, M=4, seg_gen=True)
            model = M.create_model(opt)
            model.setup(opt)
            batch = {'A': synth(1234), 'B': [synth(1235 + i) for i in range(5)], 'A_paths': ['synthetic']}      # 4 modalities + seg target
            last_batch[precision] = batch
            return (lambda: (model.set_input(batch), model.optimize_parameters())), model, GF_PER_TILE_TRAIN_18NETS, dom, \
                ('real DeepLIIF train step (modalities_no=4, seg_gen=True): 4x Resnet-9block + 5x UNet-512 generators, 4 + 5 NLayerD(n=4), '
                 'GAN/LSGAN+SmoothL1+Adam (SURVEY 8d)')
        from deepliif_amd import inference as I
        iopt = types.SimpleNamespace(model='DeepLIIF', modalities_no=4, seg_gen=True, mod_id_seg='S', input_id=0, input_nc=3, output_nc=3,
                                     ngf=args.ngf, norm='batch', padding='zero', net_g='resnet_9blocks', net_gs='unet_512', input_no=1, scale_size=s,
                                     modalities_names=['IHC', 'Hema', 'DAPI', 'Lap2', 'Marker'], gpu_ids=[local_rank])
        nets = I.build_generators(iopt, dev, precision)
        sw = [0.25, 0.15, 0.25, 0.1, 0.25]
        if args.workload == 'infer':
            tiles = synth(1234)
            infer_state.update(nets=nets, tiles=tiles, opt=iopt, sw=sw)
            return (lambda: infer_state.update(out=I.run_generators(tiles, nets, iopt, seg_weights=sw))), None, GF_PER_TILE_INFER, dom, \
                'DeepLIIF inference, 4x Resnet-9block + 5x UNet-512 generators + weighted seg sum (BASELINE configs[1])'
        # wsi: one synthetic region, identical on every rank (seeded noise, so no tile is_empty); rank r infers its band of tile rows
        R = args.region
        g = torch.Generator(device=dev).manual_seed(77)
        region = torch.randint(0, 256, (R, R, 3), dtype=torch.uint8, device=dev, generator=g)
        def run(limit):
            wsi_state['bands'] = I.infer_region([region], s, s // 16, nets, iopt, seg_weights=sw, batch_size=n, rank=rank, world=world, limit_tiles=limit)
        return run, None, GF_PER_TILE_INFER, dom, \
            (f'tile-parallel whole-slide inference: synthetic {R}x{R} uint8 region in HBM, tile {s}, overlap {s // 16}, crop + is_empty + 4x Resnet-9block '
             f'+ 5x UNet-512 + uint8 stitch on the GPU, batches of {n} tiles, one band of tile rows per rank (BASELINE configs[4])')

    def timed(step, warmup, steps, timer=None):
        for _ in range(warmup):
            step()
        barrier()
        if timer is not None:
            timer.enabled = True
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        barrier()
        dt = time.perf_counter() - t0
        if timer is not None:
            timer.enabled = False
        if world > 1:
            t = torch.tensor([dt], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    step, model, gf_per_tile, dom_shape, workload = build(args.precision)
    exchange_report = None
    # how many ranks the collective backend REALLY spans: a sum all-reduce of ones (not the environment variable)
    ranks_seen = world
    if world > 1:
        one = torch.ones(1, device=dev)
        torch.distributed.all_reduce(one)
        sync()
        ranks_seen = int(round(float(one.item())))

    # ---- strict-parity leg, part 1 (before any optimizer step): distance of the headline policy from the strict policy on this batch
    strict = None
    want_strict = args.full and (not args.no_strict) and args.precision != 'fp32' and args.workload in ('train', 'train18', 'ext') and (world == 1 or args.strict)
    if want_strict:
        sstep, smodel, _, _, _ = build('fp32')
        for mdl in (model, smodel):
            mdl.set_input(mdl_batch(mdl, args, synth))
            mdl.calculate_losses()
        sync()
        la, lb = model.get_current_losses(), smodel.get_current_losses()
        img_err = 0.0
        for k in [k for k in model.visual_names if k.startswith('fake_B')]:
            if hasattr(model, k) and hasattr(smodel, k):
                a_, b_ = getattr(model, k).float(), getattr(smodel, k).float()
                img_err = max(img_err, float((a_ - b_).abs().max() / b_.abs().max().clamp_min(1e-30)))
        loss_err = max(abs(la[k] - lb[k]) / max(abs(lb[k]), 1e-3) for k in la)
        strict = {'dtype': 'f32 storage, split-bf16x3 MFMA (fp32-class products)', 'asserted_vs_oracle': 'network outputs / step-0 losses <= 1e-3 '
                  '(tests/test_gpu_networks.py, tests/test_gpu_fullsize_step.py: the benched step itself; profiles/parity_errors_r05.json)',
                  'headline_vs_strict': {'what': f'{args.precision} policy vs strict policy, same weights, this batch, before any update',
                                         'generated_images_max_abs_over_max': round(img_err, 6), 'losses_max_rel': round(float(loss_err), 6)}}

    if args.workload == 'wsi':
        from deepliif_amd.tiling import TilePlan, split_rows
        plan = TilePlan(args.region, args.region, s, s // 16)
        rows = split_rows(len(plan.ys), world)
        per_rank = min((r1 - r0) * len(plan.xs) for r0, r1 in rows)           # every rank processes the same number of tiles in the timed region
        n_batches = min(args.steps, per_rank // n)
        assert n_batches >= 1, 'region too small for this many ranks'
        timer = KernelTimer(backend_of(args.precision), dom_shape) if args.full and not dry else types.SimpleNamespace(mean_seconds=lambda: None, pairs=[], kernel='?', enabled=False)
        step(n * max(args.warmup, 1))
        barrier()
        timer.enabled = True
        t0 = time.perf_counter()
        step(n * n_batches)
        barrier()
        dt = time.perf_counter() - t0
        timer.enabled = False
        if world > 1:
            t = torch.tensor([dt], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt = float(t.item())
        args.steps = n_batches
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, step_outputs(None, wsi_state['bands']))
        if args.full and not args.no_wsi_whole:
            # configs[4] end to end, once: EVERY tile of this rank's band (crop, is_empty, 9 generators, uint8 paste), then the bands of all ranks gathered on rank 0
            # (inference.gather_bands) -- the stitched result images exist on rank 0 when the clock stops
            from deepliif_amd import inference as I2
            barrier()
            t0 = time.perf_counter()
            step(None)
            local, band = wsi_state['bands']
            keys = sorted(local.keys()) if local else []
            if world > 1:
                allk = [None] * world
                torch.distributed.all_gather_object(allk, keys)
                keys = sorted({k for ks in allk for k in ks})
            full = I2.gather_bands(local, band, args.region, args.region, keys, rank, world)
            barrier()
            wdt = time.perf_counter() - t0
            if world > 1:
                t = torch.tensor([wdt], device=dev, dtype=torch.float64)
                torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
                wdt = float(t.item())
            ntiles = len(plan.ys) * len(plan.xs)
            whole_slide = {'tiles': ntiles, 'seconds': round(wdt, 3), 'tiles_per_s': round(ntiles / wdt, 2), 'result_images': len(keys),
                           'what': f'the whole {args.region}x{args.region} region once: every tile of every band (crop + is_empty + 9 generators + uint8 paste), bands gathered on '
                                   f'rank 0; wall clock between two barriers, max over ranks'}
            del full, local
            wsi_state['bands'] = None
    else:
        timer = KernelTimer(backend_of(args.precision), dom_shape) if args.full and not dry else types.SimpleNamespace(mean_seconds=lambda: None, pairs=[], kernel='?', enabled=False)
        exch = getattr(model, 'exchange', None) if (args.full and model is not None and D.active()) else None
        if exch is not None:
            exch.profile = not dry          # device-side events around the waits of GradExchanger.finish(): the exposed part of the exchange
        dt = timed(step, args.warmup, args.steps, timer)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, step_outputs(model, infer_state.get('out')))
        if exch is not None:
            exch.profile = False
            sync()
            exposed = exch.exposed_ms()
            last = {p['tag']: p for p in exch.pass_log[-2:]}
            exchange_report = {'what': 'data-parallel gradient exchange per step (sum all-reduce of the flat fp32 gradients, one per network slice, launched from '
                                       'tape markers during backward; 1/world folded into Adam): *_ms_exposed = device time the compute stream waits in '
                                       'GradExchanger.finish(), mean over the timed steps',
                               'd_ms_exposed': round(exposed.get('D', 0.0), 3) if exposed else None, 'g_ms_exposed': round(exposed.get('G', 0.0), 3) if exposed else None,
                               'bytes': {k: v['bytes'] for k, v in last.items()}, 'buckets': {k: v['calls'] for k, v in last.items()},
                               'early_ranges': {k: v['early_ranges'] for k, v in last.items()},
                               'wire_dtype': 'bf16 (DL_DP_GRAD_BF16=1: round, sum, widen)' if D.GRAD_BF16 else 'fp32'}

    tiles_total = args.steps * n * world
    value = tiles_total / dt

    def n_streams(m):
        return len(getattr(m, '_streams', None) or []) if m is not None else 0

    def solo_pass(stepfn, m, tm):
        """Branch streams (models.BaseModel._branch_streams): launches of different streams share the GPU, so the event-bracketed duration of ONE launch inside
        the timed region measures contention, not the kernel.  The same steps once more on ONE stream (streams switched off on the same model, per-launch
        events on) give the launch duration the roofline block is about; the concurrent figure stays in the line next to it."""
        conc = (tm.mean_seconds(), tm.median_seconds(), len(tm.pairs))
        saved, m._streams = m._streams, None
        try:
            tm.pairs, tm.pairs_add = [], []
            sdt_ = timed(stepfn, 1, args.steps, tm)
        finally:
            m._streams = saved
        return conc, sdt_
    # what do the event pairs around the dominant launches cost?  the same K steps once more, events off (same process, same state of the clocks)
    dt_noev = None
    if args.workload != 'wsi' and not dry and timer.pairs and not args.no_timer_check:
        dt_noev = timed(step, 1, args.steps)

    conc_info, dt_solo = None, None
    if n_streams(model) > 1 and not dry and timer.pairs:
        conc_info, dt_solo = solo_pass(step, model, timer)
    infer_solo = None
    if args.workload in ('infer', 'wsi') and not dry and timer.pairs:
        from deepliif_amd import inference as I3
        if I3._INFER_STREAMS > 1:
            # the inference DAG runs its chains G_i -> GS_i on DL_INFER_STREAMS streams: as above, launch durations come from one more pass on ONE stream
            conc_info = (timer.mean_seconds(), timer.median_seconds(), len(timer.pairs))
            saved_streams, I3._INFER_STREAMS = I3._INFER_STREAMS, 1
            try:
                timer.pairs = []
                if args.workload == 'wsi':
                    step(n)
                    barrier()
                    timer.enabled = True
                    t0 = time.perf_counter()
                    step(n * args.steps)
                    barrier()
                    dt_solo = time.perf_counter() - t0
                    timer.enabled = False
                else:
                    dt_solo = timed(step, 1, args.steps, timer)
            finally:
                I3._INFER_STREAMS = saved_streams
            infer_solo = saved_streams
    kt = timer.mean_seconds()
    kt_median = timer.median_seconds() if hasattr(timer, 'median_seconds') else kt
    kt_add, n_pairs_add = (timer.mean_seconds_add(), len(timer.pairs_add)) if hasattr(timer, 'pairs_add') else (None, 0)

    n_pairs, dom_kernel = len(timer.pairs), timer.kernel
    flops_per_launch = 2.0 * n * (s // 4) * (s // 4) * (4 * args.ngf) * (4 * args.ngf) * 9

    # ---- strict-parity leg, part 2: the same workload timed on the strict policy, with its own roofline block (same layer shape, same
    # ALGORITHMIC flops per launch -- the three bf16 MFMA passes per product are the policy's cost, not useful work)
    if want_strict:
        ssteps, swarm = args.steps, args.warmup            # same schedule as the headline (r03 timed 8 steps / 1 warm-up: VERDICT r3 #9)
        if hasattr(timer, '_orig'):
            timer.pairs, timer.pairs_add, timer.kernel = [], [], '?'
        sdt = timed(sstep, swarm, ssteps, timer if hasattr(timer, '_orig') else None)
        strict.update({'value': round(ssteps * n * world / sdt, 3), 'unit': 'tiles/s', 'ms_per_step': round(sdt / ssteps * 1e3, 3), 'steps': ssteps, 'warmup': swarm,
                       'model_tflops': round(ssteps * n * world / sdt * gf_per_tile / 1e3, 1)})
        sconc, sdt_solo = None, None
        if n_streams(smodel) > 1 and hasattr(timer, '_orig') and timer.pairs:
            sconc, sdt_solo = solo_pass(sstep, smodel, timer)
        skt = timer.mean_seconds() if hasattr(timer, '_orig') else None
        if skt:
            sach = flops_per_launch / skt / 1e12
            strict['roofline'] = {'bound': 'mfma', 'achieved': round(sach, 1), 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(sach / PEAK_BF16_TFLOPS, 4),
                                  'mfma_pipe_frac': round(3 * sach / PEAK_BF16_TFLOPS, 4), 'traffic': None,
                                  'kernel': f'{timer.kernel}: 3x3 256->256 @ {n}x{s // 4}x{s // 4}, ResnetBlock conv fwd + dgrad (fp32 storage, split-bf16 x3); timed by events around the host call',
                                  'launches_timed': len(timer.pairs), 'avg_launch_us': round(skt * 1e6, 2), 'median_launch_us': round(timer.median_seconds() * 1e6, 2),
                                  'note': 'achieved = algorithmic conv flops per launch / launch time; mfma_pipe_frac counts the 3 MFMA passes the policy issues per product'}
            if sconc is not None:
                strict['roofline'].update({'launch_times_from': f'a second pass of the same {ssteps} steps on ONE stream ({round(sdt_solo / ssteps * 1e3, 3)} ms/step)',
                                           'concurrent_avg_launch_us': round(sconc[0] * 1e6, 2), 'concurrent_median_launch_us': round(sconc[1] * 1e6, 2)})
            strict['streams'] = n_streams(smodel) or 1
            try:        # HBM-side bytes per launch from the committed --pmc passes over this kernel and shape (not measured in this run)
                with open(os.path.join(ROOT, 'profiles', STRICT_PMC_FILE)) as f:
                    spmc = json.load(f)
                if (n, s, args.ngf) == (8, 512, 64) and timer.kernel.split('<')[0] in spmc.get('kernel', ''):
                    strict['roofline']['traffic'] = spmc['traffic_bytes']
                    strict['roofline']['traffic_note'] = (f'NOT measured in this run: 2*FETCH_SIZE + WRITE_SIZE of separate rocprofv3 --pmc passes over the same kernel and '
                                                          f'shape (profiles/{STRICT_PMC_FILE}); algorithmic bytes {spmc["algorithmic_bytes"]}')
            except Exception:
                pass
        del smodel, sstep
    if strict is not None:
        # multi-step fidelity of BOTH policies against the oracle (tests/test_gpu_trajectory.py): the committed summary of the 100-step curves, not measured here
        try:
            with open(os.path.join(ROOT, 'profiles', TRAJECTORY_FILE)) as f:
                tj = json.load(f)
            strict['trajectory'] = {'what': 'mean over steps and the 20 losses of |L - L_oracle| / max(1, |L_oracle|) along optimize_parameters() trajectories from identical weights '
                                            'and batches; oracle_noise = the oracle against itself with fp32-sized rounding noise on every conv output (the band two correct '
                                            'fp32-class implementations differ by)',
                                    'config': {k: tj['config'][k] for k in ('steps', 'ngf', 'size', 'batch', 'norm')}, 'step0_max': tj.get('step0_max'), 'first10_max': tj['first10_max'], 'mean': tj['mean'],
                                    'last20_mean_curve': tj['last20_mean_curve'], 'bands_asserted': tj.get('bands'),
                                    'source': f'NOT measured in this run: profiles/{TRAJECTORY_FILE}, written by tests/test_gpu_trajectory.py on an MI355X'}
        except Exception:
            pass

    # ---- hipGraph leg: the same steps replayed from ONE captured graph (models.StepGraph): what the step costs when Python is out of it.  The headline
    # `value` above is the EAGER step (it carries the per-launch events the roofline block needs); this leg runs LAST, on the same model.
    graph_report = None
    if args.full and not args.no_graph and not dry and model is not None and world == 1 and args.workload in ('train', 'train18', 'ext') and args.precision in last_batch:
        try:
            sg = M.StepGraph(model, warmup=2)
        except Exception as exc:
            sg = types.SimpleNamespace(why_eager=f'StepGraph: {exc}'[:200])
        if sg.why_eager is None:
            gb = last_batch[args.precision]
            try:
                for _ in range(4):                   # two eager steps in graph mode, the capture (+ its replay), one replay
                    sg.step(gb)
                barrier()
                host = 0.0
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    h0 = time.perf_counter()
                    sg.step(gb)
                    host += time.perf_counter() - h0
                barrier()
                gdt = time.perf_counter() - t0
            except Exception as exc:              # a measurement aid must never take the contract line down
                gdt = None
                graph_report = {'error': str(exc)[:300]}
            if gdt is not None:
                graph_report = {'value': round(args.steps * n / gdt, 3), 'unit': 'tiles/s', 'ms_per_step': round(gdt / args.steps * 1e3, 3), 'steps': args.steps,
                            'host_ms_per_step': round(host / args.steps * 1e3, 3),
                            'what': 'optimize_parameters() captured once in a hipGraph and replayed (models.StepGraph; bit-identical to the eager step, '
                                    'tests/test_gpu_graph.py); host_ms_per_step = Python time to issue one step (batch copy into the static tensors, Adam scalars, '
                                    'one graph launch) -- the eager step issues ~2 400 launches from Python'}
        else:
            graph_report = {'skipped': sg.why_eager}
    roofline = None
    traffic, traffic_note = None, None
    try:        # HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes (tools/gpu_pmc.sh)
        with open(os.path.join(ROOT, 'profiles', PMC_FILE)) as f:
            pmc = json.load(f)
            # counters belong to ONE kernel at ONE shape: report them only when that is what this run dispatched
            same = (n, s, args.precision, args.ngf) == (8, 512, 'bf16', 64) and dom_kernel != '?' and dom_kernel.split('<')[0] in pmc.get('kernel', '')
            traffic = pmc['traffic_bytes'] if same else None
            traffic_note = (f'NOT measured in this run: 2*FETCH_SIZE + WRITE_SIZE of separate rocprofv3 --pmc passes over the same kernel and shape '
                            f'(profiles/{PMC_FILE}, collected with tools/gpu_r06_pmc.sh on forward launches only)') if same else None
    except Exception:
        traffic = None
    if kt:
        ach = flops_per_launch / kt / 1e12
        roofline = {'bound': 'mfma', 'achieved': round(ach, 1), 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(ach / PEAK_BF16_TFLOPS, 4),
                    'traffic': traffic, 'traffic_note': traffic_note,
                    'kernel': f'{dom_kernel}: 3x3 256->256 @ {n}x{s // 4}x{s // 4}, ResnetBlock conv ' + ('fwd + dgrad' if args.workload not in ('infer', 'wsi') else 'fwd only') + '; timed by events around the host call',
                    'launches_timed': n_pairs, 'avg_launch_us': round(kt * 1e6, 2), 'median_launch_us': round(kt_median * 1e6, 2)}
        if kt_add:
            # a quarter of the block's conv launches (the first conv's data gradient) also add the skip-connection gradient in their store pass (dl_conv_forward_add,
            # r06): the same 154.6 GF but 67 MB more algorithmic bytes -- a different launch, kept out of `avg_launch_us` (whose definition did not change) and shown here
            ach_add = flops_per_launch / kt_add / 1e12
            roofline['with_skip_add'] = {'launches_timed': n_pairs_add, 'avg_launch_us': round(kt_add * 1e6, 2), 'achieved': round(ach_add, 1), 'frac': round(ach_add / PEAK_BF16_TFLOPS, 4),
                                         'algorithmic_bytes': 3 * n * (s // 4) * (s // 4) * 4 * args.ngf * 2 + (4 * args.ngf) ** 2 * 9 * 2,
                                         'all_block_conv_launches_avg_us': round((kt * n_pairs + kt_add * n_pairs_add) / max(n_pairs + n_pairs_add, 1) * 1e6, 2),
                                         'what': 'the data gradient of a ResnetBlock\'s first conv + the gradient that came down the skip connection, one pass (replaces a separate '
                                                 'axpby over 3 x 67 MB per block)'}
        if not dry and rank == 0 and args.workload == 'train':
            try:
                sus = mfma_sustained(dev)
                roofline['sustained'] = {**sus, 'what': 'register-resident v_mfma_f32_32x32x16_bf16 loop on this box (dl_probe_mfma_sustained), random N(0,1) / zero operand '
                                                        'bits: the clock the matrix cores hold under their own power draw is data-dependent',
                                         'frac_of_sustained_random': round(ach / sus['random_tflops'], 4)}
            except Exception as exc:          # measurement aid only
                roofline['sustained'] = {'error': str(exc)[:200]}
        if conc_info is not None:
            roofline.update({'launch_times_from': f'a second pass of the same {args.steps} steps on ONE stream, per-launch events on ({round(dt_solo / args.steps * 1e3, 3)} ms/step): the timed region '
                                                  f'runs the independent branches / chains on {infer_solo or n_streams(model)} HIP streams, where the event-bracketed duration of one launch measures the '
                                                  'share of the GPU it got, not the kernel',
                             'one_stream_ms_per_step': round(dt_solo / args.steps * 1e3, 3),
                             'concurrent_avg_launch_us': round(conc_info[0] * 1e6, 2), 'concurrent_median_launch_us': round(conc_info[1] * 1e6, 2),
                             'concurrent_launches_timed': conc_info[2]})
        if dt_noev is not None:
            roofline['timer_overhead'] = {'ms_per_step_with_events': round(dt / args.steps * 1e3, 3), 'ms_per_step_without_events': round(dt_noev / args.steps * 1e3, 3),
                                          'relative': round(dt / dt_noev - 1.0, 5),
                                          'what': f'the {args.steps} timed steps carry {n_pairs} hipEvent pairs (every {KernelTimer.EVERY}th dominant launch); the same steps were timed once more '
                                                  'without them (value / ms_per_step are the run WITH the events)'}
    out = {
        'metric': {'train': '512x512 tiles/s train-step (5G+5D)', 'train18': '512x512 tiles/s train-step (real DeepLIIF: 9 G + 9 D)', 'ext': '512x512 tiles/s train-step (DeepLIIFExt, 2 modalities: 4 G + 4 D)',
                   'infer': '512x512 tiles/s inference (4 Resnet-9 + 5 UNet-512)', 'wsi': '512x512 tiles/s whole-slide inference (tile-parallel, crop + 9 generators + stitch)'}[args.workload],
        'value': round(value, 3), 'unit': 'tiles/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': round(dt / args.steps * 1e3, 3), 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'bf16' if args.precision == 'bf16' else 'f16' if args.precision == 'fp16' else ('f32(split-bf16x3 MFMA)' if args.precision == 'fp32' else 'f32 storage/bf16 MFMA'),
        'data': 'synthetic U(-1,1) tiles (seeds 1234..), N(0,0.02) random-init weights (torch.manual_seed(0)), dropout off, VGG loss off' if args.workload != 'wsi'
                else 'synthetic uint8 noise region (seed 77), N(0,0.02) random-init weights (torch.manual_seed(0))',
        'config': {'workload': workload, 'tile': f'{s}x{s}x3', 'batch_per_gpu': n, 'global_batch': n * world, 'norm': args.norm if args.workload not in ('infer', 'wsi') else 'batch (per-sample statistics)',
                   'precision_policy': args.precision, 'parallelism': f'dp{world}', 'rccl_ranks': ranks_seen, 'backend': backend},
        'model_tflops': round(value * gf_per_tile / 1e3, 1),
        'model_frac_of_bf16_peak': round(value * gf_per_tile / 1e3 / (PEAK_BF16_TFLOPS * world), 4),
        'roofline': roofline,
        'strict_parity': strict,
    }
    if exchange_report is not None:
        out['exchange'] = exchange_report
    if graph_report is not None:
        out['graph_replay'] = graph_report
    out['config']['launch_mode'] = 'eager (one HIP launch per kernel from Python; see graph_replay for the captured-graph step)'
    ns = len(getattr(model, '_streams', None) or []) if model is not None else 0
    out['config']['streams'] = ns if ns else 1          # DL_STREAMS: HIP streams the independent (G_i, D_i) branches of the step are spread over (models.BaseModel._branch_streams)
    if args.workload in ('infer', 'wsi') and not dry:
        from deepliif_amd import inference as I_
        out['config']['streams'] = I_._INFER_STREAMS      # DL_INFER_STREAMS (opt-in): the chains G_i -> GS_i of the inference DAG on their own streams
    if args.precision == 'bf16' and strict is not None:
        out['dtype_note'] = ('headline dtype bf16 is the throughput policy (BASELINE.json quotes the target on bf16 MFMA); it does NOT meet the 1e-3 parity bar -- '
                             'its measured distance from the strict policy is in strict_parity.headline_vs_strict; the strict policy (asserted at 1e-3 against '
                             'the oracle by the GPU tests) is timed on the same workload in strict_parity.value')
    if args.full and args.workload == 'infer' and infer_state and not dry and rank == 0 and args.precision != 'fp32':
        # how far this policy's output images are from the strict policy's (the one the GPU tests hold at 1e-3 against the oracle), same weights, same tiles:
        # max |difference| relative to the strict output's range, per result key, and the share of 8-bit channel values (tensor2im) that differ by more than one level
        from deepliif_amd import inference as I_
        st = infer_state

        def run_on(p):
            for net in st['nets'].values():
                net.set_precision(p)
            with torch.no_grad():
                return {k: v.float() for k, v in I_.run_generators(st['tiles'], st['nets'], st['opt'], seg_weights=st['sw']).items()}
        got, ref = run_on(args.precision), run_on('fp32')
        run_on(args.precision)
        u8 = lambda t: ((t.clamp(-1, 1) + 1) * 127.5).to(torch.int32)
        out['policy_vs_strict'] = {
            'what': f'{args.precision} policy vs strict (fp32) policy, same weights and tiles: max |diff| / max |strict| per output; u8 = share of 8-bit values off by > 1 level',
            'max_rel': {k: round(float((got[k] - ref[k]).abs().max() / ref[k].abs().max()), 5) for k in ref},
            'u8_off_by_more_than_1': {k: round(float(((u8(got[k]) - u8(ref[k])).abs() > 1).float().mean()), 5) for k in ref}}
    if dry:
        out['data'] = 'DRY RUN on CPU through the test emulation backend (launch-path check only; numbers are meaningless)'
    if whole_slide is not None:
        out['whole_slide'] = whole_slide
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and args.workload == 'infer' and not dry:
        out['cpu_baseline'] = cpu_baseline_infer(args)
    elif args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and args.workload == 'train' and not dry:
        out['cpu_baseline'] = cpu_baseline(args)
        if not args.no_cpu_baseline_n8 and args.batch != args.cpu_batch:
            # "N=1 (reference default batch_size) and N=8": the same oracle at the GPU line's per-GPU batch.  A batch-8 step at
            # 512x512 takes ~100 s on 16 host cores (measured r03), so this leg runs 256x256 tiles (reported in 512x512-tile equivalents by
            # pixel count, like the fallback of the N=1 leg): 1 warm-up + 2-3 steps, about a minute of CPU work
            if args.cpu_baseline_n8_full:
                # SURVEY 8(d) on-spec: batch 8 at 512 x 512 on the host cores, 1 warm-up + 1 timed step (~100-200 s and ~105 GB of host memory): behind a flag the
                # driver's command does not set; the result is committed as profiles/r06/cpu_baseline_n8_full.json and quoted by the default run below
                full = cpu_baseline(args, batch=args.batch, budget=1.0, half_tile=False)
                os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
                with open(os.path.join(ROOT, 'gpurun_out', 'cpu_baseline_n8_full.json'), 'w') as f:
                    json.dump(full, f, indent=1)
                out['cpu_baseline_n8'] = full
            else:
                out['cpu_baseline_n8'] = cpu_baseline(args, batch=args.batch, budget=40.0, half_tile=True)
                out['cpu_baseline_n8']['note'] = 'quick leg of the default run: 256x256 tiles scaled by pixel count; the on-spec measurement (batch 8 at 512x512) is in on_spec'
                try:
                    with open(os.path.join(ROOT, 'profiles', N8_FULL_FILE)) as f:
                        out['cpu_baseline_n8']['on_spec'] = dict(json.load(f), source=f'NOT measured in this run: profiles/{N8_FULL_FILE} (bench.py --cpu-baseline-n8-full on an MI355X box)')
                except Exception:
                    pass
    else:
        out['cpu_baseline'] = None
        out['cpu_baseline_note'] = ('runs with --full' if not args.full else 'disabled by --no-cpu-baseline' if args.no_cpu_baseline else
                                    'only timed on rank 0 of a 1-GPU run' if world != 1 else
                                    'the CPU oracle legs are implemented for the train workload (oracle optimize_parameters) and the infer workload (oracle inference DAG)')
    if args.full and rank == 0 and world == 1 and args.workload == 'train' and not dry and not args.no_other_workloads and (n, s, args.ngf) == (8, 512, 64):
        torch.cuda.empty_cache()
        out['other_workloads'] = other_workloads(args)
    if rank == 0:
        os.write(json_fd, (json.dumps(out) + '\n').encode())
    os.close(json_fd)
    if world > 1:
        torch.distributed.destroy_process_group()


def mdl_batch(model, args, synth):
    """the synthetic batch of the workload for `model` (same seeds as the timed steps)"""
    if args.workload == 'ext':
        return {'A': synth(1234), 'B': [synth(1235 + i) for i in range(2)], 'BS': [synth(1255 + i) for i in range(2)], 'A_paths': ['synthetic']}
    return {'A': synth(1234), 'B': [synth(1235 + i) for i in range(5)], 'A_paths': ['synthetic']}


if __name__ == '__main__':
    main()
