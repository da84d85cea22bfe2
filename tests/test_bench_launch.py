"""bench.py's launch path without GPUs: `python bench.py --gpus 2` (no torchrun around it) must re-execute itself as one process per
rank, rendezvous on 127.0.0.1 and print exactly ONE JSON line from rank 0 carrying the contract keys (with --full: the strict leg and the exchange too).  DL_BENCH_DRYRUN=1 routes the model
through the test emulation backend on CPU tensors and DL_BENCH_BACKEND=gloo replaces RCCL; the numbers are meaningless by construction."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
def test_bench_self_launches_two_ranks_and_prints_one_json_line():
    env = dict(os.environ, DL_BENCH_DRYRUN='1', DL_BENCH_BACKEND='gloo', OMP_NUM_THREADS='2')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0', '--size', '64', '--batch', '1',
                        '--ngf', '8', '--full', '--no-cpu-baseline', '--strict'], capture_output=True, text=True, timeout=800, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    # the gloo transport itself writes '[Gloo] Rank ...' fragments to stdout from C++, from both ranks at once (RCCL does not): look for the contract
    # line by its first key instead of trying to recognise everything that is NOT it
    lines = [l[l.index('{"metric"'):] for l in r.stdout.splitlines() if '{"metric"' in l]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config',
              'roofline', 'cpu_baseline', 'strict_parity'):
        assert k in d, k
    assert d['n_gpus'] == 2 and d['config']['rccl_ranks'] == 2 and d['config']['global_batch'] == 2 and d['scaling'] == 'weak'
    sp = d['strict_parity']
    assert sp['value'] > 0 and sp['ms_per_step'] > 0 and 0 < sp['headline_vs_strict']['generated_images_max_abs_over_max'] < 0.2
    # the 2-rank line explains itself (VERDICT r3 #8a): ranks counted by a real all-reduce, and the gradient exchange of the last step
    ex = d['exchange']
    assert set(ex['bytes']) == {'G', 'D'} and all(v > 0 for v in ex['bytes'].values()) and all(v >= 1 for v in ex['buckets'].values())
    assert ex['buckets']['G'] >= 6           # 5 generators, the first one (the pass ends with it) in two halves



@pytest.mark.timeout(600)
def test_plain_run_times_the_steps_it_was_given_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full) is the headline only: the requested number of timed steps, ms_per_step, no strict / CPU legs; --dump-outputs writes
    the last step's losses, generated images and parameter samples as float .npy files, the same bytes in two runs with the same arguments."""
    import numpy as np
    env = dict(os.environ, DL_BENCH_DRYRUN='1', DL_BENCH_BACKEND='gloo', OMP_NUM_THREADS='2')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    dumps = []
    for i in range(2):
        d_out = tmp_path / f'out{i}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--size', '64', '--batch', '1',
                            '--ngf', '8', '--dump-outputs', str(d_out)], capture_output=True, text=True, timeout=500, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l[l.index('{"metric"'):] for l in r.stdout.splitlines() if '{"metric"' in l]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert k in d, k
        assert d['steps'] == 3 and d['warmup'] == 1 and d['ms_per_step'] > 0
        assert d['strict_parity'] is None and d['cpu_baseline'] is None and 'other_workloads' not in d and 'graph_replay' not in d
        files = sorted(os.listdir(d_out))
        assert {'loss_G_L1_1.npy', 'fake_B_1.npy', 'param_G1.npy', 'param_D5.npy'} <= set(files), files
        arrays = {f: np.load(d_out / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for f, a in dumps[0].items():
        assert np.array_equal(a, dumps[1][f]), f
