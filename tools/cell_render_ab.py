"""What does rendering a stored cell list (postprocessing.cells_to_final_results) cost?  In ONE process, after a warm-up, alternated `--rounds` times,
a device synchronise either side of every window (wall clock), medians reported, on the two shapes tools/cell_outline_time.py uses: 2048 x 2048 with
4 096 discs and 8192 x 8192 from golden_util.synth_cells (61 728 cells), data versions 3 (dicts) and 4 (strings); the original image is on the device and
the results stay there (return_tensors=True):
    from the list     cells_to_final_results(dict): the JSON-like list is walked, flattened and uploaded, then the kernels
    from PackedCells  the same call on pack_cells(dict): the re-threshold cost, kernels only
                      (both under two threshold sets in turn, a median PER SET: the sets count different numbers of cells)
    pack_cells        the flattening and upload alone
    route='host'      the numpy / Python yardstick, at 2048 x 2048 only and run ONCE per version (that run is also the equality check of the GPU
                      route); at 8192 x 8192 it is minutes of Python and is not timed
Per-kernel device times come from one `rocprofv3 --kernel-trace --stats` run per shape of a fresh child process that does nothing but load the
list from a file and render it 1 + `--trace-calls` times: mean per launch, grouped into count / paint / background (mask, merge, flatten,
border flag, background) / fill / boundary / enlarge (two launches per call) / final, and per kernel.  Writes <out> (default profiles/cell_render.json).

    python tools/cell_render_ab.py [--rounds 5] [--small] [--no-trace] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SETS = [dict(size_thresh=None), dict(size_thresh=200, size_thresh_upper=2000, marker_thresh=80)]
STAGES = {'count': ['pp_render_count_kernel'], 'paint': ['pp_render_paint_kernel'],
          'background': ['pp_render_mask_kernel', 'pp_merge_kernel', 'pp_flatten_kernel', 'pp_border_flag_kernel', 'pp_background_kernel'],
          'fill': ['pp_render_fill_kernel'], 'boundary': ['pp_render_boundary_kernel'], 'enlarge': ['pp_enlarge_kernel'], 'final': ['pp_final_kernel']}


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def trace_child(path, calls):
    """the program rocprofv3 traces: the stored list from `path`, rendered 1 + calls times from one PackedCells"""
    import torch
    from deepliif_amd import postprocessing as PP
    with open(path) as f:
        job = json.load(f)
    H, W = job['size']
    orig = torch.full((H, W, 3), 200, dtype=torch.uint8, device='cuda')
    packed = PP.pack_cells(job['data'])
    for i in range(1 + calls):
        PP.cells_to_final_results(packed, orig, return_tensors=True, **SETS[i % 2])
    torch.cuda.synchronize()


def trace(data, size, calls, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'cells.json')
        with open(path, 'w') as f:
            json.dump({'size': list(size), 'data': data}, f, default=int)
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out_dir, '-o', 'render', '--', sys.executable, os.path.abspath(__file__),
               '--trace-child', path, '--trace-calls', str(calls)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=420)
        except (OSError, subprocess.TimeoutExpired) as e:
            return {'error': f'rocprofv3: {e!r}'[:300]}
    if r.returncode != 0:
        return {'error': f'rocprofv3 exited with {r.returncode}: {r.stderr[-400:]}'}
    files = glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        return {'error': 'rocprofv3 wrote no kernel_stats.csv'}
    rows = list(csv.DictReader(open(files[0])))
    out = {'traced_calls': 1 + calls, 'what': 'mean device time per LAUNCH in microseconds, summed over the kernels of the stage', 'stages_us': {}, 'launches_per_call': {}, 'kernels_us': {}}
    for stage, names in STAGES.items():
        hit = [r for r in rows if any(n in r['Name'] for n in names)]
        out['stages_us'][stage] = sum(float(r['TotalDurationNs']) / max(int(r['Calls']), 1) for r in hit) / 1e3
        out['launches_per_call'][stage] = sum(int(r['Calls']) for r in hit) / (1 + calls)
        for r in hit:
            out['kernels_us'][r['Name'].split('(')[0].replace('void ', '')] = float(r['TotalDurationNs']) / max(int(r['Calls']), 1) / 1e3
    per_call = sum(out['stages_us'][s] * (2 if s == 'enlarge' else 1) for s in STAGES)
    out['all_stages_us_per_call'] = per_call
    return out


def measure(name, seg, marker, rounds, host, trace_dir, trace_calls):
    import numpy as np
    import torch
    from deepliif_amd import postprocessing as PP
    H, W = seg.shape[:2]
    seg_d, marker_d = torch.from_numpy(seg).cuda(), torch.from_numpy(marker).cuda()
    orig_d = torch.full((H, W, 3), 200, dtype=torch.uint8, device='cuda')
    rows = []
    for version in (4, 3):
        data = PP.compute_cell_results(seg_d, marker_d, '40x', version=version, route='gpu')
        n = len(data['cells'])
        render = lambda d, k: PP.cells_to_final_results(d, orig_d, return_tensors=True, **SETS[k])
        packed = PP.pack_cells(data)
        warm = [render(data, k) for k in (0, 1)]
        for k in (0, 1):                                                  # both entries agree before anything is timed
            got = render(packed, k)
            assert got[2] == warm[k][2] and torch.equal(got[0], warm[k][0]) and torch.equal(got[1], warm[k][1])
        row = {'shape': name, 'size': [H, W], 'version': version, 'cells': n, 'items': packed.items, 'rounds': rounds, 'counted': [w[2]['num_total'] for w in warm]}
        if host:
            t, want = timed(lambda: PP.cells_to_final_results(data, orig_d, route='host', **SETS[0]))
            assert want[2] == warm[0][2] and np.array_equal(want[0], warm[0][0].cpu().numpy()) and np.array_equal(want[1], warm[0][1].cpu().numpy()), \
                f'{name} v{version}: the routes differ'
            row['route_host_s'] = t
        else:
            row['route_host_s'] = None
            row['route_host_note'] = 'not timed: minutes of Python at this size'
        list_s, packed_s, pack_s = ([], []), ([], []), []          # one series per threshold set: the sets count different numbers of cells
        for _ in range(rounds):
            for k in (0, 1):
                list_s[k].append(timed(lambda: render(data, k))[0])
                packed_s[k].append(timed(lambda: render(packed, k))[0])
            pack_s.append(timed(lambda: PP.pack_cells(data))[0])
        row.update({'gpu_from_list_s': [statistics.median(v) for v in list_s], 'gpu_from_packed_s': [statistics.median(v) for v in packed_s],
                    'pack_cells_s': statistics.median(pack_s), 'all_from_list_s': list_s, 'all_from_packed_s': packed_s})
        if host:                                                          # the host route ran threshold set 0
            row['host_over_gpu_from_list'] = row['route_host_s'] / row['gpu_from_list_s'][0]
            row['host_over_gpu_from_packed'] = row['route_host_s'] / row['gpu_from_packed_s'][0]
        if trace_dir:
            row['kernels'] = trace(data, (H, W), trace_calls, os.path.join(trace_dir, f'{name}_v{version}'))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--small', action='store_true', help='the 2048 x 2048 shape only')
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-calls', type=int, default=5)
    ap.add_argument('--trace-dir', default=None, help='where rocprofv3 writes (default: a temporary directory)')
    ap.add_argument('--trace-child', default=None, metavar='FILE')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cell_render.json'))
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.trace_child, a.trace_calls)
        return
    import torch
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    from cell_outline_time import disc_images, synth_images
    with tempfile.TemporaryDirectory() as tmp:
        tdir = None if a.no_trace else (a.trace_dir or tmp)
        rows = measure('discs_2048', *disc_images(), a.rounds, True, tdir, a.trace_calls)
        if not a.small:
            rows += measure('synth_8192', *synth_images(), a.rounds, False, tdir, a.trace_calls)
    res = {'tool': 'tools/cell_render_ab.py', 'device': torch.cuda.get_device_name(0), 'threshold_sets': [repr(s) for s in SETS], 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({'written': a.out, 'rows': len(rows)}))


if __name__ == '__main__':
    main()
