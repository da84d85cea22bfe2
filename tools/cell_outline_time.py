"""What does the per-cell export (postprocessing.compute_cell_results) cost on its two routes?  In ONE process, after a warm-up, alternated `--rounds`
times, a device synchronise either side of every window (wall clock: the host's share is the point), medians reported:
    route='host'  the cell mapping on the GPU, the label mask copied to the host, get_cell_boundary -> make_simple_contour -> encode_cell_data_v4 per
                  cell in Python (the yardstick)
    route='gpu'   the cell mapping on the GPU, dl_pp_outline_count -> scan (numpy) -> dl_pp_outline_emit, dicts / strings built from bulk copies
on two masks: 2048 x 2048 with 4 096 discs of radius 12 (262 144 outline pixels), and 8192 x 8192 from golden_util.synth_cells (a 512 x 512 image tiled,
as tools/post_probe.py does).  Data versions 3 (dicts) and 4 (strings).  Also: the cell mapping alone (both routes share it), outline_cells alone and the
share of it spent building Python objects after the last copy, and the two kernels alone (HIP events).  The results of the two routes are compared
(equality) before anything is timed.  Writes <out> (default profiles/cell_outline.json) and prints it.

    python tools/cell_outline_time.py [--rounds 3] [--small] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def disc_images(side=2048, pitch=32, radius=12):
    import numpy as np
    yy, xx = np.mgrid[0:pitch, 0:pitch]
    disc = (yy - pitch // 2) ** 2 + (xx - pitch // 2) ** 2 <= radius * radius
    m = np.tile(disc, (side // pitch, side // pitch))
    seg = np.zeros((side, side, 3), dtype=np.uint8)
    seg[m] = (230, 10, 20)
    marker = np.full((side, side, 3), 90, dtype=np.uint8)
    return seg, marker


def synth_images(side=8192):
    import numpy as np
    from golden_util import synth_cells
    _, seg, marker = synth_cells(512, 512, 300, 21)
    r = side // 512
    return tuple(np.ascontiguousarray(np.tile(a, (r, r, 1))) for a in (seg, marker))


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernels_alone(PP, cm, version, rounds):
    """HIP events around the two launches (the table, the offsets and the output buffer are in place before the first event)"""
    import numpy as np
    import torch
    from deepliif_amd import _lib as L
    from deepliif_amd import ops
    lib, p, mask = ops.impl().lib, ops._ptr, cm.mask
    H, W = cm.shape
    n, strings = len(cm.table), version in (4, 6)
    table_d = torch.from_numpy(cm.table).to(mask.device)
    counts_d = torch.empty((n, 8), dtype=torch.int32, device=mask.device)
    stream = ops._stream(mask)
    count_ms, emit_ms = [], []
    for _ in range(rounds + 1):
        a, b, c, d = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        a.record()
        L.check(lib.dl_pp_outline_count(p(mask), H, W, p(table_d), n, 0, 0, p(counts_d), stream), 'dl_pp_outline_count')
        b.record()
        counts = counts_d.cpu().numpy()
        offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts[:, 6 if strings else 5], out=offsets[1:])
        total = int(offsets[-1])
        out_d = torch.empty(total, dtype=torch.uint8, device=mask.device) if strings else torch.empty((total, 2), dtype=torch.int32, device=mask.device)
        offsets_d = torch.from_numpy(offsets).to(mask.device)
        c.record()
        L.check(lib.dl_pp_outline_emit(p(mask), H, W, p(table_d), p(counts_d), p(offsets_d), n, 0, 0, 1 if strings else 0, p(out_d), total, stream), 'dl_pp_outline_emit')
        d.record()
        torch.cuda.synchronize()
        count_ms.append(a.elapsed_time(b))
        emit_ms.append(c.elapsed_time(d))
    return statistics.median(count_ms[1:]), statistics.median(emit_ms[1:]), total


def measure(name, seg, marker, rounds):
    import torch
    from deepliif_amd import postprocessing as PP
    seg_d, marker_d = torch.from_numpy(seg).cuda(), torch.from_numpy(marker).cuda()
    rows = []
    for version in (3, 4):
        call = lambda route: PP.compute_cell_results(seg_d, marker_d, '40x', version=version, route=route)
        _, got = timed(lambda: call('gpu'))                          # warm-up of both routes, and the check that they agree
        _, want = timed(lambda: call('host'))
        assert got == want, f'{name} v{version}: the routes differ'
        host_s, gpu_s = [], []
        for _ in range(rounds):
            host_s.append(timed(lambda: call('host'))[0])
            gpu_s.append(timed(lambda: call('gpu'))[0])
        cm = PP.get_cells_info(seg_d, marker_d, '40x', PP.DEFAULT_NOISE_THRESH, PP.DEFAULT_SEG_THRESH, None)
        map_s = statistics.median(timed(lambda: PP.get_cells_info(seg_d, marker_d, '40x', PP.DEFAULT_NOISE_THRESH, PP.DEFAULT_SEG_THRESH, None))[0]
                                  for _ in range(rounds))
        out_s, py_s = [], []
        for _ in range(rounds):
            t = {}
            out_s.append(timed(lambda: PP.outline_cells(cm.mask, cm.table, version, timings=t))[0])
            py_s.append(t['python'])
        count_ms, emit_ms, items = kernels_alone(PP, cm, version, rounds)
        h, g, o, py = (statistics.median(v) for v in (host_s, gpu_s, out_s, py_s))
        n = len(cm.cells)
        row = {'mask': name, 'size': list(seg.shape[:2]), 'version': version, 'cells': n, 'items': items, 'rounds': rounds,
               'route_host_s': h, 'route_gpu_s': g, 'host_over_gpu': h / g, 'cell_mapping_s': map_s,
               'host_outlines_s': h - map_s, 'host_outlines_us_per_cell': (h - map_s) / max(n, 1) * 1e6,
               'gpu_outlines_s': o, 'gpu_outlines_us_per_cell': o / max(n, 1) * 1e6, 'outlines_host_over_gpu': (h - map_s) / o,
               'python_objects_s': py, 'python_share_of_gpu_route': py / g, 'python_share_of_gpu_outlines': py / o,
               'count_kernel_ms': count_ms, 'emit_kernel_ms': emit_ms, 'kernels_ns_per_cell': (count_ms + emit_ms) * 1e6 / max(n, 1),
               'all_host_s': host_s, 'all_gpu_s': gpu_s}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='the 2048 x 2048 mask only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cell_outline.json'))
    a = ap.parse_args()
    import torch
    rows = measure('discs_2048', *disc_images(), a.rounds)
    if not a.small:
        rows += measure('synth_8192', *synth_images(), a.rounds)
    res = {'tool': 'tools/cell_outline_time.py', 'device': torch.cuda.get_device_name(0), 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({'written': a.out, 'rows': len(rows)}))


if __name__ == '__main__':
    main()
