"""The grid of tests/test_wgrad_routing_host.py and the recorder of its fixture tests/golden/wgrad_routing.json -- TEST INFRASTRUCTURE ONLY.

A row is one weight gradient as engine.conv()'s backward hands it to ops.HipBackend.conv_wgrad: a layer of conv_routing_cases.LAYERS (the narrow head in its
wgrad_c4 and in its shift-stacked form), an N x H x W of the layer input, a storage / precision policy, split copies on neither, one or both operands and
the activation staged on x.  For every row the fixture holds

  * the library's answers: dl_wgrad_plan (return value, tiles, K steps, name), dl_conv_wgrad_deferrable and dl_wgrad_slab_floats at split-K 1, 3 and 512;
  * what HipBackend.conv_wgrad does with split-K automatic, 1 and 3, outside and inside a deferring pass, driven as tests/test_deferred_host.py drives it
    (tensors on `meta`; a proxy forwards the query exports to the real library and records the launching ones): the entry point it reaches (dl_conv_wgrad,
    dl_conv_wgrad_slabs, dl_conv_wgrad_multi, or the error), the split-K and the slab size it passes, and a CRC of the descriptor bytes of the six launches;
  * the answers of HipBackend.wgrad_takes_split and wgrad_c4_applies for the row's operands.

Names, return values, entry points and booleans are stored as an index into the list of distinct tuples, the numbers as zlib-packed columns.  SWITCH_GRID is a
thinner grid recorded once per documented runtime switch that steers the weight gradient.

The fixture is a snapshot of the routing AS IT WAS: it is recorded from a checkout of the commit BEFORE the change under test, with a library built there,

    python tests/wgrad_routing_cases.py --record <checkout of the parent commit>

and never from the tree this file lies in.  `--answers <checkout>` prints every answer of the thin grid as JSON lines, for comparing the dev builds (make dev)
of two commits: DEEPLIIF_AMD_LIB selects the library; the dev switches are read once per process, so one process per setting, with the setting in its environment."""
import base64
import ctypes as C
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TREE = os.path.abspath(sys.argv[2]) if __name__ == '__main__' and sys.argv[1:2] in (['--record'], ['--answers']) and len(sys.argv) == 3 else None
if _TREE:           # another checkout's package (and the library built there)
    assert sys.argv[1] != '--record' or not os.path.samefile(_TREE, ROOT), 'the fixture is recorded from the parent commit, never from the code under test'
    sys.path.insert(0, _TREE)
    import deepliif_amd  # noqa: E402,F401  (conv_routing_cases below then finds it loaded)
    assert os.path.samefile(os.path.dirname(os.path.dirname(deepliif_amd.__file__)), _TREE)
elif ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import conv_routing_cases as CR  # noqa: E402
from deepliif_amd import _lib as L  # noqa: E402
from deepliif_amd import ops  # noqa: E402
from deepliif_amd.geometry import cpad  # noqa: E402

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'wgrad_routing.json')
# pixel counts of P on either side of 32, 64 and 128 (the K steps and the `Ptot >= 32 / 64 * splitk` rules), a one-row image of 128 pixels, rows of 128 pixels
# from the w4 kernel's two-row minimum on, and 7x7 images with Hp % 4 != 0 / Wp % 64 != 0 next to whole 4 x 64 tiles
EDGE_SHAPES = [(8, 1, 1), (31, 1, 1), (32, 1, 1), (33, 1, 1), (1, 5, 7), (63, 1, 1), (1, 8, 8), (65, 1, 1), (127, 1, 1), (1, 8, 16), (2, 8, 9), (1, 1, 128),
               (1, 2, 128), (3, 3, 128), (1, 4, 64), (2, 8, 64), (1, 6, 64), (1, 4, 68), (1, 8, 192)]
SHAPES = CR.SHAPES + EDGE_SHAPES
POLICIES = [('bf16', torch.bfloat16, L.PREC_BF16), ('strict', torch.float32, L.PREC_BF16X3), ('fp32+bf16', torch.float32, L.PREC_BF16)]
SPLITS = ('-', 'P', 'Q', 'PQ')          # (on a policy or behind an activation that cannot read a split copy the row records the library's refusal)
ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU)
PLAN_SPLITKS = (1, 3, 512)
CALLS = [(sk, deferring) for deferring in (False, True) for sk in (None, 1, 3)]

SWITCH_SETTINGS = ['DL_NO_X3_GLDS=1', 'DL_NO_WGRAD_C4=1', 'DL_NO_C4_X3=1']
# the import-time copies of the same variables in the ops module of a commit that still had them: set together with the library's table
_OPS_COPIES = {'DL_NO_X3_GLDS': '_NO_X3_GLDS', 'DL_NO_WGRAD_C4': '_NO_WGRAD_C4', 'DL_NO_C4_X3': '_NO_C4_X3'}
SWITCH_LAYERS = ('resnet.stem[zero]', 'resnet.head.narrow[zero]', 'resnet.block[zero]', 'resnet.block[replicate]', 'resnet.down2', 'resnet.up1', 'unet.down64-128',
                 'patchgan.c1[6]')
SWITCH_SHAPES = [(1, 5, 7), (1, 8, 16), (1, 4, 64), (2, 8, 64), (3, 3, 128), (1, 64, 64), (4, 128, 128)]


def _forms(layers):
    """(label, spec, form): the narrow head is taken by wgrad_c4 or by shift_stack + stack_kw under zero padding, and like the plain head otherwise"""
    for label, spec, narrow in layers:
        if not narrow:
            yield label, spec, 'plain'
        elif spec.pad_mode == L.PAD_ZERO:
            yield label + '/c4', spec, 'c4'
            yield label + '/stack', spec, 'stack'


_META = {}


def _meta(shape, dtype):
    t = _META.get((shape, dtype))
    if t is None:
        t = _META[(shape, dtype)] = torch.empty(shape, dtype=dtype, device='meta')
    return t


def operands(spec, form, n, h, w, dtype, act):
    """(P, Q, grad, args, kwargs) of conv_wgrad(P, Q, grad, *args, prec, accumulate, **kwargs) as engine.conv()'s backward passes them (wgrad_ref.descriptor_of)"""
    oh, ow = spec.out_hw(h, w)
    if min(oh, ow) < 1:
        return None
    x, dy = (n, h, w, cpad(spec.cin)), (n, oh, ow, cpad(spec.cout))
    if form in ('c4', 'stack'):
        P = dy if form == 'c4' else (n, oh, ow, cpad(spec.cout * spec.k))
        kw = {'stack_kw': spec.k} if form == 'stack' else {}
        return _meta(P, dtype), _meta(x, dtype), _meta((spec.cout, spec.cin, spec.k, spec.k), torch.float32), (spec.k, 1, spec.pad, L.PAD_ZERO, L.ACT_NONE, act), kw
    if spec.kind == 'conv':
        return _meta(dy, dtype), _meta(x, dtype), _meta((spec.cout, spec.cin, spec.k, spec.k), torch.float32), (spec.k, spec.stride, spec.pad, spec.pad_mode,
                                                                                                                   L.ACT_NONE, act), {}
    return _meta(x, dtype), _meta(dy, dtype), _meta((spec.cin, spec.cout, spec.k, spec.k), torch.float32), (spec.k, spec.stride, spec.pad, L.PAD_ZERO, act,
                                                                                                              L.ACT_NONE), {}


def _rows(layers, shapes):
    """yields (key, (P, Q, grad, args, prec, kwargs)); key = (layer, (n, h, w), policy, split, act)"""
    for label, spec, form in _forms(layers):
        for n, h, w in shapes:
            for pol, dtype, prec in POLICIES:
                for act in ACTS:
                    ops_ = operands(spec, form, n, h, w, dtype, act)
                    if ops_ is None:
                        continue
                    P, Q, grad, args, kw = ops_
                    for split in SPLITS:
                        if split != '-' and form != 'plain':
                            continue            # (the engine hands split copies to the plain convolutions only)
                        skw = dict(kw, p_split='P' in split, q_split='Q' in split) if split != '-' else kw
                        yield (label, (n, h, w), pol, split, act), (P, Q, grad, args, prec, skw)


def main_rows():
    return _rows(CR.LAYERS, SHAPES)


def switch_rows():
    return _rows([l for l in CR.LAYERS if l[0] in SWITCH_LAYERS], SWITCH_SHAPES)


def describe(key):
    label, (n, h, w), pol, split, act = key
    return f'{label} {n}x{h}x{w} {pol} split={split} act={act}'


# ---- the recording proxy and the backend around it
QUERIES = ('dl_wgrad_plan', 'dl_conv_wgrad_deferrable', 'dl_wgrad_route_info')
MAX_QUERIES = 3          # library calls of one conv_wgrad in front of its launch: the route (or plan), the slab size, and inside a pass whether it can be deferred


class Proxy:
    """the query exports go to the real library (and are counted); the launching ones are recorded: (entry point, descriptor bytes)"""

    def __init__(self, lib):
        self.lib, self.launches, self.asked, self.queries = lib, [], [], 0
        self.dl_last_error = lib.dl_last_error
        if hasattr(lib, 'wgrad_route_memo'):
            self.wgrad_route_memo = lib.wgrad_route_memo

    def __getattr__(self, name):
        if name not in QUERIES:
            raise AttributeError(name)
        fn = getattr(self.lib, name)

        def counted(*a):
            self.queries += 1
            return fn(*a)
        return counted

    def dl_wgrad_slab_floats(self, d):
        self.queries += 1
        self.asked.append(int(self.lib.dl_wgrad_slab_floats(d)))
        return self.asked[-1]

    def dl_conv_wgrad(self, d, P, Q, grad, slab, stream):
        self.launches.append(('dl_conv_wgrad', bytes(d._obj)))
        return 0

    def dl_conv_wgrad_slabs(self, d, P, Q, grad, slab, entry, stream):
        self.launches.append(('dl_conv_wgrad_slabs', bytes(d._obj)))
        entry._obj.nblocks = 1
        return 0

    def dl_conv_wgrad_multi(self, d, n, P, Q, grad, slab, entries, stream):
        self.launches.append(('dl_conv_wgrad_multi', bytes(d._obj)))
        for l in range(n):
            entries[l].nblocks = 1
        return 0

    def dl_wgrad_reduce_batch(self, table, count, total, stream):
        return 0


class backend:
    """with backend(lib) as be: a HipBackend on the proxy, off the GPU (as the fixture of tests/test_deferred_host.py builds it)"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.saved = {n: getattr(ops, n) for n in ('WS', '_need_cuda', '_stream', '_WGRAD_DEFER', '_WGRAD_BATCH')}
        ops.WS, ops._need_cuda, ops._stream, ops._WGRAD_DEFER, ops._WGRAD_BATCH = ops.Workspace(), (lambda *ts: None), (lambda t=None: None), True, True
        be = ops.HipBackend.__new__(ops.HipBackend)
        be.lib = Proxy(self.lib)
        return be

    def __exit__(self, *exc):
        for n, v in self.saved.items():
            setattr(ops, n, v)


def _call(be, row, splitk, deferring):
    """(entry point | 'error', split-K passed, slab floats asked for, descriptor bytes) of one conv_wgrad"""
    P, Q, grad, args, prec, kw = row
    px = be.lib
    px.launches, px.asked, px.queries = [], [], 0
    try:
        if deferring:
            be.wgrad_defer_begin()
        try:
            be.conv_wgrad(P, Q, grad, *args, prec, True, splitk=splitk, **kw)
        finally:
            if deferring:
                be.wgrad_defer_end()            # (launches what was queued)
    except L.HipLibraryError:
        be.wgrad_abandon()
        assert not px.launches
        return 'error', 0, 0, b''
    assert px.queries <= MAX_QUERIES, (px.queries, splitk, deferring)
    (entry, raw), = px.launches
    return entry, L.WgradDesc.from_buffer_copy(raw).splitk, px.asked[-1], raw


def _library_answers(lib, row):
    P, Q, grad, args, prec, kw = row
    k, step, pad, pad_mode, p_act, q_act = args
    d = L.WgradDesc()
    d.N, d.Hp, d.Wp, d.CAp = P.shape
    _, d.Hq, d.Wq, d.CBp = Q.shape
    d.p_pstride, d.q_pstride = d.CAp, d.CBp
    d.KH = d.KW = k
    d.step, d.pad, d.pad_mode, d.pad_w = step, pad, pad_mode, -1
    d.CA, d.CB = grad.shape[0], grad.shape[1]
    if kw.get('stack_kw'):
        d.KW, d.pad_w, d.stack_kw, d.CA = 1, 0, kw['stack_kw'], grad.shape[0] * kw['stack_kw']
    d.dtype, d.prec, d.accumulate = ops.dl_dtype(P), prec, 1
    d.p_act, d.q_act = p_act, q_act
    d.p_split, d.q_split = int(kw.get('p_split', False)), int(kw.get('q_split', False))
    cat, num = [], []
    t, ks, nm = L.i32(), L.i32(), C.c_char_p()
    for sk in PLAN_SPLITKS:
        d.splitk = sk
        rc = int(lib.dl_wgrad_plan(C.byref(d), C.byref(t), C.byref(ks), C.byref(nm)))
        cat += [rc, (nm.value or b'').decode(), int(lib.dl_conv_wgrad_deferrable(C.byref(d)))]
        num += [t.value, ks.value, int(lib.dl_wgrad_slab_floats(C.byref(d)))]
        if hasattr(lib, 'dl_wgrad_route_info'):          # the one-call form reports the same decision
            r = L.WgradRoute()
            rc2 = int(lib.dl_wgrad_route_info(C.byref(d), C.byref(r)))
            assert (rc2 < 0) == (rc < 0) and (r.name.decode(), r.tiles, r.ksteps, r.deferrable) == (cat[-2], t.value, ks.value, cat[-1]) and \
                (rc < 0 or r.batched == rc), (bytes(d).hex(), rc, rc2)
    return cat, num


def answers(lib, rows):
    """[(key, categorical tuple, numbers, crc of the launched descriptors)] for every row"""
    out = []
    with backend(lib) as be:
        for key, row in rows:
            cat, num = _library_answers(lib, row)
            crc = 0
            for sk, deferring in CALLS:
                entry, splitk, nslab, raw = _call(be, row, sk, deferring)
                cat.append(entry)
                num += [splitk, nslab]
                crc = zlib.crc32(raw, crc)
            P, Q, grad, args, prec, kw = row
            k, step, pad, pad_mode, p_act, q_act = args
            cat.append(bool(be.wgrad_takes_split(P, Q, grad, k, pad_mode, prec, kw.get('stack_kw', 0))))
            cat.append(bool(be.wgrad_c4_applies(P, Q, grad, k, step, pad, pad_mode, p_act, q_act, prec, kw.get('stack_kw', 0))))
            out.append((key, tuple(cat), tuple(num), crc))
    return out


N_CAT = 3 * len(PLAN_SPLITKS) + len(CALLS) + 2
COL_ENTRY0, COL_TAKES_SPLIT, COL_C4 = 3 * len(PLAN_SPLITKS), N_CAT - 2, N_CAT - 1          # (the first conv_wgrad call)
N_NUM = 3 * len(PLAN_SPLITKS) + 2 * len(CALLS)
COL_TILES = 0


class switch_setting(CR.switch_setting):
    """with switch_setting(lib, 'DL_NO_C4_X3=1'): the library's table AND (in a commit whose ops module keeps its own copy) that copy"""

    def __enter__(self):
        super().__enter__()
        self.copy = _OPS_COPIES[self.name] if hasattr(ops, _OPS_COPIES[self.name]) else None
        if self.copy:
            self.copy_saved = getattr(ops, self.copy)
            setattr(ops, self.copy, True)

    def __exit__(self, *exc):
        if self.copy:
            setattr(ops, self.copy, self.copy_saved)
        super().__exit__(*exc)


# ---- the fixture
def _pack(values, size):
    return base64.b64encode(zlib.compress(b''.join(int(v).to_bytes(size, 'little') for v in values), 9)).decode()


def _unpack(s, size):
    raw = zlib.decompress(base64.b64decode(s))
    return [int.from_bytes(raw[i:i + size], 'little') for i in range(0, len(raw), size)]


def encode(tuples, got):
    pos = {t: i for i, t in enumerate(tuples)}
    idx = []
    for _, cat, _, _ in got:
        if cat not in pos:
            pos[cat] = len(tuples)
            tuples.append(cat)
        idx.append(pos[cat])
    return {'cat': _pack(idx, 2), 'num': [_pack([g[2][c] for g in got], 8) for c in range(N_NUM)], 'crc': _pack([g[3] for g in got], 4)}


def decode(fx, enc):
    """[(categorical tuple, numbers, crc)] of one recorded grid"""
    cols = [_unpack(c, 8) for c in enc['num']]
    return [(fx['tuples'][i], tuple(col[r] for col in cols), crc) for r, (i, crc) in enumerate(zip(_unpack(enc['cat'], 2), _unpack(enc['crc'], 4)))]


def load_fixture():
    with open(FIXTURE) as f:
        fx = json.load(f)
    fx['tuples'] = [tuple(t) for t in fx['tuples']]
    return fx


def record(lib):
    for s in SWITCH_SETTINGS:
        assert s.split('=')[0] not in os.environ, f'{s.split("=")[0]} is set: the main grid is recorded with every switch at its default'
    tuples = []
    main = answers(lib, main_rows())
    fx = {'tuples': tuples, 'library_version': lib.dl_version(), 'main': encode(tuples, main), 'switches': {}}
    default = [g[1:] for g in answers(lib, switch_rows())]
    for s in SWITCH_SETTINGS:
        with switch_setting(lib, s):
            got = answers(lib, switch_rows())
        assert [g[1:] for g in got] != default, f'{s} moves no row of the thin grid'
        fx['switches'][s] = encode(tuples, got)
    with open(FIXTURE, 'w') as f:
        json.dump(fx, f, indent=0, sort_keys=True)
        f.write('\n')
    entries = {c[COL_ENTRY0 + i] for _, c, _, _ in main for i in range(len(CALLS))}
    print(f'{FIXTURE}: {len(main)} rows, {len(tuples)} distinct tuples, {os.path.getsize(FIXTURE)} bytes; names {sorted({c[3 * i + 1] for _, c, _, _ in main for i in range(len(PLAN_SPLITKS))})}; '
          f'entry points {sorted(entries)}; takes_split {sorted({c[COL_TAKES_SPLIT] for _, c, _, _ in main})}')


if __name__ == '__main__':
    if sys.argv[1:2] == ['--record'] and _TREE:
        record(L.load())
    elif sys.argv[1:2] == ['--answers'] and _TREE:
        for key, cat, num, crc in answers(L.load(), switch_rows()):
            print(json.dumps([describe(key), cat, num, crc]))
    else:
        sys.exit(__doc__)
