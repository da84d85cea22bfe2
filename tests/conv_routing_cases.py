"""The descriptor grid of tests/test_conv_routing_host.py and the recorder of its fixture tests/golden/conv_routing.json -- TEST INFRASTRUCTURE ONLY.

A row is one dl_conv_desc: a layer of the Resnet-9 generator, the UNet or the PatchGAN, a direction (forward / data gradient), an N x H x W of the layer
input, a precision policy and the per-launch flags (output activation, input activation, bias, split-K).  For every row the fixture holds the four answers of
the host side of the dispatch -- dl_conv_kernel_name, dl_conv_stats_chunks, dl_conv_bnstats_chunks, dl_conv_add_supported -- as an index into the list of
distinct answer tuples.  SWITCH_GRID is a thinner grid that is recorded once per setting of the documented runtime switches that steer the routing.

The fixture is a snapshot of the dispatch AS IT WAS, so it is recorded from a library built at the commit BEFORE the change under test:

    DEEPLIIF_AMD_LIB=<parent build>/libdeepliif_hip.so python tests/conv_routing_cases.py --record

and where a change means to alter the answers of one switch setting, that setting alone is recorded again from the new library; the rows that changed are
printed and belong in the description of the change:

    python tests/conv_routing_cases.py --record-switch DL_CONV_W4X3=1
"""
import base64
import ctypes as C
import itertools
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from deepliif_amd import _lib as L  # noqa: E402
from deepliif_amd.geometry import ConvSpec, cpad, fill_conv_desc  # noqa: E402

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'conv_routing.json')
PADS = (('zero', L.PAD_ZERO), ('reflect', L.PAD_REFLECT), ('replicate', L.PAD_REPLICATE))


def _layers():
    """(label, ConvSpec, narrow): every convolution shape of the three network families (networks.py), ngf = ndf = 64"""
    out = []
    for pn, pm in PADS:
        out.append((f'resnet.stem[{pn}]', ConvSpec('conv', 3, 64, 7, 1, 3, pm), False))
    out.append(('resnet.down1', ConvSpec('conv', 64, 128, 3, 2, 1), False))
    out.append(('resnet.down2', ConvSpec('conv', 128, 256, 3, 2, 1), False))
    for pn, pm in PADS:
        out.append((f'resnet.block[{pn}]', ConvSpec('conv', 256, 256, 3, 1, 1, pm), False))
    out.append(('resnet.up1', ConvSpec('convT', 256, 128, 3, 2, 1, out_pad=1), False))
    out.append(('resnet.up2', ConvSpec('convT', 128, 64, 3, 2, 1, out_pad=1), False))
    for pn, pm in PADS:
        out.append((f'resnet.head[{pn}]', ConvSpec('conv', 64, 3, 7, 1, 3, pm), False))
        out.append((f'resnet.head.narrow[{pn}]', ConvSpec('conv', 64, 3, 7, 1, 3, pm), True))      # kernel columns folded into the rows, raw accumulators out
    for cin, cout in ((3, 64), (64, 128), (128, 256), (256, 512), (512, 512), (512, 1024)):
        out.append((f'unet.down{cin}-{cout}', ConvSpec('conv', cin, cout, 4, 2, 1), False))
    for cin, cout in ((512, 512), (1024, 512), (1024, 256), (512, 128), (256, 64), (128, 3)):
        out.append((f'unet.up{cin}-{cout}', ConvSpec('convT', cin, cout, 4, 2, 1), False))
    for cin in (6, 9, 12):
        out.append((f'patchgan.c1[{cin}]', ConvSpec('conv', cin, 64, 4, 2, 1), False))
    out.append(('patchgan.c2', ConvSpec('conv', 64, 128, 4, 2, 1), False))
    out.append(('patchgan.c3', ConvSpec('conv', 128, 256, 4, 2, 1), False))
    out.append(('patchgan.c4', ConvSpec('conv', 256, 512, 4, 2, 1), False))
    out.append(('patchgan.c5', ConvSpec('conv', 512, 512, 4, 1, 1), False))
    out.append(('patchgan.pred', ConvSpec('conv', 512, 1, 4, 1, 1), False))
    return out


LAYERS = _layers()
# N x H x W of the LAYER INPUT: from one small tile to the benched discriminator batch; 2 x 31 x 31 (the PatchGAN's last feature map), 4 x 112 x 128 (exactly
# 224 tiles of 256 pixels: the big-tile rule's edge), rows of 128 pixels at several tile counts, one odd height
SHAPES = [(1, 16, 16), (2, 31, 31), (1, 16, 128), (1, 64, 64), (3, 65, 128), (2, 112, 128), (4, 112, 128), (1, 128, 128), (4, 128, 128), (1, 256, 256),
          (2, 256, 256), (1, 512, 512), (16, 512, 512)]
# label, storage dtype, product precision, in_split
POLICIES = [('bf16', L.DL_BF16, L.PREC_BF16, 0), ('strict', L.DL_F32, L.PREC_BF16X3, 0), ('strict+split', L.DL_F32, L.PREC_BF16X3, 1),
            ('fp32+bf16', L.DL_F32, L.PREC_BF16, 0)]
ACTS = (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU, L.ACT_TANH)
IN_ACTS = (L.ACT_NONE, L.ACT_RELU)
DIRECTIONS = ('fwd', 'dgrad')

# the documented runtime switches that steer the routing (include/deepliif_hip.h), each recorded over SWITCH_GRID
SWITCH_SETTINGS = ['DL_CONV_S2F=0', 'DL_CONV_S2F=2', 'DL_CONV_S2FX3=0', 'DL_CONV_S2D=0', 'DL_CONV_DOT=0', 'DL_CONV_W4X3=1', 'DL_NO_X3_GLDS=1', 'DL_NO_C4_X3=1']
SWITCH_LAYERS = ('resnet.block[zero]', 'resnet.block[reflect]', 'resnet.block[replicate]', 'resnet.down1', 'resnet.up1', 'resnet.up2', 'resnet.stem[zero]',
                 'resnet.stem[reflect]', 'patchgan.c1[6]', 'patchgan.pred')
# two shapes on either side of the 224-tile rule of the ResnetBlock conv (8 / 112 and 224 / 256 tiles), one whose rows reach the strip kernels of c1 / down1
SWITCH_SHAPES = [(1, 16, 128), (2, 112, 128), (4, 112, 128), (4, 128, 128), (1, 64, 512)]


def _geometry(spec, narrow, direction, n, h, w):
    """(plan, hi, wi, ci_pad, ho, wo, co_pad, hq, wq) of one launch for a layer input of n x h x w, as engine.conv / its backward lay it out"""
    oh, ow = spec.out_hw(h, w)
    if direction == 'fwd':
        if narrow:
            plan = spec.narrow_forward_plan()
            return plan, h, w, cpad(spec.cin), oh, ow, cpad(plan.rows_real), oh, ow
        hq, wq = (oh, ow) if spec.kind == 'conv' else (h, w)
        return spec.forward_plan(), h, w, cpad(spec.cin), oh, ow, cpad(spec.cout), hq, wq
    plan = spec.dgrad_plan()
    if spec.kind == 'conv' and spec.pad_mode != L.PAD_ZERO:          # the gradient with respect to the explicitly padded input (a fold follows)
        hp, wp = h + 2 * spec.pad, w + 2 * spec.pad
        return plan, oh, ow, cpad(spec.cout), hp, wp, cpad(spec.cin), hp, wp
    hq, wq = ((h + 1) // 2, (w + 1) // 2) if (spec.kind == 'conv' and spec.stride == 2) else (h, w)
    return plan, oh, ow, cpad(spec.cout), h, w, cpad(spec.cin), hq, wq


def _rows(layers, shapes, acts, in_acts, splitks):
    """yields (key, descriptor); the descriptor object is reused between rows: read it before the next one is drawn.
    key = (layer, direction, (n, h, w), policy, act, in_act, bias, splitk)"""
    for label, spec, narrow in layers:
        for direction in DIRECTIONS:
            if narrow and direction == 'dgrad':
                continue                # (the narrow form exists for the forward only)
            for n, h, w in shapes:
                plan, hi, wi, cip, ho, wo, cop, hq, wq = _geometry(spec, narrow, direction, n, h, w)
                if min(hi, wi, ho, wo, hq, wq) < 1:
                    continue
                for pol, dtype, prec, in_split in POLICIES:
                    d = fill_conv_desc(plan, n, hi, wi, cip, ho, wo, cop, cop, hq, wq, dtype, prec, L.ACT_NONE, L.ACT_NONE, 0, 1, 1 if narrow else 0)
                    d.in_split = in_split
                    if narrow:          # one launch form: raw accumulators, no bias, no activation, no split-K
                        yield (label, direction, (n, h, w), pol, L.ACT_NONE, L.ACT_NONE, False, 1), d
                        continue
                    for act, in_act, bias, splitk in itertools.product(acts, in_acts, (True, False), splitks):
                        if in_split and in_act != L.ACT_NONE:
                            continue    # (dl_conv_forward refuses a split copy behind an input activation)
                        d.act, d.in_act, d.bias_n, d.splitk = act, in_act, (plan.rows_real if bias else 0), splitk
                        yield (label, direction, (n, h, w), pol, act, in_act, bias, splitk), d


def main_rows():
    return _rows(LAYERS, SHAPES, ACTS, IN_ACTS, (1, 4))


def switch_rows():
    return _rows([l for l in LAYERS if l[0] in SWITCH_LAYERS], SWITCH_SHAPES, (L.ACT_NONE, L.ACT_RELU), (L.ACT_NONE,), (1,))


def describe(key):
    label, direction, (n, h, w), pol, act, in_act, bias, splitk = key
    return f'{label} {direction} {n}x{h}x{w} {pol} act={act} in_act={in_act} bias={"on" if bias else "off"} splitk={splitk}'


def answers(lib, rows):
    """[(key, (name, stats chunks, bnstats chunks, add_supported))] for every row"""
    out = []
    for key, d in rows:
        p = C.byref(d)
        out.append((key, (lib.dl_conv_kernel_name(p).decode(), lib.dl_conv_stats_chunks(p), lib.dl_conv_bnstats_chunks(p), lib.dl_conv_add_supported(p))))
    return out


class switch_setting:
    """with switch_setting(lib, 'DL_CONV_S2F=0'): the library sees that variable (dl_switches_reload), and forgets it again afterwards"""

    def __init__(self, lib, setting):
        self.lib, (self.name, self.value) = lib, setting.split('=')

    def __enter__(self):
        self.saved = os.environ.get(self.name)
        os.environ[self.name] = self.value
        self.lib.dl_switches_reload()

    def __exit__(self, *exc):
        if self.saved is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.saved
        self.lib.dl_switches_reload()


# ---- the fixture: the distinct answer tuples once, one 16-bit index per row (zlib + base64: 100 000 rows stay far below the size limit of a committed file)
def encode(idx):
    return base64.b64encode(zlib.compress(b''.join(i.to_bytes(2, 'little') for i in idx), 9)).decode()


def decode(s):
    raw = zlib.decompress(base64.b64decode(s))
    return [int.from_bytes(raw[i:i + 2], 'little') for i in range(0, len(raw), 2)]


def load_fixture():
    with open(FIXTURE) as f:
        fx = json.load(f)
    fx['tuples'] = [tuple(t) for t in fx['tuples']]
    return fx


def _save(fx):
    with open(FIXTURE, 'w') as f:
        json.dump(fx, f, indent=0, sort_keys=True)
        f.write('\n')


def _index(tuples, got):
    pos = {t: i for i, t in enumerate(tuples)}
    idx = []
    for _, t in got:
        if t not in pos:
            pos[t] = len(tuples)
            tuples.append(t)
        idx.append(pos[t])
    return idx


def record(lib):
    for s in SWITCH_SETTINGS:
        assert s.split('=')[0] not in os.environ, f'{s.split("=")[0]} is set: the main grid is recorded with every switch at its default'
    tuples = []
    fx = {'tuples': tuples, 'library_version': lib.dl_version(), 'main': encode(_index(tuples, answers(lib, main_rows()))), 'switches': {}}
    for s in SWITCH_SETTINGS:
        with switch_setting(lib, s):
            fx['switches'][s] = encode(_index(tuples, answers(lib, switch_rows())))
    _save(fx)
    print(f'{FIXTURE}: {len(decode(fx["main"]))} rows, {len(tuples)} distinct answers, {os.path.getsize(FIXTURE)} bytes')


def record_switch(lib, setting):
    assert setting in SWITCH_SETTINGS, setting
    fx = load_fixture()
    before = decode(fx['switches'][setting])
    with switch_setting(lib, setting):
        got = answers(lib, switch_rows())
    after = _index(fx['tuples'], got)
    changed = [(k, fx['tuples'][b], t) for (k, t), b, a in zip(got, before, after) if a != b]
    fx['switches'][setting] = encode(after)
    _save(fx)
    for k, was, now in changed:
        print(f'{setting}: {describe(k)}: {was} -> {now}')
    print(f'{setting}: {len(changed)} of {len(after)} rows changed')


if __name__ == '__main__':
    if sys.argv[1:2] == ['--record']:
        record(L.load())
    elif sys.argv[1:2] == ['--record-switch'] and len(sys.argv) == 3:
        record_switch(L.load(), sys.argv[2])
    else:
        sys.exit(__doc__)
