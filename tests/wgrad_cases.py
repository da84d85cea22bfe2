"""The table of weight-gradient cases -- TEST INFRASTRUCTURE ONLY (tests/test_wgrad_ref_host.py, tests/test_gpu_wgrad.py).

One row per (kernel, edge).  A row is a LAYER (kind, channels, kernel size, stride, padding) at one input size; which tensor becomes the P and the Q
operand of the kernel, and with which step / padding / staged activation, is decided by wgrad_ref.descriptor_of() alone.  `kernel` is the name
dl_wgrad_plan gives for the row (read from a library built from this tree); the host test and the GPU test both assert it.

Fields
  kernel    expected dl_wgrad_plan name
  kind .. out_pad   the layer (geometry.ConvSpec)
  n, H, W   the layer INPUT (x) size; dy follows from the layer
  in_act    the activation staged on x (the engine's in_act); dy never carries one
  policies  'bf16' = bf16 storage + PREC_BF16, 'strict' = fp32 storage + PREC_BF16X3, 'f32b' = fp32 storage + PREC_BF16
  splitks   forced split-K values; None = the automatic choice of ops.HipBackend.conv_wgrad
  form      'plain' | 'stack' (narrow head: shift_stack + stack_kw) | 'c4' (narrow layer through the automatic path: wgrad_c4)
  p_pad8    the P operand is padded to a multiple of 8 channels only (CAp = 24, 136: no power of two), as a caller of the C ABI may do
  extras    further launches of the same problem: 'slice' (operands are channel slices of buffers twice as wide, the other half 7.0), 'multi' (three layers in
            one dl_conv_wgrad_multi), 'split' (split copies of P, of Q and of both), 'twice' (two launches give the same bits)
"""
from collections import namedtuple

from deepliif_amd import _lib as L

Row = namedtuple('Row', 'id kernel kind cin cout k stride pad pad_mode out_pad n H W in_act policies splitks form p_pad8 extras')

Z, RF = L.PAD_ZERO, L.PAD_REFLECT
NONE, RELU, LRELU = L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU
GEN, G128, G256, X128, X256 = 'wgrad_kernel', 'wgrad_glds_kernel<128>', 'wgrad_glds_kernel<256>', 'wgrad_glds_x3_kernel<128>', 'wgrad_glds_x3_kernel<256>'
ALL3 = ('bf16', 'strict', 'f32b')


def _row(id_, kernel, kind, cin, cout, k, stride, pad, n, H, W, policies, splitks=(1,), pad_mode=Z, out_pad=0, in_act=NONE, form='plain', p_pad8=False,
         extras=()):
    return Row(id_, kernel, kind, cin, cout, k, stride, pad, pad_mode, out_pad, n, H, W, in_act, tuple(policies), tuple(splitks), form, p_pad8, tuple(extras))


GENERIC = [
    # 3x3 s1, CA x CB 32 at 2 x 6 x 10: K = 120 pixels, J = 288 = two j tiles of 128 and a ragged third; split-K 3 gives ranges of 64, 56 and 0 pixels
    _row('gen-ca16', GEN, 'conv', 32, 16, 3, 1, 1, 2, 6, 10, ALL3, (1, 3, None), extras=('twice',)),
    _row('gen-ca24', GEN, 'conv', 32, 24, 3, 1, 1, 2, 6, 10, ALL3, (1, 3, None), p_pad8=True),
    _row('gen-ca64', GEN, 'conv', 32, 64, 3, 1, 1, 2, 6, 10, ALL3, (1, 3, None)),
    _row('gen-ca136', GEN, 'conv', 32, 136, 3, 1, 1, 2, 6, 10, ALL3, (1, 3, None), p_pad8=True),
    # the PatchGAN stem: 6 -> 64, 4x4 s2 p1, LeakyReLU staged on x; CBp 8 with CB 6 (two padded b columns)
    _row('gen-k4s2-6to64', GEN, 'conv', 6, 64, 4, 2, 1, 2, 16, 16, ALL3, (1,), in_act=LRELU),
    # the PatchGAN head: 512 -> 1, 4x4 s1 p1: CA 1 of CAp 8, P 7x7 != Q 8x8
    _row('gen-k4s1-512to1', GEN, 'conv', 512, 1, 4, 1, 1, 2, 8, 8, ALL3, (1,)),
    # UNet innermost up-convolution: P = x 8 x 1 x 1, ReLU staged on P, K = 8: less than one K step (and too few pixels for the strict direct-to-LDS kernel)
    _row('gen-convT-k4-1x1', GEN, 'convT', 256, 128, 4, 2, 1, 8, 1, 1, ALL3, (1,), in_act=RELU),
    _row('gen-convT-k3-op1', GEN, 'convT', 256, 128, 3, 2, 1, 2, 6, 5, ('bf16', 'f32b'), (1, 2), out_pad=1, in_act=RELU),
    _row('gen-reflect-stem', GEN, 'conv', 3, 64, 7, 1, 3, 1, 12, 10, ALL3, (1, 2), pad_mode=RF),
    _row('gen-reflect-128', GEN, 'conv', 128, 128, 3, 1, 1, 1, 6, 8, ('bf16', 'strict'), (1,), pad_mode=RF),
    # the narrow head through shift_stack: P has 3 * 7 = 21 -> 32 channels, vertical taps only; wgrad_reduce_body scatters the stacked rows
    _row('gen-head-stack', GEN, 'conv', 64, 3, 7, 1, 3, 1, 6, 10, ALL3, (1, 2), form='stack'),
    # the glds shape with a staged activation: back on the generic kernel under bf16
    _row('gen-256-relu', GEN, 'conv', 256, 256, 3, 1, 1, 2, 6, 10, ('bf16',), (1,), in_act=RELU),
]

GLDS = [
    _row('glds256-2x8x9', G256, 'conv', 256, 256, 3, 1, 1, 2, 8, 9, ('bf16',), (1, 2), extras=('slice', 'multi', 'twice')),      # split-K 2: 128 + 16 pixels
    _row('glds128-1x8x8', G128, 'conv', 32, 128, 3, 1, 1, 1, 8, 8, ('bf16',), (1,)),                                             # K = 64: exactly one step
    _row('glds128-2x8x9', G128, 'conv', 32, 128, 3, 1, 1, 2, 8, 9, ('bf16',), (1, 2), extras=('slice', 'multi', 'twice')),
    _row('glds128-s2-odd', G128, 'conv', 64, 128, 3, 2, 1, 2, 25, 19, ('bf16',), (1, 4)),                                        # P 2 x 13 x 10
    _row('glds256-k4s2', G256, 'conv', 256, 512, 4, 2, 1, 4, 8, 8, ('bf16',), (1,)),                                             # P 4 x 4 x 4
    _row('glds256-1x1', G256, 'conv', 256, 256, 1, 1, 0, 2, 6, 10, ('bf16',), (1,)),
]

X3 = [
    _row('x3-256-1x5x7', X256, 'conv', 256, 256, 3, 1, 1, 1, 5, 7, ('strict',), (1,)),                                           # K = 35: one step + 3 pixels
    _row('x3-256-2x6x10', X256, 'conv', 256, 256, 3, 1, 1, 2, 6, 10, ('strict',), (1, 2, 3), extras=('multi', 'twice')),
    # a stride-1 ConvTranspose2d puts x (128 channels, ReLU staged) on the P side
    _row('x3-128-1x5x7-prelu', X128, 'convT', 128, 64, 3, 1, 1, 1, 5, 7, ('strict',), (1,), in_act=RELU),
    _row('x3-128-2x6x10-qlrelu', X128, 'conv', 64, 128, 3, 1, 1, 2, 6, 10, ('strict',), (1, 2), in_act=LRELU),
    _row('x3-128-2x6x10', X128, 'conv', 64, 128, 3, 1, 1, 2, 6, 10, ('strict',), (1, 2), extras=('split', 'multi', 'twice', 'slice')),
    _row('x3-256-k4s2', X256, 'conv', 256, 512, 4, 2, 1, 2, 8, 8, ('strict',), (1,)),                                            # P 2 x 4 x 4: K = 32
    _row('x3-256-convT-1x1', X256, 'convT', 256, 128, 4, 2, 1, 32, 1, 1, ('strict',), (1,), in_act=RELU),                        # P 32 x 1 x 1: K = 32
]

C4 = [
    _row('c4-stem-1x4x64', 'wgrad_c4', 'conv', 3, 64, 7, 1, 3, 1, 4, 64, ('bf16', 'strict'), (None,), form='c4'),
    _row('c4-stem-2x8x64', 'wgrad_c4', 'conv', 3, 64, 7, 1, 3, 2, 8, 64, ('bf16', 'strict'), (None,), form='c4', extras=('twice',)),
    _row('c4-head-1x4x64', 'wgrad_c4', 'conv', 64, 3, 7, 1, 3, 1, 4, 64, ('bf16', 'strict'), (None,), form='c4'),
    _row('c4-head-2x8x64', 'wgrad_c4', 'conv', 64, 3, 7, 1, 3, 2, 8, 64, ('bf16', 'strict'), (None,), form='c4'),
]

W4 = [
    _row('w4-1x2x128', 'wgrad_w4_kernel', 'conv', 128, 128, 3, 1, 1, 1, 2, 128, ('bf16',), (1,)),
    _row('w4-3x3x128', 'wgrad_w4_kernel', 'conv', 128, 128, 3, 1, 1, 3, 3, 128, ('bf16',), (2,), extras=('twice',)),                # 9 rows over 2 ranges
]

ROWS = GENERIC + GLDS + X3 + C4 + W4
assert len({r.id for r in ROWS}) == len(ROWS)


def launches(row):
    """every (policy, splitk) the row runs with"""
    return [(pol, sk) for pol in row.policies for sk in row.splitks]


def launch_id(v):
    row, pol, sk = v
    return f'{row.id}/{pol}/sk{"auto" if sk is None else sk}'


ALL_LAUNCHES = [(r, pol, sk) for r in ROWS for pol, sk in launches(r)]
