"""Descriptor builders and the recorded routing table of the padding-mode tests (tests/test_replicate_host.py, tests/test_gpu_replicate.py) -- TEST
INFRASTRUCTURE ONLY.  Nothing here launches anything: dl_conv_kernel_name / dl_wgrad_plan answer on the host."""
import ctypes as C
import os

import torch

from deepliif_amd import _lib as L
from deepliif_amd.geometry import ConvSpec, cpad, fill_conv_desc

PAD = {'zero': L.PAD_ZERO, 'reflect': L.PAD_REFLECT, 'replicate': L.PAD_REPLICATE}
POLICY = {'bf16': (L.DL_BF16, L.PREC_BF16), 'strict': (L.DL_F32, L.PREC_BF16X3)}


def conv_desc(mode, n, h, w, cin, cout, k=3, policy='bf16', direction='fwd', act=L.ACT_NONE, bias_n=0, splitk=1, in_pstride=None):
    """dl_conv_desc of a stride-1 `k x k` layer with padding k // 2 of the given mode, forward or data gradient (for a non-zero mode the pad-0 plan
    over the padded extent, as engine.conv launches it)"""
    spec = ConvSpec('conv', cin, cout, k, 1, k // 2, PAD[mode])
    dtype, prec = POLICY[policy]
    if direction == 'fwd':
        plan = spec.forward_plan()
        return fill_conv_desc(plan, n, h, w, in_pstride or cpad(cin), h, w, cpad(cout), cpad(cout), h, w, dtype, prec, act, L.ACT_NONE, bias_n, splitk)
    plan = spec.dgrad_plan()
    p = 0 if mode == 'zero' else k // 2
    return fill_conv_desc(plan, n, h, w, in_pstride or cpad(cout), h + 2 * p, w + 2 * p, cpad(cin), cpad(cin), h + 2 * p, w + 2 * p, dtype, prec, act, L.ACT_NONE,
                          bias_n, splitk)


def wgrad_desc(mode, n, h, w, ca, cb, k=3, policy='bf16', splitk=1, p_pstride=None, q_pstride=None):
    """dl_wgrad_desc of the same layer: P = dL/dy (ca channels), Q = the layer input (cb channels)"""
    d = L.WgradDesc()
    d.N, d.Hp, d.Wp, d.CAp, d.p_pstride = n, h, w, cpad(ca), p_pstride or cpad(ca)
    d.Hq, d.Wq, d.CBp, d.q_pstride = h, w, cpad(cb), q_pstride or cpad(cb)
    d.KH = d.KW = k
    d.step, d.pad, d.pad_mode = 1, k // 2, PAD[mode]
    d.CA, d.CB = ca, cb
    d.dtype, d.prec = POLICY[policy]
    d.splitk, d.pad_w = splitk, -1
    return d


def conv_name(lib, d):
    return lib.dl_conv_kernel_name(C.byref(d)).decode()


def wgrad_plan(lib, d):
    """(return code, tiles, ksteps, kernel name)"""
    t, k, nm = L.i32(), L.i32(), C.c_char_p()
    rc = lib.dl_wgrad_plan(C.byref(d), C.byref(t), C.byref(k), C.byref(nm))
    return rc, t.value, k.value, (nm.value or b'').decode()


# ---- zero / reflect descriptors whose routing this feature must not move.  (kind, builder arguments) -> the kernel name the library gave BEFORE replicate
# padding existed (recorded from the parent commit's library with these very builders).
W4, W4W = 'conv_gemm_w4_kernel', 'wgrad_w4_kernel'
UNCHANGED = [
    (('conv', 'zero', 1, 2, 128, 64, 256), 'conv_gemm_glds_kernel<128,128,64>'),
    (('conv', 'zero', 224, 2, 128, 64, 256), W4),
    (('conv', 'zero', 8, 128, 128, 256, 256), W4),
    (('conv', 'zero', 8, 128, 128, 256, 256, 3, 'bf16', 'dgrad'), W4),
    (('conv', 'zero', 2, 4, 128, 128, 256), 'conv_gemm_glds_kernel<128,128,64>'),
    (('conv', 'zero', 38, 6, 128, 64, 512), W4),
    (('conv', 'zero', 1, 3, 128, 64, 256), 'conv_gemm_glds_kernel<128,128,64>'),
    (('conv', 'zero', 8, 64, 64, 256, 256), 'conv_gemm_glds_kernel<128,128,64>'),
    (('conv', 'zero', 16, 64, 64, 256, 256), 'conv_gemm_8ph_kernel'),
    (('conv', 'zero', 1, 8, 128, 32, 64), 'conv_gemm_glds_kernel<128,64,64>'),
    (('conv', 'zero', 2, 40, 24, 32, 32), 'conv_gemm_glds_kernel<128,64,64>'),
    (('conv', 'zero', 8, 128, 128, 256, 256, 3, 'strict'), 'conv_gemm_8ph_x3_kernel'),
    (('conv', 'zero', 2, 64, 64, 3, 64, 7), 'conv_c4_patch_kernel'),
    (('conv', 'zero', 2, 64, 64, 3, 64, 7, 'strict'), 'conv_c4_patch_x3_kernel'),
    (('conv', 'reflect', 8, 128, 128, 256, 256), 'conv_gemm_glds_kernel<256,256,64>'),
    (('conv', 'reflect', 8, 128, 128, 256, 256, 3, 'bf16', 'dgrad'), 'conv_gemm_8ph_kernel'),
    (('conv', 'reflect', 1, 2, 128, 64, 256), 'conv_gemm_glds_kernel<128,128,64>'),
    (('conv', 'reflect', 2, 40, 24, 32, 32), 'conv_gemm_glds_kernel<128,64,64>'),
    (('conv', 'reflect', 2, 64, 64, 3, 64, 7), 'conv_c4_patch_kernel'),
    (('conv', 'reflect', 2, 64, 64, 3, 64, 7, 'strict'), 'conv_c4_patch_x3_kernel'),
    (('conv', 'reflect', 8, 128, 128, 256, 256, 3, 'strict'), 'conv_gemm_glds_x3_kernel<128,128>'),
    (('conv', 'reflect', 1, 8, 128, 32, 64, 3, 'strict'), 'conv_gemm_glds_x3_kernel<128,64>'),
    (('wgrad', 'zero', 1, 2, 128, 128, 128), W4W),
    (('wgrad', 'zero', 8, 128, 128, 256, 256), W4W),
    (('wgrad', 'zero', 2, 3, 128, 256, 128), W4W),
    (('wgrad', 'zero', 8, 64, 64, 256, 256), 'wgrad_glds_kernel<256>'),
    (('wgrad', 'zero', 2, 40, 24, 32, 32), 'wgrad_kernel'),
    (('wgrad', 'zero', 8, 128, 128, 256, 256, 3, 'strict'), 'wgrad_glds_x3_kernel<256>'),
    (('wgrad', 'reflect', 8, 128, 128, 256, 256), 'wgrad_kernel'),
    (('wgrad', 'reflect', 1, 2, 128, 128, 128), 'wgrad_kernel'),
    (('wgrad', 'reflect', 2, 40, 24, 32, 32), 'wgrad_kernel'),
    (('wgrad', 'reflect', 8, 128, 128, 256, 256, 3, 'strict'), 'wgrad_kernel'),
]


def routed(lib, entry):
    kind, *args = entry
    return conv_name(lib, conv_desc(*args)) if kind == 'conv' else wgrad_plan(lib, wgrad_desc(*args))[3]


G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def build_replicate_dir(tmp_path, gain=0.02):
    """a DeepLIIF model directory (2 modalities + seg, ngf 8, BatchNorm) as the reference's training leaves it, with `padding: replicate` in train_opt.txt:
    G1 / G2 replicate-padded resnet_9blocks, GS0..2 unet_64 (define_G's default padding: no ResnetBlock in a U-Net)"""
    d = os.path.join(str(tmp_path), 'dl_m2_replicate')
    os.makedirs(d, exist_ok=True)
    txt = open(os.path.join(G, 'seam_train_opt_dl_m2.txt')).read()
    line = '                  padding: zero                          \n'
    assert txt.count(line) == 1
    open(os.path.join(d, 'train_opt.txt'), 'w').write(txt.replace(line, '                  padding: replicate                     \n'))
    from oracle import deepliif_oracle as O
    for j, name in enumerate(('G1', 'G2', 'GS0', 'GS1', 'GS2')):
        arch, pad = ('resnet_9blocks', 'replicate') if name in ('G1', 'G2') else ('unet_64', 'reflect')
        sd = O.random_state_dict(arch, 3, 3, 8, 'batch', pad, 4, gain, generator=torch.Generator().manual_seed(2200 + j))
        torch.save(sd, os.path.join(d, f'latest_net_{name}.pth'))
    return d
