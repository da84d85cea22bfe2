"""Inputs shared by tests/test_stat_ref_host.py and tests/test_gpu_stat.py: the reference-generated mask pairs (tests/golden/stat_cases.npz)
and seeded image pairs for MSE / SSIM."""
import os

import numpy as np

from golden_util import load_npz

Z = load_npz(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stat_cases.npz'))
NAMES = [str(n) for n in Z['names']]


def planes(name):
    return Z[f'{name}/gt'], Z[f'{name}/pred']


def rgb_masks(name):
    """(gt, pred) RGB images of a case: channel 0 = the case's planes, channel 2 = their transposes' mirror images (different content),
    channel 1 = boundary-coloured noise that no metric reads"""
    g, p = planes(name)
    rng = np.random.RandomState(len(name))
    out = []
    for a in (g, p):
        img = np.zeros(a.shape + (3,), dtype=np.uint8)
        img[..., 0] = a
        img[..., 1] = rng.randint(0, 256, size=a.shape)
        img[..., 2] = a[::-1, ::-1]
        out.append(img)
    return out[0], out[1]


def noise_pair(h, w, seed, channels=3):
    rng = np.random.RandomState(seed)
    shape = (h, w, 3) if channels == 3 else (h, w)
    a = rng.randint(0, 256, size=shape).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.randint(-40, 41, size=shape), 0, 255).astype(np.uint8)
    return a, b


def near_flat_pair(h, w, seed, channels=3):
    """200 +- 1: variances of about 1e-5 against C2 = 9e-4 -- where single precision shows"""
    rng = np.random.RandomState(seed)
    shape = (h, w, 3) if channels == 3 else (h, w)
    return (200 + rng.randint(-1, 2, size=shape)).astype(np.uint8), (200 + rng.randint(-1, 2, size=shape)).astype(np.uint8)


def black_white_pair(h, w, channels=3):
    shape = (h, w, 3) if channels == 3 else (h, w)
    return np.zeros(shape, dtype=np.uint8), np.full(shape, 255, dtype=np.uint8)


def smooth_pair(h, w, seed):
    """a blurred blob image against a noisy copy: an SSIM far from both 0 and 1"""
    from scipy import ndimage
    rng = np.random.RandomState(seed)
    f = ndimage.gaussian_filter(rng.rand(h, w, 3), (3.0, 3.0, 0))
    f = (f - f.min()) / (f.max() - f.min())
    a = (f * 255).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.randint(-12, 13, size=a.shape), 0, 255).astype(np.uint8)
    return a, b
