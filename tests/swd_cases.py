"""Inputs shared by tests/test_swd_ref_host.py, tests/test_gpu_swd.py and tests/golden/make_golden_swd.py: seeded image SETS for the sliced
Wasserstein distance.  The images are generated here from np.random.RandomState with integer and exactly rounded float64 operations only (no
library filter), so every machine gets the same bytes; the fixture (tests/golden/swd_cases.npz) stores a checksum of them, not the images.

Each pair is a noise or a smooth image and a blurred, noised version of it.  No channel is near-constant at any pyramid level: the
normalisation divides by std + 1e-8, which amplifies by 1e8 at std = 0 (in the reference too)."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'swd_cases.npz')

# name -> N, H, W, kind, seed of the images, n_repeat_projection, seed of the draws
CASES = {
    '3x48x80': dict(n=3, h=48, w=80, kind='smooth', seed=11, n_repeat_projection=8, draw_seed=101),     # levels 48x80, 24x40, 12x20 (84 positions < 128): R = 384, 384, 252
    '2x64x64': dict(n=2, h=64, w=64, kind='noise', seed=12, n_repeat_projection=4, draw_seed=102),
    '1x16x16': dict(n=1, h=16, w=16, kind='noise', seed=13, n_repeat_projection=8, draw_seed=103),      # n_pyramids = 0: one level, 100 descriptors
    '1x32x32': dict(n=1, h=32, w=32, kind='smooth', seed=14, n_repeat_projection=4, draw_seed=104),
    '1x96x160': dict(n=1, h=96, w=160, kind='smooth', seed=15, n_repeat_projection=2, draw_seed=105),   # several pyramid tiles each way, with remainders
    '65x32x32': dict(n=65, h=32, w=32, kind='mixed', seed=16, n_repeat_projection=2, draw_seed=106),    # R = 8320 at level 0
}
NAMES = list(CASES)
N_DESCRIPTORS, PROJ_PER_REPEAT = 128, 4


def blur(x, times=1):
    """[1 2 1] / 4 along rows and columns of an H x W x 3 float64 image, edge-replicated, `times` times; plain slice additions"""
    for _ in range(times):
        p = np.pad(x, ((1, 1), (0, 0), (0, 0)), mode='edge')
        x = (p[:-2] + 2.0 * p[1:-1] + p[2:]) / 4.0
        p = np.pad(x, ((0, 0), (1, 1), (0, 0)), mode='edge')
        x = (p[:, :-2] + 2.0 * p[:, 1:-1] + p[:, 2:]) / 4.0
    return x


def image_pair(h, w, kind, rng):
    if kind == 'noise':
        a = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        amp = 20
    else:
        f = blur(rng.randint(0, 256, size=(h, w, 3)).astype(np.float64), times=3)
        lo, hi = f.min(axis=(0, 1), keepdims=True), f.max(axis=(0, 1), keepdims=True)
        a = np.floor((f - lo) / (hi - lo) * 255.0).astype(np.uint8)
        amp = 8
    b = np.floor(blur(a.astype(np.float64))).astype(np.int64) + rng.randint(-amp, amp + 1, size=a.shape)
    return a, np.clip(b, 0, 255).astype(np.uint8)


def image_sets(name=None, n=None, h=None, w=None, kind=None, seed=None, **_):
    """-> (gt, pred), uint8 [N, H, W, 3] each; by case name or by explicit parameters"""
    if name is not None:
        return image_sets(**CASES[name])
    rng = np.random.RandomState(seed)
    pairs = [image_pair(h, w, ('noise', 'smooth')[i % 2] if kind == 'mixed' else kind, rng) for i in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def checksum(gt, pred):
    return hashlib.sha256(np.ascontiguousarray(gt).tobytes() + np.ascontiguousarray(pred).tobytes()).hexdigest()


def default_pyramids(h):
    return int(np.rint(np.log2(h // 16)))


def level_shapes(h, w, n_pyramids):
    shapes = [(h, w)]
    for _ in range(n_pyramids):
        shapes.append(((shapes[-1][0] - 1) // 2 + 1, (shapes[-1][1] - 1) // 2 + 1))
    return shapes
