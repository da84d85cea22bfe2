"""Tile geometry + GPU-side crop / is_empty / stitch for the inference path (BASELINE configs[4]).

The reference walks a PIL image one tile at a time (deepliif/util/__init__.py:129-331 InferenceTiler; the loop is
deepliif/models/__init__.py:496-498) and resolves overlapping pastes by paste ORDER.  Here the whole plan is integer geometry
computed up front, in closed form:

  * tile origins are separable: xs x ys, each axis = range(0, extent, centre) with the last origin clamped to extent - patch
    (:258-265); clamping makes the reference visit the last column / row more than once -- identical tiles, visited once here;
  * the nine conditional pastes of stitch() (:293-320) are one rectangle per tile: along an axis the tile at origin o owns
    [o + (0 if o == 0 else overlap), o + (patch if o == extent - patch else patch - overlap));
  * "later paste wins" along an axis means the tile with the LARGEST origin covering a pixel owns it, so tile i's effective
    interval ends where tile i+1's begins.  The effective rectangles are disjoint -> one order-independent GPU launch.

TilePlan holds that geometry (pinned against the reference's own iteration and paste sequence through the oracle,
tests/test_tiling_host.py).  RegionTiler runs it on a uint8 RGB image resident in HBM: dl_tile_gather_u8 (crop + transform()),
dl_tile_gray_stats_u8 (is_empty), dl_tile_paste_u8 (tensor2im + stitch) -- include/deepliif_hip.h.

tile_size != the networks' side (a slide scanned at 20x or 10x): the reference resizes every tile up and every result tile down with
PIL.  resample_table() restates Pillow's integer bicubic coefficients; dl_tile_gather_resample_u8 / dl_tile_paste_resample_u8 apply
them on the GPU, so RegionTiler(net_size=...) serves that case with the same geometry and the same bytes.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

EMPTY_VARIANCE_THRESHOLD = 9          # deepliif/models/__init__.py:392


def _axis_origins(extent: int, patch: int, centre: int) -> List[int]:
    """unique tile origins along one axis, increasing (range(0, extent, centre), clamped: util/__init__.py:258-265)"""
    out: List[int] = []
    for o in range(0, extent, centre):
        if o + patch > extent:
            o = extent - patch
        if not out or o != out[-1]:
            out.append(o)
    return out


def _axis_intervals(origins: Sequence[int], extent: int, patch: int, overlap: int) -> List[Tuple[int, int]]:
    """effective [lo, hi) each tile owns along the axis after "the later paste wins" (module docstring)"""
    lo = [o + (0 if o == 0 else overlap) for o in origins]
    hi = [o + (patch if o == extent - patch else patch - overlap) for o in origins]
    return [(lo[i], min(hi[i], lo[i + 1]) if i + 1 < len(origins) else hi[i]) for i in range(len(origins))]


class TilePlan:
    """Integer geometry of InferenceTiler(orig, tile_size, overlap_size, pad_size) for a width x height image."""

    def __init__(self, width: int, height: int, tile_size: int, overlap_size: int = 0, pad_size: int = 0):
        if tile_size <= 0:
            raise ValueError('InferenceTiler input tile_size must be positive and non-zero')
        if overlap_size < 0:
            raise ValueError('InferenceTiler input overlap_size must be positive or zero')
        if pad_size < 0:
            raise ValueError('InferenceTiler input pad_size must be positive or zero')
        self.orig_width, self.orig_height = int(width), int(height)
        self.tile_size, self.pad_size = int(tile_size), int(pad_size)
        self.patch_size = patch = tile_size - 2 * pad_size
        self.image_width, self.image_height = max(width, patch), max(height, patch)      # mirrored out to a patch (:196-211)
        self.overlap_width = 0 if patch >= self.image_width else overlap_size
        self.overlap_height = 0 if patch >= self.image_height else overlap_size
        self.center_width = patch - 2 * self.overlap_width
        self.center_height = patch - 2 * self.overlap_height
        if self.center_width <= 0 or self.center_height <= 0:
            raise ValueError('InferenceTiler combined overlap_size and pad_size are too large')
        self.xs = _axis_origins(self.image_width, patch, self.center_width)
        self.ys = _axis_origins(self.image_height, patch, self.center_height)
        self._ix = _axis_intervals(self.xs, self.image_width, patch, self.overlap_width)
        self._iy = _axis_intervals(self.ys, self.image_height, patch, self.overlap_height)

    def __len__(self) -> int:
        return len(self.xs) * len(self.ys)

    @property
    def origins(self) -> np.ndarray:
        """int32 [n_tiles, 2] = (x, y), row-major (the reference's iteration order without the repeated visits)"""
        return np.array([(x, y) for y in self.ys for x in self.xs], dtype=np.int32).reshape(-1, 2)

    def visit_order(self) -> List[int]:
        """tile index for every tile the reference's __iter__ yields, repeats included"""
        def axis(extent, patch, centre, origins):
            idx = []
            for o in range(0, extent, centre):
                if o + patch > extent:
                    o = extent - patch
                idx.append(origins.index(o))
            return idx
        ax = axis(self.image_width, self.patch_size, self.center_width, self.xs)
        ay = axis(self.image_height, self.patch_size, self.center_height, self.ys)
        return [j * len(self.xs) + i for j in ay for i in ax]

    def paste_rects(self) -> np.ndarray:
        """int32 [n_tiles, 6] = (l, t, w, h, px, py): window of the result TILE (pad included in l, t) and where it lands in the
        result image; disjoint, covering the image exactly once."""
        rects = []
        for j, y in enumerate(self.ys):
            y0, y1 = self._iy[j]
            for i, x in enumerate(self.xs):
                x0, x1 = self._ix[i]
                rects.append((x0 - x + self.pad_size, y0 - y + self.pad_size, x1 - x0, y1 - y0, x0, y0))
        return np.array(rects, dtype=np.int32).reshape(-1, 6)


def transform_lut() -> np.ndarray:
    """transform() per byte value (deepliif/data/__init__.py:133-138: ToTensor = v / 255 in fp32, Normalize = (x - 0.5) / 0.5)"""
    v = np.arange(256, dtype=np.float32) / np.float32(255.0)
    return ((v - np.float32(0.5)) / np.float32(0.5)).astype(np.float32)


RESAMPLE_PRECISION_BITS = 22          # Pillow's fixed point for 8-bit images (32 - 8 - 2)
_RESAMPLE_TABLES: Dict[Tuple[int, int], Tuple[np.ndarray, np.ndarray]] = {}


def _bicubic(x: float) -> float:
    """Pillow's bicubic kernel (a = -0.5), operation for operation"""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_table(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Integer coefficient table of PIL's Image.resize (default bicubic, 8-bit) along one axis, in_size -> out_size pixels:
    (bounds int32 [out_size, 2] = (xmin, n), kk int32 [out_size, ksize] zero-filled past n, ksize = 2 * ceil(support) + 1).
    Output byte xx = clip((2**21 + sum_k pixel[xmin + k] * kk[xx, k]) >> 22, 0, 255) with a 32-bit accumulator; a resize runs the
    horizontal pass first, writes uint8, and the vertical pass reads those bytes.  Python floats are IEEE doubles and the operations
    below keep Pillow's order (the filter argument is scaled by the reciprocal 1 / filterscale, as Pillow does), so the table holds
    Pillow's bits; the device kernels (dl_tile_gather_resample_u8 / dl_tile_paste_resample_u8) only apply it.  Cached per pair."""
    key = (int(in_size), int(out_size))
    if key not in _RESAMPLE_TABLES:
        n_in, n_out = key
        if n_in <= 0 or n_out <= 0:
            raise ValueError('resample_table sizes must be positive')
        scale = n_in / n_out
        filterscale = scale if scale > 1.0 else 1.0
        support = 2.0 * filterscale
        ksize = 2 * int(math.ceil(support)) + 1
        ss = 1.0 / filterscale
        one = float(1 << RESAMPLE_PRECISION_BITS)
        bounds = np.zeros((n_out, 2), dtype=np.int32)
        kk = np.zeros((n_out, ksize), dtype=np.int32)
        for xx in range(n_out):
            center = (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), n_in)
            n = xmax - xmin
            w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(n)]
            ww = 0.0
            for v in w:                       # left to right, in double
                ww += v
            if ww != 0.0:
                w = [v / ww for v in w]
            bounds[xx] = (xmin, n)
            kk[xx, :n] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        bounds.setflags(write=False)
        kk.setflags(write=False)
        _RESAMPLE_TABLES[key] = (bounds, kk)
    return _RESAMPLE_TABLES[key]


def resample_apply(a: np.ndarray, out_size: int) -> np.ndarray:
    """resample_table() applied in numpy to a square uint8 image [S, S, C] -> [out_size, out_size, C]: what the device kernels
    compute and what Image.resize returns (the tests hold all three to equality)"""
    def one_pass(src, axis_len_out):
        bounds, kk = resample_table(src.shape[1], axis_len_out)
        acc = np.full((src.shape[0], axis_len_out, src.shape[2]), 1 << (RESAMPLE_PRECISION_BITS - 1), dtype=np.int32)
        s32 = src.astype(np.int32)
        for xx in range(axis_len_out):
            x0, n = (int(v) for v in bounds[xx])
            acc[:, xx] += (s32[:, x0:x0 + n] * kk[xx, :n, None]).sum(axis=1, dtype=np.int32)
        return np.clip(acc >> RESAMPLE_PRECISION_BITS, 0, 255).astype(np.uint8)
    if a.shape[0] != a.shape[1]:
        raise ValueError('resample_apply takes square tiles')
    if a.shape[1] != out_size:
        a = one_pass(a, out_size)                                            # horizontal
        a = one_pass(a.transpose(1, 0, 2), out_size).transpose(1, 0, 2)      # vertical, on the uint8 intermediate
    return np.ascontiguousarray(a)


def gray_stats_empty(stats: np.ndarray) -> np.ndarray:
    """is_empty from {count, sum, sumsq} rows (exact): variance < 9 <=> n*s2 - s1^2 < 9*n^2; no pixel in 1..254 -> variance 0"""
    n, s1, s2 = (stats[:, k].astype(object) for k in range(3))         # Python ints: no overflow whatever the tile size
    return np.array([bool(a == 0 or a * c - b * b < EMPTY_VARIANCE_THRESHOLD * a * a) for a, b, c in zip(n, s1, s2)], dtype=bool)


def _rgb_word(c) -> int:
    return int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16)


class RegionTiler:
    """TilePlan bound to uint8 RGB image(s) [H, W, 3] in HBM (several = the input modalities of a multi-input model).

    `rows=(j0, j1)` restricts the tiler to the tile rows j0..j1-1 of the plan: the rectangles those tiles own form ONE contiguous
    horizontal band of the result, so tile-parallel inference over R ranks is "every rank takes a band, the bands are concatenated"
    -- no overlap to resolve, no collective on the data path (BASELINE configs[4]; deepliif_amd.inference.infer_region).

    `net_size` (when it differs from tile_size): the side the networks run at.  gather() then resizes every tile to it and paste()
    takes [n, net, net, cp] activations and resizes them back, both with PIL's bicubic filter bit for bit (resample_table,
    dl_tile_gather_resample_u8 / dl_tile_paste_resample_u8).  The geometry -- plan, rectangles, bands, results() -- and empty_mask()
    stay in tile coordinates: the reference tests the un-resized tile (run_wrapper, models/__init__.py:399-405)."""

    def __init__(self, images: Sequence[torch.Tensor], tile_size: int, overlap_size: int = 0, pad_size: int = 0, pad_color=(255, 255, 255),
                 rows: Optional[Tuple[int, int]] = None, net_size: Optional[int] = None):
        assert images, 'at least one image'
        for im in images:
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.stride(2) != 1 or im.stride(1) != 3:
                raise TypeError('RegionTiler images are uint8 [H, W, 3] tensors with densely packed pixels')
            if im.shape != images[0].shape:
                raise ValueError('InferenceTiler input images do not have the same size.')
        self.images = list(images)
        self.device = images[0].device
        h, w = int(images[0].shape[0]), int(images[0].shape[1])
        self.plan = p = TilePlan(w, h, tile_size, overlap_size, pad_size)
        j0, j1 = rows if rows is not None else (0, len(p.ys))
        assert 0 <= j0 <= j1 <= len(p.ys)
        self.rows = (j0, j1)
        nx = len(p.xs)
        self.tile_ids = list(range(j0 * nx, j1 * nx))                 # global tile indices this tiler owns
        # the band of result rows those tiles own (clipped to the un-mirrored image height)
        self.band = (min(p._iy[j0][0], p.orig_height), min(p._iy[j1 - 1][1], p.orig_height)) if j1 > j0 else (0, 0)
        self.pad_rgb = _rgb_word(pad_color)
        self.origins = torch.from_numpy(p.origins).to(self.device)
        self.lut = torch.from_numpy(transform_lut()).to(self.device)
        self._rects = p.paste_rects()
        self._results: Dict[str, torch.Tensor] = {}
        self.net_size = int(net_size) if net_size is not None and int(net_size) != p.tile_size else None
        if self.net_size is not None:
            dev = lambda tb: tuple(torch.from_numpy(np.array(a)).to(self.device) for a in tb)
            self._table_in = dev(resample_table(p.tile_size, self.net_size))        # tile -> net, before the networks
            self._table_out = dev(resample_table(self.net_size, p.tile_size))       # net -> tile, after them

    def __len__(self):
        return len(self.tile_ids)

    def _origins_of(self, tile_ids) -> torch.Tensor:
        idx = torch.as_tensor(list(tile_ids), dtype=torch.long, device=self.device)
        return self.origins.index_select(0, idx).contiguous()

    def empty_mask(self) -> np.ndarray:
        """is_empty for every tile of this tiler, in tile_ids order (all input images must be empty: models/__init__.py:393-394)"""
        be = ops.impl()
        p = self.plan
        empty = np.ones(len(self.tile_ids), dtype=bool)
        if not self.tile_ids:
            return empty
        org = self._origins_of(self.tile_ids)
        for im in self.images:
            stats = torch.empty((len(self.tile_ids), 3), dtype=torch.int64, device=self.device)
            be.tile_gray_stats(im, p.orig_height, p.orig_width, org, p.tile_size, p.pad_size, self.pad_rgb, stats)
            empty &= gray_stats_empty(stats.cpu().numpy())
        return empty

    def gather(self, tile_ids: Sequence[int], dtype: torch.dtype, cp: int) -> torch.Tensor:
        """engine tile batch [len(tile_ids), tile, tile, cp] in [-1, 1] (crop + transform); with net_size: [len(tile_ids), net, net, cp]
        (crop + resize + transform)"""
        p = self.plan
        if self.net_size is not None:
            out = torch.empty((len(tile_ids), self.net_size, self.net_size, cp), dtype=dtype, device=self.device)
            ops.impl().tile_gather_resampled(self.images, p.orig_height, p.orig_width, self._origins_of(tile_ids), p.tile_size, p.pad_size, self.pad_rgb,
                                             self.net_size, self._table_in, self.lut, out)
            return out
        out = torch.empty((len(tile_ids), p.tile_size, p.tile_size, cp), dtype=dtype, device=self.device)
        ops.impl().tile_gather(self.images, p.orig_height, p.orig_width, self._origins_of(tile_ids), p.tile_size, p.pad_size, self.pad_rgb, self.lut, out)
        return out

    def result(self, key: str) -> torch.Tensor:
        """this tiler's band of result image `key`: uint8 [band height (mirror extension included), image_width, 3]"""
        if key not in self._results:          # Image.new('RGB', ...) is black (util/__init__.py:289-290)
            p = self.plan
            j0, j1 = self.rows
            y0, y1 = (p._iy[j0][0], p._iy[j1 - 1][1]) if j1 > j0 else (0, 0)
            self._results[key] = torch.zeros((y1 - y0, p.image_width, 3), dtype=torch.uint8, device=self.device)
        return self._results[key]

    def paste(self, key: str, tiles: Optional[torch.Tensor], tile_ids: Sequence[int], const_rgb=None):
        """stitch tiles[i] (engine layout, values in [-1, 1]) as tile tile_ids[i] of result image `key`; tiles None pastes the
        constant colour instead (empty tiles).  With net_size the tiles are [n, net, net, cp] and are resized to the tile first."""
        if not len(tile_ids):
            return
        p = self.plan
        rec = np.zeros((len(tile_ids), 8), dtype=np.int32)
        rec[:, 0] = -1 if tiles is None else np.arange(len(tile_ids))
        rec[:, 1:7] = self._rects[list(tile_ids)]
        rec[:, 6] -= p._iy[self.rows[0]][0]                            # band-local row
        rec[:, 7] = 0 if const_rgb is None else _rgb_word(const_rgb)
        rec = rec[(rec[:, 3] > 0) & (rec[:, 4] > 0)]
        if not len(rec):
            return
        rects = torch.from_numpy(np.ascontiguousarray(rec)).to(self.device)
        if self.net_size is not None and tiles is not None:
            ops.impl().tile_paste_resampled(tiles, self.net_size, p.tile_size, self._table_out, rects, self.result(key))
        else:
            ops.impl().tile_paste(tiles, p.tile_size, rects, self.result(key))

    def results(self) -> Dict[str, torch.Tensor]:
        """result bands cropped back to the original image (util/__init__.py:322-331): rows band[0]..band[1] of the full result"""
        p = self.plan
        h = self.band[1] - self.band[0]
        return {k: v[:h, :p.orig_width] for k, v in self._results.items()}


def split_rows(n_rows: int, world: int) -> List[Tuple[int, int]]:
    """contiguous, near-equal bands of tile rows, one per rank (ranks beyond the row count get an empty band)"""
    base, extra = divmod(n_rows, world)
    out, j = [], 0
    for r in range(world):
        n = base + (1 if r < extra else 0)
        out.append((j, j + n))
        j += n
    return out
