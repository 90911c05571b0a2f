"""Host-side planning of the XYZ tile pyramid (the step after the SR path; reference
server/app/tiling.py:102-186 = gdalwarp to EPSG:3857 + gdal2tiles.py --xyz --resampling average).

The geometry is resolved here in float64 into plain integer / float32 tables; the HIP kernels
(csrc/tiles.hip) then do pixel arithmetic only:

  warp      output pixel -> source pixel coordinates, sampled on a node grid every WARP_STEP output
            pixels (the projection is smooth: linear interpolation between nodes is exact to
            << 0.01 px), bilinear sampling of the source on the device;
  base      tiles of the deepest zoom: every tile pixel averages the source pixels whose centres
            fall inside its footprint (nearest source pixel when the footprint holds none), given
            as [lo, hi] column / row index tables per tile column / row;
  overview  every shallower zoom from the four children of a tile: mean of the valid (alpha > 0)
            pixels of each 2x2 group;
  resample  the other form of both levels (csrc/resample.hip): a separable Lanczos / cubic / bilinear
            filter, given as per-column and per-row tap tables (first source index, tap count, integer
            coefficients) -- plan_resample_axis; the deepest level's box in raster pixels is level_box,
            a shallower level's box in the pixels of the level below it is overview_box.

Parity note: GDAL is not available to this build, so "bilinear" (warp) and "average" are this
build's definitions, not bit-for-bit gdalwarp / gdal2tiles.  The resampled
levels are Pillow's Image.resize arithmetic, integer throughout, and pinned to it byte for byte
(tests/test_resample_cpu.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

from . import geo

WARP_STEP = 64      # output pixels between nodes.  The projection pair is smooth on this scale: against projecting every pixel the
                    # interpolated source coordinate is off by < 1e-3 px at 64 (tests/test_tiles_cpu.py), and the plan of a 4096 x 4096
                    # raster costs 0.6 ms instead of 9 (r04: 16 -> 66k nodes through the Krueger series per pyramid)


@dataclass
class WarpPlan:
    out_h: int
    out_w: int
    placement: geo.Placement          # of the output raster, EPSG:3857
    grid: np.ndarray                  # float32 [gh, gw, 2]: source (col, row) in pixel-centre coordinates at the nodes
    step: int = WARP_STEP


def plan_warp(width: int, height: int, src: geo.Placement, crs: geo.CRS) -> WarpPlan:
    """Output grid like GDAL's suggested warp output: the extent of the densified source outline,
    square pixels sized so that the pixel count along the diagonal is preserved."""
    t = np.linspace(0.0, 1.0, 21)
    w, s, e, n = src.bounds(width, height)
    ex = np.concatenate([w + (e - w) * t, np.full(21, e), e - (e - w) * t, np.full(21, w)])
    ey = np.concatenate([np.full(21, n), n - (n - s) * t, np.full(21, s), s + (n - s) * t])
    lon, lat = crs.to_lonlat(ex, ey)
    mx, my = geo.lonlat_to_mercator(lon, lat)
    mw, me, ms, mn = float(mx.min()), float(mx.max()), float(my.min()), float(my.max())
    res = math.hypot(me - mw, mn - ms) / math.hypot(width, height)
    ow, oh = max(1, int((me - mw) / res + 0.5)), max(1, int((mn - ms) / res + 0.5))
    dst = geo.Placement(mw, mn, res, res)
    gh, gw = (oh - 1 + WARP_STEP - 1) // WARP_STEP + 1, (ow - 1 + WARP_STEP - 1) // WARP_STEP + 1
    jj, ii = np.meshgrid(np.arange(gw, dtype=np.float64) * WARP_STEP, np.arange(gh, dtype=np.float64) * WARP_STEP)
    X = mw + (jj + 0.5) * res
    Y = mn - (ii + 0.5) * res
    lon, lat = geo.mercator_to_lonlat(X, Y)
    sx, sy = crs.from_lonlat(lon, lat)
    u = (sx - src.x0) / src.dx - 0.5
    v = (src.y0 - sy) / src.dy - 0.5
    return WarpPlan(oh, ow, dst, np.stack([u, v], -1).astype(np.float32))


@dataclass
class LevelPlan:
    zoom: int
    tminx: int
    tminy: int
    tmaxx: int
    tmaxy: int                        # TMS numbering; arrays are stored north row first

    @property
    def nx(self) -> int:
        return self.tmaxx - self.tminx + 1

    @property
    def ny(self) -> int:
        return self.tmaxy - self.tminy + 1


def plan_levels(bounds, min_zoom: int, max_zoom: int) -> List[LevelPlan]:
    """Deepest zoom first."""
    return [LevelPlan(z, *geo.tile_range(bounds, z)) for z in range(max_zoom, min_zoom - 1, -1)]


def _footprint(a: np.ndarray, b: np.ndarray, n: int):
    """Index ranges [lo, hi] of the source pixels whose centres (index + 0.5) lie in [a, b), a and b in
    continuous source-pixel coordinates (columns rightwards, rows downwards).  A footprint that holds
    no centre falls back to the pixel containing its midpoint.  Clipped to the raster: lo > hi = nothing."""
    lo = np.ceil(a - 0.5).astype(np.int64)
    hi = np.ceil(b - 0.5).astype(np.int64) - 1
    centre = np.floor((a + b) * 0.5).astype(np.int64)
    empty = hi < lo
    lo = np.where(empty, centre, lo)
    hi = np.where(empty, centre, hi)
    return np.maximum(lo, 0).astype(np.int32), np.minimum(hi, n - 1).astype(np.int32)


def plan_base(level: LevelPlan, src: geo.Placement, width: int, height: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """-> col_lo, col_hi [nx*256], row_lo, row_hi [ny*256] (rows north to south)."""
    r = geo.resolution(level.zoom)
    px = np.arange(level.nx * geo.TILE, dtype=np.float64)
    x_lo = level.tminx * geo.TILE * r - geo.ORIGIN_SHIFT + px * r          # west edge of every tile-pixel column
    col_lo, col_hi = _footprint((x_lo - src.x0) / src.dx, (x_lo + r - src.x0) / src.dx, width)
    py = np.arange(level.ny * geo.TILE, dtype=np.float64)
    y_hi = (level.tmaxy + 1) * geo.TILE * r - geo.ORIGIN_SHIFT - py * r    # north edge of every tile-pixel row
    row_lo, row_hi = _footprint((src.y0 - y_hi) / src.dy, (src.y0 - (y_hi - r)) / src.dy, height)
    return col_lo, col_hi, row_lo, row_hi


def overview_offsets(parent: LevelPlan, child: LevelPlan) -> Tuple[int, int]:
    """Child-array (col, row) of the north-west child of the parent array's first tile."""
    return 2 * parent.tminx - child.tminx, child.tmaxy - (2 * parent.tmaxy + 1)


# ---------------------------------------------------------------------------------------------
# resampled levels: Lanczos / cubic / bilinear as tap tables
# ---------------------------------------------------------------------------------------------
FILTERS = ("lanczos", "cubic", "bilinear")
RESAMPLE_MAX_TAPS = 64          # S2SR_RESAMPLE_MAX_TAPS
COEF_BITS = 22                  # fractional bits of a coefficient: 32 - 8 (pixel) - 2 (headroom for sum|coef| < 2)
_SUPPORT = {"lanczos": 3.0, "cubic": 2.0, "bilinear": 1.0}


def _sinc(x: np.ndarray) -> np.ndarray:
    y = x * np.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(y) / y)


def _filter(name: str, x: np.ndarray) -> np.ndarray:
    x = np.abs(x)               # all three are even
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    if name == "cubic":         # Keys, a = -0.5
        a = -0.5
        return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                        np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))
    return np.where(x < 3.0, _sinc(x) * _sinc(x / 3.0), 0.0)


def plan_resample_axis(n_out: int, a0: float, a1: float, n_src: int, filter: str):
    """One axis of a resampled level: n_out samples cover [a0, a1) in continuous source-pixel coordinates (either end may lie
    outside [0, n_src]).  -> first [n_out] int32, count [n_out] int32, coef [n_out, K] int32, K: sample j is
    clip((2^21 + sum_t coef[j, t] * src[first[j] + t]) >> 22) over t < count[j].  The weights of the whole window
    [floor(c - support + 0.5), floor(c + support + 0.5)) are normalised in float64 and rounded (half away from zero) to 22
    fractional bits FIRST; the taps outside [0, n_src) are dropped afterwards: the raster lies in a transparent plane, its edge is
    not replicated, a window that misses it has 0 taps.  K is the largest whole window."""
    if filter not in FILTERS:
        raise ValueError(f"filter {filter!r}: one of {FILTERS}")
    if n_out <= 0 or n_src <= 0 or not a1 > a0:
        raise ValueError(f"n_out {n_out}, n_src {n_src}, [{a0}, {a1}): nothing to resample")
    scale = (float(a1) - float(a0)) / n_out
    fs = max(scale, 1.0)
    support = _SUPPORT[filter] * fs
    ss = 1.0 / fs
    c = float(a0) + (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.floor(c - support + 0.5).astype(np.int64)
    hi = np.floor(c + support + 0.5).astype(np.int64)
    K = max(1, int((hi - lo).max()))
    if K > RESAMPLE_MAX_TAPS:
        raise ValueError(f"{filter} at {scale:.2f} source pixels per tile pixel needs {K} taps, {RESAMPLE_MAX_TAPS} is the limit: "
                         "choose a deeper max_zoom")
    t = np.arange(K, dtype=np.int64)[None, :]
    inside = t < (hi - lo)[:, None]
    w = np.where(inside, _filter(filter, ((lo[:, None] + t).astype(np.float64) - c[:, None] + 0.5) * ss), 0.0)
    ww = np.add.accumulate(w, axis=1)[:, -1:]                       # summed left to right
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    full = np.trunc(w * float(1 << COEF_BITS) + np.where(w < 0.0, -0.5, 0.5)).astype(np.int64)
    skip = np.clip(-lo, 0, None)                                    # taps west / north of the raster
    first = lo + skip
    count = np.clip(np.minimum(hi, n_src) - first, 0, None)
    first = np.where(count > 0, first, 0)
    coef = np.take_along_axis(full, np.minimum(t + skip[:, None], K - 1), axis=1)
    coef = np.where(t < count[:, None], coef, 0)
    return first.astype(np.int32), count.astype(np.int32), np.ascontiguousarray(coef, np.int32), K


def level_box(level: LevelPlan, place: geo.Placement) -> Tuple[float, float, float, float]:
    """(x0, y0, x1, y1): the level mosaic's west, north, east and south edges in the raster's continuous pixel coordinates
    (columns rightwards, rows downwards) -- the geometry of plan_base."""
    r = geo.resolution(level.zoom)
    x_lo = level.tminx * geo.TILE * r - geo.ORIGIN_SHIFT
    y_hi = (level.tmaxy + 1) * geo.TILE * r - geo.ORIGIN_SHIFT
    return ((x_lo - place.x0) / place.dx, (place.y0 - y_hi) / place.dy,
            (x_lo + level.nx * geo.TILE * r - place.x0) / place.dx, (place.y0 - (y_hi - level.ny * geo.TILE * r)) / place.dy)


def overview_box(parent: LevelPlan, child: LevelPlan) -> Tuple[float, float, float, float]:
    """(x0, y0, x1, y1): the parent mosaic's extent in child-mosaic pixels; the scale is exactly 2."""
    ox, oy = overview_offsets(parent, child)
    return (float(ox * geo.TILE), float(oy * geo.TILE), float((ox + 2 * parent.nx) * geo.TILE), float((oy + 2 * parent.ny) * geo.TILE))


def plan_resample_level(level: LevelPlan, box, n_cols: int, n_rows: int, filter: str):
    """-> (cols, rows): the column and row tables (first, count, coef, K) of a level whose mosaic covers `box` of a source n_cols
    wide and n_rows high."""
    x0, y0, x1, y1 = box
    return (plan_resample_axis(level.nx * geo.TILE, x0, x1, n_cols, filter),
            plan_resample_axis(level.ny * geo.TILE, y0, y1, n_rows, filter))
