"""Display rendering of 16-bit rasters: a percentile stretch, optionally linked across the bands, with gamma, from
a uint16 [H, W, 3] image to the 8-bit image the PNG writer, the warp, the pyramid and the post-process take.

The two passes over the image run on the device (csrc/display.hip through native.Engine.display_hist_u16 / display_apply_u16);
what lies between them is policy over 3 x 65536 numbers and lives here:

  hist      hist[c][v] = number of samples of channel c with value v, the samples equal to `nodata` left out (they are still mapped).
  limits    percentiles in whole basis points bp = p * 100, 0 <= bp_lo < bp_hi <= 10000.  For a histogram g with n = sum(g):
            k = ((n - 1) * bp) // 10000, limit = the k-th smallest counted sample (0-based) = the smallest v with
            cumsum(g)[v] >= k + 1.  linked: g = hist[0] + hist[1] + hist[2], one (lo, hi) for all bands (keeps the colour balance);
            else g = hist[c].  (0, 100) is min-max.  n == 0 -> (0, 1); hi == lo -> (lo - 1, hi) if hi > 0 else (0, 1).
  lut       lut[c][x] = 0 for x <= lo, 255 for x >= hi; between them (510 * (x - lo) + (hi - lo)) // (2 * (hi - lo)) for gamma == 1
            (round half up, in integers), floor(255 * ((x - lo) / (hi - lo)) ** (1 / gamma) + 0.5) in float64 otherwise.
  out       out[y, x, c] = lut[c][img[y, x, c]].
"""
from __future__ import annotations

from dataclasses import dataclass
from decimal import Decimal
from typing import Optional, Sequence, Tuple

import numpy as np

BINS = 65536


def _basis_points(p, what: str) -> int:
    try:
        bp = Decimal(str(p)) * 100
    except Exception as e:  # noqa: BLE001 -- anything that is no number
        raise ValueError(f"{what} {p!r}: a percentile in percent") from e
    if not bp.is_finite() or bp != bp.to_integral_value():
        raise ValueError(f"{what} {p!r}: percentiles are whole basis points (at most two decimals)")
    return int(bp)


def _norm_limits(limits) -> list:
    a = np.asarray(limits)
    if a.shape == (2,):
        a = np.tile(a, (3, 1))
    if a.shape != (3, 2) or not np.all(a == np.floor(a)):
        raise ValueError(f"limits {limits!r}: (lo, hi) or three of them, integers")
    out = [[int(lo), int(hi)] for lo, hi in a]
    for lo, hi in out:
        if not lo < hi:
            raise ValueError(f"limits {limits!r}: need lo < hi")
    return out


@dataclass(frozen=True)
class Stretch:
    """p_lo, p_hi: percentiles in percent (whole basis points).  linked: one (lo, hi) from the three bands' joint histogram.
    gamma > 0.  nodata: a value left out of the statistics (None: none).  limits: explicit [[lo, hi]] x 3 (or one (lo, hi)) --
    the histogram pass is skipped and p_lo / p_hi / linked / nodata only travel into the info."""
    p_lo: float = 2.0
    p_hi: float = 98.0
    linked: bool = True
    gamma: float = 1.0
    nodata: Optional[int] = None
    limits: Optional[Sequence] = None

    def __post_init__(self):
        lo, hi = _basis_points(self.p_lo, "p_lo"), _basis_points(self.p_hi, "p_hi")
        if not 0 <= lo < hi <= 10000:
            raise ValueError(f"percentiles ({self.p_lo}, {self.p_hi}): need 0 <= p_lo < p_hi <= 100")
        g = float(self.gamma)
        if not (g > 0.0 and np.isfinite(g)):
            raise ValueError(f"gamma {self.gamma!r}: must be positive")
        if self.nodata is not None and not (int(self.nodata) == self.nodata and 0 <= int(self.nodata) <= 65535):
            raise ValueError(f"nodata {self.nodata!r}: an integer in 0..65535, or None")
        if self.limits is not None:
            object.__setattr__(self, "limits", _norm_limits(self.limits))

    @property
    def basis_points(self) -> Tuple[int, int]:
        return _basis_points(self.p_lo, "p_lo"), _basis_points(self.p_hi, "p_hi")

    @classmethod
    def of(cls, spec) -> "Stretch":
        """A Stretch, a dict of its fields, or True / {} for the defaults."""
        if isinstance(spec, cls):
            return spec
        if spec is True:
            return cls()
        if isinstance(spec, dict):
            unknown = set(spec) - set(cls.__dataclass_fields__)
            if unknown:
                raise ValueError(f"display: unknown field(s) {sorted(unknown)}")
            return cls(**spec)
        raise ValueError(f"display {spec!r}: a Stretch or a dict of its fields")

    def info(self, limits) -> dict:
        return {"p_lo": float(self.p_lo), "p_hi": float(self.p_hi), "linked": bool(self.linked), "gamma": float(self.gamma),
                "nodata": None if self.nodata is None else int(self.nodata), "limits": [[int(lo), int(hi)] for lo, hi in limits]}


def _limits_of(g: np.ndarray, bp_lo: int, bp_hi: int) -> list:
    n = int(g.sum(dtype=np.uint64))
    if n == 0:
        return [0, 1]
    cum = np.cumsum(g.astype(np.uint64), dtype=np.uint64)
    lo, hi = (int(np.searchsorted(cum, np.uint64(((n - 1) * bp) // 10000 + 1), side="left")) for bp in (bp_lo, bp_hi))
    if hi == lo:
        lo, hi = (lo - 1, hi) if hi > 0 else (0, 1)
    return [lo, hi]


def limits_from_hist(hist: np.ndarray, stretch: Stretch) -> list:
    """hist [3][65536] counts -> [[lo, hi]] x 3 by the stretch's percentiles."""
    hist = np.asarray(hist)
    if hist.shape != (3, BINS):
        raise ValueError(f"hist shape {hist.shape}: expected (3, {BINS})")
    bp_lo, bp_hi = stretch.basis_points
    if stretch.linked:
        g = hist[0].astype(np.uint64) + hist[1].astype(np.uint64) + hist[2].astype(np.uint64)
        return [_limits_of(g, bp_lo, bp_hi)] * 3
    return [_limits_of(hist[c], bp_lo, bp_hi) for c in range(3)]


def build_lut(limits, gamma: float = 1.0) -> np.ndarray:
    """[[lo, hi]] x 3 -> uint8 [3][65536]."""
    gamma = float(gamma)
    if not (gamma > 0.0 and np.isfinite(gamma)):
        raise ValueError(f"gamma {gamma!r}: must be positive")
    lut = np.empty((3, BINS), np.uint8)
    x = np.arange(BINS, dtype=np.int64)
    for c, (lo, hi) in enumerate(_norm_limits(limits)):
        d = hi - lo
        if gamma == 1.0:
            v = (510 * (x - lo) + d) // (2 * d)
        else:
            t = np.clip((x - lo).astype(np.float64) / np.float64(d), 0.0, 1.0)
            v = np.floor(255.0 * t ** (1.0 / gamma) + 0.5)
        v = np.where(x <= lo, 0, np.where(x >= hi, 255, v))
        lut[c] = v.astype(np.uint8)
    return lut


def render_u16(img16, stretch, engine, shape=None, band_rows: int = 0):
    """uint16 [H, W, 3] -> (uint8 [H, W, 3], info).  img16 None: the image of `shape` (H, W) the previous call on `engine` left on
    the device (native.Engine.enhance_u16 / enhance_blend_u16: their 4H x 4W output).  A host image crosses to the device once."""
    stretch = Stretch.of(stretch)
    if img16 is not None:
        img16 = np.asarray(img16)
        if img16.dtype != np.uint16 or img16.ndim != 3 or img16.shape[2] != 3:
            raise ValueError(f"render_u16 takes a uint16 HxWx3 image, got {img16.dtype} {img16.shape}")
        shape = img16.shape[:2]
    elif shape is None:
        raise ValueError("render_u16: the device copy needs shape=(H, W)")
    limits = stretch.limits
    src = img16
    if limits is None:
        hist = engine.display_hist_u16(img16, nodata=-1 if stretch.nodata is None else int(stretch.nodata), band_rows=band_rows, shape=shape)
        limits = limits_from_hist(hist, stretch)
        src = None                            # the histogram call left the image on the device
    out = engine.display_apply_u16(src, build_lut(limits, stretch.gamma), band_rows=band_rows, shape=shape)
    return out, stretch.info(limits)
