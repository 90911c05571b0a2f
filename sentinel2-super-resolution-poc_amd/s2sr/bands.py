"""Host-side helpers of carrying extra bands to the SR grid: the defaults, the refusals every layer above the
engine shares, the band numbers of a job and its metadata block.  The device work -- guided upsampling of a uint16 band against
the 16-bit door's image, then one back-projection step -- is in csrc/bands.hip, behind native.Engine.carry_band_u16.

What the default eps and the gain limit of 4 do on real imagery is unmeasured: they come from the definition, not from a sweep."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

WEIGHTS = (1, 1, 1)          # the guide: the plain mean of the three channels
RADIUS = 2                   # the window is (2 r + 1)^2 input pixels
GAIN_LIMIT = 4               # |A| <= 4 (csrc/bands.hip)


def default_eps(lo: int, hi: int) -> int:
    """1/256 of the band's range, squared (squared sample units), at least 1"""
    return max(1, ((int(hi) - int(lo)) >> 8) ** 2)


def check_args(S: int, lo: int, hi: int, weights: Sequence[int] = WEIGHTS, r: int = RADIUS, eps: Optional[int] = None, fill: int = 0,
               band_rows: int = 0) -> dict:
    """The library's refusals, as ValueError before anything is created; returns the arguments with the defaults filled in."""
    if S not in (2, 4):
        raise ValueError(f"bands: S must be 2 or 4, got {S!r}")
    if not (isinstance(lo, (int, np.integer)) and isinstance(hi, (int, np.integer)) and 0 <= lo < hi <= 65535):
        raise ValueError(f"bands: need integers 0 <= lo < hi <= 65535, got {lo!r}, {hi!r}")
    try:
        w = tuple(int(x) for x in weights)
    except (TypeError, ValueError):
        raise ValueError(f"bands: three guide weights 0..255 are required, got {weights!r}") from None
    if len(w) != 3 or any(x < 0 or x > 255 or x != y for x, y in zip(w, weights)) or sum(w) < 1:
        raise ValueError(f"bands: three integer guide weights 0..255, not all zero, are required, got {weights!r}")
    if not (isinstance(r, (int, np.integer)) and 1 <= r <= 4):
        raise ValueError(f"bands: the window radius r must be 1..4, got {r!r}")
    if eps is None:
        eps = default_eps(lo, hi)
    if not (isinstance(eps, (int, np.integer)) and 1 <= eps < 2 ** 31):
        raise ValueError(f"bands: eps must be an integer >= 1 (squared sample units), got {eps!r}")
    if not (isinstance(fill, (int, np.integer)) and 0 <= fill <= 65535):
        raise ValueError(f"bands: fill must be 0..65535, got {fill!r}")
    if not (isinstance(band_rows, (int, np.integer)) and band_rows >= 0):
        raise ValueError(f"bands: band_rows must be >= 0, got {band_rows!r}")
    return dict(S=int(S), lo=int(lo), hi=int(hi), weights=w, r=int(r), eps=int(eps), fill=int(fill), band_rows=int(band_rows))


def band_range(band: np.ndarray, valid: Optional[np.ndarray] = None) -> tuple:
    """(lo, hi): the band's own min and max over the valid pixels; a flat (or empty) band gets a range of one level"""
    px = np.asarray(band) if valid is None else np.asarray(band)[np.asarray(valid) != 0]
    if px.size == 0:
        return 0, 1
    lo, hi = int(px.min()), int(px.max())
    if lo == hi:
        lo, hi = (lo, lo + 1) if lo < 65535 else (lo - 1, lo)
    return lo, hi


def select_bands(extra_bands, count: Optional[int] = None) -> list:
    """A job's `extra_bands` as 1-based band numbers of a `count`-band file: "all" = 4 .. count; a list as given.  ValueError for
    a number below 4 (bands 1-3 are the net's) or absent from the file, a repeated number, and a file with no band to carry.
    count None (no file in hand yet): what can be refused without one."""
    if isinstance(extra_bands, str):
        if extra_bands != "all":
            raise ValueError(f"extra_bands {extra_bands!r}: \"all\" or a list of band numbers from 4 on")
        if count is None:
            return []
        nums = list(range(4, count + 1))
    else:
        try:
            nums = list(extra_bands)
        except TypeError:
            raise ValueError(f"extra_bands {extra_bands!r}: \"all\" or a list of band numbers from 4 on") from None
        if any(isinstance(b, bool) or not isinstance(b, (int, np.integer)) for b in nums):
            raise ValueError(f"extra_bands {extra_bands!r}: band numbers are integers")
        nums = [int(b) for b in nums]
    if not nums:
        raise ValueError("extra_bands: no band to carry" + ("" if count is None else f": the file has {count} band(s)") + " (bands 1-3 are the net's)")
    for b in nums:
        if b < 4:
            raise ValueError(f"extra_bands: band {b} is below 4 (bands 1-3 are the net's input)")
        if count is not None and b > count:
            raise ValueError(f"extra_bands: band {b} is not in the file ({count} bands)")
    if len(set(nums)) != len(nums):
        raise ValueError(f"extra_bands {extra_bands!r}: a band is listed twice")
    return nums


def metadata_block(numbers, ranges, weights_rgb, r: int, eps, inexact) -> dict:
    """The "extra_bands" block of a job's metadata."""
    return {"bands": [int(b) for b in numbers], "ranges": [[int(a), int(b)] for a, b in ranges], "weights_rgb": [int(x) for x in weights_rgb],
            "r": int(r), "eps": [int(e) for e in eps], "gain_limit": GAIN_LIMIT, "inexact_blocks": [int(v) for v in inexact]}
