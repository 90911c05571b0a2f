"""The display rendering of 16-bit images, restated from scratch for the tests: limits from the sorted counted
samples, the histogram from np.bincount, the LUT as a plain loop.  Shares no code with s2sr/display.py."""
import math

import numpy as np


def counted(img, c, nodata=None):
    """The samples of channel c that enter its statistics."""
    v = np.asarray(img)[..., c].reshape(-1).astype(np.int64)
    return v if nodata is None else v[v != nodata]


def hist(img, nodata=None):
    return np.stack([np.bincount(counted(img, c, nodata), minlength=65536) for c in range(3)]).astype(np.uint64)


def _limit_pair(samples, p_lo, p_hi):
    s = np.sort(samples)
    n = len(s)
    if n == 0:
        return [0, 1]
    lo, hi = (int(s[((n - 1) * int(round(p * 100))) // 10000]) for p in (p_lo, p_hi))
    if hi == lo:
        lo, hi = (lo - 1, hi) if hi > 0 else (0, 1)
    return [lo, hi]


def limits(img, p_lo=2.0, p_hi=98.0, linked=True, nodata=None):
    if linked:
        return [_limit_pair(np.concatenate([counted(img, c, nodata) for c in range(3)]), p_lo, p_hi)] * 3
    return [_limit_pair(counted(img, c, nodata), p_lo, p_hi) for c in range(3)]


def lut_entry(x, lo, hi, gamma=1.0):
    if x <= lo:
        return 0
    if x >= hi:
        return 255
    if gamma == 1.0:
        return (510 * (x - lo) + (hi - lo)) // (2 * (hi - lo))
    return int(math.floor(255.0 * (np.float64(x - lo) / np.float64(hi - lo)) ** (1.0 / gamma) + 0.5))


def lut(lims, gamma=1.0):
    out = np.empty((3, 65536), np.uint8)
    for c, (lo, hi) in enumerate(lims):
        for x in range(65536):
            out[c, x] = lut_entry(x, lo, hi, gamma)
    return out


def apply(img, table):
    img = np.asarray(img)
    return np.stack([table[c][img[..., c]] for c in range(3)], axis=-1)


def render(img, p_lo=2.0, p_hi=98.0, linked=True, gamma=1.0, nodata=None):
    lims = limits(img, p_lo, p_hi, linked, nodata)
    return apply(img, lut(lims, gamma)), lims
