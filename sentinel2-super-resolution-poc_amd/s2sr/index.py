"""Host-side policy of the spectral indices on the SR grid: which bands make an index, the colour ramps and their
LUT, the statistics taken from the histogram, the per-zone table, and the refusals every layer above the engine shares.  The
device work -- one pass over two uint16 planes that gives the int16 index, its RGBA rendering, its exact histogram and exact
zonal sums -- is csrc/index.hip, behind native.Engine.index_nd_u16 / index_render_i16.

  v = round_half_away_from_zero(K (a' - b') / (a' + b' + L)), a' = max(a - offset, 0), b' likewise; -32768 where a' + b' + L == 0
  or the pixel is masked.  A statistic named in index units is v / K.

An index is named by a preset (its roles filled from the bands the caller names) or spelled out:
  "ndvi"                                   the preset with the default roles: red 1, green 2, blue 3, nir 4
  {"preset": "ndre", "nir": 4, "rededge": 5}
  {"name": "mine", "a": 4, "b": 1, "offset": 1000, "L": 0, "K": 10000}
Band numbers are the 1-based bands of the job's file; 1..3 are the super-resolved product, 4 on are carried for the index.

What the default ramps and a DN offset do on real scenes is unmeasured: the ramps are conventional colours over conventional
breaks, and the offset is the caller's knowledge of the product (Sentinel-2 L2A baseline 04.00 and later: 1000)."""
from __future__ import annotations

import math
import re
from typing import Optional, Sequence

import numpy as np

NODATA = -32768
K_MAX = 16383
ROLES = {"red": 1, "green": 2, "blue": 3, "nir": 4}            # the default bands of the roles; rededge has none
# name: (role of a, role of b, L, K).  SAVI on 1/10000 reflectance: L = 0.5 -> 5000 DN, and its (1 + L) factor is K = 15000
PRESETS = {
    "ndvi": ("nir", "red", 0, 10000),
    "ndwi": ("green", "nir", 0, 10000),
    "ndre": ("nir", "rededge", 0, 10000),
    "savi": ("nir", "red", 5000, 15000),
}
# colour ramps: (value at K = 10000, r, g, b) stops; values scale with K (ramp_for)
RAMPS = {
    # bare soil and water in browns and greys, vegetation from pale to deep green
    "vegetation": [(-10000, 12, 12, 60), (-2000, 90, 90, 120), (0, 165, 145, 120), (1000, 200, 180, 140), (2000, 235, 225, 150), (3000, 200, 220, 120),
                   (4500, 140, 190, 80), (6000, 70, 150, 50), (8000, 20, 105, 35), (10000, 0, 60, 20)],
    # a diverging ramp around zero: blue below, white at zero, red above
    "diverging": [(-10000, 5, 48, 97), (-5000, 67, 147, 195), (0, 247, 247, 247), (5000, 214, 96, 77), (10000, 103, 0, 31)],
}
DEFAULT_RAMP = {"ndvi": "vegetation", "savi": "vegetation", "ndre": "vegetation", "ndwi": "diverging"}
PERCENTILES = (2.0, 25.0, 50.0, 75.0, 98.0)


def _int(v, lo: int, hi: int, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"indices: {what} must be an integer in {lo}..{hi}, got {v!r}")
    return int(v)


def resolve(indices, index_offset: int = 0, count: Optional[int] = None) -> list:
    """A job's `indices` -> [{"name", "preset", "a", "b", "offset", "L", "K"}], refusing (ValueError) whatever can be refused
    without the pixels: an unknown preset or key, a role without a band, a band outside the file (count given), a == b, a
    repeated or unusable name, K, L or offset out of range."""
    index_offset = _int(index_offset, 0, 65535, "index_offset")
    if isinstance(indices, (str, dict)) or indices is None:
        raise ValueError(f"indices {indices!r}: a list of preset names or definitions")
    try:
        entries = list(indices)
    except TypeError:
        raise ValueError(f"indices {indices!r}: a list of preset names or definitions") from None
    if not entries:
        raise ValueError("indices: the list is empty")
    out = []
    for e in entries:
        if isinstance(e, str):
            e = {"preset": e}
        if not isinstance(e, dict):
            raise ValueError(f"indices: {e!r} is neither a preset name nor a definition")
        if "preset" in e:
            p = e["preset"]
            if p not in PRESETS:
                raise ValueError(f"indices: unknown preset {p!r} (known: {', '.join(sorted(PRESETS))})")
            ra, rb, L, K = PRESETS[p]
            unknown = set(e) - {"preset", "name", "offset", "rededge", *ROLES}
            if unknown:
                raise ValueError(f"indices: unknown field(s) {sorted(unknown)} for preset {p!r}")
            bands = {}
            for role in (ra, rb):
                if role not in e and role not in ROLES:
                    raise ValueError(f"indices: preset {p!r} needs the band that plays {role!r}, e.g. {{\"preset\": \"{p}\", \"{role}\": 5}}")
                bands[role] = e.get(role, ROLES.get(role))
            d = {"name": e.get("name", p), "preset": p, "a": bands[ra], "b": bands[rb], "offset": e.get("offset", index_offset), "L": L, "K": K}
        else:
            unknown = set(e) - {"name", "a", "b", "offset", "L", "K"}
            if unknown:
                raise ValueError(f"indices: unknown field(s) {sorted(unknown)} in a definition")
            for k in ("name", "a", "b"):
                if k not in e:
                    raise ValueError(f"indices: a definition needs \"name\", \"a\" and \"b\"; {k!r} is missing from {e!r}")
            d = {"name": e["name"], "preset": None, "a": e["a"], "b": e["b"], "offset": e.get("offset", index_offset), "L": e.get("L", 0),
                 "K": e.get("K", 10000)}
        if not isinstance(d["name"], str) or not re.fullmatch(r"[A-Za-z0-9][A-Za-z0-9_-]{0,31}", d["name"]):
            raise ValueError(f"indices: the name {d['name']!r} must be 1..32 letters, digits, '_' or '-' (it names the files)")
        d["a"] = _int(d["a"], 1, 65535, f"band a of {d['name']!r}")
        d["b"] = _int(d["b"], 1, 65535, f"band b of {d['name']!r}")
        if d["a"] == d["b"]:
            raise ValueError(f"indices: {d['name']!r} takes band {d['a']} twice")
        if count is not None:
            for k in ("a", "b"):
                if d[k] > count:
                    raise ValueError(f"indices: band {d[k]} of {d['name']!r} is not in the file ({count} bands)")
        d["offset"] = _int(d["offset"], 0, 65535, f"offset of {d['name']!r}")
        d["L"] = _int(d["L"], 0, 65535, f"L of {d['name']!r}")
        d["K"] = _int(d["K"], 1, K_MAX, f"K of {d['name']!r}")
        if d["name"] in [o["name"] for o in out]:
            raise ValueError(f"indices: the name {d['name']!r} is used twice")
        out.append(d)
    return out


def carried_bands(defs) -> list:
    """the file bands from 4 on that the definitions read, in ascending order"""
    return sorted({d[k] for d in defs for k in ("a", "b") if d[k] >= 4})


# ---- colour ramps ------------------------------------------------------------------------------------------------------------------------
def check_ramp(stops) -> list:
    try:
        stops = [tuple(s) for s in stops]
    except TypeError:
        raise ValueError(f"ramp {stops!r}: a list of (value, r, g, b) stops") from None
    if len(stops) < 2 or any(len(s) != 4 for s in stops):
        raise ValueError("ramp: at least two (value, r, g, b) stops are required")
    for s in stops:
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in s):
            raise ValueError(f"ramp: the stop {s!r} must hold integers")
        if not -32767 <= s[0] <= 32767 or any(not 0 <= c <= 255 for c in s[1:]):
            raise ValueError(f"ramp: the stop {s!r} needs a value in -32767..32767 and colours in 0..255")
    if any(b[0] <= a[0] for a, b in zip(stops, stops[1:])):
        raise ValueError("ramp: the stops' values must increase strictly")
    return [tuple(int(x) for x in s) for s in stops]


def ramp_for(ramp, K: int = 10000) -> list:
    """A ramp's stops for scale K: a name from RAMPS (its values, stated at K = 10000, scaled to K and made strictly increasing)
    or explicit stops, taken as they are."""
    if isinstance(ramp, str):
        if ramp not in RAMPS:
            raise ValueError(f"ramp {ramp!r}: one of {', '.join(sorted(RAMPS))}, or a list of (value, r, g, b) stops")
        stops, last = [], None
        for v, r, g, b in RAMPS[ramp]:
            sv = (2 * v * K + 10000) // 20000 if v >= 0 else -((2 * -v * K + 10000) // 20000)
            if last is not None and sv <= last:
                continue                                        # a tiny K folds neighbouring stops into one
            stops.append((sv, r, g, b))
            last = sv
        return check_ramp(stops)
    return check_ramp(ramp)


def ramp_lut(stops) -> np.ndarray:
    """uint8 [65536][4], entry (uint16)(v + 32768): the first stop's colour at and below it, the last one's at and above it,
    between two stops c0 + floor((2 (c1 - c0) (v - v0) + (v1 - v0)) / (2 (v1 - v0))) per channel (integers, round half up);
    alpha 255.  Entry 0 (-32768, nodata) is 0, 0, 0, 0; the device writes that for nodata whatever the LUT holds."""
    stops = check_ramp(stops)
    v = np.arange(-32768, 32768, dtype=np.int64)
    vals = np.array([s[0] for s in stops], np.int64)
    cols = np.array([s[1:] for s in stops], np.int64)
    k = np.clip(np.searchsorted(vals, v, side="right") - 1, 0, len(stops) - 2)
    v0, v1 = vals[k], vals[k + 1]
    t = np.clip(v, v0, v1) - v0
    den = v1 - v0
    lut = np.empty((65536, 4), np.uint8)
    for c in range(3):
        c0, c1 = cols[k, c], cols[k + 1, c]
        lut[:, c] = c0 + (2 * (c1 - c0) * t + den) // (2 * den)
    lut[:, 3] = 255
    lut[0] = 0
    return lut


# ---- statistics from the histogram --------------------------------------------------------------------------------------------------------
def _basis_points(p) -> int:
    from .display import _basis_points as bp
    v = bp(p, "percentile")
    if not 0 <= v <= 10000:
        raise ValueError(f"percentile {p!r}: 0..100")
    return v


def stats_from_hist(hist, K: int, percentiles: Sequence[float] = PERCENTILES, threshold: Optional[float] = None,
                    pixel_size: Optional[Sequence[float]] = None) -> dict:
    """hist uint64 [2 K + 1] -> count, min, max, mean, std and percentiles in index units (v / K).  The moments are exact
    integers; the percentile of bp basis points is the k-th smallest value, k = ((n - 1) bp) // 10000 (display.py's rule).
    threshold (index units): the pixels with v >= ceil(threshold K), their fraction and, with pixel_size (x, y in metres), hectares."""
    h = np.asarray(hist)
    if h.shape != (2 * K + 1,):
        raise ValueError(f"stats_from_hist: hist must be [2 K + 1] = [{2 * K + 1}], got {h.shape}")
    counts = [int(x) for x in h]
    n = sum(counts)
    out = {"count": n, "min": None, "max": None, "mean": None, "std": None, "percentiles": {}}
    if n:
        nz = np.nonzero(h)[0]
        s = sum(c * (i - K) for i, c in enumerate(counts) if c)
        s2 = sum(c * (i - K) * (i - K) for i, c in enumerate(counts) if c)
        out.update(min=(int(nz[0]) - K) / K, max=(int(nz[-1]) - K) / K, mean=s / (n * K), std=math.sqrt(max(n * s2 - s * s, 0)) / (n * K))
        cum = np.cumsum(h.astype(np.uint64), dtype=np.uint64)
        for p in percentiles:
            bp = _basis_points(p)
            out["percentiles"][f"p{p:g}"] = (int(np.searchsorted(cum, np.uint64(((n - 1) * bp) // 10000 + 1), side="left")) - K) / K
    if threshold is not None:
        from decimal import Decimal
        tv = min(max(math.ceil(Decimal(str(threshold)) * K), -K), K + 1)      # (0.3 is 3000 / 10000, not the double next to it)
        above = sum(counts[tv + K:])
        out["threshold"] = {"value": float(threshold), "count": above, "fraction": above / n if n else None}
        if pixel_size is not None:
            out["threshold"]["area_ha"] = above * abs(float(pixel_size[0]) * float(pixel_size[1])) / 10000.0
    return out


def zonal_table(zonal, K: int) -> list:
    """zonal int64 [Z + 1][3] -> [{"zone", "count", "mean", "std"}] for the labels that hold a defined pixel (0: no zone), in index units"""
    rows = []
    for z, (n, s, s2) in enumerate(np.asarray(zonal).tolist()):
        if n:
            rows.append({"zone": z, "count": n, "mean": s / (n * K), "std": math.sqrt(max(n * s2 - s * s, 0)) / (n * K)})
    return rows


def check_zones(zones, in_shape, scale: int):
    """A label raster on the input grid (zone_scale = scale) or on the output grid (zone_scale = 1) -> (uint16 labels, zone_scale, Z)"""
    z = np.asarray(zones)
    if z.ndim == 3 and z.shape[2] == 1:
        z = z[..., 0]
    if z.ndim != 2 or z.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"zones: a single-band uint8 or uint16 label raster is required, got {z.dtype} {z.shape}")
    H, W = in_shape
    if z.shape == (H, W):
        zs = scale
    elif z.shape == (H * scale, W * scale):
        zs = 1
    else:
        raise ValueError(f"zones: the labels are {z.shape[0]} x {z.shape[1]}, neither the input grid {H} x {W} nor the output grid {H * scale} x {W * scale}")
    Z = int(z.max(initial=0))
    if Z < 1:
        raise ValueError("zones: the raster holds no label above 0")
    return np.ascontiguousarray(z, np.uint16), zs, Z


def metadata_entry(d: dict, undefined: int, stats: dict, ramp, files: dict, zones=None) -> dict:
    """one index's entry of the "indices" block of a job's metadata"""
    e = {"name": d["name"], "preset": d["preset"], "a": d["a"], "b": d["b"], "offset": d["offset"], "L": d["L"], "K": d["K"], "nodata": NODATA,
         "definition": "round_half_away(K (a' - b') / (a' + b' + L)), a' = max(band a - offset, 0), b' = max(band b - offset, 0)",
         "undefined": int(undefined), "statistics": stats, "ramp": ramp if isinstance(ramp, str) else [list(s) for s in ramp], "files": files}
    if zones is not None:
        e["zones"] = zones
    return e
