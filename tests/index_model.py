"""The definition of the normalised-difference index pass (csrc/index.hip) in numpy and Python integers: the index,
its histogram, rendering and zonal sums, the LUT of a colour ramp, and the statistics taken from the histogram.  The GPU tests
hold the kernels to this byte for byte; s2sr/index.py's policy is compared with the rules restated here.

  a' = max(a - offset, 0), b' = max(b - offset, 0), n = a' - b', d = a' + b' + L
  v  = sign(n) floor((2 |n| K + d) / (2 d)) for d > 0, -32768 for d == 0 or a pixel whose mask cell is 0
"""
import functools

import numpy as np

NODATA = -32768


def cells(m, H, W, scale):
    """the cell grid [ceil(H / scale), ceil(W / scale)] spread over the pixels [H, W]"""
    m = np.asarray(m)
    assert m.shape == (-(-H // scale), -(-W // scale)), (m.shape, H, W, scale)
    return np.repeat(np.repeat(m, scale, axis=0), scale, axis=1)[:H, :W]


def value(a, b, offset=0, L=0, K=10000):
    """one pixel in Python integers: the value, or None when d == 0; the widest intermediate as the second result"""
    a1, b1 = max(int(a) - offset, 0), max(int(b) - offset, 0)
    n, d = a1 - b1, a1 + b1 + L
    if d == 0:
        return None, 0
    top = 2 * abs(n) * K + d
    q = top // (2 * d)
    return (-q if n < 0 else q), top


def index(a, b, offset=0, L=0, K=10000, valid=None, valid_scale=1):
    """uint16 [H, W] x 2 -> (int16 [H, W], undefined): int64 numpy, the same integers as value()"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint16 and b.dtype == np.uint16 and a.shape == b.shape and a.ndim == 2
    assert 0 <= offset <= 65535 and 0 <= L <= 65535 and 1 <= K <= 16383
    H, W = a.shape
    a1 = np.maximum(a.astype(np.int64) - offset, 0)
    b1 = np.maximum(b.astype(np.int64) - offset, 0)
    n, d = a1 - b1, a1 + b1 + L
    assert int((2 * np.abs(n) * K + d).max()) < 2 ** 32
    q = (2 * np.abs(n) * K + d) // np.maximum(2 * d, 1)
    v = np.where(n < 0, -q, q)
    keep = np.ones((H, W), bool) if valid is None else cells(valid, H, W, valid_scale) != 0
    undefined = int((keep & (d == 0)).sum())
    v = np.where(keep & (d != 0), v, NODATA)
    assert np.abs(v[v != NODATA]).max(initial=0) <= K
    return v.astype(np.int16), undefined


def hist(v, K):
    """uint64 [2 K + 1]: hist[v + K], nodata left out"""
    v = np.asarray(v).astype(np.int64)
    return np.bincount(v[v != NODATA] + K, minlength=2 * K + 1).astype(np.uint64)


def render(v, lut):
    """uint8 [H, W, 4] = lut[(uint16)(v + 32768)], nodata -> 0, 0, 0, 0"""
    v = np.asarray(v)
    lut = np.asarray(lut)
    assert v.dtype == np.int16 and lut.dtype == np.uint8 and lut.shape == (65536, 4)
    out = lut[v.astype(np.int64) + 32768]
    out[v == NODATA] = 0
    return out


def zonal(v, zones, zone_scale, Z):
    """int64 [Z + 1][3]: count, sum v, sum v^2 of the defined pixels per label; labels above Z count as 0"""
    v = np.asarray(v).astype(np.int64)
    H, W = v.shape
    lab = cells(zones, H, W, zone_scale).astype(np.int64)
    lab = np.where(lab > Z, 0, lab)
    ok = v != NODATA
    out = np.zeros((Z + 1, 3), np.int64)
    np.add.at(out[:, 0], lab[ok], 1)
    np.add.at(out[:, 1], lab[ok], v[ok])
    np.add.at(out[:, 2], lab[ok], v[ok] * v[ok])
    return out


# ---- the colour ramp: (value, r, g, b) stops, strictly increasing values, integer interpolation --------------------------------------
def ramp_lut(stops):
    """uint8 [65536][4], entry v + 32768: below the first stop its colour, above the last its colour, between two stops
    c0 + round_half_up((c1 - c0) (v - v0) / (v1 - v0)) per channel in integers; alpha 255; entry 0 (nodata) all zero"""
    lut = np.zeros((65536, 4), np.uint8)
    stops = [tuple(int(x) for x in s) for s in stops]
    for v in range(-32767, 32768):
        if v <= stops[0][0]:
            c = stops[0][1:]
        elif v >= stops[-1][0]:
            c = stops[-1][1:]
        else:
            k = max(i for i, s in enumerate(stops) if s[0] <= v)
            (v0, *c0), (v1, *c1) = stops[k], stops[k + 1]
            c = [x0 + ((2 * (x1 - x0) * (v - v0) + (v1 - v0)) // (2 * (v1 - v0))) for x0, x1 in zip(c0, c1)]
        lut[v + 32768] = (*c, 255)
    return lut


# ---- statistics from the histogram -----------------------------------------------------------------------------------------------------
def percentile(h, K, bp):
    """display.py's rule: k = ((n - 1) bp) // 10000, the k-th smallest counted value (0-based)"""
    h = [int(x) for x in h]
    n = sum(h)
    if n == 0:
        return None
    k, run = ((n - 1) * bp) // 10000, 0
    for i, c in enumerate(h):
        run += c
        if run >= k + 1:
            return i - K
    raise AssertionError


def moments(h, K):
    """(count, sum v, sum v^2) in Python integers"""
    n = s = s2 = 0
    for i, c in enumerate(h):
        c, v = int(c), i - K
        n, s, s2 = n + c, s + c * v, s2 + c * v * v
    return n, s, s2


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------------
OUTPUTS = ("index", "hist", "rgba", "zonal")


@functools.lru_cache(maxsize=None)
def case(H, W):
    """(A [H, W, 3], B [H, W, 3], masks and zone grids at scales 1 and 4, the LUT): made once per shape.  The top third of the
    planes lies in 900..1199, so an offset of 1000 takes the d == 0 path there."""
    from s2sr import index as xi
    rng = np.random.default_rng(1000 * H + W)
    A, B = (rng.integers(0, 65536, (H, W, 3)).astype(np.uint16) for _ in range(2))
    top = -(-H // 3)
    A[:top], B[:top] = (rng.integers(900, 1200, (top, W, 3)).astype(np.uint16) for _ in range(2))
    grids = {}
    for s in (1, 4):
        gh, gw = -(-H // s), -(-W // s)
        grids["valid", s] = (rng.random((gh, gw)) > 0.25).astype(np.uint8)
        for Z in (1, 7, 65535):
            pool = np.array([0, 1] if Z == 1 else list(range(8)) + [9] if Z == 7 else [0, 1, 300, 65535], np.uint16)   # 9 > Z = 7: counts as 0
            lab = pool[rng.integers(0, len(pool), (gh, gw))]
            lab[: gh // 2, : gw // 2] = pool[-1] if Z != 7 else 7       # a field: neighbouring lanes share a label
            grids["zones", s, Z] = lab
    return A, B, grids, xi.ramp_lut(xi.ramp_for("vegetation"))


def plane(P3, c, ch):
    """the image as the entry takes it: one channel as a plane of its own (c == 1), or the three-channel image"""
    return np.ascontiguousarray(P3[..., ch]) if c == 1 else P3


def model(a, b, offset, L, K, valid, vs, zones, zs, Z, lut):
    """every output of s2sr_index_nd_u16 as the dict Engine.index_nd_u16 returns"""
    v, und = index(a, b, offset, L, K, valid, vs)
    return {"index": v, "undefined": und, "hist": hist(v, K), "rgba": render(v, lut), "zonal": None if zones is None else zonal(v, zones, zs, Z)}
