"""Management zones restated from their definition (include/s2sr.h: s2sr_zones_kmeans_i16), not from the kernels:
members, field statistics, the start centres on the box's diagonal, Lloyd iterations with exact integer distances and centres
rounded half away from zero, the fixed point, the ranking, the 3 x 3 mode filter and the table, all in numpy int64.  Also the
rasters, label layouts and planted cases the CPU and GPU tests share."""
import functools

import numpy as np

NODATA = -32768
LEVELS = (2000, 5000, 8000)                                        # the planted classes: ten times their noise apart
NOISE = 300
MIXES = {"thirds": (1 / 3, 1 / 3, 1 / 3), "60-30-10": (0.6, 0.3, 0.1), "10-10-80": (0.1, 0.1, 0.8), "5-90-5": (0.05, 0.9, 0.05)}
FEATURES = ("planted", "noise", "constant", "ramp", "nodata", "extremes")
LAYOUTS = ("one", "grid16", "stripes", "checker", "above", "zeros")
# the saturated rasters and the layout of tests/test_gpu_limits.py: +32767 in the upper half of the rows and -32767 in the lower, its
# negative and its half (floor); rows [H / 4, 3 H / 4) as a second field.  They are in no list above: the lists' loops stay what they are.
HALVES = ("halves", "-halves", "halves/2")


# ---- the definition --------------------------------------------------------------------------------------------------------------------
def members(feats, labels, Z):
    """-> (lab with labels above Z as 0, member mask)"""
    lab = np.where(labels <= Z, labels, 0).astype(np.int64)
    return lab, (lab > 0) & (feats != NODATA).all(axis=0)


def assign(V, L, c):
    """the smallest j of the smallest exact squared distance: V int64 [D, M], L [M], c [Z + 1, k, D] -> j [M]"""
    dist = ((V.T[:, None, :] - c[L]) ** 2).sum(axis=2)             # [M, k], below 2^35
    return np.argmin(dist, axis=1)                                 # the first of equal minima


def rounded_mean(s, n):
    """sign(s) ((2 |s| + n) // (2 n)): half away from zero"""
    return np.sign(s) * ((2 * np.abs(s) + n) // (2 * n))


def smooth_pass(zone, lab, k):
    H, W = zone.shape
    zp = np.zeros((H + 2, W + 2), np.int64)
    lp = np.full((H + 2, W + 2), -1, np.int64)                     # outside the image: no label
    zp[1:-1, 1:-1], lp[1:-1, 1:-1] = zone, lab
    votes = np.zeros((k + 1, H, W), np.int64)
    for dy in range(3):
        for dx in range(3):
            z, l = zp[dy:dy + H, dx:dx + W], lp[dy:dy + H, dx:dx + W]
            for j in range(1, k + 1):
                votes[j] += (z == j) & (l == lab)
    most = votes[1:].max(axis=0)
    best = votes[1:].argmax(axis=0) + 1                            # the smallest of the tied ids
    own = np.take_along_axis(votes, zone[None], axis=0)[0]
    return np.where(zone == 0, 0, np.where(own == most, zone, best))


def kmeans(feats, labels, Z, k=3, iters=32, min_per_zone=10, smooth=0):
    """-> {"zone": uint8 [H, W], "table": int64 [Z + 1, k, 1 + 2 D], "centres": int32 [Z + 1, k, D], "status": uint8 [Z + 1],
    "iterations": int}"""
    feats = np.asarray(feats)
    feats = (feats[None] if feats.ndim == 2 else feats).astype(np.int64)
    labels = np.asarray(labels)
    D, H, W = feats.shape
    lab, mem = members(feats, labels, Z)
    L, V = lab[mem], feats[:, mem]
    n = np.bincount(L, minlength=Z + 1)
    lo, hi = np.full((Z + 1, D), 2 ** 40, np.int64), np.full((Z + 1, D), -2 ** 40, np.int64)
    for d in range(D):
        np.minimum.at(lo[:, d], L, V[d])
        np.maximum.at(hi[:, d], L, V[d])
    status = np.where(n == 0, 0, np.where(n < k * min_per_zone, 1, 2)).astype(np.uint8)
    zoned = status == 2
    c = np.zeros((Z + 1, k, D), np.int64)
    for j in range(k):
        c[zoned, j] = lo[zoned] + ((2 * j + 1) * (hi[zoned] - lo[zoned])) // (2 * k)
    keep = zoned[L]
    Lz, Vz = L[keep], V[:, keep]
    iterations = iters
    for t in range(1, iters + 1):
        cell = Lz * k + assign(Vz, Lz, c)
        cnt = np.bincount(cell, minlength=(Z + 1) * k)
        new = c.copy().reshape(-1, D)
        for d in range(D):
            s = np.zeros((Z + 1) * k, np.int64)
            np.add.at(s, cell, Vz[d])
            new[cnt > 0, d] = rounded_mean(s[cnt > 0], cnt[cnt > 0])
        new = new.reshape(c.shape)
        fixed = (new == c).all()
        c = new
        if fixed:                                                  # nothing later changes a byte
            iterations = t
            break
    order = np.argsort(c[:, :, 0], axis=1, kind="stable")           # by (c[j][0], j)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(k)[None].repeat(Z + 1, 0), axis=1)
    centres = np.zeros((Z + 1, k, D), np.int32)
    centres[zoned] = np.take_along_axis(c, order[:, :, None], axis=1)[zoned]
    zone = np.zeros((H, W), np.int64)
    zm = np.zeros(len(L), np.int64)
    zm[keep] = 1 + rank[Lz, assign(Vz, Lz, c)]
    zone[mem] = zm
    for _ in range(smooth):
        zone = smooth_pass(zone, lab, k)
    table = np.zeros((Z + 1, k, 1 + 2 * D), np.int64)
    on = zone > 0
    cell = (lab[on], zone[on] - 1)
    np.add.at(table[:, :, 0], cell, 1)
    for d in range(D):
        np.add.at(table[:, :, 1 + 2 * d], cell, feats[d][on])
        np.add.at(table[:, :, 2 + 2 * d], cell, feats[d][on] ** 2)
    return {"zone": zone.astype(np.uint8), "table": table, "centres": centres, "status": status, "iterations": int(iterations)}


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def planted(shape, mix="thirds", seed=0, D=1):
    """-> (int16 [D, *shape], classes 0..2): LEVELS with uniform noise of +-NOISE, every class at least once, the shares those of
    the mix; further features carry the same levels with noise of their own (the start lies on the box's diagonal, so features that
    rise together are what it is made for)"""
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    counts = [max(1, int(round(p * n))) for p in MIXES[mix][:2]]
    counts.append(max(1, n - sum(counts)))
    cls = np.repeat(np.arange(3), counts)[:n]
    cls = np.concatenate([cls, np.full(n - len(cls), 2)])
    rng.shuffle(cls)
    level = np.array(LEVELS)
    feats = [level[cls] + rng.integers(-NOISE, NOISE + 1, n) for _ in range(D)]
    return np.stack(feats).reshape((D,) + tuple(shape)).astype(np.int16), cls.reshape(shape)


@functools.lru_cache(maxsize=None)
def raster(H, W, name):
    """one int16 feature raster [H, W]"""
    y, x = np.mgrid[0:H, 0:W]
    if name in HALVES:                                             # -32768 is nodata: it does not appear
        f = np.where(y < (H + 1) // 2, 32767, -32767)
        a = (f, -f, f // 2)[HALVES.index(name)].astype(np.int16)
        a.setflags(write=False)
        return a
    rng = np.random.default_rng(1000 * H + 10 * W + FEATURES.index(name))
    if name == "planted":
        a = planted((H, W), "60-30-10", seed=H * 1000 + W)[0][0] if H * W >= 3 else np.full((H, W), 5000)
    elif name == "noise":
        a = rng.integers(-10000, 10001, (H, W))
    elif name == "constant":
        a = np.full((H, W), 1234)
    elif name == "ramp":                                           # rises across the 64-pixel tile lines and the 32-row ones
        a = np.clip(-9000 + 140 * x + 45 * y, -32767, 32767)
    elif name == "nodata":
        a = rng.integers(-3000, 9000, (H, W))
        a[rng.random((H, W)) < 0.1] = NODATA
    elif name == "extremes":
        a = rng.choice(np.array([-32767, 32767, -32767, 32767, -1, 0, 1, 12345]), (H, W))
    else:
        raise KeyError(name)
    a = a.astype(np.int16)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def layout(H, W, name):
    """-> (uint16 labels [H, W], Z)"""
    y, x = np.mgrid[0:H, 0:W]
    grid = 1 + (y // 16) * ((W + 15) // 16) + x // 16
    if name == "one":
        a = np.ones((H, W))
    elif name == "grid16":
        a = grid
    elif name == "stripes":                                        # a label change inside every group of 8 pixels
        a = 1 + x % 5
    elif name == "checker":
        a = 1 + (x + y) % 2
    elif name == "above":                                          # the upper half of the numbers lies above Z
        a = grid * 3
    elif name == "zeros":
        a = np.zeros((H, W))
    elif name == "middle":                                         # a label change at H / 4 and at 3 H / 4, in every column
        a = 1 + ((y >= H // 4) & (y < 3 * H // 4))
    elif name == "late":                                           # the same, the first change 96 rows (3 tiles) later
        a = 1 + ((y >= H // 4 + 96) & (y < 3 * H // 4))
    else:
        raise KeyError(name)
    a = a.astype(np.uint16)
    a.setflags(write=False)
    Z = max(1, int(a.max()) // 2) if name == "above" else max(1, int(a.max()))
    return a, Z


# ---- the walk's geometry (csrc/mzones.hip) -----------------------------------------------------------------------------------------------
TILE_W, TILE_H, WAVE_PIXELS = 64, 32, 512                          # a tile; the pixels of a tile that one wave takes (8 rows of 64)
MOST_BLOCKS, PENDING = 2048, 65000                                 # kMostBlocks; the pixels a wave's int32 pending sums may hold


def pending_reach(H, W, cap=None):
    """One column of tiles (W <= 64) of a raster whose rows change value at H / 2: the workgroups, the longest run of tiles of one
    workgroup inside one half, the pixels a wave meets on it, and the magnitude its sum of +-32767 would reach without the flush"""
    assert W <= TILE_W
    ntiles = -(-H // TILE_H)
    grid = min(ntiles, MOST_BLOCKS if cap is None else cap)
    per = -(-ntiles // grid)
    run_tiles = min(ntiles // 2, per)
    return {"ntiles": ntiles, "grid": grid, "run_tiles": run_tiles, "pixels": run_tiles * WAVE_PIXELS, "sum": run_tiles * WAVE_PIXELS * 32767}


def inputs(H, W, features, lay):
    """-> (int16 [D, H, W], uint16 labels, Z); features: a name or a tuple of names"""
    names = (features,) if isinstance(features, str) else tuple(features)
    labels, Z = layout(H, W, lay)
    return np.stack([raster(H, W, n) for n in names]), labels, Z


@functools.lru_cache(maxsize=None)
def _case(H, W, features, lay, Z, kw):
    feats, labels, Z0 = inputs(H, W, features, lay)
    return kmeans(feats, labels, Z0 if Z is None else Z, **dict(kw))


def case(H, W, features, lay, Z=None, **kw):
    """the model's outputs for a named case, computed once per process and left unchanged"""
    features = (features,) if isinstance(features, str) else tuple(features)
    return _case(H, W, features, lay, Z, tuple(sorted(kw.items())))
