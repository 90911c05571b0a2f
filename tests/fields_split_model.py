"""The touching-fields split restated from its definition (include/s2sr.h: s2sr_fields_split_i16), not from the
kernels: the mask and the components are tests/fields_model.py's; the interior by shifted sums, the squared distance by a search
over every row for the nearest outside pixel, the cores per component, the growth breadth-first, level by level, with the smallest
key per level.  Also the rasters the CPU and GPU tests share."""
import functools

import numpy as np

import fields_model as fm
from fields_model import HI, LO, NODATA

CAP = 255
DEGENERATE = {"core_q": 1, "core_px": 0, "edge": 0, "edge_r": 0}
DEFAULT = {"core_q": 500, "core_px": 2, "edge": 0, "edge_r": 1}


# ---- the definition --------------------------------------------------------------------------------------------------------------------------
def _shift(a, dy, dx, fill):
    """a[y + dy, x + dx], `fill` (an array like a, or a scalar) where that lies outside the image"""
    H, W = a.shape
    out = np.array(np.broadcast_to(fill, a.shape), dtype=a.dtype)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    yt, xt = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    out[ys, xs] = a[yt, xt]
    return out


def gradient2(idx, r):
    """gx^2 + gy^2 of step 2 in int64 (meaningless on nodata pixels, which no mask holds)"""
    v = np.asarray(idx).astype(np.int64)
    data = np.asarray(idx) != NODATA
    B = np.zeros_like(v)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            B += np.where(_shift(data, dy, dx, False), _shift(v, dy, dx, 0), v)
    nb = lambda dy, dx: np.where(_shift(data, dy, dx, False), _shift(B, dy, dx, 0), B)
    gx = (nb(-1, 1) + 2 * nb(0, 1) + nb(1, 1)) - (nb(-1, -1) + 2 * nb(0, -1) + nb(1, -1))
    gy = (nb(1, -1) + 2 * nb(1, 0) + nb(1, 1)) - (nb(-1, -1) + 2 * nb(-1, 0) + nb(-1, 1))
    return gx * gx + gy * gy


def interior(idx, m, edge, edge_r):
    if not edge:
        return m.copy()
    n = (2 * edge_r + 1) ** 2
    return m & ~(gradient2(idx, edge_r) > (8 * n * edge) ** 2)


def distance2(I):
    """min(255^2, the squared distance to the nearest pixel of the image outside I) on I, 0 elsewhere: for every row the horizontal
    distance to that row's nearest outside pixel, then the minimum over all rows"""
    H, W = I.shape
    far = 1 << 20
    xs = np.arange(W)
    left = np.maximum.accumulate(np.where(~I, xs, -far), axis=1)
    right = np.minimum.accumulate(np.where(~I, xs, far)[:, ::-1], axis=1)[:, ::-1]
    h = np.minimum(xs - left, right - xs).astype(np.int64)          # >= far - W: the row holds no outside pixel
    D = np.full((H, W), CAP * CAP, np.int64)
    for y in range(H):
        dy = (np.arange(H) - y).astype(np.int64)[:, None]
        D = np.minimum(D, dy * dy + (h[y] * h[y])[None, :])
    return np.where(I, D, 0)


def core_pixels(I, D, conn, core_q, core_px):
    core = np.zeros(I.shape, bool)
    flat = core.reshape(-1)
    for _, pixels in fm.components(I, conn):
        p = np.array(pixels)
        d = D.reshape(-1)[p]
        top = int(d.max())
        if top < core_px * core_px:
            flat[p] = True
        else:
            flat[p] = (d >= core_px * core_px) & (1000000 * d >= core_q * core_q * top)
    return core


def grow(domain, owner, conn):
    """owner: int64, -1 = nobody.  Level by level every pixel of `domain` without an owner that touches an owned pixel takes the
    smallest key among its owned neighbours (they all joined on the level before); until a level adds nothing.  -> levels"""
    H, W = domain.shape
    near = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    own = owner.reshape(-1)
    dom = domain.reshape(-1)
    front = np.flatnonzero(own >= 0)
    levels = 0
    while len(front):
        fy, fx = front // W, front % W
        tp, tk = [], []
        for dy, dx in near:
            ny, nx = fy + dy, fx + dx
            ok = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
            q = (ny * W + nx)[ok]
            take = dom[q] & (own[q] < 0)
            tp.append(q[take])
            tk.append(own[front[ok]][take])
        tp, tk = np.concatenate(tp), np.concatenate(tk)
        if not len(tp):
            break
        best = np.full(H * W, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(best, tp, tk)
        front = np.unique(tp)
        own[front] = best[front]
        levels += 1
    return levels


def split(idx, lo, hi, r_open=0, r_close=0, conn=4, min_pixels=1, Z=65535, split=None):
    """-> {"labels" uint16 [H, W], "fields" int64 [Z + 1][6], "found", "dist2" uint16 [H, W], "cores" uint8 [H, W], "levels": the
    levels the two growths took}; split None: fields_model.segment (dist2 and cores zeros)"""
    idx = np.asarray(idx)
    H, W = idx.shape
    if split is None:
        labels, fields, found = fm.segment(idx, lo, hi, r_open, r_close, conn, min_pixels, Z)
        return {"labels": labels, "fields": fields, "found": found, "dist2": np.zeros((H, W), np.uint16), "cores": np.zeros((H, W), np.uint8), "levels": (0, 0)}
    sp = dict(DEFAULT, **split)
    m = fm.cleaned(idx, lo, hi, r_open, r_close)
    I = interior(idx, m, sp["edge"], sp["edge_r"])
    D = distance2(I)
    core = core_pixels(I, D, conn, sp["core_q"], sp["core_px"])
    owner = np.full((H, W), -1, np.int64)
    for key, pixels in fm.components(core, conn):
        owner.reshape(-1)[pixels] = key
    inside = grow(I, owner, conn)
    assert (owner[I] >= 0).all()                                   # every component of I holds a core
    over = grow(m & ~I, owner, conn)                               # the owned pixels are I's: the paths start there
    own = owner.reshape(-1)
    order = np.argsort(own, kind="stable")                         # by owner, then by linear index
    order = order[own[order] >= 0]
    starts = np.flatnonzero(np.diff(own[order], prepend=-1))
    regions = sorted((int(order[a]), order[a:b]) for a, b in zip(starts, list(starts[1:]) + [len(order)]))
    labels = np.zeros(H * W, np.uint16)
    fields = np.zeros((Z + 1, 6), np.int64)
    found = 0
    for key, p in regions:
        if len(p) < min_pixels:
            continue
        found += 1
        if found > Z:
            continue
        labels[p] = found
        fields[found] = len(p), key, (p % W).min(), (p // W).min(), (p % W).max() + 1, (p // W).max() + 1
    fields[0, 0] = H * W - int(fields[1:, 0].sum())
    return {"labels": labels.reshape(H, W), "fields": fields, "found": found, "dist2": D.astype(np.uint16), "cores": core.astype(np.uint8),
            "levels": (inside, over)}


# ---- rasters -----------------------------------------------------------------------------------------------------------------------------------
def dumbbell(sep, R1, R2):
    """two discs on 40 x 64, centres (20, 16) and (20, 16 + sep)"""
    yy, xx = np.mgrid[0:40, 0:64]
    return fm.as_index(((yy - 20) ** 2 + (xx - 16) ** 2 <= R1 * R1) | ((yy - 20) ** 2 + (xx - 16 - sep) ** 2 <= R2 * R2))


PARCEL_VALUES = ((5000, 7000, 5600), (6800, 5200, 7400))


def parcels():
    """-> (index raster, planted labels): a 2 x 3 grid of touching 32 x 40 rectangles of different values, noise of +-60, on 70 x 130"""
    rng = np.random.default_rng(3)
    idx = np.full((70, 130), 1000, np.int16)
    planted = np.zeros((70, 130), np.uint16)
    for i in range(2):
        for j in range(3):
            idx[3 + 32 * i:35 + 32 * i, 5 + 40 * j:45 + 40 * j] = PARCEL_VALUES[i][j]
            planted[3 + 32 * i:35 + 32 * i, 5 + 40 * j:45 + 40 * j] = 3 * i + j + 1
    return (idx + rng.integers(-60, 61, idx.shape)).astype(np.int16), planted


def snake(H, W, rooms=2):
    """a 9 x 9 room in the top-left corner, a one-pixel corridor that leaves it downwards and runs to and fro over every second row
    of the raster, and with rooms == 2 a second 9 x 9 room where it ends.  A raster too small for that is a corridor on row 0."""
    m = np.zeros((H, W), bool)
    last = H - 1 - (10 if rooms == 2 else 0)                       # the last row a corridor may take
    if W < 11 or last < 10:
        m[0, :] = True
        return m
    m[0:9, 0:9] = True
    m[9, 0] = True
    at_right = False                                               # where the corridor stands: it starts at column 0
    r = 10
    while True:
        m[r, :] = True
        at_right = not at_right
        if r + 2 > last:
            break
        m[r + 1, W - 1 if at_right else 0] = True
        r += 2
    if rooms == 2:
        c = W - 1 if at_right else 0
        m[r + 1, c] = True
        m[r + 2:r + 11, (c - 8 if at_right else 0):(c + 1 if at_right else 9)] = True
    return m


def edge_only(H, W):
    """a 2-pixel strip of 9000 on a ground of 1000: under an edge test of T 150 every pixel of it is an edge pixel, so nothing
    reaches it; beside it a block of 5000 whose rim is edge pixels that the growth wins back"""
    idx = np.full((H, W), 1000, np.int16)
    idx[1:max(H - 1, 2), 1:3] = 9000
    idx[2:max(H - 2, 3), 6:max(W - 3, 7)] = 5000
    return idx


NEW = ("dumbbell", "parcels", "snake", "snake1", "edge-only")


@functools.lru_cache(maxsize=None)
def _new(H, W):
    """the new rasters at H x W: the fixed-size ones cut or padded (ground 1000) to the shape"""
    def fit(a):
        out = np.full((H, W), 1000, np.int16)
        h, w = min(H, a.shape[0]), min(W, a.shape[1])
        out[:h, :w] = a[:h, :w]
        return out
    out = {"dumbbell": fit(dumbbell(16, 12, 7)), "parcels": fit(parcels()[0]), "snake": fm.as_index(snake(H, W, 2)), "snake1": fm.as_index(snake(H, W, 1)),
           "edge-only": edge_only(H, W)}
    for v in out.values():
        v.setflags(write=False)
    return out


def raster(H, W, name):
    return _new(H, W)[name] if name in NEW else fm.raster(H, W, name)


_CASES = {}


def case(H, W, name, split=None, **kw):
    """split() of raster(H, W, name) in LO..HI: made once per raster and parameter set, read-only"""
    key = (H, W, name, None if split is None else tuple(sorted(split.items())), tuple(sorted(kw.items())))
    if key not in _CASES:
        out = globals()["split"](raster(H, W, name), LO, HI, split=split, **kw)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[key] = out
    return _CASES[key]


def notched(H=300, W=600, both=False):
    """a solid rectangle wider than 510 pixels over every row, with one notch cut in from the top: D2 reaches the cap in its middle;
    both: a second notch from the bottom, so that pixels also find their nearest outside pixel below them"""
    m = np.zeros((H, W), bool)
    m[:, 20:W - 20] = True
    m[0:21, 300:303] = False
    if both:
        m[H - 21:H, 296:299] = False
    return fm.as_index(m)


SATURATED = (-32767, 32767)                                        # lo, hi of the saturated rasters: every pixel is in the mask
SATURATED_SPLITS = ({"edge": 32767, "edge_r": 4}, {"edge": 1, "edge_r": 4}, {"edge": 32767, "edge_r": 0}, {"edge": 16000, "edge_r": 2})


def saturated(H, W, cell):
    """+32767 and -32767 in a checkerboard of cell x cell pixels: the box sums of the edge test reach +-(2 r + 1)^2 * 32767 where a
    window lies inside a cell, and the Sobel sums of them their largest differences"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy // cell + xx // cell) % 2 == 0, 32767, -32767).astype(np.int16)


_SATURATED = {}


def saturated_case(H, W, cell, split, **kw):
    """split() of saturated(H, W, cell) in SATURATED: made once per raster and parameter set, read-only"""
    key = (H, W, cell, tuple(sorted(split.items())), tuple(sorted(kw.items())))
    if key not in _SATURATED:
        out = globals()["split"](saturated(H, W, cell), *SATURATED, split=split, **kw)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SATURATED[key] = out
    return _SATURATED[key]


# ---- the distance's geometry (csrc/fields_split.hip: kBand rows a thread of the column pass, kSeg pixels a workgroup of the row pass) -------
BAND, SEG = 256, 256


def band_reach(I, dist2, band=1):
    """On the rows [ya, yb) of one band of the column pass: the pixels of I at the cap and below it; among the latter those whose D2
    exceeds the squared distance to the row before the band (above) or to the row behind it (below), so that no pixel of the band's
    own rows straight above or below them is the nearest one; and those for which the band's rows alone give a larger distance
    (other): their nearest outside pixel lies in another band, whichever way one looks."""
    H = dist2.shape[0]
    ya, yb = band * BAND, min((band + 1) * BAND, H)
    d = dist2[ya:yb].astype(np.int64)
    rows = np.arange(ya, yb)[:, None]
    open_ = (d > 0) & (d < CAP * CAP)
    alone = distance2(np.asarray(I)[ya:yb])
    return {"rows": (ya, yb), "capped": int((d == CAP * CAP).sum()), "uncapped": int(open_.sum()),
            "above": int((open_ & (d > (rows - ya + 1) ** 2)).sum()), "below": int((open_ & (d > (yb - rows) ** 2)).sum()),
            "other": int((open_ & (alone > d)).sum())}
