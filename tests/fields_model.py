"""The fields pass restated from its definition (include/s2sr.h: s2sr_fields_segment_i16, s2sr_labels_trace_u16), not
from the kernels: the mask, the morphology by shifted ANDs and ORs, the components by a plain flood fill, the numbering, the fields
table, and the ring tracer's rule edge by edge.  Also the rasters the CPU and GPU tests share."""
import functools
from collections import deque

import numpy as np

NODATA = -32768


# ---- the segmentation ------------------------------------------------------------------------------------------------------------------
def mask(idx, lo, hi):
    idx = np.asarray(idx)
    return (idx != NODATA) & (idx >= lo) & (idx <= hi)


def _shifted(m, r, outside):
    """the (2 r + 1)^2 shifts of m, with `outside` where a shift looks beyond the image"""
    H, W = m.shape
    p = np.full((H + 2 * r, W + 2 * r), outside, bool)
    p[r:r + H, r:r + W] = m
    return [p[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)]


def erode(m, r):
    """the AND over the neighbours inside the image: what lies outside is neutral, True"""
    return np.logical_and.reduce(_shifted(m, r, True))


def dilate(m, r):
    return np.logical_or.reduce(_shifted(m, r, False))


def cleaned(idx, lo, hi, r_open=0, r_close=0):
    m = mask(idx, lo, hi)
    m = dilate(erode(m, r_open), r_open)
    m = erode(dilate(m, r_close), r_close)
    return m & (np.asarray(idx) != NODATA)


def components(m, conn):
    """[(key, [linear indices])] by ascending key: a flood fill from every pixel not yet reached, in linear order"""
    H, W = m.shape
    near = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    seen = np.zeros((H, W), bool)
    out = []
    for y, x in zip(*np.nonzero(m)):
        if seen[y, x]:
            continue
        seen[y, x] = True
        todo, got = deque([(int(y), int(x))]), []
        while todo:
            cy, cx = todo.popleft()
            got.append(cy * W + cx)
            for dy, dx in near:
                ny, nx = cy + dy, cx + dx
                if 0 <= ny < H and 0 <= nx < W and m[ny, nx] and not seen[ny, nx]:
                    seen[ny, nx] = True
                    todo.append((ny, nx))
        out.append((min(got), got))
    return sorted(out)


def segment(idx, lo, hi, r_open=0, r_close=0, conn=4, min_pixels=1, Z=65535):
    """-> labels uint16 [H, W], fields int64 [Z + 1][6] (pixels, key, x0, y0, x1, y1), found"""
    idx = np.asarray(idx)
    H, W = idx.shape
    labels = np.zeros(H * W, np.uint16)
    fields = np.zeros((Z + 1, 6), np.int64)
    found = 0
    for key, pixels in components(cleaned(idx, lo, hi, r_open, r_close), conn):
        if len(pixels) < min_pixels:
            continue
        found += 1
        if found > Z:
            continue
        p = np.array(pixels)
        labels[p] = found
        fields[found] = len(p), key, (p % W).min(), (p // W).min(), (p % W).max() + 1, (p // W).max() + 1
    fields[0, 0] = H * W - int(fields[1:, 0].sum())
    return labels.reshape(H, W), fields, found


# ---- the rings ---------------------------------------------------------------------------------------------------------------------------
_STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))                       # down, right, up, left in (dx, dy); the next one is the left turn


def trace(labels, Z):
    """-> xy int32 [V, 2] (pixel corners x, y), ring_start int32 [R + 1], ring_label uint16 [R]"""
    labels = np.asarray(labels)
    H, W = labels.shape
    p = np.zeros((H + 2, W + 2), np.int64)
    p[1:-1, 1:-1] = labels
    rings = []
    for l in [int(v) for v in np.unique(labels) if 1 <= v <= Z]:
        own = p == l
        # the directed unit edges with l on their left: {(corner, direction)}
        edges = set()
        for d, (ny, nx) in enumerate(((0, -1), (1, 0), (0, 1), (-1, 0))):            # the neighbour across the left, bottom, right, top side
            other = np.zeros_like(own)
            other[1:-1, 1:-1] = own[1 + ny:H + 1 + ny, 1 + nx:W + 1 + nx]
            for r, c in zip(*np.nonzero(own & ~other)):
                r, c = int(r) - 1, int(c) - 1
                edges.add((((c, r), (c, r + 1), (c + 1, r + 1), (c + 1, r))[d], d))    # where the side's edge starts
        while edges:
            first = min(edges, key=lambda e: (e[0][1], e[0][0], e[1]))
            (x, y), d = first
            ring = []
            while True:
                edges.discard(((x, y), d))
                x, y = x + _STEP[d][0], y + _STEP[d][1]
                for nd in ((d + 1) % 4, d, (d + 3) % 4):                               # left, straight on, right
                    if ((x, y), nd) in edges or ((x, y), nd) == first:
                        break
                else:
                    raise AssertionError("an open boundary")
                if nd != d:
                    ring.append((x, y))
                d = nd
                if ((x, y), d) == first:
                    break
            k = min(range(len(ring)), key=lambda i: (ring[i][1], ring[i][0]))
            ring = ring[k:] + ring[:k]
            rings.append((l, ring[0][1], ring[0][0], ring))
    rings.sort(key=lambda g: g[:3])
    xy = np.array([v for g in rings for v in g[3]], np.int32).reshape(-1, 2)
    ring_start = np.cumsum([0] + [len(g[3]) for g in rings]).astype(np.int32)
    return xy, ring_start, np.array([g[0] for g in rings], np.uint16)


def ring_area2(ring):
    """twice the signed area in (x, y) with y down: negative for a ring that runs counterclockwise on a north-up map"""
    ring = np.asarray(ring, np.int64)
    x, y = ring[:, 0], ring[:, 1]
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


# ---- rasters -----------------------------------------------------------------------------------------------------------------------------
def as_index(m, nodata=None):
    """a boolean pattern as an index raster: 5000 where set, 1000 elsewhere, -32768 where `nodata` is set"""
    idx = np.where(m, 5000, 1000).astype(np.int16)
    if nodata is not None:
        idx[nodata] = NODATA
    return idx


def spiral(H, W):
    """a one-pixel path that winds inwards from the top-left corner with one pixel of background between its turns: it walks on
    while the pixel ahead is free and the one behind that is too, and turns right otherwise"""
    m = np.zeros((H, W), bool)
    free = lambda y, x: not (0 <= y < H and 0 <= x < W) or not m[y, x]
    y, x, d = 0, 0, 0
    m[0, 0] = True
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))
    turned = 0
    while turned < 2:
        dy, dx = steps[d]
        if 0 <= y + dy < H and 0 <= x + dx < W and free(y + dy, x + dx) and free(y + 2 * dy, x + 2 * dx):
            y, x, turned = y + dy, x + dx, 0
            m[y, x] = True
        else:
            d, turned = (d + 1) % 4, turned + 1
    return m


def patterns(H, W, seed=7):
    """name -> index raster: the shapes that break a union-find, fields on every edge, nodata"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = {}
    out["spiral"] = as_index(spiral(H, W))
    out["checker"] = as_index((yy + xx) % 2 == 0)
    out["comb"] = as_index((yy == H - 1) | ((xx % 2 == 0) & (yy < H - 1)) if H > 1 else xx % 2 == 0)
    out["rings"] = as_index(np.maximum(np.abs(yy - H // 2), np.abs(xx - W // 2)) % 3 == 0)
    out["noise"] = rng.integers(-2000, 10001, (H, W)).astype(np.int16)                 # about half above 4000
    out["ones"] = as_index(np.ones((H, W), bool))
    out["zeros"] = as_index(np.zeros((H, W), bool))
    out["stripes"] = as_index(np.ones((H, W), bool), nodata=(xx % 7 == 3) | (yy % 11 == 5))
    # blobs that touch every edge, speckle, pinholes and nodata inside a field: what the morphology is for
    blobs = ((yy // 9 + xx // 13) % 2 == 0) & (rng.random((H, W)) > 0.06) | (rng.random((H, W)) > 0.97)
    out["blobs"] = as_index(blobs, nodata=rng.random((H, W)) > 0.985)
    return out


def trace_rasters():
    """name -> uint16 labels: holes, a hole's island, diagonal contacts, labels on the border, one pixel"""
    out = {"one": np.array([[1]], np.uint16), "none": np.zeros((3, 4), np.uint16)}
    a = np.zeros((9, 11), np.uint16)
    a[1:8, 1:9] = 1
    a[3:6, 3:7] = 0                                                # a hole
    a[4, 4] = 2                                                    # with an island of another label
    a[0, 10] = 3
    out["hole"] = a
    b = np.zeros((6, 6), np.uint16)
    for i in range(5):
        b[i, i] = 1                                                # a diagonal chain: five rings of label 1 that touch
    b[0, 5] = b[1, 4] = 2
    b[4, 0] = b[5, 1] = b[5, 0] = 2
    out["diagonal"] = b
    c = np.ones((5, 7), np.uint16)                                 # the whole raster, with two holes that touch at a corner
    c[1, 1] = c[2, 2] = 0
    c[3, 4:6] = 5
    out["border"] = c
    d = np.zeros((8, 8), np.uint16)
    d[1:7, 1:7] = 4
    d[2:4, 2:4] = 0
    d[4:6, 4:6] = 0                                                # two holes that meet diagonally inside one label
    d[0, 0] = 70                                                   # above Z in the tests that trace with Z = 9
    out["pinch"] = d
    rng = np.random.default_rng(5)
    out["random"] = rng.integers(0, 4, (13, 17)).astype(np.uint16)
    return out


# ---- the numbering's geometry --------------------------------------------------------------------------------------------------------------
CHUNK, TURN = 1024, 256                                            # csrc/fields.hip: kChunk pixels a chunk; the scan walks 256 chunks a turn


def scan_reach(keys, H, W):
    """Where the keys of the numbered fields fall in the numbering scan (csrc/fields.hip fields_scan_kernel): the number of chunks and
    of turns, the turns that hold a key, the keys in the last chunk of the first turn and in the first of the second, and the carry
    each turn starts with (the fields numbered before it)."""
    keys = np.sort(np.asarray(keys, np.int64))
    chunks = -(-H * W // CHUNK)
    turns = -(-chunks // TURN)
    turn = keys // (TURN * CHUNK)
    return {"chunks": chunks, "turns": turns, "met": sorted(set(turn.tolist())), "in255": int((keys // CHUNK == TURN - 1).sum()),
            "in256": int((keys // CHUNK == TURN).sum()), "carry": [int((turn < t).sum()) for t in range(turns)]}


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------------
LO, HI = 4000, 32767


@functools.lru_cache(maxsize=None)
def _patterns(H, W):
    out = patterns(H, W)
    for v in out.values():
        v.setflags(write=False)
    return out


def raster(H, W, name):
    return _patterns(H, W)[name]


_CASES = {}


def case(H, W, name, **kw):
    """segment() of raster(H, W, name) in LO..HI -> (labels, fields, found): made once per raster and parameter set"""
    key = (H, W, name, tuple(sorted(kw.items())))
    if key not in _CASES:
        labels, fields, found = segment(raster(H, W, name), LO, HI, **kw)
        labels.setflags(write=False)
        fields.setflags(write=False)
        _CASES[key] = labels, fields, found
    return _CASES[key]
