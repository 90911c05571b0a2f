"""The polygon rasteriser's definition (include/s2sr.h s2sr_zones_rasterize_u16) in numpy int64 and in Python
integers, independent of csrc/: the per-pixel rule, the per-row k form, burn order with `area`, the candidate sets of the tile
bins (csrc/zone_bins.h), and the scenes the CPU and GPU tests share.

  coordinates: int32 in 1/256 of a label pixel; the centre of pixel (r, c) is (cx, cy) = (256 c + 128, 256 r + 128)
  an edge with its endpoints exchanged so that ya < yb (ya == yb never counts) counts for a centre iff
      ya <= cy < yb  and  (cx - xa) (yb - ya) < (xb - xa) (cy - ya)
  a centre is inside a feature iff the count over all edges of all its rings is odd; the latest feature of the list wins.

A feature here is (rings, label); a ring is a list of (x, y) vertices, the edge last -> first implied."""
import functools

import numpy as np

SUB = 256
TILE = 64
COORD_MAX = 2 ** 29


def edges(ring):
    """the ring's edges as (xa, ya, xb, yb) with ya < yb; horizontal ones left out"""
    out = []
    for (px, py), (qx, qy) in zip(ring, list(ring[1:]) + [ring[0]]):
        if py == qy:
            continue
        out.append((px, py, qx, qy) if py < qy else (qx, qy, px, py))
    return out


def inside_pixels(rings, H, W):
    """the per-pixel rule, int64: bool [H, W]"""
    cx = (SUB * np.arange(W, dtype=np.int64) + SUB // 2)[None, :]
    cy = (SUB * np.arange(H, dtype=np.int64) + SUB // 2)[:, None]
    odd = np.zeros((H, W), bool)
    for ring in rings:
        for xa, ya, xb, yb in edges(ring):
            odd ^= (ya <= cy) & (cy < yb) & ((cx - xa) * (yb - ya) < (xb - xa) * (cy - ya))
    return odd


def inside_rows(rings, H, W):
    """the per-row form: an edge toggles the columns c < k = clamp(ceil(N / (256 dy)), 0, W) of every row it crosses"""
    cy = SUB * np.arange(H, dtype=np.int64) + SUB // 2
    flips = np.zeros((H, W + 1), np.int64)
    for ring in rings:
        for xa, ya, xb, yb in edges(ring):
            rows = np.nonzero((ya <= cy) & (cy < yb))[0]
            dy = yb - ya
            N = (xb - xa) * (cy[rows] - ya) + (xa - SUB // 2) * dy
            k = np.clip(-((-N) // (SUB * dy)), 0, W)
            np.add.at(flips, (rows, np.zeros_like(rows)), 1)
            np.add.at(flips, (rows, k), -1)
    return (np.cumsum(flips, axis=1)[:, :W] & 1).astype(bool)


def inside_python(rings, r, c):
    """one centre in Python integers; also returns the largest magnitude any product or sum of the rule took"""
    cx, cy, count, big = SUB * c + SUB // 2, SUB * r + SUB // 2, 0, 0
    for ring in rings:
        for xa, ya, xb, yb in edges(ring):
            lhs, rhs = (cx - xa) * (yb - ya), (xb - xa) * (cy - ya)
            N = rhs + (xa - SUB // 2) * (yb - ya)
            big = max(big, abs(lhs), abs(rhs), abs(N), abs(SUB * c * (yb - ya)))
            count += ya <= cy < yb and lhs < rhs
    return count & 1 == 1, big


def rasterize(features, Z, H, W, inside=inside_pixels):
    """(uint16 labels [H, W], uint64 area [Z + 1]): burn order, the later feature wins"""
    out = np.zeros((H, W), np.uint16)
    for rings, label in features:
        assert 1 <= label <= Z
        out[inside(rings, H, W)] = label
    return out, np.bincount(out.ravel(), minlength=Z + 1).astype(np.uint64)


def tables(features):
    """features -> (xy int32 [V, 2], ring_start int32 [R + 1], feat_start int32 [F + 1], label uint16 [F])"""
    xy, ring_start, feat_start, label = [], [0], [0], []
    for rings, lab in features:
        for ring in rings:
            xy += [tuple(v) for v in ring]
            ring_start.append(len(xy))
        feat_start.append(len(ring_start) - 1)
        label.append(lab)
    return (np.array(xy, np.int32).reshape(-1, 2), np.array(ring_start, np.int32), np.array(feat_start, np.int32), np.array(label, np.uint16))


def from_tables(xy, ring_start, feat_start, label):
    """the tables back as features"""
    xy = np.asarray(xy).tolist()
    return [([[tuple(v) for v in xy[ring_start[r]:ring_start[r + 1]]] for r in range(feat_start[f], feat_start[f + 1])], int(label[f]))
            for f in range(len(label))]


def bins(features, H, W):
    """the candidate sets of csrc/zone_bins.h: per tile (row-major) the ascending features whose closed bounding box meets the
    tile's half-open square of 16384 units, and the number of features that meet no tile"""
    tx, ty = -(-W // TILE), -(-H // TILE)
    U = TILE * SUB
    sets, dropped = [[] for _ in range(tx * ty)], 0
    for f, (rings, _) in enumerate(features):
        pts = [v for ring in rings for v in ring]
        hit = False
        if pts:
            xmin, xmax = min(p[0] for p in pts), max(p[0] for p in pts)
            ymin, ymax = min(p[1] for p in pts), max(p[1] for p in pts)
            for j in range(ty):
                for i in range(tx):
                    if xmax >= U * i and xmin < U * (i + 1) and ymax >= U * j and ymin < U * (j + 1):
                        sets[j * tx + i].append(f)
                        hit = True
        dropped += not hit
    return sets, dropped


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def _orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def mesh(H, W, n=7, seed=0):
    """A jittered mesh of 2 n n triangles with shared vertices that reaches past every side of the grid.  Where the mesh stays a
    triangulation (no triangle turns over) vertices are moved onto pixel centres, one horizontal edge is laid through the centres
    of a row and one vertical edge through the centres of a column.  -> (triangles as rings, the vertex grid)"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    m = 300
    x_lo, x_hi, y_lo, y_hi = -m, SUB * W + m, -m, SUB * H + m
    sx, sy = (x_hi - x_lo) // n, (y_hi - y_lo) // n
    P = {}
    for j in range(n + 1):
        for i in range(n + 1):
            x = x_lo + i * sx if i < n else x_hi
            y = y_lo + j * sy if j < n else y_hi
            if 0 < i < n:
                x += int(rng.integers(-(sx // 4), sx // 4 + 1))
            if 0 < j < n:
                y += int(rng.integers(-(sy // 4), sy // 4 + 1))
            P[i, j] = (x, y)

    def tris_of(Q):
        out = []
        for j in range(n):
            for i in range(n):
                a, b, c, d = Q[i, j], Q[i + 1, j], Q[i + 1, j + 1], Q[i, j + 1]
                out += [[a, b, c], [a, c, d]] if (i + j) & 1 else [[a, b, d], [b, c, d]]
        return out

    def valid(Q):
        return all(_orient(*t) > 0 for t in tris_of(Q))

    assert valid(P)
    centre = lambda v: SUB * (v // SUB) + SUB // 2                                    # the centre of the pixel that holds v

    def attempt(changes):
        Q = dict(P)
        Q.update(changes)
        if valid(Q):
            P.update(changes)

    for i, j in ((3, 3), (2, 5), (5, 2), (4, 4)):                                    # vertices onto pixel centres
        x, y = P[i, j]
        attempt({(i, j): (min(max(centre(x), SUB // 2), SUB * W - SUB // 2), min(max(centre(y), SUB // 2), SUB * H - SUB // 2))})
    y = min(max(centre(P[2, 4][1]), SUB // 2), SUB * H - SUB // 2)                    # a horizontal edge through a row's centres
    attempt({(2, 4): (P[2, 4][0], y), (3, 4): (P[3, 4][0], y)})
    x = min(max(centre(P[5, 3][0]), SUB // 2), SUB * W - SUB // 2)                    # a vertical edge through a column's centres
    attempt({(5, 3): (x, P[5, 3][1]), (5, 4): (x, P[5, 4][1])})
    return tris_of(P), P


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def scene(H, W):
    """The features of one shape, in burn order: a polygon around everything, the mesh, a sliver of a triangle with vertices at
    +-2^29 that crosses the grid, a polygon with two holes (one in each winding), a MultiPolygon with a part inside the first
    hole, overlapping rectangles of which two share a label, a bow-tie, and a polygon wholly outside.  -> (features, Z)"""
    w, h = SUB * W, SUB * H
    B = COORD_MAX
    feats = [([rect(-5000, -7000, w + 9000, h + 3000)], 200)]
    feats += [([t], 1 + k) for k, t in enumerate(mesh(H, W)[0])]
    feats.append(([[(-B, -B), (B, B), (B, B - 2 ** 21)]], 150))
    # the outer ring in thirds of the grid, the holes inside it
    ox0, oy0, ox1, oy1 = w // 8, h // 8, w - w // 8 + 77, h - h // 8 + 31
    hole_a = rect(ox0 + (ox1 - ox0) // 8, oy0 + (oy1 - oy0) // 8, ox0 + (ox1 - ox0) // 2, oy0 + (oy1 - oy0) // 2)
    hole_b = rect(ox0 + 5 * (ox1 - ox0) // 8, oy0 + 5 * (oy1 - oy0) // 8, ox0 + 7 * (ox1 - ox0) // 8, oy0 + 7 * (oy1 - oy0) // 8)[::-1]
    feats.append(([rect(ox0, oy0, ox1, oy1), hole_a, hole_b], 120))
    ax0, ay0, ax1, ay1 = hole_a[0][0], hole_a[0][1], hole_a[2][0], hole_a[2][1]
    part_in = [(ax0 + (ax1 - ax0) // 4, ay0 + (ay1 - ay0) // 4), (ax1 - (ax1 - ax0) // 5, ay0 + (ay1 - ay0) // 3), ((ax0 + ax1) // 2, ay1 - (ay1 - ay0) // 6)]
    part_out = [(w - w // 5, -300), (w + 500, h // 3), (w - w // 4, h // 4)]
    feats.append(([part_in, part_out], 121))
    feats.append(([rect(w // 3, h // 2, w // 3 + w // 4 + 130, h // 2 + h // 3 + 50)], 130))
    feats.append(([rect(w // 3 + w // 8, h // 2 + h // 8, w, h)], 131))
    feats.append(([rect(-100, h - h // 4, w // 2, h + 900)], 130))                    # shares the label of the first of the three
    feats.append(([[(w // 16, h // 16), (w // 2, h // 3), (w // 2, h // 16), (w // 16, h // 3)]], 140))   # a bow-tie
    feats.append(([rect(w + 256, h + 256, w + 40000, h + 50000)], 160))              # wholly outside
    return feats, 200


def unit_squares(n=300, seed=5):
    """n squares of one pixel inside the first 64 x 64 tile, each around one pixel centre, labels 1..7 in turn; squares may repeat
    a pixel: the later one wins"""
    rng = np.random.default_rng(seed)
    feats = []
    for k in range(n):
        r, c = (int(v) for v in rng.integers(0, 64, 2))
        feats.append(([rect(SUB * c + 10, SUB * r + 10, SUB * c + 250, SUB * r + 250)], 1 + k % 7))
    return feats, 7


def star(H, W, n=1000):
    """one ring of n vertices around the grid's middle, the radius alternating: it crosses every tile"""
    w, h = SUB * W, SUB * H
    ring = []
    for k in range(n):
        a = 2 * np.pi * k / n
        rad = 0.62 if k & 1 else 0.35
        ring.append((int(round(w / 2 + rad * w * np.cos(a))), int(round(h / 2 + rad * h * np.sin(a)))))
    return [([ring], 3)], 3


@functools.lru_cache(maxsize=None)
def case(H, W, kind="scene"):
    """(the tables, Z, the model's labels, the model's area) of scene / unit_squares ("squares") / star: made once per shape and kind"""
    feats, Z = scene(H, W) if kind == "scene" else unit_squares() if kind == "squares" else star(H, W)
    labels, area = rasterize(feats, Z, H, W)
    labels.setflags(write=False)
    area.setflags(write=False)
    return tables(feats), Z, labels, area
