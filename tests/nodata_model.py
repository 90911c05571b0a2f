"""The nodata fill and mask (csrc/nodata.hip), restated in numpy: integers throughout.

fill    a valid pixel is unchanged; an invalid pixel p = (y, x) takes the samples of the valid pixel q that minimises
        (d2, qy, qx) lexicographically, d2 = (qy - y)^2 + (qx - x)^2, among the valid q with d2 <= R^2; none: p keeps its samples.
mask    output pixel (Y, X) at scale s is invalid iff input pixel (Y // s, X // s) is; invalid output pixels get out_nodata.

Two forms of the fill: sources_brute is the definition as written (every valid pixel is a candidate), sources_separable is the
per-column form the kernel uses (the vertically nearest valid pixel of each column within R, then a minimum over the columns).
Both return the SOURCE map src [H, W, 2] = (qy, qx), a pixel that keeps its samples being its own source; tests hold them equal."""
import functools

import numpy as np

NONE = 1 << 20       # d1: no valid pixel within R in this column


def sources_brute(valid, R):
    valid = np.asarray(valid) != 0
    H, W = valid.shape
    src = np.stack(np.meshgrid(np.arange(H), np.arange(W), indexing="ij"), axis=-1).astype(np.int64)
    qy, qx = np.nonzero(valid)
    if qy.size == 0:
        return src
    for y, x in zip(*np.nonzero(~valid)):
        d2 = (qy - y) ** 2 + (qx - x) ** 2
        ok = d2 <= R * R
        if not ok.any():
            continue
        key = (d2[ok] * H + qy[ok]) * W + qx[ok]           # (d2, qy, qx), lexicographic
        k = int(np.argmin(key))
        src[y, x] = (qy[ok][k], qx[ok][k])
    return src


def column_offsets(valid, R):
    """d1 [H, W]: the signed offset in [-R, R] to the vertically nearest valid pixel of the column, a tie to the pixel above;
    NONE where there is none."""
    valid = np.asarray(valid) != 0
    H, W = valid.shape
    d1 = np.full((H, W), NONE, np.int64)
    for k in range(min(R, H - 1), -1, -1):                 # nearer offsets written later win; at equal k the upper one last
        below = np.zeros((H, W), bool)
        below[:H - k] = valid[k:] if k else valid
        d1[below] = k
        above = np.zeros((H, W), bool)
        above[k:] = valid[:H - k] if k else valid
        d1[above] = -k
    return d1


def sources_separable(valid, R):
    valid = np.asarray(valid) != 0
    H, W = valid.shape
    d1 = column_offsets(valid, R)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    best = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    for dx in range(-R, R + 1):
        c = xs + dx
        inside = (c >= 0) & (c < W)
        d = np.where(inside, d1[ys, np.clip(c, 0, W - 1)], NONE)
        cost = dx * dx + d * d
        ok = inside & (d != NONE) & (cost <= R * R)
        key = (cost * H + (ys + d)) * W + c                # ((c - x)^2 + d1^2, y + d1, c)
        best = np.where(ok & (key < best), key, best)
    src = np.stack([ys, xs], axis=-1).astype(np.int64)
    hit = ~valid & (best != np.iinfo(np.int64).max)
    src[hit, 0] = (best[hit] // W) % H
    src[hit, 1] = best[hit] % W
    return src


def fill(img, valid, R, sources=sources_separable):
    src = sources(valid, R)
    return np.ascontiguousarray(np.asarray(img)[src[..., 0], src[..., 1]])


def upsample(valid, scale):
    return np.repeat(np.repeat(np.asarray(valid) != 0, scale, axis=0), scale, axis=1)


def mask(out, valid, scale, out_nodata):
    """out [sH, sW, 3] with out_nodata in the output pixels of the invalid input pixels."""
    out = np.array(out, copy=True)
    out[~upsample(valid, scale)] = out_nodata
    return out


# ---- the masks the tests share -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_mask(kind, H, W, seed=0):
    rng = np.random.default_rng(seed + 7919 * H + W)
    if kind == "holes":                                   # random holes: blobs of several sizes plus single pixels
        v = rng.random((H, W)) > 0.15
        for _ in range(6):
            y, x, r = rng.integers(0, H), rng.integers(0, W), rng.integers(2, max(3, min(H, W) // 3))
            yy, xx = np.ogrid[:H, :W]
            v &= (yy - y) ** 2 + (xx - x) ** 2 > r * r
    elif kind == "edge":                                  # a diagonal swath edge: about 30 % invalid
        yy, xx = np.ogrid[:H, :W]
        v = (yy * W + xx * H) * 1000 >= 775 * H * W       # the corner triangle below y / H + x / W = 0.775: 0.775^2 / 2 = 0.30
    elif kind == "island":                                # three valid pixels in an invalid plane
        v = np.zeros((H, W), bool)
        v[H // 2, W // 2] = v[H // 2, W // 2 + 1] = v[H // 2 + 1, W // 2] = True
    elif kind == "all_valid":
        v = np.ones((H, W), bool)
    elif kind == "all_invalid":
        v = np.zeros((H, W), bool)
    else:
        raise ValueError(kind)
    v = v.astype(np.uint8)
    v.setflags(write=False)
    return v
