"""The cases that tests/test_gpu_limits.py runs on the device and tests/test_limits_cpu.py on the models alone, and the arithmetic that
shows, on the model's outputs, that a case takes the path it is there for ("Limits the tests reach").  The rasters
themselves are the model modules': fields_model, fields_split_model, mzones_model, bands_model."""
import numpy as np

import bands_model as bm
import fields_model as fm
import fields_split_model as sm
import mzones_model as mm

# ---- A: the numbering scan past its first turn --------------------------------------------------------------------------------------------
# What the keys of a case reach.  FULL: every turn of the scan holds a key, and so do the last chunk of the first turn and the first of
# the second.  TURNS: every turn holds a key.  COUNT: every key lies in the first turn; the later turns add nothing, and the carry still
# has to come through them to `found` and to the sums of their chunks.
FULL, TURNS, COUNT = "full", "turns", "count"
EDGE = {"edge": 150, "edge_r": 1}
MORPH = dict(r_open=1, r_close=2)
SCAN_SHAPES = [(513, 512), (730, 730)]                             # 257 chunks: the last turn holds one; 521 chunks: three turns
FIELDS = [(513, 512, "blobs", dict(conn=4), FULL), (513, 512, "noise", dict(conn=8, min_pixels=2), FULL), (513, 512, "checker", dict(conn=4), FULL),
          (730, 730, "blobs", dict(conn=4), FULL), (730, 730, "noise", dict(conn=8, min_pixels=2), TURNS), (730, 730, "checker", dict(conn=4), FULL)]
# the split numbers REGIONS, whose key is their smallest linear index: the one chunk of 513 x 512's second turn is the last row, and no
# region lies in one row alone, so there the split shows the carry in `found` only; 730 x 730 and 520 x 512 have keys on both sides
SPLITS = [(513, 512, "blobs", EDGE, dict(conn=4), COUNT), (730, 730, "blobs", EDGE, dict(conn=4), FULL),
          (513, 512, "noise", {}, dict(conn=8, **MORPH), COUNT), (730, 730, "parcels", EDGE, dict(conn=4), COUNT),
          (520, 512, "blobs", EDGE, dict(conn=4), FULL)]
CAPPED = [("fields", FIELDS[0]), ("split", SPLITS[0])]             # the cases that also run under grid caps 1 and 3


def fields_keys(H, W, name, kw):
    """the keys of every field the numbering counts: the model's table holds them up to Z; the checkerboard under conn 4 has more,
    and there every pixel of the mask is a field of its own"""
    labels, fields, found = fm.case(H, W, name, **kw)
    if found <= kw.get("Z", 65535):
        return fields[1:found + 1, 1]
    assert name == "checker" and kw.get("conn") == 4
    keys = np.flatnonzero(fm.cleaned(fm.raster(H, W, name), fm.LO, fm.HI))
    assert len(keys) == found
    return keys


def split_keys(H, W, name, split, kw):
    want = sm.case(H, W, name, split=split, **kw)
    assert want["found"] <= kw.get("Z", 65535)
    return want["fields"][1:want["found"] + 1, 1]


def scan_preconditions(keys, H, W, reach):
    """-> fields_model.scan_reach(keys, H, W), after asserting what `reach` promises"""
    assert -(-H * W // 1024) > 256
    r = fm.scan_reach(keys, H, W)
    assert r["chunks"] == -(-H * W // fm.CHUNK) and r["turns"] == -(-r["chunks"] // fm.TURN) >= 2
    assert len(keys) > 0 and r["carry"][1] > 0, "the carry is zero"
    if reach == COUNT:
        assert r["met"] == [0] and r["carry"][-1] == len(keys)
    else:
        assert r["met"] == list(range(r["turns"])), r
        assert all(a < b for a, b in zip(r["carry"], r["carry"][1:]))
    if reach == FULL:
        assert r["in255"] >= 1 and r["in256"] >= 1, r
    return r


# ---- C: the pending sums of the management zones -------------------------------------------------------------------------------------------
MZ_SHAPE = (16384, 64)                                             # one column of 512 tiles, 2 MB a plane
MZ_KW = dict(smooth=0, min_per_zone=10)
MZ_PARAMS = [("halves", 2), ("halves", 3), (("halves", "-halves", "halves", "halves/2"), 8)]       # the last: D = 4, k = 8, the widest ws[KM * D]
# "middle": rows [H / 4, 3 H / 4) are a second field, so a label change (tile 128) meets a run that has just flushed (tile 126); its runs
# of one label and one value are 128 tiles, 65536 pixels, whose sum 2^31 - 65536 still fits.  "late": the change comes 3 tiles later, so
# the first run is 131 tiles and would wrap as well
MZ_LAYOUTS = ("one", "middle", "late")
MZ_CAPS = (1, 3)


def pending_preconditions(cap):
    """the workgroup whose run of tiles lies in one half: a wave of it meets more pixels of one label and one value than its int32
    pending sums may hold, and their sum would wrap"""
    H, W = MZ_SHAPE
    ntiles = -(-H // 32)
    run_tiles = min(ntiles // 2, -(-ntiles // cap))
    assert ntiles == 512 and run_tiles * 512 > 65000 and run_tiles * 512 * 32767 >= 2 ** 31
    r = mm.pending_reach(H, W, cap)
    assert r["run_tiles"] == run_tiles and r["pixels"] > mm.PENDING and r["sum"] >= 2 ** 31
    return r


HALF_VALUES = {"halves": (-32767, 32767), "-halves": (32767, -32767), "halves/2": (-16384, 16383)}       # (lower half, upper half)


def halves_by_hand(names, lay, k):
    """What the definition gives on the halves, in plain integer arithmetic.  A field holds n_low members in the lower half of the
    rows and n_high in the upper.  The start centres lie on the diagonal of the box; every member of the lower half is nearest to
    the first and every member of the upper half to the last; the first update puts those two on the two values,
    (2 n |v| + n) // (2 n) = |v|, and leaves the empty ones where they started; the second changes nothing: 2 iterations.  The first
    raster is "halves", so zone 1 is the lower half and zone k the upper.
    -> (Z, per field 1..Z: (n_low, n_high), the two centres, the two table rows: n, then n v and n v^2 per feature)"""
    H, W = MZ_SHAPE
    names = (names,) if isinstance(names, str) else tuple(names)
    assert names[0] == "halves" and k >= 2
    first = {"one": None, "middle": H // 4, "late": H // 4 + 96}[lay]          # field 2: rows [first, 3 H / 4)
    rows = [(H // 2, H // 2)] if first is None else [(H // 4, first), (3 * H // 4 - H // 2, H // 2 - first)]       # (lower, upper) rows per field
    low, high = [HALF_VALUES[m][0] for m in names], [HALF_VALUES[m][1] for m in names]
    row = lambda n, vals: [n] + [x for v in vals for x in (n * v, n * v * v)]
    return len(rows), [((a * W, b * W), (low, high), (row(a * W, low), row(b * W, high))) for a, b in rows]


# ---- D: saturated bands ---------------------------------------------------------------------------------------------------------------------
BANDS_SHAPES = [(35, 40), (37, 45)]
BANDS_WEIGHTS = [(1, 1, 1), (255, 255, 255)]
BANDS_EPS = (1, 2 ** 31 - 1)                                       # the entry takes eps as an int32
BANDS_FILL = 77


def bands_cases(H, W, S):
    """every saturated scene with every band, weights, r, eps, masked and not -> (scene, band name, w, r, eps, masked)"""
    return [(name, band, w, r, eps, masked) for name in bm.SATURATED for band in bm.SATURATED_BANDS for w in BANDS_WEIGHTS for r in (1, 4)
            for eps in BANDS_EPS for masked in (False, True)]


_BANDS = {}


def bands_modelled(H, W, S, case):
    """-> (the carried band, inexact, the largest |A|, the blocks whose gain was clipped): made once per case"""
    key = (H, W, S) + case
    if key not in _BANDS:
        name, band, w, r, eps, masked = case
        q, b = bm.saturated_scene(H, W, S, name), bm.saturated_band(H, W, S, name, band)
        out, bad, parts = bm.carry(q, b, S, 0, 65535, w=w, r=r, eps=eps, valid=bm.holes(H, W, seed=7) if masked else None, fill=BANDS_FILL, parts=True)
        out.setflags(write=False)
        _BANDS[key] = out, bad, int(np.abs(parts["A"]).max()), int((np.abs(parts["A"]) == bm.GAIN_LIMIT).sum())
    return _BANDS[key]


def bands_preconditions(H, W, S):
    """over the cases of one shape and scale: some |A| >= 65535 (a gain of one in Q16), some block on the clip path (inexact), and a
    guide sum w0 q0 + w1 q1 + w2 q2 within a factor of two of 765 * 65535 (it is 765 * 65535 itself wherever a pixel is white) ->
    (largest |A|, most inexact blocks of a case)"""
    cases = bands_cases(H, W, S)
    top = max(bands_modelled(H, W, S, c)[2] for c in cases)
    inexact = max(bands_modelled(H, W, S, c)[1] for c in cases)
    assert top >= 65535 and inexact > 0
    for name in bm.SATURATED:
        x = int((255 * bm.saturated_scene(H, W, S, name).astype(np.int64).sum(axis=2)).max())
        assert 765 * 65535 // 2 <= x <= 765 * 65535 < 2 ** 26
    return top, inexact


# ---- D: the split's edge test on +-32767 ----------------------------------------------------------------------------------------------------
SATURATED_SHAPES = [(65, 129), (65, 128)]
SATURATED_CELLS = (1, 3, 8)


def saturated_preconditions(H, W, cell, split):
    """the raster holds +32767 and -32767 and nothing else; with r = 0 and cells of 3 or more a Sobel sum across a cell border is
    4 * 32767 against 4 * -32767, the largest the definition allows for n = 1; with larger windows a box sum lies inside a cell where
    the cell is wide enough, |B| = n * 32767, and the squared gradient needs more than 32 bits -> the largest gx^2 + gy^2"""
    idx = sm.saturated(H, W, cell)
    assert set(np.unique(idx).tolist()) == {-32767, 32767}
    r = split["edge_r"]
    g2 = int(sm.gradient2(idx, r).max())
    n = (2 * r + 1) ** 2
    assert 2 ** 32 < g2 <= 2 * (8 * n * 32767) ** 2 < 2 ** 63
    if r == 0 and cell >= 3:
        assert g2 >= (8 * 32767) ** 2
    return g2
