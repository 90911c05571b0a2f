"""The touching-fields split without a GPU: the definition's model (tests/fields_split_model.py) against scipy's
distance transform, against the plain segmentation under the degenerate parameters, on planted parcels, dumbbells and the snake; the
host policy (s2sr/fields.py: the "split" key, its refusals, resolve() and the metadata with and without it); the rings of a split
result; and the C ABI's declarations."""
import re
from pathlib import Path

import numpy as np
import pytest

import fields_model as fm
import fields_split_model as sm
import zones_model as zm
from fields_model import HI, LO
from s2sr import fields as xf
from s2sr import native

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "s2sr.h").read_text()
PATTERNS = ("spiral", "checker", "comb", "rings", "noise", "ones", "zeros", "stripes", "blobs")


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def test_the_distance_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for H, W in ((37, 45), (65, 129), (65, 128), (37, 180)):
        for name in PATTERNS:
            for kw in ({}, dict(r_open=1, r_close=2)):
                I = fm.cleaned(fm.patterns(H, W)[name], LO, HI, **kw)
                if I.all():                                        # scipy has no outside pixel to measure from: the definition says the cap
                    want = np.full(I.shape, 255 * 255, np.int64)
                else:
                    d = ndi.distance_transform_edt(I)
                    want = np.minimum(np.rint(d * d).astype(np.int64), 255 * 255) * I
                assert (sm.distance2(I) == want).all(), (H, W, name, kw)
    # the cap, and a raster's edge that does not count: a full column band is as far from its sides as it is wide
    I = np.ones((5, 600), bool)
    I[:, 0] = False
    D = sm.distance2(I)
    assert D[2, 1] == 1 and D[2, 254] == 254 * 254 and D[2, 255] == D[2, 599] == 255 * 255 and D[:, 0].max() == 0


def test_the_distance_by_brute_force():
    """every pixel of I against every pixel outside it, on shapes small enough for that"""
    rng = np.random.default_rng(11)
    for H, W in ((1, 1), (1, 17), (9, 1), (13, 21)):
        for p in (0.05, 0.5, 0.95):
            I = rng.random((H, W)) > p
            ys, xs = np.nonzero(~I)
            want = np.zeros((H, W), np.int64)
            for y, x in zip(*np.nonzero(I)):
                want[y, x] = min(255 * 255, int(((ys - y) ** 2 + (xs - x) ** 2).min())) if len(ys) else 255 * 255
            assert (sm.distance2(I) == want).all(), (H, W, p)


def test_the_gradient_on_hand_made_cases():
    N = fm.NODATA
    flat = np.full((5, 6), 700, np.int16)
    assert not sm.gradient2(flat, 0).any() and not sm.gradient2(flat, 2).any()        # borders replaced by the centre: no gradient at the rim
    step = flat.copy()
    step[:, 3:] = 1000
    g = sm.gradient2(step, 0)
    assert g[2, 2] == g[2, 3] == (4 * 300) ** 2 and g[2, 1] == g[2, 4] == 0
    assert g[0, 2] == (3 * 300) ** 2 + 300 ** 2                    # the row above the raster counts as the centre: three quarters across, one down
    # a threshold of T per pixel: a ramp of T per pixel has gx = 8 T, which is not above it; T + 1 is
    ramp = (np.arange(8)[None, :] * 50 + np.zeros((6, 1))).astype(np.int16)
    assert (sm.gradient2(ramp, 0)[2, 2:6] == (8 * 50) ** 2).all() and (sm.gradient2(ramp, 1)[3, 3] == (8 * 9 * 50) ** 2)
    m = np.ones(ramp.shape, bool)
    assert sm.interior(ramp, m, 50, 0)[:, 1:7].all() and not sm.interior(ramp, m, 49, 0)[1:5, 1:7].any()
    assert sm.interior(ramp, m, 50, 1)[2:4, 2:6].all() and not sm.interior(ramp, m, 49, 1)[2:4, 2:6].any()
    hole = step.copy()
    hole[2, 3] = N                                                 # a nodata neighbour counts as the centre
    g = sm.gradient2(hole, 0)
    assert g[2, 2] == (2 * 300) ** 2 + 0 and g[1, 2] == (3 * 300) ** 2 + (300) ** 2


@pytest.mark.parametrize("conn", [4, 8])
def test_the_degenerate_parameters_and_none_are_the_plain_segmentation(conn):
    for H, W in ((37, 45), (65, 129), (65, 128), (37, 180)):
        for name in PATTERNS:
            for kw in (dict(conn=conn), dict(conn=conn, r_open=1, r_close=2, min_pixels=3, Z=9)):
                idx = fm.patterns(H, W)[name]
                labels, fields, found = fm.segment(idx, LO, HI, **kw)
                for split in (None, sm.DEGENERATE, dict(sm.DEGENERATE, edge_r=4)):
                    got = sm.split(idx, LO, HI, split=split, **kw)
                    assert (got["labels"] == labels).all() and (got["fields"] == fields).all() and got["found"] == found, (H, W, name, kw, split)
                    if split is not None:
                        assert (got["cores"] == fm.cleaned(idx, LO, HI, kw.get("r_open", 0), kw.get("r_close", 0))).all()


def test_the_rasters_are_real_cases_at_the_widths_of_the_sr_grid():
    """tests/doors.py WIDTHS, which tests/test_gpu_fields_split.py splits: at least two fields on blobs, parcels and noise with
    the edge test, and on the blobs behind the morphology.  5 x 8 and 1 x 68 are left out: a single vector group and a single row are there for
    the addresses, and hold one blob."""
    import doors
    for H, W in doors.WIDTHS:
        if (H, W) in ((5, 8), (1, 68)):
            continue
        for name in ("blobs", "parcels", "noise"):
            assert sm.case(H, W, name, split={"edge": 150, "edge_r": 1}, conn=4)["found"] >= 2, (H, W, name)
        assert sm.case(H, W, "blobs", split={}, conn=8, r_open=1, r_close=2)["found"] >= 2, (H, W)


def test_the_parcels_come_out_as_planted():
    idx, planted = sm.parcels()
    assert fm.segment(idx, LO, HI)[2] == 1                          # one blob without the split
    assert sm.split(idx, LO, HI, split={})["found"] < 6             # and the distance alone does not find six rectangles
    for r in (0, 1):
        got = sm.split(idx, LO, HI, conn=4, split={"edge": 150, "edge_r": r})
        assert got["found"] == 6 and (got["labels"] == planted).all(), r
        assert got["fields"][1].tolist() == [32 * 40, 3 * 130 + 5, 5, 3, 45, 35] and got["levels"][1] >= 1


@pytest.mark.parametrize("sep,R1,R2,fields,cut", [(22, 12, 12, 2, 27), (16, 12, 7, 2, 27), (14, 12, 5, 1, None)])
def test_the_dumbbells(sep, R1, R2, fields, cut):
    got = sm.split(sm.dumbbell(sep, R1, R2), LO, HI, split={})
    L = got["labels"]
    assert got["found"] == fields
    cuts = sorted(set(np.nonzero((L[:, :-1] != L[:, 1:]) & (L[:, :-1] > 0) & (L[:, 1:] > 0))[1].tolist()))
    assert cuts == ([cut] if cut is not None else [])
    assert (L > 0).sum() == (fm.segment(sm.dumbbell(sep, R1, R2), LO, HI)[0] > 0).sum()       # the same pixels, otherwise owned


def _steps_from(seed, domain, conn):
    """steps of the shortest path inside `domain` from the pixel set `seed`, -1 where none: a plain queue, not the model's levels"""
    from collections import deque
    H, W = domain.shape
    near = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    steps = np.full((H, W), -1, np.int64)
    todo = deque()
    for y, x in zip(*np.nonzero(seed)):
        steps[y, x] = 0
        todo.append((int(y), int(x)))
    while todo:
        y, x = todo.popleft()
        for dy, dx in near:
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and domain[ny, nx] and steps[ny, nx] < 0:
                steps[ny, nx] = steps[y, x] + 1
                todo.append((ny, nx))
    return steps


@pytest.mark.parametrize("H,W", [(40, 23), (41, 24), (65, 30)])
def test_the_snake_is_cut_at_its_geodesic_midpoint(H, W):
    """two rooms, one corridor: every pixel goes to the nearer room's marker along the corridor, a tie to the smaller key; judged by
    one queue per marker, which knows nothing of levels"""
    m = sm.snake(H, W, 2)
    got = sm.split(fm.as_index(m), LO, HI, conn=4, split={})
    assert got["found"] == 2 and got["levels"][0] > (H - 20) // 2 * W // 2
    markers = fm.components(got["cores"].astype(bool), 4)
    assert len(markers) == 2 and markers[0][0] == 0
    a, b = (_steps_from(np.isin(np.arange(H * W).reshape(H, W), px), m, 4) for _, px in markers)
    assert (a[m] >= 0).all() and (b[m] >= 0).all()
    want = np.where(m, np.where(a <= b, 1, 2), 0)                  # the first marker holds the smaller key: the tie is its
    assert (got["labels"] == want).all()
    ties = int((m & (a == b)).sum())
    assert ties <= 1
    if (H, W) == (40, 23):
        assert ties == 1                                           # this one has the tie
    # one room: one field, however long the corridor
    one = sm.split(fm.as_index(sm.snake(H, W, 1)), LO, HI, conn=4, split={})
    assert one["found"] == 1 and one["fields"][1, 0] == sm.snake(H, W, 1).sum()


def test_a_component_that_is_all_edge_gets_no_label():
    idx = sm.edge_only(40, 50)
    got = sm.split(idx, LO, HI, conn=4, split={"edge": 150, "edge_r": 0})
    strip = idx == 9000
    assert strip.sum() > 50 and not got["labels"][strip].any() and not got["cores"][strip].any()
    block = idx == 5000
    assert got["found"] == 1 and (got["labels"][block] == 1).all() and got["levels"][1] >= 1      # the block's rim is won back
    assert got["fields"][0, 0] == idx.size - block.sum()
    assert fm.segment(idx, LO, HI)[2] == 2                          # the plain segmentation keeps the strip


def test_the_field_key_is_the_fields_first_pixel_not_the_markers():
    """an L whose core lies in its foot: the marker's key is in the foot, the field's key is the top of the stem"""
    m = np.zeros((30, 30), bool)
    m[0:20, 2:4] = True
    m[20:29, 2:20] = True
    got = sm.split(fm.as_index(m), LO, HI, split={})
    assert got["found"] == 1 and got["fields"][1, 1] == 2 and got["cores"][:20].sum() == 0 and got["fields"][1].tolist() == [m.sum(), 2, 2, 0, 20, 29]


def test_the_rings_of_a_split_result_burn_back_to_its_labels():
    for idx, split, kw in ((sm.parcels()[0], {"edge": 150, "edge_r": 1}, {}), (fm.patterns(65, 129)["blobs"], {}, dict(r_open=1, r_close=2, conn=8)),
                           (sm.dumbbell(16, 12, 7), {}, {}), (sm.edge_only(40, 50), {"edge": 150, "edge_r": 0}, {})):
        got = sm.split(idx, LO, HI, split=split, **kw)
        labels, Z = got["labels"], got["found"]
        xy, ring_start, ring_label = fm.trace(labels, Z)
        feats = [([[(256 * int(x), 256 * int(y)) for x, y in xy[ring_start[k]:ring_start[k + 1]]] for k in np.flatnonzero(ring_label == l)], l)
                 for l in sorted(set(ring_label.tolist()))]
        assert (zm.rasterize(feats, Z, *labels.shape)[0] == labels).all()
        polys = xf.polygons((xy, ring_start, ring_label), got["fields"][:Z + 1])
        assert [p["pixels"] for p in polys] == got["fields"][1:Z + 1, 0].tolist()


# ---- s2sr/fields.py --------------------------------------------------------------------------------------------------------------------------
DEFS = [{"name": "ndvi", "K": 10000}, {"name": "ndwi", "K": 5000}]
GOOD = {"index": "ndvi", "min": 0.3, "max": None, "open": 1, "close": 2, "connectivity": 4, "min_area_ha": 0.5}
TODAY = {"index": 0, "name": "ndvi", "K": 10000, "lo": 3000, "hi": 32767, "r_open": 1, "r_close": 2, "conn": 4, "min_pixels": 800}


def test_resolve_with_and_without_the_key():
    assert xf.resolve({"segment": GOOD}, DEFS, 6.25) == TODAY       # without the key: today's dict, key for key
    assert xf.resolve({"segment": dict(GOOD, split=True)}, DEFS, 6.25) == dict(TODAY, split={"core_q": 500, "core_px": 2, "edge": 0, "edge_r": 1})
    assert xf.resolve({"segment": dict(GOOD, split={})}, DEFS, 6.25)["split"] == {"core_q": 500, "core_px": 2, "edge": 0, "edge_r": 1}
    p = xf.resolve({"segment": dict(GOOD, split={"core": 0.3333, "core_px": 0, "edge": 0.015, "edge_smooth": 4})}, DEFS, 6.25)
    assert p["split"] == {"core_q": 333, "core_px": 0, "edge": 150, "edge_r": 4}
    p = xf.resolve({"segment": dict(GOOD, index="ndwi", split={"core": 1, "core_px": 255, "edge": 0.015, "edge_smooth": 0})}, DEFS, 6.25)
    assert p["split"] == {"core_q": 1000, "core_px": 255, "edge": 75, "edge_r": 0}                      # in units of 1 / K of the named index
    assert xf.resolve({"segment": dict(GOOD, split={"edge": 1e-9})}, DEFS, 6.25)["split"]["edge"] == 1           # kept inside 1..32767
    assert xf.resolve({"segment": dict(GOOD, split={"edge": 99.0})}, DEFS, 6.25)["split"]["edge"] == 32767
    assert xf.resolve({"segment": dict(GOOD, split={"core": 0.0006})}, DEFS, 6.25)["split"]["core_q"] == 1
    assert xf.check_option({"segment": GOOD}) == dict(xf.DEFAULTS, **GOOD)


@pytest.mark.parametrize("value,text", [
    (False, "True, or a dict"), (None, "True, or a dict"), (1, "True, or a dict"), ("yes", "True, or a dict"), ([], "True, or a dict"),
    ({"colour": 1}, "unknown key"), ({"core_q": 500}, "unknown key"), ({"core": 0}, "core"), ({"core": -0.5}, "core"), ({"core": 1.01}, "core"),
    ({"core": "0.5"}, "core"), ({"core": True}, "core"), ({"core": float("nan")}, "core"), ({"core": 0.0004}, "core"), ({"core_px": -1}, "core_px"),
    ({"core_px": 256}, "core_px"), ({"core_px": 2.0}, "core_px"), ({"core_px": True}, "core_px"), ({"edge": 0}, "edge"), ({"edge": -0.1}, "edge"),
    ({"edge": float("inf")}, "edge"), ({"edge": "x"}, "edge"), ({"edge": True}, "edge"), ({"edge_smooth": -1}, "edge_smooth"),
    ({"edge_smooth": 5}, "edge_smooth"), ({"edge_smooth": 1.0}, "edge_smooth"), ({"edge_smooth": None}, "edge_smooth")])
def test_every_refusal_of_the_split_key(value, text):
    with pytest.raises(ValueError, match=text):
        xf.resolve({"segment": dict(GOOD, split=value)}, DEFS, 6.25)


class _StubEngine:
    """the two entries answer from the models without a device; which of them s2sr.fields.segment calls"""
    import threading
    chain_lock = threading.RLock()

    def __init__(self):
        self.calls = []

    def fields_segment_i16(self, idx, lo, hi, **kw):
        self.calls.append("segment")
        return fm.segment(idx, lo, hi, **kw)

    def fields_split_i16(self, idx, lo, hi, split=None, **kw):
        self.calls.append("split")
        assert kw["Z"] == 65535 and split is not None
        r = sm.split(idx, lo, hi, split=split, **kw)
        return r["labels"], r["fields"], r["found"]

    def labels_trace_u16(self, labels, Z):
        return fm.trace(labels, Z)


def test_segment_calls_the_new_entry_only_with_the_key_and_the_metadata_follows():
    idx, planted = sm.parcels()
    option = {"segment": {"index": "ndvi", "min": 0.4, "open": 0, "close": 0, "min_pixels": 5}}
    e = _StubEngine()
    params = xf.resolve(option, DEFS, None)
    plain = xf.segment(e, idx, params)
    assert e.calls == ["segment"] and plain["found"] == 1 and "split" not in params
    with_key = {"segment": dict(option["segment"], split={"edge": 0.015})}
    params_s = xf.resolve(with_key, DEFS, None)
    got = xf.segment(e, idx, params_s)
    assert e.calls == ["segment", "split"] and got["found"] == 6 and (got["labels"] == planted).all() and got["fields"].shape == (7, 6)
    assert len(xf.polygons(got["rings"], got["fields"])) == 6
    today = {"name": "ndvi", "K": 10000, "lo": 4000, "hi": 32767, "r_open": 0, "r_close": 0, "conn": 4, "min_pixels": 5}
    block = xf.metadata_block(params, 1, plain["fields"], idx.shape, None, None, None)
    assert block["parameters"] == today and list(block["parameters"]) == list(today)
    block = xf.metadata_block(params_s, 6, got["fields"], idx.shape, None, None, None)
    assert block["parameters"] == dict(today, split={"core_q": 500, "core_px": 2, "edge": 150, "edge_r": 1}) and block["found"] == 6
    # the refusals stay: no field, too many
    with pytest.raises(ValueError, match="found no field"):
        xf.segment(e, idx, dict(params_s, lo=20000))

    class Many(_StubEngine):
        def fields_split_i16(self, *a, **kw):
            labels, fields, _ = super().fields_split_i16(*a, **kw)
            return labels, fields, 65536
    with pytest.raises(ValueError, match="found 65536 fields"):
        xf.segment(Many(), idx, params_s)


def test_the_job_checks_the_key_in_both_forms_before_anything_is_created():
    from app.job_options import JobOptions
    seg = {"segment": dict(GOOD, split={"core": 0.4, "edge": 0.02})}
    JobOptions(bit_depth=16, indices=["ndvi"], zones=seg).check(False, 4)
    JobOptions(bit_depth=16, indices=["ndvi"], zones={"segment": dict(GOOD, split=True)}).check(False, 4)
    JobOptions(bit_depth=16, indices=["ndvi"], zones={"manage": {"index": "ndvi"}, "fields": seg}).check(False, 4)
    for bad, text in (({"core": 2}, "core"), ({"edge_smooth": 9}, "edge_smooth"), ({"colour": 1}, "unknown key"), (0, "True, or a dict")):
        for zones in ({"segment": dict(GOOD, split=bad)}, {"manage": {"index": "ndvi"}, "fields": {"segment": dict(GOOD, split=bad)}}):
            with pytest.raises(ValueError, match=text):
                JobOptions(bit_depth=16, indices=["ndvi"], zones=zones).check(False, 4)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_and_refuse_a_null_handle():
    for name, n in (("s2sr_fields_split_i16", 17), ("s2sr_debug_fields_split_stage_ms", 4)):
        assert name in native.EXPORTED_SYMBOLS and re.search(rf"\b{name}\(", HEADER)
        decl = re.search(rf"{name}\(([^;]*)\);", HEADER).group(1)
        assert len([a for a in re.sub(r"/\*.*?\*/", "", decl).split(",") if a.strip()]) == len(native._PROTOS[name][1]) == n
    lib = native.load_library()
    assert lib.s2sr_fields_split_i16(None, None, 1, 1, 0, 0, 0, 0, 4, 1, 1, None, None, None, None, None, None) == -1
    assert lib.s2sr_debug_fields_split_stage_ms(None, None, None, None) == -1
    stages = [int(v) for _, v in sorted(re.findall(r"#define S2SR_FSPLIT_(?!STAGES)(\w+) (\d+)", HEADER), key=lambda m: int(m[1]))]
    assert stages == list(range(len(native.FSPLIT_STAGES))) and int(re.search(r"#define S2SR_FSPLIT_STAGES (\d+)", HEADER).group(1)) == len(stages) == 7
    record = re.search(r"typedef struct s2sr_fields_split \{(.*?)\} s2sr_fields_split;", HEADER, re.S).group(1)
    assert re.findall(r"int32_t (\w+);", record) == ["core_q", "core_px", "edge", "edge_r"]
    text = HEADER[HEADER.index("Touching fields split"):HEADER.index("typedef struct s2sr_fields_split")]
    assert "scratch" in text and "voids" in text and "keeps nothing" in text and "order of atomics" in text
    # the plain entry and its hook are what they were
    assert int(re.search(r"#define S2SR_FIELDS_STAGES (\d+)", HEADER).group(1)) == len(native.FIELDS_STAGES) == 8


def test_the_python_layer_checks_before_the_library():
    with pytest.raises(TypeError):
        native.Engine.fields_split_i16(None, np.zeros((2, 2), np.uint16), 0, 1)
    with pytest.raises(ValueError, match="unknown output"):
        native.Engine.fields_split_i16(None, np.zeros((2, 2), np.int16), 0, 1, want=("labels",))
