"""Touching fields split on the GPU (include/s2sr.h: s2sr_fields_split_i16; csrc/fields_split.hip): labels, fields,
found, dist2 and cores byte for byte against tests/fields_split_model.py on shapes that cross the 64 x 64 tile lines, on the patterns
that break a union-find and on the rasters made for the split (dumbbell, parcels, snake, edge-only), under both connectivities, with
and without morphology and edge test; a 300 x 600 rectangle whose distance reaches the cap; every parameter at its limits; NULL and
the degenerate parameters against s2sr_fields_segment_i16 on the device; the independence of the number of workgroups (caps 1 and
3); every refusal, the void rule, the stage hook, and the job that splits its own NDVI.  The shapes include the widths of the SR grid
(doors.WIDTHS: at W % 8 == 0 the mask, morphology and label kernels the entry shares with the fields pass move 8 and 16 bytes a lane).
The entry under red zones, poison, stalls and cap 8: its rows of tests/doors.py, whose baselines this module holds to the model.

The pass's capped launches are counted in the grid-cap family "display"."""
import json

import numpy as np
import pytest

import diag
import doors
import fields_model as fm
import fields_split_model as sm
import gpu_engines
from diag import same_values as same
from fields_model import HI, LO
from s2sr import native

pytestmark = pytest.mark.gpu

HP = native.PREC_F16_HP
SHAPES = [(1, 1), (1, 130), (63, 65), (64, 64), (65, 129), (130, 197)] + doors.WIDTHS
PATTERNS = ("spiral", "checker", "comb", "rings", "noise", "ones", "zeros", "stripes", "blobs") + sm.NEW
GRID_FAMILY = "display"
PLAIN = {}                                                        # the defaults: core 0.5, 2 pixels, no edge test
EDGE = {"edge": 150, "edge_r": 1}
MORPH = dict(r_open=1, r_close=2)
KEYS = ("labels", "fields", "dist2", "cores")


@pytest.fixture(scope="module")
def bare():
    with gpu_engines.bare(precision=HP) as e:                    # the entry needs no weights
        yield e


def run(e, idx, split, **kw):
    labels, fields, found, dist2, cores = e.fields_split_i16(idx, LO, HI, split=split, want=("dist2", "cores"), **kw)
    return {"labels": np.array(labels), "fields": fields, "found": found, "dist2": dist2, "cores": cores}


def compare(got, want, what):
    assert got["found"] == want["found"], f"{what}: found {got['found']} against {want['found']}"
    for key in KEYS:
        same(got[key], want[key], f"{what}: {key}")
    assert int(got["fields"][:, 0].sum()) == got["labels"].size


def check(e, H, W, name, split, **kw):
    want = sm.case(H, W, name, split=split, **kw)
    compare(run(e, sm.raster(H, W, name), split, **kw), want, f"{H} x {W} {name} {split} {kw}")
    return want


@pytest.mark.parametrize("H,W", SHAPES)
def test_byte_for_byte_against_the_model(bare, H, W):
    """every raster under conn 4 with the edge test and under conn 8 with the morphology; the other two combinations on the rasters
    with the most fields"""
    found = {}
    for name in PATTERNS:
        found[name, 4] = check(bare, H, W, name, EDGE, conn=4)["found"]
        found[name, 8] = check(bare, H, W, name, PLAIN, conn=8, **MORPH)["found"]
    for name in ("snake", "snake1", "dumbbell"):                   # the corridor survives only without the open
        found[name, 0] = check(bare, H, W, name, PLAIN, conn=4)["found"]
    for name in ("noise", "blobs", "parcels"):
        check(bare, H, W, name, {"core_q": 700, "core_px": 3}, conn=4, min_pixels=2, **MORPH)
        check(bare, H, W, name, {"edge": 150, "edge_r": 0}, conn=8)
    assert found["zeros", 4] == found["zeros", 8] == 0 and found["ones", 8] == 1
    if (H, W) == (130, 197):
        assert found["parcels", 4] == 6 and found["dumbbell", 0] == 2 and found["snake", 0] == 2 and found["snake1", 0] == 1
        assert found["blobs", 8] > fm.case(H, W, "blobs", conn=8, **MORPH)[2]                 # the split has something to split


def test_the_planted_parcels_and_the_dumbbells(bare):
    idx, planted = sm.parcels()
    for r in (0, 1):
        got = run(bare, idx, {"edge": 150, "edge_r": r}, conn=4)
        same(got["labels"], planted, f"parcels, edge_r {r}")
    for (sep, R1, R2), n in (((22, 12, 12), 2), ((16, 12, 7), 2), ((14, 12, 5), 1)):
        idx = sm.dumbbell(sep, R1, R2)
        got = run(bare, idx, PLAIN)
        compare(got, sm.split(idx, LO, HI, split=PLAIN), f"dumbbell {sep} {R1} {R2}")
        assert got["found"] == n


def test_the_distance_reaches_its_cap_through_the_halo(bare):
    """300 x 600: a rectangle 560 pixels wide over every row (beyond the raster nothing counts), so D2 is 255^2 in its middle, with a
    notch of 21 rows from the top: the pixel (270, 290) is 250 rows and 10 columns from the notch's corner and scans 250 columns each
    way, and (299, 300) is further than 255 pixels from everything"""
    idx = sm.notched()
    want = sm.split(idx, LO, HI, split=PLAIN)
    compare(run(bare, idx, PLAIN), want, "the notched rectangle")
    assert want["dist2"].max() == 255 * 255 and want["dist2"][270, 290] == 250 * 250 + 10 * 10 and want["dist2"][299, 300] == 255 * 255 and want["dist2"][150, 20] == 1


@pytest.mark.parametrize("H,W", [(65, 129), (65, 128)])
def test_every_parameter_at_its_limits(bare, H, W):
    """(65 x 128: the same on the vector path of the kernels shared with the fields pass)"""
    for name in ("blobs", "parcels", "noise"):
        for conn in (4, 8):
            for split in ({"core_q": 1}, {"core_q": 1000}, {"core_px": 0}, {"core_px": 255}, {"core_q": 1000, "core_px": 255, "edge": 1, "edge_r": 4},
                          {"edge": 32767, "edge_r": 0}, {"edge": 32767, "edge_r": 4}, {"edge": 1, "edge_r": 0}, {"core_q": 1, "core_px": 0, "edge": 150, "edge_r": 2}):
                check(bare, H, W, name, split, conn=conn)
        check(bare, H, W, name, EDGE, conn=4, min_pixels=40)
        n = check(bare, H, W, name, EDGE, conn=8, min_pixels=2, Z=3)["found"]
        assert n > 3
        check(bare, H, W, name, PLAIN, conn=4, Z=1)
        check(bare, H, W, name, EDGE, conn=4, r_open=8, r_close=8)


def test_null_and_the_degenerate_parameters_are_the_plain_segmentation(bare):
    for H, W in ((63, 65), (130, 197)):
        for name, kw in (("blobs", dict(conn=4, min_pixels=3, **MORPH)), ("noise", dict(conn=8)), ("spiral", dict(conn=4)), ("stripes", dict(conn=8, Z=7)),
                         ("parcels", dict(conn=4))):
            idx = sm.raster(H, W, name)
            labels, fields, found = bare.fields_segment_i16(idx, LO, HI, **kw)
            labels = np.array(labels)
            for split in (None, sm.DEGENERATE):
                got = bare.fields_split_i16(idx, LO, HI, split=split, **kw)
                what = f"{H} x {W} {name} {kw} split {split}"
                same(np.array(got[0]), labels, what + ": labels")
                same(got[1], fields, what + ": fields")
                assert got[2] == found, what
            same(labels, sm.case(H, W, name, **kw)["labels"], "and the model's")


@pytest.mark.parametrize("cap", [1, 3])
def test_under_capped_grids(bare, cap):
    """the same bytes with every workgroup on several trips: 130 x 197 pixels are 3 x 4 tiles"""
    H, W = 130, 197
    for name, split, kw in (("snake", PLAIN, dict(conn=4)), ("noise", EDGE, dict(conn=8, min_pixels=2)), ("blobs", EDGE, dict(conn=4, **MORPH)),
                            ("parcels", {"edge": 150, "edge_r": 0}, dict(conn=4))):
        with diag.under(cap):
            check(bare, H, W, name, split, **kw)
            launches, trips = native.grid_cap_stats()[GRID_FAMILY]
        assert launches >= 20 and trips == -(-101 // cap), (name, launches, trips)      # the most trips are the per-pixel passes': 25610 pixels, 256 a workgroup
    native.grid_cap_stats(reset=True)
    check(bare, H, W, "snake", PLAIN, conn=4)
    assert native.grid_cap_stats()[GRID_FAMILY] == (0, 0)                                  # off means off


@pytest.mark.parametrize("ident", doors.owned("fields_split_i16"))
def test_the_door_table_s_baseline_is_the_model(ident):
    """tests/doors.py's rows of this pass: the red-zone, poison, stall and grid-cap matrices hold every mode to diag.baseline, and
    this holds the baseline to the model, sample for sample"""
    same(diag.baseline(ident), doors.MODELS[ident](), ident)


def test_stage_times_by_events_and_the_rounds(bare):
    """s2sr_debug_fields_split_stage_ms: every launch of a profiled call is booked to its stage; no figure is asserted beyond its
    sign.  The snake's corridor crosses tile lines again and again, so its growth takes many rounds and still matches."""
    H, W = 130, 197
    kw = dict(conn=8, min_pixels=3, **MORPH)
    check(bare, H, W, "blobs", EDGE, **kw)
    off = bare.fields_split_stage_ms()
    assert all(off[s] == (0.0, 0) for s in native.FSPLIT_STAGES), "a call without profiling leaves no stage times"
    assert off["rounds"][0] >= 2 and off["rounds"][1] >= 2
    bare.set_profiling(1)
    bare.reset_kernel_stats()
    try:
        check(bare, H, W, "blobs", EDGE, **kw)
        per = bare.fields_split_stage_ms()
        bare.kernel_stats()
        check(bare, H, W, "snake", PLAIN, conn=4)
        snake = bare.fields_split_stage_ms()
        bare.kernel_stats()
    finally:
        bare.set_profiling(0)
    assert list(per) == list(native.FSPLIT_STAGES) + ["rounds"]
    ri, re_ = per["rounds"]
    # mask + 8 morphology passes + nodata mask + edge; the two distance passes as one; 2 x (local, border, flatten) + cores + seeds
    assert [per[s][1] for s in native.FSPLIT_STAGES] == [11, 1, 8, ri, 1 + re_, 1, 4]
    assert all(per[s][0] > 0 for s in native.FSPLIT_STAGES)
    si, se = snake["rounds"]
    assert si > 4 and se == 0, snake["rounds"]
    assert [snake[s][1] for s in native.FSPLIT_STAGES] == [1, 1, 8, si, 0, 1, 4]
    check(bare, H, W, "blobs", EDGE, **kw)
    assert all(bare.fields_split_stage_ms()[s] == (0.0, 0) for s in native.FSPLIT_STAGES)


def test_every_refusal_returns_minus_one_and_leaves_the_next_call_intact(bare):
    H, W = 63, 65
    idx = np.ascontiguousarray(sm.raster(H, W, "blobs"))
    kw = dict(conn=8, min_pixels=2)
    want = sm.case(H, W, "blobs", split=EDGE, **kw)
    lib = native.load_library()
    Z = 65535
    labels, fields, found = np.zeros((H, W), np.uint16), np.zeros((Z + 1, 6), np.int64), np.zeros(1, np.uint64)
    dist2, cores = np.zeros((H, W), np.uint16), np.zeros((H, W), np.uint8)
    rec = lambda **over: np.array([dict(dict(sm.DEFAULT, **EDGE), **over)[k] for k in ("core_q", "core_px", "edge", "edge_r")], np.int32)
    base = dict(idx=idx, H=H, W=W, lo=LO, hi=HI, r_open=0, r_close=0, conn=8, min_pixels=2, Z=Z, split=rec(), labels=labels, fields=fields, found=found,
                dist2=dist2, cores=cores)
    order = list(base)
    p = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
    assert lib.s2sr_fields_split_i16(bare._h, *[p(base[k]) for k in order]) == 0
    compare({"labels": labels, "fields": fields, "found": int(found[0]), "dist2": dist2, "cores": cores}, want, "the raw call")
    alone = np.zeros((H, W), np.uint16)
    assert lib.s2sr_fields_split_i16(bare._h, *[p(dict(base, labels=alone, fields=None, found=None, dist2=None, cores=None)[k]) for k in order]) == 0
    same(alone, want["labels"], "labels without the other outputs")
    refusals = [dict(idx=None), dict(labels=None), dict(H=0), dict(W=0), dict(H=-1), dict(W=-5), dict(H=65536, W=32768), dict(lo=-32768), dict(hi=32768),
                dict(lo=HI, hi=LO), dict(lo=5, hi=4), dict(r_open=-1), dict(r_open=9), dict(r_close=-1), dict(r_close=9), dict(conn=0), dict(conn=6),
                dict(conn=-4), dict(min_pixels=0), dict(min_pixels=-3), dict(Z=0), dict(Z=65536), dict(Z=-1)]
    refusals += [dict(split=rec(**{k: v})) for k, v in (("core_q", 0), ("core_q", 1001), ("core_q", -1), ("core_px", -1), ("core_px", 256), ("edge", -1),
                                                         ("edge", 32768), ("edge_r", -1), ("edge_r", 5))]
    for bad in refusals:
        args = dict(base, **bad)
        assert lib.s2sr_fields_split_i16(bare._h, *[p(args[k]) for k in order]) == -1, list(bad)
        check(bare, H, W, "blobs", EDGE, **kw)
    # with NULL for the split the plain entry's refusals come through
    for bad in (dict(conn=5), dict(Z=0), dict(idx=None)):
        args = dict(base, split=None, **bad)
        assert lib.s2sr_fields_split_i16(bare._h, *[p(args[k]) for k in order]) == -1, list(bad)
    for bad in (idx.astype(np.int32), idx.astype(np.uint16), idx.ravel()):                 # the Python layer's own
        with pytest.raises(TypeError):
            bare.fields_split_i16(bad, LO, HI, split=EDGE)
    with pytest.raises(ValueError, match="unknown key"):
        bare.fields_split_i16(idx, LO, HI, split={"core": 0.5})
    with pytest.raises(ValueError, match="unknown output"):
        bare.fields_split_i16(idx, LO, HI, split=EDGE, want=("dist",))
    with pytest.raises(native.S2srError, match="core_q"):
        bare.fields_split_i16(idx, LO, HI, split={"core_q": 0})
    with pytest.raises(native.S2srError, match="edge_r"):
        bare.fields_split_i16(idx, LO, HI, split={"edge_r": 5})
    assert lib.s2sr_debug_fields_split_stage_ms(bare._h, None, None, None) == -1
    check(bare, H, W, "blobs", EDGE, **kw)


def test_the_call_voids_the_kept_image():
    """the void rule of csrc/scratch.h: the call requests scratch, so the uint16 image the door before it kept is gone"""
    e = gpu_engines.default(1, HP)
    H, W = 9, 11
    rng = np.random.default_rng(3)
    img = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
    b = rng.integers(0, 65536, (4 * H, 4 * W)).astype(np.uint16)
    split = {"core_q": 500, "core_px": 1, "edge": 900, "edge_r": 1}
    with e.chain_lock:
        e.enhance_u16(img, tile=16, pad=3)
        first = np.array(e.index_nd_u16(None, b, ca=2)["index"])                           # the kept image serves
        labels, fields, found = e.fields_split_i16(first, -2000, 2000, conn=8, min_pixels=2, split=split)
        labels = np.array(labels)
        with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
            e.index_nd_u16(None, b, ca=2)
        e.enhance_u16(img, tile=16, pad=3)
        same(np.array(e.index_nd_u16(None, b, ca=2)["index"]), first, "the chain works again")
    want = sm.split(first, -2000, 2000, conn=8, min_pixels=2, split=split)
    same(labels, want["labels"], "labels on the shared engine")
    same(fields, want["fields"], "fields on the shared engine")
    assert found == want["found"] and found > 0


# ---- the job -------------------------------------------------------------------------------------------------------------------------------------
def _patch_weights(monkeypatch, tmp_path, nb_by_name):
    """Seeded synthetic checkpoints where the drop-in looks for them (tests/test_gpu_app.py)."""
    import torch

    from s2sr.weights import synthetic_state_dict
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir(exist_ok=True)
    for name, nb in nb_by_name.items():
        sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(nb, seed=0).items()}
        torch.save({"params_ema": sd}, tmp_path / "models" / f"{name}.pth")


def test_the_wow_job_splits_the_fields_it_segments(monkeypatch, tmp_path):
    """the 24 x 20 UTM GeoTIFF of the fields job test with two touching NIR blocks of different brightness: with "split" in the segment
    option <stem>_zones.tif is the model's split of the job's own NDVI file, the GeoJSON has one Feature per split field and the
    metadata's parameters carry "split"; without the key the labels are the plain model's and the parameters are today's"""
    from app.wow_sr import process_wow_sr
    from s2sr import rasterio_lite as rio
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    H, W = 24, 20
    rng = np.random.default_rng(52)
    four = rng.integers(1000, 4000, size=(H, W, 4)).astype(np.uint16)
    four[4:20, 2:10, 3] += 9000                                    # two bright NIR blocks side by side: one blob of the mask
    four[4:20, 10:18, 3] += 3500
    g = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0),
                    rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633)})
    src = tmp_path / "scene4.tif"
    rio.write_geotiff_u16(src, four, g)
    common = dict(enhance_crops=False, model="realesrgan_anime", bit_depth=16, indices=["ndvi"])
    seg = {"index": "ndvi", "min": 0.15, "max": None, "open": 1, "close": 2, "connectivity": 4, "min_pixels": 12}
    split = {"core": 0.4, "core_px": 2, "edge": 0.04, "edge_smooth": 1}
    res = process_wow_sr(src, tmp_path / "split", zones={"segment": dict(seg, split=split)}, **common)
    plain = process_wow_sr(src, tmp_path / "plain", zones={"segment": seg}, **common)
    ndvi = rio.read_bands_raw(tmp_path / "split" / "scene4_wow_sr_ndvi.tif")[0][..., 0]
    assert ndvi.dtype == np.int16 and ndvi.shape == (96, 80)
    assert (tmp_path / "plain" / "scene4_wow_sr_ndvi.tif").read_bytes() == (tmp_path / "split" / "scene4_wow_sr_ndvi.tif").read_bytes()
    kw = dict(r_open=1, r_close=2, conn=4, min_pixels=12)
    params = {"core_q": 400, "core_px": 2, "edge": 400, "edge_r": 1}
    want = sm.split(ndvi, 1500, 32767, split=params, **kw)
    want_plain = fm.segment(ndvi, 1500, 32767, **kw)
    print("fields with the split", want["found"], "without", want_plain[2])
    assert want["found"] >= want_plain[2] >= 1
    for d, labels, n in (("split", want["labels"], want["found"]), ("plain", want_plain[0], want_plain[2])):
        arr, zg = rio.read_bands_raw(tmp_path / d / "scene4_wow_sr_zones.tif")
        assert arr.dtype == np.uint16 and arr.shape == (96, 80, 1) and zg.nodata == 0
        same(arr[..., 0], labels, f"{d}: the zones GeoTIFF against the model")
        fc = json.load(open(tmp_path / d / "scene4_wow_sr_fields.geojson"))
        assert [f["properties"]["label"] for f in fc["features"]] == list(range(1, n + 1))
    today = {"name": "ndvi", "K": 10000, "lo": 1500, "hi": 32767, "r_open": 1, "r_close": 2, "conn": 4, "min_pixels": 12}
    assert plain["sr_metadata"]["zones"]["parameters"] == today
    assert res["sr_metadata"]["zones"]["parameters"] == dict(today, split=params)
    assert res["sr_metadata"]["zones"]["found"] == want["found"]
    assert [r["pixels"] for r in res["sr_metadata"]["zones"]["labels"]] == want["fields"][1:want["found"] + 1, 0].tolist()
    rows = res["sr_metadata"]["indices"][0]["zones"]
    assert [r["zone"] for r in rows][-1] == want["found"]
