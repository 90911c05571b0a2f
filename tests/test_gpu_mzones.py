"""Management zones on the GPU (include/s2sr.h: s2sr_zones_kmeans_i16; csrc/mzones.hip): zone, table, centres,
status and iterations byte for byte against tests/mzones_model.py on shapes that cross the 64 x 32 tile lines, for every pair of
feature pattern and label layout, and at the widths of the SR grid (doors.WIDTHS: W % 8 == 0 takes the 16-byte loads of labels and
features and the 8-byte loads and stores of zones, every other width the scalar forms); every parameter; the independence of the row
bands and of the number of workgroups (caps 1 and 3, with the launch and trip arithmetic); every refusal, the void rule, the round
trip through the segmentation, the ring tracer and the polygon rasteriser, and one whole job against the model.  The entry under red
zones, poison, stalls and cap 8: its rows of tests/doors.py, whose baselines this module holds to the model.

The pass's capped launches are counted in the grid-cap family "display", as the index, zones and fields passes' are."""
import json

import numpy as np
import pytest

import diag
import doors
import fields_model as fm
import gpu_engines
import mzones_model as mm
from diag import same_values as same
from s2sr import native

pytestmark = pytest.mark.gpu

HP = native.PREC_F16_HP
# one pixel, one row across two tile lines, one short of / one past a tile, exactly one tile column, 3 x 3 and 5 x 4 tiles with ragged edges
# (and the widths of the SR grid: tests/doors.py WIDTHS)
SHAPES = [(1, 1), (1, 130), (63, 65), (64, 64), (65, 129), (130, 197)] + doors.WIDTHS
GRID_FAMILY = "display"
KEYS = ("zone", "table", "centres", "status")


@pytest.fixture(scope="module")
def bare():
    with gpu_engines.bare(precision=HP) as e:                    # the entry needs no weights
        yield e


def check(e, H, W, features, lay, Z=None, band_rows=0, **kw):
    feats, labels, Z0 = mm.inputs(H, W, features, lay)
    Z = Z0 if Z is None else Z
    want = mm.case(H, W, features, lay, Z=Z, **kw)
    got = e.zones_kmeans_i16(feats, labels, Z, band_rows=band_rows, **kw)
    what = f"{H} x {W} {features} on {lay}, Z {Z}, band_rows {band_rows}, {kw}"
    assert got["iterations"] == want["iterations"], f"{what}: {got['iterations']} iterations against {want['iterations']}"
    for key in KEYS:
        same(np.array(got[key]), want[key], f"{what}: {key}")
    return want


@pytest.mark.parametrize("H,W", SHAPES)
def test_byte_for_byte_against_the_model(bare, H, W):
    """every feature pattern on every label layout, one smoothing pass behind the zones"""
    zoned = 0
    for features in mm.FEATURES:
        for lay in mm.LAYOUTS:
            want = check(bare, H, W, features, lay, min_per_zone=2, smooth=1)
            zoned += int((want["status"] == 2).sum())
            if lay == "zeros":
                assert not want["zone"].any() and not want["status"].any()
            if features == "constant":
                assert want["zone"].max() <= 1 and want["iterations"] == 1
    assert zoned >= (1 if H * W >= 6 else 0)


@pytest.mark.parametrize("H,W", [(65, 129), (130, 197), (65, 128)])
def test_every_parameter(bare, H, W):
    """(65 x 128: every parameter on the vector path -- k 8, D 4, smooth 4 and Z below the largest label among them)"""
    for k in (2, 3, 8):
        for lay in ("grid16", "stripes", "one"):
            check(bare, H, W, "noise", lay, k=k, smooth=1)
            check(bare, H, W, ("planted", "nodata"), lay, k=k)
    for names in (("ramp",), ("noise", "ramp"), ("planted", "noise", "nodata", "extremes")):
        for k in (3, 8):
            check(bare, H, W, names, "grid16", k=k, min_per_zone=1, smooth=1)
            check(bare, H, W, names, "checker", k=k)
    for iters in (1, 2, 32):
        w = check(bare, H, W, "noise", "one", iters=iters)
        assert w["iterations"] == min(iters, mm.case(H, W, "noise", "one")["iterations"])
        check(bare, H, W, ("nodata", "planted"), "grid16", iters=iters)
    for min_per_zone in (1, 10, 5000):
        w = check(bare, H, W, "nodata", "grid16", min_per_zone=min_per_zone)
        check(bare, H, W, "extremes", "one", min_per_zone=min_per_zone)
    assert (w["status"][1:] == 1).all() and not w["zone"].any()                             # 5000 a zone: every field is skipped
    for smooth in (0, 1, 4):
        check(bare, H, W, "noise", "grid16", smooth=smooth)
        check(bare, H, W, "planted", "checker", smooth=smooth, k=2)
    labels, Z = mm.layout(H, W, "grid16")
    for Z_low in (1, Z // 2, Z - 1):                               # Z below the largest label
        w = check(bare, H, W, "noise", "grid16", Z=Z_low, smooth=1)
        assert not w["zone"][labels > Z_low].any()


def test_the_bytes_do_not_depend_on_the_row_bands(bare):
    """(65 x 128: every band starts on a multiple of 8 bytes of every plane and is read and written in vectors; 37 x 180: no vectors)"""
    for H, W in ((65, 129), (130, 197), (65, 128), (37, 180)):
        for band_rows in (0, 1, 7):
            check(bare, H, W, ("noise", "nodata"), "grid16", band_rows=band_rows, smooth=2, min_per_zone=3)
            check(bare, H, W, "ramp", "stripes", band_rows=band_rows, smooth=1, k=4)


def launches_and_trips(H, W, cap, Z, k, iterations, smooth):
    """Tiles of 64 x 32 for the passes with sums (130 x 197: 5 x 4), blocks of 256 groups of 8 pixels for the final assignment and for
    a pass of the mode filter (130 x 197: 13), and the tables' blocks of 256 fields or cells; a launch is counted where the cap made
    its grid smaller"""
    blocks = lambda n: -(-n // 256)
    cells, tiles, groups = blocks((Z + 1) * k), -(-H // 32) * -(-W // 64), blocks(H * -(-W // 8))
    grids = [blocks(Z + 1), tiles, cells] + [tiles, cells] * iterations + [cells, groups] + [groups] * smooth + [tiles]
    counted = [g for g in grids if g > cap]
    return len(counted), max(-(-g // cap) for g in counted)


@pytest.mark.parametrize("cap", [1, 3])
def test_under_capped_grids(bare, cap):
    """the same bytes with every workgroup on several trips: 130 x 197, and 65 x 128 and 37 x 180 (6 tiles and 5 and 4 blocks of
    groups: two trips at the least under either cap, on the vector path and beside it)"""
    for H, W in ((130, 197), (65, 128), (37, 180)):
        for features, lay, kw in (("noise", "grid16", dict(smooth=1)), (("planted", "nodata"), "one", dict(k=8, smooth=2)),
                                  ("ramp", "stripes", dict(min_per_zone=1))):
            with diag.under(cap):
                want = check(bare, H, W, features, lay, **kw)
                launches, trips = native.grid_cap_stats()[GRID_FAMILY]
            Z = mm.layout(H, W, lay)[1]
            arithmetic = launches_and_trips(H, W, cap, Z, kw.get("k", 3), want["iterations"], kw.get("smooth", 0))
            assert (launches, trips) == arithmetic and trips >= 2, (H, W, features, lay)
    native.grid_cap_stats(reset=True)
    check(bare, 130, 197, "noise", "grid16", smooth=1)
    assert native.grid_cap_stats()[GRID_FAMILY] == (0, 0)                                  # off means off


@pytest.mark.parametrize("ident", doors.owned("zones_kmeans_i16"))
def test_the_door_table_s_baseline_is_the_model(ident):
    """tests/doors.py's rows of this pass: the red-zone, poison, stall and grid-cap matrices hold every mode to diag.baseline, and
    this holds the baseline to the model, sample for sample"""
    same(diag.baseline(ident), doors.MODELS[ident](), ident)


def test_stage_times_by_events(bare):
    """s2sr_debug_mzones_stage_ms: every launch of a profiled call is booked to its stage; no figure is asserted beyond its sign"""
    H, W = 130, 197
    kw = dict(smooth=2)
    want = check(bare, H, W, "noise", "grid16", **kw)
    assert all(v == (0.0, 0) for v in bare.mzones_stage_ms().values()), "a call without profiling leaves no stage times"
    bare.set_profiling(1)
    bare.reset_kernel_stats()
    try:
        check(bare, H, W, "noise", "grid16", **kw)
        per = bare.mzones_stage_ms()
        bare.kernel_stats()
    finally:
        bare.set_profiling(0)
    assert list(per) == list(native.MZONES_STAGES)
    assert [n for _, n in per.values()] == [3, 2 * want["iterations"], 2, 2, 1] and all(ms > 0 for ms, _ in per.values())
    check(bare, H, W, "noise", "grid16", **kw)
    assert all(v == (0.0, 0) for v in bare.mzones_stage_ms().values())


def test_every_refusal_returns_minus_one_and_leaves_the_next_call_intact(bare):
    H, W = 63, 65
    feats, labels, Z = mm.inputs(H, W, ("noise", "nodata"), "grid16")
    feats, labels = np.ascontiguousarray(feats), np.ascontiguousarray(labels)
    kw = dict(k=3, min_per_zone=2, smooth=1)
    want = mm.case(H, W, ("noise", "nodata"), "grid16", **kw)
    lib = native.load_library()
    zone, table, centres = np.zeros((H, W), np.uint8), np.zeros((Z + 1, 3, 5), np.int64), np.zeros((Z + 1, 3, 2), np.int32)
    status, iterations = np.zeros(Z + 1, np.uint8), np.zeros(1, np.uint32)
    base = dict(feat=feats, D=2, H=H, W=W, labels=labels, Z=Z, k=3, iters=32, min_per_zone=2, smooth=1, band_rows=0, zone=zone, table=table,
                centres=centres, status=status, iterations=iterations)
    order = list(base)
    p = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
    assert lib.s2sr_zones_kmeans_i16(bare._h, *[p(base[n]) for n in order]) == 0
    for key, got in (("zone", zone), ("table", table), ("centres", centres), ("status", status)):
        same(got, want[key], f"the raw call: {key}")
    assert int(iterations[0]) == want["iterations"]
    alone = np.zeros((H, W), np.uint8)
    assert lib.s2sr_zones_kmeans_i16(bare._h, *[p(dict(base, zone=alone, table=None, centres=None, status=None, iterations=None)[n]) for n in order]) == 0
    same(alone, want["zone"], "zone without the optional outputs")
    refusals = [dict(feat=None), dict(labels=None), dict(zone=None), dict(D=0), dict(D=5), dict(D=-1), dict(k=1), dict(k=9), dict(k=0), dict(iters=0),
                dict(iters=65), dict(iters=-1), dict(smooth=-1), dict(smooth=5), dict(Z=0), dict(Z=65536), dict(Z=-1), dict(min_per_zone=0),
                dict(min_per_zone=-7), dict(H=0), dict(W=0), dict(H=-1), dict(W=-5), dict(H=65536, W=32768), dict(band_rows=-1)]
    for bad in refusals:
        args = dict(base, **bad)
        assert lib.s2sr_zones_kmeans_i16(bare._h, *[p(args[n]) for n in order]) == -1, list(bad)
        check(bare, H, W, ("noise", "nodata"), "grid16", **kw)
    for bad_f, bad_l in ((feats.astype(np.int32), labels), (feats.astype(np.uint16), labels), (feats.ravel(), labels), (feats, labels.astype(np.int16)),
                         (feats, labels[:-1])):                    # the Python layer's own
        with pytest.raises(TypeError):
            bare.zones_kmeans_i16(bad_f, bad_l, Z)
    with pytest.raises(native.S2srError, match="k must be"):
        bare.zones_kmeans_i16(feats, labels, Z, k=9)
    check(bare, H, W, ("noise", "nodata"), "grid16", **kw)


def test_the_call_voids_the_kept_image():
    """the void rule of csrc/scratch.h: the call requests scratch, so the uint16 image the door before it kept is gone"""
    e = gpu_engines.default(1, HP)
    H, W = 9, 11
    rng = np.random.default_rng(3)
    img = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
    b = rng.integers(0, 65536, (4 * H, 4 * W)).astype(np.uint16)
    labels = mm.layout(4 * H, 4 * W, "grid16")[0]
    Z = int(labels.max())
    with e.chain_lock:
        e.enhance_u16(img, tile=16, pad=3)
        first = np.array(e.index_nd_u16(None, b, ca=2)["index"])                           # the kept image serves
        got = e.zones_kmeans_i16(first, labels, Z, smooth=1)
        got = {key: np.array(got[key]) for key in KEYS}
        with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
            e.index_nd_u16(None, b, ca=2)
        e.enhance_u16(img, tile=16, pad=3)
        same(np.array(e.index_nd_u16(None, b, ca=2)["index"]), first, "the chain works again")
    want = mm.kmeans(first, labels, Z, smooth=1)
    for key in KEYS:
        same(got[key], want[key], f"{key} on the shared engine")


def test_round_trip_through_the_segmentation_the_tracer_and_the_rasteriser(bare):
    """fields from the raster, zones inside them, a ring trace per zone id: the rings burn back to exactly where(zone == j, labels, 0)"""
    H, W = 130, 197
    idx = fm.raster(H, W, "blobs")
    labels, fields, found = bare.fields_segment_i16(idx, fm.LO, fm.HI, r_open=1, r_close=1, conn=4, min_pixels=12)
    labels = np.array(labels)
    assert found > 3
    feats = np.stack([mm.raster(H, W, "noise"), mm.raster(H, W, "ramp")])
    k = 3
    got = bare.zones_kmeans_i16(feats, labels, found, k=k, min_per_zone=2, smooth=1)
    zone = np.array(got["zone"])
    want = mm.kmeans(feats, labels, found, k=k, min_per_zone=2, smooth=1)
    same(zone, want["zone"], "the zones of the segmented fields")
    same(got["table"], want["table"], "their table")
    assert (got["status"][1:] == 2).sum() > 3
    for j in range(1, k + 1):
        part = np.where(zone == j, labels, 0).astype(np.uint16)
        xy, ring_start, ring_label = bare.labels_trace_u16(part, found)
        assert len(ring_label) > 0
        change = np.flatnonzero(np.diff(ring_label.astype(np.int64))) + 1
        feat_start = np.concatenate([[0], change, [len(ring_label)]]).astype(np.int32)
        burnt, _ = bare.zones_rasterize_u16((xy * 256).astype(np.int32), ring_start, feat_start, ring_label[feat_start[:-1]], found, (H, W))
        same(np.array(burnt), part, f"zone {j}: the rings burn back")


def test_a_wave_lets_its_pending_sums_go_before_they_overflow(bare):
    """64 x 4160 pixels of one field at 32767 under a cap of one workgroup: each wave meets 130 tiles of one label, 66560 pixels, more
    than the 65000 its int32 pending sums may hold (65000 * 32767 < 2^31 < 66560 * 32767)"""
    H, W = 4160, 64
    feats = np.full((2, H, W), 32767, np.int16)
    feats[1] = -32767
    feats[:, ::97, ::5] = mm.raster(H, W, "noise")[::97, ::5]
    labels = np.ones((H, W), np.uint16)
    want = mm.kmeans(feats, labels, 1, k=2, min_per_zone=1)
    with diag.under(1):
        got = bare.zones_kmeans_i16(feats, labels, 1, k=2, min_per_zone=1)
    assert got["iterations"] == want["iterations"]
    for key in KEYS:
        same(np.array(got[key]), want[key], f"one tall field: {key}")
    assert abs(int(want["table"][1, :, 1].sum())) > 2 ** 31


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


def test_the_wow_job_zones_the_fields_it_segments(monkeypatch, tmp_path):
    """the 24 x 20 UTM GeoTIFF of 4 bands of the fields job test with {"manage": ..., "fields": {"segment": ...}}: <stem>_mzones.tif is the
    model's zones of the job's own index files inside the job's own labels, the block is the policy's of the model's outputs, the
    GeoJSON's features burn back to the raster, and every other file is what the job writes for the segment option alone"""
    from app.wow_sr import process_wow_sr
    from s2sr import mzones as xm
    from s2sr import rasterio_lite as rio
    from s2sr import zones as xz
    import zones_model as zm
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    H, W = 24, 20
    rng = np.random.default_rng(52)
    four = rng.integers(1000, 4000, size=(H, W, 4)).astype(np.uint16)
    four[6:18, 4:15, 3] += 2500                                    # a bright NIR block: a field among the noise
    g = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0),
                    rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633)})
    src = tmp_path / "scene4.tif"
    rio.write_geotiff_u16(src, four, g)
    common = dict(enhance_crops=False, model="realesrgan_anime", bit_depth=16, indices=["ndvi", "ndwi"])
    segment = {"segment": {"index": "ndvi", "min": 0.15, "max": None, "open": 1, "close": 2, "connectivity": 8, "min_pixels": 12}}
    manage = {"index": ["ndvi", "ndwi"], "k": 3, "iterations": 32, "min_per_zone": 4, "smooth": 1, "polygons": True}
    res = process_wow_sr(src, tmp_path / "m", zones={"manage": manage, "fields": segment}, **common)
    plain = process_wow_sr(src, tmp_path / "p", zones=segment, **common)
    feats = np.stack([rio.read_bands_raw(tmp_path / "m" / f"scene4_wow_sr_{n}.tif")[0][..., 0] for n in ("ndvi", "ndwi")])
    labels = rio.read_bands_raw(tmp_path / "m" / "scene4_wow_sr_zones.tif")[0][..., 0]
    found = res["sr_metadata"]["zones"]["found"]
    want = mm.kmeans(feats, labels, found, k=3, iters=32, min_per_zone=4, smooth=1)
    assert (want["status"] == 2).sum() >= 1 and len(set(want["zone"].ravel().tolist())) == 4
    mtif, mgj = tmp_path / "m" / "scene4_wow_sr_mzones.tif", tmp_path / "m" / "scene4_wow_sr_mzones.geojson"
    arr, zg = rio.read_bands_raw(mtif)
    assert arr.dtype == np.uint8 and arr.shape == (96, 80, 1) and zg.nodata == 0 and zg.pixel_size == (2.5, 2.5)
    same(arr[..., 0], want["zone"], "the management GeoTIFF against the model")
    params = xm.resolve({"manage": manage, "fields": "x"}, [{"name": "ndvi", "K": 10000}, {"name": "ndwi", "K": 10000}])
    block = dict(res["sr_metadata"]["zones"])
    management = block.pop("management")
    assert management == xm.metadata_block(params, want, xm.zone_rows(want["table"], want["status"], params, (2.5, 2.5)), mtif, mgj)
    assert res["outputs"]["management_tif"] == str(mtif) and res["outputs"]["management_geojson"] == str(mgj)
    fc = json.load(open(mgj))
    for j in (1, 2, 3):
        part = [f for f in fc["features"] if f["properties"]["zone_id"] == j]
        assert part and all(f["properties"]["zone_class"] == ("low", "medium", "high")[j - 1] for f in part)
        grid = xz.to_grid(xz.read({"type": "FeatureCollection", "features": part}), g, (H, W), 4)
        burnt = zm.rasterize(zm.from_tables(grid["xy"], grid["ring_start"], grid["feat_start"], [f["properties"]["label"] for f in part]), found, 96, 80)[0]
        same(burnt, np.where(want["zone"] == j, labels, 0).astype(np.uint16), f"zone {j}: the GeoJSON burnt back")
    # everything else is the segment job's
    swap = lambda d: json.loads(json.dumps(d).replace(str(tmp_path / "m"), str(tmp_path / "p")))
    assert swap(block) == json.loads(json.dumps(plain["sr_metadata"]["zones"]))
    names = sorted(p.name for p in (tmp_path / "p").iterdir())
    assert sorted(p.name for p in (tmp_path / "m").iterdir()) == sorted(names + [mtif.name, mgj.name])
    for name in names:
        if not name.endswith("_metadata.json"):
            assert (tmp_path / "m" / name).read_bytes() == (tmp_path / "p" / name).read_bytes(), name
    assert "management_tif" not in plain["outputs"] and "management" not in plain["sr_metadata"]["zones"]
