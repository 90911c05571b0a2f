"""Fields from the image on the GPU (include/s2sr.h: s2sr_fields_segment_i16, s2sr_labels_trace_u16; csrc/fields.hip):
labels, fields and found byte for byte against tests/fields_model.py on shapes that cross the 64 x 64 tile lines and patterns chosen
to break a union-find; every parameter; the independence of the number of workgroups (caps 1 and 3, with the launch and trip
arithmetic); every refusal, the void rule, the round trip through the ring tracer and the polygon rasteriser, and the job that segments
its own NDVI.  The entry under red zones, poison, stalls and cap 8: its rows of tests/doors.py, whose baselines this module holds to
the model.

The pass's capped launches are counted in the grid-cap family "display", as the index and zones passes' are."""
import json

import numpy as np
import pytest

import diag
import doors
import fields_model as fm
import gpu_engines
import zones_model as zm
from diag import same_values as same
from fields_model import HI, LO, case, raster
from s2sr import native

pytestmark = pytest.mark.gpu

HP = native.PREC_F16_HP
# one pixel, one row across two tile lines, one short of / one past a tile, exactly one tile, 2 x 3 and 3 x 4 tiles with ragged edges
# (and the widths of the SR grid, tests/doors.py WIDTHS: at W % 8 == 0 the mask, morphology and label kernels move 8 and 16 bytes a lane)
SHAPES = [(1, 1), (1, 130), (63, 65), (64, 64), (65, 129), (130, 197)] + doors.WIDTHS
PATTERNS = ("spiral", "checker", "comb", "rings", "noise", "ones", "zeros", "stripes", "blobs")
GRID_FAMILY = "display"


@pytest.fixture(scope="module")
def bare():
    with gpu_engines.bare(precision=HP) as e:                    # the entry needs no weights
        yield e


def check(e, H, W, name, **kw):
    want_labels, want_fields, want_found = case(H, W, name, **kw)
    labels, fields, found = e.fields_segment_i16(raster(H, W, name), LO, HI, **kw)
    what = f"{H} x {W} {name} {kw}"
    assert found == want_found, f"{what}: found {found} against {want_found}"
    same(np.array(labels), want_labels, f"{what}: labels")
    same(fields, want_fields, f"{what}: fields")
    assert int(fields[:, 0].sum()) == H * W
    return want_found


@pytest.mark.parametrize("H,W", SHAPES)
def test_byte_for_byte_against_the_model(bare, H, W):
    """every pattern under both connectivities: the spiral is one component through every tile, the checkerboard H W / 2 components
    or one, the comb's teeth hang on its last row"""
    found = {}
    for name in PATTERNS:
        for conn in (4, 8):
            found[name, conn] = check(bare, H, W, name, conn=conn)
    assert found["spiral", 4] == found["ones", 4] == 1 and found["zeros", 8] == 0
    assert found["comb", 4] == (1 if H > 1 else (W + 1) // 2)      # (one row: the teeth have no back to hang on)
    assert found["checker", 4] == (H * W + 1) // 2 and found["checker", 8] == (1 if min(H, W) > 1 else (H * W + 1) // 2)
    if H * W > 4096:
        assert found["noise", 4] > found["noise", 8] > 10 and found["rings", 4] > 5


@pytest.mark.parametrize("H,W", [(65, 129), (130, 197), (65, 128)])
def test_every_parameter(bare, H, W):
    """min_pixels of 1 and above, a Z below found (found still counts them), radii 0, 1, 2 and 8 on fields that touch every edge
    (65 x 128: the same in 8-byte masks and 16-byte labels, a tile line between two vector groups)"""
    for name in ("noise", "blobs"):
        for conn in (4, 8):
            for min_pixels in (2, 7, 400):
                check(bare, H, W, name, conn=conn, min_pixels=min_pixels)
            n = check(bare, H, W, name, conn=conn, min_pixels=2, Z=5)
            assert n > 5
            check(bare, H, W, name, conn=conn, Z=1)
    for r_open, r_close in ((1, 0), (0, 1), (1, 2), (2, 1), (2, 2), (8, 0), (0, 8), (8, 8)):
        for name in ("blobs", "stripes", "noise"):
            check(bare, H, W, name, r_open=r_open, r_close=r_close, conn=4 if r_open & 1 else 8, min_pixels=3)
    # the morphology does what it is for: the opened and closed blobs are fewer and larger, and they still touch every edge
    labels, fields, n = case(H, W, "blobs", r_open=1, r_close=2, conn=8, min_pixels=3)
    assert 3 < n < case(H, W, "blobs", conn=8)[2]
    assert labels[0].any() and labels[-1].any() and labels[:, 0].any() and labels[:, -1].any()
    assert not labels[raster(H, W, "blobs") == fm.NODATA].any()


def test_radii_on_the_small_shapes(bare):
    for H, W in ((1, 1), (1, 130), (63, 65), (64, 64), (5, 8), (65, 128), (1, 68)):
        for r_open, r_close in ((1, 1), (2, 8), (8, 2)):
            for name in ("blobs", "ones", "stripes"):
                check(bare, H, W, name, r_open=r_open, r_close=r_close, conn=8)


@pytest.mark.parametrize("cap", [1, 3])
def test_under_capped_grids(bare, cap):
    """the same bytes with every workgroup on several trips: 130 x 197 pixels are 3 x 4 tiles, 26 numbering chunks"""
    H, W = 130, 197
    for name, kw in (("spiral", dict(conn=4)), ("noise", dict(conn=8, min_pixels=2)), ("blobs", dict(r_open=1, r_close=2, conn=4))):
        with diag.under(cap):
            check(bare, H, W, name, **kw)
            launches, trips = native.grid_cap_stats()[GRID_FAMILY]
        # mask, local, border, flatten, count, apply, labels (and the morphology's 8 passes and the nodata mask where it runs)
        assert launches == (7 + 9 if "r_open" in kw else 7), (name, launches)
        assert trips == -(-101 // cap), (name, trips)           # the most trips are the flatten pass's: 25610 pixels, 256 a workgroup
    native.grid_cap_stats(reset=True)
    check(bare, H, W, "spiral", conn=4)
    assert native.grid_cap_stats()[GRID_FAMILY] == (0, 0)                                  # off means off


def test_stage_times_by_events(bare):
    """s2sr_debug_fields_stage_ms: every launch of a profiled call is booked to its stage, and the bytes are the unprofiled call's;
    no figure is asserted beyond its sign"""
    H, W = 130, 197
    kw = dict(r_open=1, r_close=2, conn=8, min_pixels=3)
    check(bare, H, W, "blobs", **kw)
    assert all(v == (0.0, 0) for v in bare.fields_stage_ms().values()), "a call without profiling leaves no stage times"
    bare.set_profiling(1)
    bare.reset_kernel_stats()
    try:
        check(bare, H, W, "blobs", **kw)
        per = bare.fields_stage_ms()
        total = bare.kernel_stats()["index"]
        check(bare, H, W, "spiral", conn=4)
        bare_per = bare.fields_stage_ms()
        bare.kernel_stats()
    finally:
        bare.set_profiling(0)
    assert list(per) == list(native.FIELDS_STAGES)
    assert [n for _, n in per.values()] == [10, 1, 1, 1, 1, 1, 1, 1] and [n for _, n in bare_per.values()] == [1] * 8
    assert all(ms > 0 for ms, _ in per.values()) and int(total["launches"]) == 17
    assert abs(sum(ms for ms, _ in per.values()) - float(total["total_ms"])) < 1e-3 * max(1.0, float(total["total_ms"]))
    check(bare, H, W, "blobs", **kw)
    assert all(v == (0.0, 0) for v in bare.fields_stage_ms().values())


def test_every_refusal_returns_minus_one_and_leaves_the_next_call_intact(bare):
    H, W = 63, 65
    idx = np.ascontiguousarray(raster(H, W, "blobs"))
    kw = dict(conn=8, min_pixels=2)
    want_labels, want_fields, want_found = case(H, W, "blobs", **kw)
    lib = native.load_library()
    Z = 65535
    labels, fields, found = np.zeros((H, W), np.uint16), np.zeros((Z + 1, 6), np.int64), np.zeros(1, np.uint64)
    base = dict(idx=idx, H=H, W=W, lo=LO, hi=HI, r_open=0, r_close=0, conn=8, min_pixels=2, Z=Z, labels=labels, fields=fields, found=found)
    order = list(base)
    p = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
    assert lib.s2sr_fields_segment_i16(bare._h, *[p(base[k]) for k in order]) == 0
    same(labels, want_labels, "the raw call: labels")
    same(fields, want_fields, "the raw call: fields")
    assert int(found[0]) == want_found
    alone = np.zeros((H, W), np.uint16)
    assert lib.s2sr_fields_segment_i16(bare._h, *[p(dict(base, labels=alone, fields=None, found=None)[k]) for k in order]) == 0
    same(alone, want_labels, "labels without fields and found")
    refusals = [dict(idx=None), dict(labels=None), dict(H=0), dict(W=0), dict(H=-1), dict(W=-5), dict(H=65536, W=32768), dict(lo=-32768), dict(hi=32768),
                dict(lo=HI, hi=LO), dict(lo=5, hi=4), dict(r_open=-1), dict(r_open=9), dict(r_close=-1), dict(r_close=9), dict(conn=0), dict(conn=6),
                dict(conn=-4), dict(min_pixels=0), dict(min_pixels=-3), dict(Z=0), dict(Z=65536), dict(Z=-1)]
    for bad in refusals:
        args = dict(base, **bad)
        assert lib.s2sr_fields_segment_i16(bare._h, *[p(args[k]) for k in order]) == -1, list(bad)
        check(bare, H, W, "blobs", **kw)
    for bad in (idx.astype(np.int32), idx.astype(np.uint16), idx.ravel()):                 # the Python layer's own
        with pytest.raises(TypeError):
            bare.fields_segment_i16(bad, LO, HI)
    with pytest.raises(native.S2srError, match="conn"):
        bare.fields_segment_i16(idx, LO, HI, conn=5)
    # the tracer's refusals and its capacity protocol
    counts = np.zeros(2, np.uint64)
    lab = np.ascontiguousarray(want_labels)
    for bad in (dict(labels=None), dict(H=0), dict(W=-1), dict(Z=0), dict(Z=65536), dict(counts=None)):
        a = dict(dict(labels=lab, H=H, W=W, Z=Z, counts=counts), **bad)
        assert lib.s2sr_labels_trace_u16(bare._h, p(a["labels"]), a["H"], a["W"], a["Z"], 0, 0, None, None, None, p(a["counts"])) == -1, list(bad)
    assert lib.s2sr_labels_trace_u16(bare._h, p(lab), H, W, Z, 0, 0, None, None, None, p(counts)) == 0
    xy, ring_start, ring_label = fm.trace(lab, Z)
    assert counts.tolist() == [len(xy), len(ring_label)] and len(ring_label) >= want_found
    small = np.full((len(xy), 2), -7, np.int32)
    rs, rl = np.full(len(ring_label) + 1, -7, np.int32), np.full(len(ring_label), 7, np.uint16)
    assert lib.s2sr_labels_trace_u16(bare._h, p(lab), H, W, Z, len(xy) - 1, len(ring_label), p(small), p(rs), p(rl), p(counts)) == 0
    assert (small == -7).all() and (rs == -7).all() and counts.tolist() == [len(xy), len(ring_label)]          # too small: nothing written
    check(bare, H, W, "blobs", **kw)


def test_the_call_voids_the_kept_image():
    """the void rule of csrc/scratch.h: the call requests scratch, so the uint16 image the door before it kept is gone"""
    e = gpu_engines.default(1, HP)
    H, W = 9, 11
    rng = np.random.default_rng(3)
    img = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
    b = rng.integers(0, 65536, (4 * H, 4 * W)).astype(np.uint16)
    with e.chain_lock:
        e.enhance_u16(img, tile=16, pad=3)
        first = np.array(e.index_nd_u16(None, b, ca=2)["index"])                           # the kept image serves
        labels, fields, found = e.fields_segment_i16(first, -2000, 2000, conn=8, min_pixels=2)
        labels = np.array(labels)
        with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
            e.index_nd_u16(None, b, ca=2)
        q = np.array(e.enhance_u16(img, tile=16, pad=3))
        same(np.array(e.index_nd_u16(None, b, ca=2)["index"]), first, "the chain works again")
        # the labels as a caller's array: zonal sums from them
        z = e.index_nd_u16(q, b, ca=2, zones=labels, Z=max(found, 1), want=("zonal",))["zonal"]
    want = fm.segment(first, -2000, 2000, conn=8, min_pixels=2)
    same(labels, want[0], "labels on the shared engine")
    same(fields, want[1], "fields on the shared engine")
    assert found == want[2] and found > 0 and z[1:, 0].tolist() == fields[1:found + 1, 0].tolist()


@pytest.mark.parametrize("ident", doors.owned("fields_segment_i16"))
def test_the_door_table_s_baseline_is_the_model(ident):
    """tests/doors.py's rows of this pass: the red-zone, poison, stall and grid-cap matrices hold every mode to diag.baseline, and
    this holds the baseline to the model, sample for sample"""
    same(diag.baseline(ident), doors.MODELS[ident](), ident)


def _tables(labels, Z, engine):
    xy, ring_start, ring_label = engine.labels_trace_u16(labels, Z)
    mxy, mrs, mrl = fm.trace(labels, Z)
    same(xy, mxy, "the rings' vertices against the model")
    same(ring_start, mrs, "ring_start against the model")
    same(ring_label, mrl, "ring_label against the model")
    return xy, ring_start, ring_label


def test_round_trip_through_the_tracer_and_the_rasteriser(bare):
    """every ring a feature of its own with its ring's label: with the even-odd rule per feature and later features winning, holes
    have to be cut out, so a label's rings form ONE feature; labels ascend, and no two labels overlap"""
    for H, W, name, kw in ((130, 197, "blobs", dict(r_open=1, r_close=1, conn=4, min_pixels=2)), (65, 129, "noise", dict(conn=4)),
                           (63, 65, "rings", dict(conn=8)), (1, 1, "ones", {}), (64, 64, "checker", dict(conn=4, Z=100))):
        labels = np.array(bare.fields_segment_i16(raster(H, W, name), LO, HI, **kw)[0])
        Z = kw.get("Z", 65535)
        xy, ring_start, ring_label = _tables(labels, Z, bare)
        if len(ring_label) == 0:
            continue
        change = np.flatnonzero(np.diff(ring_label.astype(np.int64))) + 1
        feat_start = np.concatenate([[0], change, [len(ring_label)]]).astype(np.int32)
        feat_label = ring_label[feat_start[:-1]]
        burnt, area = bare.zones_rasterize_u16((xy * 256).astype(np.int32), ring_start, feat_start, feat_label, Z, (H, W))
        same(np.array(burnt), labels, f"{H} x {W} {name}: the rings burn back to the labels")


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


def test_the_wow_job_segments_its_own_ndvi(monkeypatch, tmp_path):
    """the 24 x 20 UTM GeoTIFF of 4 bands of the zones job test: <stem>_zones.tif is the model's labels of the job's own NDVI file, the
    GeoJSON's features burn back to them, the per-zone tables are those of a second job handed the label raster, and without the
    option no new file or block appears"""
    from app.wow_sr import process_wow_sr
    from s2sr import fields as xf
    from s2sr import rasterio_lite as rio
    from s2sr import zones as xz
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    H, W = 24, 20
    rng = np.random.default_rng(52)
    four = rng.integers(1000, 4000, size=(H, W, 4)).astype(np.uint16)
    four[6:18, 4:15, 3] += 2500                                    # a bright NIR block: a field among the noise
    x0, y0 = 600000.0, 5100000.0
    g = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, x0, y0, 0.0),
                    rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633)})
    src = tmp_path / "scene4.tif"
    rio.write_geotiff_u16(src, four, g)
    common = dict(enhance_crops=False, model="realesrgan_anime", bit_depth=16, indices=["ndvi", "ndwi"])
    option = {"segment": {"index": "ndvi", "min": 0.15, "max": None, "open": 1, "close": 2, "connectivity": 8, "min_pixels": 12}}
    res = process_wow_sr(src, tmp_path / "seg", zones=option, **common)
    none = process_wow_sr(src, tmp_path / "none", **common)
    # the labels: the model's of the job's own NDVI file
    ndvi = rio.read_bands_raw(tmp_path / "seg" / "scene4_wow_sr_ndvi.tif")[0][..., 0]
    assert ndvi.dtype == np.int16 and ndvi.shape == (96, 80)
    want_labels, want_fields, want_found = fm.segment(ndvi, 1500, 32767, r_open=1, r_close=2, conn=8, min_pixels=12)
    assert 1 <= want_found < 200
    ztif = tmp_path / "seg" / "scene4_wow_sr_zones.tif"
    arr, zg = rio.read_bands_raw(ztif)
    assert arr.dtype == np.uint16 and arr.shape == (96, 80, 1) and zg.nodata == 0 and zg.pixel_size == (2.5, 2.5)
    same(arr[..., 0], want_labels, "the zones GeoTIFF against the model")
    # the block and the outputs
    block = res["sr_metadata"]["zones"]
    gj = tmp_path / "seg" / "scene4_wow_sr_fields.geojson"
    assert block["source"] == "segment" and block["found"] == want_found and block["file"] == str(ztif) and block["geojson"] == str(gj)
    assert block["parameters"] == {"name": "ndvi", "K": 10000, "lo": 1500, "hi": 32767, "r_open": 1, "r_close": 2, "conn": 8, "min_pixels": 12}
    assert block["labels"] == [{"label": l, "pixels": int(want_fields[l, 0]), "area_ha": int(want_fields[l, 0]) * (6.25 / 10000.0),
                                "bbox": [int(v) for v in want_fields[l, 2:6]]} for l in range(1, want_found + 1)]
    assert block["grid"] == [96, 80] and block["unlabelled"] == int(want_fields[0, 0])
    assert res["outputs"]["zones_tif"] == str(ztif) and res["outputs"]["fields_geojson"] == str(gj)
    assert json.load(open(tmp_path / "seg" / "scene4_wow_sr_metadata.json"))["sr_metadata"]["zones"] == json.loads(json.dumps(block))
    # the GeoJSON's features burn back to the labels, through the policy and the rasteriser's model of 7.9
    fc = json.load(open(gj))
    assert [f["properties"]["label"] for f in fc["features"]] == list(range(1, want_found + 1))
    grid = xz.to_grid(xz.read(gj), g, (H, W), 4)
    assert grid["grid"] == (96, 80) and grid["dropped"] == 0
    burnt = zm.rasterize(zm.from_tables(grid["xy"], grid["ring_start"], grid["feat_start"], list(range(1, want_found + 1))), want_found, 96, 80)[0]
    same(burnt, want_labels, "the GeoJSON burnt back")
    # the per-zone tables: those of a second job handed the label raster; every other byte and entry is what it is without the option
    ref = process_wow_sr(src, tmp_path / "raster", zones=want_labels, **common)
    for name in ("scene4_wow_sr.tif", "scene4_wow_sr_ndvi.tif", "scene4_wow_sr_ndvi.png", "scene4_wow_sr_ndwi.tif", "scene4_wow_sr_ndwi.png"):
        assert (tmp_path / "seg" / name).read_bytes() == (tmp_path / "raster" / name).read_bytes() == (tmp_path / "none" / name).read_bytes(), name
    for k in range(2):
        m, m_ref = res["sr_metadata"]["indices"][k], ref["sr_metadata"]["indices"][k]
        assert m["zones"] == m_ref["zones"] and [r["zone"] for r in m["zones"]][-1] == want_found and "zones" not in none["sr_metadata"]["indices"][k]
        rows = {r["zone"]: r for r in m["zones"]}
        for f in fc["features"]:
            assert f["properties"][m["name"]] == {"mean": rows[f["properties"]["label"]]["mean"], "std": rows[f["properties"]["label"]]["std"]}
    strip = lambda d: {k: v for k, v in d.items() if k not in ("indices", "output_file", "zones")}
    assert strip(res["sr_metadata"]) == strip(ref["sr_metadata"]) == strip(none["sr_metadata"])
    for other, d in ((ref, "raster"), (none, "none")):                                     # a label raster, or no zones: no such file or block
        assert "zones" not in other["sr_metadata"] and "zones_tif" not in other["outputs"] and "fields_geojson" not in other["outputs"]
        assert not list((tmp_path / d).glob("*_zones.tif")) and not list((tmp_path / d).glob("*.geojson"))
    # the refusals that need the raster: no field found, and found beyond 65535 is the same message's sibling (s2sr/fields.py)
    with pytest.raises(ValueError, match="found no field"):
        process_wow_sr(src, tmp_path / "empty", zones={"segment": {"index": "ndvi", "min": 0.99, "min_pixels": 1}}, **common)
    assert not (tmp_path / "empty").exists() or not list((tmp_path / "empty").glob("*"))
