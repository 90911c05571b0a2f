"""Management zones without a GPU: the definition's model (tests/mzones_model.py) against planted classes and
against the reference's scikit-learn call, its properties, the host policy (s2sr/mzones.py: every refusal of the option, the rows,
the class names), the job on a stand-in engine that answers with the model, and the C ABI's declaration."""
import json
import re
import threading
from pathlib import Path

import numpy as np
import pytest

import fields_model as fm
import index_model as im
import mzones_model as mm
import zones_model as zm
from s2sr import fields as xf
from s2sr import mzones as xm
from s2sr import native
from s2sr import rasterio_lite as rio
from s2sr import zones as xz

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "s2sr.h").read_text()
N = mm.NODATA
SIZES = (30, 400, 20000)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("mix", sorted(mm.MIXES))
def test_the_model_recovers_planted_classes(mix, D):
    """three levels ten times their noise apart: the fixed point comes in iteration 2 and every pixel has its planted class"""
    for n in SIZES:
        feats, cls = mm.planted((1, n), mix, seed=n, D=D)
        r = mm.kmeans(feats, np.ones((1, n), np.uint16), 1, k=3, min_per_zone=1)
        assert r["iterations"] == 2 and r["status"].tolist() == [0, 2], (mix, n)
        assert (r["zone"] == cls + 1).all(), (mix, n, D)
        assert r["table"][1, :, 0].tolist() == np.bincount(cls.ravel(), minlength=3).tolist()


@pytest.mark.parametrize("mix", sorted(mm.MIXES))
def test_the_model_against_the_reference_s_clustering(mix):
    """KMeans(n_clusters=3, random_state=42, n_init=10), ranked by centre, on the planted case: the same classes exactly"""
    cluster = pytest.importorskip("sklearn.cluster")
    for n in SIZES:
        feats, cls = mm.planted((1, n), mix, seed=n)
        km = cluster.KMeans(n_clusters=3, random_state=42, n_init=10)
        got = km.fit_predict(feats.reshape(-1, 1).astype(np.float64))
        rank = np.argsort(np.argsort(km.cluster_centers_[:, 0]))
        ours = mm.kmeans(feats, np.ones((1, n), np.uint16), 1, k=3, min_per_zone=1)["zone"].ravel()
        assert (rank[got] + 1 == ours).all() and (ours == cls.ravel() + 1).all(), (mix, n)


def test_the_cases_are_real_at_the_widths_of_the_sr_grid():
    """tests/doors.py WIDTHS, which tests/test_gpu_mzones.py zones: at every shape a zoned field (status 2) and more than one zone id
    in the raster, for one raster and for two, on the grid of fields and on the layout that changes its label inside every group"""
    import doors
    for H, W in doors.WIDTHS:
        for features, lay in (("noise", "grid16"), (("noise", "ramp"), "stripes"), ("planted", "one")):
            r = mm.case(H, W, features, lay, min_per_zone=2, smooth=1)
            assert (r["status"] == 2).any() and len(np.unique(r["zone"][r["zone"] > 0])) > 1, (H, W, features, lay)


def test_a_constant_field_ends_in_zone_one():
    r = mm.kmeans(np.full((6, 7), 321, np.int16), np.ones((6, 7), np.uint16), 1, k=4, min_per_zone=1, smooth=2)
    assert (r["zone"] == 1).all() and r["iterations"] == 1 and r["centres"][1].tolist() == [[321]] * 4
    assert r["table"][1].tolist() == [[42, 42 * 321, 42 * 321 * 321], [0, 0, 0], [0, 0, 0], [0, 0, 0]]


def test_empty_clusters_keep_rank_and_centre():
    """two values and four clusters: the two middle start centres catch nothing, stay where they started and keep ranks 2 and 3"""
    v = np.array([[0] * 10 + [900] * 10], np.int16)
    r = mm.kmeans(v, np.ones((1, 20), np.uint16), 1, k=4, min_per_zone=1)
    assert r["centres"][1].ravel().tolist() == [0, 337, 562, 900]                      # 0 + (3 * 900) // 8, (5 * 900) // 8
    assert r["table"][1, :, 0].tolist() == [10, 0, 0, 10] and sorted(set(r["zone"].ravel().tolist())) == [1, 4]
    assert r["iterations"] == 2


def test_half_away_from_zero_and_ties_to_the_smallest_cluster():
    assert mm.rounded_mean(np.array([3, -3, 5, -5, 1, -1]), np.array([2, 2, 2, 2, 3, 3])).tolist() == [2, -2, 3, -3, 0, 0]
    # -10 and 10 start the centres at -5 and 5; the pixel at 0 is as far from both and goes to cluster 0
    r = mm.kmeans(np.array([[-10, 0, 10]], np.int16), np.ones((1, 3), np.uint16), 1, k=2, min_per_zone=1)
    assert r["zone"].tolist() == [[1, 1, 2]] and r["centres"][1].ravel().tolist() == [-5, 10]


def test_skipped_and_absent_fields():
    feats, labels, Z = mm.inputs(65, 129, "nodata", "grid16")
    labels = labels.copy()
    labels[labels == 3] = 0                                        # field 3 is absent
    nod = np.where(labels == 5, N, feats[0])[None]                 # field 5 has pixels and no member
    r = mm.kmeans(nod, labels, Z, k=3, min_per_zone=77)            # 231 members and more: the whole 256-pixel fields with less than a tenth nodata
    assert r["status"][3] == 0 and r["status"][5] == 0 and r["status"][0] == 0 and set(r["status"].tolist()) == {0, 1, 2}
    for l in np.flatnonzero(r["status"] != 2):
        assert not r["table"][l].any() and not r["centres"][l].any() and not r["zone"][labels == l].any()
    lab, mem = mm.members(nod.astype(np.int64), labels, Z)
    zoned = np.isin(lab, np.flatnonzero(r["status"] == 2))
    assert int(r["table"][:, :, 0].sum()) == int((mem & zoned).sum()) and ((r["zone"] > 0) == (mem & zoned)).all()
    n = np.bincount(lab[mem], minlength=Z + 1)
    assert ((r["status"] == 1) == ((n > 0) & (n < 231))).all()


def test_iterations_is_the_first_fixed_point():
    feats, labels, Z = mm.inputs(65, 129, "noise", "one")
    full = mm.kmeans(feats, labels, Z)
    t = full["iterations"]
    assert 2 < t < 32
    for iters in (1, t - 1, t, t + 1, 64):
        r = mm.kmeans(feats, labels, Z, iters=iters)
        assert r["iterations"] == min(iters, t)
        assert (r["centres"] == full["centres"]).all() == (iters >= t - 1)        # iteration t changed nothing: t - 1 had the centres already


def test_smoothing_keeps_zone_zero_and_label_borders():
    feats, labels, Z = mm.inputs(65, 129, "nodata", "checker")
    plain = mm.kmeans(feats, labels, Z, smooth=0)
    for smooth in (1, 4):
        r = mm.kmeans(feats, labels, Z, smooth=smooth)
        assert ((r["zone"] == 0) == (plain["zone"] == 0)).all()
        assert int(r["table"][:, :, 0].sum()) == int((plain["zone"] > 0).sum())
    # a checkerboard of two labels: a pixel's 4-neighbours carry the other label, so no vote crosses; each label smoothed alone
    for l in (1, 2):
        alone = mm.kmeans(feats, np.where(labels == l, labels, 0).astype(np.uint16), Z, smooth=1)
        both = mm.kmeans(feats, labels, Z, smooth=1)
        assert (alone["zone"][labels == l] == both["zone"][labels == l]).all()
    # a lone pixel of zone 2 among zone 1 is voted away, a pixel of zone 0 never is; a tie keeps the own id
    z = np.array([[1, 1, 1], [1, 2, 1], [1, 0, 1]])
    assert mm.smooth_pass(z, np.ones((3, 3), np.int64), 3).tolist() == [[1, 1, 1], [1, 1, 1], [1, 0, 1]]
    assert mm.smooth_pass(np.array([[1, 2]]), np.ones((1, 2), np.int64), 2).tolist() == [[1, 2]]
    assert mm.smooth_pass(np.array([[3, 1, 2]]), np.ones((1, 3), np.int64), 3).tolist() == [[3, 1, 2]]      # own among the tied
    assert mm.smooth_pass(np.array([[3, 3, 1, 2, 2]]), np.ones((1, 5), np.int64), 3)[0, 2] == 1


def test_labels_above_z_count_as_zero():
    feats, labels, Z = mm.inputs(65, 129, "noise", "above")
    assert labels.max() > Z
    r = mm.kmeans(feats, labels, Z, min_per_zone=1)
    assert not r["zone"][labels > Z].any() and r["zone"][(labels <= Z) & (labels > 0)].all() and r["table"].shape == (Z + 1, 3, 3)


# ---- s2sr/mzones.py --------------------------------------------------------------------------------------------------------------------------
DEFS = [{"name": "ndvi", "K": 10000}, {"name": "ndwi", "K": 5000}, {"name": "ndre", "K": 10000}]
GOOD = {"index": "ndvi", "k": 3, "iterations": 32, "min_per_zone": 10, "smooth": 1, "polygons": True}
SEGMENT = {"segment": {"index": "ndvi", "min": 0.3, "min_pixels": 12}}


def test_resolve_fills_the_defaults():
    p = xm.resolve({"manage": {"index": "ndwi"}, "fields": "fields.tif"}, DEFS)
    assert p == {"indices": [1], "names": ["ndwi"], "K": [5000], "k": 3, "iterations": 32, "min_per_zone": 10, "smooth": 1, "polygons": True}
    p = xm.resolve({"manage": {"index": ["ndre", "ndvi"], "k": 8, "iterations": 64, "min_per_zone": 1, "smooth": 0, "polygons": False},
                    "fields": SEGMENT}, DEFS)
    assert p == {"indices": [2, 0], "names": ["ndre", "ndvi"], "K": [10000, 10000], "k": 8, "iterations": 64, "min_per_zone": 1, "smooth": 0,
                 "polygons": False}
    assert xm.is_manage({"manage": {}}) and not xm.is_manage(SEGMENT) and not xm.is_manage("x.geojson") and not xm.is_manage(None)
    assert xm.class_names(3) == ["low", "medium", "high"] and xm.class_names(2) == ["zone_1", "zone_2"] and xm.class_names(5)[-1] == "zone_5"


@pytest.mark.parametrize("change,text", [
    ({"colour": 1}, "unknown key"), ({"index": "evi"}, "not among"), ({"index": ["ndvi", "evi"]}, "not among"), ({"index": None}, "index"),
    ({"index": []}, "index"), ({"index": [1]}, "index"), ({"index": ["ndvi", "ndwi", "ndre", "ndvi"]}, "twice"), ({"index": ["ndvi", "ndvi"]}, "twice"),
    ({"index": ["ndvi", "ndwi", "ndre", "a", "b"]}, "at most 4"), ({"k": 1}, "k"), ({"k": 9}, "k"), ({"k": 3.0}, "k"), ({"k": True}, "k"),
    ({"iterations": 0}, "iterations"), ({"iterations": 65}, "iterations"), ({"smooth": -1}, "smooth"), ({"smooth": 5}, "smooth"),
    ({"min_per_zone": 0}, "min_per_zone"), ({"min_per_zone": 2.5}, "min_per_zone"), ({"polygons": 1}, "polygons")])
def test_every_refusal_of_the_option(change, text):
    with pytest.raises(ValueError, match=text):
        xm.resolve({"manage": dict(GOOD, **change), "fields": "fields.tif"}, DEFS)


def test_refusals_of_the_options_form():
    for bad, text in (({"manage": GOOD}, "needs \"fields\""), ({"manage": GOOD, "fields": None}, "needs \"fields\""),
                      ({"manage": GOOD, "fields": "f.tif", "property": "x"}, "unknown field"), ({"manage": [1], "fields": "f.tif"}, "takes a dict"),
                      ({"manage": None, "fields": "f.tif"}, "takes a dict"), ({"manage": GOOD, "fields": {"manage": GOOD, "fields": "f.tif"}}, "cannot be"),
                      (SEGMENT, "is no"), ("f.tif", "is no")):
        with pytest.raises(ValueError, match=text):
            xm.resolve(bad, DEFS)
    with pytest.raises(ValueError, match="manage index 'ndvi' is not among"):
        xm.resolve({"manage": GOOD, "fields": "f.tif"}, [])


def test_the_job_s_check_unwraps_the_form():
    """JobOptions.check: the form's own refusals, then `fields` as the value it is -- the segment option's refusals with their messages"""
    from app.job_options import JobOptions
    check = lambda zones, **kw: JobOptions(**dict(dict(bit_depth=16, indices=["ndvi"], zones=zones), **kw)).check(False, 4)
    check({"manage": GOOD, "fields": SEGMENT})
    check({"manage": GOOD, "fields": np.zeros((8, 8), np.uint16)})
    check({"manage": GOOD, "fields": "fields.geojson"})
    for bad, text in ((dict(GOOD, colour=1), "unknown key"), (dict(GOOD, index="ndwi"), "not among"), (dict(GOOD, index=["ndvi", "ndvi"]), "twice"),
                      (dict(GOOD, k=9), "k 9"), (dict(GOOD, iterations=0), "iterations"), (dict(GOOD, smooth=5), "smooth")):
        with pytest.raises(ValueError, match=text):
            check({"manage": bad, "fields": SEGMENT})
    with pytest.raises(ValueError, match="needs \"fields\""):
        check({"manage": GOOD})
    seg = SEGMENT["segment"]
    for inner, text in (({"segment": dict(seg, colour=1)}, "segment has unknown key"), ({"segment": dict(seg, index="ndwi")}, "segment index 'ndwi' is not among"),
                        ({"segment": dict(seg, min=0.9, max=0.1)}, "min 0.9 > max 0.1"), ({"segment": dict(seg, min_area_ha=1.0)}, "exactly one")):
        with pytest.raises(ValueError, match=text) as wrapped:
            check({"manage": GOOD, "fields": inner})
        with pytest.raises(ValueError) as bare:
            check(inner)
        assert str(wrapped.value) == str(bare.value)               # the inner value's exact message
    with pytest.raises(ValueError, match="belong to indices"):
        check({"manage": GOOD, "fields": SEGMENT}, indices=None)
    with pytest.raises(ValueError, match="16-bit path"):
        check({"manage": GOOD, "fields": SEGMENT}, bit_depth=8)


def test_zone_rows_and_the_metadata_block():
    feats = np.stack([mm.raster(65, 129, "noise"), mm.raster(65, 129, "ramp")])
    labels, Z = mm.layout(65, 129, "grid16")
    params = xm.resolve({"manage": dict(GOOD, index=["ndvi", "ndwi"], k=2), "fields": "f.tif"}, DEFS)
    r = mm.kmeans(feats, labels, Z, k=2, min_per_zone=10, smooth=1)
    rows = xm.zone_rows(r["table"], r["status"], params, (2.5, 2.5))
    assert [row["label"] for row in rows] == np.flatnonzero(r["status"] == 2).tolist() and len(rows) > 10
    row = rows[3]
    l = row["label"]
    for j, z in enumerate(row["zones"]):
        inside = (labels == l) & (r["zone"] == j + 1)
        assert z["zone_id"] == j + 1 and z["zone_class"] == f"zone_{j + 1}" and z["pixels"] == int(inside.sum()) and z["area_ha"] == z["pixels"] * 6.25e-4
        for d, (name, K) in enumerate((("ndvi", 10000), ("ndwi", 5000))):
            v = feats[d][inside].astype(np.float64) / K
            assert abs(z[name]["mean"] - v.mean()) < 1e-9 and abs(z[name]["std"] - v.std()) < 1e-9
    assert xm.zone_rows(r["table"], r["status"], params, None)[0]["zones"][0]["area_ha"] is None
    block = xm.metadata_block(params, r, rows, Path("out/x_mzones.tif"), None)
    assert block["parameters"] == {"index": ["ndvi", "ndwi"], "K": [10000, 5000], "k": 2, "iterations": 32, "min_per_zone": 10, "smooth": 1, "polygons": True}
    assert block["iterations"] == r["iterations"] and block["zoned"] == len(rows) and block["skipped"] == int((r["status"] == 1).sum()) > 0
    assert block["classes"] == ["zone_1", "zone_2"] and block["file"] == "out/x_mzones.tif" and block["geojson"] is None
    assert json.loads(json.dumps(block)) == block


# ---- the job on a stand-in engine ----------------------------------------------------------------------------------------------------------
class StandInEngine:
    """answers the raster entries with the models"""
    chain_lock = threading.RLock()
    calls = []

    def zones_kmeans_i16(self, feats, labels, Z, k=3, iters=32, min_per_zone=10, smooth=0, band_rows=0):
        StandInEngine.calls.append(("zones_kmeans_i16", np.asarray(feats).shape, int(Z), k, iters, min_per_zone, smooth))
        return mm.kmeans(feats, labels, Z, k=k, iters=iters, min_per_zone=min_per_zone, smooth=smooth)

    def labels_trace_u16(self, labels, Z):
        return fm.trace(np.asarray(labels), Z)

    def fields_segment_i16(self, idx, lo, hi, **kw):
        return fm.segment(idx, lo, hi, **kw)

    def index_nd_u16(self, a, b, ca=0, cb=0, offset=0, L=0, K=10000, valid=None, valid_scale=1, zones=None, zone_scale=1, Z=0, want=()):
        a = np.ascontiguousarray(a[..., ca]) if a.ndim == 3 else a
        v, _ = im.index(a, b, offset, L, K, valid, valid_scale)
        return {"zonal": im.zonal(v, zones, zone_scale, Z)}


class StandInESRGAN:
    """stands in for the GPU operator: nearest-neighbour x4 and the index model"""
    def __init__(self, model_name=None, tile_size=256, **kw):
        self.scale, self._engine = 4, StandInEngine()

    def product16(self, img, value_range=None, valid=None, nodata=None, fill_radius=32, extra=None, extra_weights=None, indices=None, display=None):
        from app.cnn_super_resolution import Product16
        up = lambda a: np.ascontiguousarray(np.repeat(np.repeat(a, 4, axis=0), 4, axis=1))
        out16, carried = up(img), None if extra is None else up(extra)
        found = []
        for d in indices or []:
            (ka, ca), (kb, cb) = d["a"], d["b"]
            side = lambda kind, c: np.ascontiguousarray((out16 if kind == "img" else carried)[..., c])
            v, undefined = im.index(side(ka, ca), side(kb, cb), d["offset"], d["L"], d["K"], valid, 4)
            r = {"index": v, "hist": im.hist(v, d["K"]), "undefined": undefined, "rgba": im.render(v, d["lut"])}
            if d.get("zones") is not None:
                r["zonal"] = im.zonal(v, d["zones"], d["zone_scale"], d["Z"])
            found.append(r)
        return Product16(out16=out16, carried=carried, carried_record={}, indices=found)


def georef(epsg, x0, y0, dx, dy):
    return rio.GeoRef({rio.TAG_PIXEL_SCALE: (dx, dy, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, x0, y0, 0.0),
                       rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, epsg)})


@pytest.fixture
def scene(tmp_path, monkeypatch):
    from app import wow_sr
    monkeypatch.setattr(wow_sr, "RealESRGAN", StandInESRGAN)
    H, W = 24, 20
    rng = np.random.default_rng(52)
    four = rng.integers(1000, 4000, size=(H, W, 4)).astype(np.uint16)
    four[6:18, 4:15, 3] += 2500
    g = georef(32633, 600000.0, 5100000.0, 10.0, 10.0)
    src = tmp_path / "scene4.tif"
    rio.write_geotiff_u16(src, four, g)
    y, x = np.mgrid[0:4 * H, 0:4 * W]
    labels = (1 + (y // 48) * 2 + x // 40).astype(np.uint16)      # four fields of 48 x 40 output pixels
    labels[:, 78:] = 0
    labels[40:44, :30] = 9                                         # a field too small to be zoned
    return src, g, labels


def test_the_job_writes_the_raster_the_geojson_and_the_block(scene, tmp_path, monkeypatch):
    from app.wow_sr import process_wow_sr
    src, g, labels = scene
    seen = []
    for mod, name in ((xz, "is_geojson"), (xz, "rasterize"), (xf, "is_segment"), (xf, "resolve"), (xf, "check_option")):
        real = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, _real=real, _name=name, **kw: (seen.append((_name, a)), _real(*a, **kw))[1])
    common = dict(enhance_crops=False, model="realesrgan_anime", bit_depth=16, indices=["ndvi", "ndwi"])
    option = {"manage": {"index": ["ndvi", "ndwi"], "k": 3, "min_per_zone": 10, "smooth": 1}, "fields": labels}
    StandInEngine.calls.clear()
    res = process_wow_sr(src, tmp_path / "m", zones=option, **common)
    plain = process_wow_sr(src, tmp_path / "p", zones=labels, **common)
    assert seen and not any(xm.is_manage(v) for _, args in seen for v in args), "the form reached the GeoJSON reader or the segmenter as it is"
    assert StandInEngine.calls == [("zones_kmeans_i16", (2, 96, 80), 9, 3, 32, 10, 1)]
    # the raster: the model's zones of the job's own index files
    feats = np.stack([rio.read_bands_raw(tmp_path / "m" / f"scene4_wow_sr_{n}.tif")[0][..., 0] for n in ("ndvi", "ndwi")])
    want = mm.kmeans(feats, labels, 9, k=3, iters=32, min_per_zone=10, smooth=1)
    mtif = tmp_path / "m" / "scene4_wow_sr_mzones.tif"
    arr, zg = rio.read_bands_raw(mtif)
    assert arr.dtype == np.uint8 and arr.shape == (96, 80, 1) and zg.nodata == 0 and zg.pixel_size == (2.5, 2.5)
    assert (arr[..., 0] == want["zone"]).all() and want["status"].tolist() == [0, 2, 2, 2, 2, 0, 0, 0, 0, 2]
    # the block and the outputs
    block = res["sr_metadata"]["zones"]["management"]
    mgj = tmp_path / "m" / "scene4_wow_sr_mzones.geojson"
    params = xm.resolve(dict(option, fields="x"), [{"name": "ndvi", "K": 10000}, {"name": "ndwi", "K": 10000}])
    assert block == xm.metadata_block(params, want, xm.zone_rows(want["table"], want["status"], params, (2.5, 2.5)), mtif, mgj)
    assert block["zoned"] == 5 and block["skipped"] == 0 and block["iterations"] == want["iterations"] and block["classes"] == ["low", "medium", "high"]
    assert res["outputs"]["management_tif"] == str(mtif) and res["outputs"]["management_geojson"] == str(mgj)
    assert json.load(open(tmp_path / "m" / "scene4_wow_sr_metadata.json"))["sr_metadata"]["zones"] == json.loads(json.dumps(res["sr_metadata"]["zones"]))
    # the GeoJSON: one Feature per (field, zone) with a pixel, its properties the block's rows, its rings burning back to the raster
    fc = json.load(open(mgj))
    rows = {(r["label"], z["zone_id"]): z for r in block["fields"] for z in r["zones"]}
    assert [(f["properties"]["label"], f["properties"]["zone_id"]) for f in fc["features"]] == sorted(key for key, z in rows.items() if z["pixels"])
    for f in fc["features"]:
        assert f["properties"] == dict(rows[f["properties"]["label"], f["properties"]["zone_id"]], label=f["properties"]["label"])
        assert f["properties"]["zone_class"] == ["low", "medium", "high"][f["properties"]["zone_id"] - 1]
    for j in (1, 2, 3):
        part = [f for f in fc["features"] if f["properties"]["zone_id"] == j]
        grid = xz.to_grid(xz.read({"type": "FeatureCollection", "features": part}), g, (24, 20), 4)
        assert grid["grid"] == (96, 80) and grid["dropped"] == 0
        burnt = zm.rasterize(zm.from_tables(grid["xy"], grid["ring_start"], grid["feat_start"], [f["properties"]["label"] for f in part]), 9, 96, 80)[0]
        assert (burnt == np.where(want["zone"] == j, labels, 0)).all(), j
    # without the form every byte, file and metadata entry is what it is for the label raster alone
    names = sorted(p.name for p in (tmp_path / "p").iterdir())
    assert sorted(p.name for p in (tmp_path / "m").iterdir()) == sorted(names + ["scene4_wow_sr_mzones.tif", "scene4_wow_sr_mzones.geojson"])
    for name in names:
        if not name.endswith("_metadata.json"):
            assert (tmp_path / "m" / name).read_bytes() == (tmp_path / "p" / name).read_bytes(), name
    strip = lambda d: {k: v for k, v in d.items() if k not in ("output_file", "zones") and not (k == "indices")}
    assert strip(res["sr_metadata"]) == strip(plain["sr_metadata"]) and "zones" not in plain["sr_metadata"]
    for a, b in zip(res["sr_metadata"]["indices"], plain["sr_metadata"]["indices"]):
        assert {k: v for k, v in a.items() if k != "files"} == {k: v for k, v in b.items() if k != "files"}
    assert set(res["outputs"]) - set(plain["outputs"]) == {"management_tif", "management_geojson"}
    assert list(res["sr_metadata"]["zones"]) == ["management"]


def test_the_job_on_segmented_fields_and_without_polygons(scene, tmp_path):
    """`fields` in its segment form: the zones block is the segmentation's with "management" added; polygons False: no GeoJSON"""
    from app.wow_sr import process_wow_sr
    src, g, _ = scene
    common = dict(enhance_crops=False, model="realesrgan_anime", bit_depth=16, indices=["ndvi"])
    segment = {"segment": {"index": "ndvi", "min": 0.15, "open": 1, "close": 2, "connectivity": 8, "min_pixels": 12}}
    res = process_wow_sr(src, tmp_path / "m", zones={"manage": {"index": "ndvi", "k": 2, "min_per_zone": 5, "smooth": 0, "polygons": False},
                                                     "fields": segment}, **common)
    plain = process_wow_sr(src, tmp_path / "p", zones=segment, **common)
    block = dict(res["sr_metadata"]["zones"])
    management = block.pop("management")
    swap = lambda d: json.loads(json.dumps(d).replace(str(tmp_path / "m"), str(tmp_path / "p")))
    assert swap(block) == json.loads(json.dumps(plain["sr_metadata"]["zones"]))
    ndvi = rio.read_bands_raw(tmp_path / "m" / "scene4_wow_sr_ndvi.tif")[0][..., 0]
    labels = rio.read_bands_raw(tmp_path / "m" / "scene4_wow_sr_zones.tif")[0][..., 0]
    want = mm.kmeans(ndvi, labels, block["found"], k=2, min_per_zone=5)
    assert (rio.read_bands_raw(tmp_path / "m" / "scene4_wow_sr_mzones.tif")[0][..., 0] == want["zone"]).all() and want["zone"].any()
    assert management["geojson"] is None and "management_geojson" not in res["outputs"] and not (tmp_path / "m" / "scene4_wow_sr_mzones.geojson").exists()
    assert management["classes"] == ["zone_1", "zone_2"] and management["zoned"] == int((want["status"] == 2).sum()) >= 1
    for name in ("scene4_wow_sr.tif", "scene4_wow_sr_ndvi.tif", "scene4_wow_sr_ndvi.png", "scene4_wow_sr_zones.tif", "scene4_wow_sr_fields.geojson"):
        assert (tmp_path / "m" / name).read_bytes() == (tmp_path / "p" / name).read_bytes(), name


def test_the_job_refuses_a_bad_form_before_anything_is_created(scene, tmp_path):
    from app.wow_sr import process_wow_sr
    src, g, labels = scene
    common = dict(enhance_crops=False, model="realesrgan_anime", bit_depth=16, indices=["ndvi"])
    for bad, text in (({"manage": dict(GOOD, index="savi"), "fields": labels}, "not among"), ({"manage": GOOD}, "needs \"fields\""),
                      ({"manage": dict(GOOD, k=1), "fields": labels}, "k 1"),
                      ({"manage": GOOD, "fields": {"segment": {"index": "ndvi", "open": 9, "min_pixels": 3}}}, "open")):
        with pytest.raises(ValueError, match=text):
            process_wow_sr(src, tmp_path / "out", zones=bad, **common)
        assert not (tmp_path / "out").exists()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_and_refuses_a_null_handle():
    for name, n in (("s2sr_zones_kmeans_i16", 17), ("s2sr_debug_mzones_stage_ms", 3)):
        assert name in native.EXPORTED_SYMBOLS and re.search(rf"\b{name}\(", HEADER)
        decl = re.search(rf"{name}\(([^;]*)\);", HEADER).group(1)
        assert len([a for a in re.sub(r"/\*.*?\*/", "", decl).split(",") if a.strip()]) == len(native._PROTOS[name][1]) == n
    lib = native.load_library()
    assert lib.s2sr_zones_kmeans_i16(None, None, 1, 1, 1, None, 1, 3, 1, 1, 0, 0, None, None, None, None, None) == -1
    assert lib.s2sr_debug_mzones_stage_ms(None, None, None) == -1
    stages = sorted(int(v) for v in re.findall(r"#define S2SR_MZONES_(?!STAGES)\w+ (\d+)", HEADER))
    assert stages == list(range(len(native.MZONES_STAGES))) and int(re.search(r"#define S2SR_MZONES_STAGES (\d+)", HEADER).group(1)) == 5
    text = HEADER[HEADER.index("Management zones"):HEADER.index("s2sr_zones_kmeans_i16(")]
    assert "scratch" in text and "voids" in text and "keeps nothing" in text and "half away from zero" in text
    with pytest.raises(TypeError):
        native.Engine.zones_kmeans_i16(None, np.zeros((2, 2), np.uint16), np.zeros((2, 2), np.uint16), 1)
    with pytest.raises(TypeError):
        native.Engine.zones_kmeans_i16(None, np.zeros((2, 2), np.int16), np.zeros((2, 3), np.uint16), 1)
