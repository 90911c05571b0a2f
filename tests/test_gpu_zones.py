"""Field polygons as zones on the GPU (include/s2sr.h: s2sr_zones_rasterize_u16; csrc/zones.hip): labels and area byte
for byte against tests/zones_model.py, the independence of band_rows and of the number of workgroups (caps 1 and 3, with the launch
and trip arithmetic), every refusal, the void rule, and the job that takes a GeoJSON file as its `zones`.  The entry under red zones,
poison, stalls and cap 8: its rows of tests/doors.py, whose baselines this module holds to the model.

The pass's capped launches are counted in the grid-cap family "display", as the index pass's are (the launcher families are a closed
list that tests/test_gridcap_cpu.py spells out)."""
import json

import numpy as np
import pytest

import diag
import doors
import gpu_engines
import zones_model as zm
from diag import same_values as same
from zones_model import case
from s2sr import geo, native
from s2sr import zones as xz

pytestmark = pytest.mark.gpu

HP = native.PREC_F16_HP
# the ragged shape, one pixel, a sliver, exactly one tile, one row and one column more than whole tiles, and 4 x 5 tiles with ragged edges
# (and the widths of the SR grid, tests/doors.py WIDTHS: 16-byte stores at W % 8 == 0, 8-byte stores with a row tail of 4 at W % 8 == 4;
# 3 x 68 beside 1 x 68, whose single row changes its label between pairs of pixels only: exchanged halves of a store leave it as it is)
SHAPES = [(37, 45), (1, 1), (3, 70), (64, 64), (65, 129), (255, 257)] + doors.WIDTHS + [(3, 68)]
GRID_FAMILY = "display"


@pytest.fixture(scope="module")
def bare():
    with gpu_engines.bare(precision=HP) as e:                    # the entry needs no weights
        yield e


def run(e, H, W, kind="scene", **kw):
    tabs, Z, labels, area = case(H, W, kind)
    got, got_area = e.zones_rasterize_u16(*tabs, Z, (H, W), **kw)
    return np.array(got), got_area, labels, area


@pytest.mark.parametrize("H,W", SHAPES)
def test_byte_for_byte_against_the_model(bare, H, W):
    """the mesh, holes, a MultiPolygon with a part in another feature's hole, overlaps with a shared label, a polygon around
    everything, one wholly outside and one at +-2^29"""
    got, got_area, labels, area = run(bare, H, W)
    same(got, labels, f"{H} x {W}: labels")
    same(got_area, area, f"{H} x {W}: area")
    assert int(got_area.sum()) == H * W
    if H * W > 1:
        assert len(np.unique(labels)) > 2
    alone, none = bare.zones_rasterize_u16(*case(H, W)[0], case(H, W)[1], (H, W), want_area=False)
    assert none is None
    same(alone, labels, f"{H} x {W}: labels without area")


def test_many_features_in_one_tile_and_many_edges_in_one_ring(bare):
    """300 unit squares inside the first 64 x 64 tile (later squares win repeated pixels); a ring of 1000 vertices across all 20 tiles"""
    for H, W, kind in ((65, 129, "squares"), (255, 257, "star")):
        got, got_area, labels, area = run(bare, H, W, kind)
        same(got, labels, f"{kind}: labels")
        same(got_area, area, f"{kind}: area")
    assert len(case(255, 257, "star")[0][0]) == 1000 and len(case(65, 129, "squares")[0][3]) == 300
    assert 150 < int((case(65, 129, "squares")[2] > 0).sum()) < 300                       # some squares repeat a pixel


@pytest.mark.parametrize("H,W", [(37, 45), (65, 129), (65, 128), (37, 180), (39, 78)])
def test_band_rows_do_not_change_a_byte(bare, H, W):
    for rows in (0, 1, 3, H - 1):
        got, got_area, labels, area = run(bare, H, W, band_rows=rows)
        same(got, labels, f"band_rows {rows}: labels")
        same(got_area, area, f"band_rows {rows}: area")


@pytest.mark.parametrize("cap", [1, 3])
def test_under_capped_grids(bare, cap):
    """the same bytes, and the trips are what ceil(items / cap) says: 255 x 257 pixels are 4 x 5 tiles"""
    H, W = 255, 257
    for kind in ("scene", "star"):
        with diag.under(cap):
            got, got_area, labels, area = run(bare, H, W, kind)
            launches, trips = native.grid_cap_stats()[GRID_FAMILY]
            native.grid_cap_stats(reset=True)
            got2, area2, _, _ = run(bare, H, W, kind, band_rows=100)                       # bands of 100, 100, 55 rows: 2, 3 and 1 tile rows
            launches2, trips2 = native.grid_cap_stats()[GRID_FAMILY]
        same(got, labels, f"cap {cap}, {kind}: labels")
        same(got_area, area, f"cap {cap}, {kind}: area")
        same(got2, labels, f"cap {cap}, {kind}, in bands: labels")
        same(area2, area, f"cap {cap}, {kind}, in bands: area")
        assert (launches, trips) == (1, -(-20 // cap)), (launches, trips)
        assert (launches2, trips2) == (3, -(-15 // cap)), (launches2, trips2)
    native.grid_cap_stats(reset=True)
    run(bare, H, W)
    assert native.grid_cap_stats()[GRID_FAMILY] == (0, 0)                                  # off means off


def test_every_refusal_returns_minus_one_and_leaves_the_next_call_intact(bare):
    H, W = 3, 70
    (xy, ring_start, feat_start, label), Z, labels, area = case(H, W)
    lib = native.load_library()
    out, got_area = np.zeros((H, W), np.uint16), np.zeros(Z + 1, np.uint64)
    base = dict(xy=xy, ring_start=ring_start, feat_start=feat_start, label=label, F=len(label), Z=Z, H=H, W=W, band_rows=0, out=out, area=got_area)
    order = list(base)
    p = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
    assert lib.s2sr_zones_rasterize_u16(bare._h, *[p(base[k]) for k in order]) == 0
    same(out, labels, "the raw call: labels")
    same(got_area, area, "the raw call: area")

    def changed(name, at, value):
        t = base[name].copy()
        t[at] = value
        return {name: t}
    far = xy.copy()
    far[5, 1] = -2 ** 29 - 1
    refusals = [dict(H=0), dict(W=0), dict(H=-1), dict(H=65536, W=32768), dict(F=0), dict(F=-1), dict(Z=0), dict(Z=65536), dict(Z=Z - 1),
                changed("label", 3, 0), changed("label", 0, Z + 1), changed("feat_start", 0, 1), changed("feat_start", 4, 2),
                changed("ring_start", 0, 1), changed("ring_start", 7, 3), changed("ring_start", 2, int(ring_start[1]) + 2),
                changed("xy", (0, 0), 2 ** 29 + 1), dict(xy=far), dict(xy=None), dict(ring_start=None), dict(feat_start=None), dict(label=None),
                dict(out=None), dict(band_rows=-1)]
    for kw in refusals:
        args = dict(base, **kw)
        assert lib.s2sr_zones_rasterize_u16(bare._h, *[p(args[k]) for k in order]) == -1, list(kw)
        got, got_a, _, _ = run(bare, H, W)
        same(got, labels, f"after the refusal of {list(kw)}: labels")
        same(got_a, area, f"after the refusal of {list(kw)}: area")
    # the Python layer's own refusals: dtypes, shapes, starts that point outside their tables
    for bad in (dict(xy=xy.astype(np.int64)), dict(label=label.astype(np.int32)), dict(xy=xy.ravel()), dict(label=label[:-1]),
                dict(feat_start=feat_start + 1), dict(ring_start=ring_start + 1)):
        t = dict(xy=xy, ring_start=ring_start, feat_start=feat_start, label=label)
        t.update(bad)
        with pytest.raises((TypeError, ValueError)):
            bare.zones_rasterize_u16(t["xy"], t["ring_start"], t["feat_start"], t["label"], Z, (H, W))
    with pytest.raises(native.S2srError):
        bare.zones_rasterize_u16(xy, ring_start, feat_start, label, Z - 1, (H, W))
    got, got_a, _, _ = run(bare, H, W)
    same(got, labels, "after the Python refusals")


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
        got, got_area, labels, area = run(e, 37, 45)
        with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
            e.index_nd_u16(None, b, ca=2)
        q = np.array(e.enhance_u16(img, tile=16, pad=3))
        same(np.array(e.index_nd_u16(None, b, ca=2)["index"]), first, "the chain works again")
        # the labels as a caller's array: zonal sums from them
        z = e.index_nd_u16(q, b, ca=2, zones=np.ascontiguousarray(labels[:36, :44]), Z=200, want=("zonal",))["zonal"]
    same(got, labels, "labels on the shared engine")
    same(got_area, area, "area on the shared engine")
    assert int(z[:, 0].sum()) > 0


@pytest.mark.parametrize("ident", doors.owned("zones_rasterize_u16"))
def test_the_door_table_s_baseline_is_the_model(ident):
    """tests/doors.py's rows of this pass: the red-zone, poison, stall and grid-cap matrices hold every mode to diag.baseline, and
    this holds the baseline to the model, sample for sample"""
    same(diag.baseline(ident), doors.MODELS[ident](), ident)


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


def test_the_wow_job_takes_field_polygons(monkeypatch, tmp_path):
    """a 24 x 20 UTM GeoTIFF of 4 bands and a lon / lat GeoJSON of three fields: the index raster, its PNG and the per-zone tables are
    those of the same job given the model's label raster; the job writes the labels and says what it did"""
    from app.wow_sr import process_wow_sr
    from s2sr import rasterio_lite as rio
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    H, W = 24, 20
    rng = np.random.default_rng(52)
    four = rng.integers(1000, 4000, size=(H, W, 4)).astype(np.uint16)
    x0, y0 = 600000.0, 5100000.0
    g = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, x0, y0, 0.0),
                    rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633)})
    src = tmp_path / "scene4.tif"
    rio.write_geotiff_u16(src, four, g)
    crs = geo.CRS(32633)

    def lonlat_ring(pixels):
        """a ring given in input pixels (col, row), closed as GeoJSON wants it"""
        lon, lat = crs.to_lonlat(np.array([x0 + 10 * c for c, _ in pixels]), np.array([y0 - 10 * r for _, r in pixels]))
        ring = [[float(a), float(b)] for a, b in zip(lon, lat)]
        return ring + [ring[0]]
    fields = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "id": "north", "properties": {"crop": "wheat"},
         "geometry": {"type": "Polygon", "coordinates": [lonlat_ring([(1.2, 1.1), (11.7, 2.3), (10.9, 9.6), (2.1, 8.8)]),
                                                         lonlat_ring([(4.1, 3.9), (6.2, 4.1), (5.3, 6.4)])]}},                  # with a hole
        {"type": "Feature", "properties": {"crop": "maize"},
         "geometry": {"type": "MultiPolygon", "coordinates": [[lonlat_ring([(12.3, 1.0), (23.0, 3.0), (17.2, 11.1)])],          # reaches past the right edge
                                                              [lonlat_ring([(4.6, 4.3), (5.8, 4.5), (5.2, 5.7)])]]}},           # a part inside the hole
        {"type": "Feature", "properties": {"crop": "wheat"},
         "geometry": {"type": "Polygon", "coordinates": [lonlat_ring([(3.3, 12.2), (15.1, 13.4), (16.8, 22.9), (1.1, 21.0), (8.7, 17.0)])]}}]}
    (tmp_path / "fields.geojson").write_text(json.dumps(fields))
    # the model's label raster of the same polygons on the x4 grid
    feats = xz.read(tmp_path / "fields.geojson")
    grid = xz.to_grid(feats, g, (H, W), 4)
    assert grid["grid"] == (96, 80) and grid["dropped"] == 0
    want_labels, want_area = zm.rasterize(zm.from_tables(grid["xy"], grid["ring_start"], grid["feat_start"], [1, 2, 3]), 3, 96, 80)
    assert all(want_area[1:] > 50) and want_area[0] > 1000
    common = dict(enhance_crops=False, model="realesrgan_anime", bit_depth=16, indices=["ndvi"])
    res = process_wow_sr(src, tmp_path / "poly", zones=tmp_path / "fields.geojson", **common)
    ref = process_wow_sr(src, tmp_path / "raster", zones=want_labels, **common)
    none = process_wow_sr(src, tmp_path / "none", **common)
    for name in ("scene4_wow_sr.tif", "scene4_wow_sr_ndvi.tif", "scene4_wow_sr_ndvi.png"):
        assert (tmp_path / "poly" / name).read_bytes() == (tmp_path / "raster" / name).read_bytes() == (tmp_path / "none" / name).read_bytes(), name
    m, m_ref = res["sr_metadata"]["indices"][0], ref["sr_metadata"]["indices"][0]
    assert m["zones"] == m_ref["zones"] and [r["zone"] for r in m["zones"]] == [0, 1, 2, 3] and "zones" not in none["sr_metadata"]["indices"][0]
    strip = lambda d: {k: v for k, v in d.items() if k not in ("indices", "output_file", "zones")}
    assert strip(res["sr_metadata"]) == strip(ref["sr_metadata"]) == strip(none["sr_metadata"])
    # the label raster the job wrote, and what it says about it
    ztif = tmp_path / "poly" / "scene4_wow_sr_zones.tif"
    arr, zg = rio.read_bands_raw(ztif)
    assert arr.dtype == np.uint16 and arr.shape == (96, 80, 1) and zg.nodata == 0 and zg.pixel_size == (2.5, 2.5)
    same(arr[..., 0], want_labels, "the zones GeoTIFF against the model")
    block = res["sr_metadata"]["zones"]
    assert block == {"source": str(tmp_path / "fields.geojson"), "features": 3, "dropped": 0, "grid": [96, 80], "zone_scale": 1, "file": str(ztif),
                     "labels": [{"label": k + 1, "id": i, "features": 1, "pixels": int(want_area[k + 1]), "area_ha": int(want_area[k + 1]) * 6.25 / 10000}
                                for k, i in enumerate(["north", None, None])]}
    assert res["outputs"]["zones_tif"] == str(ztif)
    assert json.load(open(tmp_path / "poly" / "scene4_wow_sr_metadata.json"))["sr_metadata"]["zones"] == json.loads(json.dumps(block))
    for other, d in ((ref, "raster"), (none, "none")):                                     # a label raster, or no zones: no such file or block
        assert "zones" not in other["sr_metadata"] and "zones_tif" not in other["outputs"] and not list((tmp_path / d).glob("*_zones.tif"))
    # labels by a property: the two wheat fields share label 1
    by = process_wow_sr(src, tmp_path / "crop", zones={"geojson": fields, "property": "crop"}, **common)
    merged = np.where(want_labels == 3, 1, want_labels).astype(np.uint16)
    same(rio.read_bands_raw(tmp_path / "crop" / "scene4_wow_sr_zones.tif")[0][..., 0], merged, "labels by property")
    assert [(r["label"], r["value"], r["features"], r["pixels"]) for r in by["sr_metadata"]["zones"]["labels"]] == \
        [(1, "wheat", 2, int(want_area[1] + want_area[3])), (2, "maize", 1, int(want_area[2]))]
    assert by["sr_metadata"]["zones"]["source"] == "inline" and [r["zone"] for r in by["sr_metadata"]["indices"][0]["zones"]] == [0, 1, 2]
