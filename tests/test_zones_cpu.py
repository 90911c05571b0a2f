"""Field polygons as zones without a GPU: the definition's model (tests/zones_model.py) against itself -- the mesh
partition, the per-row form, windings, holes and bow-ties, the magnitudes at +-2^29 --, the host policy (s2sr/zones.py: every input
form, every refusal, quantisation on hand-computed vertices, dropped features, property labels), the tile bins of csrc/zone_bins.h
under the address and undefined-behaviour sanitizers, and the C ABI's declaration."""
import json
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import zones_model as zm
from s2sr import geo, native
from s2sr import rasterio_lite as rio
from s2sr import zones as xz

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "s2sr.h").read_text()
SHAPES = [(37, 45), (1, 1), (3, 70), (64, 64), (65, 129), (255, 257), (65, 128), (37, 180)]


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_the_mesh_partitions_the_grid(H, W):
    """every pixel belongs to exactly one triangle of the shared-vertex mesh, and area sums to H W"""
    tris, P = zm.mesh(H, W)
    assert len(tris) == 98
    xs, ys = [p[0] for p in P.values()], [p[1] for p in P.values()]
    assert min(xs) < 0 and min(ys) < 0 and max(xs) > 256 * W and max(ys) > 256 * H          # it reaches past every side
    count = np.zeros((H, W), np.int64)
    for t in tris:
        count += zm.inside_pixels([t], H, W)
    assert (count == 1).all(), f"{int((count != 1).sum())} pixels lie in no triangle or in several"
    labels, area = zm.rasterize([([t], 1 + k) for k, t in enumerate(tris)], 98, H, W)
    assert (labels > 0).all() and int(area.sum()) == H * W and area[0] == 0


def test_the_mesh_has_vertices_and_edges_on_pixel_centres():
    H, W = 37, 45
    tris, P = zm.mesh(H, W)
    on_centre = [p for p in P.values() if p[0] % 256 == 128 and p[1] % 256 == 128 and 0 < p[0] < 256 * W and 0 < p[1] < 256 * H]
    assert len(on_centre) >= 2
    assert P[2, 4][1] == P[3, 4][1] and P[2, 4][1] % 256 == 128                            # a horizontal edge through a row's centres
    assert P[5, 3][0] == P[5, 4][0] and P[5, 3][0] % 256 == 128                            # a vertical edge through a column's centres
    r = P[2, 4][1] // 256
    assert any(256 * c + 128 > min(P[2, 4][0], P[3, 4][0]) and 256 * c + 128 < max(P[2, 4][0], P[3, 4][0]) for c in range(W)) and 0 <= r < H


@pytest.mark.parametrize("H,W", SHAPES)
def test_the_row_form_is_the_pixel_form(H, W):
    feats, Z = zm.scene(H, W)
    for rings, _ in feats:
        assert np.array_equal(zm.inside_rows(rings, H, W), zm.inside_pixels(rings, H, W))
    a, b = zm.rasterize(feats, Z, H, W), zm.rasterize(feats, Z, H, W, inside=zm.inside_rows)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and int(a[1].sum()) == H * W


def test_the_scene_is_a_real_case_at_the_widths_of_the_sr_grid():
    """tests/doors.py WIDTHS, which tests/test_gpu_zones.py rasterises: at least two labels at every shape, and where W % 8 == 4 a
    row whose last group of 4 pixels -- the 8-byte store of the row tail -- holds a label; with more than one row, a tail whose two
    pairs differ and a full group of 8 whose first two pairs differ (every border in the single row of 1 x 68 falls between pairs)"""
    import doors
    for H, W in doors.WIDTHS + [(3, 68)]:                          # (3 x 68: what the GPU module runs beside 1 x 68 for that reason)
        labels = zm.case(H, W)[2]
        assert len(np.unique(labels[labels > 0])) >= 2, (H, W)
        if W % 8 == 4:
            tail = labels[:, W - 4:]
            full = labels[:, :W - 4].reshape(H, -1, 8)
            assert tail.any() and (H == 1 or ((tail[:, :2] != tail[:, 2:]).any() and (full[..., :2] != full[..., 2:4]).any())), (H, W)


def test_windings_holes_and_bow_ties():
    H, W = 37, 45
    feats, Z = zm.scene(H, W)
    want = zm.rasterize(feats, Z, H, W)[0]
    turned = [([ring[::-1] for ring in rings], lab) for rings, lab in feats]                # every ring reversed
    assert np.array_equal(zm.rasterize(turned, Z, H, W)[0], want)
    rolled = [([ring[2:] + ring[:2] for ring in rings], lab) for rings, lab in feats]       # another first vertex
    assert np.array_equal(zm.rasterize(rolled, Z, H, W)[0], want)
    holed = next(rings for rings, lab in feats if lab == 120)
    outer, hole_a, hole_b = holed
    full = zm.inside_pixels([outer], H, W)
    for ha in (hole_a, hole_a[::-1]):                                                       # a hole in either winding
        for hb in (hole_b, hole_b[::-1]):
            got = zm.inside_pixels([outer, ha, hb], H, W)
            assert np.array_equal(got, full & ~zm.inside_pixels([hole_a], H, W) & ~zm.inside_pixels([hole_b], H, W))
    assert (full & ~zm.inside_pixels(holed, H, W)).sum() > 20                               # the holes hold pixels
    bow = next(rings for rings, lab in feats if lab == 140)[0]
    a, b, c, d = bow                                                                         # a-b and c-d cross: two triangles meet at the crossing
    got = zm.inside_pixels([bow], H, W)
    assert got.any() and np.array_equal(got, zm.inside_pixels([bow[::-1]], H, W))
    assert got.sum() < zm.inside_pixels([[a, c, b, d]], H, W).sum()                         # the untwisted quadrilateral holds more
    # the part inside the other feature's hole is labelled, the hole around it is not
    part = next(rings for rings, lab in feats if lab == 121)[0]
    inner = zm.inside_pixels([part], H, W)
    assert inner.any() and not (inner & zm.inside_pixels(holed, H, W)).any()


def test_magnitudes_at_the_extremes_stay_below_2_63():
    B = zm.COORD_MAX
    rings = [[(-B, -B), (B, -B + 1), (B, B), (-B, B - 1)], [(-B, B), (B, -B), (B, B)], [(B, -B), (-B, B), (-B, -B)]]
    big = 0
    for r, c in ((0, 0), (0, 2 ** 21 - 1), (2 ** 21 - 1, 0), (2 ** 21 - 1, 2 ** 21 - 1), (2 ** 20, 2 ** 20), (2 ** 21, 2 ** 21)):
        big = max(big, zm.inside_python(rings, r, c)[1])
    assert 2 ** 59 < big < 2 ** 63
    # the same centres through the int64 model: no overflow changed an answer
    for r, c in ((0, 0), (2 ** 20, 2 ** 20)):
        cx, cy = np.int64(256 * c + 128), np.int64(256 * r + 128)
        odd = False
        for ring in rings:
            for xa, ya, xb, yb in zm.edges(ring):
                odd ^= bool((ya <= cy) & (cy < yb) & ((cx - np.int64(xa)) * np.int64(yb - ya) < np.int64(xb - xa) * (cy - np.int64(ya))))
        assert odd == zm.inside_python(rings, r, c)[0]


def test_a_sliver_that_holds_no_centre_labels_nothing():
    H, W = 37, 45
    slivers = [([[(100, 130), (256 * W - 50, 250), (256 * W - 50, 140)]], 1),                # between two rows of centres
               ([[(130, 10), (250, 256 * H), (140, 256 * H)]], 2),                           # between two columns
               ([[(128, 128), (384, 128), (256, 127)]], 3)]                                  # its flat edge runs through two centres from above: the row test is half-open
    labels, area = zm.rasterize(slivers, 3, H, W)
    assert not labels.any() and area.tolist() == [H * W, 0, 0, 0]
    # from below, the same flat edge is the triangle's top: rows are closed at the top and columns at the left, so it holds the
    # centre at its left end and not the one at its right end
    below = zm.inside_pixels([[(128, 128), (384, 128), (256, 129)]], H, W)
    assert below.sum() == 1 and below[0, 0]
    assert zm.inside_pixels([[(127, 127), (130, 127), (130, 130), (127, 130)]], H, W).sum() == 1


# ---- s2sr/zones.py ------------------------------------------------------------------------------------------------------------------------------
SQUARE = {"type": "Polygon", "coordinates": [[[15.0, 46.0], [15.01, 46.0], [15.01, 46.01], [15.0, 46.01], [15.0, 46.0]]]}
MULTI = {"type": "MultiPolygon", "coordinates": [SQUARE["coordinates"], [[[15.02, 46.0], [15.03, 46.0], [15.03, 46.01], [15.02, 46.0]]]]}


def feature(geom, **props):
    return {"type": "Feature", "geometry": geom, "properties": props or None}


def georef(epsg, x0, y0, dx, dy):
    return rio.GeoRef({rio.TAG_PIXEL_SCALE: (dx, dy, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, x0, y0, 0.0),
                       rio.TAG_GEOKEYS: (1, 1, 0, 1, 3072 if epsg != 4326 else 2048, 0, 1, epsg)})


def test_every_accepted_input_form(tmp_path):
    fc = {"type": "FeatureCollection", "features": [feature(SQUARE, name="a"), feature(MULTI, name="b")]}
    for suffix in (".geojson", ".json"):
        (tmp_path / f"fields{suffix}").write_text(json.dumps(fc))
    forms = {"path": tmp_path / "fields.geojson", "str": str(tmp_path / "fields.json"), "collection": fc, "feature": fc["features"][0],
             "geometry": MULTI, "list": [fc["features"][1], SQUARE, tmp_path / "fields.geojson"]}
    counts = {"path": 2, "str": 2, "collection": 2, "feature": 1, "geometry": 1, "list": 4}
    for k, src in forms.items():
        got = xz.read(src)
        assert len(got) == counts[k] and [f["index"] for f in got] == list(range(counts[k])), k
        assert all(f["epsg"] == 4326 for f in got)
        assert xz.is_geojson(src)
    got = xz.read(fc)
    assert got[0]["rings"] == [[(15.0, 46.0), (15.01, 46.0), (15.01, 46.01), (15.0, 46.01)]]       # the closing vertex is dropped
    assert len(got[1]["rings"]) == 2 and len(got[1]["rings"][1]) == 3 and got[1]["properties"] == {"name": "b"}
    assert xz.read(feature(SQUARE))[0]["properties"] == {}
    assert not xz.is_geojson(np.zeros((2, 2), np.uint16)) and not xz.is_geojson("zones.tif") and not xz.is_geojson(tmp_path / "z.tiff")
    assert xz.split_option({"geojson": fc, "property": "name"}) == (fc, "name") and xz.split_option(fc) == (fc, None)
    # a legacy crs member that geo.CRS supports is honoured
    for name, epsg in (("urn:ogc:def:crs:EPSG::32633", 32633), ("EPSG:3857", 3857), ("urn:ogc:def:crs:OGC:1.3:CRS84", 4326), ("urn:ogc:def:crs:EPSG:6.6:32733", 32733)):
        tagged = dict(fc, crs={"type": "name", "properties": {"name": name}})
        assert [f["epsg"] for f in xz.read(tagged)] == [epsg, epsg]


def test_every_refusal_of_read(tmp_path):
    point = {"type": "Point", "coordinates": [15.0, 46.0]}
    with pytest.raises(ValueError, match=r"feature 1 .*'Point'"):
        xz.read({"type": "FeatureCollection", "features": [feature(SQUARE), feature(point)]})
    with pytest.raises(ValueError, match=r"feature 0 .*'LineString'"):
        xz.read({"type": "LineString", "coordinates": [[0, 0], [1, 1]]})
    with pytest.raises(ValueError, match="feature 0 .*None"):
        xz.read(feature(None))
    for crs in ({"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::2154"}}, {"type": "name", "properties": {"name": "Lambert"}},
                {"type": "link", "properties": {"href": "x"}}, "EPSG:4326"):
        with pytest.raises(ValueError):
            xz.read(dict(SQUARE, crs=crs))
    for bad in ({"type": "FeatureCollection", "features": []}, [], {"type": "FeatureCollection"}, {"features": []}, 7, tmp_path / "fields.txt",
                {"type": "FeatureCollection", "features": [SQUARE]}, {"type": "Polygon", "coordinates": [[[0, 0], [1, 1], [0, 0]]]},
                {"type": "Polygon", "coordinates": [[0, 0]]}, {"type": "Polygon", "coordinates": 3}):
        with pytest.raises(ValueError):
            xz.read(bad)
    with pytest.raises(ValueError, match="unknown field"):
        xz.split_option({"geojson": SQUARE, "label": "x"})
    with pytest.raises(ValueError, match="property"):
        xz.split_option({"geojson": SQUARE, "property": 3})


def expected_units(px, py):
    """floor(256 p + 0.5) by hand"""
    return [math.floor(256 * px + 0.5), math.floor(256 * py + 0.5)]


@pytest.mark.parametrize("epsg", [32633, 32733, 3857, 4326])
def test_quantisation_on_hand_computed_vertices(epsg):
    """a raster of 10-unit pixels whose top-left corner is a round number: a vertex given in the raster's own coordinates through
    to_lonlat lands where the arithmetic says, in UTM north and south, 3857 and 4326"""
    crs = geo.CRS(epsg)
    if epsg == 4326:
        x0, y0, d = 15.0, 46.0, 0.0001
    elif epsg == 3857:
        x0, y0, d = 1670000.0, 5780000.0, 10.0
    else:
        x0, y0, d = 500000.0 + 40000.0, (5100000.0 if epsg == 32633 else 10000000.0 - 5100000.0), 10.0
    g = georef(epsg, x0, y0, d, d)
    H, W, scale = 20, 30, 4
    # input-pixel positions (col, row) of a triangle; on the x4 grid they are 4 times as far
    pos = [(1.0, 2.0), (10.25, 3.5), (7.1298828125, 15.0009765625)]         # the last: 1825.25 / 256, 3840.25 / 256
    lon, lat = crs.to_lonlat(np.array([x0 + c * d for c, _ in pos]), np.array([y0 - r * d for _, r in pos]))
    poly = {"type": "Polygon", "coordinates": [[[float(a), float(b)] for a, b in zip(lon, lat)]]}
    got = xz.to_grid(xz.read(poly), g, (H, W), scale)
    assert got["grid"] == (80, 120) and got["dropped"] == 0 and got["kept"] == [0]
    assert got["ring_start"].tolist() == [0, 3] and got["feat_start"].tolist() == [0, 1] and got["xy"].dtype == np.int32
    want = np.array([expected_units(scale * c, scale * r) for c, r in pos])
    # the projection round trip is good to well below 1e-6 pixels, and no position here is within 0.2 units of a half-unit tie
    assert got["xy"].tolist() == want.tolist()
    assert want.tolist() == [[1024, 2048], [10496, 3584], [7301, 15361]]
    # zone_scale 4: the label grid is the input grid
    got4 = xz.to_grid(xz.read(poly), g, (H, W), scale, zone_scale=4)
    assert got4["grid"] == (20, 30) and got4["xy"].tolist() == [expected_units(c, r) for c, r in pos] == [[256, 512], [2624, 896], [1825, 3840]]
    # the same vertices given in the raster's own CRS through a crs member: no projection at all, exact
    if epsg != 4326:
        own = {"type": "Polygon", "crs": {"type": "name", "properties": {"name": f"EPSG:{epsg}"}},
               "coordinates": [[[x0 + c * d, y0 - r * d] for c, r in pos]]}
        assert xz.to_grid(xz.read(own), g, (H, W), scale)["xy"].tolist() == want.tolist()


def test_quantise_is_floor_of_256_p_plus_half():
    assert xz.quantise([0.0, 0.001953125, 0.0019, -0.001953125, -0.002, 1.0, 1.498046875 / 256]).tolist() == [0, 1, 0, 0, -1, 256, 1]


def test_dropped_features_and_coordinates_beyond_the_range():
    g = georef(32633, 540000.0, 5100000.0, 10.0, 10.0)
    crs = geo.CRS(32633)

    def poly_at(c0, r0, c1, r1):
        lon, lat = crs.to_lonlat(np.array([540000.0 + 10 * c for c in (c0, c1, c1, c0)]), np.array([5100000.0 - 10 * r for r in (r0, r0, r1, r1)]))
        return {"type": "Polygon", "coordinates": [[[float(a), float(b)] for a, b in zip(lon, lat)]]}
    inside, left, below, straddle = poly_at(2, 2, 9, 9), poly_at(-30, 2, -1, 9), poly_at(2, 25, 9, 40), poly_at(-5, -5, 3, 3)
    got = xz.to_grid(xz.read([inside, left, below, straddle]), g, (20, 30), 4)
    assert got["dropped"] == 2 and got["kept"] == [0, 3] and got["feat_start"].tolist() == [0, 1, 2] and len(got["xy"]) == 8
    far = poly_at(5, 5, 600000, 10)             # meets the grid and reaches 2.4e6 output pixels to the right: beyond 2^29 / 256
    with pytest.raises(ValueError, match="2\\^29"):
        xz.to_grid(xz.read([inside, far]), g, (20, 30), 4)
    assert xz.to_grid(xz.read([inside, poly_at(700000, 5, 800000, 10)]), g, (20, 30), 4)["dropped"] == 1      # far away and wholly outside: dropped
    # a raster without placement tags, without a CRS, or with one geo.CRS does not know
    for bad in (None, rio.GeoRef({}), rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 1.0, 2.0, 0.0)}),
                georef(2154, 1.0, 2.0, 10.0, 10.0)):
        with pytest.raises(ValueError):
            xz.to_grid(xz.read(inside), bad, (20, 30), 4)


def test_labels_by_place_and_by_property():
    fc = {"type": "FeatureCollection", "features": [dict(feature(SQUARE, farm="north", n=1), id="f-7"), feature(MULTI, farm="south", n=1),
                                                    feature(SQUARE, farm="north", n=2)]}
    feats = xz.read(fc)
    labels, table = xz.labels_of(feats)
    assert labels == [1, 2, 3] and table == [{"label": 1, "id": "f-7", "features": 1}, {"label": 2, "id": None, "features": 1}, {"label": 3, "id": None, "features": 1}]
    labels, table = xz.labels_of(feats, "farm")
    assert labels == [1, 2, 1] and table == [{"label": 1, "value": "north", "features": 2}, {"label": 2, "value": "south", "features": 1}]
    assert xz.labels_of(feats, "n")[0] == [1, 1, 2]
    with pytest.raises(ValueError, match="feature 1 has no property"):
        xz.labels_of(xz.read([feature(SQUARE, a=1), feature(SQUARE, b=1)]), "a")
    many = [{"index": i, "rings": [], "properties": {"k": i}, "id": None, "epsg": 4326} for i in range(65536)]
    with pytest.raises(ValueError, match="65535"):
        xz.labels_of(many)
    with pytest.raises(ValueError, match="65535"):
        xz.labels_of(many, "k")
    assert len(xz.labels_of(many[:65535])[0]) == 65535


def test_metadata_block():
    table = [{"label": 1, "value": "north", "features": 2}, {"label": 2, "value": "south", "features": 1}]
    block = xz.metadata_block(Path("fields.geojson"), 3, table, 1, (80, 120), 1, Path("out/x_zones.tif"), np.array([9000, 500, 100], np.uint64), (2.5, 2.5))
    assert set(block) == {"source", "features", "labels", "dropped", "grid", "zone_scale", "file"}
    assert block["labels"] == [{"label": 1, "value": "north", "features": 2, "pixels": 500, "area_ha": 500 * 6.25 / 10000},
                               {"label": 2, "value": "south", "features": 1, "pixels": 100, "area_ha": 100 * 6.25 / 10000}]
    assert (block["source"], block["features"], block["dropped"], block["grid"], block["zone_scale"], block["file"]) == \
        ("fields.geojson", 3, 1, [80, 120], 1, "out/x_zones.tif")
    assert json.loads(json.dumps(block)) == block
    assert xz.metadata_block({"type": "x"}, 1, table[:1], 0, (1, 1), 1, None, np.array([0, 1], np.uint64), None)["labels"][0]["area_ha"] is None


# ---- csrc/zone_bins.h ---------------------------------------------------------------------------------------------------------------------------
def _case_text(feats, Z, H, W):
    xy, ring_start, feat_start, label = zm.tables(feats)
    nums = [len(label), Z, H, W, len(xy), len(ring_start) - 1] + xy.ravel().tolist() + ring_start.tolist() + feat_start.tolist() + label.tolist()
    return " ".join(str(int(v)) for v in nums)


def test_zone_bins_under_address_and_ub_sanitizers(tmp_path):
    """csrc/zone_bins.h checks the caller's tables and builds the candidate lists the kernel indexes with: tests/native/zone_bins_main.cpp
    drives it on exact-size heap tables under ASan / UBSan and prints its bins, which are the model's candidate sets: every scene of
    the GPU tests, a feature that meets no tile, one that meets every tile, the unit squares and the star."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "zone_bins"
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", str(REPO / "sentinel2-super-resolution-poc_amd" / "csrc"),
                        str(REPO / "tests" / "native" / "zone_bins_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    cases = [(*zm.scene(H, W), H, W) for H, W in SHAPES] + [(*zm.unit_squares(), 65, 129), (*zm.star(255, 257), 255, 257)]
    (tmp_path / "cases.txt").write_text(f"{len(cases)}\n" + "\n".join(_case_text(*c) for c in cases) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    lines = r.stdout.strip().split("\n")
    at = 0
    for i, (feats, Z, H, W) in enumerate(cases):
        sets, dropped = zm.bins(feats, H, W)
        assert lines[at] == f"case {i} {-(-W // 64)} {-(-H // 64)} {dropped}", lines[at]
        for t, want in enumerate(sets):
            assert lines[at + 1 + t] == f"{t}:" + "".join(f" {f}" for f in want), (i, t)
        at += 1 + len(sets)
    assert at == len(lines)
    feats, Z = zm.scene(255, 257)
    sets, dropped = zm.bins(feats, 255, 257)
    assert dropped == 1 and len(sets) == 20 and all(0 in s for s in sets)          # one feature meets no tile, the first meets every tile
    assert len({tuple(s) for s in sets}) > 4                                         # and the lists differ from tile to tile


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_and_refuses_a_null_handle():
    name = "s2sr_zones_rasterize_u16"
    assert name in native.EXPORTED_SYMBOLS and re.search(rf"\b{name}\(", HEADER)
    decl = re.search(rf"{name}\(([^;]*)\);", HEADER).group(1)
    assert len([a for a in re.sub(r"/\*.*?\*/", "", decl).split(",") if a.strip()]) == len(native._PROTOS[name][1]) == 12
    lib = native.load_library()
    assert lib.s2sr_zones_rasterize_u16(None, None, None, None, None, 1, 1, 1, 1, 0, None, None) == -1
    assert "scratch" in HEADER[HEADER.index("Polygons to zone labels"):HEADER.index(name)] and "voids" in HEADER[HEADER.index("Polygons to zone labels"):HEADER.index(name)]
