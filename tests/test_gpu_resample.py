"""GPU parity of the resampled tile levels (csrc/resample.hip through s2sr_tiles_resample_u8): the device's bytes equal the integer
model (tests/resample_model.py) on the same tap tables in every case -- and Pillow's own bytes once, directly -- then the chain
into the device PNG writer, the two application doors (generate_xyz_tiles with a filter, run_esrgan_and_tiles) and the unchanged
"average" door.  Shapes are the smallest at which the passes can still go wrong; the source is 37 x 53 with an opaque part, a hole
and partial alpha."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import resample_model as rm
from s2sr import geo, native, tiles
from s2sr import rasterio_lite as rio
from s2sr.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

H, W = rm.H, rm.W
SRC = rm.source()
# the box leaves the raster on all four sides: taps clipped at both ends of both axes, columns and rows with no tap at all (west
# and north of the filter's reach), and the two northern tiles transparent.  x9 across, x6.1 down.
OVERZOOM = (-3.7, -46.0, -3.7 + 512 / 9.0, 38.1)


@pytest.fixture(scope="module")
def eng():
    e = native.Engine(num_block=1)
    yield e
    e.close()


def _tables(box, nx, ny, filt, n_cols=W, n_rows=H):
    return (tiles.plan_resample_axis(nx * 256, box[0], box[2], n_cols, filt), tiles.plan_resample_axis(ny * 256, box[1], box[3], n_rows, filt))


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint8
    assert int((got != want).sum()) == 0, (int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


_OVERZOOM_WANT = {}


def _overzoom_want(filt):
    if filt not in _OVERZOOM_WANT:
        cols, rows = _tables(OVERZOOM, 2, 2, filt)
        _OVERZOOM_WANT[filt] = (cols, rows, rm.apply_tables(SRC, rm.SRC_RASTER, cols, rows, 2, 2))
    return _OVERZOOM_WANT[filt]


@pytest.mark.parametrize("filt", tiles.FILTERS)
def test_raster_overzoom_two_by_two_tiles(eng, filt):
    cols, rows, want = _overzoom_want(filt)
    for first, count, _coef, K in (cols, rows):             # the case holds what it is meant to hold
        assert (count == 0).any() and (count == K).any() and ((count > 0) & (count < K) & (first == 0)).any()
        assert ((count > 0) & (count < K) & (first > 0)).any()
    assert not want[0][..., 3].any() and want[1, 0][..., 3].any() and want[1, 1][..., 3].any()
    assert ((want[..., 3] > 0) & (want[..., 3] < 255)).any()
    _same(eng.tiles_resample_u8(SRC, cols, rows, 2, 2), want)


@pytest.mark.parametrize("filt", tiles.FILTERS)
def test_raster_minify_one_tile_reads_a_strict_subrange_of_rows(eng, filt):
    box = (-100.0, 12.0, -100.0 + 256 * 2.7, 12.0 + 256 * 2.7)
    cols, rows = _tables(box, 1, 1, filt)
    used = rows[1] > 0
    assert rows[0][used].min() > 0 and (rows[0] + rows[1])[used].max() == H          # the horizontal pass skips the first source rows
    if filt == "lanczos":
        assert cols[3] == 17 and rows[3] == 17
    want = rm.apply_tables(SRC, rm.SRC_RASTER, cols, rows, 1, 1)
    assert want[..., 3].any()
    _same(eng.tiles_resample_u8(SRC, cols, rows, 1, 1), want)


def test_tap_limit_and_refused_tables(eng):
    """Lanczos at 64 / 6 source pixels per tile pixel needs exactly 64 taps: the raster covers a handful of output pixels.  Then
    hand-made tables the entry must refuse before it touches the device -- and the engine still answers the first case."""
    scale = 64.0 / 6.0
    box = (-1000.0, -1200.0, -1000.0 + 256 * scale, -1200.0 + 256 * scale)
    cols, rows = _tables(box, 1, 1, "lanczos")
    assert cols[3] == 64 and rows[3] == 64 and cols[1].max() == W and rows[1].max() == H
    want = rm.apply_tables(SRC, rm.SRC_RASTER, cols, rows, 1, 1)
    assert 9 <= int((want[0, 0, ..., 3] > 0).sum()) <= 200
    _same(eng.tiles_resample_u8(SRC, cols, rows, 1, 1), want)

    first, count, coef, K = cols
    wide = (first, count, np.concatenate([coef, np.zeros((256, 1), np.int32)], 1))                   # K = 65
    with pytest.raises(native.S2srError, match="1..64"):
        eng.tiles_resample_u8(SRC, wide, rows, 1, 1)
    with pytest.raises(native.S2srError, match="1..64"):
        eng.tiles_resample_u8(SRC, cols, wide, 1, 1)
    j = int(np.argmax(count))
    past = first.copy()
    past[j] = W - count[j] + 1                                                                       # first + count = W + 1
    with pytest.raises(native.S2srError, match="leave the source"):
        eng.tiles_resample_u8(SRC, (past, count, coef), rows, 1, 1)
    neg = first.copy()
    neg[j] = -1
    with pytest.raises(native.S2srError, match="leave the source"):
        eng.tiles_resample_u8(SRC, (neg, count, coef), rows, 1, 1)
    many = count.copy()
    many[j] = K + 1
    with pytest.raises(native.S2srError, match="0..K"):
        eng.tiles_resample_u8(SRC, (first, many, coef), rows, 1, 1)
    big = coef.copy()
    big[j, 0], big[j, 1] = 5_000_000, -4_000_000                                                     # 255 * 9e6 > 2^31
    with pytest.raises(native.S2srError, match="overflow"):
        eng.tiles_resample_u8(SRC, (first, count, big), rows, 1, 1)
    with pytest.raises(native.S2srError, match="overflow"):
        eng.tiles_resample_u8(SRC, cols, (rows[0], rows[1], np.where(rows[2] != 0, 2 ** 30, 0).astype(np.int32)), 1, 1)
    with pytest.raises(native.S2srError, match="did not leave a warped raster"):                     # nothing left a raster on the device
        eng.tiles_resample_u8((H, W), cols, rows, 1, 1, on_device=True)
    c1, r1, want1 = _overzoom_want("lanczos")
    _same(eng.tiles_resample_u8(SRC, c1, r1, 2, 2), want1)


def test_level_source_parent_reaches_past_the_child(eng):
    """Child 3 x 2 tiles, parent 2 x 2 with ox = -1, oy = 0: the west half of the parent's first tile column and its south tile row
    lie outside the child, and so do taps.  Host-fed and from the device copy a base call left; a wrong level shape is not "the previous level"."""
    child_lv = tiles.LevelPlan(12, 21, 10, 23, 11)
    parent_lv = tiles.LevelPlan(11, 10, 4, 11, 5)
    assert tiles.overview_offsets(parent_lv, child_lv) == (-1, 0) and (child_lv.nx, child_lv.ny, parent_lv.nx, parent_lv.ny) == (3, 2, 2, 2)
    bc, br = _tables((-2.5, -3.0, 55.0, 39.5), 3, 2, "cubic")
    child = eng.tiles_resample_u8(SRC, bc, br, 3, 2)
    _same(child, rm.apply_tables(SRC, rm.SRC_RASTER, bc, br, 3, 2))
    for filt in tiles.FILTERS:
        cols, rows = tiles.plan_resample_level(parent_lv, tiles.overview_box(parent_lv, child_lv), 3 * 256, 2 * 256, filt)
        assert (cols[1][:120] == 0).all() and cols[1][256] > 0 and (rows[1][-250:] == 0).all()      # parent pixel j sits at child pixel 2j - 256
        assert ((cols[1] > 0) & (cols[1] < cols[1].max()) & (cols[0] == 0)).any()      # taps clipped at the child's west edge
        want = rm.apply_tables(child, rm.SRC_LEVEL, cols, rows, 2, 2)
        assert not want[:, 0, :, :120, 3].any() and want[0, 0][..., 3].any() and want[0, 1][..., 3].any() and not want[1, :, 6:, :, 3].any()
        _same(eng.tiles_resample_u8(child, cols, rows, 2, 2), want)                    # host-fed
        eng.tiles_resample_u8(SRC, bc, br, 3, 2, fetch=False)                          # the base call leaves the child on the device
        with pytest.raises(native.S2srError, match="did not leave a tile level"):
            eng.tiles_resample_u8(None, cols, rows, 2, 2, level_shape=(2, 4), on_device=True)       # (tables that fit it: the size is what is wrong)
        _same(eng.tiles_resample_u8(None, cols, rows, 2, 2, level_shape=(2, 3), on_device=True), want)
    # the averaged overview finds a resampled level too, and the resampler an averaged one
    eng.tiles_resample_u8(SRC, bc, br, 3, 2, fetch=False)
    from oracle import tiles_ref as ref
    _same(eng.tiles_overview_u8((2, 3), -1, 0, 2, 2, on_device=True), ref.overview(child, -1, 0, 2, 2))
    ident_c, ident_r = np.minimum(np.arange(768) // 15, W - 1).astype(np.int32), np.minimum(np.arange(512) // 14, H - 1).astype(np.int32)
    base = eng.tiles_base_u8(SRC, ident_c, ident_c, ident_r, ident_r)
    cols, rows = tiles.plan_resample_level(parent_lv, tiles.overview_box(parent_lv, child_lv), 768, 512, "lanczos")
    _same(eng.tiles_resample_u8(None, cols, rows, 2, 2, level_shape=(2, 3), on_device=True), rm.apply_tables(base, rm.SRC_LEVEL, cols, rows, 2, 2))


@pytest.mark.parametrize("filt", tiles.FILTERS)
def test_device_equals_pillow_directly(eng, filt):
    box = (-4.5, -3.25, 59.5, 60.75)                       # dyadic: exact in Pillow's float32 box; x8 over-zoom
    cols, rows = _tables(box, 2, 2, filt)
    got = eng.tiles_resample_u8(SRC, cols, rows, 2, 2)
    _same(rm.mosaic(got), rm.pillow_resize(SRC, box, (512, 512), filt))


def test_chain_warp_resample_overview_png(eng, tmp_path):
    """warp -> resample from the warped raster's device copy -> Lanczos overview from the level's device copy -> XYZ PNG files of
    both levels: the files decode to the model's bytes (fractional alpha included); tiles without coverage get no file."""
    rgb = np.ascontiguousarray(SRC[..., :3])
    plan = tiles.plan_warp(W, H, geo.Placement(600000.0, 5100000.0, 2.5, 2.5), geo.CRS(32633))
    rgba = eng.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w)
    place, h, w = plan.placement, plan.out_h, plan.out_w
    levels = tiles.plan_levels(place.bounds(w, h), 17, 18)
    want, prev, n_files, n_empty, fractional = None, None, 0, 0, False
    for lv in levels:
        if prev is None:
            cols, rows = tiles.plan_resample_level(lv, tiles.level_box(lv, place), w, h, "lanczos")
            assert eng.tiles_resample_u8((h, w), cols, rows, lv.nx, lv.ny, on_device=True, fetch=False) is None
            want = rm.apply_tables(np.asarray(rgba), rm.SRC_RASTER, cols, rows, lv.nx, lv.ny)
        else:
            cols, rows = tiles.plan_resample_level(lv, tiles.overview_box(lv, prev), prev.nx * 256, prev.ny * 256, "lanczos")
            assert eng.tiles_resample_u8(None, cols, rows, lv.nx, lv.ny, level_shape=(prev.ny, prev.nx), on_device=True, fetch=False) is None
            want = rm.apply_tables(want, rm.SRC_LEVEL, cols, rows, lv.nx, lv.ny)
        y_rows = [geo.xyz_row(lv.tmaxy - j, lv.zoom) for j in range(lv.ny)]
        wrote = eng.tiles_write_png_xyz(lv.nx, lv.ny, tmp_path, lv.zoom, lv.tminx, y_rows)
        for j in range(lv.ny):
            for i in range(lv.nx):
                q = tmp_path / str(lv.zoom) / str(lv.tminx + i) / f"{y_rows[j]}.png"
                has = bool(want[j, i, ..., 3].any())
                assert bool(wrote[j, i]) == has == q.exists(), (lv.zoom, j, i)
                if has:
                    _same(np.asarray(Image.open(q)), want[j, i])
                    n_files += 1
                    fractional |= bool(((want[j, i, ..., 3] > 0) & (want[j, i, ..., 3] < 255)).any())
                else:
                    n_empty += 1
        prev = lv
    assert n_files >= 2 and fractional
    # a level with tiles nothing reaches: the same raster in a mosaic two tiles wider than its level
    lv = levels[0]
    wide = tiles.LevelPlan(lv.zoom, lv.tminx, lv.tminy, lv.tmaxx + 2, lv.tmaxy)
    cols, rows = tiles.plan_resample_level(wide, tiles.level_box(wide, place), w, h, "lanczos")
    eng.tiles_resample_u8(np.asarray(rgba), cols, rows, wide.nx, wide.ny, fetch=False)
    wrote = eng.tiles_write_png_xyz(wide.nx, wide.ny, tmp_path / "wide", wide.zoom, wide.tminx, [geo.xyz_row(wide.tmaxy - j, wide.zoom) for j in range(wide.ny)])
    assert not wrote[:, -1].any() and wrote.any() and not list((tmp_path / "wide" / str(wide.zoom) / str(wide.tmaxx)).glob("*.png"))


def _scene(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([120 + 90 * np.sin(xx / 6.0 + c) * np.cos(yy / 4.0) + rng.integers(-15, 16, (h, w)) for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


def _files(root):
    return {str(q.relative_to(root)): q.read_bytes() for q in sorted(root.glob("*/*/*.png"))}


def _mercator_tif(path, rgb, zoom=17):
    """A 3857 GeoTIFF whose raster straddles a corner of z`zoom` tiles: four tiles at the deepest zoom."""
    import app.tiling as tiling
    tx, ty = geo.meters_to_tile(1500000.0, 6000000.0, zoom)
    west, south, _east, _north = geo.tile_bounds(tx, ty, zoom)
    place = geo.Placement(west - 60.3, south + 55.1, 2.4, 2.4)          # the corner (west, south) lies inside the raster
    rio.write_geotiff_rgb(path, rgb, tiling._mercator_tags(place))
    return place


def test_generate_xyz_tiles_lanczos_against_the_model(tmp_path):
    """generate_xyz_tiles(resampling="lanczos") on a 40 x 56 EPSG:3857 GeoTIFF, z17..15 (x2 over-zoom, about 1:1, x2 minified):
    every file is the model's tile, run level by level with the planner's tables; every tile the model gives coverage has a file;
    the files "average" writes -- the tiles the raster covers -- are among them (Lanczos may add tiles only its support reaches)."""
    import app.tiling as tiling
    rgb = _scene(40, 56, seed=3)
    place = _mercator_tif(tmp_path / "m.tif", rgb)
    out = tiling.generate_xyz_tiles(tmp_path / "m.tif", tmp_path / "lz", min_zoom=15, max_zoom=17, resampling="lanczos")
    assert out == tmp_path / "lz"
    rgba = np.dstack([rgb, np.full((40, 56), 255, np.uint8)])
    levels = tiles.plan_levels(place.bounds(56, 40), 15, 17)
    assert (levels[0].nx, levels[0].ny) == (2, 2)
    want, prev, expected = None, None, set()
    for lv in levels:
        if prev is None:
            cols, rows = tiles.plan_resample_level(lv, tiles.level_box(lv, place), 56, 40, "lanczos")
            want = rm.apply_tables(rgba, rm.SRC_RASTER, cols, rows, lv.nx, lv.ny)
        else:
            cols, rows = tiles.plan_resample_level(lv, tiles.overview_box(lv, prev), prev.nx * 256, prev.ny * 256, "lanczos")
            want = rm.apply_tables(want, rm.SRC_LEVEL, cols, rows, lv.nx, lv.ny)
        for j in range(lv.ny):
            for i in range(lv.nx):
                if want[j, i, ..., 3].any():
                    name = f"{lv.zoom}/{lv.tminx + i}/{geo.xyz_row(lv.tmaxy - j, lv.zoom)}.png"
                    expected.add(name)
                    _same(np.asarray(Image.open(tmp_path / "lz" / name)), want[j, i])
        prev = lv
    got = set(_files(tmp_path / "lz"))
    assert got == expected and len(got) >= 6
    tiling.generate_xyz_tiles(tmp_path / "m.tif", tmp_path / "av", min_zoom=15, max_zoom=17, resampling="average")
    assert set(_files(tmp_path / "av")) <= got
    for name in ("cubic", "bilinear"):                      # the other two filters go the same way: same tiles, other bytes
        tiling.generate_xyz_tiles(tmp_path / "m.tif", tmp_path / name, min_zoom=16, max_zoom=17, resampling=name)
        assert set(_files(tmp_path / name)) == {k for k in got if not k.startswith("15/")}


def test_average_door_is_unchanged(tmp_path):
    """resampling="average" and the default write the same files, byte for byte (tests/test_gpu_tiles.py judges their content)."""
    import app.tiling as tiling
    _mercator_tif(tmp_path / "m.tif", _scene(40, 56, seed=4))
    tiling.generate_xyz_tiles(tmp_path / "m.tif", tmp_path / "a", min_zoom=15, max_zoom=17)
    tiling.generate_xyz_tiles(tmp_path / "m.tif", tmp_path / "b", min_zoom=15, max_zoom=17, resampling="average")
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert a == b and len(a) >= 6
    t = np.asarray(Image.open(tmp_path / "a" / sorted(a)[-1]))
    assert set(np.unique(t[..., 3]).tolist()) <= {0, 255}                                 # footprint means: alpha is never fractional


def test_run_esrgan_and_tiles(monkeypatch, tmp_path):
    """The SR-to-tiles job on a 24 x 32 UTM GeoTIFF (10 m pixels) with a seeded 1-block checkpoint: x4 GeoTIFF under sr_esrgan/,
    reprojection, a z18-20 Lanczos pyramid under tiles_esrgan/ with the job's tile template; skip_sr on the written raster cuts the
    same tiles."""
    import app.cnn_super_resolution as m
    import app.tiling as tiling
    from app.esrgan_tiles import run_esrgan_and_tiles
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir()
    monkeypatch.setitem(m.MODELS, "realesrgan_x4", {**m.MODELS["realesrgan_x4"], "blocks": 1})
    sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(1, seed=0).items()}
    torch.save({"params_ema": sd}, tmp_path / "models" / "realesrgan_x4.pth")
    georef = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0),
                         rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633)})
    rio.write_geotiff_rgb(tmp_path / "s2.tif", _scene(24, 32, seed=8), georef)
    res = run_esrgan_and_tiles(tmp_path / "s2.tif", tmp_path / "out")
    assert res.get("status") == "completed", res
    assert {"timestamp", "input", "min_zoom", "max_zoom", "steps", "status", "sr_output", "tiles_dir", "tile_count"} <= set(res)
    assert (res["input"], res["min_zoom"], res["max_zoom"]) == (str(tmp_path / "s2.tif"), 18, 20)
    assert [(s["step"], s["name"], s["status"]) for s in res["steps"]] == [(1, "Real-ESRGAN SR", "completed"), (2, "Tile Generation", "completed")]
    sr_tif, tdir = tmp_path / "out" / "sr_esrgan" / "s2_esrgan_x4.tif", tmp_path / "out" / "tiles_esrgan"
    assert res["sr_output"] == str(sr_tif) == res["steps"][0]["output"] and res["tiles_dir"] == str(tdir) == res["steps"][1]["output_dir"]
    info = tiling.get_raster_info(sr_tif)
    assert (info.crs, info.width, info.height) == ("EPSG:32633", 128, 96)
    assert (tmp_path / "out" / "sr_esrgan" / "s2_esrgan_x4_3857.tif").exists()
    meta = json.loads((tdir / "tileset.json").read_text())
    assert meta["tileTemplate"] == "/tiles_esrgan/{z}/{x}/{y}.png" and (meta["minzoom"], meta["maxzoom"]) == (18, 20)
    assert meta == res["steps"][1]["metadata"] and res["steps"][1]["zoom_levels"] == [18, 19, 20]
    files = _files(tdir)
    assert res["tile_count"] == res["steps"][1]["tile_count"] == len(files) and {k.split("/")[0] for k in files} == {"18", "19", "20"}
    # the tiles plan_levels predicts for the warped raster: no file outside them; the files "average" writes for the same raster
    # (the tiles it covers) are all there; what Lanczos adds are tiles only its support reaches
    arr, g3857 = rio.read_rgb_u8(tmp_path / "out" / "sr_esrgan" / "s2_esrgan_x4_3857.tif")
    place = geo.placement_from_tags(g3857.tags)
    levels = tiles.plan_levels(place.bounds(arr.shape[1], arr.shape[0]), 18, 20)
    planned = {f"{lv.zoom}/{lv.tminx + i}/{geo.xyz_row(lv.tmaxy - j, lv.zoom)}.png" for lv in levels for j in range(lv.ny) for i in range(lv.nx)}
    tiling.process_raster_to_tiles(sr_tif, tmp_path / "avg", min_zoom=18, max_zoom=20)
    covered = set(_files(tmp_path / "avg"))
    assert covered <= set(files) <= planned
    print(f"z18-20: {len(planned)} planned, {len(covered)} covered, {len(files)} written with Lanczos")
    t = np.asarray(Image.open(tdir / sorted(files)[0]))
    assert t.shape == (256, 256, 4) and t[..., 3].any()
    # the same tiles from the written raster alone
    res2 = run_esrgan_and_tiles(tmp_path / "s2.tif", tmp_path / "out2", skip_sr=True, sr_output=sr_tif)
    assert [s["status"] for s in res2["steps"]] == ["skipped", "completed"] and res2["status"] == "completed"
    assert res2["sr_output"] == str(sr_tif) and _files(tmp_path / "out2" / "tiles_esrgan") == files
    assert not list((tmp_path / "out2" / "sr_esrgan").iterdir())
