"""The nodata-transparent tile pyramid on the GPU: the masked warp (csrc/tiles.hip warp_bilinear_masked_kernel
through s2sr_warp_bilinear_masked_u8) against its numpy model byte for byte, the pyramid chained on the raster it keeps, the tiler
and one /api/wow job, and the door under caps 1 and 3.  No tolerance anywhere: every comparison is of bytes.  The door under red zones,
poison, stalls and cap 8: its two rows of tests/doors.py, whose baselines this module holds to the model (what the door reads is in the
list of tests/test_gpu_poison.py).

Each figure is printed before it is judged (pytest -s).  The model's outputs are computed once per case and shared."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import diag
import doors
import warp_masked_model as wm
from diag import keep, same
from doors import Inputs
from s2sr import geo, native, tiles
from warp_masked_model import H, W
from warp_masked_model import case as _case
from warp_masked_model import warp as _warp
from s2sr import rasterio_lite as rio
from tiff_fixture import write_tiff

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def eng():
    e = native.Engine(num_block=1)
    yield e
    e.close()


def _differ(got, want):
    return int((np.asarray(got) != np.asarray(want)).sum())


# ---- the kernel against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "coarse", "thirds", "none"])
@pytest.mark.parametrize("epsg", [s[0] for s in wm.SCENES])
def test_kernel_equals_model(eng, epsg, kind):
    rgb, valid, vs, plan, want = _case(epsg, kind)
    got = _warp(eng, rgb, valid, vs, plan)
    a = want[..., 3]
    print(f"EPSG:{epsg} {kind}: vs {vs}, mask {valid.shape} {1 - valid.mean():.2f} invalid, raster {want.shape[:2]}, alpha 0 in {(a == 0).mean():.3f}, "
          f"{_differ(got, want)} bytes differ")
    assert got.shape == (plan.out_h, plan.out_w, 4) and got.dtype == np.uint8
    assert np.array_equal(got, want), _differ(got, want)
    if kind == "none":
        assert not got.any()
    else:
        assert 0.2 < (a == 0).mean() < 0.8                       # the mask bites and leaves something
        if kind == "coarse":
            assert valid.shape == (38, 53) and H % 4 and W % 4   # the last mask row and column are partly used


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (7, 1)])
def test_kernel_equals_model_on_degenerate_sources(eng, h, w):
    """every tap is edge-replicated in at least one direction; the identity warp shifted by a fraction so that weights are mixed"""
    rgb = wm.scene(h, w, seed=h * 10 + w)
    grid = wm.identity_grid(h + 2, w + 2, step=4, shift=(-0.75, -0.625))
    masks = [np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8)]
    if h * w > 1:
        alt = (np.arange(h * w).reshape(h, w) % 3 != 1).astype(np.uint8)
        masks += [alt, 1 - alt]
    for k, valid in enumerate(masks):
        got = eng.warp_bilinear_u8(rgb, grid, 4, h + 2, w + 2, valid=valid, valid_scale=1)
        want = wm.warp_bilinear_masked(rgb, valid, 1, grid, 4, h + 2, w + 2)
        print(f"{h} x {w}, mask {k}: alpha 255 in {int((want[..., 3] == 255).sum())} of {want[..., 3].size}, {_differ(got, want)} bytes differ")
        assert np.array_equal(got, want)
    for vs in (2, 3, 16):                                        # one mask byte covers several pixels, or the whole source
        valid = np.ones((-(-h // vs), -(-w // vs)), np.uint8)
        assert np.array_equal(eng.warp_bilinear_u8(rgb, grid, 4, h + 2, w + 2, valid=valid, valid_scale=vs),
                              eng.warp_bilinear_u8(rgb, grid, 4, h + 2, w + 2))


@pytest.mark.parametrize("epsg", [s[0] for s in wm.SCENES])
def test_all_valid_mask_is_the_plain_warp(eng, epsg):
    rgb, valid, vs, plan, want = _case(epsg, "every")
    plain = keep(eng.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w))
    for v, s in ((valid, vs), _case(epsg, "every3")[1:3], (np.ones((H, W), np.uint8), 1), (np.full((H, W), 255, np.uint8), 1)):
        got = _warp(eng, rgb, v, s, plan)
        print(f"EPSG:{epsg} all valid at vs {s}: {_differ(got, plain)} bytes differ from warp_bilinear_u8")
        assert np.array_equal(got, plain)
    assert np.array_equal(plain, want)


@pytest.mark.parametrize("kind", ["mixed", "coarse"])
def test_invalid_pixel_values_never_reach_the_output(eng, kind):
    rgb, valid, vs, plan, want = _case(32633, kind)
    for how in (0, 255, "random"):
        got = _warp(eng, wm.repaint(rgb, valid, vs, how), valid, vs, plan)
        print(f"{kind}, invalid pixels repainted {how}: {_differ(got, want)} bytes differ")
        assert np.array_equal(got, want), how
    assert not want[want[..., 3] == 0].any() and np.isin(want[..., 3], (0, 255)).all()


def test_refusals(eng):
    rgb, valid, vs, plan, _ = _case(32633, "coarse")
    lib, h = eng._lib, eng._h
    out = np.zeros((plan.out_h, plan.out_w, 4), np.uint8)
    grid = np.ascontiguousarray(plan.grid, np.float32)
    args = lambda v, s, step=plan.step, g=grid: (h, rgb.ctypes.data, H, W, v, s, g.ctypes.data, g.shape[0], g.shape[1], step, plan.out_h, plan.out_w,
                                                 out.ctypes.data)
    assert lib.s2sr_warp_bilinear_masked_u8(*args(None, 4)) != 0 and b"valid is NULL" in lib.s2sr_last_error(h)
    assert lib.s2sr_warp_bilinear_masked_u8(*args(valid.ctypes.data, 0)) != 0 and b"valid_scale" in lib.s2sr_last_error(h)
    with pytest.raises(native.S2srError, match="power of two"):
        eng.warp_bilinear_u8(rgb, plan.grid, 12, plan.out_h, plan.out_w, valid=valid, valid_scale=vs)
    with pytest.raises(native.S2srError, match="does not cover"):
        eng.warp_bilinear_u8(rgb, plan.grid[:-1], plan.step, plan.out_h, plan.out_w, valid=valid, valid_scale=vs)
    with pytest.raises(ValueError, match="valid: expected uint8"):
        eng.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w, valid=valid, valid_scale=1)
    assert not out.any()


# ---- the pyramid behind the masked warp ------------------------------------------------------------------------------------------------
def _big_case():
    """The 300 x 420 scene of test_base_and_overview_bit_exact as a UTM raster of 10 m pixels (3 x 4.2 km: some 4 x 5 tiles at z15,
    whose tiles are 1223 Mercator metres, about 850 m on the ground here), z12-15 on the warped grid.  The mask, at vs = 4, has
    random holes and a hole of 200 x 280 source pixels at the north-west corner: more than two tiles each way, so it holds a whole one."""
    rgb = wm.scene(300, 420, seed=2)
    valid = wm.mask_coarse(300, 420, 4, seed=9)
    valid[:50, :70] = 0
    plan = tiles.plan_warp(420, 300, geo.Placement(600000.0, 5100000.0, 10.0, 10.0), geo.CRS(32633))
    levels = tiles.plan_levels(plan.placement.bounds(plan.out_w, plan.out_h), 12, 15)
    return rgb, valid, plan, levels


def _chain(e, raster, plan, levels, tmp, resampling, on_device):
    """base (z15) from the raster, overviews / resampled levels up to z12, each fetched and written as PNGs -> [(level, files, wrote)]"""
    place = plan.placement
    h, w = raster.shape[:2] if hasattr(raster, "shape") else raster
    out, prev = [], None
    for lv in levels:
        if resampling == "average":
            if prev is None:
                got = e.tiles_base_u8(raster, *tiles.plan_base(lv, place, w, h), on_device=on_device)
            else:
                ox, oy = tiles.overview_offsets(lv, prev)
                got = e.tiles_overview_u8((prev.ny, prev.nx), ox, oy, lv.nx, lv.ny, on_device=True)
        elif prev is None:
            cols, rows = tiles.plan_resample_level(lv, tiles.level_box(lv, place), w, h, resampling)
            got = e.tiles_resample_u8(raster, cols, rows, lv.nx, lv.ny, on_device=on_device)
        else:
            cols, rows = tiles.plan_resample_level(lv, tiles.overview_box(lv, prev), prev.nx * geo.TILE, prev.ny * geo.TILE, resampling)
            got = e.tiles_resample_u8(None, cols, rows, lv.nx, lv.ny, level_shape=(prev.ny, prev.nx), on_device=True)
        got = keep(got)
        paths = [tmp / f"{resampling}{int(on_device)}" / str(lv.zoom) / f"{j}_{i}.png" for j in range(lv.ny) for i in range(lv.nx)]
        wrote = keep(e.tiles_write_png(lv.nx, lv.ny, paths))
        out.append((got, [q.read_bytes() if q.exists() else None for q in paths], wrote))
        prev = lv
    return out


@pytest.mark.parametrize("resampling", ["average", "lanczos"])
def test_pyramid_chain_on_the_kept_raster(eng, tmp_path, resampling):
    rgb, valid, plan, levels = _big_case()
    host = keep(eng.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w, valid=valid, valid_scale=4))
    want = _chain(eng, host, plan, levels, tmp_path, resampling, on_device=False)
    eng.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w, valid=valid, valid_scale=4)
    got = _chain(eng, host.shape[:2], plan, levels, tmp_path, resampling, on_device=True)
    absent = 0
    for lv, (g, gf, gw), (w_, wf, ww) in zip(levels, got, want):
        print(f"{resampling} z{lv.zoom}: {lv.nx} x {lv.ny} tiles, {int(gw.sum())} files, {_differ(g, w_)} bytes differ from the chain fed the host copy")
        assert np.array_equal(g, w_) and np.array_equal(gw, ww) and gf == wf
        for j in range(lv.ny):
            for i in range(lv.nx):
                assert bool(gw[j, i]) == bool(g[j, i, ..., 3].any()) == (gf[j * lv.nx + i] is not None)
        absent += int((gw == 0).sum())
    # z15 tiles wholly inside the hole produce no file: the tiles the plain warp covers (in part or whole) and the masked one leaves empty
    lv = levels[0]
    plain = keep(eng.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w))
    covered = keep(eng.tiles_base_u8(plain, *tiles.plan_base(lv, plan.placement, plan.out_w, plan.out_h)))[..., 3]
    in_hole = [(j, i) for j in range(lv.ny) for i in range(lv.nx) if covered[j, i].any() and not got[0][0][j, i, ..., 3].any()]
    whole = [(j, i) for j, i in in_hole if covered[j, i].all()]
    print(f"{resampling}: z15 is {lv.nx} x {lv.ny}; tiles the plain warp covers and the mask empties: {in_hole}, of which fully covered: {whole}; "
          f"tiles without a file, all levels: {absent}")
    assert in_hole and all(not got[0][2][j, i] and got[0][1][j * lv.nx + i] is None for j, i in in_hole)
    if resampling == "average":
        assert whole


# ---- the kept raster: the masked warp is a "raster" producer (tests/test_gpu_kept.py) ---------------------------------------------------
K_RGB = np.random.default_rng(20261020).integers(0, 256, (4, 4, 3), dtype=np.uint8)
K_VALID = np.array([[1, 1, 1, 0], [1, 1, 1, 1], [0, 1, 1, 1], [1, 1, 1, 1]], np.uint8)
K_GRID = np.stack(np.meshgrid(np.arange(2) * 4.0, np.arange(2) * 4.0), -1).astype(np.float32)      # the identity warp


def _footprint(n):
    return (np.arange(256) * n // 256).astype(np.int32)


def _k_base(e, src, size):
    h, w = size
    return e.tiles_base_u8(size if src is None else src, _footprint(w), _footprint(w), _footprint(h), _footprint(h), on_device=src is None)


def _k_resample(e, src, size):
    h, w = size
    taps = lambda n: tiles.plan_resample_axis(256, 0.0, float(n), n, "bilinear")
    return e.tiles_resample_u8(size if src is None else src, taps(w), taps(h), 1, 1, on_device=src is None)


@pytest.mark.parametrize("between", ["direct", "synchronize", "scratch_taker"])
def test_the_masked_warp_keeps_its_raster(eng, between):
    produce = lambda: eng.warp_bilinear_u8(K_RGB, K_GRID, 4, 4, 4, valid=K_VALID, valid_scale=1)
    host = keep(produce())
    assert host[0, 3, 3] == 0 and host[2, 0, 3] == 0 and (host[..., 3] == 255).sum() == 14
    for name, call, other in (("tiles_base_u8", _k_base, (4, 5)), ("tiles_resample_u8", _k_resample, (5, 4))):
        want = keep(call(eng, host, (4, 4)))
        for size in ((4, 4), other):
            produce()
            if between == "synchronize":
                eng.synchronize()
            elif between == "scratch_taker":
                eng.postprocess_u8(np.full((5, 9, 3), 90, np.uint8), native.pp_wow())
            takes = size == (4, 4) and between != "scratch_taker"
            print(f"{between:14s} masked warp -> {name} {size}: {'bytes' if takes else 'refused'}")
            if takes:
                same(keep(call(eng, None, size)), want, f"{name} behind the masked warp, {between}")
            else:
                with pytest.raises(native.S2srError, match="did not leave a warped raster"):
                    call(eng, None, size)


# ---- the tiler ---------------------------------------------------------------------------------------------------------------------------
UTM = [(33550, 12, (2.5, 2.5, 0.0)), (33922, 12, (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0)),
       (34735, 3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633))]
NODATA_TAG = (42113, 2, "0")


def _tree(d):
    return {str(q.relative_to(d)): q.read_bytes() for q in sorted(d.rglob("*")) if q.is_file()}


def _holed_scene():
    rgb = wm.scene(200, 260, seed=5)
    rgb[rgb == 0] = 1                                            # no measured pixel equals the value
    hole = np.zeros((200, 260), bool)
    hole[60:140, 80:200] = True
    hole[:25, :30] = True
    return rgb, hole


def _tile_pixel(mx, my, z):
    """the tile (TMS) and the pixel inside it that hold the Web-Mercator point"""
    tx, ty = geo.meters_to_tile(mx, my, z)
    west, _south, _east, north = geo.tile_bounds(tx, ty, z)
    return tx, ty, min(255, int((north - my) / geo.resolution(z))), min(255, int((mx - west) / geo.resolution(z)))


def test_process_raster_to_tiles_with_a_nodata_tag(tmp_path):
    """~200 x 260 UTM GeoTIFF with GDAL_NODATA = 0, z15-16: the holes as the value (mask from the tag) and as two kinds of junk
    under the caller's own mask give one and the same tile tree and _3857.tif"""
    import app.tiling as tiling
    rgb, hole = _holed_scene()
    out = []
    for k in range(3):
        d = tmp_path / f"t{k}"
        d.mkdir()
        img = rgb.copy()
        img[hole] = 0 if k == 0 else np.random.default_rng(6 + k).integers(1, 256, rgb.shape, dtype=np.uint8)[hole]
        write_tiff(d / "aoi.tif", img, extra=UTM + [NODATA_TAG])
        own = {} if k == 0 else {"valid": (~hole).astype(np.uint8)}
        tiling.process_raster_to_tiles(d / "aoi.tif", d / "tiles", min_zoom=15, max_zoom=16, nodata="tag", **own)
        out.append((_tree(d / "tiles"), (d / "aoi_3857.tif").read_bytes()))
    print(f"{len(out[0][0])} files per tree")
    assert out[0][0] and out[0] == out[1] == out[2], "files whose holes hold different junk give different tiles"
    d = tmp_path / "t0"
    arr, g3857 = rio.read_rgb_u8(d / "aoi_3857.tif")
    place = geo.placement_from_tags(g3857.tags)
    assert g3857.nodata == 0, "the _3857.tif carries the GDAL_NODATA tag"
    # the model of the masked warp says where alpha is 0; the file holds the value there
    plan = tiles.plan_warp(260, 200, geo.Placement(600000.0, 5100000.0, 2.5, 2.5), geo.CRS(32633))
    want = wm.warp_bilinear_masked(rgb, (~hole).astype(np.uint8), 1, plan.grid, plan.step, plan.out_h, plan.out_w)
    assert arr.shape[:2] == want.shape[:2] and np.array_equal(arr, want[..., :3]) and not arr[want[..., 3] == 0].any()
    # decoded tiles have alpha 0 over the hole: the raster pixel the centre of the big hole (source 100, 140) is warped to
    score = np.abs(plan.grid[..., 0] - 140.0) + np.abs(plan.grid[..., 1] - 100.0)
    gi, gj = np.unravel_index(np.argmin(score), score.shape)
    hy, hx = min(gi * plan.step, plan.out_h - 1), min(gj * plan.step, plan.out_w - 1)
    assert want[hy, hx, 3] == 0
    for z in (15, 16):
        for q in (d / "tiles" / str(z)).glob("*/*.png"):
            t = np.asarray(Image.open(q))
            assert t.shape == (256, 256, 4) and np.isin(t[..., 3], (0, 255)).all() and not t[t[..., 3] == 0].any()
        tx, ty, py, px = _tile_pixel(place.x0 + (hx + 0.5) * place.dx, place.y0 - (hy + 0.5) * place.dy, z)
        q = d / "tiles" / str(z) / str(tx) / f"{geo.xyz_row(ty, z)}.png"
        t = np.asarray(Image.open(q)) if q.exists() else np.zeros((256, 256, 4), np.uint8)           # (a tile wholly in the hole has no file)
        print(f"z{z}: tile {tx}/{geo.xyz_row(ty, z)} ({'file' if q.exists() else 'no file'}) pixel ({py}, {px}) over the hole: {t[py, px].tolist()}; "
              f"alpha 0 in {(t[..., 3] == 0).mean():.3f} of the tile")
        assert t[py, px].tolist() == [0, 0, 0, 0]
    # a value other than 0 is held in the alpha-0 pixels of the _3857.tif, the wedges outside the source included
    d = tmp_path / "t7"
    d.mkdir()
    img = rgb.copy()
    img[img == 7] = 8
    img[hole] = 7
    write_tiff(d / "aoi.tif", img, extra=UTM + [(42113, 2, "7")])
    tiling.process_raster_to_tiles(d / "aoi.tif", d / "tiles", min_zoom=15, max_zoom=15, nodata="tag")
    arr7, g7 = rio.read_rgb_u8(d / "aoi_3857.tif")
    wedge = wm.warp_bilinear_masked(rgb, np.ones((200, 260), np.uint8), 1, plan.grid, plan.step, plan.out_h, plan.out_w)[..., 3] == 0
    print(f"value 7: {int((want[..., 3] == 0).sum())} alpha-0 pixels, {int(wedge.sum())} of them outside the source")
    assert g7.nodata == 7 and wedge.any() and (arr7[wedge] == 7).all() and (arr7[want[..., 3] == 0] == 7).all()
    assert np.array_equal(arr7[want[..., 3] == 255], want[want[..., 3] == 255][:, :3])


def test_off_means_off(tmp_path):
    """without the new arguments every file is what a plain call writes: two calls, byte-identical trees and _3857.tif, no tag"""
    import app.tiling as tiling
    rgb, hole = _holed_scene()
    rgb[hole] = 0
    out = []
    for k in range(2):
        d = tmp_path / f"p{k}"
        d.mkdir()
        write_tiff(d / "aoi.tif", rgb, extra=UTM + [NODATA_TAG])               # the tag is there; nobody asked for it
        if k == 0:
            tiling.process_raster_to_tiles(d / "aoi.tif", d / "tiles", min_zoom=15, max_zoom=16)
        else:
            tiling.process_raster_to_tiles(d / "aoi.tif", d / "tiles", min_zoom=15, max_zoom=16, nodata=None, valid=None, valid_scale=1)
        out.append((_tree(d / "tiles"), (d / "aoi_3857.tif").read_bytes()))
    assert out[0][0] and out[0] == out[1]
    assert rio.read_rgb_u8(tmp_path / "p0" / "aoi_3857.tif")[1].nodata is None
    # ... and they are the tiles of the plain warp: opaque black over the hole
    plan = tiles.plan_warp(260, 200, geo.Placement(600000.0, 5100000.0, 2.5, 2.5), geo.CRS(32633))
    e = native.Engine(num_block=1)
    try:
        plain = keep(e.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w))
    finally:
        e.close()
    assert np.array_equal(rio.read_rgb_u8(tmp_path / "p0" / "aoi_3857.tif")[0], plain[..., :3])


def test_http_wow_job_with_transparent_tiles(monkeypatch, tmp_path):
    """POST /api/wow with nodata + transparent_tiles (the pattern of tests/test_gpu_tiles.py::test_http_wow_job_tiles_by_default): a
    64 x 64 UTM GeoTIFF whose north-west corner was never measured; the tiler's own 1-block engine cuts z10..18"""
    from fastapi.testclient import TestClient

    from app.sr_routes import create_app
    from s2sr.weights import synthetic_state_dict
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir()
    sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(23, seed=0).items()}
    torch.save({"params_ema": sd}, tmp_path / "models" / "realesrgan_x4.pth")
    rgb = wm.scene(64, 64, seed=8)
    rgb[rgb == 0] = 1
    rgb[:32, :32] = 0
    georef = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0),
                         rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633)})
    (tmp_path / "data" / "source").mkdir(parents=True)
    rio.write_geotiff_rgb(tmp_path / "data" / "source" / "s2.tif", rgb, georef, nodata=0)
    c = TestClient(create_app(tmp_path / "data"))
    r = c.post("/api/wow", json={"auto_fetch": False, "nodata": "tag", "transparent_tiles": True})
    assert r.status_code == 200, r.text
    st = c.get(f"/api/sr/{r.json()['job_id']}").json()
    assert st["status"] == "completed", st
    tdir = tmp_path / "data" / "tiles_wow"
    meta = json.loads((tdir / "tileset.json").read_text())
    assert (meta["minzoom"], meta["maxzoom"]) == (10, 18) and st["result"]["sr_metadata"]["nodata"]["invalid_pixels"] == 32 * 32
    # the centre of the invalid corner (160 m east, 160 m south of the origin) at z18: its tile is absent or transparent there;
    # the centre of the measured south-east quarter is opaque
    sr3857 = next((tmp_path / "data" / "wow").rglob("*_3857.tif"))
    assert rio.read_rgb_u8(sr3857)[1].nodata == 0
    for (east, south), opaque in (((160.0, 160.0), False), ((480.0, 480.0), True)):
        lon, lat = geo.CRS(32633).to_lonlat(600000.0 + east, 5100000.0 - south)
        mx, my = geo.lonlat_to_mercator(float(lon), float(lat))
        tx, ty, py, px = _tile_pixel(float(mx), float(my), 18)
        q = tdir / "18" / str(tx) / f"{geo.xyz_row(ty, 18)}.png"
        alpha = int(np.asarray(Image.open(q))[py, px, 3]) if q.exists() else 0
        print(f"z18 tile {tx}/{geo.xyz_row(ty, 18)} {'exists' if q.exists() else 'absent'}: alpha {alpha} at ({py}, {px}), expected {'255' if opaque else '0'}")
        assert alpha == (255 if opaque else 0)
    for q in tdir.glob("*/*/*.png"):
        t = np.asarray(Image.open(q))
        assert not t[t[..., 3] == 0].any()


# ---- the door's rows of tests/doors.py -------------------------------------------------------------------------------------------------------
MASKED_WARP = doors.owned("warp_bilinear_masked_u8")


@pytest.mark.parametrize("ident", MASKED_WARP)
def test_the_door_table_s_baseline_is_the_model(ident):
    """the red-zone, poison, stall and grid-cap matrices hold every mode to diag.baseline, and this holds the baseline's raster to the
    model, sample for sample (the base level behind it is the pyramid modules' to judge)"""
    diag.same_values(diag.baseline(ident), doors.MODELS[ident](), ident)


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("ident", MASKED_WARP)
def test_door_under_the_grid_cap(ident, cap):
    """the raster has some 32 k pixels: 128 blocks of 256 threads on 1 and on 3 workgroups, a ragged last trip"""
    name, fn = doors.DOORS[ident]
    want = diag.baseline(ident)
    with diag.engines_under(native.grid_cap_workgroups, native.grid_cap, cap) as capped:
        e = capped(name)
        with diag.under(cap):
            got = keep(fn(e, Inputs()))
            st = native.grid_cap_stats()
    print(f"{ident}, cap {cap}: tiles {st['tiles']}")
    assert st["tiles"][0] >= 1 and st["tiles"][1] >= 3, st
    same(got, want, f"{ident}, cap {cap}")
