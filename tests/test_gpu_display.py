"""The display rendering of 16-bit images on the GPU (include/s2sr.h: s2sr_display_hist_u16, s2sr_display_apply_u16)
byte for byte against the from-scratch model of tests/display_model.py, the device-copy protocol behind the 16-bit enhance doors,
and the app seam (process_wow_sr(bit_depth=16, display=...), process_raster_to_tiles(stretch=...), /api/wow)."""
import functools
import json

import numpy as np
import pytest
import torch
from PIL import Image

import display_model as M
import gpu_engines
from s2sr import display as D
from s2sr import native
from s2sr import rasterio_lite as rio
from s2sr import tiff_lite
from s2sr.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

HP = native.PREC_F16_HP
MERCATOR = (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 3857)
UTM33 = (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633)


@pytest.fixture(scope="module")
def eng():
    e = native.Engine(num_block=1)       # neither entry needs weights
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def random_lut():
    t = np.random.default_rng(99).integers(0, 256, size=(3, 65536), dtype=np.uint8)
    t.setflags(write=False)
    return t


def contents(H, W):
    """name -> (image, nodata)"""
    rng = np.random.default_rng(H * 1000 + W)
    two = np.where(rng.random((H, W, 3)) < 0.4, 777, 50000).astype(np.uint16)
    return {"random": (rng.integers(0, 65536, size=(H, W, 3)).astype(np.uint16), -1),
            "zeros": (np.zeros((H, W, 3), np.uint16), -1),
            "top": (np.full((H, W, 3), 65535, np.uint16), -1),
            "two, nodata one of them": (two, 777),
            "random, nodata 0": (rng.integers(0, 4, size=(H, W, 3)).astype(np.uint16), 0)}


def check(eng, img, nodata, band_rows, what):
    want_h = M.hist(img, None if nodata < 0 else nodata)
    got_h = eng.display_hist_u16(img, nodata=nodata, band_rows=band_rows)
    assert got_h.dtype == np.uint64 and got_h.shape == (3, 65536)
    assert np.array_equal(got_h, want_h), (what, "hist", int(np.abs(got_h.astype(np.int64) - want_h.astype(np.int64)).sum()))
    want = M.apply(img, random_lut())
    got = eng.display_apply_u16(img, random_lut(), band_rows=band_rows)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (what, "apply from the host image")
    got = eng.display_apply_u16(None, random_lut(), band_rows=band_rows, shape=img.shape[:2])
    assert np.array_equal(got, want), (what, "apply from the device copy")


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (3, 7), (37, 53), (64, 64), (255, 257)])
def test_hist_and_apply_byte_for_byte(eng, H, W):
    """Band edges inside, at and beyond the image; 37 x 53 and 255 x 257: odd row lengths, no band starts on a 16-byte boundary."""
    for name, (img, nodata) in contents(H, W).items():
        for band_rows in sorted({0, 1, 7, H}):
            check(eng, img, nodata, band_rows, f"{H}x{W} {name}, band_rows {band_rows}")


def test_every_value_once_per_channel(eng):
    rng = np.random.default_rng(5)
    img = np.stack([rng.permutation(65536) for _ in range(3)], axis=-1).reshape(256, 256, 3).astype(np.uint16)
    for band_rows in (0, 100):
        h = eng.display_hist_u16(img, band_rows=band_rows)
        assert (h == 1).all()
        h = eng.display_hist_u16(img, nodata=4242, band_rows=band_rows)
        assert h.sum() == 3 * 65535 and (h[:, 4242] == 0).all()
        assert np.array_equal(eng.display_apply_u16(img, random_lut(), band_rows=band_rows), M.apply(img, random_lut()))


def test_a_million_samples_in_one_bin(eng):
    """1024 x 1024 of (1234, 1234, 1234): 2^20 samples per bin (a narrow counter wraps) and the worst case for contention."""
    img = np.full((1024, 1024, 3), 1234, np.uint16)
    for band_rows in (0, 300):
        h = eng.display_hist_u16(img, band_rows=band_rows)
        assert (h[:, 1234] == 1 << 20).all() and h.sum() == 3 << 20
    img2 = img.copy()
    img2[..., 1] = 40000                                        # three bins in three value ranges
    h = eng.display_hist_u16(img2)
    assert h[0, 1234] == h[1, 40000] == h[2, 1234] == 1 << 20 and h.sum() == 3 << 20
    out = eng.display_apply_u16(None, random_lut(), shape=(1024, 1024))
    assert np.array_equal(out, np.broadcast_to(np.array([random_lut()[0, 1234], random_lut()[1, 40000], random_lut()[2, 1234]], np.uint8), out.shape))


def test_render_equals_the_model(eng):
    rng = np.random.default_rng(17)
    img = rng.integers(900, 3200, size=(77, 91, 3)).astype(np.uint16)
    img[rng.random((77, 91)) < 0.1] = 0
    img[3, 4] = 65535                                           # the glint that sets a global max
    for kw in ({}, {"linked": False, "nodata": 0}, {"p_lo": 0, "p_hi": 100}, {"gamma": 2.2, "p_lo": 0.01, "p_hi": 99.99, "nodata": 0}):
        out, info = D.render_u16(img, kw, eng)
        lims = M.limits(img, kw.get("p_lo", 2.0), kw.get("p_hi", 98.0), kw.get("linked", True), kw.get("nodata"))
        assert info["limits"] == lims
        assert np.array_equal(out, M.apply(img, D.build_lut(lims, kw.get("gamma", 1.0))))
        if "gamma" not in kw:
            assert np.array_equal(out, M.render(img, **kw)[0])


def test_refusals(eng):
    img = np.zeros((4, 4, 3), np.uint16)
    hist = np.zeros((3, 65536), np.uint64)
    for nodata in (-2, 65536):
        with pytest.raises(native.S2srError, match="nodata"):
            eng.display_hist_u16(img, nodata=nodata)
    with pytest.raises(native.S2srError, match="band_rows"):
        eng.display_hist_u16(img, band_rows=-1)
    lib, h = eng._lib, eng._h
    assert lib.s2sr_display_hist_u16(h, native._ptr(img), 4, 4, -1, 0, None) == -1
    assert lib.s2sr_display_hist_u16(h, native._ptr(img), 0, 4, -1, 0, native._ptr(hist)) == -1
    assert lib.s2sr_display_apply_u16(h, native._ptr(img), 4, 4, None, 0, native._ptr(hist)) == -1
    assert lib.s2sr_display_apply_u16(h, native._ptr(img), 4, 4, native._ptr(hist), 0, None) == -1
    assert lib.s2sr_display_apply_u16(h, native._ptr(img), 4, -4, native._ptr(hist), 0, native._ptr(hist)) == -1
    assert lib.s2sr_display_hist_u16(None, native._ptr(img), 4, 4, -1, 0, native._ptr(hist)) == -1
    with pytest.raises(TypeError):
        eng.display_hist_u16(img.astype(np.uint8))
    assert eng.display_hist_u16(img)[:, 0].tolist() == [16, 16, 16]          # the handle still works


# ---- the device copy behind the 16-bit enhance doors --------------------------------------------------------------------------
@pytest.mark.parametrize("door", ["enhance_u16", "enhance_blend_u16"])
def test_device_copy_after_the_16_bit_doors(door):
    e = gpu_engines.default(1, HP)
    img = np.random.default_rng(3).integers(0, 65536, size=(40, 56, 3)).astype(np.uint16)
    run = getattr(e, door)
    out = run(img, tile=16, pad=3)                              # tiled: 40 x 56 > 4 x 16 x 16
    assert out.shape == (160, 224, 3)
    first = out.copy()
    for band_rows in (0, 33):
        assert np.array_equal(e.display_hist_u16(None, band_rows=band_rows, shape=(160, 224)), M.hist(out))
        assert np.array_equal(e.display_hist_u16(None, nodata=int(out[0, 0, 0]), shape=(160, 224)), M.hist(out, int(out[0, 0, 0])))
        assert np.array_equal(e.display_apply_u16(None, random_lut(), band_rows=band_rows, shape=(160, 224)), M.apply(out, random_lut()))
    assert np.array_equal(e.display_hist_u16(None, shape=(160, 224)), M.hist(out))        # still there behind an apply
    # the door's own bytes do not depend on a display call behind it
    assert np.array_equal(run(img, tile=16, pad=3), first)
    # a wrong size
    for shape in [(224, 160), (160, 223), (40, 56)]:
        with pytest.raises(native.S2srError, match="did not leave"):
            e.display_hist_u16(None, shape=shape)
        with pytest.raises(native.S2srError, match="did not leave"):
            e.display_apply_u16(None, random_lut(), shape=shape)
    assert np.array_equal(e.display_hist_u16(None, shape=(160, 224)), M.hist(out))        # a refusal leaves the copy alone
    # another call in between
    grid = np.zeros((2, 2, 2), np.float32)
    e.warp_bilinear_u8(np.zeros((4, 4, 3), np.uint8), grid, 4, 4, 4)
    with pytest.raises(native.S2srError, match="did not leave"):
        e.display_hist_u16(None, shape=(160, 224))
    with pytest.raises(native.S2srError, match="did not leave"):
        e.display_apply_u16(None, random_lut(), shape=(160, 224))
    # ... an 8-bit door as well
    run(img, tile=16, pad=3)
    e.enhance_u8((img >> 8).astype(np.uint8), tile=16, pad=3)
    with pytest.raises(native.S2srError, match="did not leave"):
        e.display_hist_u16(None, shape=(160, 224))


def test_a_fresh_handle_holds_no_image():
    e = native.Engine(num_block=1)
    try:
        with pytest.raises(native.S2srError, match="did not leave"):
            e.display_hist_u16(None, shape=(4, 4))
        with pytest.raises(native.S2srError, match="did not leave"):
            e.display_apply_u16(None, random_lut(), shape=(4, 4))
    finally:
        e.close()


# ---- the app seam --------------------------------------------------------------------------------------------------------------
def _patch_weights(monkeypatch, tmp_path, nb_by_name):
    """Seeded synthetic checkpoints where the drop-in looks for them (tests/test_gpu_app.py)."""
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir(exist_ok=True)
    for name, nb in nb_by_name.items():
        sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(nb, seed=0).items()}
        torch.save({"params_ema": sd}, tmp_path / "models" / f"{name}.pth")


def _png(path):
    return np.asarray(Image.open(path).convert("RGB"))


def test_wow_job_with_display(monkeypatch, tmp_path):
    import app.cnn_super_resolution as m
    from app.wow_sr import _pp_engine, process_wow_sr
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    rng = np.random.default_rng(45)
    rgb = rng.integers(100, 4000, size=(40, 56, 3)).astype(np.uint16)
    rgb[..., 2] //= 2                                           # the bands differ: a swapped channel order shows
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)})
    src = tmp_path / "scene16.tif"
    rio.write_geotiff_rgb16(src, rgb, geo)

    plain = process_wow_sr(src, tmp_path / "plain", enhance_crops=False, model="realesrgan_anime", bit_depth=16)
    assert plain["outputs"]["sr_png"] is None and "display" not in plain["sr_metadata"] and plain["sr_metadata"]["enhancements"] == []
    tif_plain = open(plain["outputs"]["sr_tif"], "rb").read()

    for k, disp in enumerate([{"p_lo": 2, "p_hi": 98}, {"linked": False, "p_lo": 1, "p_hi": 99.5, "nodata": int(rgb[0, 0, 0])},
                              {"limits": [[200, 3000], [300, 3500], [50, 1500]], "gamma": 2.2}]):
        res = process_wow_sr(src, tmp_path / f"d{k}", enhance_crops=False, model="realesrgan_anime", bit_depth=16, display=disp)
        assert open(res["outputs"]["sr_tif"], "rb").read() == tif_plain                 # the GeoTIFF stays raw
        arr, _ = tiff_lite.read_tiff(res["outputs"]["sr_tif"])
        meta = res["sr_metadata"]
        st = D.Stretch.of(disp)
        lims = st.limits or M.limits(arr, float(st.p_lo), float(st.p_hi), st.linked, st.nodata)
        assert meta["display"] == st.info(lims) and meta["enhancements"] == [] and meta["bit_depth"] == 16
        assert json.load(open(tmp_path / f"d{k}" / "scene16_wow_sr_metadata.json"))["sr_metadata"] == meta
        assert res["outputs"]["sr_png"] == str(tmp_path / f"d{k}" / "scene16_wow_sr.png")
        assert np.array_equal(_png(res["outputs"]["sr_png"]), M.apply(arr, D.build_lut(lims, st.gamma)))
        if st.gamma == 1.0:
            assert np.array_equal(_png(res["outputs"]["sr_png"]), M.apply(arr, M.lut(lims)))

    # the crop-visibility post-process runs on the display image
    res = process_wow_sr(src, tmp_path / "crops", enhance_crops=True, model="realesrgan_anime", bit_depth=16, display={"p_lo": 2, "p_hi": 98})
    assert open(res["outputs"]["sr_tif"], "rb").read() == tif_plain
    arr, _ = tiff_lite.read_tiff(res["outputs"]["sr_tif"])
    shown, lims = M.render(arr)
    assert res["sr_metadata"]["display"]["limits"] == lims
    assert res["sr_metadata"]["enhancements"] == ["CLAHE local contrast", "Unsharp mask", "Vegetation boost"]
    assert np.array_equal(_png(res["outputs"]["sr_png"]), _pp_engine().postprocess_u8(np.ascontiguousarray(shown), native.pp_wow()))

    # RealESRGAN.enhance16(display=...): the same 16-bit image, plus its rendering in the channel order given
    e = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)
    out16 = e.enhance16(rgb)
    got16, disp8, info = e.enhance16(rgb, display=D.Stretch(linked=False))
    assert np.array_equal(got16, out16)
    want8, lims = M.render(out16, linked=False)
    assert np.array_equal(disp8, want8) and info["limits"] == lims


def _tree(d):
    return {str(p.relative_to(d)): p.read_bytes() for p in sorted(d.rglob("*.png"))}


def test_tiling_a_uint16_raster_with_a_stretch(tmp_path):
    import app.tiling as tiling
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:96, 0:128]
    img = np.stack([1500 + 9 * xx + 5 * yy, 1200 + 7 * xx, 900 + 11 * yy], axis=-1) + rng.integers(0, 200, size=(96, 128, 3))
    img = img.astype(np.uint16)
    img[5, 5] = 65535                                           # a glint: the global min-max would darken everything
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (2.5, 2.5, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 1.5e6, 6.0e6, 0.0), rio.TAG_GEOKEYS: MERCATOR})
    src16 = tmp_path / "a" / "raster.tif"
    src16.parent.mkdir()
    rio.write_geotiff_rgb16(src16, img, geo)
    stretch = {"p_lo": 1, "p_hi": 99, "linked": False}
    shown, lims = M.render(img, 1, 99, False)
    src8 = tmp_path / "b" / "raster.tif"
    src8.parent.mkdir()
    rio.write_geotiff_rgb(src8, np.ascontiguousarray(shown), geo)
    tiling.process_raster_to_tiles(src8, tmp_path / "t8", min_zoom=14, max_zoom=17)
    want = _tree(tmp_path / "t8")
    assert want
    tiling.process_raster_to_tiles(src16, tmp_path / "t16", min_zoom=14, max_zoom=17, stretch=stretch)
    assert _tree(tmp_path / "t16") == want
    tiling.process_raster_to_tiles(src16, tmp_path / "t16l", min_zoom=14, max_zoom=17, stretch={"limits": lims})
    assert _tree(tmp_path / "t16l") == want
    tiling.process_raster_to_tiles(src16, tmp_path / "t16m", min_zoom=14, max_zoom=17)          # without: the global min-max, as ever
    assert _tree(tmp_path / "t16m") != want
    tiling.process_raster_to_tiles(src8, tmp_path / "t8s", min_zoom=14, max_zoom=17, stretch=stretch)   # ignored on a uint8 raster
    assert _tree(tmp_path / "t8s") == want
    # the warp door: a UTM raster, stretched, onto the EPSG:3857 grid
    utm = rio.GeoRef({rio.TAG_PIXEL_SCALE: (2.5, 2.5, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0), rio.TAG_GEOKEYS: UTM33})
    rio.write_geotiff_rgb16(tmp_path / "u16.tif", img, utm)
    rio.write_geotiff_rgb(tmp_path / "u8.tif", np.ascontiguousarray(shown), utm)
    tiling.reproject_to_web_mercator(tmp_path / "u16.tif", tmp_path / "w16.tif", stretch=stretch)
    tiling.reproject_to_web_mercator(tmp_path / "u8.tif", tmp_path / "w8.tif")
    assert np.array_equal(tiff_lite.read_tiff(tmp_path / "w16.tif")[0], tiff_lite.read_tiff(tmp_path / "w8.tif")[0])


def test_http_wow_16_bit_job_shows_one_rendering(monkeypatch, tmp_path):
    """POST /api/wow with bit_depth 16 and display: uint16 GeoTIFF + PNG + pyramid, the PNG and the tiles from one rendering."""
    import app.tiling as tiling
    from fastapi.testclient import TestClient

    from app.sr_routes import create_app
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_x4": 23})
    rng = np.random.default_rng(9)
    rgb = rng.integers(300, 5000, size=(24, 32, 3)).astype(np.uint16)
    georef = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0), rio.TAG_GEOKEYS: UTM33})
    (tmp_path / "data" / "source").mkdir(parents=True)
    rio.write_geotiff_rgb16(tmp_path / "data" / "source" / "s2.tif", rgb, georef)
    c = TestClient(create_app(tmp_path / "data", tile_min_zoom=14, tile_max_zoom=15))
    assert c.post("/api/wow", json={"auto_fetch": False, "display": {"p_lo": 2, "p_hi": 98}}).status_code == 400      # an 8-bit job
    assert c.post("/api/wow", json={"auto_fetch": False, "bit_depth": 16, "display": {"p_lo": 2.005}}).status_code == 400
    r = c.post("/api/wow", json={"auto_fetch": False, "enhance_crops": False, "bit_depth": 16, "display": {"p_lo": 1, "p_hi": 99, "linked": False}})
    st = c.get(f"/api/sr/{r.json()['job_id']}").json()
    assert st["status"] == "completed", st
    out = st["result"]["outputs"]
    arr, tags = tiff_lite.read_tiff(out["sr_tif"])
    assert arr.dtype == np.uint16 and arr.shape == (96, 128, 3)
    shown, lims = M.render(arr, 1, 99, False)
    assert st["result"]["sr_metadata"]["display"]["limits"] == lims
    assert np.array_equal(_png(out["sr_png"]), shown)
    # the pyramid: that of the PNG's pixels at the GeoTIFF's place
    rio.write_geotiff_rgb(tmp_path / "shown.tif", np.ascontiguousarray(shown), georef.scaled(4))
    tiling.process_raster_to_tiles(tmp_path / "shown.tif", tmp_path / "want", min_zoom=14, max_zoom=17)
    want = _tree(tmp_path / "want")
    assert want and _tree(tmp_path / "data" / "tiles_wow") == want
