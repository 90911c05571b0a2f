"""The nodata-transparent tile pyramid without a GPU: the numpy model of the masked warp (tests/warp_masked_model.py)
tied to the pinned plain warp and to hand-computed bytes, its two promises (an invalid pixel's value never reaches the output;
colour is 0 wherever alpha is 0), the ABI, and the refusals of the binding, the tiler and the route, all of which are raised
before a device is touched.  The kernel against this model: tests/test_gpu_tiles_nodata.py."""
import re
from pathlib import Path

import numpy as np
import pytest

import warp_masked_model as wm
from oracle import tiles_ref as ref
from s2sr import native
from s2sr import rasterio_lite as rio
from tiff_fixture import write_tiff

REPO = Path(__file__).resolve().parent.parent

UTM = [(33550, 12, (2.5, 2.5, 0.0)), (33922, 12, (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0)),
       (34735, 3, (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633))]


@pytest.mark.parametrize("epsg,origin", wm.SCENES)
def test_all_valid_mask_is_the_pinned_plain_warp(epsg, origin):
    rgb = wm.scene(150, 211, seed=epsg)
    plan = wm.plan_for(epsg, origin)
    want = ref.warp_bilinear(rgb, plan.grid, plan.step, plan.out_h, plan.out_w)
    for vs in (1, 4):
        ones = np.ones((-(-150 // vs), -(-211 // vs)), np.uint8)
        got = wm.warp_bilinear_masked(rgb, ones, vs, plan.grid, plan.step, plan.out_h, plan.out_w)
        assert np.array_equal(got, want), (vs, int((got != want).sum()))


# one output pixel that samples the 2 x 2 source at (u, v) = (fx, fy): a single grid node
SRC = np.array([[[100, 0, 7], [200, 255, 9]], [[40, 255, 250], [255, 255, 255]]], np.uint8)      # p00 p10 / p01 p11
E = 2.0 ** -24                                                                                    # the spacing of float32 in [0.5, 1)
HAND = [
    # fx, fy, mask [[k00, k10], [k01, k11]], expected RGBA
    # fy = 0, p10 invalid: ws = 1 - fx
    (0.5 + E, 0.0, [[1, 0], [1, 1]], (0, 0, 0, 0)),                  # ws = 0.5 - 2^-24: just below
    (0.5, 0.0, [[1, 0], [1, 1]], (100, 0, 7, 255)),                  # ws = 0.5 exactly: kept, the colour of the one tap with weight
    (0.5 - E, 0.0, [[1, 0], [1, 1]], (100, 0, 7, 255)),              # ws = 0.5 + 2^-24: just above
    # fx = fy = 0.25: w00 .5625, w10 .1875, w01 .1875, w11 .0625
    (0.25, 0.25, [[1, 1], [1, 0]], (108, 102, 56, 255)),             # ws .9375: (56.25 + 37.5 + 7.5) / .9375 = 108, 95.625 / .9375 = 102, 52.5 / .9375 = 56
    (0.25, 0.25, [[1, 0], [1, 0]], (85, 64, 68, 255)),               # ws .75: 63.75 / .75 = 85, 47.8125 / .75 = 63.75 -> 64, 50.8125 / .75 = 67.75 -> 68
    (0.25, 0.25, [[1, 0], [0, 0]], (100, 0, 7, 255)),                # ws .5625: p00 alone
    (0.25, 0.25, [[0, 1], [1, 1]], (0, 0, 0, 0)),                    # ws .4375
    (0.25, 0.25, [[0, 1], [0, 0]], (0, 0, 0, 0)),                    # ws .1875
    (0.25, 0.25, [[0, 0], [0, 0]], (0, 0, 0, 0)),                    # no tap valid
    (0.25, 0.25, [[1, 1], [1, 1]], (117, 112, 68, 255)),             # all valid: the lerp chain, t = 125, 63.75, 7.5; b = 93.75, 255, 251.25 -> 117.1875, 111.5625, 68.4375
]


@pytest.mark.parametrize("fx,fy,mask,want", HAND)
def test_hand_made_pixels_around_the_threshold(fx, fy, mask, want):
    assert np.float32(fx) == fx and np.float32(fy) == fy            # the cases are float32 numbers
    grid = np.array([[[fx, fy]]], np.float32)
    got = wm.warp_bilinear_masked(SRC, np.array(mask, np.uint8), 1, grid, 4, 1, 1)
    assert tuple(got[0, 0]) == want


def _masked_cases():
    for epsg, origin in wm.SCENES[:1]:
        rgb, plan = wm.scene(150, 211, seed=epsg), wm.plan_for(epsg, origin)
        yield rgb, wm.mask_mixed(150, 211), 1, plan
        yield rgb, wm.mask_coarse(150, 211, 4), 4, plan


def test_invalid_pixel_values_never_reach_the_output_and_colour_is_zero_under_alpha_zero():
    for rgb, valid, vs, plan in _masked_cases():
        outs = [wm.warp_bilinear_masked(wm.repaint(rgb, valid, vs, how), valid, vs, plan.grid, plan.step, plan.out_h, plan.out_w)
                for how in (0, 255, "random")]
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), vs
        a = outs[0][..., 3]
        assert np.isin(a, (0, 255)).all() and not outs[0][a == 0].any()
        plain = ref.warp_bilinear(rgb, plan.grid, plan.step, plan.out_h, plan.out_w)
        assert 0.2 < (a == 0).mean() < 0.8 and (a[plain[..., 3] == 0] == 0).all()        # the mask bites, and the wedges stay empty


def test_the_symbol_is_declared_and_exported():
    header = (REPO / "include" / "s2sr.h").read_text()
    assert re.search(r"\bs2sr_warp_bilinear_masked_u8\s*\(", header)
    assert "s2sr_warp_bilinear_masked_u8" in native.EXPORTED_SYMBOLS
    assert hasattr(native.load_library(), "s2sr_warp_bilinear_masked_u8")


def test_the_binding_refuses_masks_of_the_wrong_shape():
    ok = native.warp_mask((150, 211, 3), np.ones((38, 53), np.uint8), 4)
    assert ok.shape == (38, 53) and ok.flags.c_contiguous
    assert native.warp_mask((150, 211, 3), np.ones((150, 211), np.uint8), 1).shape == (150, 211)
    for valid, vs in ((np.ones((37, 53), np.uint8), 4), (np.ones((38, 52), np.uint8), 4), (np.ones((150, 211), np.uint8), 4),
                      (np.ones((38, 53, 1), np.uint8), 4), (np.ones((38, 53), bool), 4), (np.ones((38, 53), np.float32), 4)):
        with pytest.raises(ValueError, match="valid: expected uint8"):
            native.warp_mask((150, 211, 3), valid, vs)
    for vs in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="valid_scale"):
            native.warp_mask((150, 211, 3), np.ones((150, 211), np.uint8), vs)
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        native.warp_mask((150, 211, 4), np.ones((150, 211), np.uint8), 1)


def test_the_tiler_refuses_before_it_touches_a_device(tmp_path):
    import app.tiling as tiling
    rgb = wm.scene(40, 52, seed=1)
    plain, tagged = tmp_path / "plain.tif", tmp_path / "tagged.tif"
    write_tiff(plain, rgb, extra=UTM)
    write_tiff(tagged, rgb, extra=UTM + [(42113, 2, "0")])
    merc = UTM[:1] + [(33922, 12, (0.0, 0.0, 0.0, 1500000.0, 6000000.0, 0.0)), (34735, 3, UTM[2][2][:-1] + (3857,))]
    plain_m, tagged_m = tmp_path / "plain_m.tif", tmp_path / "tagged_m.tif"          # generate_xyz_tiles takes EPSG:3857 rasters
    write_tiff(plain_m, rgb, extra=merc)
    write_tiff(tagged_m, rgb, extra=merc + [(42113, 2, "0")])
    for fn, src in ((tiling.process_raster_to_tiles, plain), (tiling.generate_xyz_tiles, plain_m), (tiling.reproject_to_web_mercator, plain)):
        with pytest.raises(ValueError, match="no GDAL_NODATA tag"):
            fn(src, tmp_path / "out", nodata="tag")
        for bad in (1.5, True, "auto"):
            with pytest.raises(ValueError, match="nodata"):
                fn(src, tmp_path / "out", nodata=bad)
    for fn, src in ((tiling.process_raster_to_tiles, tagged), (tiling.generate_xyz_tiles, tagged_m)):
        with pytest.raises(ValueError, match="valid: expected uint8"):
            fn(src, tmp_path / "out", valid=np.ones((10, 14), np.uint8), valid_scale=4)            # ceil(40 / 4) x ceil(52 / 4) = 10 x 13
        with pytest.raises(ValueError, match="valid: expected uint8"):
            fn(src, tmp_path / "out", nodata="tag", valid=np.ones((40, 52), np.uint8), valid_scale=2)
        with pytest.raises(ValueError, match="valid_scale"):
            fn(src, tmp_path / "out", valid=np.ones((40, 52), np.uint8), valid_scale=0)
    assert not (tmp_path / "out").exists() and not (tmp_path / "plain_3857.tif").exists()
    # what the refusals guard: the mask of a tagged file, from the raster as read
    arr, tags, _, _ = tiling._read(tagged)
    rgb0 = rgb.copy()
    rgb0[:5, :7] = 0
    assert tiling._mask_of(rgb0, tags, tagged, "tag", None, 1)[0][:5, :7].sum() == 0
    own = np.zeros((10, 13), np.uint8)
    mask, vs, value = tiling._mask_of(arr, tags, tagged, "tag", own, 4)
    assert mask is not None and not mask.any() and (vs, value) == (4, 0)                          # the caller's mask wins
    assert [tiling._u8_nodata(v) for v in (None, 0, 255, 256, 65535, -1)] == [None, 0, 255, 0, 0, 0]


def test_the_route_refuses_transparent_tiles_without_nodata(tmp_path):
    from fastapi.testclient import TestClient

    from app.sr_routes import create_app
    c = TestClient(create_app(tmp_path / "data"))
    f = tmp_path / "a.tif"
    f.write_bytes(b"II*\x00")
    r = c.post("/api/wow", json={"input_file": str(f), "transparent_tiles": True})
    assert r.status_code == 400 and "nodata" in r.json()["detail"]
    assert c.post("/api/wow", json={"input_file": str(f), "transparent_tiles": True, "nodata": 1.5}).status_code in (400, 422)
    assert c.get("/api/sr").json() == {"jobs": {}}


def test_esrgan_tiles_hands_the_inputs_mask_to_the_tiler(tmp_path, monkeypatch):
    """run_esrgan_and_tiles(nodata=): the SR step is a nodata job, the tiler gets the input's mask at the SR scale and the SR file's
    tag; with skip_sr the value as given; without the keyword both calls are what they were (the two steps replaced by recorders)"""
    import app.esrgan_tiles as et
    rgb = wm.scene(24, 32, seed=3)
    rgb[rgb == 0] = 1
    rgb[:6, :9] = 0
    write_tiff(tmp_path / "in.tif", rgb, extra=UTM + [(42113, 2, "0")])
    calls = {}

    def sr(**kw):
        calls["sr"] = kw
        return kw["output_path"], {"scale": 4}

    def tiler(*a, **kw):
        calls["tiles"] = kw
        return {}
    monkeypatch.setattr(et, "apply_wow_sr", sr)
    monkeypatch.setattr(et, "process_raster_to_tiles", tiler)
    monkeypatch.setattr(et, "get_raster_info", lambda p: type("I", (), {"width": 1, "height": 1, "crs": "x"})())
    assert et.run_esrgan_and_tiles(tmp_path / "in.tif", tmp_path / "o", nodata="tag")["status"] == "completed"
    assert calls["sr"]["nodata"] == "tag"
    kw = calls["tiles"]
    assert kw["nodata"] == "tag" and kw["valid_scale"] == 4 and kw["valid"].shape == (24, 32) and kw["valid"][:6, :9].sum() == 0 and kw["valid"].sum() == 24 * 32 - 54
    et.run_esrgan_and_tiles(tmp_path / "in.tif", tmp_path / "o", skip_sr=True, sr_output=tmp_path / "in.tif", nodata=0)
    assert calls["tiles"]["nodata"] == 0 and "valid" not in calls["tiles"]
    et.run_esrgan_and_tiles(tmp_path / "in.tif", tmp_path / "o")
    assert "nodata" not in calls["sr"] and not {"nodata", "valid", "valid_scale"} & set(calls["tiles"])
    with pytest.raises(ValueError, match="nodata"):
        et.run_esrgan_and_tiles(tmp_path / "in.tif", tmp_path / "o", nodata=1.5)


def test_the_jobs_mask_has_one_definition(tmp_path):
    """app.wow_sr.input_mask is the mask the job itself enhances with: the raster as stored, 8 and 16 bits"""
    from app.wow_sr import input_mask, read_masked
    rgb = wm.scene(24, 32, seed=3)
    rgb[rgb == 0] = 1
    rgb[:6, :9] = 0
    write_tiff(tmp_path / "u8.tif", rgb, extra=UTM + [(42113, 2, "0")])
    want = np.ones((24, 32), np.uint8)
    want[:6, :9] = 0
    assert np.array_equal(input_mask(tmp_path / "u8.tif", "tag"), want) and np.array_equal(input_mask(tmp_path / "u8.tif", 0, 8), want)
    img16 = rgb.astype(np.uint16) * 40
    write_tiff(tmp_path / "u16.tif", img16, extra=UTM)
    img, georef, valid, value = read_masked(tmp_path / "u16.tif", 0, 16)
    assert np.array_equal(img, img16) and np.array_equal(valid, want) and value == 0 and georef is not None
    assert read_masked(tmp_path / "u16.tif", None, 16)[2:] == (None, None)
    with pytest.raises(ValueError, match="no GDAL_NODATA tag"):
        input_mask(tmp_path / "u16.tif", "tag", 16)
    with pytest.raises(ValueError, match="uint16"):
        input_mask(tmp_path / "u8.tif", 0, 16)
    assert rio.TAG_GDAL_NODATA == 42113
