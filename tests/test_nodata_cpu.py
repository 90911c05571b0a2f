"""The nodata-aware enhance off the GPU: the model's two forms of the fill against each other, the GDAL_NODATA tag
through the GeoTIFF reader and writers, the RGBA PNG, the Python helpers and the argument refusals of the job functions."""
import hashlib
import io

import numpy as np
import pytest
from PIL import Image

import nodata_model as nm
from s2sr import nodata as nd
from s2sr import rasterio_lite as rio
from s2sr import tiff_lite


# ---- the model: the definition (brute force) and the separable form the kernel uses agree on the SOURCE pixel everywhere -------------
def both(valid, R):
    a, b = nm.sources_brute(valid, R), nm.sources_separable(valid, R)
    assert np.array_equal(a, b), np.argwhere((a != b).any(axis=2))[:5]
    return a


@pytest.mark.parametrize("R", [1, 3, 8, 12])
@pytest.mark.parametrize("H,W", [(13, 17), (21, 19), (25, 25)])
def test_model_forms_agree_on_random_masks(H, W, R):
    rng = np.random.default_rng(100 * H + W + R)
    filled = 0
    for density in (0.02, 0.3, 0.8):
        valid = rng.random((H, W)) < density
        src = both(valid, R)
        own = np.stack(np.meshgrid(np.arange(H), np.arange(W), indexing="ij"), axis=-1)
        moved = (src != own).any(axis=2)
        assert not moved[valid].any()                                     # a valid pixel is its own source
        assert valid[src[..., 0], src[..., 1]][moved].all()               # a moved pixel's source is valid ...
        d2 = ((src - own) ** 2).sum(axis=2)
        assert (d2[moved] <= R * R).all()                                 # ... and within the radius
        filled += int(moved.sum())
    assert filled > 0


def test_model_degenerate_masks():
    H, W = 13, 17
    own = np.stack(np.meshgrid(np.arange(H), np.arange(W), indexing="ij"), axis=-1)
    for R in (1, 8, 12):
        assert np.array_equal(both(np.ones((H, W), bool), R), own)        # all valid: the identity
        assert np.array_equal(both(np.zeros((H, W), bool), R), own)       # all invalid: nothing to take, the identity
        one = np.zeros((H, W), bool)
        one[5, 9] = True
        src = both(one, R)
        yy, xx = np.ogrid[:H, :W]
        near = (yy - 5) ** 2 + (xx - 9) ** 2 <= R * R
        assert (src[near] == (5, 9)).all() and np.array_equal(src[~near], own[~near])
    img = np.arange(H * W * 3, dtype=np.uint16).reshape(H, W, 3)
    assert np.array_equal(nm.fill(img, one, 3), nm.fill(img, one, 3, nm.sources_brute))
    assert (nm.fill(img, one, 3)[5, 7] == img[5, 9]).all() and (nm.fill(img, one, 3)[0, 0] == img[0, 0]).all()


def test_model_four_way_tie_takes_the_upper_pixel():
    valid = np.zeros((9, 9), bool)
    valid[2, 4] = valid[6, 4] = valid[4, 2] = valid[4, 6] = True          # four pixels at distance 2 of the centre
    src = both(valid, 3)
    assert tuple(src[4, 4]) == (2, 4)                                     # (d2, qy, qx): the smallest qy
    valid[2, 4] = False
    assert tuple(both(valid, 3)[4, 4]) == (4, 2)                          # then, at equal qy, the smallest qx
    diag = np.zeros((9, 9), bool)
    diag[3, 3] = diag[3, 5] = diag[5, 3] = diag[5, 5] = True
    assert tuple(both(diag, 3)[4, 4]) == (3, 3)


def test_model_mask():
    valid = np.array([[1, 0], [0, 1], [1, 1]], np.uint8)
    out = np.full((6, 4, 3), 9, np.uint8)
    got = nm.mask(out, valid, 2, 0)
    up = nm.upsample(valid, 2)
    assert up.shape == (6, 4) and up[0, 0] and not up[0, 2] and not up[3, 1] and up[3, 2]
    assert (got[up] == 9).all() and (got[~up] == 0).all() and (out == 9).all()


# ---- GeoTIFF: the tag round-trips; a file written without nodata= is what it always was ------------------------------------------------
def _img(dtype):
    rng = np.random.default_rng(42)
    a = rng.integers(0, 256 if dtype == np.uint8 else 12000, size=(150, 97, 3)).astype(dtype)
    a[:40, :30] = 0
    return a


GEOREF = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 500000.0, 4200000.0, 0.0),
                     rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633), rio.TAG_GEOASCII: "WGS 84 / UTM zone 33N|"})
# sha256 of the files the writers made of _img / GEOREF before they knew the tag (recorded from the commit before this feature)
BEFORE = {"u8.tif": "781056c0c5d072dc55b2e8e5cc2adc3dcd0a67f37504bdd92f498affd368d082",
          "u16.tif": "5271db3f2885a28e0aaa1ff544bcc5f4895a9984b46380272913286539e8a203",
          "rgb.png": "9fc6247c0d07dd69a26001ff30f673ccd5d28b977fa8eb0bb72e472d66444fc2"}


def _sha(path):
    return hashlib.sha256(path.read_bytes()).hexdigest()


def test_files_written_without_nodata_are_byte_identical_to_before(tmp_path):
    rio.write_geotiff_rgb(tmp_path / "u8.tif", _img(np.uint8), GEOREF)
    rio.write_geotiff_rgb16(tmp_path / "u16.tif", _img(np.uint16), GEOREF)
    rio.write_png(tmp_path / "rgb.png", _img(np.uint8))
    for name, want in BEFORE.items():
        assert _sha(tmp_path / name) == want, name
    rio.write_outputs(_img(np.uint8), tmp_path / "o.png", tmp_path / "o.tif", GEOREF)
    assert _sha(tmp_path / "o.tif") == BEFORE["u8.tif"] and _sha(tmp_path / "o.png") == BEFORE["rgb.png"]
    assert rio.read_rgb_u8(tmp_path / "u8.tif")[1].nodata is None


@pytest.mark.parametrize("dtype,value", [(np.uint8, 0), (np.uint8, 255), (np.uint16, 0), (np.uint16, 65535)])
def test_nodata_tag_round_trips(tmp_path, dtype, value):
    img = _img(dtype)
    path = tmp_path / "n.tif"
    (rio.write_geotiff_rgb if dtype == np.uint8 else rio.write_geotiff_rgb16)(path, img, GEOREF, nodata=value)
    arr, tags = tiff_lite.read_tiff(path)
    assert np.array_equal(arr, img)
    assert tags[tiff_lite.GDAL_NODATA] == (str(value),) and tiff_lite.parse_nodata(tags[tiff_lite.GDAL_NODATA]) == value
    raw, georef = rio.read_rgb_raw(path)
    assert georef.nodata == value and georef.scaled(4).nodata == value and np.array_equal(raw, img)
    assert georef.tags == rio.read_rgb_raw(path)[1].tags and rio.TAG_GEOKEYS in georef.tags      # the geo tags came along
    with Image.open(path) as im:                                          # another reader sees the tag too
        assert str(im.tag_v2[42113]).strip("\0") == str(value)
    assert rio.resolve_nodata("tag", georef) == value and rio.resolve_nodata(7, georef) == 7
    if dtype == np.uint8:
        u8, g2, valid, v = rio.read_rgb_u8_nodata(path, "tag")
        assert v == value and g2.nodata == value and np.array_equal(u8, img) and np.array_equal(valid, nd.mask_from_value(img, value))


def test_parse_nodata():
    p = tiff_lite.parse_nodata
    assert p(("0",)) == 0 and p("65535") == 65535 and p(("-9999.0",)) == -9999 and isinstance(p(("-9999.0",)), int)
    assert p(("1.5",)) == 1.5 and p(("nan",)) is None and p(None) is None and p(("n/a",)) is None and p(("inf",)) == float("inf")


def test_tag_is_required_when_asked_for(tmp_path):
    rio.write_geotiff_rgb(tmp_path / "plain.tif", _img(np.uint8), GEOREF)
    with pytest.raises(ValueError, match="GDAL_NODATA"):
        rio.read_rgb_u8_nodata(tmp_path / "plain.tif", "tag")
    img, georef, valid, value = rio.read_rgb_u8_nodata(tmp_path / "plain.tif", 0)
    assert value == 0 and int((valid == 0).sum()) >= 40 * 30


def test_the_squeeze_of_a_nodata_job_ignores_the_invalid_pixels(tmp_path):
    img = _img(np.uint16)
    img[img == 0] = 1
    img[:40, :30] = 0                                                     # the nodata corner; the data are 1 .. 11999
    img[100, 50] = (0, 5, 0)                                              # a zero band is not a nodata pixel
    rio.write_geotiff_rgb16(tmp_path / "n.tif", img, GEOREF, nodata=0)
    u8, _, valid, value = rio.read_rgb_u8_nodata(tmp_path / "n.tif", "tag")
    assert valid[100, 50] == 1 and not valid[:40, :30].any() and valid[40:].all()
    px = img[valid != 0]
    lo, hi = int(px.min()), int(px.max())
    want = ((np.clip(img, lo, hi).astype(np.float64) - lo) / (hi - lo) * 255).astype(np.uint8)
    assert np.array_equal(u8, want)


# ---- PNG: RGBA, alpha = 255 x the upsampled mask ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,band_rows,kw", [(4, 128, {}), (4, 6, {}), (2, 5, {}), (1, 7, {}), (4, 10, {"level": 6})])
def test_rgba_png_decodes_to_rgb_plus_the_upsampled_mask(scale, band_rows, kw):
    rng = np.random.default_rng(scale + band_rows)
    H, W = 23, 31
    valid = (rng.random((H, W)) > 0.3).astype(np.uint8)
    rgb = rng.integers(0, 256, size=(H * scale, W * scale, 3), dtype=np.uint8)
    data = b"".join(rio.encode_png_pieces(rgb, band_rows=band_rows, valid=valid, valid_scale=scale, **kw))
    im = Image.open(io.BytesIO(data))
    assert im.mode == "RGBA"
    a = np.asarray(im)
    assert np.array_equal(a[..., :3], rgb)
    assert np.array_equal(a[..., 3], nd.upsample_mask(valid, scale) * 255)
    assert np.array_equal(nd.upsample_mask(valid, scale) != 0, nm.upsample(valid, scale))
    with pytest.raises(ValueError):
        rio.encode_png_pieces(rgb, valid=valid[:-1], valid_scale=scale)


def test_write_outputs_of_a_nodata_job(tmp_path):
    valid = np.ones((25, 20), np.uint8)
    valid[:5, :7] = 0
    out = np.random.default_rng(3).integers(1, 256, size=(100, 80, 3), dtype=np.uint8)
    rio.write_outputs(out, tmp_path / "o.png", tmp_path / "o.tif", GEOREF.scaled(4), nodata=0, valid=valid, valid_scale=4)
    assert rio.read_rgb_raw(tmp_path / "o.tif")[1].nodata == 0
    a = np.asarray(Image.open(tmp_path / "o.png"))
    assert a.shape == (100, 80, 4) and np.array_equal(a[..., :3], out) and np.array_equal(a[..., 3] != 0, nm.upsample(valid, 4))


# ---- the helpers ------------------------------------------------------------------------------------------------------------------------
def test_mask_from_value_needs_all_three_bands():
    img = np.full((3, 4, 3), 5, np.uint16)
    img[0, 0] = 0
    img[1, 1] = (0, 0, 5)
    img[2, 3] = (7, 7, 7)
    v = nd.mask_from_value(img, 0)
    assert v.dtype == np.uint8 and v.shape == (3, 4) and v[0, 0] == 0 and v[1, 1] == 1 and v.sum() == 11
    assert nd.mask_from_value(img, 7).sum() == 11 and nd.mask_from_value(img, 7)[2, 3] == 0
    assert nd.mask_from_value(img, -9999).all() and nd.mask_from_value(img, 70000).all()
    with pytest.raises(ValueError):
        nd.mask_from_value(img[..., 0], 0)


def test_valid_range_and_its_degenerate_rules():
    img = np.zeros((4, 4, 3), np.uint16)
    img[2:] = 300
    img[3, 3] = (250, 900, 300)
    valid = nd.mask_from_value(img, 0)
    assert nd.valid_range(img, None) == (0, 900) and nd.valid_range(img, valid) == (250, 900)
    flat = np.full((2, 2, 3), 77, np.uint16)
    assert nd.valid_range(flat, None) == (76, 77)                         # a constant raster: (v - 1, v) ...
    assert nd.valid_range(np.zeros((2, 2, 3), np.uint16), None) == (0, 1)  # ... or (0, 1) at 0: _apply_wow_sr16's rules
    assert nd.valid_range(img, np.zeros((4, 4), np.uint8)) == (0, 1)      # no valid pixel
    img2 = np.array(img)
    img2[3, 3] = 300
    assert nd.valid_range(img2, valid) == (299, 300)                      # constant over the valid pixels


def test_upsample_mask():
    v = np.array([[1, 0, 2]], np.uint8)
    assert np.array_equal(nd.upsample_mask(v, 2), [[1, 1, 0, 0, 1, 1]] * 2)
    with pytest.raises(ValueError):
        nd.upsample_mask(v, 0)


@pytest.mark.parametrize("kw,match", [(dict(nodata=0, fill_radius=0), "fill_radius"), (dict(nodata=0, fill_radius=65), "fill_radius"),
                                      (dict(nodata=0, fill_radius=2.5), "fill_radius"), (dict(nodata="band"), "nodata"),
                                      (dict(nodata=1.5), "nodata"), (dict(nodata=True), "nodata"), (dict(nodata=-1), "nodata"),
                                      (dict(nodata=65536, bit_depth=16, enhance_crops=False), "nodata"),
                                      (dict(nodata="tag"), "GDAL_NODATA"), (dict(nodata="tag", bit_depth=16, enhance_crops=False), "GDAL_NODATA")])
def test_process_wow_sr_refuses_bad_arguments_before_anything_is_created(tmp_path, kw, match):
    from app import wow_sr
    src = tmp_path / "in.tif"
    rio.write_geotiff_rgb16(src, _img(np.uint16), GEOREF)                 # (no tag)
    out = tmp_path / "out"
    with pytest.raises(ValueError, match=match):
        wow_sr.process_wow_sr(src, out, **kw)
    assert not out.exists() or not any(out.iterdir())


def test_api_wow_body_takes_nodata_and_refuses_bad_values(tmp_path, monkeypatch):
    from fastapi.testclient import TestClient

    from app import wow_sr
    from app.sr_routes import create_app
    seen = {}

    def fake(input_tif, output_dir, enhance_crops=True, model="realesrgan_x4", **kw):      # the job function, without a GPU
        seen.update(kw)
        raise RuntimeError("stop here")
    monkeypatch.setattr(wow_sr, "process_wow_sr", fake)
    c = TestClient(create_app(tmp_path / "data"))
    f = tmp_path / "a.tif"
    rio.write_geotiff_rgb(f, _img(np.uint8), GEOREF, nodata=0)
    for body in ({"nodata": "band"}, {"nodata": 0, "fill_radius": 0}, {"nodata": 0, "fill_radius": 65}):
        r = c.post("/api/wow", json=dict(body, input_file=str(f)))
        assert r.status_code == 400, (body, r.status_code)
    assert not seen
    assert c.post("/api/wow", json={"input_file": str(f)}).status_code == 200
    assert "nodata" not in seen and "fill_radius" not in seen                              # a plain job's call is what it was
    assert c.post("/api/wow", json={"input_file": str(f), "nodata": "tag", "fill_radius": 16}).status_code == 200
    assert seen["nodata"] == "tag" and seen["fill_radius"] == 16
