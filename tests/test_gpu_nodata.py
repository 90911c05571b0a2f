"""Nodata-aware enhance on the GPU (include/s2sr.h: s2sr_fill_nodata_*, s2sr_enhance_masked_*) and its Python seam.

The fill is held to tests/nodata_model.py byte for byte (the model's two forms are held to each other in tests/test_nodata_cpu.py).
The masked doors are held to the definition's composition, exactly: masked(img) == numpy_mask(unmasked door(model_fill(img))), the
unmasked door being the engine's own.  Every test runs under red zones (native.redzone(Z)) on engines created with them, and ends
with a clean redzone_check().  1-block nets, tile 16: the shapes of tests/test_gpu_blend.py."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import diag
import nodata_model as nm
import probe_model as pm
from diag import Z, clean
from s2sr import native

pytestmark = pytest.mark.gpu

HP = native.PREC_F16_HP
NAMES = {"x4": "x4_hp", "x2": "x2plus", "compact": "compact"}       # this module's names for the 1-block HP configs of tests/doors.py
WHOLE, BANDED, CHUNKED = (28, 36, 256, 10), (100, 90, 16, 2), (53, 200, 16, 3)     # tests/test_gpu_blend.py: untiled, one chunk, three chunks
FILL_SHAPES = [(37, 53), (70, 300)]                # the second: wider than one workgroup tile (256 columns), five tile rows
RADII = [1, 5, 32, 64]
KINDS = ["holes", "edge", "island", "all_valid", "all_invalid"]
LO, HI = 100, 10300


@pytest.fixture(scope="module")
def zoned():
    """name -> an engine created (and so allocated) under red zones"""
    with diag.engines_under(native.redzone_bytes, native.redzone, Z) as get:
        yield lambda name: get(NAMES[name])


def same(got, want, what):
    why = pm.first_difference(got, want)
    assert not why, f"{what}: {why}"


@functools.lru_cache(maxsize=None)
def image(H, W, dtype="uint8", seed=11):
    top = 256 if dtype == "uint8" else 13000
    a = np.random.default_rng(seed + 1000 * H + W).integers(1, top, size=(H, W, 3)).astype(dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def sources(kind, H, W, R):
    s = nm.sources_separable(nm.make_mask(kind, H, W), R)
    s.setflags(write=False)
    return s


def model_fill(img, kind, R):
    H, W = img.shape[:2]
    s = sources(kind, H, W, R)
    return np.ascontiguousarray(img[s[..., 0], s[..., 1]])


def nodata_image(H, W, kind, dtype="uint8"):
    """The raster as a file would hold it: the invalid pixels are 0."""
    img = np.array(image(H, W, dtype))
    img[nm.make_mask(kind, H, W) == 0] = 0
    return img


# ---- the fill --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("H,W", FILL_SHAPES)
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_fill_is_the_model_byte_for_byte(zoned, dtype, H, W, R):
    e = zoned("x4")
    for kind in KINDS:
        valid = nm.make_mask(kind, H, W)
        img = nodata_image(H, W, kind, dtype)
        got = e.fill_nodata(img, valid, R)
        want = model_fill(img, kind, R)
        changed = int((want != img).any(axis=2).sum())
        print(f"{dtype} {H}x{W} R {R} {kind}: {int((valid == 0).sum())} invalid, {changed} filled")
        assert got.dtype == img.dtype
        same(got, want, f"{dtype} {H}x{W} R {R} {kind}")
        if kind in ("all_valid", "all_invalid"):
            same(got, img, f"{kind} is the identity")
        elif R >= 5:
            assert changed > 0                               # the case does fill something
    clean(e)


def test_fill_needs_no_weights_and_takes_any_truthy_mask(zoned):
    native.redzone(Z)
    e = native.Engine(num_block=1, precision=HP)
    try:
        H, W = 37, 53
        img, valid = nodata_image(H, W, "holes"), nm.make_mask("holes", H, W)
        same(e.fill_nodata(img, valid * 200, 5), model_fill(img, "holes", 5), "mask bytes of 200")
        same(e.fill_nodata(img, valid.astype(bool), 5), model_fill(img, "holes", 5), "a bool mask")
        clean(e, least=3)                                        # the trash page, the image (scratch 0), the mask copy (scratch 6)
    finally:
        e.close()


def test_out_of_range_arguments_are_refused_and_the_engine_works_afterwards(zoned):
    e = zoned("x4")
    H, W = 37, 53
    img, valid = nodata_image(H, W, "holes"), nm.make_mask("holes", H, W)
    img16 = nodata_image(H, W, "holes", "uint16")
    for R in (0, -1, 65, 1 << 20):
        with pytest.raises(native.S2srError, match="radius"):
            e.fill_nodata(img, valid, R)
        with pytest.raises(native.S2srError, match="radius"):
            e.enhance_masked_u8(img, valid, radius=R)
        with pytest.raises(native.S2srError, match="radius"):
            e.enhance_masked_u16(img16, valid, LO, HI, radius=R)
    for bad in (-1, 256):
        with pytest.raises(native.S2srError, match="out_nodata"):
            e.enhance_masked_u8(img, valid, out_nodata=bad)
    for bad in (-1, 65536):
        with pytest.raises(native.S2srError, match="out_nodata"):
            e.enhance_masked_u16(img16, valid, LO, HI, out_nodata=bad)
    with pytest.raises(ValueError):
        e.fill_nodata(img, valid[:, :-1], 5)
    # m == NULL and m->valid == NULL, through the C ABI
    out = np.zeros((4 * H, 4 * W, 3), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = e._lib
    assert lib.s2sr_enhance_masked_u8(e._h, ptr(img), H, W, 16, 2, None, 0, 0, None, ptr(out)) == -1
    assert b"mask" in lib.s2sr_last_error(e._h)
    m = native.Mask(None, 32, 0)
    assert lib.s2sr_enhance_masked_u8(e._h, ptr(img), H, W, 16, 2, None, 0, 0, C.byref(m), ptr(out)) == -1
    assert b"mask" in lib.s2sr_last_error(e._h)
    out16 = np.zeros((4 * H, 4 * W, 3), np.uint16)
    assert lib.s2sr_enhance_masked_u16(e._h, ptr(img16), H, W, 16, 2, LO, HI, 0, None, ptr(out16)) == -1
    assert lib.s2sr_fill_nodata_u8(e._h, ptr(img), None, H, W, 5, ptr(out)) == -1
    assert not out.any() and not out16.any()                 # refused before anything was written
    same(e.fill_nodata(img, valid, 5), model_fill(img, "holes", 5), "the engine after the refusals")
    clean(e)


# ---- composition: masked == numpy_mask(unmasked door(model_fill(img))) -------------------------------------------------------------
def _u8(**kw):
    """(masked call, unmasked door) of an 8-bit door"""
    def masked(e, img, valid, R, nd, tile, pad):
        return e.enhance_masked_u8(img, valid, radius=R, out_nodata=nd, tile=tile, pad=pad, **kw)

    def plain(e, img, tile, pad):
        if kw.get("blend"):
            return e.enhance_blend_u8(img, prm=kw.get("prm"), swap_rb=kw.get("swap_rb", False), tile=tile, pad=pad)
        if kw.get("swap_rb"):
            return e.enhance_job_u8(img, kw.get("prm"), tile=tile, pad=pad)
        return e.enhance_u8(img, tile=tile, pad=pad)
    return masked, plain


def _u16(blend):
    def masked(e, img, valid, R, nd, tile, pad):
        return e.enhance_masked_u16(img, valid, LO, HI, radius=R, out_nodata=nd, blend=blend, tile=tile, pad=pad)

    def plain(e, img, tile, pad):
        return (e.enhance_blend_u16 if blend else e.enhance_u16)(img, LO, HI, tile=tile, pad=pad)
    return masked, plain


# door -> (engine, dtype, (masked, plain), images)
DOORS = {
    "u8": ("x4", "uint8", _u8(), [WHOLE, BANDED, CHUNKED]),
    "u8_swap_rb": ("x4", "uint8", _u8(swap_rb=True), [WHOLE, CHUNKED]),
    "job": ("x4", "uint8", _u8(swap_rb=True, prm=native.pp_wow()), [WHOLE, BANDED, CHUNKED]),     # whole / one chunk: the single-chunk tail; three chunks: banded
    "blend_u8": ("x4", "uint8", _u8(blend=True), [BANDED, CHUNKED]),
    "blend_job": ("x4", "uint8", _u8(blend=True, swap_rb=True, prm=native.pp_wow()), [BANDED]),
    "u16": ("x4", "uint16", _u16(False), [WHOLE, BANDED, CHUNKED]),
    "blend_u16": ("x4", "uint16", _u16(True), [BANDED, CHUNKED]),
    "compact": ("compact", "uint8", _u8(), [CHUNKED]),
    "x2_odd": ("x2", "uint8", _u8(), [(27, 35, 256, 10), (53, 37, 16, 2)]),                        # odd H and W: the job runs on the padded image
}
CASES = [(d, im) for d, v in DOORS.items() for im in v[3]]


@pytest.mark.parametrize("door,im", CASES, ids=[f"{d}-{im[0]}x{im[1]}" for d, im in CASES])
def test_masked_door_is_mask_of_door_of_fill(zoned, door, im):
    name, dtype, (masked, plain), _ = DOORS[door]
    e = zoned(name)
    H, W, tile, pad = im
    kind, R = ("edge", 32) if door in ("u8", "u16") else ("holes", 5)
    nd = {"u8": 0, "u16": 0}.get(door, 65535 if dtype == "uint16" else 7)
    valid = nm.make_mask(kind, H, W)
    img = nodata_image(H, W, kind, dtype)
    filled = model_fill(img, kind, R)
    assert (filled != img).any()
    got = np.array(masked(e, img, valid, R, nd, tile, pad))
    door_out = np.array(plain(e, filled, tile, pad))
    want = nm.mask(door_out, valid, e.scale, nd)
    inv = ~nm.upsample(valid, e.scale)
    print(f"{door} {H}x{W}: {int(inv.sum())} of {inv.size} output pixels masked")
    assert got.dtype == door_out.dtype and inv.any() and not inv.all()
    same(got, want, f"{door} {H}x{W} {tile}/{pad}")
    assert (np.array(plain(e, img, tile, pad))[~inv] != got[~inv]).any()        # the control: the fill changed what the net made of the valid area
    clean(e)


# ---- no side effects ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("door", ["u8", "job", "blend_u8", "u16", "blend_u16", "x2_odd"])
def test_an_all_valid_mask_gives_the_unmasked_doors_bytes(zoned, door):
    name, dtype, (masked, plain), images = DOORS[door]
    e = zoned(name)
    for H, W, tile, pad in images:
        img = np.array(image(H, W, dtype))
        img[: H // 3, : W // 2] = 0                        # zeros that are data: valid, so they stay what the net makes of them
        got = np.array(masked(e, img, np.ones((H, W), np.uint8), 32, 0, tile, pad))
        same(got, np.array(plain(e, img, tile, pad)), f"{door} {H}x{W}")
    clean(e)


def test_a_masked_call_between_two_plain_calls_and_a_repeat(zoned):
    e = zoned("x4")
    H, W, tile, pad = CHUNKED
    img, valid = nodata_image(H, W, "holes"), nm.make_mask("holes", H, W)
    img16 = nodata_image(H, W, "holes", "uint16")
    before = np.array(e.enhance_u8(img, tile=tile, pad=pad))
    before16 = np.array(e.enhance_u16(img16, LO, HI, tile=tile, pad=pad))
    m1 = np.array(e.enhance_masked_u8(img, valid, radius=5, out_nodata=9, tile=tile, pad=pad))
    same(np.array(e.enhance_u8(img, tile=tile, pad=pad)), before, "the plain u8 door after a masked call")
    m16 = np.array(e.enhance_masked_u16(img16, valid, LO, HI, radius=5, tile=tile, pad=pad))
    same(np.array(e.enhance_u16(img16, LO, HI, tile=tile, pad=pad)), before16, "the plain u16 door after a masked call")
    _, r0 = e.graph_stats()
    same(np.array(e.enhance_masked_u8(img, valid, radius=5, out_nodata=9, tile=tile, pad=pad)), m1, "the repeat u8 call")
    same(np.array(e.enhance_masked_u16(img16, valid, LO, HI, radius=5, tile=tile, pad=pad)), m16, "the repeat u16 call")
    _, r1 = e.graph_stats()
    assert r1 > r0, (r0, r1)                               # the repeats replayed the captured groups
    # the device image the 16-bit door leaves for the display calls is the masked one
    hist = e.display_hist_u16(None, shape=(4 * H, 4 * W))
    want = np.stack([np.bincount(m16[..., c].ravel(), minlength=65536) for c in range(3)]).astype(np.uint64)
    same(hist, want, "the histogram of the image left on the device")
    clean(e)


# ---- the Python seam -----------------------------------------------------------------------------------------------------------------
def _patch_weights(monkeypatch, tmp_path):
    """A seeded 6-block checkpoint where the operator looks for realesrgan_anime (tests/test_gpu_app.py)."""
    import torch
    from s2sr.weights import synthetic_state_dict
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir(exist_ok=True)
    sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(6, seed=0).items()}
    torch.save({"params_ema": sd}, tmp_path / "models" / "realesrgan_anime.pth")


def _scene(dtype):
    """64 x 48, a zeroed corner: the raster of a clipped AOI."""
    img = np.array(image(64, 48, dtype, seed=5))
    img[:20, :17] = 0
    if dtype == "uint8":       # zero bands of a measured pixel; the uint16 scene has none, so the smallest sample of its valid
        img[40, 30] = (0, img[40, 30, 1], 0)               # pixels -- the job's lo -- is above the nodata value
    return img


def test_realesrgan_keywords_are_the_engine_entries(zoned, monkeypatch, tmp_path):
    import app.cnn_super_resolution as m
    from s2sr.nodata import mask_from_value
    _patch_weights(monkeypatch, tmp_path)
    op = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)
    eng = op._engine
    img, img16 = _scene("uint8"), _scene("uint16")
    valid = mask_from_value(img, 0)
    assert not valid[:20, :17].any() and valid[40, 30] and int((valid == 0).sum()) == 20 * 17
    want = np.array(eng.enhance_masked_u8(img, valid, radius=32, out_nodata=0, tile=256, pad=10))
    same(np.array(op.enhance(img, nodata=0)), want, "enhance(img, nodata=0)")
    same(np.array(op.enhance(img, valid=valid)), want, "enhance(img, valid=valid)")
    assert not want[:80, :68].any() and (np.array(op.enhance(img))[:80, :68] != 0).any()
    want = np.array(eng.enhance_masked_u8(img, valid, radius=7, out_nodata=0, prm=native.pp_wow(), swap_rb=True, tile=256, pad=10))
    same(np.array(op.enhance_job(img, native.pp_wow(), nodata=0, fill_radius=7)), want, "enhance_job(nodata=0, fill_radius=7)")
    want = np.array(eng.enhance_masked_u16(img16, mask_from_value(img16, 0), LO, HI, radius=32, out_nodata=0, tile=256, pad=10))
    same(np.array(op.enhance16(img16, value_range=(LO, HI), nodata=0)), want, "enhance16(nodata=0)")
    blended = m.RealESRGAN(model_name="realesrgan_anime", tile_size=16, seam_blend=True)
    blended.tile_pad = 2
    want = np.array(eng.enhance_masked_u8(img, valid, radius=32, out_nodata=0, blend=True, tile=16, pad=2))
    same(np.array(blended.enhance(img, nodata=0)), want, "seam_blend + nodata")
    for bad in (dict(nodata=0, fill_radius=0), dict(nodata="tag"), dict(valid=valid[:, :-1])):
        with pytest.raises(ValueError):
            op.enhance(img, **bad)
    clean(eng, least=0)


def test_process_wow_sr_with_the_files_nodata_tag(zoned, monkeypatch, tmp_path):
    from PIL import Image

    from app.wow_sr import process_wow_sr
    from s2sr import rasterio_lite as rio
    from s2sr.nodata import mask_from_value, upsample_mask, valid_range
    import app.cnn_super_resolution as m
    _patch_weights(monkeypatch, tmp_path)
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)})
    img, img16 = _scene("uint8"), _scene("uint16")
    rio.write_geotiff_rgb(tmp_path / "s8.tif", img, geo, nodata=0)
    rio.write_geotiff_rgb16(tmp_path / "s16.tif", img16, geo, nodata=0)
    rio.write_geotiff_rgb(tmp_path / "plain.tif", img, geo)
    up = upsample_mask(mask_from_value(img, 0), 4) != 0
    block = {"value": 0, "invalid_pixels": 20 * 17, "fill_radius": 32}

    # the 8-bit job: tag, RGBA PNG, metadata; the bytes are the operator's
    res = process_wow_sr(tmp_path / "s8.tif", tmp_path / "w8", enhance_crops=True, model="realesrgan_anime", nodata="tag")
    meta = res["sr_metadata"]
    assert meta["nodata"] == block
    assert json.load(open(tmp_path / "w8" / "s8_wow_sr_metadata.json"))["sr_metadata"]["nodata"] == block
    out, g4 = rio.read_rgb_raw(res["outputs"]["sr_tif"])
    assert g4.nodata == 0 and g4.pixel_size == (2.5, 2.5) and out.shape == (256, 192, 3)
    op = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)
    same(out, np.array(op.enhance_job(img, native.pp_wow(), nodata=0)), "the job's GeoTIFF")
    assert not out[~up].any() and (out[up] != 0).any()
    png = np.asarray(Image.open(res["outputs"]["sr_png"]))
    assert png.shape == (256, 192, 4) and np.array_equal(png[..., :3], out) and np.array_equal(png[..., 3], up * np.uint8(255))
    # without nodata the job is what it was: no tag, an RGB PNG, no metadata block
    plain = process_wow_sr(tmp_path / "s8.tif", tmp_path / "p8", enhance_crops=True, model="realesrgan_anime")
    assert "nodata" not in plain["sr_metadata"] and rio.read_rgb_raw(plain["outputs"]["sr_tif"])[1].nodata is None
    assert np.asarray(Image.open(plain["outputs"]["sr_png"])).shape == (256, 192, 3)
    same(rio.read_rgb_raw(plain["outputs"]["sr_tif"])[0], np.array(op.enhance_job(img, native.pp_wow())), "the plain job's GeoTIFF")
    with pytest.raises(ValueError, match="GDAL_NODATA"):
        process_wow_sr(tmp_path / "plain.tif", tmp_path / "none", model="realesrgan_anime", nodata="tag")

    # the 16-bit job: the value range ignores the zeros; with a display stretch the PNG carries the mask and the stretch the value
    valid16 = mask_from_value(img16, 0)
    lo, hi = valid_range(img16, valid16)
    assert lo > 0 and (lo, hi) == (int(img16[valid16 != 0].min()), int(img16.max()))
    res = process_wow_sr(tmp_path / "s16.tif", tmp_path / "w16", enhance_crops=False, model="realesrgan_anime", bit_depth=16, nodata="tag",
                         fill_radius=9, display={"p_lo": 2.0, "p_hi": 98.0})
    meta = res["sr_metadata"]
    assert meta["value_range"] == [lo, hi] and meta["nodata"] == dict(block, fill_radius=9) and meta["display"]["nodata"] == 0
    out16, g16 = rio.read_rgb_raw(res["outputs"]["sr_tif"])
    assert out16.dtype == np.uint16 and g16.nodata == 0 and not out16[~up].any() and (out16[up] >= lo).all()
    want = op.enhance16(np.ascontiguousarray(img16[:, :, ::-1]), value_range=(lo, hi), nodata=0, fill_radius=9)
    same(out16, np.ascontiguousarray(np.array(want)[:, :, ::-1]), "the 16-bit job's GeoTIFF")
    png = np.asarray(Image.open(res["outputs"]["sr_png"]))
    assert png.shape == (256, 192, 4) and np.array_equal(png[..., 3], up * np.uint8(255))
    clean(op._engine, least=0)
