"""Radiometric consistency on the GPU (include/s2sr.h: s2sr_consistency_*, s2sr_enhance_consistent_*) and its
Python seam.

The pass alone is held to tests/consistency_model.py byte for byte, counts included.  The consistent doors are held to the
composition law, exactly: consistent(img) == tail(model(plain door's bytes, the image the net saw)), the plain door and the tail
(post-process, mask) being the engine's own and numpy's.  Every test runs under red zones on engines created with them and ends
with a clean redzone_check().  1-block nets, tile 16: the shapes of tests/test_gpu_nodata.py."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import consistency_model as cm
import diag
import nodata_model as nm
import probe_model as pm
from diag import Z, clean
from s2sr import native

pytestmark = pytest.mark.gpu

HP = native.PREC_F16_HP
NAMES = {"x4": "x4_hp", "x2": "x2plus", "compact": "compact"}       # this module's names for the 1-block HP configs of tests/doors.py
WHOLE, BANDED, CHUNKED = (28, 36, 256, 10), (100, 90, 16, 2), (53, 200, 16, 3)     # tests/test_gpu_blend.py: untiled, one chunk, three chunks
# 1 x 1; odd; ragged; three 16-pixel workgroup tiles on both axes, ragged on both (S = 2: two 32-pixel tiles); one block row; one block column
PASS_SHAPES = [(1, 1), (3, 5), (17, 33), (40, 75), (5, 300), (300, 5)]
# (0..65535: half the samples of either input have bit 15 set; cm.clip_free_input's corner of hi + 500 does not fit uint16 there and wraps
# to 499 under a prediction of 65535: a residual of -65036 a sample, which the smooth step spreads into its neighbours until they clip)
KINDS = [("uint8", 0, 255), ("uint16", 100, 4000), ("uint16", 0, 65535)]
LO, HI = 100, 10300
MODES = [cm.EXACT, cm.SMOOTH]


@pytest.fixture(scope="module")
def zoned():
    """name -> an engine created (and so allocated) under red zones"""
    with diag.engines_under(native.redzone_bytes, native.redzone, Z) as get:
        yield lambda name: get(NAMES[name])


def same(got, want, what):
    why = pm.first_difference(np.asarray(got), np.asarray(want))
    assert not why, f"{what}: {why}"


@functools.lru_cache(maxsize=None)
def pass_case(kind, H, W, S, dtype, lo, hi):
    make = cm.clip_free_input if kind == "clip_free" else cm.saturating_input
    sr, img = make(H, W, S, dtype=dtype, lo=lo, hi=hi)
    sr.setflags(write=False)
    img.setflags(write=False)
    return sr, img


@functools.lru_cache(maxsize=None)
def modelled(kind, H, W, S, dtype, lo, hi, mode):
    sr, img = pass_case(kind, H, W, S, dtype, lo, hi)
    out, bad = cm.consistency(sr, img, S, mode, lo, hi)
    out.setflags(write=False)
    return out, bad


# ---- the pass alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,lo,hi", KINDS)
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("mode", MODES)
def test_pass_is_the_model_byte_for_byte(zoned, mode, S, dtype, lo, hi):
    e = zoned("x4")
    for kind in ("clip_free", "saturating"):
        for H, W in PASS_SHAPES:
            sr, img = pass_case(kind, H, W, S, dtype, lo, hi)
            want, bad = modelled(kind, H, W, S, dtype, lo, hi, mode)
            got, n = e.consistency(sr, img, mode, lo, hi)
            print(f"{dtype} S {S} mode {mode} {kind} {H}x{W}: inexact {n.tolist()} (model {bad.tolist()}) of {H * W}")
            assert got.dtype == sr.dtype
            same(got, want, f"{dtype} S {S} mode {mode} {kind} {H}x{W}")
            assert n.tolist() == bad.tolist()
            if kind == "clip_free" and (hi + 500 <= 65535 or mode == cm.EXACT):
                assert not n.any()
            elif H * W >= 500:
                assert n.min() > 0                               # the clip paths are taken
    clean(e)


def test_pass_needs_no_weights(zoned):
    native.redzone(Z)
    e = native.Engine(num_block=1, precision=HP)
    try:
        for mode in MODES:
            sr, img = pass_case("saturating", 17, 33, 4, "uint8", 0, 255)
            want, bad = modelled("saturating", 17, 33, 4, "uint8", 0, 255, mode)
            got, n = e.consistency(sr, img, mode)
            same(got, want, f"mode {mode} on an engine without weights")
            assert n.tolist() == bad.tolist()
        clean(e, least=3)                                        # the trash page, the two images (and the counters' area)
    finally:
        e.close()


@pytest.mark.parametrize("dtype,lo,hi", KINDS)
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("mode", MODES)
def test_bands_do_not_change_the_bytes(zoned, mode, S, dtype, lo, hi):
    """band_rows drives the trailing-band logic: a band that ends inside a block row, and mode 2's wait for the block row below."""
    e = zoned("x4")
    for H, W in [(17, 33), (40, 75)]:
        sr, img = pass_case("saturating", H, W, S, dtype, lo, hi)
        want, bad = modelled("saturating", H, W, S, dtype, lo, hi, mode)
        for band_rows in (S, 3 * S, 7, 1, 5 * S + 1, 0):
            got, n = e.consistency(sr, img, mode, lo, hi, band_rows=band_rows)
            same(got, want, f"{dtype} S {S} mode {mode} {H}x{W} band_rows {band_rows}")
            assert n.tolist() == bad.tolist(), band_rows
    clean(e)


def test_refusals_and_the_engine_works_afterwards(zoned):
    e = zoned("x4")
    sr, img = pass_case("saturating", 17, 33, 4, "uint8", 0, 255)
    sr16, img16 = pass_case("saturating", 17, 33, 4, "uint16", 100, 4000)
    for mode in (0, 3, -1):
        with pytest.raises(native.S2srError, match="mode"):
            e.consistency(sr, img, mode)
        with pytest.raises(native.S2srError, match="mode"):
            e.consistency(sr16, img16, mode, 100, 4000)
        with pytest.raises(native.S2srError, match="mode"):
            e.enhance_consistent_u8(img, mode, tile=16, pad=2)
        with pytest.raises(native.S2srError, match="mode"):
            e.enhance_consistent_u16(img16, LO, HI, mode, tile=16, pad=2)
    with pytest.raises(native.S2srError, match="band_rows"):
        e.consistency(sr, img, 1, band_rows=-1)
    with pytest.raises(native.S2srError, match="lo < hi"):
        e.consistency(sr16, img16, 1, 4000, 100)
    out = np.zeros_like(sr)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = e._lib
    assert lib.s2sr_consistency_u8(e._h, None, ptr(img), 17, 33, 4, 1, 0, ptr(out), None) == -1
    assert b"images" in lib.s2sr_last_error(e._h)
    assert lib.s2sr_consistency_u8(e._h, ptr(sr), None, 17, 33, 4, 1, 0, ptr(out), None) == -1
    assert lib.s2sr_consistency_u8(e._h, ptr(sr), ptr(img), 17, 33, 4, 1, 0, None, None) == -1
    assert lib.s2sr_consistency_u8(e._h, ptr(sr), ptr(img), 17, 33, 3, 1, 0, ptr(out), None) == -1
    assert lib.s2sr_consistency_u8(e._h, ptr(sr), ptr(img), 0, 33, 4, 1, 0, ptr(out), None) == -1
    big = np.zeros((68, 132, 3), np.uint8)
    assert lib.s2sr_enhance_consistent_u8(e._h, None, 17, 33, 16, 2, None, 0, 0, None, 1, ptr(big), None) == -1
    assert not out.any() and not big.any()                       # refused before anything was written
    want, bad = modelled("saturating", 17, 33, 4, "uint8", 0, 255, 2)
    got, n = e.consistency(sr, img, 2)                           # inexact may be NULL, and out may be sr
    same(got, want, "the engine after the refusals")
    inplace = np.array(sr)
    assert lib.s2sr_consistency_u8(e._h, ptr(inplace), ptr(img), 17, 33, 4, 2, 8, ptr(inplace), None) == 0
    same(inplace, want, "out == sr, inexact NULL")
    clean(e)


# ---- the composition law -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def image(H, W, dtype="uint8", seed=11):
    top = 256 if dtype == "uint8" else 13000
    a = np.random.default_rng(seed + 1000 * H + W).integers(1, top, size=(H, W, 3)).astype(dtype)
    a.setflags(write=False)
    return a


def flip(a):
    return np.ascontiguousarray(np.asarray(a)[:, :, ::-1])


# door -> (engine, dtype, keywords of the consistent call, images)
DOORS = {
    "u8": ("x4", "uint8", {}, [WHOLE, BANDED, CHUNKED]),
    "job": ("x4", "uint8", dict(swap_rb=True, prm=native.pp_wow()), [WHOLE, BANDED, CHUNKED]),   # three chunks: the banded post-process
    "u8_swap_rb": ("x4", "uint8", dict(swap_rb=True), [WHOLE, CHUNKED]),
    "blend_u8": ("x4", "uint8", dict(blend=True), [BANDED, CHUNKED]),
    "blend_job": ("x4", "uint8", dict(blend=True, swap_rb=True, prm=native.pp_wow()), [BANDED]),
    "blend_swap_rb": ("x4", "uint8", dict(blend=True, swap_rb=True), [BANDED, CHUNKED]),          # the paste has exchanged R and B: the flag
    "u16": ("x4", "uint16", {}, [WHOLE, BANDED, CHUNKED]),
    "blend_u16": ("x4", "uint16", dict(blend=True), [BANDED, CHUNKED]),
    "x2_odd": ("x2", "uint8", {}, [(27, 35, 256, 10), (53, 37, 16, 2)]),                          # odd H and W: the job runs on the padded image
    "compact": ("compact", "uint8", {}, [CHUNKED]),
}
CASES = [(d, im) for d, v in DOORS.items() for im in v[3]]
MASKED = [("u8", CHUNKED), ("job", CHUNKED), ("blend_job", BANDED), ("u16", CHUNKED), ("blend_u16", BANDED), ("x2_odd", (53, 37, 16, 2))]


def consistent(e, door, img, mode, tile, pad, **mask):
    _, dtype, kw, _ = DOORS[door]
    if dtype == "uint16":
        return e.enhance_consistent_u16(img, LO, HI, mode, tile=tile, pad=pad, **kw, **mask)
    return e.enhance_consistent_u8(img, mode, tile=tile, pad=pad, **kw, **mask)


def by_the_law(e, door, img, mode, tile, pad):
    """(bytes, inexact, the plain door's bytes through the same tail) from the plain door's bytes"""
    _, dtype, kw, _ = DOORS[door]
    S = e.scale
    if dtype == "uint16":
        plain = np.array((e.enhance_blend_u16 if kw.get("blend") else e.enhance_u16)(img, LO, HI, tile=tile, pad=pad))
        out, bad = cm.consistency(plain, img, S, mode, LO, HI)
        return out, bad, plain
    door8 = (lambda a: e.enhance_blend_u8(a, tile=tile, pad=pad)) if kw.get("blend") else (lambda a: e.enhance_u8(a, tile=tile, pad=pad))
    if not kw.get("swap_rb"):
        plain = np.array(door8(img))
        out, bad = cm.consistency(plain, img, S, mode)
        return out, bad, plain
    bgr = flip(img)                                              # the job: the net sees B, G, R; the pass runs before the exchange back
    plain = np.array(door8(bgr))
    out, bad = cm.consistency(plain, bgr, S, mode)
    out, bad, plain = flip(out), bad[::-1], flip(plain)
    if kw.get("prm") is not None:                                # the job's tail: the post-process on the model's output
        out, plain = e.postprocess_u8(out, kw["prm"]), e.postprocess_u8(plain, kw["prm"])
    return np.asarray(out), bad, np.asarray(plain)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("door,im", CASES, ids=[f"{d}-{im[0]}x{im[1]}" for d, im in CASES])
def test_consistent_door_is_tail_of_model_of_door(zoned, door, im, mode):
    name, dtype, _, _ = DOORS[door]
    e = zoned(name)
    H, W, tile, pad = im
    img = np.array(image(H, W, dtype))
    got, n = consistent(e, door, img, mode, tile, pad)
    want, bad, plain = by_the_law(e, door, img, mode, tile, pad)
    print(f"{door} {H}x{W} mode {mode}: inexact {n.tolist()} of {H * W}; {int((np.asarray(got) != plain).sum())} samples differ from the plain door's")
    assert np.asarray(got).dtype == want.dtype
    same(got, want, f"{door} {H}x{W} {tile}/{pad} mode {mode}")
    assert n.tolist() == bad.tolist()
    assert (np.asarray(got) != plain).any()                      # the control: the pass changed the door's bytes
    clean(e)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("door,im", MASKED, ids=[f"{d}-{im[0]}x{im[1]}" for d, im in MASKED])
def test_masked_consistent_door_is_mask_of_the_law_on_the_filled_image(zoned, door, im, mode):
    name, dtype, _, _ = DOORS[door]
    e = zoned(name)
    H, W, tile, pad = im
    R, nd = 5, 65535 if dtype == "uint16" else 7
    valid = nm.make_mask("edge", H, W)                           # a diagonal edge: bands, blocks and workgroup tiles all cut through it
    img = np.array(image(H, W, dtype))
    img[valid == 0] = 0
    filled = nm.fill(img, valid, R)
    assert (filled != img).any()
    got, n = consistent(e, door, img, mode, tile, pad, valid=valid, radius=R, out_nodata=nd)
    want, bad, _ = by_the_law(e, door, filled, mode, tile, pad)
    want = nm.mask(want, valid, e.scale, nd)
    inv = ~nm.upsample(valid, e.scale)
    assert inv.any() and not inv.all()
    same(got, want, f"masked {door} {H}x{W} mode {mode}")
    assert n.tolist() == bad.tolist()                            # every block counts, filled ones included
    clean(e)


# ---- no side effects ---------------------------------------------------------------------------------------------------------------
def test_a_consistent_call_between_two_plain_calls_and_a_repeat(zoned):
    e = zoned("x4")
    H, W, tile, pad = CHUNKED
    img, img16 = np.array(image(H, W)), np.array(image(H, W, "uint16"))
    before = np.array(e.enhance_u8(img, tile=tile, pad=pad))
    before16 = np.array(e.enhance_u16(img16, LO, HI, tile=tile, pad=pad))
    c1, n1 = e.enhance_consistent_u8(img, 2, tile=tile, pad=pad)
    c1 = np.array(c1)
    same(e.enhance_u8(img, tile=tile, pad=pad), before, "the plain u8 door after a consistent call")
    c16, n16 = e.enhance_consistent_u16(img16, LO, HI, 2, tile=tile, pad=pad)
    c16 = np.array(c16)
    # the device image the 16-bit door leaves for the display calls is the consistent one
    hist = e.display_hist_u16(None, shape=(4 * H, 4 * W))
    want = np.stack([np.bincount(c16[..., c].ravel(), minlength=65536) for c in range(3)]).astype(np.uint64)
    same(hist, want, "the histogram of the image left on the device")
    assert (c16 != before16).any()
    same(e.enhance_u16(img16, LO, HI, tile=tile, pad=pad), before16, "the plain u16 door after a consistent call")
    r1, m1 = e.enhance_consistent_u8(img, 2, tile=tile, pad=pad)
    same(r1, c1, "the repeat u8 call")
    r16, m16 = e.enhance_consistent_u16(img16, LO, HI, 2, tile=tile, pad=pad)
    same(r16, c16, "the repeat u16 call")
    assert m1.tolist() == n1.tolist() and m16.tolist() == n16.tolist()
    with pytest.raises(native.S2srError, match="mode"):          # a refused call in between leaves the handle working
        e.enhance_consistent_u8(img, 3, tile=tile, pad=pad)
    same(e.enhance_consistent_u8(img, 2, tile=tile, pad=pad)[0], c1, "after a refusal")
    clean(e)


def test_kernel_statistics_have_the_family(zoned):
    e = zoned("x4")
    sr, img = pass_case("saturating", 40, 75, 4, "uint8", 0, 255)
    e.reset_kernel_stats()
    e.set_profiling(1)
    try:
        e.consistency(sr, img, 2)
        st = e.kernel_stats()
    finally:
        e.set_profiling(0)
    assert "consistency" in st and st["consistency"]["launches"] == 2, st.get("consistency")     # the residuals, then the pass
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


def test_realesrgan_keyword_reaches_the_engine_entries(zoned, monkeypatch, tmp_path):
    import app.cnn_super_resolution as m
    _patch_weights(monkeypatch, tmp_path)
    img, img16 = np.array(image(64, 48, seed=5)), np.array(image(64, 48, "uint16", seed=5))
    valid = nm.make_mask("edge", 64, 48)
    for name, mode in (("exact", 1), ("smooth", 2)):
        op = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256, consistency=name)
        eng = op._engine
        assert op.last_inexact_blocks is None
        want, n = eng.enhance_consistent_u8(img, mode, tile=256, pad=10)
        want = np.array(want)
        same(op.enhance(img), want, f"enhance, consistency={name}")
        assert op.last_inexact_blocks == n.tolist()
        assert (want != np.array(eng.enhance_u8(img, tile=256, pad=10))).any()
        want, n = eng.enhance_consistent_u8(img, mode, prm=native.pp_wow(), swap_rb=True, tile=256, pad=10)
        same(op.enhance_job(img, native.pp_wow()), np.array(want), f"enhance_job, consistency={name}")
        assert op.last_inexact_blocks == n.tolist()
        want, n = eng.enhance_consistent_u8(img, mode, valid=valid, radius=9, out_nodata=0, tile=256, pad=10)
        same(op.enhance(img, valid=valid, fill_radius=9), np.array(want), f"enhance(valid=), consistency={name}")
        want, n = eng.enhance_consistent_u16(img16, LO, HI, mode, tile=256, pad=10)
        same(op.enhance16(img16, value_range=(LO, HI)), np.array(want), f"enhance16, consistency={name}")
        assert op.last_inexact_blocks == n.tolist()
        want, n = eng.enhance_consistent_u16(img16, LO, HI, mode, valid=valid, radius=32, out_nodata=0, tile=256, pad=10)
        same(op.enhance16(img16, value_range=(LO, HI), valid=valid), np.array(want), f"enhance16(valid=), consistency={name}")
    blended = m.RealESRGAN(model_name="realesrgan_anime", tile_size=16, seam_blend=True, consistency="smooth")
    blended.tile_pad = 2
    want, n = blended._engine.enhance_consistent_u8(img, 2, blend=True, tile=16, pad=2)
    same(blended.enhance(img), np.array(want), "seam_blend + consistency")
    plain = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)
    same(plain.enhance(img), np.array(plain._engine.enhance_u8(img, tile=256, pad=10)), "without the option: the plain door")
    assert plain.last_inexact_blocks is None
    with pytest.raises(ValueError, match="consistency"):
        m.RealESRGAN(model_name="realesrgan_anime", tile_size=256, consistency="both")
    clean(plain._engine, least=0)


def test_process_wow_sr_writes_the_engines_bytes_and_the_metadata_block(zoned, monkeypatch, tmp_path):
    from app.wow_sr import process_wow_sr
    from s2sr import rasterio_lite as rio
    import app.cnn_super_resolution as m
    _patch_weights(monkeypatch, tmp_path)
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)})
    img, img16 = np.array(image(64, 48, seed=5)), np.array(image(64, 48, "uint16", seed=5))
    rio.write_geotiff_rgb(tmp_path / "s8.tif", img, geo)
    rio.write_geotiff_rgb16(tmp_path / "s16.tif", img16, geo)
    eng = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)._engine

    res = process_wow_sr(tmp_path / "s8.tif", tmp_path / "w8", enhance_crops=True, model="realesrgan_anime", consistency="smooth")
    want, n = eng.enhance_consistent_u8(img, 2, prm=native.pp_wow(), swap_rb=True, tile=256, pad=10)
    block = {"mode": "smooth", "inexact_blocks": n.tolist(), "applied_before": "post_process"}
    assert res["sr_metadata"]["consistency"] == block
    assert json.load(open(tmp_path / "w8" / "s8_wow_sr_metadata.json"))["sr_metadata"]["consistency"] == block
    out, g4 = rio.read_rgb_raw(res["outputs"]["sr_tif"])
    assert g4.pixel_size == (2.5, 2.5)
    same(out, np.array(want), "the 8-bit job's GeoTIFF")
    plain = process_wow_sr(tmp_path / "s8.tif", tmp_path / "p8", enhance_crops=True, model="realesrgan_anime")
    assert "consistency" not in plain["sr_metadata"]
    same(rio.read_rgb_raw(plain["outputs"]["sr_tif"])[0], np.array(eng.enhance_job_u8(img, native.pp_wow(), tile=256, pad=10)), "the plain job's GeoTIFF")

    lo, hi = int(img16.min()), int(img16.max())
    res = process_wow_sr(tmp_path / "s16.tif", tmp_path / "w16", enhance_crops=False, model="realesrgan_anime", bit_depth=16, consistency="smooth")
    want, n = eng.enhance_consistent_u16(flip(img16), lo, hi, 2, tile=256, pad=10)
    assert res["sr_metadata"]["value_range"] == [lo, hi]
    assert res["sr_metadata"]["consistency"] == {"mode": "smooth", "inexact_blocks": n.tolist()[::-1]}
    out16, _ = rio.read_rgb_raw(res["outputs"]["sr_tif"])
    assert out16.dtype == np.uint16
    same(out16, flip(want), "the 16-bit job's GeoTIFF")
    # the promise itself, on the file: where nothing clipped, 4 x 4 block means are the input pixels
    exact = cm.block_sums(out16, 4) == 16 * img16.astype(np.int64)      # (lo, hi are the image's own min and max: nothing clamps)
    assert (~exact).sum(axis=(0, 1)).tolist() == n.tolist()[::-1] and exact.any()
    clean(eng, least=0)
