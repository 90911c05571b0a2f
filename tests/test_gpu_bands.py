"""Carrying an extra band to the SR grid on the GPU (include/s2sr.h: s2sr_carry_band_u16; csrc/bands.hip): byte for
byte against tests/bands_model.py, the independence of band_rows, the chain behind the 16-bit door's kept image and every refusal.
The entry under red zones, poison, stalls and capped grids: its rows of tests/doors.py, whose baselines this module holds to the model."""
import numpy as np
import pytest

import bands_model as bm
import diag
import doors
import gpu_engines
from bands_model import case, modelled
from diag import same_values as same
from s2sr import native

pytestmark = pytest.mark.gpu

HP = native.PREC_F16_HP
# the ragged shape, one pixel, a sliver, two tiles of 16 down and across (33 x 17), three by three tiles
SHAPES = [(37, 45), (1, 1), (3, 70), (33, 17), (35, 40)]
RANGES = [(0, 65535), (1000, 11000)]
WEIGHTS = [(1, 1, 1), (0, 0, 1)]


@pytest.fixture(scope="module")
def bare():
    with gpu_engines.bare(precision=HP) as e:                    # the entry needs no weights
        yield e


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("H,W", SHAPES)
def test_byte_for_byte_against_the_model(bare, H, W, S):
    q, b, v = case(H, W, S)
    seen = 0
    for lo, hi in RANGES:
        for w in WEIGHTS:
            for r in (1, 2, 4):
                for masked in (False, True):
                    eps = 1 if r == 1 else bm.default_eps(lo, hi)
                    want, bad = modelled(H, W, S, lo, hi, w, r, eps, masked, fill=77)
                    got, n = bare.carry_band_u16(b, S, sr=q, lo=lo, hi=hi, weights=w, r=r, eps=eps, valid=v if masked else None, fill=77)
                    what = f"{H} x {W} x{S} range {lo}..{hi} weights {w} r {r} eps {eps} masked {masked}"
                    same(got, want, what)
                    assert n == bad, what
                    seen += bad
    if H * W > 1:
        assert seen > 0                      # the clip path was taken: the band strays outside 1000..11000


def test_other_weights_and_the_gain_limit(bare):
    """weights whose sum is no power of two and is large (the guide's division), and a band so steep that A sits on the limit"""
    H, W, S = 37, 45, 4
    q, b, v = case(H, W, S)
    for w in ((77, 150, 29), (255, 255, 255), (1, 0, 2)):
        want, bad = bm.carry(q, b, S, 0, 65535, w=w, r=2, eps=3)
        got, n = bare.carry_band_u16(b, S, sr=q, weights=w, r=2, eps=3)
        same(got, want, f"weights {w}")
        assert n == bad
    steep, _ = bm.affine_band(q // 8, S, -6.0, 40000)
    want, bad, parts = bm.carry(q // 8, steep.astype(np.uint16), S, 0, 65535, r=1, eps=1, parts=True)
    assert (np.abs(parts["A"]) == bm.GAIN_LIMIT).any()
    got, n = bare.carry_band_u16(steep.astype(np.uint16), S, sr=q // 8, r=1, eps=1)
    same(got, want, "a gain beyond the limit")
    assert n == bad


@pytest.mark.parametrize("S", [2, 4])
def test_band_rows_do_not_change_a_byte(bare, S):
    H, W = 37, 45
    q, b, v = case(H, W, S)
    for masked in (False, True):
        want, bad = modelled(H, W, S, 1000, 11000, (1, 1, 1), 4, 5, masked)
        for rows in (0, S, 3 * S, 2 * S + 1, 1, S * H - 1):
            got, n = bare.carry_band_u16(b, S, sr=q, lo=1000, hi=11000, r=4, eps=5, valid=v if masked else None, band_rows=rows)
            same(got, want, f"band_rows {rows}, masked {masked}")
            assert n == bad


def test_kept_image_chain():
    """enhance_u16, two bands from the device copy, then the display pass on the same copy; an unrelated call in between voids it"""
    e = gpu_engines.default(1, HP)
    H, W = 37, 45
    rng = np.random.default_rng(3)
    img = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
    b1, b2 = bm.stray_band(bm.scene(H, W, 4, seed=1), 4, seed=2), rng.integers(0, 65536, (H, W)).astype(np.uint16)
    with e.chain_lock:
        q = np.array(e.enhance_u16(img, tile=16, pad=3))
        g1 = e.carry_band_u16(b1, 4, lo=1000, hi=11000)
        g2 = e.carry_band_u16(b2, 4, r=1, eps=9, band_rows=10)
        hist = e.display_hist_u16(None, shape=(4 * H, 4 * W))
        g3 = e.carry_band_u16(b1, 4, lo=1000, hi=11000)              # behind a display call too
    assert np.array_equal(hist, e.display_hist_u16(q))
    for got, (b, kw) in ((g1, (b1, dict(lo=1000, hi=11000))), (g2, (b2, dict(r=1, eps=9))), (g3, (b1, dict(lo=1000, hi=11000)))):
        want = e.carry_band_u16(b, 4, sr=q, **kw)
        same(got[0], want[0], "sr=None against the explicit image")
        assert got[1] == want[1]
        model = bm.carry(q, b, 4, kw.get("lo", 0), kw.get("hi", 65535), r=kw.get("r", 2), eps=kw.get("eps", 1))
        same(got[0], model[0], "sr=None against the model")
        assert got[1] == model[1]
    with e.chain_lock:
        e.enhance_u16(img, tile=16, pad=3)
        e.enhance_u8(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8))
        with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
            e.carry_band_u16(b1, 4)
        e.enhance_u16(img, tile=16, pad=3)
        with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
            e.carry_band_u16(b1[:-1], 4)                              # another size
        same(e.carry_band_u16(b1, 4)[0], bm.carry(q, b1, 4, 0, 65535)[0], "after a refusal the kept image still serves")


REFUSALS = [dict(S=3), dict(S=0), dict(r=0), dict(r=5), dict(eps=0), dict(lo=5, hi=5), dict(lo=-1), dict(hi=65536), dict(weights=(0, 0, 0)),
            dict(weights=(256, 0, 0)), dict(weights=(-1, 2, 0)), dict(fill=-1), dict(fill=65536), dict(band_rows=-1)]


def test_every_refusal_leaves_the_engine_answering(bare):
    H, W, S = 3, 70, 4
    q, b, v = case(H, W, S)
    want, bad = modelled(H, W, S, 0, 65535, (1, 1, 1), 2, 1, False)
    lib = native.load_library()
    for kw in REFUSALS:
        S_ = kw.get("S", S)
        args = dict(kw)
        args.pop("S", None)
        with pytest.raises(native.S2srError, match="invalid argument"):
            bare.carry_band_u16(b, S_, sr=None if S_ != S else q, **args)
        same(bare.carry_band_u16(b, S, sr=q)[0], want, f"after the refusal of {kw}")
    out, w3 = np.zeros((S * H, S * W), np.uint16), np.ones(3, np.int32)
    p = lambda a: a.ctypes.data
    for band, dst, wts, h, wd in ((None, p(out), p(w3), H, W), (p(b), None, p(w3), H, W), (p(b), p(out), None, H, W), (p(b), p(out), p(w3), 0, W),
                                  (p(b), p(out), p(w3), H, -1)):
        assert lib.s2sr_carry_band_u16(bare._h, p(q), band, h, wd, S, 0, 65535, wts, 2, 1, None, 0, 0, dst, None) == -1
    same(bare.carry_band_u16(b, S)[0], want, "the guide uploaded before the refusals is still the kept image")
    with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
        bare.carry_band_u16(b, 2)                                      # ... of S H x S W, and of no other size
    same(bare.carry_band_u16(b, S)[0], want, "after the refusal of sr=None")


@pytest.mark.parametrize("ident", doors.owned("carry_band_u16"))
def test_the_door_table_s_baseline_is_the_model(ident):
    """tests/doors.py's rows of this pass: the red-zone, poison, stall and grid-cap matrices hold every mode to diag.baseline, and
    this holds the baseline to the model, sample for sample"""
    same(diag.baseline(ident), doors.MODELS[ident](), ident)


def test_the_pass_has_a_kernel_family(bare):
    q, b, v = case(33, 17, 4)
    bare.set_profiling(1)
    try:
        bare.reset_kernel_stats()
        bare.carry_band_u16(b, 4, sr=q)
        bare.synchronize()
        st = bare.kernel_stats()
    finally:
        bare.set_profiling(0)
    assert st["bands"]["launches"] == 2 and st["bands"]["total_ms"] > 0, st["bands"]


# ---- the Python seam and the job ------------------------------------------------------------------------------------------------------
def _patch_weights(monkeypatch, tmp_path, nb_by_name):
    """Seeded synthetic checkpoints where the drop-in looks for them (tests/test_gpu_app.py)."""
    import torch

    from s2sr.weights import synthetic_state_dict
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir(exist_ok=True)
    for name, nb in nb_by_name.items():
        sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(nb, seed=0).items()}
        torch.save({"params_ema": sd}, tmp_path / "models" / f"{name}.pth")


def test_enhance16_and_the_wow_job_carry_the_fourth_band(monkeypatch, tmp_path):
    import json

    import app.cnn_super_resolution as m
    from app.wow_sr import process_wow_sr
    from s2sr import bands as xb
    from s2sr import rasterio_lite as rio
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    H, W = 40, 52
    rng = np.random.default_rng(52)
    four = rng.integers(100, 4000, size=(H, W, 4)).astype(np.uint16)
    four[..., 3] = (four[..., :3].sum(axis=2) // 5 + rng.integers(0, 300, (H, W))).astype(np.uint16)     # a band that follows the guide loosely
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)})
    e = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)
    stretch = dict(p_lo=2.0, p_hi=98.0)
    for nodata in (None, 0):
        tag = "plain" if nodata is None else "nodata"
        src4 = four.copy()
        if nodata is not None:
            src4[5:9, 7:30] = 0                                          # bands 1-3 (and 4) all nodata there
            src4[20, 20, :3] = 0
        bgr, nir = np.ascontiguousarray(src4[:, :, 2::-1]), src4[..., 3:4]
        valid = None if nodata is None else (src4[..., :3] != 0).any(axis=2).astype(np.uint8)
        lo, hi = (int(src4[..., :3].min()), int(src4[..., :3].max())) if valid is None else \
            (int(src4[..., :3][valid != 0].min()), int(src4[..., :3][valid != 0].max()))
        kw = {} if nodata is None else dict(nodata=0)
        # the operator: the door's bytes are what they were, the carried band is the model's on those bytes, the display pass still answers
        plain = np.array(e.enhance16(bgr, value_range=(lo, hi), **kw))
        out16, carried = e.enhance16(bgr, value_range=(lo, hi), extra=nir, **kw)
        out16 = np.array(out16)
        assert np.array_equal(out16, plain) and carried.shape == (4 * H, 4 * W, 1) and carried.dtype == np.uint16
        blo, bhi = xb.band_range(nir[..., 0], valid)
        eps = xb.default_eps(blo, bhi)
        want, bad = bm.carry(out16, nir[..., 0], 4, blo, bhi, eps=eps, valid=valid, fill=0)
        same(carried[..., 0], want, f"enhance16(extra=), {tag}")
        assert e.last_extra["inexact"] == [bad] and e.last_extra["ranges"] == [(blo, bhi)] and e.last_extra["eps"] == [eps]
        d_plain = e.enhance16(bgr, value_range=(lo, hi), display=stretch, **kw)
        d_extra = e.enhance16(bgr, value_range=(lo, hi), display=stretch, extra=nir, **kw)
        assert len(d_extra) == 4 and np.array_equal(d_extra[0], d_plain[0]) and np.array_equal(d_extra[1], d_plain[1]) and d_extra[2] == d_plain[2]
        same(d_extra[3][..., 0], want, f"enhance16(display=, extra=), {tag}")
        # the job
        src = tmp_path / f"scene4_{tag}.tif"
        rio.write_geotiff_u16(src, src4, geo, nodata=nodata)
        base = process_wow_sr(src, tmp_path / f"base_{tag}", enhance_crops=False, model="realesrgan_anime", bit_depth=16, **kw)
        res = process_wow_sr(src, tmp_path / f"four_{tag}", enhance_crops=False, model="realesrgan_anime", bit_depth=16, extra_bands="all", **kw)
        arr, g2 = rio.read_bands_raw(res["outputs"]["sr_tif"])
        rgb_only, _ = rio.read_bands_raw(base["outputs"]["sr_tif"])
        assert arr.shape == (4 * H, 4 * W, 4) and rgb_only.shape == (4 * H, 4 * W, 3)
        assert np.array_equal(arr[..., :3], rgb_only) and np.array_equal(rgb_only, out16[:, :, ::-1])
        same(arr[..., 3], want, f"band 4 of the job's file, {tag}")
        assert g2.pixel_size == (2.5, 2.5) and g2.nodata == nodata
        meta = res["sr_metadata"]
        assert meta["extra_bands"] == {"bands": [4], "ranges": [[blo, bhi]], "weights_rgb": [1, 1, 1], "r": 2, "eps": [eps], "gain_limit": 4,
                                       "inexact_blocks": [bad]}
        assert json.load(open(tmp_path / f"four_{tag}" / f"scene4_{tag}_wow_sr_metadata.json"))["sr_metadata"] == meta
        assert "extra_bands" not in base["sr_metadata"]
        strip = lambda d: {k: v for k, v in d.items() if k not in ("extra_bands", "output_file")}
        assert strip(meta) == strip(base["sr_metadata"])
        # without the option the job's file is, byte for byte, what the 3-band writer makes of the door's image
        rio.write_geotiff_rgb16(tmp_path / "direct.tif", np.ascontiguousarray(out16[:, :, ::-1]), geo.scaled(4), **({} if nodata is None else {"nodata": 0}))
        assert (tmp_path / "direct.tif").read_bytes() == open(base["outputs"]["sr_tif"], "rb").read()
    # guide weights in R, G, B terms reach the B, G, R image reversed
    res = process_wow_sr(src, tmp_path / "weighted", enhance_crops=False, model="realesrgan_anime", bit_depth=16, extra_bands=[4], extra_weights=(3, 2, 0), nodata=0)
    arr, _ = rio.read_bands_raw(res["outputs"]["sr_tif"])
    want, bad = bm.carry(out16, nir[..., 0], 4, blo, bhi, w=(0, 2, 3), eps=eps, valid=valid, fill=0)
    same(arr[..., 3], want, "weights (3, 2, 0) on R, G, B")
    assert res["sr_metadata"]["extra_bands"]["weights_rgb"] == [3, 2, 0]
