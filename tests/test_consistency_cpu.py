"""Radiometric consistency without a GPU: the numpy model's own properties (tests/consistency_model.py is what
tests/test_gpu_consistency.py holds the kernel to, byte for byte), the argument checks of s2sr/consistency.py, and the seam of
the app layers: the metadata block appears only with the option, an unknown mode on the routes is a 400."""
import json

import numpy as np
import pytest

import consistency_model as cm
from s2sr import consistency as sc
from s2sr import rasterio_lite as rio

SHAPES = [(1, 1), (3, 5), (17, 33), (40, 75)]
KINDS = [("uint8", 0, 255), ("uint16", 100, 4000)]
GEOREF = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)})


def recount(out, img, S, lo, hi):
    """The inexact blocks per channel, counted block by block with none of the model's helpers."""
    out = out.astype(np.int64)
    v = np.clip(img.astype(np.int64), lo, hi)
    bad = np.zeros(3, np.int64)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            for c in range(3):
                bad[c] += int(out[S * y:S * y + S, S * x:S * x + S, c].sum()) != S * S * int(v[y, x, c])
    return bad


@pytest.mark.parametrize("dtype,lo,hi", KINDS)
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("mode", [cm.EXACT, cm.SMOOTH])
def test_clip_free_input_comes_out_exact(mode, S, dtype, lo, hi):
    for H, W in SHAPES:
        sr, img = cm.clip_free_input(H, W, S, dtype=dtype, lo=lo, hi=hi)
        if dtype == "uint16" and H * W > 1:
            assert (img < lo).any() and (img > hi).any()                  # input values on both sides of the range
        out, bad = cm.consistency(sr, img, S, mode, lo, hi)
        assert out.dtype == sr.dtype and out.shape == sr.shape
        assert not bad.any(), (H, W, bad)
        want = S * S * np.clip(img.astype(np.int64), lo, hi)
        assert np.array_equal(cm.block_sums(out, S), want), (H, W)
        assert (out != sr).any()                                          # the case does correct something
        assert out.min() >= lo and out.max() <= hi


@pytest.mark.parametrize("dtype,lo,hi", KINDS)
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("mode", [cm.EXACT, cm.SMOOTH])
def test_saturating_input_counts_what_a_recount_gives(mode, S, dtype, lo, hi):
    H, W = 17, 33
    sr, img = cm.saturating_input(H, W, S, dtype=dtype, lo=lo, hi=hi)
    out, bad = cm.consistency(sr, img, S, mode, lo, hi)
    again = recount(out, img, S, lo, hi)
    print(f"{dtype} S {S} mode {mode}: inexact {bad.tolist()} of {H * W} blocks")
    assert np.array_equal(bad, again), (bad, again)
    assert 0 < bad.min() and bad.max() < H * W                            # the clip paths are taken, and not everywhere
    assert out.min() >= lo and out.max() <= hi


@pytest.mark.parametrize("S", [2, 4])
def test_exact_mode_leaves_an_exact_block_alone(S):
    sr, img = cm.clip_free_input(6, 7, S)
    once, _ = cm.consistency(sr, img, S, cm.EXACT)
    mixed = np.array(sr)
    mixed[:3 * S] = once[:3 * S]                                          # the upper block rows are exact already
    out, bad = cm.consistency(mixed, img, S, cm.EXACT)
    assert not bad.any()
    assert np.array_equal(out[:3 * S], mixed[:3 * S])
    assert np.array_equal(out[3 * S:], once[3 * S:])                      # (blocks do not see each other in this mode)
    assert np.array_equal(cm.consistency(once, img, S, cm.EXACT)[0], once)


def test_swap_compares_against_the_other_channel():
    sr, img = cm.clip_free_input(5, 6, 4)
    a, _ = cm.consistency(sr, img, 4, cm.SMOOTH, swap=True)
    b, _ = cm.consistency(sr[:, :, ::-1], img, 4, cm.SMOOTH)
    assert np.array_equal(a, b[:, :, ::-1])


def test_smooth_mode_moves_the_correction_off_the_block_grid():
    """A smooth radiometric bias: mode 2's correction steps less across block lines than mode 1's (the point of the mode)."""
    S, H, W = 4, 32, 32
    yy, xx = np.mgrid[0:H * S, 0:W * S]
    truth = 100 + 40 * np.sin(yy / 37.0) + 30 * np.cos(xx / 23.0)
    img = np.repeat(np.rint(truth.reshape(H, S, W, S).mean(axis=(1, 3)))[..., None], 3, axis=2).astype(np.uint8)
    sr = np.repeat(np.rint(truth + 12 * np.sin(yy / 50.0 + xx / 61.0))[..., None], 3, axis=2).astype(np.uint8)
    step = {}
    for mode in (cm.EXACT, cm.SMOOTH):
        out, bad = cm.consistency(sr, img, S, mode)
        assert not bad.any()
        corr = out.astype(np.int64) - sr
        step[mode] = float(np.abs(np.diff(corr, axis=1))[:, S - 1::S].mean())
    print(f"mean |step| of the correction across block lines: exact {step[cm.EXACT]:.3f}, smooth {step[cm.SMOOTH]:.3f}")
    assert step[cm.SMOOTH] < step[cm.EXACT]


def test_argument_checks():
    assert sc.mode_of(None) == 0 and sc.mode_of("exact") == sc.EXACT == 1 and sc.mode_of("smooth") == sc.SMOOTH == 2
    assert sc.NAMES == {1: "exact", 2: "smooth"}
    for bad in ("", "Exact", "both", 1, 2, True, 1.0, b"exact"):
        with pytest.raises(ValueError, match="consistency"):
            sc.mode_of(bad)
        with pytest.raises(ValueError, match="consistency"):
            sc.check_args(bad)
    assert sc.check_args(None) is None and sc.check_args("smooth") == "smooth"
    assert sc.metadata_block("exact", np.array([1, 2, 3], np.uint64)) == {"mode": "exact", "inexact_blocks": [1, 2, 3]}
    assert sc.metadata_block("smooth", [0, 0, 0], "post_process") == {"mode": "smooth", "inexact_blocks": [0, 0, 0], "applied_before": "post_process"}
    json.dumps(sc.metadata_block("exact", np.array([1, 2, 3], np.uint64)))


def _img():
    return np.random.default_rng(3).integers(1, 256, size=(12, 10, 3)).astype(np.uint8)


class FakeESRGAN:
    """Stands in for the GPU operator: what the job functions hand it, and a fixed count."""
    seen = []

    def __init__(self, scale=4, device=None, tile_size=256, model_name=None, **kw):
        self.scale, self.model_name, self.kw = scale, model_name, kw
        self.last_inexact_blocks = [1, 2, 3] if kw.get("consistency") else None
        FakeESRGAN.seen.append(kw)

    def enhance_job(self, img, post=None, **kw):
        return np.repeat(np.repeat(img, 4, axis=0), 4, axis=1)


@pytest.mark.parametrize("enhance_crops", [True, False])
def test_metadata_block_appears_only_with_the_option(tmp_path, monkeypatch, enhance_crops):
    from app import farm_sr, wow_sr
    monkeypatch.setattr(wow_sr, "RealESRGAN", FakeESRGAN)
    monkeypatch.setattr(farm_sr, "RealESRGAN", FakeESRGAN)
    src = tmp_path / "in.tif"
    rio.write_geotiff_rgb(src, _img(), GEOREF)
    FakeESRGAN.seen.clear()
    plain = wow_sr.process_wow_sr(src, tmp_path / "p", enhance_crops=enhance_crops)
    assert "consistency" not in plain["sr_metadata"] and FakeESRGAN.seen == [{}]        # a plain job's operator is built as it was
    got = wow_sr.process_wow_sr(src, tmp_path / "c", enhance_crops=enhance_crops, consistency="smooth")
    want = {"mode": "smooth", "inexact_blocks": [1, 2, 3]}
    if enhance_crops:
        want["applied_before"] = "post_process"
    assert got["sr_metadata"]["consistency"] == want and FakeESRGAN.seen[-1] == {"consistency": "smooth"}
    assert json.load(open(tmp_path / "c" / "in_wow_sr_metadata.json"))["sr_metadata"]["consistency"] == want
    assert [k for k in got["sr_metadata"] if k != "consistency"] == list(plain["sr_metadata"])
    if enhance_crops:
        farm = farm_sr.process_farm_sr(src, tmp_path / "fp")
        assert "consistency" not in farm["sr_metadata"]
        farm = farm_sr.process_farm_sr(src, tmp_path / "fc", consistency="exact")
        assert farm["sr_metadata"]["consistency"] == {"mode": "exact", "inexact_blocks": [1, 2, 3], "applied_before": "post_process"}


def test_job_functions_refuse_an_unknown_mode_before_anything_is_created(tmp_path):
    from app import farm_sr, wow_sr
    src = tmp_path / "in.tif"
    rio.write_geotiff_rgb(src, _img(), GEOREF)
    for fn in (wow_sr.process_wow_sr, farm_sr.process_farm_sr):
        out = tmp_path / fn.__name__
        with pytest.raises(ValueError, match="consistency"):
            fn(src, out, consistency="both")
        assert not out.exists() or not any(out.iterdir())


def test_routes_take_consistency_and_an_unknown_mode_is_a_400(tmp_path, monkeypatch):
    from fastapi.testclient import TestClient

    from app import farm_sr, wow_sr
    from app.sr_routes import create_app
    seen = {}

    def fake_wow(input_tif, output_dir, enhance_crops=True, model="realesrgan_x4", **kw):      # the job functions, without a GPU
        seen["wow"] = kw
        raise RuntimeError("stop here")

    def fake_farm(input_tif, output_dir, scale=4, **kw):
        seen["farm"] = kw
        raise RuntimeError("stop here")
    monkeypatch.setattr(wow_sr, "process_wow_sr", fake_wow)
    monkeypatch.setattr(farm_sr, "process_farm_sr", fake_farm)
    c = TestClient(create_app(tmp_path / "data"))
    f = tmp_path / "a.tif"
    rio.write_geotiff_rgb(f, _img(), GEOREF)
    for route in ("/api/wow", "/api/sr"):
        for bad in ("both", "", "EXACT"):
            r = c.post(route, json={"input_file": str(f), "consistency": bad})
            assert r.status_code == 400 and "consistency" in r.json()["detail"], (route, bad, r.status_code)
    assert not seen
    assert c.post("/api/wow", json={"input_file": str(f)}).status_code == 200
    assert c.post("/api/sr", json={"input_file": str(f)}).status_code == 200
    assert "consistency" not in seen["wow"] and "consistency" not in seen["farm"]            # a plain job's call is what it was
    assert c.post("/api/wow", json={"input_file": str(f), "consistency": "smooth"}).status_code == 200
    assert c.post("/api/sr", json={"input_file": str(f), "consistency": "exact"}).status_code == 200
    assert seen["wow"]["consistency"] == "smooth" and seen["farm"]["consistency"] == "exact"
