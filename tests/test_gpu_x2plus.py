"""RealESRGAN_x2plus (s2sr_config.scale 2) on the MI355X: pixel_unshuffle folded into the input packers, a 12-channel conv_first,
the x4 body and tail on the half grid.  Checked against the reference's goldens (tests/golden/g9_x2plus.npz), against the CPU model
tests/x2plus_model.py (ragged and odd sizes: the mod-2 reflect rule), in situ at the head (s2sr_debug_forward_taps), by byte
identities across the run-time switches, and by the schedule it launches (the x4 schedule of the half-size tiles)."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import gpu_engines
import tail_model as tm
import x2plus_model as xm
from oracle import postprocess_ref as pp
from oracle import rrdbnet_ref as ref
from s2sr import native
from s2sr import rasterio_lite as rio
from s2sr.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

TOL_F16 = 2.5e-3
TOL_HP = 3e-4
TOL_FP8_23 = 1e-2
HP, FAST, FP8 = native.PREC_F16_HP, native.PREC_F16, native.PREC_FP8


def _sd(nb):
    return synthetic_state_dict(nb, seed=0, scale=2)


def _tsd(nb):
    return ref.to_torch_sd(_sd(nb))


def engine(nb, precision=HP):
    """Cached default-configuration scale-2 engines (created with every S2SR_* switch cleared)."""
    return gpu_engines.default(nb, precision, scale=2)


def _fresh(monkeypatch, nb, precision, env, **kw):
    """s2sr_create reads every switch once: a test of a switch creates its own handle after setting it."""
    return gpu_engines.fresh(monkeypatch, env, nb, precision, scale=2, **kw)


def _u8_close(a, b, frac=0.99):
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return d.max() <= 1 and (d == 0).mean() >= frac


def _img(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------
def test_g9_nets(golden_dir):
    g = np.load(golden_dir / "g9_x2plus.npz")
    for nb in (1, 2, 23):
        for prec, tol in ((FAST, TOL_F16), (HP, TOL_HP)):
            y = engine(nb, prec).forward_f32(g["net_x"])
            assert y.shape == (2, 3, 48, 64)
            err = float(np.abs(y - g[f"net_b{nb}"]).max())
            assert err <= tol, (nb, prec, err)
    # the u8 entry against the f32 entry on the same integers
    e = engine(2, HP)
    o8 = e.forward_batch_u8(g["net_u8"])
    of = e.forward_f32(g["net_x"])
    q = (of.transpose(0, 2, 3, 1) * 255.0).clip(0, 255).astype(np.uint8)
    assert o8.shape == (2, 48, 64, 3) and _u8_close(o8, q)


# ---- 2. whole-image enhance -------------------------------------------------------------------------------------------------
def test_g9_enhance_whole_image(golden_dir):
    g = np.load(golden_dir / "g9_x2plus.npz")
    e = engine(23, HP)
    f = e.enhance_f32(g["enh_img"])
    assert f.shape == (80, 112, 3) and np.abs(f - g["enh_f32"]).max() <= TOL_HP
    assert _u8_close(e.enhance_u8(g["enh_img"]), g["enh_u8"])


# ---- 3. tiled enhance --------------------------------------------------------------------------------------------------------
def test_g9_tiled_small(golden_dir):
    g = np.load(golden_dir / "g9_x2plus.npz")
    f = engine(1, HP).tile_process_f32(g["tiled_img"], tile=16, pad=2)
    assert f.shape == (76, 92, 3)
    assert np.abs(f - g["tiled_f32"][0].transpose(1, 2, 0)).max() <= TOL_HP


@pytest.mark.parametrize("hw,tile", [((530, 601), 256), ((277, 514), 256), ((277, 514), 128), ((2, 3), 256), ((45, 38), 16)])
def test_enhance_ragged_and_odd_vs_model(hw, tile):
    """Tiled and whole-image branches on odd sizes: the reflect row / column comes from the packer (whole image) or the window
    gather (tiled), the crop from the stitch maps."""
    nb = 6
    e = engine(nb, HP)
    img = _img(hw[0] * 7 + hw[1], *hw)
    pad = 2 if tile == 16 else 10
    f = e.enhance_f32(img, tile=tile, pad=pad)
    exp = xm.enhance_float(img, _tsd(nb), nb, tile, pad)
    assert f.shape == (2 * hw[0], 2 * hw[1], 3) == exp.shape
    assert np.abs(f - exp).max() <= TOL_HP, hw
    u8 = e.enhance_u8(img, tile=tile, pad=pad)
    assert _u8_close(u8, (exp * 255.0).clip(0, 255).astype(np.uint8)), hw


# ---- 4. the head in situ ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [HP, FAST])
@pytest.mark.parametrize("B,th,tw", [(1, 24, 32), (5, 40, 44)])
def test_head_in_situ(prec, B, th, tw):
    e = engine(1, prec)
    tiles = np.random.default_rng(B * 100 + th).integers(0, 256, (B, th, tw, 3), dtype=np.uint8)
    geo, taps, of32, ou8 = e.debug_forward_taps(tiles=tiles)
    assert ou8.shape == (B, 2 * th, 2 * tw, 3) and of32.shape == (B, 3, 2 * th, 2 * tw)
    if B > 1:
        assert geo["mos_kx"] * geo["mos_ky"] >= 2 and (geo["mos_wh"], geo["mos_ww"]) == (th // 2, tw // 2)
    p0 = xm.expected_p0(tiles, geo)
    bad = taps["P0"] != p0
    assert not bad.any(), f"P0: {int(bad.sum())} elements differ (first at {np.argwhere(bad)[0].tolist()})"
    sd = _sd(1)
    s = tm.split(sd["conv_first.weight"])
    L = tm.Layer(tm.conv3, 9 * (2 if prec == HP else 1))
    L.add(p0[:, :12], s["hi"])
    if prec == HP:
        L.add(p0[:, :12], s["lo16"], True)
    m, _, tol = L.result(sd["conv_first.bias"], scale=1.0 / 255.0)
    live = np.zeros((geo["n"], 1) + m.shape[2:], bool)             # the live trunk pixels of every window
    kx, ky = (geo["mos_kx"], geo["mos_ky"]) if geo["mos_kx"] else (1, 1)
    h, w = th // 2, tw // 2
    for t in range(B):
        i, slot = divmod(t, kx * ky)
        wy, wx = divmod(slot, kx)
        live[i, 0, wy * (h + 1):wy * (h + 1) + h, wx * (w + 1):wx * (w + 1) + w] = True
    Fg = taps["F"][:, :, 1:-1, 1:-1].astype(np.float64)
    ratio = np.abs(m - Fg) / tol
    L4 = np.broadcast_to(live, m.shape)
    assert (ratio[L4] <= 1).all(), f"conv_first: F off the model by {float(ratio[L4].max()):.3g} x tol"


# ---- 5. byte identities ------------------------------------------------------------------------------------------------------
def test_mosaic_groups_graphs_and_batches_give_the_same_bytes(monkeypatch):
    tiles = np.random.default_rng(5).integers(0, 256, (7, 60, 84, 3), dtype=np.uint8)
    base = _fresh(monkeypatch, 2, HP, {})
    ref8 = base.forward_batch_u8(tiles).copy()
    for _ in range(2):                                              # second sighting captures, third replays
        assert np.array_equal(base.forward_batch_u8(tiles), ref8)
    assert base.graph_stats()[1] >= 1
    variants = {"no mosaic": _fresh(monkeypatch, 2, HP, {"S2SR_MOSAIC": "0"}),
                "no graphs": _fresh(monkeypatch, 2, HP, {"S2SR_GRAPH": "0"}),
                "group 2": _fresh(monkeypatch, 2, HP, {}, group=2)}
    for name, e in variants.items():
        for _ in range(3):
            assert np.array_equal(e.forward_batch_u8(tiles), ref8), name
        e.close()
    singles = np.concatenate([base.forward_batch_u8(tiles[i:i + 1]) for i in range(len(tiles))])
    assert np.array_equal(singles, ref8)
    base.close()


@pytest.mark.parametrize("hw,tile", [((39, 57), 256), ((301, 433), 128)])
def test_odd_enhance_equals_padded_enhance_cropped(hw, tile):
    e = engine(2, HP)
    img = _img(11, *hw)
    padded = np.pad(img, ((0, hw[0] % 2), (0, hw[1] % 2), (0, 0)), mode="reflect")
    out = e.enhance_u8(img, tile=tile)
    exp = e.enhance_u8(padded, tile=tile)[:2 * hw[0], :2 * hw[1]]
    assert np.array_equal(out, exp)
    f = e.enhance_f32(img, tile=tile)
    assert np.array_equal(f, e.enhance_f32(padded, tile=tile)[:2 * hw[0], :2 * hw[1]])


@pytest.mark.parametrize("hw,tile", [((40, 56), 256), ((301, 433), 64)])
def test_enhance_job_equals_enhance_plus_postprocess(hw, tile):
    e = engine(2, HP)
    rgb = _img(13, *hw)
    exp_sr = np.ascontiguousarray(e.enhance_u8(np.ascontiguousarray(rgb[:, :, ::-1]), tile=tile)[:, :, ::-1])
    assert np.array_equal(e.enhance_job_u8(rgb, None, tile=tile), exp_sr)
    assert np.array_equal(e.enhance_job_u8(rgb, native.pp_wow(), tile=tile), e.postprocess_u8(exp_sr, native.pp_wow()))


# ---- 6. the schedule ------------------------------------------------------------------------------------------------------------
def test_schedule_is_the_x4_schedule_of_half_size_tiles():
    """One step of 32 x 512^2 at scale 2 launches what one step of 32 x 256^2 at scale 4 launches: same families, same counts."""
    stats = {}
    for scale, size in ((2, 512), (4, 256)):
        e = native.Engine(num_block=23, precision=HP, scale=scale)
        e.load_state_dict(synthetic_state_dict(23, seed=0, scale=scale))
        tiles = np.random.default_rng(1).integers(0, 256, (32, size, size, 3), dtype=np.uint8)
        e.set_profiling(1)
        e.reset_kernel_stats()
        out = e.forward_batch_u8(tiles)
        assert out.shape == (32, 1024, 1024, 3)
        stats[scale] = {k: v["launches"] for k, v in e.kernel_stats().items() if v["launches"]}
        e.close()
    assert stats[2] == stats[4], stats


# ---- 7. fp8 ------------------------------------------------------------------------------------------------------------------------
def test_fp8_calibrated_scale2(golden_dir):
    g = np.load(golden_dir / "g9_x2plus.npz")
    e = native.Engine(num_block=23, precision=FP8, scale=2)
    e.load_state_dict(_sd(23))
    from s2sr.synth import synthetic_tiles
    e.calibrate_fp8(synthetic_tiles(4, 64, seed=0), headroom=2.0)
    y = e.forward_f32(g["net_x"])
    assert np.isfinite(y).all() and np.abs(y - g["net_b23"]).max() <= TOL_FP8_23
    e.close()


# ---- 8. the drop-in ------------------------------------------------------------------------------------------------------------------
def test_app_x2plus(monkeypatch, tmp_path):
    import app.cnn_super_resolution as m
    from app.wow_sr import process_wow_sr
    sd = {k: torch.from_numpy(v) for k, v in _sd(23).items()}
    e = m.RealESRGAN(model_name="realesrgan_x2plus", state_dict=sd)
    assert e.scale == 2 and e.model_name == "realesrgan_x2plus" and e._engine.scale == 2
    img = _img(17, 40, 56)
    out = e.enhance(img)
    assert out.shape == (80, 112, 3) and _u8_close(out, xm.enhance(img, _tsd(23), 23))
    t = e._tile_process(torch.from_numpy(img.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0))
    assert tuple(t.shape) == (1, 3, 80, 112)
    assert e.enhance_job(img).shape == (80, 112, 3)
    with pytest.raises(ValueError, match="Unknown model"):
        m.RealESRGAN(scale=2)
    # process_wow_sr end to end on a GeoTIFF: the checkpoint where the drop-in looks for it
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir()
    sd6 = {k: torch.from_numpy(v) for k, v in _sd(6).items()}
    monkeypatch.setitem(m.EXTRA_MODELS, "realesrgan_x2plus", {**m.EXTRA_MODELS["realesrgan_x2plus"], "blocks": 6})
    torch.save({"params_ema": sd6}, tmp_path / "models" / "realesrgan_x2plus.pth")
    rgb = _img(19, 25, 33)
    src = tmp_path / "scene.tif"
    rio.write_geotiff_rgb(src, rgb, rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)}))
    res = process_wow_sr(src, tmp_path / "wow", enhance_crops=True, model="realesrgan_x2plus")
    meta = res["sr_metadata"]
    assert meta["scale"] == 2 and meta["effective_resolution_m"] == 5.0 and meta["output_size"] == [50, 66]
    assert meta["stages"][0] == {"model": "realesrgan_x2plus", "scale": 2, "purpose": "GAN upscaling"}
    out, g2 = rio.read_rgb_u8(res["outputs"]["sr_tif"])
    assert out.shape == (50, 66, 3) and g2.pixel_size == (5.0, 5.0)
    assert json.load(open(tmp_path / "wow" / "scene_wow_sr_metadata.json"))["sr_metadata"] == meta
    res2 = process_wow_sr(src, tmp_path / "wow2", enhance_crops=False, model="realesrgan_x2plus")
    sr_plain, _ = rio.read_rgb_u8(res2["outputs"]["sr_tif"])
    assert np.array_equal(pp.enhance_for_crops(sr_plain), out)
    exp_sr = xm.enhance(np.ascontiguousarray(rgb[:, :, ::-1]), _tsd(6), 6)[:, :, ::-1]
    assert np.abs(sr_plain.astype(np.int16) - exp_sr.astype(np.int16)).max() <= 1


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------
def test_scale2_errors():
    e = engine(1, HP)
    with pytest.raises(native.S2srError, match="even tile sizes"):
        e.forward_batch_u8(np.zeros((1, 24, 33, 3), np.uint8))
    with pytest.raises(native.S2srError, match="even tile sizes"):
        e.forward_f32(np.zeros((1, 3, 25, 32), np.float32))
    with pytest.raises(native.S2srError, match="even tile"):
        e.enhance_u8(np.zeros((40, 40, 3), np.uint8), tile=15)
    with pytest.raises(native.S2srError, match="bad weight blob"):
        e.load_blob(np.zeros(native.load_library().s2sr_expected_blob_floats(1), np.float32))
    e.load_state_dict(_sd(1))                                        # the handle still works
    with pytest.raises(native.S2srError, match="scale-4 handles only"):
        e.debug_trunk_taps(0, 1, tiles=np.zeros((1, 24, 32, 3), np.uint8))
    with pytest.raises(native.S2srError, match="unsupported net shape"):
        native.Engine(num_block=1, scale=3)
    with pytest.raises(ValueError, match="conv_first"):
        e.load_state_dict(synthetic_state_dict(1, seed=0))           # an x4 state dict into a scale-2 engine
