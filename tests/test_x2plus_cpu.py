"""RealESRGAN_x2plus (scale 2) without a GPU: the CPU model against the reference's goldens, the x2plus weights and blob layout,
the scale-2 window plan, the drop-in's model tables and the multi-GPU refusal."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest
import torch

import x2plus_model as xm
from oracle import rrdbnet_ref as ref
from s2sr import native
from s2sr.weights import conv_specs, flatten_state_dict, num_params, synthetic_state_dict


def _tsd(nb):
    return ref.to_torch_sd(synthetic_state_dict(nb, seed=0, scale=2))


def test_x2plus_model_reproduces_g9(golden_dir):
    g = np.load(golden_dir / "g9_x2plus.npz")
    x = torch.from_numpy(g["net_x"])
    with torch.no_grad():
        for nb in (1, 2, 23):
            y = xm.forward(x, _tsd(nb), nb).numpy()
            assert y.shape == (2, 3, 48, 64)
            assert np.abs(y - g[f"net_b{nb}"]).max() <= 1e-5, nb
    img = g["enh_img"]
    f = xm.enhance_float(img, _tsd(23), 23)
    assert np.abs(f - g["enh_f32"]).max() <= 1e-5
    assert np.array_equal(xm.enhance(img, _tsd(23), 23), g["enh_u8"])
    t = xm.enhance_float(g["tiled_img"], _tsd(1), 1, tile_size=16, tile_pad=2, force_tiled=True)
    assert np.abs(t - g["tiled_f32"][0].transpose(1, 2, 0)).max() <= 1e-5


def test_x2plus_reflect_rule_is_the_padded_image_cropped():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(7, 9, 3), dtype=np.uint8)
    padded = np.pad(img, ((0, 1), (0, 1), (0, 0)), mode="reflect")
    assert np.array_equal(padded[7, :9], img[5]) and np.array_equal(padded[:, 9], padded[:, 7])
    sd = _tsd(1)
    a = xm.enhance_float(img, sd, 1)
    b = xm.enhance_float(padded, sd, 1)[:14, :18]
    assert a.shape == (14, 18, 3) and np.array_equal(a, b)


def test_synthetic_x2plus_weights():
    sd = synthetic_state_dict(2, seed=0, scale=2)
    assert sd["conv_first.weight"].shape == (64, 12, 3, 3)
    assert list(sd) == list(synthetic_state_dict(2, seed=0))          # the x4plus keys
    for k, v in synthetic_state_dict(2, seed=0).items():
        if k != "conv_first.weight":
            assert sd[k].shape == v.shape, k
    again = synthetic_state_dict(2, seed=0, scale=2)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
    assert sum(v.size for v in sd.values()) == num_params(2, scale=2) == num_params(2) + 9 * 64 * 9
    with pytest.raises(ValueError):
        synthetic_state_dict(1, scale=3)


def test_x4_weight_stream_unchanged(golden_dir):
    g = np.load(golden_dir / "g7_weightgen.npz")
    for seed in (0, 1):
        h = hashlib.sha256()
        for k, v in synthetic_state_dict(23, seed=seed, scale=4).items():
            h.update(k.encode())
            h.update(v.tobytes())
        assert np.array_equal(np.frombuffer(h.digest(), dtype=np.uint8), g[f"seed{seed}_sha256"])


def test_flatten_x2plus_and_blob_sizes():
    lib = native.load_library()
    assert lib.s2sr_expected_blob_floats_scale(23, 2) == 16_703_171
    assert lib.s2sr_expected_blob_floats_scale(23, 4) == 16_697_987 == lib.s2sr_expected_blob_floats(23)
    assert lib.s2sr_expected_blob_floats_scale(23, 2) - lib.s2sr_expected_blob_floats_scale(23, 4) == 9 * 64 * 9
    assert lib.s2sr_expected_blob_floats_scale(23, 3) == 0
    sd = synthetic_state_dict(2, seed=0, scale=2)
    blob = flatten_state_dict(sd)                                      # scale from conv_first's shape
    assert blob.size == lib.s2sr_expected_blob_floats_scale(2, 2)
    assert np.array_equal(blob[:64 * 12 * 9], sd["conv_first.weight"].ravel())
    assert np.array_equal(flatten_state_dict(sd, 2, scale=2), blob)
    with pytest.raises(ValueError, match="conv_first"):
        flatten_state_dict(sd, 2, scale=4)
    with pytest.raises(ValueError, match="conv_first"):
        flatten_state_dict(synthetic_state_dict(2, seed=0), 2, scale=2)
    assert conv_specs(1, num_in_ch=12)[0] == ("conv_first", 12, 64, False)


@pytest.mark.parametrize("hw,tile,pad", [((38, 46), 16, 2), ((530, 602), 256, 10), ((278, 514), 128, 10), ((1024, 600), 256, 7)])
def test_plan_tiles_scale2_matches_reference_plan(hw, tile, pad):
    h, w = hw
    wins = native.plan_tiles(h, w, tile, pad, 2)
    plan = ref.tile_plan(h, w, tile, pad, scale=2)
    assert len(wins) == len(plan)
    for q, (r, c, o) in zip(wins, plan):
        assert (q.y1, q.y2, q.x1, q.x2) == r
        assert (q.crop_top, q.crop_bottom, q.crop_left, q.crop_right) == c
        assert (q.oy1, q.oy2, q.ox1, q.ox2) == o
        assert all(v % 2 == 0 for v in r)                              # even tile, even image: even windows


def test_app_tables_resolve_x2plus(tmp_path, monkeypatch):
    import app.cnn_super_resolution as m
    assert set(m.MODELS) == {"realesrgan_x4", "realesrgan_anime"}
    assert "realesrgan_x2plus" not in m.MODELS and "realesrgan_x2" not in m.EXTRA_MODELS
    cfg = m.model_config("realesrgan_x2plus")
    assert cfg["scale"] == 2 and cfg["blocks"] == 23 and cfg["channels"] == 64
    assert cfg["url"].endswith("/RealESRGAN_x2plus.pth")
    assert m.model_config("realesrgan_x2") is None
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path))
    monkeypatch.delenv("S2SR_ALLOW_DOWNLOAD", raising=False)
    with pytest.raises(FileNotFoundError, match="RealESRGAN_x2plus.pth"):
        m.download_weights("realesrgan_x2plus")                       # never reaches the network
    with pytest.raises(ValueError, match="Unknown model"):
        m.download_weights("realesrgan_x2")


def test_shell_loads_x2plus_strictly_and_rejects_x4():
    import app.cnn_super_resolution as m
    net = m.RRDBNet(num_in_ch=12, num_block=2)
    assert net.scale == 2
    sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(2, seed=0, scale=2).items()}
    net.load_state_dict(sd, strict=True)
    assert tuple(net.conv_first.weight.shape) == (64, 12, 3, 3)
    with pytest.raises(RuntimeError, match="conv_first"):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(2, seed=0).items()}, strict=True)
    with pytest.raises(RuntimeError, match="conv_first"):
        m.RRDBNet(num_block=2).load_state_dict(sd, strict=True)
    with pytest.raises(ValueError):
        m.RRDBNet(num_block=2, scale=2)                               # the reference's one-upsample branch stays refused


def test_distributed_refuses_scale2():
    from s2sr import dist as sd

    class X2(sd.BackendBase):
        scale = 2

    with pytest.raises(ValueError, match="scale-4"):
        sd.enhance_distributed(X2(), np.zeros((64, 64, 3), np.uint8))
