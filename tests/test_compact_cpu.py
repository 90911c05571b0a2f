"""CPU checks of the SRVGGNetCompact support (realesr-general-x4v3, -wdn-x4v3, realesr-animevideov3): the weight layout and blob,
deep network interpolation, the CPU checker (tests/compact_model.py) against tests/golden/g10_compact.npz, the choice of the
golden's seeded weights, and the app's model names.  No GPU."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import compact_model as cm
from s2sr import native
from s2sr import weights as W


def _torch_module(num_conv):
    body = nn.ModuleList([nn.Conv2d(3, 64, 3, 1, 1), nn.PReLU(num_parameters=64)])
    for _ in range(num_conv):
        body.append(nn.Conv2d(64, 64, 3, 1, 1))
        body.append(nn.PReLU(num_parameters=64))
    body.append(nn.Conv2d(64, 48, 3, 1, 1))
    m = nn.Module()
    m.body = body
    return m


# ---- layout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_conv", [16, 32])
def test_compact_specs_equal_a_torch_module(num_conv):
    m = _torch_module(num_conv)
    tsd = m.state_dict()
    specs = W.compact_specs(num_conv)
    assert [k for k, _ in specs] == list(tsd.keys())
    assert [tuple(s) for _, s in specs] == [tuple(v.shape) for v in tsd.values()]
    assert W.num_params_compact(num_conv) == sum(v.numel() for v in tsd.values())
    sd = W.synthetic_compact_state_dict(num_conv, seed=3)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)          # ours into torch's
    back = {k: v.numpy() for k, v in m.state_dict().items()}
    assert W.flatten_state_dict(back).tobytes() == W.flatten_state_dict(sd).tobytes()         # torch's into ours


def test_num_params_and_library_blob_length():
    assert W.num_params_compact(32) == 1_213_296
    assert native.expected_blob_floats_cfg(32, 4, "compact") == 1_213_296
    assert native.expected_blob_floats_cfg(16, 4, "compact") == W.num_params_compact(16)
    assert native.expected_blob_floats_cfg(7, 4, "compact") == 0        # a config s2sr_create refuses
    assert native.expected_blob_floats_cfg(32, 2, "compact") == 0
    assert native.expected_blob_floats_cfg(23, 4, "rrdb") == W.num_params(23)
    assert native.expected_blob_floats_cfg(23, 2, "rrdb") == W.num_params(23, scale=2)


def test_infer_arch():
    assert W.infer_arch(W.synthetic_state_dict(6).keys()) == ("rrdb", 6)
    assert W.infer_arch(W.synthetic_state_dict(2, scale=2).keys()) == ("rrdb", 2)
    assert W.infer_arch(W.synthetic_compact_state_dict(32).keys()) == ("compact", 32)
    assert W.infer_arch(W.synthetic_compact_state_dict(16).keys()) == ("compact", 16)
    assert W.MODEL_TABLE["realesr_general_x4v3"]["arch"] == "compact" and W.MODEL_TABLE["realesr_general_x4v3"]["num_conv"] == 32
    assert W.MODEL_TABLE["realesr_general_wdn_x4v3"]["num_conv"] == 32 and W.MODEL_TABLE["realesr_animevideov3"]["num_conv"] == 16
    assert all(W.MODEL_TABLE[k]["scale"] == 4 for k in ("realesr_general_x4v3", "realesr_general_wdn_x4v3", "realesr_animevideov3"))


def test_flatten_order_and_length():
    sd = W.synthetic_compact_state_dict(16, seed=1)
    blob = W.flatten_state_dict(sd)
    assert blob.dtype == np.float32 and blob.size == W.num_params_compact(16)
    assert blob.tobytes() == np.concatenate([sd[k].ravel() for k, _ in W.compact_specs(16)]).tobytes()
    assert W.flatten_state_dict(sd, 16, arch="compact").tobytes() == blob.tobytes()
    bad = dict(sd)
    del bad["body.3.weight"]
    with pytest.raises((KeyError, ValueError)):
        W.flatten_state_dict(bad)
    bad = dict(sd)
    bad["body.34.weight"] = np.zeros((3, 64, 3, 3), np.float32)
    with pytest.raises(ValueError):
        W.flatten_state_dict(bad)
    with pytest.raises(KeyError):
        W.flatten_state_dict(sd, 32, arch="compact")


def test_rrdb_blobs_unchanged(golden_dir):
    """The RRDB side of flatten_state_dict / synthetic_state_dict is what it was: the seeded tensors hash to the digests pinned
    in g7_weightgen.npz, and the blob is those tensors in conv_specs order (weight, bias), for both scales, whether the arch is
    inferred or named."""
    g = np.load(golden_dir / "g7_weightgen.npz")
    for seed in (0, 1):
        sd = W.synthetic_state_dict(23, seed=seed)
        h = hashlib.sha256()
        for k, v in sd.items():
            h.update(k.encode())
            h.update(v.tobytes())
        assert np.array_equal(np.frombuffer(h.digest(), dtype=np.uint8), g[f"seed{seed}_sha256"])
        blob = W.flatten_state_dict(sd)
        assert blob.tobytes() == b"".join(v.tobytes() for v in sd.values())     # state-dict order IS conv_specs order
        assert blob.size == int(g[f"seed{seed}_nparams"])
    for nb, scale in ((1, 4), (6, 4), (2, 2)):
        sd = W.synthetic_state_dict(nb, seed=0, scale=scale)
        blob = W.flatten_state_dict(sd)
        parts = []
        for name, _, _, _ in W.conv_specs(nb, num_in_ch=W.first_conv_cin(scale)):
            parts += [sd[name + ".weight"].ravel(), sd[name + ".bias"].ravel()]
        assert blob.tobytes() == np.concatenate(parts).tobytes()
        assert blob.size == W.num_params(nb, scale)
        assert W.flatten_state_dict(sd, nb, scale=scale).tobytes() == blob.tobytes()
        assert W.flatten_state_dict(sd, nb, scale=scale, arch="rrdb").tobytes() == blob.tobytes()


# ---- dni ----------------------------------------------------------------------------------------------------------
def test_dni():
    a = W.synthetic_compact_state_dict(16, seed=1)
    b = W.synthetic_compact_state_dict(16, seed=2)
    one, zero, half = W.dni(a, b, 1.0), W.dni(a, b, 0.0), W.dni(a, b, 0.5)
    assert list(one.keys()) == list(a.keys())
    for k in a:
        assert one[k].tobytes() == a[k].tobytes() and zero[k].tobytes() == b[k].tobytes()
        assert half[k].dtype == np.float32
        assert half[k].tobytes() == (np.float32(0.5) * a[k] + np.float32(0.5) * b[k]).astype(np.float32).tobytes()
    q = W.dni(a, b, 0.25)
    assert np.allclose(q["body.2.weight"], 0.25 * a["body.2.weight"].astype(np.float64) + 0.75 * b["body.2.weight"], atol=1e-7)
    ta = {k: torch.from_numpy(v) for k, v in a.items()}
    assert W.dni(ta, b, 0.5)["body.0.bias"].tobytes() == half["body.0.bias"].tobytes()
    for s in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            W.dni(a, b, s)
    c = dict(b)
    del c["body.1.weight"]
    with pytest.raises(ValueError):
        W.dni(a, c, 0.5)


# ---- checker against the golden ------------------------------------------------------------------------------------
def test_golden_weight_checksums(golden_dir):
    g = np.load(golden_dir / "g10_compact.npz")
    for nc in (16, 32):
        blob = W.flatten_state_dict(W.synthetic_compact_state_dict(nc, seed=0))
        assert hashlib.sha256(blob.tobytes()).hexdigest() == str(g[f"blob_sha256_c{nc}"])


def _u8_equal_up_to_boundary(f, want_u8):
    """u8 of the float image equals the golden's except where the float lands within 1e-6 of an integer level."""
    d = cm.quantise(f).astype(int) - want_u8.astype(int)
    frac = np.abs(f * 255.0 - np.rint(f * 255.0))
    return bool(np.all((d == 0) | ((np.abs(d) == 1) & (frac < 255e-6))) and (d != 0).mean() < 1e-3)


def test_checker_against_golden(golden_dir):
    g = np.load(golden_dir / "g10_compact.npz")
    x = torch.from_numpy(g["net_u8"]).permute(0, 3, 1, 2).double() / 255.0
    for nc in (16, 32):
        sd = W.synthetic_compact_state_dict(nc, seed=0)
        err = float(np.abs(cm.forward(x, sd).numpy() - g[f"net_c{nc}"]).max())
        print(f"num_conv {nc}: checker vs golden max-abs {err:.3g}")
        assert err <= 1e-6
        e32 = float(np.abs(cm.forward(torch.from_numpy(g["net_x"]), sd, torch.float32).numpy() - g[f"net_c{nc}"]).max())
        assert e32 <= 2e-5      # the float32 form of the checker (fp32 rounding over num_conv + 2 layers)
    sd32, sd16 = W.synthetic_compact_state_dict(32, seed=0), W.synthetic_compact_state_dict(16, seed=0)
    assert _u8_equal_up_to_boundary(cm.enhance_float(g["enh_img"], sd32), g["enh_u8"])      # enhance, whole-image branch
    # _tile_process and enhance's tiled branch (22 * 26 > 8 * 8 * 4)
    t = cm.enhance_float(g["tiled_img"], sd16, 8, 2, force_tiled=True)
    assert float(np.abs(t.transpose(2, 0, 1)[None] - g["tiled_f32"]).max()) <= 1e-6
    t2 = cm.enhance_float(g["tiled_img"], sd16, 8, 2)
    assert np.array_equal(t, t2)
    assert _u8_equal_up_to_boundary(t2, g["tiled_enh_u8"])


def test_tile_plan_exact():
    """The checker's tiled path pastes every output pixel per the reference's plan (later windows overwrite): with an identity
    'net' (nearest x4) the stitched image equals nearest x4 of the input, exactly."""
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.random((1, 3, 37, 45)))
    near = lambda t: F.interpolate(t, scale_factor=4, mode="nearest")
    out = cm.tile_process(x, None, 16, 2, fwd=near)
    assert torch.equal(out, near(x))


def test_pixel_shuffle_channel_order():
    """One channel of the last conv set to a delta: exactly one HR sub-pixel of one colour moves -- channel c*16 + dy*4 + dx
    goes to colour c of HR pixel (4y + dy, 4x + dx)."""
    sd = W.synthetic_compact_state_dict(16, seed=0)
    last = "body.34"
    sd = {k: (np.zeros_like(v) if k.startswith(last) else v) for k, v in sd.items()}
    x = torch.zeros((1, 3, 5, 6), dtype=torch.float64)
    base = cm.forward(x, sd).numpy()
    assert np.all(base == 0)
    for ch in (0, 5, 17, 30, 47):
        b = np.zeros(48, np.float32)
        b[ch] = 1.0
        sd[last + ".bias"] = b
        out = cm.forward(x, sd).numpy()[0]
        c, dy, dx = ch // 16, (ch % 16) // 4, ch % 4
        exp = np.zeros_like(out)
        exp[c, dy::4, dx::4] = 1.0
        assert np.array_equal(out, exp), ch


# ---- the golden is well chosen ---------------------------------------------------------------------------------------
def _nearest(img_u8):
    return np.repeat(np.repeat(img_u8.astype(np.float64) / 255.0, 4, axis=0), 4, axis=1)


def test_golden_weights_are_well_chosen(golden_dir):
    """On the golden's weights and its largest image the fp16 emulation stays within 5e-4 of the float64 forward (half the
    project's 1e-3, leaving the device a factor of two for accumulation order), and the body contributes: std of
    out - nearest(x) at least 0.03, and it moves with the input (not bias alone)."""
    g = np.load(golden_dir / "g10_compact.npz")
    img = g["enh_img"]
    for nc in (16, 32):
        sd = W.synthetic_compact_state_dict(nc, seed=0)
        f = cm.enhance_float(img, sd)
        e = cm.enhance_float(img, sd, emulated=True).astype(np.float64)
        err = float(np.abs(f - e).max())
        body = f - _nearest(img)
        flipped = np.ascontiguousarray(img[::-1, ::-1])
        body2 = cm.enhance_float(flipped, sd) - _nearest(flipped)
        moved = float(np.abs(body2[::-1, ::-1] - body).std())
        print(f"num_conv {nc}: emulation max-abs {err:.3g}, body std {body.std():.4f}, moves with the input by {moved:.4f}")
        assert err <= 5e-4
        assert body.std() >= 0.03
        assert moved >= 0.01


def test_u8_cap_is_reachable_on_the_gpu_images():
    """The GPU test allows 1 level at no more than 4 % of the values.  Truncation flips a level wherever the float lands within
    the error of an integer; here the checker-versus-emulation pair must stay within HALF that (2 %, 1 level) on the very images
    the GPU test uses, so the cap is known to be reachable before a GPU run.  (The two large images are checked on a corner
    each: the error statistics are per pixel, and the float64 net on 700 x 900 pixels takes minutes on a CPU.)"""
    imgs = cm.gpu_test_images()
    sd = W.synthetic_compact_state_dict(32, seed=0)
    for name, img in (("batch", imgs["batch"][0]), ("whole", imgs["whole"][:160, :200]), ("tiled", imgs["tiled"][:128, :160])):
        q = cm.enhance(img, sd)
        e = cm.enhance(img, sd, emulated=True)
        mx, share, ok = cm.u8_cap_check(q, e, 0.02)
        print(f"{name}: checker vs emulation max {mx}, share {share:.4f}")
        assert ok, (name, mx, share)


def test_u8_base_roundtrip_all_256():
    """(x/255)*255 and (x*(1/255f))*255 in fp32 truncate back to x for all 256 values: with a zero body the tail returns
    nearest-x4 of the input exactly."""
    x = np.arange(256, dtype=np.float32)
    a = (x / np.float32(255.0)) * np.float32(255.0)
    b = (x * np.float32(1.0 / 255.0)) * np.float32(255.0)
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(np.clip(a, 0, 255).astype(np.uint8), np.arange(256))
    assert np.array_equal(np.clip(b, 0, 255).astype(np.uint8), np.arange(256))


# ---- app ------------------------------------------------------------------------------------------------------------
def test_app_resolves_the_compact_names(tmp_path, monkeypatch):
    import inspect

    import app.cnn_super_resolution as m
    from app import sr_routes
    for name, nc in (("realesr_general_x4v3", 32), ("realesr_general_wdn_x4v3", 32), ("realesr_animevideov3", 16)):
        cfg = m.model_config(name)
        assert cfg["arch"] == "compact" and cfg["num_conv"] == nc and cfg["scale"] == 4
        assert cfg["url"].startswith("https://github.com/xinntao/Real-ESRGAN/releases/download/") and cfg["description"]
        assert name not in m.MODELS and name in m.EXTRA_MODELS
    assert set(m.MODELS) == {"realesrgan_x4", "realesrgan_anime"}
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path))
    monkeypatch.delenv("S2SR_ALLOW_DOWNLOAD", raising=False)
    with pytest.raises(ValueError):
        m.RealESRGAN(model_name="realesr_general_x2v3", device="cuda:0")
    with pytest.raises(ValueError):                      # a strength with any other model
        m.RealESRGAN(model_name="realesr_animevideov3", device="cuda:0", denoise_strength=0.5)
    with pytest.raises(ValueError):
        m.RealESRGAN(model_name="realesrgan_x4", device="cuda:0", denoise_strength=0.5)
    with pytest.raises(ValueError):
        m.RealESRGAN(model_name="realesr_general_x4v3", device="cuda:0", denoise_strength=1.5)
    with pytest.raises(FileNotFoundError):               # known name, no checkpoint file, no download
        m.RealESRGAN(model_name="realesr_general_x4v3", device="cuda:0")
    # the parameter container takes a real checkpoint's layout
    net = m.SRVGGNetCompact(num_conv=16)
    sd = W.synthetic_compact_state_dict(16)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert list(net.state_dict().keys()) == [k for k, _ in W.compact_specs(16)]
    with pytest.raises(ValueError):
        m.SRVGGNetCompact(num_conv=8)
    # the HTTP routes keep the reference's validation lists
    src = inspect.getsource(sr_routes)
    assert "realesr_general" not in src and "animevideov3" not in src


def test_dist_refuses_compact():
    from s2sr import dist

    class _Eng:
        arch, scale = "compact", 4

    class _Backend:
        scale, engine = 4, _Eng()

    with pytest.raises(ValueError, match="compact"):
        dist.enhance_distributed(_Backend(), np.zeros((8, 8, 3), np.uint8))
