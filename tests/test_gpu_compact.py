"""SRVGGNetCompact (s2sr_config.arch = S2SR_ARCH_COMPACT: realesr-general-x4v3, -wdn-x4v3, realesr-animevideov3) on the MI355X,
through the C ABI.  Checked against the float64 CPU checker tests/compact_model.py (pinned by tests/golden/g10_compact.npz):
network parity at the project's 1e-3, layers 0, 1, 16, num_conv and the last conv in situ on two batches against the checker fed
with the device's own previous activation (the judge of tests/compact_insitu.py; bound: tests/tail_model.py Layer.result), the
pixel-shuffle tail exactly, the u8 paths, byte identities across the run-time switches, the schedule, the error codes, and the
drop-in.  Every layer of both depths, the shape classes (mosaics with dead slots, AOI windows, whole tiles, degenerate sizes, the
fp32 entry off the u8 grid), out_u8 byte for byte, workspace reuse and guard bytes: tests/test_gpu_compact_insitu.py.

Measured (MI355X, seeded weights, u8 / 255 inputs): network max-abs error against float64 3.6e-4 at num_conv 16, 1.5e-4 at
num_conv 32 (the CPU emulation of the same formats on the golden: 2.8e-4 / 1.2e-4); u8 off by one level at 0.5 % of the values
(num_conv 32); per layer in situ the worst element sits at 0.996 of the bound."""
from __future__ import annotations


import numpy as np
import pytest
import torch

import compact_insitu as ci
import gpu_engines
import compact_model as cm
from s2sr import native
from s2sr import rasterio_lite as rio
from s2sr import weights as W

pytestmark = pytest.mark.gpu

TOL = 1e-3            # the project's tolerance against the fp32-class reference
U8_CAP = 0.04         # share of u8 values allowed to be one level off (twice what the CPU emulation shows)
HP, FAST, FP8 = native.PREC_F16_HP, native.PREC_F16, native.PREC_FP8
_SD = {}


def _sd(nc):
    if nc not in _SD:
        _SD[nc] = W.synthetic_compact_state_dict(nc, seed=0)
    return _SD[nc]


def engine(nc, precision=HP):
    return gpu_engines.default(nc, precision, arch="compact")


def _fresh(monkeypatch, nc, env, sd=None, **kw):
    return gpu_engines.fresh(monkeypatch, env, nc, HP, arch="compact", sd=sd if sd is not None else _sd(nc), **kw)


def _u8(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _ref_f64(u8_nhwc, sd):
    return cm.forward(torch.from_numpy(u8_nhwc).permute(0, 3, 1, 2).double() / 255.0, sd).numpy()


# ---- 1. network parity --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [16, 32])
def test_golden_net(golden_dir, nc):
    g = np.load(golden_dir / "g10_compact.npz")
    for prec in (HP, FAST):                       # the same arithmetic on this arch: same bytes
        y = engine(nc, prec).forward_f32(g["net_x"])
        assert y.shape == (1, 3, 80, 96)
        err = float(np.abs(y - g[f"net_c{nc}"]).max())
        print(f"num_conv {nc} precision {prec}: golden max-abs {err:.3g}")
        assert err <= TOL
    assert np.array_equal(engine(nc, HP).forward_f32(g["net_x"]), engine(nc, FAST).forward_f32(g["net_x"]))


@pytest.mark.parametrize("nc,shape", [(32, (1, 37, 53)), (32, (3, 64, 64)), (16, (3, 37, 53)), (16, (1, 256, 256)), (32, (32, 40, 24))])
def test_forward_f32_vs_checker(nc, shape):
    u = _u8(sum(shape) + nc, *shape, 3)
    x = (u.astype(np.float32) / 255.0).transpose(0, 3, 1, 2)
    y = engine(nc).forward_f32(x)
    exp = _ref_f64(u, _sd(nc))
    err = float(np.abs(y - exp).max())
    print(f"num_conv {nc} {shape}: max-abs {err:.3g}")
    assert y.shape == exp.shape and err <= TOL


# ---- 2. in situ per layer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,B,th,tw", [(32, 2, 40, 56), (16, 5, 37, 45)])
def test_layers_in_situ(nc, B, th, tw, monkeypatch):
    """The activation after the first conv and after body convs 1, 16 and num_conv, each against the checker's arithmetic on the
    DEVICE's own previous activation (so one layer is what is judged).  Bound per element: tail_model.Layer.result (stages x taps
    fp32 accumulator roundings of half an ulp of the running sum, two ulps for the epilogue) through the PReLU (slopes below 1
    do not widen it), then half an fp16 quantum for the store.  The arithmetic lives in tests/compact_insitu.py (judge), which
    judges the last conv, out_u8, p0 and the zeros outside the live pixels of the same run as well; all layers and the other
    shape classes: tests/test_gpu_compact_insitu.py."""
    sd = ci.insitu_sd(nc)
    e = _fresh(monkeypatch, nc, {}, sd=sd)
    tiles = ci.insitu_tiles(nc + B, B, th, tw)
    want = sorted({0, 1, 15, 16, nc - 1, nc})
    geo, acts, p0, out_f32, out_u8 = e.debug_compact_taps(want, tiles=tiles)
    rep = ci.judge(geo, acts, p0, out_f32, out_u8, sd, B, th, tw, tiles=tiles)      # need_negative: every channel, every judged layer
    print(rep.text(f"num_conv {nc} {B}x{th}x{tw}"))
    assert set(rep.judged) == {0, 1, 16, nc, nc + 1}
    assert not rep.fails, rep.message()
    # the hook's outputs are production's
    assert np.array_equal(out_f32, e.forward_f32((tiles.astype(np.float32) / 255.0).transpose(0, 3, 1, 2)))
    e.close()


# ---- 3. the tail ------------------------------------------------------------------------------------------------------------
def _zero_body(nc):
    sd = {k: v.copy() for k, v in _sd(nc).items()}
    last = f"body.{2 * nc + 2}"
    for k in sd:
        if k.startswith(last) or (len(sd[k].shape) == 4 and k != "body.0.weight"):
            sd[k] = np.zeros_like(sd[k])
    return sd, last


def test_zero_body_returns_nearest_x4_exactly(monkeypatch):
    sd, _ = _zero_body(16)
    e = _fresh(monkeypatch, 16, {}, sd=sd)
    ramp = np.arange(256, dtype=np.uint8)
    tiles = np.stack([np.stack([np.roll(ramp, 7 * c + 31 * r) for c in range(3)], axis=-1) for r in range(8)])[None]   # [1, 8, 256, 3]
    tiles = np.concatenate([tiles, tiles[:, ::-1, ::-1]])
    assert all(set(np.unique(tiles[..., c])) == set(range(256)) for c in range(3))
    out = e.forward_batch_u8(tiles)
    assert np.array_equal(out, np.repeat(np.repeat(tiles, 4, axis=1), 4, axis=2))
    f = e.forward_f32((tiles.astype(np.float32) / 255.0).transpose(0, 3, 1, 2))
    assert np.abs(f.transpose(0, 2, 3, 1) - np.repeat(np.repeat(tiles, 4, axis=1), 4, axis=2) / 255.0).max() <= 2e-7
    e.close()


def test_sub_pixel_order_on_the_device(monkeypatch):
    """A one-hot last conv (bias delta on one of the 48 channels, everything behind the first conv zero): the device moves the
    same single HR sub-pixel of the same colour as the checker."""
    sd, last = _zero_body(16)
    x = np.zeros((1, 3, 9, 35), np.float32)
    e = _fresh(monkeypatch, 16, {}, sd=sd)
    for ch in range(48):
        b = np.zeros(48, np.float32)
        b[ch] = 0.5
        sd[last + ".bias"] = b
        e.load_state_dict(sd)
        out = e.forward_f32(x)
        exp = cm.forward(torch.from_numpy(x), sd).numpy()
        assert np.array_equal(out, exp.astype(np.float32)), ch
        o8 = e.forward_batch_u8(np.zeros((1, 9, 35, 3), np.uint8))
        assert np.array_equal(o8, cm.quantise(exp.transpose(0, 2, 3, 1))), ch
    e.close()


# ---- 4. u8 paths -----------------------------------------------------------------------------------------------------------
def test_u8_paths_vs_checker():
    imgs = cm.gpu_test_images()
    sd, e = _sd(32), engine(32)
    q = cm.quantise(_ref_f64(imgs["batch"], sd).transpose(0, 2, 3, 1))
    mx, share, ok = cm.u8_cap_check(e.forward_batch_u8(imgs["batch"]), q, U8_CAP)
    print(f"forward_batch_u8: max {mx}, share {share:.4f}")
    assert ok
    for name, tile in (("whole", 256), ("tiled", 256)):          # 300 x 420 <= 256^2 * 4 < 700 x 900: both branches of the rule
        img = imgs[name]
        assert (img.shape[0] * img.shape[1] > tile * tile * 4) == (name == "tiled")
        exp_f = cm.enhance_float(img, sd, tile, 10)
        out = e.enhance_u8(img, tile=tile, pad=10)
        mx, share, ok = cm.u8_cap_check(out, cm.quantise(exp_f), U8_CAP)
        print(f"enhance_u8 {name}: max {mx}, share {share:.4f}")
        assert out.shape == (4 * img.shape[0], 4 * img.shape[1], 3) and ok
        f = e.enhance_f32(img, tile=tile, pad=10)
        assert float(np.abs(f - exp_f).max()) <= TOL
    img = imgs["whole"]
    t = e.tile_process_f32(img, tile=128, pad=10)
    exp_t = cm.enhance_float(img, sd, 128, 10, force_tiled=True)
    err = float(np.abs(t - exp_t).max())
    mx, share, ok = cm.u8_cap_check(cm.quantise(t.astype(np.float64)), cm.quantise(exp_t), U8_CAP)
    print(f"tile_process_f32: max-abs {err:.3g}; u8 max {mx}, share {share:.4f}")
    assert err <= TOL and ok


def test_enhance_job_equals_enhance_plus_postprocess():
    e = engine(16)
    rgb = _u8(13, 301, 433, 3)
    exp_sr = np.ascontiguousarray(e.enhance_u8(np.ascontiguousarray(rgb[:, :, ::-1]), tile=64)[:, :, ::-1])
    assert np.array_equal(e.enhance_job_u8(rgb, None, tile=64), exp_sr)
    assert np.array_equal(e.enhance_job_u8(rgb, native.pp_wow(), tile=64), e.postprocess_u8(exp_sr, native.pp_wow()))


# ---- 5. byte identities --------------------------------------------------------------------------------------------------
def test_mosaic_groups_graphs_and_batches_give_the_same_bytes(monkeypatch):
    tiles = _u8(5, 7, 60, 84, 3)
    base = _fresh(monkeypatch, 16, {})
    ref8 = base.forward_batch_u8(tiles).copy()
    for _ in range(2):                                              # second sighting captures, third replays
        assert np.array_equal(base.forward_batch_u8(tiles), ref8)
    assert base.graph_stats()[1] >= 1
    variants = {"no mosaic": _fresh(monkeypatch, 16, {"S2SR_MOSAIC": "0"}),
                "no graphs": _fresh(monkeypatch, 16, {"S2SR_GRAPH": "0"}),
                "group 4": _fresh(monkeypatch, 16, {}, group=4),
                "group 16": _fresh(monkeypatch, 16, {}, group=16)}
    for name, e in variants.items():
        for _ in range(3):
            assert np.array_equal(e.forward_batch_u8(tiles), ref8), name
        e.close()
    singles = np.concatenate([base.forward_batch_u8(tiles[i:i + 1]) for i in range(len(tiles))])
    assert np.array_equal(singles, ref8)
    # a batch of the plan's windows against enhance on the image they were cut from
    img = _u8(6, 150, 170, 3)
    out = base.enhance_u8(img, tile=64, pad=10)
    wins = native.plan_tiles(150, 170, 64, 10, 4)
    batch = np.stack([img[w.y1:w.y2, w.x1:w.x2] for w in wins])
    o = base.forward_batch_u8(batch)
    for k, w in enumerate(wins):
        t = o[k][w.crop_top:o[k].shape[0] - w.crop_bottom, w.crop_left:o[k].shape[1] - w.crop_right]
        last = all(not (v.oy1 < w.oy2 and w.oy1 < v.oy2 and v.ox1 < w.ox2 and w.ox1 < v.ox2) for v in wins[k + 1:])
        if last:
            assert np.array_equal(out[w.oy1:w.oy2, w.ox1:w.ox2], t), k
    base.close()


def test_dev_entries_equal_host_entries():
    e = engine(16)
    tiles = _u8(8, 6, 276, 276, 3)
    exp = e.forward_batch_u8(tiles)
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(tiles).to(dev)
    out = torch.empty((6, 1104, 1104, 3), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    e.forward_batch_u8_dev(x.data_ptr(), 6, 276, 276, out.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), exp)
    out.zero_()
    e.forward_part_u8_dev(x.data_ptr(), 4, 276, 276, 6, out.data_ptr(), st)
    e.forward_part_u8_dev(x[4:].data_ptr(), 2, 276, 276, 6, out[4:].data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), exp)


# ---- 6. the schedule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [16, 32])
def test_schedule(nc):
    e = engine(nc)
    tiles = _u8(1, 32, 256, 256, 3)
    e.set_profiling(1)
    e.reset_kernel_stats()
    out = e.forward_batch_u8(tiles)
    st = {k: v for k, v in e.kernel_stats().items() if v["launches"]}
    e.set_profiling(0)
    assert out.shape == (32, 1024, 1024, 3)
    groups = -(-32 // e.group_images())
    assert st["compact_first"]["launches"] == groups and st["compact_last"]["launches"] == groups
    assert st["compact_body"]["launches"] == nc * groups
    assert sum(st[k]["launches"] for k in ("compact_first", "compact_body", "compact_last")) == (nc + 2) * groups
    assert set(st) == {"pack_u8", "compact_first", "compact_body", "compact_last"}, st.keys()
    px = 32 * 256 * 256
    assert st["compact_body"]["flops"] == pytest.approx(nc * 2 * 9 * 64 * 64 * px) and st["compact_body"]["bytes"] == pytest.approx(nc * 256 * px)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------
def test_errors():
    with pytest.raises(native.S2srError, match="invalid argument"):
        native.Engine(num_block=7, arch="compact")
    with pytest.raises(native.S2srError, match="invalid argument"):
        native.Engine(num_block=32, arch="compact", scale=2)
    with pytest.raises(native.S2srError, match="fp8"):
        native.Engine(num_block=32, arch="compact", precision=FP8)
    lib = native.load_library()
    import ctypes as C
    cfg = native._Config(32, 64, 32, 4, HP, 0, 0, 2)                  # an arch nobody defined
    h = C.c_void_p()
    assert lib.s2sr_create(C.byref(cfg), C.byref(h)) == -1
    e = engine(16)
    with pytest.raises(native.S2srError, match="bad weight blob"):
        e.load_blob(np.zeros(lib.s2sr_expected_blob_floats(1), np.float32))
    with pytest.raises(native.S2srError, match="bad weight blob"):
        e.load_blob(np.zeros(W.num_params_compact(32), np.float32))
    with pytest.raises(ValueError, match="rrdb"):
        e.load_state_dict(W.synthetic_state_dict(1, seed=0))
    tiles = np.zeros((1, 24, 32, 3), np.uint8)
    with pytest.raises(native.S2srError, match="invalid argument"):
        e.debug_trunk_taps(0, 1, tiles=tiles)
    with pytest.raises(native.S2srError, match="invalid argument"):
        e.debug_forward_taps(tiles=tiles)
    with pytest.raises(native.S2srError, match="invalid argument"):
        e.rdb_persistent(0, 8, 2, 1, 1)
    with pytest.raises(native.S2srError, match="invalid argument"):
        e.debug_conv_trunk(0, np.zeros((1, 64, 8, 32), np.float32), np.zeros((32, 64, 3, 3), np.float32), np.zeros(32, np.float32))
    with pytest.raises(native.S2srError, match="invalid argument"):
        e.calibrate_fp8(tiles)
    rrdb = native.Engine(num_block=1)
    rrdb.load_state_dict(W.synthetic_state_dict(1, seed=0))
    with pytest.raises(native.S2srError, match="compact handles only"):
        rrdb.debug_compact_taps([0], tiles=tiles)
    rrdb.close()
    u = _u8(3, 2, 24, 32, 3)                                          # the handle keeps working
    assert np.abs(e.forward_f32((u.astype(np.float32) / 255.0).transpose(0, 3, 1, 2)) - _ref_f64(u, _sd(16))).max() <= TOL


# ---- 8. RRDB unchanged ---------------------------------------------------------------------------------------------------
def test_rrdb_engines_unchanged_next_to_a_compact_engine():
    tiles4, tiles2 = _u8(21, 3, 40, 56, 3), _u8(22, 3, 48, 64, 3)

    def run_rrdb():
        outs = []
        for scale, tiles in ((4, tiles4), (2, tiles2)):
            r = native.Engine(num_block=2, precision=HP, scale=scale)
            r.load_state_dict(W.synthetic_state_dict(2, seed=0, scale=scale))
            outs.append(r.forward_batch_u8(tiles).copy())
            r.close()
        return outs

    alone = run_rrdb()
    c = native.Engine(num_block=16, precision=HP, arch="compact")
    c.load_state_dict(_sd(16))
    c8 = c.forward_batch_u8(tiles4).copy()
    r4 = native.Engine(num_block=2, precision=HP, scale=4)
    r4.load_state_dict(W.synthetic_state_dict(2, seed=0, scale=4))
    r2 = native.Engine(num_block=2, precision=HP, scale=2)
    r2.load_state_dict(W.synthetic_state_dict(2, seed=0, scale=2))
    for _ in range(2):
        assert np.array_equal(r4.forward_batch_u8(tiles4), alone[0])
        assert np.array_equal(c.forward_batch_u8(tiles4), c8)
        assert np.array_equal(r2.forward_batch_u8(tiles2), alone[1])
    for x in (c, r4, r2):
        x.close()
    from oracle import rrdbnet_ref as ref
    exp = ref.enhance(tiles4[0], ref.to_torch_sd(W.synthetic_state_dict(2, seed=0)), 2)
    assert np.abs(alone[0][0].astype(int) - exp.astype(int)).max() <= 1


# ---- 9. the drop-in ------------------------------------------------------------------------------------------------------
def test_app_compact(monkeypatch, tmp_path):
    import app.cnn_super_resolution as m
    from app.wow_sr import process_wow_sr
    mdir = tmp_path / "models"
    mdir.mkdir()
    monkeypatch.setenv("S2SR_MODEL_DIR", str(mdir))
    a, b = W.synthetic_compact_state_dict(32, seed=0), W.synthetic_compact_state_dict(32, seed=1)
    torch.save({"params": {k: torch.from_numpy(v) for k, v in a.items()}}, mdir / "realesr_general_x4v3.pth")
    torch.save({"params": {k: torch.from_numpy(v) for k, v in b.items()}}, mdir / "realesr_general_wdn_x4v3.pth")
    img = _u8(17, 40, 56, 3)
    e = m.RealESRGAN(model_name="realesr_general_x4v3")
    assert e.scale == 4 and e._engine.arch == "compact" and e._engine.num_block == 32
    out = e.enhance(img)
    assert out.shape == (160, 224, 3) and cm.u8_cap_check(out, cm.enhance(img, a), U8_CAP)[2]
    assert tuple(e._tile_process(torch.from_numpy(img.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)).shape) == (1, 3, 160, 224)
    assert e.enhance_job(img).shape == (160, 224, 3)
    d = m.RealESRGAN(model_name="realesr_general_x4v3", denoise_strength=0.5)
    mix = W.dni(a, b, 0.5)
    out_d = d.enhance(img)
    assert cm.u8_cap_check(out_d, cm.enhance(img, mix), U8_CAP)[2]
    assert not cm.u8_cap_check(out_d, out, U8_CAP)[2]                   # the interpolated weights are another net
    with pytest.raises(ValueError, match="denoise_strength"):
        m.RealESRGAN(model_name="realesr_general_wdn_x4v3", denoise_strength=0.5)
    # process_wow_sr end to end on a GeoTIFF
    rgb = _u8(19, 25, 33, 3)
    src = tmp_path / "scene.tif"
    rio.write_geotiff_rgb(src, rgb, rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)}))
    res = process_wow_sr(src, tmp_path / "wow", enhance_crops=False, model="realesr_general_x4v3")
    meta = res["sr_metadata"]
    assert meta["scale"] == 4 and sorted(meta["output_size"]) == [100, 132]
    assert meta["stages"][0] == {"model": "realesr_general_x4v3", "scale": 4, "purpose": "GAN upscaling"}
    sr, g2 = rio.read_rgb_u8(res["outputs"]["sr_tif"])
    assert sr.shape == (100, 132, 3) and g2.pixel_size == (2.5, 2.5)
    exp_sr = cm.enhance(np.ascontiguousarray(rgb[:, :, ::-1]), a)[:, :, ::-1]
    assert cm.u8_cap_check(sr, exp_sr, U8_CAP)[2]
