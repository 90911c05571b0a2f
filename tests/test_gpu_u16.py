"""The 16-bit door on the GPU (include/s2sr.h: s2sr_forward_batch_u16, s2sr_forward_batch_u16_dev, s2sr_enhance_u16) and its
Python seam (RealESRGAN.enhance16, process_wow_sr(bit_depth=16)).

The arithmetic is fixed: the net sees x = (clip(v, lo, hi) - lo) / (hi - lo), the output is lo + rint(clip(y, 0, 1) * (hi - lo)) with the
product in fp32.  The oracle is oracle.rrdbnet_ref fed that x as float32; the float tolerances are the ones tests/test_gpu_net.py
holds the same arithmetic to."""
import ctypes as C
import functools
import json
import math

import numpy as np
import pytest
import torch

import gpu_engines
from oracle import rrdbnet_ref as ref
from s2sr import native
from s2sr import rasterio_lite as rio
from s2sr import tiff_lite
from s2sr.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

# tests/test_gpu_net.py's constants for the same nets
TOL_F16 = 2.5e-3
TOL_HP = 3e-4
TOL_FP8_6 = 1e-3
F16, HP, FP8 = native.PREC_F16, native.PREC_F16_HP, native.PREC_FP8
MODES = [(HP, TOL_HP), (F16, TOL_F16)]
FULL, SUB = (0, 65535), (1000, 11000)
BANDED = (100, 90, 16, 2)        # H, W, tile, pad: 42 planned windows, 36 distinct ones that fill one 6 x 6 mosaic -- ONE chunk
CHUNKED = (53, 200, 16, 3)       # 3 x 13 distinct windows of 22 x 22, one per launch image, a launch group of 16: three chunks of one row
assert native.pick_mosaic(39, 22, 22) == (1, 1) and native.plan_chunks(3, 1, 13, 1, 1, 256) == [1, 1, 1]


def quantise(y, lo, hi):
    """The 16-bit door's output rule, restated."""
    return lo + np.rint(np.clip(y, 0, 1).astype(np.float32) * np.float32(hi - lo)).astype(np.int64)


def net_input(v, lo, hi):
    return ((np.clip(v.astype(np.int64), lo, hi) - lo) / (hi - lo)).astype(np.float32)


def levels(tol, lo, hi):
    return math.ceil(tol * (hi - lo)) + 1


@functools.lru_cache(maxsize=None)
def tsd(nb):
    return ref.to_torch_sd(synthetic_state_dict(nb, seed=0))


@functools.lru_cache(maxsize=None)
def data(kind):
    """The inputs the tests share (never written to)."""
    rng = np.random.default_rng({"img_full": 1, "img_stray": 2, "batch_full": 3, "batch_stray": 4, "chunked_full": 5, "chunked_stray": 6}[kind])
    top = 65536 if kind.endswith("full") else 13000          # 'stray': values below 1000 and above 11000
    shape = {"img": (BANDED[0], BANDED[1], 3), "chunked": (CHUNKED[0], CHUNKED[1], 3), "batch": (3, 50, 33, 3)}[kind.split("_")[0]]
    a = rng.integers(0, top, size=shape).astype(np.uint16)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle(kind, lo, hi):
    """float32 oracle output for data(kind) under the range: HWC for the image (the tiled path), NCHW for the batch."""
    x = net_input(data(kind), lo, hi)
    with torch.no_grad():
        if kind.startswith("img"):
            o = ref.tile_process(torch.from_numpy(x).permute(2, 0, 1).unsqueeze(0), tsd(1), 1, BANDED[2], BANDED[3])
            out = o[0].permute(1, 2, 0).contiguous().numpy()
        else:
            out = ref.rrdbnet_forward(torch.from_numpy(x).permute(0, 3, 1, 2).contiguous(), tsd(1), 1).numpy()
    out.setflags(write=False)
    return out


def nhwc(f):
    return np.ascontiguousarray(f.transpose(0, 2, 3, 1))


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [F16, HP])
def test_bit_identity_with_the_8_bit_door(prec):
    """Data below 256 with range (0, 255): the input plane holds what pack_u8 writes (the high channels are exact zeros), so the
    float output is the u8 door's, bit for bit."""
    e = gpu_engines.default(2, prec)
    rng = np.random.default_rng(40)
    for shape in [(5, 24, 40, 3), (2, 64, 64, 3)]:          # a ragged mosaic, plain images
        t8 = rng.integers(0, 256, size=shape, dtype=np.uint8)
        q, f = e.forward_batch_u16(t8.astype(np.uint16), 0, 255, want_f32=True)
        f8 = e.forward_f32(np.ascontiguousarray((t8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)))
        assert np.array_equal(f, f8), (shape, float(np.abs(f - f8).max()))
        assert np.array_equal(q, quantise(nhwc(f), 0, 255))
    for H, W, ts, tp in (BANDED, CHUNKED):
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        _, f = e.enhance_u16(img.astype(np.uint16), 0, 255, tile=ts, pad=tp, want_f32=True)
        assert np.array_equal(f, e.enhance_f32(img, tile=ts, pad=tp)), (H, W)
    whole = rng.integers(0, 256, size=(28, 36, 3), dtype=np.uint8)
    _, f = e.enhance_u16(whole.astype(np.uint16), 0, 255, want_f32=True)
    assert np.array_equal(f, e.enhance_f32(whole))


# ---- 2, 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,tol", MODES)
def test_full_range_parity_and_own_quantisation(prec, tol):
    """Random uint16 over 0..65535, default range: float error within the mode's tolerance against the oracle; the u16 output is
    exactly the stated rule applied to the same call's float output, and within ceil(tol * range) + 1 levels of the oracle's."""
    e = gpu_engines.default(1, prec)
    H, W, ts, tp = BANDED
    assert len(native.plan_tiles(H, W, ts, tp)) > 16
    img, tiles = data("img_full"), data("batch_full")
    q, f = e.enhance_u16(img, tile=ts, pad=tp, want_f32=True)
    err = float(np.abs(f - oracle("img_full", *FULL)).max())
    print(f"banded u16 {H}x{W} prec {prec}: float err {err:.3e}")
    assert err <= tol
    assert q.dtype == np.uint16 and q.shape == (4 * H, 4 * W, 3) and np.array_equal(q, quantise(f, *FULL))
    dq = np.abs(q.astype(np.int64) - quantise(oracle("img_full", *FULL), *FULL))
    print(f"   u16 vs oracle: max {int(dq.max())} levels (bound {levels(tol, *FULL)})")
    assert dq.max() <= levels(tol, *FULL)
    # the chunked route (u16 only: bands stitched and copied chunk by chunk) gives the same image
    assert np.array_equal(e.enhance_u16(img, tile=ts, pad=tp), q)
    _, _, tsc, tpc = CHUNKED                                                             # ... in several chunks
    qc, _ = e.enhance_u16(data("chunked_full"), tile=tsc, pad=tpc, want_f32=True)
    assert np.array_equal(e.enhance_u16(data("chunked_full"), tile=tsc, pad=tpc), qc)
    qb, fb = e.forward_batch_u16(tiles, want_f32=True)
    errb = float(np.abs(fb - oracle("batch_full", *FULL)).max())
    print(f"batch u16 (3, 50, 33) prec {prec}: float err {errb:.3e}")
    assert errb <= tol
    assert qb.shape == (3, 200, 132, 3) and np.array_equal(qb, quantise(nhwc(fb), *FULL))
    assert np.abs(qb.astype(np.int64) - quantise(nhwc(oracle("batch_full", *FULL)), *FULL)).max() <= levels(tol, *FULL)
    assert np.array_equal(e.forward_batch_u16(tiles), qb)


# ---- 3, 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,tol", MODES)
def test_value_range_clamps_and_rescales(prec, tol):
    """Range (1000, 11000) on data that strays below and above it: the result is the one for the clipped data, the float output
    matches the oracle fed the clipped, rescaled data, the u16 output is the rule on that float output and stays in [lo, hi]."""
    e = gpu_engines.default(1, prec)
    lo, hi = SUB
    H, W, ts, tp = BANDED
    img, tiles = data("img_stray"), data("batch_stray")
    assert img.min() < lo and img.max() > hi and tiles.min() < lo and tiles.max() > hi
    q, f = e.enhance_u16(img, lo, hi, tile=ts, pad=tp, want_f32=True)
    qc, fc = e.enhance_u16(np.clip(img, lo, hi), lo, hi, tile=ts, pad=tp, want_f32=True)
    assert np.array_equal(q, qc) and np.array_equal(f, fc)
    err = float(np.abs(f - oracle("img_stray", lo, hi)).max())
    print(f"banded u16 range {SUB} prec {prec}: float err {err:.3e}")
    assert err <= tol
    assert np.array_equal(q, quantise(f, lo, hi)) and q.min() >= lo and q.max() <= hi
    assert np.abs(q.astype(np.int64) - quantise(oracle("img_stray", lo, hi), lo, hi)).max() <= levels(tol, lo, hi)
    assert np.array_equal(e.enhance_u16(img, lo, hi, tile=ts, pad=tp), q)               # the chunked route
    _, _, tsc, tpc = CHUNKED                                                             # ... in several chunks
    qc, _ = e.enhance_u16(data("chunked_stray"), lo, hi, tile=tsc, pad=tpc, want_f32=True)
    assert np.array_equal(e.enhance_u16(data("chunked_stray"), lo, hi, tile=tsc, pad=tpc), qc)
    qb, fb = e.forward_batch_u16(tiles, lo, hi, want_f32=True)
    qbc, fbc = e.forward_batch_u16(np.clip(tiles, lo, hi), lo, hi, want_f32=True)
    assert np.array_equal(qb, qbc) and np.array_equal(fb, fbc)
    errb = float(np.abs(fb - oracle("batch_stray", lo, hi)).max())
    print(f"batch u16 range {SUB} prec {prec}: float err {errb:.3e}")
    assert errb <= tol
    assert np.array_equal(qb, quantise(nhwc(fb), lo, hi)) and qb.min() >= lo and qb.max() <= hi
    assert np.abs(qb.astype(np.int64) - quantise(nhwc(oracle("batch_stray", lo, hi)), lo, hi)).max() <= levels(tol, lo, hi)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_graphs_are_keyed_by_the_value_range(monkeypatch):
    """Same shapes, same scratch pointers, alternating ranges: the range's constants are baked into a captured graph, so a graph
    of one range must never be replayed for the other."""
    tiles, img = data("batch_stray"), data("img_stray")
    H, W, ts, tp = BANDED
    plain = gpu_engines.fresh(monkeypatch, {"S2SR_GRAPH": "0"}, 1, HP)
    want = {r: (plain.forward_batch_u16(tiles, *r), plain.enhance_u16(img, *r, tile=ts, pad=tp)) for r in (FULL, SUB)}
    assert plain.graph_stats() == (0, 0)
    plain.close()
    assert not np.array_equal(want[FULL][0], want[SUB][0])
    e = gpu_engines.fresh(monkeypatch, {}, 1, HP)
    for i, r in enumerate((FULL, SUB, FULL, SUB, FULL)):
        assert np.array_equal(e.forward_batch_u16(tiles, *r), want[r][0]), (i, r)
    cap, rep = e.graph_stats()
    print(f"batch: captures {cap}, replays {rep}")
    assert cap >= 2 and rep >= 3
    for i, r in enumerate((FULL, SUB, FULL, SUB, FULL)):
        assert np.array_equal(e.enhance_u16(img, *r, tile=ts, pad=tp), want[r][1]), (i, r)
    cap2, rep2 = e.graph_stats()
    print(f"enhance: captures {cap2 - cap}, replays {rep2 - rep}")
    assert cap2 >= cap + 2 and rep2 >= rep + 3
    e.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [HP, F16])
def test_interleaving_with_8_bit_calls(prec):
    """The doors share the input plane and the workspace: after a 16-bit call channels 4..5 of the plane hold stale values that
    pack_u8 does not overwrite (their u8 weights are zero).  u8 results before and after 16-bit calls are byte-identical."""
    e = gpu_engines.default(2, prec)
    rng = np.random.default_rng(41)
    H, W, ts, tp = BANDED
    tm = rng.integers(0, 256, size=(5, 24, 40, 3), dtype=np.uint8)            # travels as a mosaic
    tp8 = rng.integers(0, 256, size=(2, 64, 64, 3), dtype=np.uint8)           # plain images
    im = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    before = (e.forward_batch_u8(tm), e.forward_batch_u8(tp8), e.enhance_u8(im, ts, tp))
    u = {s: rng.integers(0, 65536, size=s).astype(np.uint16) for s in (tm.shape, tp8.shape, im.shape)}
    first16 = (e.forward_batch_u16(u[tm.shape]), e.forward_batch_u16(u[tp8.shape]), e.enhance_u16(u[im.shape], tile=ts, pad=tp))
    for _ in range(2):
        # 16-bit on a shape, then 8-bit on the same shape; a mosaic shape followed by a plain one
        a16 = e.forward_batch_u16(u[tm.shape])
        a8 = e.forward_batch_u8(tm)
        b16 = e.forward_batch_u16(u[tp8.shape])
        b8 = e.forward_batch_u8(tp8)
        c16 = e.enhance_u16(u[im.shape], tile=ts, pad=tp)
        c8 = e.enhance_u8(im, ts, tp)
        assert np.array_equal(a8, before[0]) and np.array_equal(b8, before[1]) and np.array_equal(c8, before[2])
        assert np.array_equal(a16, first16[0]) and np.array_equal(b16, first16[1]) and np.array_equal(c16, first16[2])
    assert np.array_equal(e.forward_batch_u8(tm), before[0])


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_window_mosaics_give_the_same_bytes_u16(monkeypatch):
    on = gpu_engines.fresh(monkeypatch, {}, 2, HP)
    off = gpu_engines.fresh(monkeypatch, {"S2SR_MOSAIC": "0"}, 2, HP)
    assert on.debug_config()["mosaic_on"] == 1 and off.debug_config()["mosaic_on"] == 0
    rng = np.random.default_rng(42)
    tiles = rng.integers(0, 65536, size=(7, 50, 33, 3)).astype(np.uint16)
    (qa, fa), (qb, fb) = on.forward_batch_u16(tiles, want_f32=True), off.forward_batch_u16(tiles, want_f32=True)
    assert np.array_equal(qa, qb) and np.array_equal(fa, fb)
    assert np.array_equal(on.forward_batch_u16(tiles), qa)                              # replay and stale-slot hygiene
    img = rng.integers(0, 65536, size=(150, 170, 3)).astype(np.uint16)
    a, b = on.enhance_u16(img, tile=64, pad=10), off.enhance_u16(img, tile=64, pad=10)
    assert np.array_equal(a, b)
    assert np.array_equal(on.enhance_u16(img, *SUB, tile=64, pad=10), off.enhance_u16(img, *SUB, tile=64, pad=10))
    on.close(); off.close()


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
def test_dev_entry_equals_the_host_entry():
    e = gpu_engines.default(1, HP)
    tiles = data("batch_stray")
    B, h, w, _ = tiles.shape
    x = torch.from_numpy(tiles.view(np.int16).copy()).cuda()                            # (torch has no uint16 arithmetic: the bits travel as int16)
    side = torch.cuda.Stream()
    for r in (FULL, SUB):
        want = e.forward_batch_u16(tiles, *r)
        y = torch.zeros((B, 4 * h, 4 * w, 3), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(3):                                                          # direct, capture, replay
                y.zero_()
                e.forward_batch_u16_dev(x.data_ptr(), B, h, w, y.data_ptr(), *r, stream=side.cuda_stream)
        side.synchronize()
        assert np.array_equal(y.cpu().numpy().view(np.uint16), want), r


# ---- 9 -------------------------------------------------------------------------------------------------------------------------
def test_fp8_trunk_takes_16_bit_input(golden_dir):
    g3 = np.load(golden_dir / "g3_small_nets.npz")
    v = np.rint(g3["x"] * 65535).astype(np.uint16)                                      # [1, 3, 16, 16]
    e = gpu_engines.default(6, FP8)
    q, f = e.forward_batch_u16(nhwc(v), want_f32=True)
    with torch.no_grad():
        exp = ref.rrdbnet_forward(torch.from_numpy((v.astype(np.float32) / np.float32(65535.0))), tsd(6), 6).numpy()
    err = float(np.abs(f - exp).max())
    print(f"fp8 nb 6, 16-bit input: float err {err:.3e}")
    assert np.isfinite(f).all() and err <= TOL_FP8_6
    assert np.array_equal(q, quantise(nhwc(f), *FULL))


# ---- 10 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_working():
    e = gpu_engines.default(1, HP)
    tiles, img = data("batch_full"), data("img_full")
    H, W, ts, tp = BANDED
    want_b, want_i = e.forward_batch_u16(tiles), e.enhance_u16(img, tile=ts, pad=tp)

    def still_fine():
        assert np.array_equal(e.forward_batch_u16(tiles), want_b) and np.array_equal(e.enhance_u16(img, tile=ts, pad=tp), want_i)

    for lo, hi in [(5, 5), (0, 65536), (-1, 100), (200, 100)]:
        with pytest.raises(native.S2srError, match=r"invalid argument.*value range"):
            e.forward_batch_u16(tiles, lo, hi)
        with pytest.raises(native.S2srError, match=r"invalid argument.*value range"):
            e.enhance_u16(img, lo, hi, tile=ts, pad=tp)
        still_fine()
    # both outputs NULL
    lib = e._lib
    B, h, w, _ = tiles.shape
    assert lib.s2sr_forward_batch_u16(e._h, tiles.ctypes.data_as(C.c_void_p), B, h, w, 0, 65535, None, None) == -1
    assert lib.s2sr_last_error(e._h)
    assert lib.s2sr_enhance_u16(e._h, img.ctypes.data_as(C.c_void_p), H, W, ts, tp, 0, 65535, None, None) == -1
    assert lib.s2sr_last_error(e._h)
    still_fine()
    # a scale-2 handle and a compact handle: S2SR_E_INVALID with a message; their own doors still answer
    t8 = np.random.default_rng(43).integers(0, 256, size=(2, 24, 32, 3), dtype=np.uint8)
    for other in (gpu_engines.default(1, HP, scale=2), gpu_engines.default(16, F16, arch="compact")):
        w8 = other.forward_batch_u8(t8)
        for call in (lambda: other.forward_batch_u16(t8.astype(np.uint16)), lambda: other.enhance_u16(t8[0].astype(np.uint16))):
            with pytest.raises(native.S2srError, match=r"invalid argument.*16-bit input is not available") as ei:
                call()
            assert "scale-2" in str(ei.value) or "COMPACT" in str(ei.value)
        assert np.array_equal(other.forward_batch_u8(t8), w8)
    # no weights
    bare = native.Engine(num_block=1, precision=HP)
    with pytest.raises(native.S2srError, match="weights not loaded"):
        bare.forward_batch_u16(tiles)
    with pytest.raises(native.S2srError, match="weights not loaded"):
        bare.enhance_u16(img, tile=ts, pad=tp)
    bare.load_state_dict(synthetic_state_dict(1, seed=0))
    assert np.array_equal(bare.forward_batch_u16(tiles), want_b)
    bare.close()
    with pytest.raises(TypeError):
        e.forward_batch_u16(tiles.astype(np.uint8))
    with pytest.raises(TypeError):
        e.enhance_u16(img.astype(np.float32))
    still_fine()


# ---- 11 ------------------------------------------------------------------------------------------------------------------------
def _patch_weights(monkeypatch, tmp_path, nb_by_name):
    """Seeded synthetic checkpoints where the drop-in looks for them (tests/test_gpu_app.py)."""
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir(exist_ok=True)
    for name, nb in nb_by_name.items():
        sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(nb, seed=0).items()}
        torch.save({"params_ema": sd}, tmp_path / "models" / f"{name}.pth")


def test_app_enhance16_and_wow_sr_16_bit(monkeypatch, tmp_path):
    import app.cnn_super_resolution as m
    from app.wow_sr import process_wow_sr
    monkeypatch.delenv("S2SR_PRECISION", raising=False)                                 # the app's default arithmetic: hp
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    e = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)
    rng = np.random.default_rng(44)
    img = rng.integers(0, 65536, size=(40, 56, 3)).astype(np.uint16)
    out = e.enhance16(img)
    with torch.no_grad():
        exp = ref.rrdbnet_forward(torch.from_numpy(net_input(img, *FULL)).permute(2, 0, 1).unsqueeze(0), tsd(6), 6)[0].permute(1, 2, 0).numpy()
    d = np.abs(out.astype(np.int64) - quantise(exp, *FULL))
    print(f"enhance16 vs oracle: max {int(d.max())} levels (bound {levels(TOL_HP, *FULL)})")
    assert out.dtype == np.uint16 and out.shape == (160, 224, 3) and d.max() <= levels(TOL_HP, *FULL)
    assert np.array_equal(e.enhance16(img, value_range=(0, 65535)), out)
    with pytest.raises(TypeError):
        e.enhance(img)                                                                  # the 8-bit door stays 8-bit
    with pytest.raises(TypeError):
        e.enhance16(img.astype(np.uint8))
    with pytest.raises(ValueError):
        e.enhance16(img, value_range=(10, 10))
    monkeypatch.setitem(m.EXTRA_MODELS, "realesrgan_x2plus", {**m.EXTRA_MODELS["realesrgan_x2plus"], "blocks": 1})
    x2 = m.RealESRGAN(model_name="realesrgan_x2plus", state_dict={k: torch.from_numpy(v) for k, v in synthetic_state_dict(1, seed=0, scale=2).items()})
    with pytest.raises(ValueError, match="x4 RRDB"):
        x2.enhance16(img)

    # a job: uint16 GeoTIFF in, uint16 GeoTIFF out
    rgb = rng.integers(100, 4000, size=(40, 56, 3)).astype(np.uint16)
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)})
    src = tmp_path / "scene16.tif"
    rio.write_geotiff_rgb16(src, rgb, geo)
    res = process_wow_sr(src, tmp_path / "wow16", enhance_crops=False, model="realesrgan_anime", bit_depth=16)
    assert set(res) == {"timestamp", "input", "outputs", "sr_metadata"} and res["outputs"]["sr_png"] is None
    meta = res["sr_metadata"]
    lo, hi = int(rgb.min()), int(rgb.max())
    assert meta["bit_depth"] == 16 and meta["value_range"] == [lo, hi]
    assert meta["original_size"] == [40, 56] and meta["output_size"] == [160, 224] and meta["scale"] == 4
    assert json.load(open(tmp_path / "wow16" / "scene16_wow_sr_metadata.json"))["sr_metadata"] == meta
    arr, tv = tiff_lite.read_tiff(res["outputs"]["sr_tif"])
    assert arr.dtype == np.uint16 and arr.shape == (160, 224, 3)
    want = e.enhance16(np.ascontiguousarray(rgb[:, :, ::-1]), value_range=(lo, hi))[:, :, ::-1]
    assert np.array_equal(arr, want) and arr.min() >= lo and arr.max() <= hi
    assert tuple(tv[rio.TAG_PIXEL_SCALE])[:2] == (2.5, 2.5) and tuple(tv[rio.TAG_TIEPOINT]) == geo.tags[rio.TAG_TIEPOINT]
    assert not (tmp_path / "wow16" / "scene16_wow_sr.png").exists()
    with pytest.raises(ValueError, match="enhance_crops"):
        process_wow_sr(src, tmp_path / "wow16b", enhance_crops=True, model="realesrgan_anime", bit_depth=16)
    src8 = tmp_path / "scene8.tif"
    rio.write_geotiff_rgb(src8, (rgb >> 4).astype(np.uint8), geo)
    with pytest.raises(ValueError, match="uint16"):
        process_wow_sr(src8, tmp_path / "wow16c", enhance_crops=False, model="realesrgan_anime", bit_depth=16)
    # bit_depth=8 on the same file: today's route and bytes (min-max to u8, BGR through the net, RGB back)
    res8 = process_wow_sr(src, tmp_path / "wow8", enhance_crops=False, model="realesrgan_anime", bit_depth=8)
    res8d = process_wow_sr(src, tmp_path / "wow8d", enhance_crops=False, model="realesrgan_anime")
    u8, _ = rio.read_rgb_u8(src)
    want8 = e.enhance_job(u8, None)
    for r in (res8, res8d):
        got, g4 = rio.read_rgb_u8(r["outputs"]["sr_tif"])
        png, _ = rio.read_rgb_u8(r["outputs"]["sr_png"])
        assert got.dtype == np.uint8 and np.array_equal(got, want8) and np.array_equal(png, want8) and g4.pixel_size == (2.5, 2.5)
        assert "bit_depth" not in r["sr_metadata"]
    assert open(res8["outputs"]["sr_tif"], "rb").read() == open(res8d["outputs"]["sr_tif"], "rb").read()
