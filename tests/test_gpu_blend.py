"""The seam-blended stitch on the GPU (include/s2sr.h: s2sr_enhance_blend_u8, s2sr_enhance_blend_u16) and its Python seam
(RealESRGAN(seam_blend=True), process_wow_sr(seam_blend=True)).

The definition is fixed and restated in tests/blend_model.py from oracle.rrdbnet_ref.tile_plan alone.  The device image is held to
it bit for bit: the distinct windows are cut on the host, run through forward_f32 as one batch (a window's bytes do not depend on
how it is batched: tests/test_gpu_net.py test_batch_consistency_and_group_invariance, tests/test_gpu_tiles.py
test_window_mosaics_give_the_same_bytes) and blended in numpy float32.  1-block nets, tile 16."""
import functools
import json

import numpy as np
import pytest
import torch

import blend_model as bm
import gpu_engines
import probe_model as pm
from oracle import rrdbnet_ref as ref
from s2sr import native
from s2sr import rasterio_lite as rio
from s2sr.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

TOL_F16, TOL_HP = 2.5e-3, 3e-4                     # tests/test_gpu_net.py's constants for the same nets
F16, HP = native.PREC_F16, native.PREC_F16_HP
MODES = [(HP, TOL_HP), (F16, TOL_F16)]
BANDED = (100, 90, 16, 2)        # one chunk, a 6 x 6 mosaic
CHUNKED = (53, 200, 16, 3)       # three chunks of one window row: the carry; shortened column ramps
IMAGES = [BANDED, CHUNKED, (130, 37, 16, 2), (39, 39, 16, 3)]      # the last: shortened ramps on both axes
assert native.pick_mosaic(39, 22, 22) == (1, 1) and native.plan_chunks(3, 1, 13, 1, 1, 256) == [1, 1, 1]


def quantise(y, lo, hi):
    """The 16-bit door's output rule, restated."""
    return lo + np.rint(np.clip(y, 0, 1).astype(np.float32) * np.float32(hi - lo)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def image(H, W, seed=7):
    a = np.random.default_rng(seed + 1000 * H + W).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def cut(img, tile, pad, scale=4):
    """The job's distinct windows [T, wh, ww, 3], cut on the host (scale 2: from the reflect-padded image), and the model's tables."""
    src = pm.reflect_even(np.asarray(img)) if scale == 2 else np.asarray(img)
    PH, PW = src.shape[:2]
    rects, _ = bm.distinct_rects(PH, PW, tile, pad, scale)
    rows, cols, ys, xs = bm.tables(PH, PW, tile, pad, scale)
    return np.stack([src[y1:y2, x1:x2] for y1, y2, x1, x2 in rects]), rows, cols, len(xs)


def window_floats(e, wins):
    """The engine's own float output of every window, [T, S wh, S ww, 3]."""
    x = np.ascontiguousarray((wins.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))
    return np.ascontiguousarray(e.forward_f32(x).transpose(0, 2, 3, 1))


def same(got, want, what):
    why = pm.first_difference(got, want)
    assert not why, f"{what}: {why}"


# ---- bit for bit against the model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,tile,pad", IMAGES)
@pytest.mark.parametrize("prec", [HP, F16])
def test_float_image_is_the_model_bit_for_bit(prec, H, W, tile, pad):
    e = gpu_engines.default(1, prec)
    img = image(H, W)
    u8, f = e.enhance_blend_u8(img, tile=tile, pad=pad, want_f32=True)
    wins, rows, cols, nx = cut(img, tile, pad)
    wf = window_floats(e, wins)
    want = bm.blend(wf, rows, cols, nx)
    d = np.abs(f - want)
    print(f"{H}x{W} {tile}/{pad} prec {prec}: {int((f != want).sum())} of {f.size} floats differ from the model, max {float(d.max()):.3e}")
    assert f.shape == (4 * H, 4 * W, 3) and np.array_equal(f, want), pm.first_difference(f, want)
    oh, ow = wf.shape[1:3]
    for wr, wc in ((bm.reversed_weights(rows), bm.reversed_weights(cols)), (bm.shifted_ramp(rows, oh), bm.shifted_ramp(cols, ow)),
                   (bm.reversed_weights(rows), cols), (rows, bm.shifted_ramp(cols, ow))):
        assert not np.array_equal(f, bm.blend(wf, wr, wc, nx))                   # the controls: two wrong models do not match
    # relations to the default door
    ramp = bm.in_ramp(rows, cols)
    plain = e.enhance_f32(img, tile=tile, pad=pad)
    assert ramp.any() and not ramp.all() and np.array_equal(f[~ramp], plain[~ramp]) and (f[ramp] != plain[ramp]).any()
    same(u8, bm.quant_u8(f), "out_u8 against the truncation of out_f32")
    if prec == HP:
        assert np.array_equal(u8[~ramp], e.enhance_u8(img, tile=tile, pad=pad)[~ramp])
    # without the float image the chunks' bands are pasted as they become final (the carried window row): the same bytes
    same(e.enhance_blend_u8(img, tile=tile, pad=pad), u8, "banded u8 against the one-chunk u8")


@pytest.mark.parametrize("prec", [HP, F16])
def test_pad_0_and_an_untiled_image_are_the_default_doors(prec):
    e = gpu_engines.default(1, prec)
    for img, kw in ((image(53, 200), dict(tile=16, pad=0)), (image(100, 90), dict(tile=16, pad=0)), (image(28, 36), dict())):
        u8, f = e.enhance_blend_u8(img, want_f32=True, **kw)
        assert np.array_equal(f, e.enhance_f32(img, **kw)) and np.array_equal(u8, e.enhance_u8(img, **kw))
        assert np.array_equal(e.enhance_blend_u8(img, **kw), u8)
    img16 = image(28, 36).astype(np.uint16) * 257
    assert np.array_equal(e.enhance_blend_u16(img16), e.enhance_u16(img16))


@pytest.mark.parametrize("lo,hi", [(0, 65535), (1000, 11000)])
@pytest.mark.parametrize("prec", [HP, F16])
def test_u16_door(prec, lo, hi):
    e = gpu_engines.default(1, prec)
    for H, W, tile, pad in (BANDED, CHUNKED):
        img = np.random.default_rng(H).integers(0, 13000 if hi < 65535 else 65536, size=(H, W, 3)).astype(np.uint16)
        q, f = e.enhance_blend_u16(img, lo, hi, tile=tile, pad=pad, want_f32=True)
        assert q.dtype == np.uint16 and np.array_equal(q, quantise(f, lo, hi))
        same(e.enhance_blend_u16(img, lo, hi, tile=tile, pad=pad), q, "banded u16 against the one-chunk u16")
        rects, _ = bm.distinct_rects(H, W, tile, pad, 4)
        rows, cols, ys, xs = bm.tables(H, W, tile, pad, 4)
        wins = np.stack([img[y1:y2, x1:x2] for y1, y2, x1, x2 in rects])
        wf = np.ascontiguousarray(e.forward_batch_u16(wins, lo, hi, want_f32=True)[1].transpose(0, 2, 3, 1))
        assert np.array_equal(f, bm.blend(wf, rows, cols, len(xs)))
        ramp = bm.in_ramp(rows, cols)
        assert np.array_equal(q[~ramp], e.enhance_u16(img, lo, hi, tile=tile, pad=pad)[~ramp])


# ---- accuracy --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_blend(H, W, tile, pad):
    """The oracle's own per-window outputs, blended by the model."""
    wins, rows, cols, nx = cut(image(H, W), tile, pad)
    x = torch.from_numpy(np.ascontiguousarray((wins.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)))
    with torch.no_grad():
        y = ref.rrdbnet_forward(x, ref.to_torch_sd(synthetic_state_dict(1, seed=0)), 1).numpy()
    out = bm.blend(np.ascontiguousarray(y.transpose(0, 2, 3, 1)).astype(np.float32), rows, cols, nx)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("prec,tol", MODES)
def test_accuracy_against_the_blended_oracle(prec, tol):
    """A convex combination cannot exceed its inputs' error: the mode's tolerance of the plain doors holds."""
    e = gpu_engines.default(1, prec)
    for H, W, tile, pad in (BANDED, CHUNKED):
        _, f = e.enhance_blend_u8(image(H, W), tile=tile, pad=pad, want_f32=True)
        err = float(np.abs(f - oracle_blend(H, W, tile, pad)).max())
        print(f"blend {H}x{W} prec {prec}: float err {err:.3e} (bound {tol:.1e})")
        assert err <= tol


# ---- probe nets: windows that differ by whole grey levels along their borders --------------------------------------------------------
def probe_checks(e, img, tile, pad, scale):
    u8 = e.enhance_blend_u8(img, tile=tile, pad=pad)
    wins, rows, cols, nx = cut(img, tile, pad, scale)
    H, W = img.shape[:2]
    # compact nets add the input to the output: a window's floats come from the u8 door there (each window a whole image)
    wf = np.stack([e.enhance_f32(w, tile=256) for w in wins]) if e.arch == "compact" else window_floats(e, wins)
    want = bm.quant_u8(bm.blend(wf, rows, cols, nx))[:scale * H, :scale * W]
    same(u8, want, ("blend against the model on the engine's window floats", img.shape, tile, pad, scale))
    ramp = bm.in_ramp(rows, cols)[:scale * H, :scale * W]
    paste = e.enhance_u8(img, tile=tile, pad=pad)
    assert np.array_equal(u8[~ramp], paste[~ramp])
    return bool((u8[ramp] != paste[ramp]).any())      # (a shortened ramp may not reach the border pixels the windows differ in)


@pytest.mark.parametrize("prec", [HP, F16])
def test_probe_net_x4(monkeypatch, prec):
    e = gpu_engines.fresh(monkeypatch, {}, 1, prec, sd=pm.probe_state_dict(1, tap=(0, 2)))
    try:
        differs = [probe_checks(e, pm.coded(H, W), tile, pad, 4) for H, W, tile, pad in IMAGES]
        assert differs[:3] == [True] * 3, differs                # full-width ramps reach the windows' borders
    finally:
        e.close()


def test_probe_net_x2_odd_image_and_compact(monkeypatch):
    e = gpu_engines.fresh(monkeypatch, {}, 1, HP, scale=2, sd=pm.probe_state_dict(1, scale=2, tap=(2, 0), sub=(1, 0)))
    try:
        sizes = ((53, 91, 16, 3), (39, 39, 16, 3), (100, 37, 16, 2))                     # reflect pad, ramps cropped at the far edges
        assert any([probe_checks(e, pm.coded(H, W), tile, pad, 2) for H, W, tile, pad in sizes])
    finally:
        e.close()
    e = gpu_engines.fresh(monkeypatch, {}, 16, HP, arch="compact", sd=pm.compact_probe_state_dict(16, (0, 2)))
    try:
        assert probe_checks(e, pm.coded(37, 45) >> 1, 16, 2, 4) and probe_checks(e, pm.coded(53, 200) >> 1, 16, 3, 4)
        with pytest.raises(native.S2srError, match="S2SR_ARCH_COMPACT"):
            e.enhance_blend_u16(np.zeros((53, 200, 3), np.uint16), tile=16, pad=3)
        assert np.array_equal(e.enhance_blend_u8(pm.coded(20, 20)), e.enhance_u8(pm.coded(20, 20)))
    finally:
        e.close()


# ---- the job route -----------------------------------------------------------------------------------------------------------------
def test_job_route_on_the_three_chunk_image():
    e = gpu_engines.default(1, HP)
    H, W, tile, pad = CHUNKED
    rgb = image(H, W, seed=11)
    plain = e.enhance_blend_u8(np.ascontiguousarray(rgb[..., ::-1]), tile=tile, pad=pad)[..., ::-1]
    same(e.enhance_blend_u8(rgb, swap_rb=True, tile=tile, pad=pad), plain, "swap_rb without a post-process")
    for prm in (native.pp_wow(), native.pp_farm()):
        want = e.postprocess_u8(np.ascontiguousarray(plain), prm)
        same(e.enhance_blend_u8(rgb, prm=prm, swap_rb=True, tile=tile, pad=pad), want, "the job against its separate steps")
    same(e.enhance_blend_u8(rgb, prm=native.pp_wow(), tile=tile, pad=pad),
         e.postprocess_u8(e.enhance_blend_u8(rgb, tile=tile, pad=pad), native.pp_wow()), "a post-process without the swap")
    H, W, tile, pad = BANDED                                                             # one chunk
    rgb = image(H, W, seed=12)
    want = e.postprocess_u8(np.ascontiguousarray(e.enhance_blend_u8(np.ascontiguousarray(rgb[..., ::-1]), tile=tile, pad=pad)[..., ::-1]), native.pp_wow())
    same(e.enhance_blend_u8(rgb, prm=native.pp_wow(), swap_rb=True, tile=tile, pad=pad), want, "the one-chunk job")


# ---- hygiene -----------------------------------------------------------------------------------------------------------------------
def test_repeats_replay_graphs_and_leave_the_default_doors_alone(monkeypatch):
    e = gpu_engines.fresh(monkeypatch, {}, 1, HP)
    try:
        H, W, tile, pad = CHUNKED
        img, img16 = image(H, W), image(H, W).astype(np.uint16) * 257
        batch = np.ascontiguousarray(image(40, 44)[None].repeat(3, 0))
        before = (e.enhance_u8(img, tile=tile, pad=pad).copy(), e.enhance_u16(img16, tile=tile, pad=pad).copy(), e.forward_batch_u8(batch).copy())
        first = e.enhance_blend_u8(img, tile=tile, pad=pad).copy()
        r0 = e.graph_stats()[1]
        for _ in range(2):
            assert np.array_equal(e.enhance_blend_u8(img, tile=tile, pad=pad), first)
        assert e.graph_stats()[1] > r0, e.graph_stats()
        q = e.enhance_blend_u16(img16, tile=tile, pad=pad).copy()
        assert np.array_equal(e.enhance_blend_u16(img16, tile=tile, pad=pad), q)
        e.enhance_blend_u8(img, prm=native.pp_wow(), swap_rb=True, tile=tile, pad=pad)
        after = (e.enhance_u8(img, tile=tile, pad=pad), e.enhance_u16(img16, tile=tile, pad=pad), e.forward_batch_u8(batch))
        for b, a in zip(before, after):
            assert np.array_equal(b, a)
    finally:
        e.close()


def test_refusals_leave_the_engine_working():
    e = gpu_engines.default(1, HP)
    H, W, tile, pad = BANDED
    img = image(H, W)
    want = e.enhance_blend_u8(img, tile=tile, pad=pad).copy()
    lib, h, p = e._lib, e._h, native._ptr
    out, f = np.empty((4 * H, 4 * W, 3), np.uint8), np.empty((4 * H, 4 * W, 3), np.float32)
    prm = native.pp_wow()
    import ctypes as C
    assert lib.s2sr_enhance_blend_u8(h, p(img), H, W, tile, pad, None, 0, None, None) != 0                 # no output
    assert lib.s2sr_enhance_blend_u8(h, p(img), H, W, tile, pad, C.byref(prm), 0, p(out), p(f)) != 0       # the float image of a job
    assert lib.s2sr_enhance_blend_u8(h, p(img), H, W, tile, pad, None, 1, p(out), p(f)) != 0
    assert lib.s2sr_enhance_blend_u8(h, p(img), H, W, tile, pad, C.byref(prm), 1, None, None) != 0
    assert lib.s2sr_enhance_blend_u8(h, None, H, W, tile, pad, None, 0, p(out), None) != 0
    img16 = img.astype(np.uint16)
    assert lib.s2sr_enhance_blend_u16(h, p(img16), H, W, tile, pad, 0, 65535, None, None) != 0
    for lo, hi in ((10, 10), (-1, 100), (0, 65536), (500, 100)):
        with pytest.raises(native.S2srError):
            e.enhance_blend_u16(img16, lo, hi, tile=tile, pad=pad)
    x2 = gpu_engines.default(1, HP, scale=2)
    with pytest.raises(native.S2srError) as today:
        x2.enhance_u16(img16, tile=tile, pad=pad)
    with pytest.raises(native.S2srError) as blend:
        x2.enhance_blend_u16(img16, tile=tile, pad=pad)
    assert str(blend.value).split(":", 1)[1] == str(today.value).split(":", 1)[1]                        # today's message
    with pytest.raises(native.S2srError, match="even tile"):
        x2.enhance_blend_u8(img, tile=15, pad=2)
    with pytest.raises(TypeError):
        e.enhance_blend_u16(img)
    assert np.array_equal(e.enhance_blend_u8(img, tile=tile, pad=pad), want)


def test_two_threads_on_one_handle_get_the_bytes_of_calls_made_alone(monkeypatch):
    """A whole-image call holds the handle's lock from its checks to its last synchronise (engine_aoi.hip enhance_call): the
    scratch areas, the carry buffer and the tables of a three-chunk blend call are not another thread's to rewrite in between."""
    import threading
    e = gpu_engines.fresh(monkeypatch, {}, 1, HP)
    try:
        H, W, tile, pad = CHUNKED
        img, img16 = image(H, W), image(H, W).astype(np.uint16) * 257
        calls = {"blend_u8": lambda: e.enhance_blend_u8(img, tile=tile, pad=pad), "u8": lambda: e.enhance_u8(img, tile=tile, pad=pad),
                 "blend_u16": lambda: e.enhance_blend_u16(img16, tile=tile, pad=pad)}
        alone = {k: f().copy() for k, f in calls.items()}
        got, errors = {}, []

        def run(name, seq):
            try:
                got[name] = [(k, calls[k]().copy()) for k in seq]
            except Exception as ex:       # noqa: BLE001 (reported below, on the test's thread)
                errors.append((name, repr(ex)))

        threads = [threading.Thread(target=run, args=("a", ["blend_u8"] * 3)),
                   threading.Thread(target=run, args=("b", ["u8", "blend_u16", "u8"]))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not any(t.is_alive() for t in threads) and not errors, errors
        assert [len(v) for v in got.values()] == [3, 3]
        for name, results in got.items():
            for i, (k, a) in enumerate(results):
                same(a, alone[k], f"thread {name} call {i} ({k}) against the call made alone")
        same(e.enhance_u8(img, tile=tile, pad=pad), alone["u8"], "a plain enhance_u8 afterwards")
    finally:
        e.close()


# ---- the app -----------------------------------------------------------------------------------------------------------------------
def _patch_weights(monkeypatch, tmp_path, nb_by_name):
    """Seeded synthetic checkpoints where the drop-in looks for them (tests/test_gpu_app.py)."""
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir(exist_ok=True)
    for name, nb in nb_by_name.items():
        sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(nb, seed=0).items()}
        torch.save({"params_ema": sd}, tmp_path / "models" / f"{name}.pth")


def test_app_seam_blend(monkeypatch, tmp_path):
    import app.cnn_super_resolution as m
    from app.wow_sr import process_wow_sr
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    plain = m.RealESRGAN(model_name="realesrgan_anime", tile_size=32)
    e = m.RealESRGAN(model_name="realesrgan_anime", tile_size=32, seam_blend=True)
    assert e.seam_blend is True and plain.seam_blend is False
    eng = e._engine
    img = image(70, 90, seed=21)
    assert np.array_equal(e.enhance(img), eng.enhance_blend_u8(img, tile=32, pad=10))
    assert np.array_equal(plain.enhance(img), eng.enhance_u8(img, tile=32, pad=10)) and not np.array_equal(plain.enhance(img), e.enhance(img))
    assert np.array_equal(e.enhance_job(img, native.pp_wow()), eng.enhance_blend_u8(img, native.pp_wow(), swap_rb=True, tile=32, pad=10))
    assert np.array_equal(e.enhance_job(img), eng.enhance_blend_u8(img, swap_rb=True, tile=32, pad=10))
    img16 = img.astype(np.uint16) * 40 + 100
    assert np.array_equal(e.enhance16(img16, value_range=(100, 10300)), eng.enhance_blend_u16(img16, 100, 10300, tile=32, pad=10))
    assert np.array_equal(plain.enhance16(img16, value_range=(100, 10300)), eng.enhance_u16(img16, 100, 10300, tile=32, pad=10))

    # a job: tiled at the app's 256 / 10
    rgb = image(530, 520, seed=22)
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)})
    src = tmp_path / "scene.tif"
    rio.write_geotiff_rgb(src, rgb, geo)
    on = process_wow_sr(src, tmp_path / "on", model="realesrgan_anime", seam_blend=True)
    off = process_wow_sr(src, tmp_path / "off", model="realesrgan_anime")
    off2 = process_wow_sr(src, tmp_path / "off2", model="realesrgan_anime", seam_blend=False)
    assert on["sr_metadata"]["seam_blend"] is True
    assert json.load(open(tmp_path / "on" / "scene_wow_sr_metadata.json"))["sr_metadata"]["seam_blend"] is True
    assert "seam_blend" not in off["sr_metadata"] and "seam_blend" not in off2["sr_metadata"]
    assert {k: v for k, v in on["sr_metadata"].items() if k not in ("seam_blend", "output_file")} == \
           {k: v for k, v in off["sr_metadata"].items() if k != "output_file"}
    u8, _ = rio.read_rgb_u8(src)
    got, _ = rio.read_rgb_u8(on["outputs"]["sr_tif"])
    assert np.array_equal(got, eng.enhance_blend_u8(u8, native.pp_wow(), swap_rb=True))
    got_off, _ = rio.read_rgb_u8(off["outputs"]["sr_tif"])
    assert np.array_equal(got_off, eng.enhance_job_u8(u8, native.pp_wow())) and not np.array_equal(got, got_off)
    assert open(off["outputs"]["sr_tif"], "rb").read() == open(off2["outputs"]["sr_tif"], "rb").read()
