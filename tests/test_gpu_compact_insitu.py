"""SRVGGNetCompact IN SITU on the MI355X: one batch through the production schedule (s2sr_debug_compact_taps: forward_dev ->
run_net_compact with the handle's weights, no graph), and everything it stored judged by tests/compact_insitu.py -- every conv
0 .. num_conv recomputed in float64 from the stored activation it read, the last conv with the pixel-shuffle tail and the base
from the stored p0, out_u8 byte for byte from the device's own out_f32, p0 against the input bit for bit, zeros outside the live
pixels.  tests/test_compact_insitu_cpu.py shows the judge fails a wrong layer's slopes / bias / weights, a wrong sub-pixel,
colour or byte order, a wrong base, a wrong rounding and a store 0.75 fp16 quanta off.

  1. all layers of both depths (num_conv 32 on 2 x 40 x 56, 16 on 5 x 37 x 45: the batches whose every channel is known to go
     negative at every layer), eight taps per call, consecutive calls overlapping in one layer that must come back byte-identical;
  2. the shape classes of SHAPES (modelled on test_gpu_trunk_insitu.SHAPES; the hook accepts every one of them as listed: each is
     one launch group and one mosaic segment) -- all layers on the small ones, {0, 1, 16, num_conv, last} on the large ones;
     both routes of px_live are taken (printed per case): multiply-high by 37 x 53 and 276 x 276 windows, modulo by 20 x 20 and
     24 x 40;
  3. off-grid float input at network level;
  4. degenerate image sizes through enhance, and shape changes on one engine (workspace reuse, graphs);
  5. guard bytes around the device outputs.

s2sr_forward_f32 quantises its input to fp16(fp32(255 x)) (pack_f32_nchw_kernel): off the u8 grid that moves an input above 0.5
by up to 0.0625 / 255 = 2.5e-4, which the tail's base add carries to the output.  Measured (MI355X, the golden's seeded weights,
uniform random floats, max-abs against the float64 checker): fed the same floats, (i) 4.98e-4 at num_conv 16 and 3.42e-4 at 32
(the CPU emulation of the formats: 5.4e-4 / 3.4e-4) -- inside the project's 1e-3, so it is asserted; fed p0 / 255, what the device
read, (ii) 3.1e-4 / 1.31e-4.
Measured worst |err| / bound over all cases, layers 0 .. num_conv: interior 0.997, last partial patch row / column 0.997, border
ring 0.996, next to a separator 0.995 (all of it the fp16 store's own rounding: the bound is half a quantum plus an accumulation
tolerance some 100x smaller); the last conv 0.76.  275 layers judged in 46 hook calls over 18 batches; the module runs in 17 s.

Found by this module: pack_f32_nchw_kernel's `(f16)(x * 255)` was compiled to one v_fma_mixlo_f16, which rounds the exact product
once; x = 0.21868873f packed as 55.78125 where fp16(fp32(255 x)) is 55.75 (case f32u_2x37x53, 1 of 11766 values).  The kernel
now keeps the fp32 product (csrc/pack.hip); on the u8 grid both roundings agree (test_compact_insitu_cpu.py)."""
from __future__ import annotations

import time

import numpy as np
import pytest
import torch

import compact_insitu as ci
import gpu_engines
import compact_model as cm
from s2sr import native
from compact_insitu import NO_NEGATIVE_GUARD, SHAPES, shape_inputs
from s2sr import weights as W

pytestmark = pytest.mark.gpu

TOL = 1e-3            # the project's tolerance against the fp32-class reference (test_gpu_compact.TOL)
U8_CAP = 0.04         # test_gpu_compact.U8_CAP
HP = native.PREC_F16_HP
_WORST = {}           # region -> (ratio, case), over the module's cases
_COUNT = {"layers": 0, "cases": 0, "t0": None}


@pytest.fixture(autouse=True)
def _clock():
    if _COUNT["t0"] is None:
        _COUNT["t0"] = time.time()


ROUTES = {"ragged_2x37x53": "multiply-high", "aoi_3x276x276": "multiply-high", "mosaic_9x20x20": "modulo", "dead_7of9x20x20": "modulo",
          "mosaic_16x24x40": "modulo"}


def _fresh(monkeypatch, nc, env, sd):
    return gpu_engines.fresh(monkeypatch, env, nc, HP, arch="compact", sd=sd)


def _note(title, rep, seen=()):
    print("\n" + rep.text(title))
    _COUNT["layers"] += len(set(rep.judged) - set(seen))
    _COUNT["cases"] += 1
    for r, v in rep.worst().items():
        if v is not None and v > _WORST.get(r, (0.0, ""))[0]:
            _WORST[r] = (v, title)


def _windows(nc, step=7):
    """tap lists of eight layers, consecutive ones sharing a layer: [0..7], [7..14], ... up to num_conv"""
    out, a = [], 0
    while True:
        out.append(list(range(a, min(a + step, nc) + 1)))
        if a + step >= nc:
            return out
        a += step


def _judge_all_layers(e, sd, nc, B, th, tw, hook_kw, judge_kw, title, need_negative=True):
    """every layer 0 .. num_conv + 1 through the judge, eight taps per hook call; the overlapping layer and both outputs byte-identical
    between calls"""
    judged, prev = set(), None
    for layers in _windows(nc):
        geo, acts, p0, of32, ou8 = e.debug_compact_taps(layers, **hook_kw)
        rep = ci.judge(geo, acts, p0, of32, ou8, sd, B, th, tw, need_negative=need_negative, **judge_kw)
        _note(f"{title} layers {layers[0]}..{layers[-1]}", rep, judged)
        assert not rep.fails, rep.message()
        judged |= set(rep.judged)
        if prev is not None:
            assert np.array_equal(prev[0], acts[layers[0]]), f"layer {layers[0]} differs between two hook calls"
            assert np.array_equal(prev[1], p0) and np.array_equal(prev[2], of32) and np.array_equal(prev[3], ou8), "the run is not deterministic"
        prev = (acts[layers[-1]], p0, of32, ou8)
    assert judged == set(range(nc + 2)), sorted(set(range(nc + 2)) - judged)
    return geo, prev[2], prev[3]


# ---- 1. all layers, both depths ------------------------------------------------------------------------------------------------
def test_tap_windows():
    assert _windows(16) == [list(range(0, 8)), list(range(7, 15)), [14, 15, 16]]
    assert [w[0] for w in _windows(32)] == [0, 7, 14, 21, 28] and _windows(32)[-1] == [28, 29, 30, 31, 32]
    assert all(len(w) <= native.COMPACT_TAPS_MAX for nc in (16, 32) for w in _windows(nc))


@pytest.mark.parametrize("nc,B,th,tw", [(32, 2, 40, 56), (16, 5, 37, 45)])
def test_every_layer_in_situ(nc, B, th, tw, monkeypatch):
    """Body conv k runs on layer k's weights, bias and slopes, on the right ping-pong buffer, for every k; the last conv and the
    u8 packing on real data.  The taps change nothing: the hook's outputs are forward_f32 / forward_batch_u8 of the same handle."""
    sd = ci.insitu_sd(nc)
    e = _fresh(monkeypatch, nc, {}, sd)
    tiles = ci.insitu_tiles(nc + B, B, th, tw)
    _, of32, ou8 = _judge_all_layers(e, sd, nc, B, th, tw, dict(tiles=tiles), dict(tiles=tiles), f"num_conv {nc} {B}x{th}x{tw}")
    assert np.array_equal(e.forward_f32((tiles.astype(np.float32) / 255.0).transpose(0, 3, 1, 2)), of32)
    assert np.array_equal(e.forward_batch_u8(tiles), ou8)
    e.close()


# ---- 2. shape classes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shape_classes(shape, monkeypatch):
    kind, B, th, tw, job, env, every = SHAPES[shape]
    nc = 16 if every else 32
    sd = ci.insitu_sd(nc)
    e = _fresh(monkeypatch, nc, env, sd)
    hook_kw, judge_kw = shape_inputs(shape)
    guard = shape not in NO_NEGATIVE_GUARD
    t0 = time.time()
    if every:
        geo, of32, ou8 = _judge_all_layers(e, sd, nc, B, th, tw, hook_kw, judge_kw, shape, need_negative=guard)
    else:
        mid = 16
        geo, acts, p0, of32, ou8 = e.debug_compact_taps([0, 1, mid - 1, mid, nc - 1, nc], **hook_kw)
        rep = ci.judge(geo, acts, p0, of32, ou8, sd, B, th, tw, need_negative=guard, **judge_kw)
        _note(shape, rep)
        assert rep.judged == [0, 1, mid, nc, nc + 1] and not rep.fails, rep.message()
    route = ci.px_live_route(geo)
    print(f"{shape}: n {geo['n']} images of {geo['H']} x {geo['W']} in planes {geo['Hp']} x {geo['Wp']}, mosaic {geo['mos_kx']} x {geo['mos_ky']}, "
          f"px_live route: {route}; {time.time() - t0:.1f} s")
    assert route == ROUTES.get(shape, "no mosaic")
    if kind == "u8":
        if job == 0:
            assert np.array_equal(e.forward_batch_u8(hook_kw["tiles"]), ou8), "hook u8 output differs from forward_batch_u8"
    else:
        assert np.array_equal(e.forward_f32(hook_kw["x"]), of32), "hook f32 output differs from forward_f32"
    e.close()


def test_both_px_live_routes_are_listed():
    assert {"multiply-high", "modulo"} <= set(ROUTES.values())
    for shape, route in ROUTES.items():
        _, B, th, tw, job = SHAPES[shape][:5]
        kx, ky = native.pick_mosaic(max(B, job), th, tw)
        assert kx * ky > 1, shape
        assert route == ("multiply-high" if th + 1 >= 32 and tw + 1 >= 32 else "modulo")


# ---- 3. off-grid floats at network level -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [16, 32])
def test_off_grid_floats_at_network_level(nc, monkeypatch):
    """forward_f32 on uniform random floats against the float64 checker fed (ii) p0 / 255, what the device read -- held to TOL --
    and (i) the same floats: the entry quantises its input to fp16(255 x) (include/s2sr.h says so), which is worth up to 2.5e-4
    at the input.  (i) is printed and recorded in the module docstring."""
    sd = W.synthetic_compact_state_dict(nc, seed=0)
    e = _fresh(monkeypatch, nc, {}, sd)
    worst = [0.0, 0.0]
    for B, th, tw in ((2, 37, 53), (1, 64, 64)):
        x = np.random.default_rng(100 + th).random((B, 3, th, tw), dtype=np.float32)
        geo, _, p0, of32, _ = e.debug_compact_taps([0], x=x)
        y = e.forward_f32(x)
        assert np.array_equal(y, of32)
        read = p0[:, :3, 1:1 + th, 1:1 + tw]
        assert np.array_equal(read, ci.expected_p0(geo, B, th, tw, x=x)[:, :, 1:1 + th, 1:1 + tw])
        err_i = float(np.abs(y - cm.forward(torch.from_numpy(x), sd).numpy()).max())
        err_ii = float(np.abs(y - cm.forward(torch.from_numpy(read).double() / 255.0, sd).numpy()).max())
        dx = float(np.abs(read.astype(np.float64) / 255.0 - x).max())
        print(f"num_conv {nc} {B}x{th}x{tw} off-grid floats: (i) against the same floats {err_i:.3g}, (ii) against p0 / 255 {err_ii:.3g}; "
              f"input moved by up to {dx:.3g}")
        worst = [max(worst[0], err_i), max(worst[1], err_ii)]
        assert err_ii <= TOL
        assert err_i <= TOL      # the CPU emulation of the same formats gives 5.4e-4 / 3.4e-4 here: inside the tolerance, so it is held to it
    print(f"num_conv {nc}: worst (i) {worst[0]:.3g}, (ii) {worst[1]:.3g}")
    e.close()


# ---- 4. degenerate and changing shapes ---------------------------------------------------------------------------------------------
def _engine(nc):
    return gpu_engines.default(nc, HP, arch="compact")


@pytest.mark.parametrize("H,Wd", [(1, 1), (1, 7), (5, 1), (2, 3), (3, 33), (33, 2)])
def test_degenerate_image_sizes(H, Wd):
    sd, e = W.synthetic_compact_state_dict(32, seed=0), _engine(32)
    img = np.random.default_rng(1000 * H + Wd).integers(0, 256, (H, Wd, 3), dtype=np.uint8)
    exp_f = cm.enhance_float(img, sd, 256, 10)
    f = e.enhance_f32(img, tile=256, pad=10)
    err = float(np.abs(f - exp_f).max())
    out = e.enhance_u8(img, tile=256, pad=10)
    mx, share, ok = cm.u8_cap_check(out, cm.quantise(exp_f), U8_CAP)
    print(f"{H} x {Wd}: max-abs {err:.3g}; u8 max {mx}, share {share:.4f}")
    assert f.shape == (4 * H, 4 * Wd, 3) and out.shape == (4 * H, 4 * Wd, 3)
    assert err <= TOL and ok
    assert np.array_equal(out, ci.quantise_f32(f.transpose(2, 0, 1)[None])[0])            # the two entries agree to the byte


def test_shape_changes_keep_the_workspace_clean(monkeypatch):
    """One engine through batches of changing geometry, every visit three sightings (direct, graph capture, graph replay), every
    sighting held to the bytes a fresh engine gives for that batch alone.  ensure_workspace keeps its planes only while the image
    geometry and the mosaic period stay and the group does not grow, so the visits are ordered to make it reuse them:
      31 windows of 40 x 40 (a full 6 x 5 mosaic and a remainder mosaic inside the full one's planes), 30 of them (the full
      mosaic alone: the remainder's planes are stale now), 31 again;
      20 tiles of 32 x 32 (no mosaic, two groups of 16 and 4), 3 of them (a group of 3 inside the planes of 16), 20 again;
      three tiles of 24 x 24 (no mosaic, smaller planes);
      seven 60 x 84 windows (one 7 x 1 mosaic), a single one (no mosaic: the planes are allocated anew), seven again;
      22 windows of 40 x 40 (eleven 2 x 1 mosaics in one group: another period than the 6 x 5 plan's images)."""
    sd = W.synthetic_compact_state_dict(16, seed=0)
    rng = np.random.default_rng(31)
    shapes = {"a31": (31, 40, 40), "a30": (30, 40, 40), "b20": (20, 32, 32), "b3": (3, 32, 32), "e3": (3, 24, 24),
              "c7": (7, 60, 84), "c1": (1, 60, 84), "d22": (22, 40, 40)}
    batches = {k: rng.integers(0, 256, s + (3,), dtype=np.uint8) for k, s in shapes.items()}
    assert native.pick_mosaic(31, 40, 40) == (6, 5) and native.pick_mosaic(30, 40, 40) == (6, 5) and native.pick_mosaic(7, 60, 84) == (7, 1)
    assert native.pick_mosaic(22, 40, 40) == (2, 1) and native.pick_mosaic(20, 32, 32) == (1, 1) and native.pick_mosaic(3, 24, 24) == (1, 1)
    ref = {}
    for k, b in batches.items():
        f = _fresh(monkeypatch, 16, {}, sd)
        ref[k] = f.forward_batch_u8(b).copy()
        f.close()
    e = _fresh(monkeypatch, 16, {}, sd)
    first_visit = set()
    for k in ("a31", "a30", "a31", "b20", "b3", "b20", "e3", "c7", "c1", "c7", "d22"):
        cap0, rep0 = e.graph_stats()
        for sighting in range(3):
            assert np.array_equal(e.forward_batch_u8(batches[k]), ref[k]), f"batch {k}, sighting {sighting}"
        cap, rep = e.graph_stats()
        print(f"{k}: graphs captured {cap - cap0}, replays {rep - rep0}")
        assert rep > rep0, f"batch {k}: no graph replayed by the third sighting"
        if k not in first_visit and k != "a30":       # a30's one launch group is a31's first segment: the same graph, replayed
            assert cap > cap0, f"batch {k}: no graph captured on the second sighting"
        first_visit.add(k)
    e.close()


# ---- 5. guard bytes ------------------------------------------------------------------------------------------------------------------
FRONT, BACK, FILL = 4100, 4096, 0x5A     # the output starts 4-byte aligned and no better: all the tail's u8 stores promise


@pytest.mark.parametrize("B,th,tw", [(1, 9, 35), (5, 37, 45), (6, 276, 276)])
def test_guard_bytes_around_the_device_output(B, th, tw):
    e = _engine(16)
    tiles = np.random.default_rng(B + th).integers(0, 256, (B, th, tw, 3), dtype=np.uint8)
    exp = e.forward_batch_u8(tiles).copy()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    x = torch.from_numpy(tiles).to(dev)
    per = 16 * th * tw * 3
    buf = torch.full((FRONT + B * per + BACK,), FILL, dtype=torch.uint8, device=dev)
    out = buf[FRONT:FRONT + B * per]
    e.forward_batch_u8_dev(x.data_ptr(), B, th, tw, out.data_ptr(), st)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:FRONT] == FILL).all() and (got[FRONT + B * per:] == FILL).all(), "forward_batch_u8_dev wrote outside its output"
    assert np.array_equal(got[FRONT:FRONT + B * per].reshape(exp.shape), exp)
    # a part of a job: the last `part` tiles of B land in their own slice, everything in front of it stays untouched
    part = 2 if B > 2 else 1
    buf.fill_(FILL)
    first = B - part
    e.forward_part_u8_dev(x[first:].data_ptr(), part, th, tw, B, out[first * per:].data_ptr(), st)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:FRONT + first * per] == FILL).all(), "forward_part_u8_dev wrote in front of its tiles"
    assert (got[FRONT + B * per:] == FILL).all(), "forward_part_u8_dev wrote behind its output"
    assert np.array_equal(got[FRONT + first * per:FRONT + B * per].reshape(exp[first:].shape), exp[first:])


# ---- the module's figures ------------------------------------------------------------------------------------------------------------
def test_zz_summary():
    """run last in this module: the worst ratio per region over all cases, the number of layers judged, the wall time"""
    print(f"\nlayers judged: {_COUNT['layers']} in {_COUNT['cases']} hook calls; module wall time {time.time() - _COUNT['t0']:.0f} s")
    for r in ci.REGIONS:
        if r in _WORST:
            print(f"worst |err| / bound, {r}: {_WORST[r][0]:.3f} ({_WORST[r][1]})")
    assert all(v[0] <= 1.0 for v in _WORST.values())
    gpu_engines.close_default(arch="compact")
