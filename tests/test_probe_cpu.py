"""tests/probe_model.py pinned to the oracle (which tests/test_oracle_golden.py pins to the reference): with probe weights
oracle.rrdbnet_ref.enhance, tests/x2plus_model.py and tests/compact_model.py give `expected` byte for byte; the reference's paste
replayed in numpy gives tiled == whole on every plan-changing size; and the inputs of the device stitch test have the power to
tell a wrong paste from the right one."""
import numpy as np
import pytest
import torch

import compact_model as cm
import probe_model as pm
import x2plus_model as xm
from oracle import rrdbnet_ref as ref

REPLAY_TILE_PADS = [(16, 1), (16, 2), (16, 3), (32, 4)]
REPLAY_TAPS = [(1, 1), (0, 0), (2, 2)]


def _tsd(sd):
    return ref.to_torch_sd(sd)


def _same(got, want, what):
    d = pm.first_difference(got, want)
    assert not d, f"{what}: {d}"


def test_coded_images_have_distinct_neighbours():
    for H, W in [(1, 1), (1, 7), (3, 5), (64, 64), (200, 199), (300, 520)]:
        a, b = pm.coded(H, W), pm.coded_u16(H, W)
        assert a.min() >= 1 and b.min() >= 1
        assert pm.min_neighbour_gap(a) >= 1, (H, W)
        assert pm.min_neighbour_gap(b) >= 1024, (H, W)
    # the job test's image (values <= 200) keeps them apart too
    j = np.maximum(pm.coded(100, 90).astype(np.int64) * 200 // 256, 1)
    assert j.max() <= 200 and pm.min_neighbour_gap(j) >= 1


def test_all_256_values_are_their_own_output():
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    img[..., 1] = img[::-1, :, 0]
    img[..., 2] = img[:, ::-1, 0]
    q, f = ref.enhance(img, _tsd(pm.probe_state_dict(1)), 1, return_float=True)
    _same(q, pm.expected_u8(img), "256 values")
    frac = f.astype(np.float64) * 255.0 - pm.expected(img)
    assert np.abs(frac - 0.5).max() < 1e-3                   # the float oracle sits in the middle of the truncation's interval


@pytest.mark.parametrize("tap_layer", pm.TAP_LAYERS)
@pytest.mark.parametrize("tap", [(0, 0), (2, 2), (0, 2), (1, 0)])
def test_shift_tap_in_each_layer_whole_and_tiled(tap_layer, tap):
    sd = _tsd(pm.probe_state_dict(1, tap_layer=tap_layer, tap=tap, out_offset=(0, 10, 20)))
    kw = dict(tap_layer=tap_layer, tap=tap, out_offset=(0, 10, 20))
    whole = pm.coded(13, 9)
    _same(ref.enhance(whole, sd, 1), pm.expected_u8(whole, **kw), "whole")
    tiled = pm.coded(37, 45)                                  # 3 x 3 windows at tile 16, pad 2
    assert pm.is_tiled(37, 45, 16)
    q = ref.enhance(tiled, sd, 1, tile_size=16, tile_pad=2)
    _same(q, pm.expected_u8(tiled, **kw), "tiled")
    _same(np.clip(pm.tiled_expected(tiled, 16, 2, **kw), 0, 255), q, "tiled replay")


@pytest.mark.parametrize("sub", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_scale_2_every_sub_pixel_channel(sub):
    for tap in [(1, 1), (2, 0)]:
        sd = _tsd(pm.probe_state_dict(1, scale=2, tap=tap, sub=sub))
        for (H, W, tile, pad) in [(12, 10, 256, 10), (7, 9, 256, 10), (45, 38, 16, 2)]:      # even, odd (reflect), tiled and odd
            img = pm.coded(H, W)
            want = pm.expected_u8(img, scale=2, tap=tap, sub=sub)
            _same(xm.enhance(img, sd, 1, tile, pad), want, (sub, tap, H, W))
            if pm.is_tiled(H, W, tile, 2):
                _same(np.clip(pm.tiled_expected(img, tile, pad, scale=2, tap=tap, sub=sub), 0, 255), want, ("replay", sub, tap))


def test_compact_probes_and_their_margin():
    """The zero net is nearest-x4 through the base add; the shift probe is u + shift(u) with integer expectation, and the device's
    arithmetic (compact_model.forward_emulated) leaves at least 0.25 LSB of margin on either side of the truncation."""
    img = (pm.coded(21, 18) >> 1)                             # <= 127: u + shift(u) stays below the clip
    big = pm.coded(37, 45) >> 1
    assert pm.min_neighbour_gap(img) >= 1
    for tap in (None, (0, 0), (2, 2), (0, 2)):
        sd = pm.compact_probe_state_dict(16, tap)
        want = pm.compact_expected(img, tap)
        assert want.max() <= 255
        _same(cm.enhance(img, sd), want, ("compact", tap))
        _same(cm.enhance(big, sd, 16, 2), pm.compact_expected(big, tap), ("compact tiled", tap))
        f = cm.enhance_float(img, sd, emulated=True).astype(np.float64) * 255.0 - want
        assert f.min() >= 0.25 and f.max() <= 0.75, (tap, float(f.min()), float(f.max()))
        _same(cm.enhance(img, sd, emulated=True), want, ("compact emulated", tap))
    allv = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    _same(cm.enhance(allv, pm.compact_probe_state_dict(16, None), emulated=True), pm.up(allv, 4), "compact 256 values")


def _replay_geometries(t, p):
    e = pm.edge_sizes(t, p)
    return [(H, W) for H in e for W in e if pm.is_tiled(H, W, t)]


def test_paste_replay_tiled_equals_whole():
    """The reference's paste with the shift probe on every pair of plan-changing sizes that takes the tiled route: an uncropped
    window side is always a true image border, so for pad >= 1 the windows' zeros never reach the output."""
    cases = 0
    for t, p in REPLAY_TILE_PADS:
        for H, W in _replay_geometries(t, p):
            img = pm.coded(H, W)
            for tap in REPLAY_TAPS:
                _same(pm.tiled_expected(img, t, p, tap=tap), pm.expected(img, tap=tap), (H, W, t, p, tap))
                cases += 1
    assert cases == 501, cases


def test_paste_replay_forced_tiling_of_small_images():
    """s2sr_tile_process_f32 runs the plan whatever the size: duplicate windows (t < H < win), H < win and 1- to 3-pixel sides
    are plans the whole / tiled switch never reaches at these tiles; the same identity holds there."""
    for t, p in [(16, 2), (32, 4)]:
        e = pm.edge_sizes(t, p)
        for H in e:
            for W in e:
                for tap in REPLAY_TAPS:
                    _same(pm.tiled_expected(pm.coded(H, W), t, p, tap=tap), pm.expected(pm.coded(H, W), tap=tap), (H, W, t, p, tap))


def test_oracle_tile_process_on_a_duplicate_window_plan():
    sd = _tsd(pm.probe_state_dict(1, tap=(0, 2)))
    img = pm.coded(17, 53)                                    # t < H < win: both window rows are the same rectangle
    x = torch.from_numpy(img.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    with torch.no_grad():
        o = ref.tile_process(x, sd, 1, 16, 2)[0].permute(1, 2, 0).numpy()
    _same((o * 255.0).clip(0, 255).astype(np.uint8), pm.expected_u8(img, tap=(0, 2)), "17 x 53")


@pytest.mark.parametrize("scale", [4, 2])
def test_power_of_the_stitch_inputs(scale):
    """On the window-coded tiles of tests/test_gpu_cut_stitch.py a 'first covering window wins' paste and a paste with each crop
    moved by one output pixel both differ from the true paste, on every geometry that test uses."""
    for H, W, t, p in pm.STITCH_GEOS:
        PH, PW = (H + H % 2, W + W % 2) if scale == 2 else (H, W)
        plan = ref.tile_plan(PH, PW, t, p, scale)
        (y1, y2, x1, x2) = plan[0][0]
        tiles = pm.window_tiles(len(plan), scale * (y2 - y1), scale * (x2 - x1))
        true = pm.paste_replay(tiles, plan)
        assert true.shape == (scale * PH, scale * PW, 3)
        assert not np.array_equal(pm.paste_first_wins(tiles, plan), true), (H, W, t, p, "first wins")
        for dy, dx in [(1, 0), (0, 1), (-1, 0), (0, -1)]:
            wrong = pm.paste_crop_moved(tiles, plan, dy, dx)
            assert (wrong != true).mean() > 0.9, (H, W, t, p, dy, dx)


def test_f32_packing_rule_in_the_scale_2_channel_order():
    """fp16(fp32(x * 255)), as tests/test_compact_insitu_cpu.py models it, laid out as the scale-2 packer lays it out: on u8-grid
    input it is x2plus_model.expected_p0 (the integers), and the known tie value lands as 55.75 in its unshuffled channel."""
    import compact_insitu as ci
    x1 = np.array([0.21868873], np.float32)
    assert float(pm.pack_f32_rule(x1)[0]) == 55.75 and float((x1.astype(np.float64) * 255.0).astype(np.float16)[0]) == 55.78125
    rng = np.random.default_rng(3)
    xs = rng.random((2, 3, 6, 8)).astype(np.float32)
    geo1 = {"n": 2, "Hp": [8], "Wp": [10], "mos_kx": 0, "mos_ky": 0}
    _same(pm.expected_p0_f32(xs, geo1, 4)[:, :3], ci.expected_p0({"n": 2, "Hp": 8, "Wp": 10, "mos_kx": 0, "mos_ky": 0}, 2, 6, 8, x=xs), "scale 4")
    assert not pm.expected_p0_f32(xs, geo1, 4)[:, 3:].any()
    for B, th, tw, geo in [(1, 6, 8, {"n": 1, "Hp": [5], "Wp": [6], "mos_kx": 0, "mos_ky": 0}),
                           (5, 6, 8, {"n": 2, "Hp": [9], "Wp": [11], "mos_kx": 2, "mos_ky": 2})]:
        tiles = rng.integers(0, 256, (B, th, tw, 3), dtype=np.uint8)
        x = np.ascontiguousarray((tiles.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))
        _same(pm.expected_p0_f32(x, geo, 2), xm.expected_p0(tiles, geo).astype(np.float32), ("scale 2", B))
    x = np.full((1, 3, 2, 2), 0.5, np.float32)
    x[0, 1, 1, 0] = x1[0]                                     # colour 1, sub-pixel (1, 0): channel 1*4 + 1*2 + 0
    p0 = pm.expected_p0_f32(x, {"n": 1, "Hp": [3], "Wp": [3], "mos_kx": 0, "mos_ky": 0}, 2)
    assert p0[0, 6, 1, 1] == 55.75 and p0[0, 5, 1, 1] == 127.5 and not p0[0, 12:].any()
