"""Every door of the library under capped grids: no door's bytes may depend on the number of workgroups.

Every hot kernel is a loop over work items inside a workgroup that stays: the conv kernels walk their patches with the LDS ring and
the counted waits carried across the patch boundary, the integer passes restage LDS on every trip behind a loop-top barrier, the
byte movers are grid-stride loops.  At the sizes a test can afford a 256-CU part gives every workgroup ONE item, so the second trip
-- where a stale LDS stage, a wait that counts the previous epilogue's stores, a missing barrier or a narrow stride would live --
does not run.  The library's grid cap (include/s2sr.h s2sr_debug_grid_cap; csrc/gridcap.hip, capped_grid of csrc/s2sr_internal.h)
limits every such launch to a few workgroups, so the small shapes below make many trips.  No tolerance anywhere in this module:
every comparison is byte for byte, against the same call with the cap off (whose bytes the parity modules judge) or against the
numpy model of the pass.
  (a) the conv kernels alone through debug_conv_trunk / debug_conv, cap 8 (the smallest grid the tile schedulers take);
  (b) every stored layer of a 1-block net (the taps of the in-situ modules) and the output in three sightings, cap 8;
  (c) the door table of tests/doors.py, the raster passes' rows included, on engines made under cap 8, against diag.baseline;
  (d) the tile-loop passes and the byte movers against their models under caps 1 and 3 (a stride that is no power of two, a
      ragged last trip);
  (e) the controls: off means off, a cap above every grid counts nothing, refused values change nothing, launches where a
      workgroup is the work item are not capped.
The precondition of every case is read from the library's counter (native.grid_cap_stats): the launches the cap made smaller and
the largest ceil(work items / workgroups) among them, per launcher family.  A case that relies on the second trip asserts it ran.
The cap is read when a launch is enqueued and a captured graph keeps its grids, so the engines are made, and capture, under the cap.
Nothing here can fault where the library is wrong: a cap changes how many workgroups share the same in-bounds work."""
import functools
import math
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import bands_model as bm
import consistency_model as cm
import diag
import display_model as dm
import doors
import gpu_engines
import nodata_model as nm
from diag import baseline, keep, same, same_values, trips, under
from doors import CONFIGS, DOORS, NET_SHAPES, Inputs
from s2sr import native

pytestmark = pytest.mark.gpu

CAP = 8
K14, K5, K5R, F14, F5, F5R = (native.TRUNK_F16_CONV14, native.TRUNK_F16_CONV5, native.TRUNK_F16_CONV5_RRDB,
                              native.TRUNK_F8_CONV14, native.TRUNK_F8_CONV5, native.TRUNK_F8_CONV5_RRDB)


# operands as tests/test_gpu_trunk.py makes them: representable in the kernel's operand format
def _h(a):
    return a.astype(np.float16).astype(np.float32)


def _rand(rng, N, Cin, Cout, H, W):
    x = _h(rng.standard_normal((N, Cin, H, W)).astype(np.float32))
    w = _h((rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32))
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    return x, w, b


def _e4m3_vals(rng, shape, exp):
    """random values exactly representable as e4m3(v * 2^exp), |v * 2^exp| <= 8"""
    b = rng.integers(0, 256, size=shape, dtype=np.uint8)
    b = np.where((b & 0x7F) == 0x7F, 0, b).astype(np.uint8)                 # no NaN codes
    v = torch.from_numpy(b).view(torch.float8_e4m3fn).float().numpy()
    return (np.clip(v, -8.0, 8.0) * 2.0 ** -exp).astype(np.float32)


def same_bytes(got, want, what):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: output {k} is {g.dtype} {g.shape}, uncapped {w.dtype} {w.shape}"
        differ = int((g.view(np.uint8) != w.view(np.uint8)).sum())
        assert differ == 0, f"{what}: {differ} of {g.nbytes} bytes of output {k} differ from the uncapped call"


@pytest.fixture(scope="module")
def capped():
    """name -> the engine of doors.CONFIGS[name] made, and its weights loaded, under cap 8; closed at the end, the cap put back"""
    with diag.engines_under(native.grid_cap_workgroups, native.grid_cap, CAP) as get:
        yield get


@pytest.fixture(scope="module")
def bare():
    """engines without weights for the hooks and passes that need none, made under cap 8: (fp16, fp8)"""
    before = native.grid_cap_workgroups()
    native.grid_cap(CAP)
    e, e8 = native.Engine(num_block=1, precision=native.PREC_F16_HP), native.Engine(num_block=1, precision=native.PREC_FP8)
    native.grid_cap(before)
    yield e, e8
    e.close(), e8.close()


@pytest.fixture(autouse=True)
def _cap_back_between_tests():
    before = native.grid_cap_workgroups()
    yield
    native.grid_cap(before)


def both(call, cap, what, family, least=3):
    """call() under the cap and with the cap off: the same bytes, and the family's busiest workgroup made at least `least` trips"""
    with under(cap):
        got = keep(call())
        n, st = trips(family)
    with under(0):
        want = keep(call())
        assert trips()[0] == 0, "the cap is off and a launch was counted"
    print(f"{what}: cap {cap}, {family} {st[family]}")
    assert n >= least, f"{what}: the busiest {family} workgroup made {n} trips under cap {cap}: {st}"
    same_bytes(got, want, what)
    return got


# ---- (a) the conv kernels alone, cap 8 ---------------------------------------------------------------------------------------------
# N = 3, 72 x 100: ragged in both directions, so an edge patch is first, middle and last somewhere; 36 patches of 32x32, 60 of
# 16x32, 108 of 8x32 on 8 workgroups: 5, 8 and 14 trips.
A_SHAPE = (3, 72, 100)
A_FULL = (3, 96, 128)            # the whole-patch forms refuse ragged shapes: 36 / 72 / 144 patches


@pytest.mark.parametrize("form", [1, 2, 5, 10])
def test_f16_conv14_forms_under_the_cap(bare, form):
    e, _ = bare
    N, H, W = A_SHAPE
    x, w, b = _rand(np.random.default_rng(1000 + form), N, 160, 32, H, W)
    both(lambda: e.debug_conv_trunk(K14, x, w, b, form=form), CAP, f"conv1-4 form {form}", "trunk_f16")


@pytest.mark.parametrize("form", [6, 7, 8])
def test_f16_conv14_whole_patch_forms_under_the_cap(bare, form):
    e, _ = bare
    N, H, W = A_FULL
    x, w, b = _rand(np.random.default_rng(1100 + form), N, 160, 32, H, W)
    both(lambda: e.debug_conv_trunk(K14, x, w, b, form=form), CAP, f"conv1-4 whole-patch form {form}", "trunk_f16")


@pytest.mark.parametrize("form", [1, 5, 10])
def test_f16_conv5_forms_under_the_cap(bare, form):
    e, _ = bare
    N, H, W = A_SHAPE
    rng = np.random.default_rng(1200 + form)
    x, w, b = _rand(rng, N, 192, 64, H, W)
    le = e.debug_config()["lo_exp"]
    lo = (rng.integers(-7, 8, size=(N, 64, H, W)) * 2.0 ** (-4 - le)).astype(np.float32)
    skip = _h(rng.standard_normal((N, 64, H, W)).astype(np.float32))
    both(lambda: e.debug_conv_trunk(K5, x, w, b, lo=lo, form=form), CAP, f"conv5 form {form}", "trunk_f16")
    both(lambda: e.debug_conv_trunk(K5R, x, w, b, lo=lo, skip=skip, form=form), CAP, f"conv5 of rdb3 form {form}", "trunk_f16")


def test_f8_trunk_hooks_under_the_cap(bare):
    """operands as tests/test_gpu_trunk.py makes them: e4m3 values at the handle's scales"""
    _, e8 = bare
    N, H, W = A_SHAPE
    cfg = e8.debug_config()
    xe, ge = cfg["fp8_x_exp"], cfg["fp8_g_exp"]
    rng = np.random.default_rng(1300)
    for Cin in (64, 160):                                    # conv1 (resident weights) and conv4
        x = np.concatenate([_e4m3_vals(rng, (N, 64, H, W), xe)] + ([_e4m3_vals(rng, (N, Cin - 64, H, W), ge)] if Cin > 64 else []), axis=1)
        w = (rng.standard_normal((32, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
        b = (rng.standard_normal(32) * 0.1).astype(np.float32)
        both(lambda: e8.debug_conv_trunk(F14, x, w, b), CAP, f"fp8 conv1-4, {Cin} channels in", "trunk_f8")
    x = np.concatenate([_e4m3_vals(rng, (N, 64, H, W), xe), _e4m3_vals(rng, (N, 128, H, W), ge)], axis=1)
    w = (rng.standard_normal((64, 192, 3, 3)) / np.sqrt(9 * 192)).astype(np.float32)
    b = (rng.standard_normal(64) * 0.1).astype(np.float32)
    skip = _h(rng.standard_normal((N, 64, H, W)).astype(np.float32))
    both(lambda: e8.debug_conv_trunk(F5, x, w, b), CAP, "fp8 conv5", "trunk_f8")
    both(lambda: e8.debug_conv_trunk(F5R, x, w, b, skip=skip), CAP, "fp8 conv5 of rdb3", "trunk_f8")


@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("up", [False, True])
def test_debug_conv_under_the_cap(bare, up, cout):
    e, _ = bare
    N, H, W = A_SHAPE
    rng = np.random.default_rng(1400 + cout + up)
    x = _h(rng.standard_normal((N, 64, H, W)).astype(np.float32))
    w = _h((rng.standard_normal((cout, 64, 3, 3)) / np.sqrt(9 * 64)).astype(np.float32))
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    both(lambda: e.debug_conv(x, w, b, upsample=up, act=True), CAP, f"debug_conv cout {cout} upsample {up}", "conv")


# ---- (b) every stored layer, cap 8 -------------------------------------------------------------------------------------------------
LAYER_SHAPES = ["ragged_2x37x53", "mosaic_9x20x20"]          # tests/test_gpu_tail.py SHAPES
# the launch image of each shape on the trunk grid: a 1 x 2 mosaic of 37 x 53 windows, a 3 x 3 mosaic of 20 x 20 windows (one
# separator row / column between neighbours)
LAUNCH_IMAGE = {"ragged_2x37x53": (37, 107), "mosaic_9x20x20": (62, 62), "mosaic_16x24x40": (49, 327)}
# The compact net has no HR tail: all its convs run on the LR grid, where the two shapes above leave it 2 trips and none.  So it also
# takes the 2 x 8 mosaic of tests/compact_insitu.py's SHAPES (period 25 x 41: 49 x 327 pixels, 44 patches of 16x32, 6 trips), and
# the PReLU and pixel-shuffle forms make their third trip.
LAYER_CASES = [(n, sh) for n in CONFIGS for sh in LAYER_SHAPES] + [("compact", "mosaic_16x24x40")]
SHAPE_OF = {**NET_SHAPES, "mosaic_16x24x40": (16, 24, 40, 0)}


def _least(name, shape):
    """What the busiest workgroup must have done at the least, by arithmetic: {family: trips}.  The trunk kernels take 8x32
    patches at these sizes (fp8: 16x32), the convs of conv3x3.hip 16x32; the RRDB nets' HR tail runs at 4x (x2plus: 2x) the
    trunk grid, the compact net has no tail.  On 8 workgroups: 20 trunk patches of ragged_2x37x53 are 3 trips (fp8: 12, 2 trips),
    its HR tail of 148 x 428 has 140 patches; the mosaic's 16 trunk patches are 2 trips (fp8: 8 patches on 8 workgroups, nothing
    to cap).  A family that the arithmetic leaves at one trip is not asserted."""
    H, W = LAUNCH_IMAGE[shape]
    nb, prec, S, arch = CONFIGS[name]
    per = lambda h, w, rows: math.ceil(math.ceil(h / rows) * math.ceil(w / 32) / CAP)
    if arch == "compact":
        out = {"conv": per(H, W, 16)}
    else:
        out = {"conv": per(S * H, S * W, 16), "trunk": per(H, W, 16 if prec == native.PREC_FP8 else 8)}
    # the tail's own patch forms (sub-pixel up-convs, whole patches) deal out a few patches less than this count: what is asked of a
    # family is the 3 trips this module asks everywhere, or the 2 that the arithmetic leaves it
    return {f: min(n, 3) for f, n in out.items() if n >= 2}


def _taps(e, name, tiles):
    """every tapped field of one batch through the production forward, and both outputs: a flat {name: array}"""
    out = {}
    if CONFIGS[name][3] == "compact":
        nc = CONFIGS[name][0]
        for a in range(0, nc + 1, native.COMPACT_TAPS_MAX):
            layers = list(range(a, min(a + native.COMPACT_TAPS_MAX, nc + 1)))
            _, acts, p0, of32, ou8 = e.debug_compact_taps(layers, tiles=tiles)
            out.update({f"act{k}": v for k, v in acts.items()})
            out.update(p0=p0, out_f32=of32, out_u8=ou8)
        return out
    _, taps, of32, ou8 = e.debug_forward_taps(tiles=tiles)
    out.update(taps)
    out.update(out_f32=of32, out_u8=ou8)
    if CONFIGS[name][2] == 4:                                 # the trunk hook is the scale-4 nets'
        _, fields, _, tf32, tu8 = e.debug_trunk_taps(0, 3 * CONFIGS[name][0], tiles=tiles)
        out.update({f"trunk_{k}": v for k, v in fields.items()})
        out.update(trunk_out_f32=tf32, trunk_out_u8=tu8)
    return out


@pytest.mark.parametrize("name,shape", LAYER_CASES)
def test_every_stored_layer_under_the_cap(capped, name, shape):
    B, th, tw, _ = SHAPE_OF[shape]
    S = CONFIGS[name][2]
    if S == 2:
        th, tw = 2 * th, 2 * tw                              # x2plus: the listed shape is the trunk grid
    tiles = Inputs().u8((B, th, tw, 3), B * 10000 + th * 100 + tw)
    e = capped(name)
    with diag.modes_off():
        ref = gpu_engines.default(*CONFIGS[name])
        want = _taps(ref, name, tiles)
        want_out = keep(ref.forward_batch_u8(tiles))
    with under(CAP):
        got = _taps(e, name, tiles)
        st = native.grid_cap_stats()
        sight = [keep(e.forward_batch_u8(tiles)) for _ in range(3)]          # direct launches, the capture, a replay
    seen = {"conv": st["conv"][1], "trunk": max(st["trunk_f16"][1], st["trunk_f8"][1])}
    print(f"{name} {shape}: {len(got)} fields, trips {seen}, {st}")
    for fam, least in _least(name, shape).items():
        assert seen[fam] >= least, f"{name} {shape}: the busiest {fam} workgroup made {seen[fam]} trips: {st}"
    assert set(got) == set(want)
    for k in sorted(got):
        same_bytes(got[k], want[k], f"{name} {shape}, field {k}")
    same_bytes(got["out_u8"], want_out, f"{name} {shape}: the hook's output against forward_batch_u8")
    for k, y in enumerate(sight):
        same_bytes(y, want_out, f"{name} {shape}, forward_batch_u8 sighting {k + 1}")


# ---- (c) the door table on engines made under cap 8 --------------------------------------------------------------------------------
@pytest.mark.parametrize("ident", list(DOORS))
def test_door_under_the_cap(capped, ident):
    name, fn = DOORS[ident]
    e = capped(name)
    want = baseline(ident)
    sightings = 3 if "-forward_" in ident else 1                # net doors: direct launches, the capture, a replay
    with under(CAP):
        for k in range(sightings):
            same(keep(fn(e, Inputs())), want, f"{ident}, cap {CAP}, sighting {k + 1}")


def test_the_door_table_ran_capped(capped):
    """The precondition of (c): on an engine made under the cap, one door of each kind counts capped launches in its families.
    Of the raster passes: the carried band whole (9 tiles in one launch; in bands of 2 S + 1 guide rows no launch has more than 6,
    which a cap of 8 leaves alone), the index pass's rendering, the zones and the fields pass at 255 x 257 and 130 x 197 (32 blocks,
    20 and 12 tiles; index_nd_u16 itself takes 1024 lanes of 8 pixels a workgroup, so its 65535 pixels are 8 workgroups' worth and
    cap 8 changes nothing there: caps 1 and 3 judge it in tests/test_gpu_index.py), management zones and the split at 130 x 197
    (20 tiles of 64 x 32 whole -- in bands of 7 rows no launch has more than 4 --, and 12 growth tiles and 101 per-pixel blocks),
    and the masked warp."""
    for ident, fams in (("x4_hp-ragged_2x37x53-forward_batch_u8", ("conv", "trunk_f16", "pack")), ("x4_fp8-ragged_2x37x53-forward_batch_u8", ("trunk_f8",)),
                        ("x4_hp-banded-consistent_u8-smooth", ("consistency",)), ("x4_hp-banded-masked_u8", ("nodata",)),
                        ("postprocess_batch_u8_dev-67x101-wow", ("postprocess",)), ("display_apply_u16-255x257-bands0", ("display",)),
                        ("tiles_base_u8", ("tiles",)), ("tiles_resample_u8-lanczos", ("resample",)), ("carry_band_u16-x4-whole", ("bands",)),
                        ("index_render_i16-255x257", ("display",)), ("zones_rasterize_u16-scene-255x257", ("display",)),
                        ("fields_segment_i16-130x197-spiral", ("display",)), ("zones_kmeans_i16-130x197-planted_nodata-one-k8", ("display",)),
                        ("fields_split_i16-130x197-blobs-edge", ("display",)), ("warp_bilinear_masked_u8", ("tiles",))):
        name, fn = DOORS[ident]
        e = diag.new_engine(name)                               # a fresh engine: no graph from an earlier test stands in for the launches
        try:
            with under(CAP):
                same(keep(fn(e, Inputs())), baseline(ident), ident)
                st = native.grid_cap_stats()
        finally:
            e.close()
        for f in fams:
            assert st[f][0] > 0 and st[f][1] >= 2, f"{ident}: no capped launch of {f} made a second trip: {st}"


# ---- (d) the tile-loop passes against their models, caps 1 and 3 -------------------------------------------------------------------
CAPS = [1, 3]


def _expect(family, cap, items):
    """the counter holds exactly what the arithmetic says: ceil(items / cap) trips"""
    n, st = trips(family)
    assert n == math.ceil(items / cap), f"{family}: {n} trips counted, {items} items on {cap} workgroups: {st}"
    return n


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("H,W", [(37, 45), (33, 17)])
def test_carry_band_under_the_cap(bare, H, W, S, cap):
    """tests/test_gpu_bands.py's cases: 9 tiles of 16 x 16 input pixels (3 x 3) and 6 (3 x 2).  Under cap 1 both make at least 3
    trips; under cap 3 the 6 tiles of 33 x 17 make 2, which is what is asserted there."""
    e, _ = bare
    q = bm.scene(H, W, S, seed=5)
    b, v = bm.stray_band(q, S, seed=6), bm.holes(H, W, seed=7)
    tiles = math.ceil(H / 16) * math.ceil(W / 16)
    for masked in (False, True):
        want, bad = bm.carry(q, b, S, 1000, 11000, r=2, eps=bm.default_eps(1000, 11000), valid=v if masked else None, fill=77)
        with under(cap):
            got, n = e.carry_band_u16(b, S, sr=q, lo=1000, hi=11000, r=2, eps=bm.default_eps(1000, 11000), valid=v if masked else None, fill=77)
            made = _expect("bands", cap, tiles)
        assert made >= (3 if tiles >= 3 * cap else 2)
        same_values(got, want, f"{H} x {W} x{S} masked {masked}, cap {cap}")
        assert n == bad


def _board(h, w, S, flip):
    """tests/test_carry_bands_cpu.py test_the_extremes_stay_inside_int64: the 0 / 65535 checkerboards"""
    yy, xx = np.mgrid[0:h, 0:w]
    board = ((yy + xx) % 2) * 65535
    board[:, 4:] = np.where(xx[:, 4:] % 2 == 0, 65535, 0)
    q = np.repeat(cm._up(board, S)[..., None], 3, axis=2).astype(np.uint16)
    return q, (65535 - board if flip else board).astype(np.uint16)


@pytest.mark.parametrize("cap", [0] + CAPS)
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("S", [2, 4])
def test_carry_band_on_the_extremes(bare, S, flip, cap):
    """The width paragraph of bands.hip on the device: the checkerboards whose covariances need up to 60 bits, at the CPU test's
    11 x 13 (one tile: the cap changes nothing there, asserted) and, built the same way, at 37 x 45 (9 tiles, several trips)."""
    e, _ = bare
    for h, w in ((11, 13), (37, 45)):
        q, b = _board(h, w, S, flip)
        want, bad = bm.carry(q, b, S, 0, 65535, r=4, eps=1)
        with under(cap):
            got, n = e.carry_band_u16(b, S, sr=q, lo=0, hi=65535, r=4, eps=1)
            tiles = math.ceil(h / 16) * math.ceil(w / 16)
            if cap and tiles > cap:
                assert _expect("bands", cap, tiles) >= 3
            else:
                assert trips("bands")[0] == 0
        same_values(got, want, f"{h} x {w} x{S} flip {flip}, cap {cap}")
        assert n == bad


@functools.lru_cache(maxsize=None)
def _consistency_case(H, W, S, dtype, lo, hi, mode):
    """consistency_model's saturating input and the model's answer: once for both caps"""
    sr, img = cm.saturating_input(H, W, S, dtype=dtype, lo=lo, hi=hi)
    want, bad = cm.consistency(sr, img, S, mode, lo, hi)
    return sr, img, want, bad


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("dtype,lo,hi", [("uint8", 0, 255), ("uint16", 100, 4000)])
@pytest.mark.parametrize("mode", [cm.EXACT, cm.SMOOTH])
@pytest.mark.parametrize("H,W,S", [(37, 45, 4), (70, 75, 2)])
def test_consistency_pass_under_the_cap(bare, H, W, S, mode, dtype, lo, hi, cap):
    """9 tiles of 64 x 64 output pixels at either shape, on the saturating input"""
    e, _ = bare
    sr, img, want, bad = _consistency_case(H, W, S, dtype, lo, hi, mode)
    with under(cap):
        got, n = e.consistency(sr, img, mode, lo, hi)
        assert _expect("consistency", cap, 9) >= 3
    same_values(got, want, f"{dtype} {H} x {W} x{S} mode {mode}, cap {cap}")
    assert n.tolist() == bad.tolist()


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("kind", ["holes", "island"])
@pytest.mark.parametrize("R", [5, 64])
def test_fill_nodata_under_the_cap(bare, R, kind, cap):
    """70 x 300: 10 tiles of 16 rows x 256 columns"""
    e, _ = bare
    H, W = 70, 300
    valid = nm.make_mask(kind, H, W)
    src = nm.sources_separable(valid, R)
    for dtype in ("uint8", "uint16"):
        img = np.random.default_rng(11 + 1000 * H + W).integers(1, 256 if dtype == "uint8" else 13000, size=(H, W, 3)).astype(dtype)
        img[valid == 0] = 0                                  # the raster as a file would hold it
        with under(cap):
            got = e.fill_nodata(img, valid, R)
            assert _expect("nodata", cap, 10) >= 3
        same_values(got, np.ascontiguousarray(img[src[..., 0], src[..., 1]]), f"{dtype} R {R} {kind}, cap {cap}")


@pytest.mark.parametrize("cap", CAPS)
def test_display_under_the_cap(bare, cap):
    """255 x 257: 8192 groups of 24 samples -- 8 chunks of the histogram kernel (its grid stays a multiple of its 8 ranges: one
    workgroup per range walks all 8 chunks under either cap), 32 blocks of the apply kernel"""
    e, _ = bare
    H, W = 255, 257
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 65536, size=(H, W, 3)).astype(np.uint16)
    lut = rng.integers(0, 256, size=(3, 65536), dtype=np.uint8)
    with under(cap):
        got_h = e.display_hist_u16(img, nodata=int(img[0, 0, 0]))
        n_h, st_h = trips("display")
        native.grid_cap_stats(reset=True)
        got_a = e.display_apply_u16(img, lut)
        n_a, st_a = trips("display")
    print(f"cap {cap}: hist {st_h['display']}, apply {st_a['display']}")
    assert n_h >= 3 and n_a >= 3, (st_h, st_a)
    assert np.array_equal(got_h, dm.hist(img, int(img[0, 0, 0])))
    assert np.array_equal(got_a, dm.apply(img, lut))


PYRAMID = ["warp_bilinear_u8", "tiles_base_u8", "tiles_overview_u8-host_child", "tiles_overview_u8-device_child", "tiles_overview_u8-two_levels"] + [
    i for i in DOORS if i.startswith("tiles_resample_u8-")]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("ident", PYRAMID)
def test_pyramid_under_the_cap(capped, ident, cap):
    """the shapes of tests/doors.py, whose baselines the pyramid modules hold to their models"""
    name, fn = DOORS[ident]
    e = capped(name)
    want = baseline(ident)
    with under(cap):
        got = keep(fn(e, Inputs()))
        n, st = trips("resample" if "resample" in ident else "tiles")
    assert n >= 3, f"{ident}: {st}"
    same(got, want, f"{ident}, cap {cap}")


# ---- (e) the controls --------------------------------------------------------------------------------------------------------------
def test_off_means_off_and_a_cap_above_every_grid_counts_nothing(bare):
    e, _ = bare
    x, w, b = _rand(np.random.default_rng(3), 1, 64, 32, 40, 70)
    for cap in (0, native.GRID_CAP_MAX):
        with under(cap):
            assert native.grid_cap_workgroups() == cap
            y = e.debug_conv_trunk(K14, x, w, b, form=5)
            e.fill_nodata(Inputs().u8((37, 53, 3), 1), nm.make_mask("holes", 37, 53), 5)
            st = native.grid_cap_stats()
        assert all(v == (0, 0) for v in st.values()), (cap, st)
    with under(CAP):
        same_bytes(e.debug_conv_trunk(K14, x, w, b, form=5), y, "cap 8")
        assert native.grid_cap_stats()["trunk_f16"] == (1, 2)            # 15 patches of 8x32: the grid of 16 became 8


def test_refused_values_leave_the_cap_where_it_was():
    with under(3):
        for bad in (-1, -8, native.GRID_CAP_MAX + 1, 2 ** 31 - 1):
            with pytest.raises(native.S2srError):
                native.grid_cap(bad)
            assert native.grid_cap_workgroups() == 3
    assert tuple(native.grid_cap_stats()) == native.grid_cap_families() and len(native.grid_cap_families()) == native.GRID_CAP_FAMILIES


def test_launches_whose_workgroup_is_the_work_item_are_not_capped(capped):
    """The PNG kernels take one workgroup per tile, the CLAHE histogram and LUT kernels one per grid tile, the blur one per pixel
    tile: a cap would drop work, so these launches never see it.  Asserted from the counter, not from the bytes: under cap 1 the
    PNG writer counts nothing, and a post-process counts its one grid-stride launch (the CLAHE apply) and nothing else."""
    e = capped("x4_hp")
    rgba = doors.png_level(Inputs())
    iy, ix = np.arange(512, dtype=np.int32), np.arange(512, dtype=np.int32)
    with under(0):
        e.tiles_base_u8(rgba, ix, ix, iy, iy, fetch=False)             # the level, left on the device
    with under(1), tempfile.TemporaryDirectory() as d:
        paths = [Path(d) / f"{j}_{i}.png" for j in range(2) for i in range(2)]
        wrote = e.tiles_write_png(2, 2, paths, row_threads=True).copy()
        files = [np.frombuffer(q.read_bytes(), np.uint8) if q.exists() else np.zeros(0, np.uint8) for q in paths]
        st = native.grid_cap_stats()
    assert all(v == (0, 0) for v in st.values()), f"the PNG writer under cap 1: {st}"
    same((wrote, *files), baseline("tiles_write_png-row_threads"), "the PNG writer under cap 1")
    ident = "postprocess_u8-70x101-grid16_wide"
    with under(1):
        got = keep(DOORS[ident][1](e, Inputs()))
        st = native.grid_cap_stats()
    assert st.pop("postprocess") == (1, math.ceil(math.ceil(70 * 101 / 4) / 256)), st
    assert all(v == (0, 0) for v in st.values()), f"{ident} under cap 1: {st}"
    same(got, baseline(ident), f"{ident}, cap 1")
