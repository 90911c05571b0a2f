"""Probe nets on the device (tests/probe_model.py; pinned to the oracle by tests/test_probe_cpu.py): with weights that make the
net nearest-upsampling of its input shifted by one pixel, every public door must give the expectation BYTE FOR BYTE -- any zero
inside the image (a halo, a mosaic separator or a stale workspace byte read as data), any non-zero at its border (a neighbour
window or stale data read where a zero belongs), a wrong crop offset or a wrong window placement changes bytes.  The coded images
make any two neighbouring pixels differ in every channel, so a value taken from one pixel off is never right by accident.

The f32 doors are held to |f * 255 - 0.5 - expectation| <= 0.13: the one rounding is the fp16 storage of u / 255 (relative
2^-11, at most 0.1245 after the x 255), which is also why the truncating u8 door is exact (it sees u + 0.5 +- 0.125)."""
import math
import time

import numpy as np
import pytest

import gpu_engines
import probe_model as pm
from s2sr import native

pytestmark = pytest.mark.gpu

F16, HP, FP8 = native.PREC_F16, native.PREC_F16_HP, native.PREC_FP8
F32_TOL = 0.13
TOL_F16, TOL_HP = 2.5e-3, 3e-4                     # tests/test_gpu_net.py's constants for the same nets
CHUNKED = [(100, 90, 16, 2), (53, 200, 16, 3), (130, 37, 16, 2)]
# geometries a door refuses: (door, H, W, tile, pad) -> the error text it must raise (none known: every geometry below runs)
REFUSED = {}


def _same(got, want, what):
    d = pm.first_difference(got, want)
    if d:
        print(f"{what}: {d}")
    assert not d, f"{what}: {d}"


def _f32_close(f, want, what):
    """f: HWC float output of a probe net with the 0.5 / 255 bias."""
    d = np.abs(f.astype(np.float64) * 255.0 - 0.5 - want)
    worst = float(d.max())
    if worst > F32_TOL:
        i = np.unravel_index(int(d.argmax()), d.shape)
        print(f"{what}: {int((d > F32_TOL).sum())} beyond {F32_TOL}, worst {worst:.4f} at {list(i)}")
    assert worst <= F32_TOL, (what, worst)


def _run(door, fn, H, W, t, p):
    """The door's output, or None for a geometry listed as refused (which must then raise what the list says)."""
    key = (door, H, W, t, p)
    if key in REFUSED:
        with pytest.raises(native.S2srError, match=REFUSED[key]):
            fn()
        return None
    return fn()


# ---- the geometry sweep ----------------------------------------------------------------------------------------------------------
def sweep_geometries(t, p):
    """The full cross of the plan-changing sizes, plus wide images that take the tiled route with H < win, with duplicate window
    rows and with few rows; visited alternating large and small, so that what the previous shape left in the workspace lies where
    the next one has its halo."""
    e = pm.edge_sizes(t, p)
    geos = {(H, W) for H in e for W in e}
    win = t + 2 * p
    geos |= {(win - 1, 6 * t + 4), (t + 1, 7 * t + 8), (6, 200), (6 * t + 4, win - 1), (200, 6)}
    geos = sorted(geos, key=lambda g: (g[0] * g[1], g))
    order = []
    while geos:
        order.append(geos.pop())
        if geos:
            order.append(geos.pop(0))
    return order


WHOLE_EXTRA = [(1, 1), (3, 5), (64, 64), (1000, 3)]


@pytest.mark.parametrize("tap", [(1, 1), (0, 0), (2, 2)])
@pytest.mark.parametrize("prec", [HP, F16])
def test_u8_door_geometry_sweep(monkeypatch, prec, tap):
    """s2sr_enhance_u8 on every geometry of the sweep, whichever branch the whole / tiled switch takes; where it takes the whole
    image, the window plan is run as well (s2sr_tile_process_f32: 1- to 3-pixel sides, duplicate windows)."""
    e = gpu_engines.fresh(monkeypatch, {}, 1, prec, sd=pm.probe_state_dict(1, tap=tap))
    t0, ran, tiled_n, forced_n = time.perf_counter(), 0, 0, 0
    try:
        for t, p in [(16, 2), (32, 4)]:
            for H, W in sweep_geometries(t, p):
                img = pm.coded(H, W)
                want = pm.expected_u8(img, tap=tap)
                got = _run("enhance_u8", lambda: e.enhance_u8(img, tile=t, pad=p), H, W, t, p)
                if got is not None:
                    _same(got, want, ("enhance_u8", prec, tap, H, W, t, p))
                    ran += 1
                if pm.is_tiled(H, W, t):
                    tiled_n += 1
                else:
                    f = _run("tile_process_f32", lambda: e.tile_process_f32(img, tile=t, pad=p), H, W, t, p)
                    if f is not None:
                        _f32_close(f, want, ("tile_process_f32", prec, tap, H, W, t, p))
                        forced_n += 1
        for H, W in WHOLE_EXTRA:                                                      # the whole-image branch at the default tile
            img = pm.coded(H, W)
            _same(e.enhance_u8(img), pm.expected_u8(img, tap=tap), ("whole", prec, tap, H, W))
            ran += 1
    finally:
        e.close()
    print(f"sweep prec {prec} tap {tap}: {ran} geometries through enhance_u8 ({tiled_n} tiled), {forced_n} more window plans through "
          f"tile_process_f32, {time.perf_counter() - t0:.2f} s")


def test_u8_door_fp8(monkeypatch):
    """The fp8 trunk adds exactly zero (conv_body is zero): the data path around it is the same bytes."""
    e = gpu_engines.fresh(monkeypatch, {}, 1, FP8, sd=pm.probe_state_dict(1, tap=(0, 2)))
    try:
        img = pm.coded(37, 45)
        _same(e.enhance_u8(img, tile=16, pad=2), pm.expected_u8(img, tap=(0, 2)), "fp8 37 x 45 tiled")
        _same(e.enhance_u8(img), pm.expected_u8(img, tap=(0, 2)), "fp8 37 x 45 whole")
    finally:
        e.close()


# ---- halos and separators at the HR levels -------------------------------------------------------------------------------------
def _batch(B, h, w):
    """B distinct coded tiles (crops of one coded image, one pixel apart)."""
    big = pm.coded(h + B, w + B)
    return np.stack([big[i:i + h, i:i + w] for i in range(B)])


HR_BATCHES = [(5, 24, 40), (9, 20, 20), (7, 60, 84), (2, 64, 64), (1, 33, 17)]          # ragged mosaics; plain images
HR_CONFIGS = [("default", {}, 0), ("no mosaic", {"S2SR_MOSAIC": "0"}, 0), ("no graphs", {"S2SR_GRAPH": "0"}, 0), ("group 2", {}, 2)]


@pytest.mark.parametrize("tap_layer", ["conv_up1", "conv_up2", "conv_hr", "conv_last"])
def test_hr_level_halos_and_separators(monkeypatch, tap_layer):
    """The shift tap in each tail conv: its zeros come from the halo ring and the mosaic separators of the 2x / 4x planes.  Every
    configuration is exact on its own; three calls each (first sighting, capture, replay)."""
    for name, env, group in HR_CONFIGS:
        for prec, tap in [(HP, (0, 0)), (HP, (2, 2)), (F16, (0, 2)), (F16, (2, 0))]:
            e = gpu_engines.fresh(monkeypatch, env, 1, prec, group=group, sd=pm.probe_state_dict(1, tap_layer=tap_layer, tap=tap))
            cfg = e.debug_config()
            assert cfg["mosaic_on"] == (0 if name == "no mosaic" else 1) and cfg["graphs_on"] == (0 if name == "no graphs" else 1)
            try:
                for B, h, w in HR_BATCHES:
                    tiles = _batch(B, h, w)
                    want = np.stack([pm.expected_u8(x, tap_layer=tap_layer, tap=tap) for x in tiles])
                    for call in range(3):
                        _same(e.forward_batch_u8(tiles), want, (name, prec, tap_layer, tap, B, h, w, "call", call))
                img = pm.coded(37, 45)
                want = pm.expected_u8(img, tap_layer=tap_layer, tap=tap)
                for call in range(3):
                    _same(e.enhance_u8(img, tile=16, pad=2), want, (name, tap_layer, tap, "tiled 37 x 45", "call", call))
            finally:
                e.close()


@pytest.mark.parametrize("tap_layer", ["conv_first", "conv_last"])
def test_plain_image_then_mosaic_of_the_same_extent(monkeypatch, tap_layer):
    """A plain image whose size is exactly the extent of the next call's window mosaic (k windows of w and their separators:
    k (w + 1) - 1), on one handle: where the plain image left data, the mosaic has its separators, and they must read as zeros.
    Then back, and once more (the second sightings capture)."""
    B, h, w = 9, 20, 20
    kx, ky = native.pick_mosaic(B, h, w)
    assert kx * ky > 1
    PH, PW = ky * (h + 1) - 1, kx * (w + 1) - 1
    for tap in [(0, 0), (2, 2)]:
        e = gpu_engines.fresh(monkeypatch, {}, 1, HP, sd=pm.probe_state_dict(1, tap_layer=tap_layer, tap=tap))
        try:
            plain, tiles = pm.coded(PH, PW)[None], _batch(B, h, w)
            want_plain = pm.expected_u8(plain[0], tap_layer=tap_layer, tap=tap)[None]
            want_tiles = np.stack([pm.expected_u8(x, tap_layer=tap_layer, tap=tap) for x in tiles])
            for call in range(3):
                _same(e.forward_batch_u8(plain), want_plain, ("plain", tap_layer, tap, PH, PW, call))
                _same(e.forward_batch_u8(tiles), want_tiles, ("mosaic behind the plain image", tap_layer, tap, call))
        finally:
            e.close()


# ---- the chunked routes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [HP, F16])
def test_chunked_routes(monkeypatch, prec):
    for tap in [(0, 0), (2, 2)]:
        e = gpu_engines.fresh(monkeypatch, {}, 1, prec, sd=pm.probe_state_dict(1, tap=tap))
        try:
            for H, W, t, p in CHUNKED:
                img = pm.coded(H, W)
                want = pm.expected_u8(img, tap=tap)
                _same(e.enhance_u8(img, tile=t, pad=p), want, ("enhance_u8", prec, tap, H, W))
                _f32_close(e.enhance_f32(img, tile=t, pad=p), want, ("enhance_f32", prec, tap, H, W))
                _f32_close(e.tile_process_f32(img, tile=t, pad=p), want, ("tile_process_f32", prec, tap, H, W))
        finally:
            e.close()


# ---- the job -------------------------------------------------------------------------------------------------------------------
def test_job_swaps_channels_once_on_each_side(monkeypatch):
    """s2sr_enhance_job_u8 without a post-process: RGB in, the net on BGR, RGB out.  The net adds (0, 10, 20) to ITS channels, so
    the caller sees (20, 10, 0): a missing or doubled swap on either side changes bytes."""
    off = (0, 10, 20)
    e = gpu_engines.fresh(monkeypatch, {}, 1, HP, sd=pm.probe_state_dict(1, tap=(2, 0), out_offset=off))
    try:
        for H, W, t, p in [(20, 24, 256, 10), (37, 45, 16, 2)] + CHUNKED[:2]:
            rgb = np.maximum(pm.coded(H, W).astype(np.int64) * 200 // 256, 1).astype(np.uint8)
            want = pm.expected_u8(rgb, tap=(2, 0), out_offset=off[::-1])
            assert want.max() <= 220
            _same(e.enhance_job_u8(rgb, None, tile=t, pad=p), want, ("job", H, W, t, p))
            _same(e.enhance_u8(rgb, tile=t, pad=p), pm.expected_u8(rgb, tap=(2, 0), out_offset=off), ("plain door", H, W, t, p))
    finally:
        e.close()


# ---- the 16-bit door -------------------------------------------------------------------------------------------------------------
def _u16_doors(e, img, batch, lo, hi):
    """[(name, input, output)] of the 16-bit doors: a ragged mosaic batch, a whole image, the banded and the chunked route."""
    out = [("forward_batch_u16", batch, e.forward_batch_u16(batch, lo, hi)),
           ("enhance_u16 whole", img[:28, :36], e.enhance_u16(np.ascontiguousarray(img[:28, :36]), lo, hi))]
    for H, W, t, p in CHUNKED[:2]:
        x = np.ascontiguousarray(img[:H, :W])
        out.append((f"enhance_u16 {H} x {W}", x, e.enhance_u16(x, lo, hi, tile=t, pad=p)))
    return out


@pytest.mark.parametrize("prec", [HP, F16])
def test_u16_door_narrow_ranges_are_exact(monkeypatch, prec):
    """Ranges of 255 levels, bias 0 (this door rounds): the output is lo + clip(v - lo, 0, hi - lo), upsampled and shifted, for
    data that strays below and above the range."""
    tap = (0, 2)
    e = gpu_engines.fresh(monkeypatch, {}, 1, prec, sd=pm.probe_state_dict(1, tap=tap, bias=0.0))
    try:
        for lo, hi in [(0, 255), (1000, 1255)]:
            img = lo + pm.coded(130, 200).astype(np.int64)
            img[5::7, 3::11] = hi + 1                       # strays: just outside and far outside, both sides
            img[2::13, 1::5, 1] = 65535
            if lo:
                img[1::9, 4::7] = lo - 1
                img[6::11, 2::9, 2] = 0
            img = img.astype(np.uint16)
            batch = np.stack([img[i:i + 24, i:i + 40] for i in range(5)])
            for name, x, got in _u16_doors(e, img, batch, lo, hi):
                d = np.clip(x.astype(np.int64), lo, hi) - lo
                want = lo + (np.stack([pm.expected(v, tap=tap) for v in d]) if d.ndim == 4 else pm.expected(d, tap=tap))
                assert got.dtype == np.uint16
                _same(got.astype(np.int64), want, (name, prec, lo, hi))
    finally:
        e.close()


@pytest.mark.parametrize("prec,tol", [(HP, TOL_HP), (F16, TOL_F16)])
def test_u16_door_full_range_places_every_pixel(monkeypatch, prec, tol):
    """Full range on the u16 coded image: values within tests/test_gpu_u16.py's levels(tol, 0, 65535) of the expectation; any neighbour is
    >= 1024 levels away, so WHERE every value came from is still decided exactly."""
    tap = (2, 0)
    bound = math.ceil(tol * 65535) + 1
    assert 2 * bound < 1024
    e = gpu_engines.fresh(monkeypatch, {}, 1, prec, sd=pm.probe_state_dict(1, tap=tap, bias=0.0))
    try:
        img = pm.coded_u16(130, 200)
        batch = np.stack([img[i:i + 24, i:i + 40] for i in range(5)])
        worst = 0
        for name, x, got in _u16_doors(e, img, batch, 0, 65535):
            want = np.stack([pm.expected(v, tap=tap) for v in x]) if x.ndim == 4 else pm.expected(x, tap=tap)
            d = np.abs(got.astype(np.int64) - want)
            print(f"u16 full range prec {prec} {name}: worst {int(d.max())} levels (bound {bound})")
            assert d.max() <= bound, (name, prec, int(d.max()), pm.first_difference(d <= bound, np.ones_like(d, bool)))
            worst = max(worst, int(d.max()))
        print(f"u16 full range prec {prec}: worst level difference {worst}")
    finally:
        e.close()


# ---- x2plus ----------------------------------------------------------------------------------------------------------------------
X2_SIZES = [(39, 57, 256, 10), (2, 3, 256, 10), (45, 38, 16, 2), (277, 514, 128, 10), (40, 58, 256, 10), (38, 45, 16, 2)]


@pytest.mark.parametrize("sub", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_x2plus_every_sub_pixel_channel(monkeypatch, sub):
    """Scale 2: conv_first reads ONE pixel-unshuffle channel per colour, so the output names the sub-pixel the packer (whole image)
    or the window gather (tiled) put there; odd sizes read the reflect row / column.  Centre tap and one shift tap."""
    for tap in [(1, 1), (2 * sub[0], 2 * (1 - sub[1]))]:
        e = gpu_engines.fresh(monkeypatch, {}, 1, HP, scale=2, sd=pm.probe_state_dict(1, scale=2, tap=tap, sub=sub))
        try:
            for H, W, t, p in X2_SIZES:
                img = pm.coded(H, W)
                want = pm.expected_u8(img, scale=2, tap=tap, sub=sub)
                assert pm.is_tiled(H, W, t, 2) == (t < 256)
                _same(e.enhance_u8(img, tile=t, pad=p), want, ("enhance_u8", sub, tap, H, W, t))
                _f32_close(e.enhance_f32(img, tile=t, pad=p), want, ("enhance_f32", sub, tap, H, W, t))
                if H % 2 == 0 and W % 2 == 0:
                    x = np.ascontiguousarray((img.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)[None])
                    _f32_close(e.forward_f32(x)[0].transpose(1, 2, 0), want, ("forward_f32", sub, tap, H, W))
        finally:
            e.close()


# ---- compact ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap", [None, (0, 0), (2, 2), (0, 2)])
def test_compact_probes(monkeypatch, tap):
    """SRVGGNetCompact: the zero net (nearest-x4 through the base add, all 256 values) and the shift probe u + shift(u) on inputs
    <= 127; plain and mosaic batches, a whole and a tiled image."""
    e = gpu_engines.fresh(monkeypatch, {}, 16, HP, arch="compact", sd=pm.compact_probe_state_dict(16, tap))
    try:
        for B, h, w in HR_BATCHES:
            tiles = _batch(B, h, w) >> 1
            want = np.stack([pm.compact_expected(x, tap) for x in tiles])
            assert want.max() <= 255
            for call in range(3):
                _same(e.forward_batch_u8(tiles), want, ("compact batch", tap, B, h, w, call))
        img = pm.coded(37, 45) >> 1
        _same(e.enhance_u8(img, tile=16, pad=2), pm.compact_expected(img, tap), ("compact tiled", tap))
        _same(e.enhance_u8(img), pm.compact_expected(img, tap), ("compact whole", tap))
        if tap is None:
            allv = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
            _same(e.enhance_u8(allv), pm.up(allv, 4), "compact 256 values")
    finally:
        e.close()


# ---- the f32 packers in situ -------------------------------------------------------------------------------------------------------
TIE = np.float32(0.21868873)          # fp32(255 x) lies on an fp16 tie that the exact product does not (55.75 against 55.78125)


@pytest.mark.parametrize("scale", [4, 2])
@pytest.mark.parametrize("B,th,tw", [(1, 24, 34), (5, 40, 44)])
def test_f32_packers_store_the_pinned_rounding(monkeypatch, scale, B, th, tw):
    """pack_f32_nchw_kernel and its unshuffling twin, judged OFF the u8 grid: tap P0 is fp16(fp32(255 x)) bit for bit at the
    positions the packer writes, and zero everywhere else."""
    e = gpu_engines.fresh(monkeypatch, {}, 1, HP, scale=scale, sd=pm.probe_state_dict(1, scale=scale))
    try:
        rng = np.random.default_rng(100 * B + scale)
        x = rng.random((B, 3, th, tw), dtype=np.float32)
        x[:, :, ::5, ::3] = TIE                                   # in every sub-pixel phase and colour
        x[:, :, 1::7, 2::5] = TIE
        geo, taps, _, _ = e.debug_forward_taps(x=x)
        want = pm.expected_p0_f32(x, geo, scale)
        assert (want == np.float32(55.75)).sum() >= 100
        _same(taps["P0"], want, ("P0", scale, B, th, tw))
    finally:
        e.close()
