"""Every door of the library under red zones: no store may land outside the buffer it belongs to.

The parity tests read what a kernel was meant to write.  A stray vector store at a ragged edge, or a batch's last image running
one padded row long, lands in allocator slack or in the neighbouring workspace plane and changes no byte any of them reads.  Here
the library's red-zone mode (include/s2sr.h s2sr_debug_redzone; csrc/redzone.h) puts Z = 65536 patterned bytes in front of and
behind every device allocation and behind every workspace plane -- a whole padded row of these shapes is about 2 KB, so a
row-long overrun stays inside a zone -- and each case asserts
  (a) the bytes returned equal those of the same call on an engine without zones (the cached engines of gpu_engines.py, every
      allocation of theirs made with the mode off), and
  (b) redzone_check() finds no damaged zone anywhere in the process, and counts a plausible number of zoned allocations.
The controls poke one wrong byte into a zone and must be caught, with side and offset.  The `_dev` doors write into the caller's
memory, which the library cannot zone: torch buffers with guard bytes around the output, two fills, no byte outside may change
and every byte inside must be written.

x2plus refuses odd tile sizes (pixel_unshuffle by 2), so its net-door cases run the listed shapes as the trunk grid: tiles of
2 th x 2 tw.  The 16-bit doors exist on the x4 RRDB nets only; x2plus and the compact net must refuse them and stay clean."""
import numpy as np
import pytest
import torch

import gpu_engines
import resample_model as rm
from s2sr import geo, native, tiles

pytestmark = pytest.mark.gpu

Z = 65536
HP, F16, FP8 = native.PREC_F16_HP, native.PREC_F16, native.PREC_FP8
# name -> gpu_engines.default's arguments: num_block, precision, scale, arch
CONFIGS = {"x4_hp": (1, HP, 4, "rrdb"), "x4_f16": (1, F16, 4, "rrdb"), "x4_fp8": (1, FP8, 4, "rrdb"), "x2plus": (1, HP, 2, "rrdb"),
           "compact": (16, HP, 4, "compact")}
# tests/test_gpu_tail.py SHAPES (B, th, tw, job_windows) and the degenerate ones
NET_SHAPES = {"full_1x16x32": (1, 16, 32, 0), "ragged_2x37x53": (2, 37, 53, 0), "short_3x7x45": (3, 7, 45, 0),
              "mosaic_9x20x20": (9, 20, 20, 0), "dead_7of9x20x20": (7, 20, 20, 9), "one_1x1x1": (1, 1, 1, 0), "row_1x1x9": (1, 1, 9, 0),
              "col_1x7x1": (1, 7, 1, 0)}
BANDED, CHUNKED = (100, 90, 16, 2), (53, 200, 16, 3)          # tests/test_gpu_u16.py, tests/test_gpu_blend.py
IMAGES = {"banded": BANDED, "chunked": CHUNKED, "short_ramps": (39, 39, 16, 3), "untiled": (28, 36, 256, 10), "one_pixel": (1, 1, 256, 10)}
FULL, SUB = (0, 65535), (1000, 11000)


def _new_engine(name):
    nb, prec, scale, arch = CONFIGS[name]
    e = native.Engine(num_block=nb, precision=prec, scale=scale, arch=arch)
    e.load_state_dict(gpu_engines.state_dict(nb, scale, arch))
    return e


@pytest.fixture(scope="module")
def zoned():
    """name -> a fresh engine created (and so allocated) with Z = 65536; all closed at the end, and the zone size put back to what
    the module found (0, or what S2SR_REDZONE set for the whole run)."""
    before = native.redzone_bytes()
    native.redzone(Z)
    made = {}

    def get(name):
        if name not in made:
            made[name] = _new_engine(name)
        return made[name]
    yield get
    for e in made.values():
        e.close()
    native.redzone(before)


def baseline(name, fn):
    """fn(the cached engine without zones), run with the mode off: whatever it allocates or regrows on the way has no zones."""
    native.redzone(0)
    try:
        return fn(gpu_engines.default(*CONFIGS[name]))
    finally:
        native.redzone(Z)


def clean(e):
    n, bad, msg = e.redzone_check()
    assert bad == 0, msg
    # its own: the trash page, the bias pool, at least two head / tail weight buffers ... up to some dozens with workspace planes
    assert 4 <= n <= 400, n
    return n


def keep(r):
    """results may live in the pinned pool, which the next call reuses"""
    return tuple(np.array(a) for a in r) if isinstance(r, tuple) else np.array(r)


def same(got, want, what):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{what}: {int((g != w).sum())} of {g.size} elements differ with red zones"


def both(zoned, name, fn, what):
    """(a) and (b) for one call"""
    e = zoned(name)
    got = keep(fn(e))
    same(got, baseline(name, lambda b: keep(fn(b))), f"{name} {what}")
    clean(e)
    return got


def _dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- net doors -----------------------------------------------------------------------------------------------------------------------
def _part(e, tiles_u8, job, scale):
    B, th, tw, _ = tiles_u8.shape
    x = _dev_u8(tiles_u8)
    y = torch.zeros((B, scale * th, scale * tw, 3), dtype=torch.uint8, device="cuda")
    e.forward_part_u8_dev(x.data_ptr(), B, th, tw, job, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("shape", list(NET_SHAPES))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_net_doors(zoned, name, shape):
    B, th, tw, job = NET_SHAPES[shape]
    scale = CONFIGS[name][2]
    if scale == 2:
        th, tw = 2 * th, 2 * tw                      # the listed shape is the trunk grid
    rng = np.random.default_rng(B * 10000 + th * 100 + tw)
    t8 = rng.integers(0, 256, (B, th, tw, 3), dtype=np.uint8)
    if job:
        both(zoned, name, lambda e: _part(e, t8, job, scale), f"{shape} forward_part_u8_dev")
        return
    both(zoned, name, lambda e: e.forward_batch_u8(t8), f"{shape} forward_batch_u8")
    x = np.ascontiguousarray(t8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))
    both(zoned, name, lambda e: e.forward_f32(x), f"{shape} forward_f32")
    t16 = rng.integers(0, 65536, (B, th, tw, 3)).astype(np.uint16)
    if name.startswith("x4"):
        for lo, hi in (FULL, SUB):
            both(zoned, name, lambda e: e.forward_batch_u16(t16, lo, hi, want_f32=True), f"{shape} forward_batch_u16 + f32 {lo, hi}")
            both(zoned, name, lambda e: e.forward_batch_u16(t16, lo, hi), f"{shape} forward_batch_u16 {lo, hi}")
    else:
        with pytest.raises(native.S2srError, match="16-bit input is not available"):
            zoned(name).forward_batch_u16(t16)
        clean(zoned(name))


def test_x2plus_refuses_odd_tiles_and_stays_clean(zoned):
    """why the x2plus cases above run doubled"""
    with pytest.raises(native.S2srError, match="even tile sizes"):
        zoned("x2plus").forward_batch_u8(np.zeros((1, 7, 45, 3), np.uint8))
    clean(zoned("x2plus"))


# ---- image doors ---------------------------------------------------------------------------------------------------------------------
def _image(H, W, seed):
    return np.random.default_rng(seed + 1000 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _image_doors_u8(zoned, name, img, tile, pad, what):
    both(zoned, name, lambda e: e.enhance_u8(img, tile=tile, pad=pad), f"{what} enhance_u8")
    both(zoned, name, lambda e: e.enhance_f32(img, tile=tile, pad=pad), f"{what} enhance_f32")
    both(zoned, name, lambda e: e.enhance_blend_u8(img, tile=tile, pad=pad), f"{what} enhance_blend_u8")
    both(zoned, name, lambda e: e.enhance_blend_u8(img, tile=tile, pad=pad, want_f32=True), f"{what} enhance_blend_u8 + f32")
    both(zoned, name, lambda e: e.enhance_job_u8(img, native.pp_wow(), tile=tile, pad=pad), f"{what} enhance_job_u8 wow")


@pytest.mark.parametrize("case", list(IMAGES))
def test_image_doors_x4(zoned, case):
    H, W, tile, pad = IMAGES[case]
    img = _image(H, W, 7)
    _image_doors_u8(zoned, "x4_hp", img, tile, pad, case)
    img16 = np.random.default_rng(H).integers(0, 65536, (H, W, 3)).astype(np.uint16)
    for lo, hi in (FULL, SUB):
        both(zoned, "x4_hp", lambda e: e.enhance_u16(img16, lo, hi, tile=tile, pad=pad), f"{case} enhance_u16 {lo, hi}")
        both(zoned, "x4_hp", lambda e: e.enhance_blend_u16(img16, lo, hi, tile=tile, pad=pad), f"{case} enhance_blend_u16 {lo, hi}")
    both(zoned, "x4_hp", lambda e: e.enhance_u16(img16, tile=tile, pad=pad, want_f32=True), f"{case} enhance_u16 + f32")
    both(zoned, "x4_hp", lambda e: e.enhance_blend_u16(img16, tile=tile, pad=pad, want_f32=True), f"{case} enhance_blend_u16 + f32")


@pytest.mark.parametrize("name", ["x4_f16", "x4_fp8", "compact"])
def test_image_doors_other_nets(zoned, name):
    H, W, tile, pad = CHUNKED
    _image_doors_u8(zoned, name, _image(H, W, 8), tile, pad, "chunked")
    _image_doors_u8(zoned, name, _image(39, 39, 8), 16, 3, "short_ramps")


def test_image_doors_x2plus_odd_image(zoned):
    """39 x 39 at scale 2: the reflect-padded 40 x 40 image, tiled and untiled, output cropped by the stitch maps"""
    img = _image(39, 39, 9)
    _image_doors_u8(zoned, "x2plus", img, 16, 3, "x2plus 39x39 tiled")
    _image_doors_u8(zoned, "x2plus", img, 256, 10, "x2plus 39x39 untiled")
    _image_doors_u8(zoned, "x2plus", _image(3, 3, 9), 256, 10, "x2plus 3x3")       # the smallest odd image: 2 x 2 is the entry's minimum


# ---- post-process --------------------------------------------------------------------------------------------------------------------
def _pp(grid, sigma=1.2):
    return native.PPParams(2.5, grid, sigma, 1.4, -0.4, 35, 85, 1.2, 7)


@pytest.mark.parametrize("grid", [8, 16])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 300), (70, 101)])
def test_postprocess(zoned, H, W, grid):
    img = _image(H, W, 10)
    img[..., 1] = np.maximum(img[..., 1], 90)
    both(zoned, "x4_hp", lambda e: e.postprocess_u8(img, _pp(grid)), f"postprocess_u8 {H}x{W} grid {grid}")


def _banded(e, img, prm, step, fill=0x5A, after_band=None):
    H, W, _ = img.shape
    x = _dev_u8(img)
    y = torch.full_like(x, fill)
    st = torch.cuda.current_stream().cuda_stream
    e.pp_band_begin_dev(H, W, prm, 0, st)
    for a in range(0, H, step):
        e.pp_band_hist_dev(x.data_ptr(), a, min(a + step, H), st)
    e.pp_band_lut_dev(st)
    for a in range(0, H, step):
        e.pp_band_rows_dev(x.data_ptr(), a, min(a + step, H), y.data_ptr(), st)
        if after_band:
            torch.cuda.synchronize()
            after_band(min(a + step, H), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_postprocess_in_bands_of_five_rows(zoned):
    """70 x 101 in bands of 5 rows with the widest Gaussian the entries accept (sigma < 2.75: 17 taps, 8 rows of look-ahead,
    more than a band)"""
    img = _image(70, 101, 11)
    img[..., 1] = np.maximum(img[..., 1], 90)
    for grid in (8, 16):
        prm = _pp(grid, sigma=2.7)
        got = both(zoned, "x4_hp", lambda e: _banded(e, img, prm, 5), f"banded post-process, grid {grid}")
        same(got, baseline("x4_hp", lambda b: keep(b.postprocess_u8(img, prm))), "banded against the whole image")


# ---- pyramid -------------------------------------------------------------------------------------------------------------------------
def _scene(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([120 + 90 * np.sin(xx / 11.0 + c) * np.cos(yy / 7.0) + rng.integers(-15, 16, (h, w)) for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


def test_warp(zoned):
    rgb = _scene(150, 211, seed=32633)
    plan = tiles.plan_warp(211, 150, geo.Placement(600000.0, 5100000.0, 2.5, 2.5), geo.CRS(32633))
    both(zoned, "x4_hp", lambda e: e.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w), "warp 150x211")


def test_base_and_two_overviews(zoned):
    rng = np.random.default_rng(9)
    rgba = np.concatenate([_scene(300, 420, seed=2), np.full((300, 420, 1), 255, np.uint8)], -1)
    rgba[..., 3] = np.where(rng.random((300, 420)) < 0.15, 0, 255)
    place = geo.Placement(1500017.3, 5999994.9, 3.1, 3.1)
    levels = tiles.plan_levels(place.bounds(420, 300), 12, 15)[:3]
    assert len(levels) == 3

    def run(e):
        out = [e.tiles_base_u8(rgba, *tiles.plan_base(levels[0], place, 420, 300))]
        for k in (1, 2):                            # the first from the host copy, the second from the level left on the device
            ox, oy = tiles.overview_offsets(levels[k], levels[k - 1])
            out.append(e.tiles_overview_u8(out[-1], ox, oy, levels[k].nx, levels[k].ny, on_device=(k == 2)))
        return tuple(out)
    both(zoned, "x4_hp", run, "base + two overviews of 300x420")


@pytest.mark.parametrize("filt", tiles.FILTERS)
def test_resample_overzoom(zoned, filt):
    box = (-3.7, -46.0, -3.7 + 512 / 9.0, 38.1)     # tests/test_gpu_resample.py OVERZOOM
    cols = tiles.plan_resample_axis(2 * 256, box[0], box[2], rm.W, filt)
    rows = tiles.plan_resample_axis(2 * 256, box[1], box[3], rm.H, filt)
    src = rm.source()
    both(zoned, "x4_hp", lambda e: e.tiles_resample_u8(src, cols, rows, 2, 2), f"over-zoom {filt}")


def test_tile_pngs_in_small_groups(zoned, tmp_path):
    """The 5 x 4 level of test_gpu_tiles.test_tile_png_groups_pipeline_writes_the_same_files in groups of 3 tiles: the stream
    buffers regrow between groups, so zoned buffers are freed -- and checked -- while the call runs."""
    rng = np.random.default_rng(23)
    H, W = 4 * 256, 5 * 256
    yy, xx = np.mgrid[0:H, 0:W]
    rgba = np.empty((H, W, 4), np.uint8)
    rgba[..., :3] = np.clip(120 + 80 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 23.0)[..., None] + rng.integers(-4, 5, (H, W, 3)), 0, 255)
    rgba[256:512, 512:768, :3] = rng.integers(0, 256, (256, 256, 3))
    rgba[..., 3] = 255
    rgba[768:, :256, 3] = 0
    rgba[:128, 1024:, 3] = 0
    iy, ix = np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32)

    def run(e, sub):
        e.tiles_base_u8(rgba, ix, ix, iy, iy, fetch=False)
        paths = [tmp_path / sub / f"{j}_{i}.png" for j in range(4) for i in range(5)]
        paths[7] = None
        wrote = e.tiles_write_png(5, 4, paths, small_groups=True)
        return wrote.copy(), [None if q is None or not q.exists() else q.read_bytes() for q in paths]
    e = zoned("x4_hp")
    wrote, files = run(e, "zoned")
    wrote0, files0 = baseline("x4_hp", lambda b: run(b, "plain"))
    assert np.array_equal(wrote, wrote0) and files == files0 and sum(f is not None for f in files) == 18
    clean(e)


# ---- display -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,band_rows", [(37, 53, 7), (255, 257, 0)])
def test_display(zoned, H, W, band_rows):
    lut = np.random.default_rng(99).integers(0, 256, size=(3, 65536), dtype=np.uint8)
    img = np.random.default_rng(H).integers(0, 65536, (H, W, 3)).astype(np.uint16)
    both(zoned, "x4_hp", lambda e: e.display_hist_u16(img, band_rows=band_rows), f"display_hist_u16 {H}x{W}")
    both(zoned, "x4_hp", lambda e: e.display_hist_u16(img, nodata=int(img[0, 0, 0]), band_rows=band_rows), f"display_hist_u16 nodata {H}x{W}")
    both(zoned, "x4_hp", lambda e: e.display_apply_u16(img, lut, band_rows=band_rows), f"display_apply_u16 {H}x{W}")

    def behind_enhance(e):                          # the device copy enhance_u16 leaves: 4H x 4W
        with e.chain_lock:
            q = keep(e.enhance_u16(img))
            h = e.display_hist_u16(None, band_rows=band_rows, shape=(4 * H, 4 * W))
            a = e.display_apply_u16(None, lut, band_rows=band_rows, shape=(4 * H, 4 * W))
        return q, h, a
    both(zoned, "x4_hp", behind_enhance, f"display behind enhance_u16 {H}x{W}")


# ---- calibration ---------------------------------------------------------------------------------------------------------------------
def test_calibrate_fp8(zoned):
    """engines of their own on both sides: a calibration changes the scales of the handle it runs on"""
    t8 = np.random.default_rng(5).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    zoned("x4_hp")                                  # the mode is on
    e = _new_engine("x4_fp8")
    native.redzone(0)
    try:
        b = _new_engine("x4_fp8")
        try:
            want = b.calibrate_fp8(t8), keep(b.forward_batch_u8(t8))
            assert b.redzone_check()[:2] == (0, 0)  # nothing of the plain engine's has zones
        finally:
            b.close()
    finally:
        native.redzone(Z)
    try:
        assert e.calibrate_fp8(t8) == want[0]
        same(keep(e.forward_batch_u8(t8)), want[1], "forward after the calibration")
        clean(e)
    finally:
        e.close()
    assert zoned("x4_hp").redzone_check()[1] == 0   # ... and the frees of the two found nothing


# ---- the controls --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot,offset,side,at", [(1, 0, "back", 0), (1, Z - 1, "back", Z - 1), (1, -1, "front", Z - 1), (4, 17, "back", 17)])
def test_a_poked_zone_is_reported_once_with_side_and_offset(zoned, slot, offset, side, at):
    e = zoned("x4_hp")
    img16 = np.random.default_rng(3).integers(0, 65536, (39, 39, 3)).astype(np.uint16)
    want = keep(e.enhance_u16(img16, tile=16, pad=3))             # takes scratch 0, 1, 2 and 4
    clean(e)
    e.redzone_poke(slot, offset)
    n, bad, msg = e.redzone_check()
    print(msg)
    assert bad == 1 and n >= 4
    assert f"{side} zone damaged at offset {at}:" in msg and msg.startswith("redzone: allocation of "), msg
    clean(e)                                                      # reported once: the zone was patterned again
    same(keep(e.enhance_u16(img16, tile=16, pad=3)), want, "the engine after a poke")
    clean(e)


def test_pokes_outside_a_zone_are_refused(zoned):
    e = zoned("x4_hp")
    e.enhance_u16(np.zeros((39, 39, 3), np.uint16), tile=16, pad=3)
    for slot, offset in ((1, Z), (1, -Z - 1), (4, 1 << 40), (6, 0), (-1, 0)):
        with pytest.raises(native.S2srError, match="invalid argument"):
            e.redzone_poke(slot, offset)
    e.redzone_poke(1, -Z)                                         # the first byte of the front zone is inside
    n, bad, msg = e.redzone_check()
    assert bad == 1 and "front zone damaged at offset 0:" in msg, msg
    clean(e)


def test_with_the_mode_off_nothing_is_zoned(zoned):
    e0 = zoned("x4_hp")
    native.redzone(0)
    try:
        e = _new_engine("x4_hp")
        try:
            e.enhance_u16(np.zeros((39, 39, 3), np.uint16), tile=16, pad=3)
            for slot in range(6):
                with pytest.raises(native.S2srError, match="no red zone"):
                    e.redzone_poke(slot, 0)
            n, bad, _ = e.redzone_check()
            assert (n, bad) == (0, 0)
        finally:
            e.close()
    finally:
        native.redzone(Z)
    clean(e0)
    for bad in (1, 4095, 65536 + 512):
        with pytest.raises(native.S2srError):
            native.redzone(bad)
    e0.enhance_u8(_image(20, 20, 1))                              # a refused size changed nothing: still Z
    clean(e0)


# ---- caller-owned buffers ------------------------------------------------------------------------------------------------------------
FRONT, BACK = 4100, 4096          # tests/test_gpu_compact_insitu.py: the output starts 4-byte aligned and no better
FILLS = (0x5A, 0xA5)


def _guarded(nbytes, fill, front=FRONT):
    buf = torch.full((front + nbytes + BACK,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[front:front + nbytes]


def _outside_untouched(buf, fill, a, b, what):
    got = buf.cpu().numpy()
    assert (got[:a] == fill).all(), f"{what} wrote in front of its output"
    assert (got[b:] == fill).all(), f"{what} wrote behind its output"
    return got[a:b]


@pytest.mark.parametrize("B,th,tw", [(1, 9, 35), (5, 37, 45)])
@pytest.mark.parametrize("name", ["x4_hp", "x4_f16", "x4_fp8", "x2plus"])
def test_caller_owned_output_u8(zoned, name, B, th, tw):
    e = zoned(name)
    S = CONFIGS[name][2]
    if S == 2:
        th, tw = 2 * th, 2 * tw
    t8 = np.random.default_rng(B + th).integers(0, 256, (B, th, tw, 3), dtype=np.uint8)
    exp = keep(e.forward_batch_u8(t8))
    x = _dev_u8(t8)
    st = torch.cuda.current_stream().cuda_stream
    per = S * S * th * tw * 3
    part = 2 if B > 2 else 1
    first = B - part
    for fill in FILLS:
        buf, out = _guarded(B * per, fill)
        e.forward_batch_u8_dev(x.data_ptr(), B, th, tw, out.data_ptr(), st)
        torch.cuda.synchronize()
        got = _outside_untouched(buf, fill, FRONT, FRONT + B * per, "forward_batch_u8_dev")
        assert np.array_equal(got.reshape(exp.shape), exp), fill
        buf.fill_(fill)
        e.forward_part_u8_dev(x[first:].data_ptr(), part, th, tw, B, out[first * per:].data_ptr(), st)
        torch.cuda.synchronize()
        got = _outside_untouched(buf, fill, FRONT + first * per, FRONT + B * per, "forward_part_u8_dev")
        assert np.array_equal(got.reshape(exp[first:].shape), exp[first:]), fill
    clean(e)


@pytest.mark.parametrize("lo,hi", [FULL, SUB])
def test_caller_owned_output_u16(zoned, lo, hi):
    """the entry wants its output 8-byte aligned (include/s2sr.h): the guards are 4104 and 4096 bytes"""
    e = zoned("x4_hp")
    B, th, tw = 3, 50, 33
    t16 = np.random.default_rng(6).integers(0, 13000 if hi < 65535 else 65536, (B, th, tw, 3)).astype(np.uint16)
    exp = keep(e.forward_batch_u16(t16, lo, hi))
    x = torch.from_numpy(t16.view(np.int16).copy()).cuda()
    nbytes = exp.nbytes
    for fill in FILLS:
        buf, out = _guarded(nbytes, fill, front=4104)
        assert out.data_ptr() % 8 == 0 and out.data_ptr() % 16 != 0
        e.forward_batch_u16_dev(x.data_ptr(), B, th, tw, out.data_ptr(), lo, hi, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = _outside_untouched(buf, fill, 4104, 4104 + nbytes, "forward_batch_u16_dev")
        assert np.array_equal(got.view(np.uint16).reshape(exp.shape), exp), fill
    clean(e)
    buf, out = _guarded(nbytes, 0x5A)               # FRONT = 4100: not 8-byte aligned, refused before anything is written
    with pytest.raises(native.S2srError):
        e.forward_batch_u16_dev(x.data_ptr(), B, th, tw, out.data_ptr(), lo, hi, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A).all()


def test_caller_owned_output_postprocess_batch(zoned):
    e = zoned("x4_hp")
    B, H, W = 3, 35, 203
    imgs = np.random.default_rng(12).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    imgs[..., 1] = np.maximum(imgs[..., 1], 90)
    x = _dev_u8(imgs)
    for prm in (native.pp_wow(), native.pp_farm()):
        exp = np.stack([keep(e.postprocess_u8(imgs[i], prm)) for i in range(B)])
        for fill in FILLS:
            buf, out = _guarded(imgs.nbytes, fill)
            e.postprocess_batch_u8_dev(x.data_ptr(), B, H, W, prm, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = _outside_untouched(buf, fill, FRONT, FRONT + imgs.nbytes, "postprocess_batch_u8_dev")
            assert np.array_equal(got.reshape(exp.shape), exp), fill
    clean(e)


def test_caller_owned_output_pp_band_rows(zoned):
    """band by band into a filled whole image: after each band the rows not yet written still hold the fill"""
    e = zoned("x4_hp")
    H, W = 70, 101
    img = _image(H, W, 13)
    img[..., 1] = np.maximum(img[..., 1], 90)
    row = W * 3
    for prm in (native.pp_wow(), _pp(16, sigma=2.7)):
        exp = keep(e.postprocess_u8(img, prm))
        for fill in FILLS:
            x = _dev_u8(img)
            buf, out = _guarded(img.nbytes, fill)
            st = torch.cuda.current_stream().cuda_stream
            e.pp_band_begin_dev(H, W, prm, 0, st)
            e.pp_band_hist_dev(x.data_ptr(), 0, H, st)
            e.pp_band_lut_dev(st)
            for a in range(0, H, 5):
                b = min(a + 5, H)
                e.pp_band_rows_dev(x.data_ptr(), a, b, out.data_ptr(), st)
                torch.cuda.synchronize()
                got = _outside_untouched(buf, fill, FRONT, FRONT + b * row, f"pp_band_rows_dev rows {a}..{b}")
                assert np.array_equal(got.reshape(b, W, 3), exp[:b]), (fill, a)
    clean(e)
