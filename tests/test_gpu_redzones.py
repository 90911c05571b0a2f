"""Every door of the library under red zones: no store may land outside the buffer it belongs to.

The parity tests read what a kernel was meant to write.  A stray vector store at a ragged edge, or a batch's last image running
one padded row long, lands in allocator slack or in the neighbouring workspace plane and changes no byte any of them reads.  Here
the library's red-zone mode (include/s2sr.h s2sr_debug_redzone; csrc/redzone.h) puts Z = 65536 patterned bytes in front of and
behind every device allocation and behind every workspace plane -- a whole padded row of these shapes is about 2 KB, so a
row-long overrun stays inside a zone -- and each door of tests/doors.py, the table the poison and the stall module judge too, must
  (a) return on an engine created under zones the bytes of the same call on an engine without them (diag.baseline: the cached
      engines of gpu_engines.py with every mode off, so whatever they allocate or regrow on the way has no zones), and
  (b) leave no damaged zone anywhere in the process, with a plausible number of zoned allocations (redzone_check()).
Beside the matrix: the banded post-process against the whole image, the 18 files of the PNG writer in small groups, the refusals
(16-bit input on x2plus and compact, odd tiles on x2plus) that must leave the zones clean, and fp8 calibration.  The controls poke
one wrong byte into a zone and must be caught, with side and offset.  The `_dev` doors write into the caller's memory, which the
library cannot zone: torch buffers with guard bytes around the output, two fills, no byte outside may change and every byte inside
must be written."""
import functools

import numpy as np
import pytest
import torch

import diag
import doors
from diag import Z, baseline, keep, new_engine, same
from doors import CONFIGS, DOORS, FULL, NET_SHAPES, SUB, Inputs
from s2sr import native

pytestmark = pytest.mark.gpu

clean = functools.partial(diag.clean, most=400)


@pytest.fixture(scope="module")
def zoned():
    """name -> a fresh engine created (and so allocated) with Z = 65536"""
    with diag.engines_under(native.redzone_bytes, native.redzone, Z) as get:
        yield get


# ---- the door matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ident", list(DOORS))
def test_door_under_red_zones(zoned, ident):
    name, fn = DOORS[ident]
    e = zoned(name)
    same(keep(fn(e, Inputs())), baseline(ident), f"{ident}, with red zones")
    clean(e)


@pytest.mark.parametrize("grid", [8, 16])
def test_postprocess_in_bands_of_five_rows_is_the_whole_image(grid):
    """70 x 101 in bands of 5 rows with the widest Gaussian the entries accept (sigma < 2.75: 17 taps, 8 rows of look-ahead,
    more than a band): the two doors run on one image"""
    same(baseline(f"pp_band_sequence-70x101-grid{grid}_wide"), baseline(f"postprocess_u8-70x101-grid{grid}_wide"), "banded against the whole image")


def test_tile_pngs_in_small_groups_are_18_files(zoned):
    """the 5 x 4 level has one transparent tile and one without a path"""
    wrote, *files = DOORS["tiles_write_png-small_groups_5x4"][1](zoned("x4_hp"), Inputs())
    assert wrote.sum() == 18 and sum(f.size > 0 for f in files) == 18
    assert not wrote[1, 2] and not wrote[3, 0]
    clean(zoned("x4_hp"))


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s, (_, _, _, job) in NET_SHAPES.items() if not job])
@pytest.mark.parametrize("name", ["x2plus", "compact"])
def test_16_bit_input_is_refused_off_the_x4_nets_and_the_zones_stay_clean(zoned, name, shape):
    B, th, tw, _ = NET_SHAPES[shape]
    if CONFIGS[name][2] == 2:
        th, tw = 2 * th, 2 * tw                      # the listed shape is the trunk grid
    with pytest.raises(native.S2srError, match="16-bit input is not available"):
        zoned(name).forward_batch_u16(Inputs().u16((B, th, tw, 3), B + th))
    clean(zoned(name))


def test_x2plus_refuses_odd_tiles_and_stays_clean(zoned):
    """why the x2plus net doors run doubled"""
    with pytest.raises(native.S2srError, match="even tile sizes"):
        zoned("x2plus").forward_batch_u8(np.zeros((1, 7, 45, 3), np.uint8))
    clean(zoned("x2plus"))


# ---- calibration ---------------------------------------------------------------------------------------------------------------------
def test_calibrate_fp8(zoned):
    """engines of their own on both sides: a calibration changes the scales of the handle it runs on"""
    t8 = np.random.default_rng(5).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    zoned("x4_hp")                                  # the mode is on
    e = new_engine("x4_fp8")
    native.redzone(0)
    try:
        b = new_engine("x4_fp8")
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
        e = new_engine("x4_hp")
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
    e0.enhance_u8(Inputs().u8((20, 20, 3), 1))                             # a refused size changed nothing: still Z
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
    x = doors._dev_u8(t8)
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
    x = doors._dev_u8(imgs)
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
    img = Inputs().green((H, W, 3), 13)
    row = W * 3
    for prm in (native.pp_wow(), doors._pp(16, sigma=2.7)):
        exp = keep(e.postprocess_u8(img, prm))
        for fill in FILLS:
            x = doors._dev_u8(img)
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
