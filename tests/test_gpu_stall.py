"""Every door of the library under stalled streams: no door's bytes may depend on which stream runs first.

The parity tests ask whether a kernel wrote the right values, the red zones whether it wrote outside its buffer, poison whether it
read bytes nobody wrote.  This module asks the fourth question: does every consumer wait for its producer when the two sit on
different streams -- the compute stream (the handle's, or the one a *_dev door was given) against the handle's copy stream, and
two calls on one handle that run on different streams?  A missing or mis-indexed wait changes no byte on an idle card at natural
timing, where the producer happens to be done in time.  The library's stall mode (include/s2sr.h s2sr_debug_delay; csrc/stall.hip,
the wrappers of csrc/engine_internal.h) holds one side back with a kernel that only lets time pass, at the head of every stream
segment, so the producer is provably late; poison and a saturated predecessor make the stale bytes provably different.
  (a) every door of tests/doors.py (the table the red-zone and the poison module judge too), on a real side stream, with the
      compute side stalled (mode 1) and the copy side (mode 2), returns byte for byte what the call returns on the cached engine
      with every mode off (diag.baseline); net doors in three sightings (direct launches, the graph capture, a replay); the
      workspace counter does not move.
  (b) the *_dev doors as stream citizens: input arriving late on the caller's stream from pinned memory, an in-stream consumer,
      a stream synchronise only -- no device-wide synchronise anywhere.
  (c) two calls on one handle, two streams, nothing in between, timed so that they overlap.
  (d) the controls: with one droppable wait dropped (s2sr_debug_delay_drop) the door that runs through it must return WRONG
      bytes, and the right ones again once the wait is back.
  (e) the precondition: the handle's two streams, and the torch side streams against them, really run side by side.  A process
      gets a few hardware queues and the runtime spreads its streams over them, so two streams may share one and are then
      serialised: every engine of the module is probed when it is made, and each side stream is picked by the same probe.
Nothing here can fault even where the library is wrong: (c) runs two calls of one geometry (tables and plans byte-identical), (d)
drops only waits whose stream next copies finished pixels, stalls are bounded (20 ms, and an iteration cap).

STALL_USEC: profiles/stall_sensitivity.txt -- four times the smallest of 100, 300, 1000, 3000 us at which every control of (d)
differed from its baseline in each of 5 consecutive runs in a fresh process."""
import os
import time

import numpy as np
import pytest
import torch

import diag
import doors
import gpu_engines
from diag import baseline, keep, same
from doors import DOORS, FILL, Inputs
from s2sr import native

pytestmark = pytest.mark.gpu

# profiles/stall_sensitivity.txt: 4 x 300.  The override is tools/stall_sensitivity.py's, which measures that figure.
STALL_USEC = int(os.environ.get("S2SR_TEST_STALL_USEC", "1200"))
CONFIGS, NET_SHAPES, IMAGES, SUB = doors.CONFIGS, doors.NET_SHAPES, doors.IMAGES, doors.SUB


@pytest.fixture(scope="module")
def stalled():
    """name -> an engine created under poison pattern 2 (so poison_scratch() is allowed), its two streams probed; at the end the
    three modes are put back to what the module found."""
    (mode, usec), dropped = native.delay_mode(), native.delay_dropped()
    probed = set()
    with diag.engines_under(native.poison_pattern, native.poison) as made:
        def get(name):
            e = made(name, 2)
            if name not in probed:
                probed.add(name)
                assert _beside(e, (0, 0), (1, 0)) and _beside(e, (1, 0), (0, 0)), f"{name}: the engine's stream and its copy stream share a hardware queue"
            return e
        yield get
    native.delay_drop(dropped)
    native.delay(mode, usec)


PROBE_USEC = 5000


def _beside(e, stalled_one, other_one):
    """(e) Do two streams run side by side?  Each is (which, stream) as s2sr_debug_stall takes them.  One sits in a stall of
    PROBE_USEC, a 64-byte memset goes to the other, and the host waits for that memset.  On one hardware queue the wait takes at
    least the stall, on independent queues tens of microseconds: under half the stall counts as side by side.  The seconds
    of the last probe stay in _beside.last, for the messages."""
    torch.cuda.synchronize()
    e.stall(stalled_one[0], 10, stalled_one[1])                          # warm: the first use of a stream or a kernel is not what is measured
    e.stream_touch(other_one[0], other_one[1], wait=True)
    torch.cuda.synchronize()
    e.stall(stalled_one[0], PROBE_USEC, stalled_one[1])
    t0 = time.perf_counter()
    e.stream_touch(other_one[0], other_one[1], wait=True)
    _beside.last = time.perf_counter() - t0
    torch.cuda.synchronize()
    return _beside.last < 0.5 * PROBE_USEC * 1e-6


_SIDE = {}


def _pick(e, beside, what):
    """A torch stream that runs side by side with every stream of `beside` ((which, stream) pairs of engine e).  A process gets a
    few hardware queues and the runtime spreads its streams over them, so a given torch stream may share a queue with one of the
    engine's; torch hands out the 32 streams of its pool in turn.  None that qualifies among them fails the caller: a stall on a
    stream that is serialised with the stream it is meant to overtake shows nothing."""
    for _ in range(32):
        s = torch.cuda.Stream()
        me = (2, s.cuda_stream)
        if all(_beside(e, me, o) and _beside(e, o, me) for o in beside):
            return s
    raise AssertionError(f"no torch stream runs side by side with {what}")


@pytest.fixture(scope="module")
def side():
    """e -> a side stream that runs beside both of e's streams (picked once per engine)"""
    def get(e):
        if id(e) not in _SIDE:
            _SIDE[id(e)] = (e, _pick(e, [(0, 0), (1, 0)], "the engine's stream and its copy stream"))
        return _SIDE[id(e)][1]
    yield get
    _SIDE.clear()


@pytest.fixture(autouse=True)
def _modes_off_between_tests():
    yield
    native.delay(0)
    native.delay_drop(-1)


# ---- (a) the door matrix under stalls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ident", list(DOORS))
def test_door_under_stalls(stalled, side, ident, mode):
    name, fn = DOORS[ident]
    e = stalled(name)
    side = side(e)
    want = baseline(ident)
    native.poison(0)
    with torch.cuda.stream(side):
        fn(e, Inputs(dirty=True))                                       # large stale values in every reused plane and staging buffer
    allocs = e.debug_config()["ws_allocs"]
    sightings = 3 if "-forward_" in ident else 1                    # net doors: direct launches, the capture, a replay
    native.poison(2)
    for k in range(sightings):
        torch.cuda.synchronize()
        e.poison_scratch()
        native.delay(mode, STALL_USEC)
        try:
            with torch.cuda.stream(side):
                got = keep(fn(e, Inputs()))
        finally:
            native.delay(0)
        same(got, want, f"{ident}, mode {mode}, sighting {k + 1}")
    assert e.debug_config()["ws_allocs"] == allocs, "the workspace was reallocated between the dirty call and the judged one"


# ---- (b) the *_dev doors as stream citizens ------------------------------------------------------------------------------------------
def _late(e, side, host, fill=FILL):
    """a device buffer that holds `fill` and, behind a stall on the caller's stream, receives `host` from pinned memory"""
    pinned = torch.from_numpy(np.ascontiguousarray(host)).pin_memory()
    x = torch.full(pinned.shape, fill, dtype=pinned.dtype, device="cuda")
    side.synchronize()                                                  # the fill is through: what a door that runs early would read
    e.stall(2, STALL_USEC, side.cuda_stream)
    x.copy_(pinned, non_blocking=True)
    return x, pinned


def _net_case(shape):
    B, th, tw, job = NET_SHAPES[shape]
    return (B, th, tw, 3), B * 10000 + th * 100 + tw, job             # doors._net_doors: dims, seed


def _citizen(side, body):
    """body() on the side stream, then the in-stream consumer; only the side stream is synchronised"""
    with torch.cuda.stream(side):
        y = body()
        z = tuple(t.clone() for t in y) if isinstance(y, tuple) else y.clone()
        side.synchronize()
    return tuple(t.cpu().numpy() for t in z) if isinstance(z, tuple) else z.cpu().numpy()


@pytest.mark.parametrize("shape", ["ragged_2x37x53", "mosaic_9x20x20"])
def test_forward_batch_u8_dev_is_a_stream_citizen(stalled, side, shape):
    e = stalled("x4_hp")
    side = side(e)
    dims, seed, _ = _net_case(shape)
    B, th, tw, _ = dims

    def body():
        x, _keep = _late(e, side, Inputs().u8(dims, seed))
        y = doors._out((B, 4 * th, 4 * tw, 3))
        e.forward_batch_u8_dev(x.data_ptr(), B, th, tw, y.data_ptr(), side.cuda_stream)
        return y
    for k in range(3):                                                  # direct launches, the capture, a replay
        same(_citizen(side, body), baseline(f"x4_hp-{shape}-forward_batch_u8_dev"), f"{shape}, sighting {k + 1}")


@pytest.mark.parametrize("shape", ["ragged_2x37x53", "mosaic_9x20x20"])
def test_forward_batch_u16_dev_is_a_stream_citizen(stalled, side, shape):
    e = stalled("x4_hp")
    side = side(e)
    dims, seed, _ = _net_case(shape)
    B, th, tw, _ = dims

    def body():
        x, _keep = _late(e, side, Inputs().u16(dims, seed + 1).view(np.int16), fill=0x5A5A)
        y = torch.full((B, 4 * th, 4 * tw, 3), 0x5A5A, dtype=torch.int16, device="cuda")
        e.forward_batch_u16_dev(x.data_ptr(), B, th, tw, y.data_ptr(), *SUB, stream=side.cuda_stream)
        return y
    for k in range(3):
        same(_citizen(side, body).view(np.uint16), baseline(f"x4_hp-{shape}-forward_batch_u16_dev"), f"{shape}, sighting {k + 1}")


def test_forward_part_u8_dev_is_a_stream_citizen(stalled, side):
    e = stalled("x4_hp")
    side = side(e)
    dims, seed, job = _net_case("dead_7of9x20x20")                      # the only shape with a part door: 7 windows of a job of 9
    B, th, tw, _ = dims

    def body():
        x, _keep = _late(e, side, Inputs().u8(dims, seed))
        y = torch.zeros((B, 4 * th, 4 * tw, 3), dtype=torch.uint8, device="cuda")
        e.forward_part_u8_dev(x.data_ptr(), B, th, tw, job, y.data_ptr(), side.cuda_stream)
        return y
    for k in range(3):
        same(_citizen(side, body), baseline("x4_hp-dead_7of9x20x20-forward_part_u8_dev"), f"sighting {k + 1}")


@pytest.mark.parametrize("case", ["banded", "short_ramps"])
def test_cut_and_stitch_dev_are_stream_citizens(stalled, side, case):
    e = stalled("x4_hp")
    side = side(e)
    H, W, tile, pad = IMAGES[case]
    T, wh, ww = doors._plan(e, H, W, tile, pad)

    def cut():
        img, _keep = _late(e, side, Inputs().u8((H, W, 3), H + W))
        buf = doors._out((T, wh, ww, 3))
        e.cut_windows_u8_dev(img.data_ptr(), H, W, tile, pad, 0, T, buf.data_ptr(), side.cuda_stream)
        return buf
    want = baseline(f"x4_hp-{case}-cut_windows")
    same(_citizen(side, cut), want[0] if isinstance(want, tuple) else want, f"{case} cut_windows_u8_dev")

    def stitch(rows):
        def body():
            d_tiles, _keep = _late(e, side, Inputs().u8((T, 4 * wh, 4 * ww, 3), H * W))
            out = doors._out((4 * H, 4 * W, 3))
            if not rows:
                e.stitch_windows_u8_dev(d_tiles.data_ptr(), H, W, tile, pad, out.data_ptr(), side.cuda_stream)
            else:                                                       # doors._stitch: bottom band first
                cuts = [0, 1, 7, 4 * H // 2 + 1, 4 * H]
                for a, b in reversed(list(zip(cuts[:-1], cuts[1:]))):
                    e.stitch_rows_u8_dev(d_tiles.data_ptr(), H, W, tile, pad, a, b, out.data_ptr(), side.cuda_stream)
            return out
        return body
    same(_citizen(side, stitch(False)), baseline(f"x4_hp-{case}-stitch_windows"), f"{case} stitch_windows_u8_dev")
    same(_citizen(side, stitch(True)), baseline(f"x4_hp-{case}-stitch_rows"), f"{case} stitch_rows_u8_dev")


def test_postprocess_dev_doors_are_stream_citizens(stalled, side):
    e = stalled("x4_hp")
    side = side(e)
    H, W, prm = 67, 101, native.pp_wow()

    def batch():
        x, _keep = _late(e, side, Inputs().green((3, H, W, 3), 12))
        y = doors._out((3, H, W, 3))
        e.postprocess_batch_u8_dev(x.data_ptr(), 3, H, W, prm, y.data_ptr(), side.cuda_stream)
        return y
    same(_citizen(side, batch), baseline(f"postprocess_batch_u8_dev-{H}x{W}-wow"), "postprocess_batch_u8_dev")

    def bands():                                                        # doors._banded, on the side stream and without its synchronise
        x, _keep = _late(e, side, Inputs().green((H, W, 3), 11))
        y = torch.full_like(x, FILL)
        st = side.cuda_stream
        e.pp_band_begin_dev(H, W, prm, 0, st)
        for a in range(0, H, 5):
            e.pp_band_hist_dev(x.data_ptr(), a, min(a + 5, H), st)
        e.pp_band_lut_dev(st)
        for a in range(0, H, 5):
            e.pp_band_rows_dev(x.data_ptr(), a, min(a + 5, H), y.data_ptr(), st)
        return y
    same(_citizen(side, bands), baseline(f"pp_band_sequence-{H}x{W}-wow"), "the pp_band sequence")


def test_copy_to_host_is_a_stream_citizen(stalled, side):
    e = stalled("x4_hp")
    side = side(e)
    src = Inputs().u8((37, 53, 3), 77)
    dst = np.full_like(src, FILL)
    with torch.cuda.stream(side):
        x, _keep = _late(e, side, src)
        e.copy_to_host(dst, x.data_ptr(), side.cuda_stream)             # returns when the bytes are there: nothing to synchronise
    assert np.array_equal(dst, src)


def test_load_weights_dev_then_a_forward(stalled, side):
    """the blob arrives late on the caller's stream; the forward follows on the same stream"""
    from s2sr.weights import flatten_state_dict
    nb, prec, scale, arch = CONFIGS["x4_hp"]
    blob = flatten_state_dict(gpu_engines.state_dict(nb, scale, arch), nb, scale=scale, arch=arch)
    dims, seed, _ = _net_case("ragged_2x37x53")
    B, th, tw, _ = dims
    native.poison(2)
    e = native.Engine(num_block=nb, precision=prec, scale=scale, arch=arch)
    try:
        side = side(e)

        def body():
            d_blob, _keep = _late(e, side, blob.view(np.int32), fill=0x5A5A5A5A)
            e.load_blob_dev(d_blob.data_ptr(), blob.size, side.cuda_stream)
            x, _keep2 = _late(e, side, Inputs().u8(dims, seed))
            y = doors._out((B, 4 * th, 4 * tw, 3))
            e.forward_batch_u8_dev(x.data_ptr(), B, th, tw, y.data_ptr(), side.cuda_stream)
            return y
        same(_citizen(side, body), baseline("x4_hp-ragged_2x37x53-forward_batch_u8_dev"), "forward behind s2sr_load_weights_dev")
    finally:
        e.close()


# ---- (c) two calls on one handle, two streams, nothing in between --------------------------------------------------------------------
# Both streams get their stall first, A's of PAIR_T and the other's of PAIR_T + PAIR_LEAD, then the two calls are made back to back
# (both enqueues fit well inside PAIR_T): the second call's work starts PAIR_LEAD after the first call's work began, while that work
# still runs -- the two streams run side by side, section (e).  At these settings a build without the handle's order event returns
# wrong bytes in the three forward pairs (profiles/stall_sensitivity.txt); the post-process, cut and stitch pairs guard the same
# contract but did not show the bug there.  Both calls of a pair have one geometry -- tables, plans and workspace layout are
# byte-identical -- so a race can only corrupt pixel values.
PAIR_T, PAIR_LEAD = 2000, 150
PAIR_SHAPE = (8, 64, 64, 3)


def _ref(fn):
    """fn(the cached engine) alone, everything synchronised before and after"""
    with diag.modes_off():
        torch.cuda.synchronize()
        r = keep(fn(gpu_engines.default(*CONFIGS["x4_hp"])))
        torch.cuda.synchronize()
    return r


@pytest.fixture(scope="module")
def other(side):
    """e -> a second side stream, beside the first one and the engine's own stream"""
    made = {}

    def get(e):
        if id(e) not in made:
            made[id(e)] = (e, _pick(e, [(0, 0), (2, side(e).cuda_stream)], "the engine's stream and the first side stream"))
        return made[id(e)][1]
    return get


def _both_streams_done(*streams):
    for s in streams:
        s.synchronize()


def test_pair_forward_u8_dev_then_forward_u8(stalled, side):
    e = stalled("x4_hp")
    side = side(e)
    B, th, tw, _ = PAIR_SHAPE
    t1, t2 = Inputs().u8(PAIR_SHAPE, 1), Inputs().u8(PAIR_SHAPE, 2)
    want1, want2 = _ref(lambda b: b.forward_batch_u8(t1)), _ref(lambda b: b.forward_batch_u8(t2))
    x1, y1 = doors._dev_u8(t1), doors._out((B, 4 * th, 4 * tw, 3))
    for k in range(3):                                                  # direct launches, the capture, a replay
        y1.fill_(FILL)
        torch.cuda.synchronize()
        e.stall(2, PAIR_T, side.cuda_stream)
        e.stall(0, PAIR_T + PAIR_LEAD)
        e.forward_batch_u8_dev(x1.data_ptr(), B, th, tw, y1.data_ptr(), side.cuda_stream)
        got2 = keep(e.forward_batch_u8(t2))
        side.synchronize()
        same(y1.cpu().numpy(), want1, f"the *_dev call on the side stream, sighting {k + 1}")
        same(got2, want2, f"the host-facing call behind it, sighting {k + 1}")


def test_pair_forward_u8_dev_on_two_streams(stalled, side, other):
    e = stalled("x4_hp")
    side, other = side(e), other(e)
    B, th, tw, _ = PAIR_SHAPE
    t1, t2 = Inputs().u8(PAIR_SHAPE, 3), Inputs().u8(PAIR_SHAPE, 4)
    want1, want2 = _ref(lambda b: b.forward_batch_u8(t1)), _ref(lambda b: b.forward_batch_u8(t2))
    x1, x2 = doors._dev_u8(t1), doors._dev_u8(t2)
    y1, y2 = doors._out((B, 4 * th, 4 * tw, 3)), doors._out((B, 4 * th, 4 * tw, 3))
    for k in range(3):
        y1.fill_(FILL), y2.fill_(FILL)
        torch.cuda.synchronize()
        e.stall(2, PAIR_T, side.cuda_stream)
        e.stall(2, PAIR_T + PAIR_LEAD, other.cuda_stream)
        e.forward_batch_u8_dev(x1.data_ptr(), B, th, tw, y1.data_ptr(), side.cuda_stream)
        e.forward_batch_u8_dev(x2.data_ptr(), B, th, tw, y2.data_ptr(), other.cuda_stream)
        _both_streams_done(side, other)
        same(y1.cpu().numpy(), want1, f"stream A, sighting {k + 1}")
        same(y2.cpu().numpy(), want2, f"stream B, sighting {k + 1}")


def test_pair_forward_u16_dev_then_forward_u16(stalled, side):
    """both keep the net's fp32 tiles in scratch 1"""
    e = stalled("x4_hp")
    side = side(e)
    B, th, tw, _ = PAIR_SHAPE
    t1, t2 = Inputs().u16(PAIR_SHAPE, 5), Inputs().u16(PAIR_SHAPE, 6)
    want1, want2 = _ref(lambda b: b.forward_batch_u16(t1, *SUB)), _ref(lambda b: b.forward_batch_u16(t2, *SUB))
    x1 = torch.from_numpy(t1.view(np.int16).copy()).cuda()
    y1 = torch.full((B, 4 * th, 4 * tw, 3), 0x5A5A, dtype=torch.int16, device="cuda")
    e.forward_batch_u16(t2, *SUB)                                       # scratch 0 .. 2 at their sizes: no regrow between the two calls
    for k in range(3):
        y1.fill_(0x5A5A)
        torch.cuda.synchronize()
        e.stall(2, PAIR_T, side.cuda_stream)
        e.stall(0, PAIR_T + PAIR_LEAD)
        e.forward_batch_u16_dev(x1.data_ptr(), B, th, tw, y1.data_ptr(), *SUB, stream=side.cuda_stream)
        got2 = keep(e.forward_batch_u16(t2, *SUB))
        side.synchronize()
        same(y1.cpu().numpy().view(np.uint16), want1, f"the *_dev call on the side stream, sighting {k + 1}")
        same(got2, want2, f"the host-facing call behind it, sighting {k + 1}")


def test_pair_postprocess_dev_then_postprocess_u8(stalled, side):
    """Both keep histograms, LUTs and the CLAHE'd image in scratch 5.  A guard of the contract only: the *_dev call computes for
    some 50 us, less than the twin's upload takes, and a build without the order event passed at every lead tried
    (profiles/stall_sensitivity.txt)."""
    e = stalled("x4_hp")
    side = side(e)
    H, W, prm = 512, 512, native.pp_wow()
    i1, i2 = Inputs().green((1, H, W, 3), 7), Inputs().green((H, W, 3), 8)
    want1, want2 = _ref(lambda b: b.postprocess_u8(i1[0], prm)), _ref(lambda b: b.postprocess_u8(i2, prm))
    x1, y1 = doors._dev_u8(i1), doors._out((1, H, W, 3))
    e.postprocess_u8(i2, prm)                                           # scratch at its sizes
    torch.cuda.synchronize()
    e.stall(2, PAIR_T, side.cuda_stream)
    e.stall(0, PAIR_T + PAIR_LEAD // 3)                                 # a post-process of 512 x 512 is short
    e.postprocess_batch_u8_dev(x1.data_ptr(), 1, H, W, prm, y1.data_ptr(), side.cuda_stream)
    got2 = keep(e.postprocess_u8(i2, prm))
    side.synchronize()
    same(y1.cpu().numpy()[0], want1, "the *_dev call on the side stream")
    same(got2, want2, "the host-facing call behind it")


def test_pair_cut_windows_dev_on_two_streams(stalled, side, other):
    """the same plan, so the same table bytes in scratch 3, other pixels"""
    e = stalled("x4_hp")
    side, other = side(e), other(e)
    H, W, tile, pad = IMAGES["banded"]
    T, wh, ww = doors._plan(e, H, W, tile, pad)
    i1, i2 = Inputs().u8((H, W, 3), 9), Inputs().u8((H, W, 3), 10)

    def cut(b, img, st):
        x, buf = doors._dev_u8(img), doors._out((T, wh, ww, 3))
        b.cut_windows_u8_dev(x.data_ptr(), H, W, tile, pad, 0, T, buf.data_ptr(), st.cuda_stream)
        return x, buf
    want = [_ref(lambda b, i=i: doors._back(cut(b, i, torch.cuda.current_stream())[1])) for i in (i1, i2)]
    torch.cuda.synchronize()
    x1, x2 = doors._dev_u8(i1), doors._dev_u8(i2)
    b1, b2 = doors._out((T, wh, ww, 3)), doors._out((T, wh, ww, 3))
    torch.cuda.synchronize()
    e.stall(2, PAIR_T, side.cuda_stream)
    e.stall(2, PAIR_T + PAIR_LEAD // 3, other.cuda_stream)
    e.cut_windows_u8_dev(x1.data_ptr(), H, W, tile, pad, 0, T, b1.data_ptr(), side.cuda_stream)
    e.cut_windows_u8_dev(x2.data_ptr(), H, W, tile, pad, 0, T, b2.data_ptr(), other.cuda_stream)
    _both_streams_done(side, other)
    same(b1.cpu().numpy(), want[0], "stream A")
    same(b2.cpu().numpy(), want[1], "stream B")


def test_pair_stitch_rows_dev_then_stitch_windows_dev(stalled, side, other):
    e = stalled("x4_hp")
    side, other = side(e), other(e)
    H, W, tile, pad = IMAGES["banded"]
    T, wh, ww = doors._plan(e, H, W, tile, pad)
    t1, t2 = Inputs().u8((T, 4 * wh, 4 * ww, 3), 11), Inputs().u8((T, 4 * wh, 4 * ww, 3), 12)

    def whole(b, tiles_u8):
        d, out = doors._dev_u8(tiles_u8), doors._out((4 * H, 4 * W, 3))
        b.stitch_windows_u8_dev(d.data_ptr(), H, W, tile, pad, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return doors._back(out)
    want1, want2 = _ref(lambda b: whole(b, t1)), _ref(lambda b: whole(b, t2))
    d1, d2 = doors._dev_u8(t1), doors._dev_u8(t2)
    o1, o2 = doors._out((4 * H, 4 * W, 3)), doors._out((4 * H, 4 * W, 3))
    torch.cuda.synchronize()
    e.stall(2, PAIR_T, side.cuda_stream)
    e.stall(2, PAIR_T + PAIR_LEAD // 3, other.cuda_stream)
    for a, b in ((0, 2 * H + 1), (2 * H + 1, 4 * H)):
        e.stitch_rows_u8_dev(d1.data_ptr(), H, W, tile, pad, a, b, o1.data_ptr(), side.cuda_stream)
    e.stitch_windows_u8_dev(d2.data_ptr(), H, W, tile, pad, o2.data_ptr(), other.cuda_stream)
    _both_streams_done(side, other)
    same(o1.cpu().numpy(), want1, "the bands on stream A")
    same(o2.cpu().numpy(), want2, "the whole image on stream B")


# ---- (d) the controls ---------------------------------------------------------------------------------------------------------------
def _differs(got, want):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    return any(g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))


def _control(e, site, call, want, what):
    """mode 1 and `site` dropped: wrong bytes; the wait back: the baseline again"""
    native.poison(2)
    torch.cuda.synchronize()
    e.poison_scratch()                                                  # what a copy that runs early finds
    native.delay(1, STALL_USEC)
    native.delay_drop(site)
    try:
        got = keep(call())
    finally:
        native.delay_drop(-1)
    assert _differs(got, want), f"{what}: the wait of site {site} was dropped and nobody noticed"
    try:
        again = keep(call())
    finally:
        native.delay(0)
    same(again, want, f"{what}, the wait restored")
    same(keep(call()), want, f"{what}, the mode off")


def test_control_batch_group_wait(stalled):
    nb, prec, scale, arch = CONFIGS["x4_hp"]
    native.poison(2)
    e = native.Engine(num_block=nb, precision=prec, scale=scale, arch=arch, group=1)    # B = 3 in groups of one
    try:
        e.load_state_dict(gpu_engines.state_dict(nb, scale, arch))
        assert _beside(e, (0, 0), (1, 0)), "the engine's stream and its copy stream share a hardware queue"
        t8 = Inputs().u8((3, 16, 32, 3), 31)
        want = _ref(lambda b: b.forward_batch_u8(t8))
        _control(e, native.SITE_BATCH_GROUP_D2H, lambda: e.forward_batch_u8(t8), want, "forward_batch_u8 in three groups")
    finally:
        e.close()


def test_control_chunk_band_wait(stalled):
    e = stalled("x4_hp")
    H, W, tile, pad = IMAGES["chunked"]
    img = Inputs().u8((H, W, 3), 7 + 1000 * H + W)
    _control(e, native.SITE_CHUNK_BAND_D2H, lambda: e.enhance_u8(img, tile=tile, pad=pad), baseline("x4_hp-chunked-enhance_u8"),
             "enhance_u8 of the chunked image")


def test_control_display_band_wait(stalled):
    e = stalled("x4_hp")
    _control(e, native.SITE_DISPLAY_BAND_D2H, lambda: DOORS["display_apply_u16-bands7"][1](e, Inputs()), baseline("display_apply_u16-bands7"),
             "display_apply_u16 in bands of 7 rows")


def test_control_copy_to_host_wait(stalled, side):
    e = stalled("x4_hp")
    side = side(e)
    src = Inputs().u8((37, 53, 3), 78)

    def call():
        dst = np.full_like(src, FILL)
        with torch.cuda.stream(side):
            x, _keep = _late(e, side, src)
            e.copy_to_host(dst, x.data_ptr(), side.cuda_stream)
            side.synchronize()
        return dst
    _control(e, native.SITE_COPY_TO_HOST, call, src, "s2sr_copy_to_host")


def test_only_copy_consumed_waits_can_be_dropped():
    for site in range(-3, 40):
        if site == -1 or site in native.DROPPABLE_SITES:
            native.delay_drop(site)
            assert native.delay_dropped() == site
        else:
            with pytest.raises(native.S2srError):
                native.delay_drop(site)
    native.delay_drop(-1)
    for mode, usec in ((1, 0), (4, 100), (-1, 100), (1, native.STALL_MAX_USEC + 1), (3, -1)):
        with pytest.raises(native.S2srError):
            native.delay(mode, usec)
    assert native.delay_mode() == (0, 0)


# ---- (e) the precondition -----------------------------------------------------------------------------------------------------------
def test_a_stall_lasts_as_long_as_it_says(stalled):
    e = stalled("x4_hp")
    e.stall(0, 10)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.stall(0, PROBE_USEC)
    e.stream_touch(0, wait=True)
    dt = time.perf_counter() - t0
    print(f"a stall of {PROBE_USEC} us and the wait behind it: {dt * 1e6:.0f} us")
    assert 0.9 * PROBE_USEC * 1e-6 <= dt <= 10 * PROBE_USEC * 1e-6, dt
    for which, usec in ((3, 100), (-1, 100), (0, 0), (0, native.STALL_MAX_USEC + 1)):
        with pytest.raises(native.S2srError, match="s2sr_debug_stall"):
            e.stall(which, usec)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_streams_run_side_by_side(stalled, side, other, name):
    """A stall is worth something only if the streams it separates really run side by side: the engine's stream and its copy
    stream (asserted again here, with the figures), the side stream the other tests use against both, and the second side stream
    of (c) against the first.  Serialised on one hardware queue the memset waits at least the stall (_beside)."""
    e = stalled(name)
    s, o = (2, side(e).cuda_stream), (2, other(e).cuda_stream)
    pairs = {"compute stalled, copy runs": ((0, 0), (1, 0)), "copy stalled, compute runs": ((1, 0), (0, 0)),
             "side stalled, compute runs": (s, (0, 0)), "compute stalled, side runs": ((0, 0), s),
             "side stalled, copy runs": (s, (1, 0)), "copy stalled, side runs": ((1, 0), s),
             "side stalled, second side runs": (s, o), "second side stalled, side runs": (o, s), "second side stalled, compute runs": (o, (0, 0))}
    for what, (a, b) in pairs.items():
        ok = _beside(e, a, b)
        print(f"{name}, {what}: the memset was through after {_beside.last * 1e6:.0f} us of a {PROBE_USEC} us stall")
        assert ok, f"{name}, {what}: {_beside.last * 1e6:.0f} us -- the two streams do not run side by side"
