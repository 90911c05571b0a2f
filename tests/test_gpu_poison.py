"""Every door of the library on poisoned memory: no door may read in-bounds bytes that nobody wrote in this call.

The parity tests ask whether a kernel wrote the right values, the red zones whether it wrote outside its buffer.  This module asks
the third question.  A handle's scratch slots grow and are never cleared, fresh device memory reads as zeros in practice, and the
workspace is zeroed once and reused -- so a histogram without its memset, a stream assembled with atomicOr, a carry buffer, a dead
mosaic window or a ragged patch edge reads a plausible value in every fresh process and something else in a long-lived one.  The
library's poison mode (include/s2sr.h s2sr_debug_poison; csrc/redzone.h namespace poison) fills what an allocation hands out, and
on request what the scratch slots hold, with 0xFF bytes (pattern 1: NaN as fp32 / fp16 / e4m3, -1 as an index) or with a
position-dependent non-zero byte (pattern 2).  Each door of tests/doors.py -- the table the red-zone and the
stall module judge too -- must return, byte for byte (dtype and shape included), what the same call returns on the cached engine of
gpu_engines.py with every mode off (diag.baseline), in three states:
  (a) fresh: on an engine created under poison, so every first allocation and every regrow is poisoned -- patterns 1 and 2;
  (b) scratch: poison_scratch() in front of every sighting -- the second sighting is the graph capture, the third (net doors) a
      replay -- the patterns taking turns from sighting to sighting;
  (c) dirty: the same call on a saturated input (255 / 65535) first, then the judged call: large stale values in every live
      interior element of the reused workspace; the workspace counter shows that nothing was reallocated in between.
The controls: poison_scratch() really fills what it reports, a poisoned engine's trash page holds the pattern, the doors that
consume what the last call left refuse after poison_scratch(), and with the mode off poison_scratch() is refused.

Garbage read as an index could send a load anywhere, so before this module first ran every ensure_scratch call site was read for
its index and offset tables: each is uploaded in full, on the stream of the kernel that reads it, before that kernel is queued.
(The slots by the names of enum Slot, csrc/engine_internal.h: SRC 0, DST 1, MID 2, TABLES 3, CHUNK 4, PP 5, VALID 6, CONS 7.)
  engine.hip forward_batch_u8_once SRC, DST: tiles uploaded whole; the net writes every output tile.  No table.
  engine.hip s2sr_forward_batch_u16_dev DST: the fp32 tiles, written by the net before the quantiser reads them.  No table.
  engine.hip forward_batch_u16_once SRC, DST, MID: tiles uploaded whole; fp32 tiles and the quantised image written in full.  No table.
  engine.hip forward_f32_once SRC, DST: input uploaded whole, output written by the net.  No table.
  engine.hip s2sr_calibrate_fp8 SRC, DST: as forward_batch_u8; the two maxima live in an allocation of their own, memset per pass.
  engine_aoi.hip upload_tables TABLES: rectangles, row table, column table, one behind the other, each copied whole, then a stream
    synchronise: gather, stitch, quantise and blend kernels are queued behind it.  (enhance_locked, s2sr_cut_windows_u8_dev.)
  engine_aoi.hip postprocess_dev_locked PP: histograms memset in launch_postprocess, LUTs and the CLAHE'd image written before read.
  engine_aoi.hip pp_band_begin_locked PP: histograms memset by launch_pp_band_begin; a run another call took scratch from is refused.
  engine_aoi.hip s2sr_postprocess_u8 SRC, DST: image uploaded whole; output written by the last stage.
  engine_aoi.hip enhance_locked SRC, DST, MID, CHUNK (MID untiled), VALID, CONS and CHUNK again for an unbanded post-process: image
    and mask uploaded whole; windows gathered for the whole plan; every chunk's tiles written by the net before the paste; the blend's carry row
    copied from the chunk before (the first chunk's tables never point in front of it); counters memset by cons_begin, mode 2's
    residual plane written by form 0 for the block rows form 2 reads.
  engine_aoi.hip consistency_impl SRC, DST, CONS: both images uploaded (the large one band by band, ahead of the pass), CONS as above.
  engine_aoi.hip fill_nodata_impl SRC, VALID: image and mask uploaded whole.
  engine_aoi.hip s2sr_stitch_rows_u8_dev: the paste maps are an allocation of their own, uploaded whole (blocking) before use.
  engine_tiles.hip s2sr_warp_bilinear_u8 SRC, DST, TABLES: raster and node grid uploaded whole; every output pixel written.
  engine_tiles.hip s2sr_tiles_base_u8 SRC / DST, TABLES: the four footprint tables (checked against the raster on the host) uploaded whole.
  engine_tiles.hip s2sr_tiles_overview_u8 SRC / DST: child level uploaded whole or left by the call before; no table.
  engine_tiles.hip s2sr_tiles_resample_u8 SRC / DST, MID, TABLES: both packed tap tables (checked on the host) in one copy; the intermediate
    rows the vertical pass reads are the rows the horizontal pass writes (r_lo .. r_hi).
  engine_tiles.hip tiles_write_png_locked MID, TABLES, CHUNK / PP: statistics written per tile by the stats kernel (histogram, Adler pairs,
    flag); the plan block carries a TileMeta for EVERY tile (skip = 1, out_word set) and token table + cleared header for every
    emitting one; the stream buffer is memset before the atomicOr emit.
  engine_display.hip display_hist_impl SRC, TABLES: image uploaded band by band ahead of its kernel; histogram memset.
  engine_display.hip display_apply_impl SRC, SRC / DST, TABLES: as above; the LUT uploaded whole.
  engine_tiles.hip s2sr_warp_bilinear_masked_u8 SRC, DST, TABLES, VALID: raster, node grid and mask uploaded whole, on the kernel's stream,
    before it is queued; the mask index is y / vs, x / vs of a clamped tap, so at most ceil(H / vs) - 1, ceil(W / vs) - 1; every output
    pixel is written.
  The raster passes run on the handle's stream alone, uploads included, so "before the kernel is queued" is the order of the calls:
  engine_bands.hip carry_band_impl SRC (the guide; from the kept copy: the slot that holds it), the other of SRC / DST (the carried plane),
    MID (the band), VALID (the mask), CONS (the inexact counter, then C and A).  None holds an index.  The counter is memset, band and
    mask are uploaded whole before the loop, a band of guide rows ahead of the coefficient launch whose windows end inside it
    (coeffs_end), and the rows of A and C an apply launch reads are written by the coefficient launches before it (apply_end trails by a row).
  engine_index.hip index_nd_impl SRC (image a, or the kept copy where it lies), the other of SRC / DST (the index plane, the RGBA behind
    it), MID (plane b), VALID (the mask, the zone grid behind it), TABLES (the LUT, the undefined counter, histogram, zonal sums).
    Index-like: the zone grid (a label picks the row of the zonal sums; one above Z counts as 0) and the LUT (entered by the value,
    never read as an index).  Counter, histogram and sums are memset in one piece; LUT, mask and zone grid are uploaded whole before
    the first band's kernel; each band of a and b ahead of the kernel that reads it.
  engine_index.hip index_render_impl SRC (the index raster), DST (the RGBA), TABLES (the LUT, uploaded whole before the first band); the
    raster goes up band by band ahead of its kernel.
  engine_zones.hip zones_impl DST (the labels), TABLES (xy, ring_start, feat_start, label, the tile bins' start table and feature lists,
    area).  All but xy and area are index-like: starts into the rings, the vertices and the lists, feature numbers, labels as rows of
    area.  The host checks them against one another (zone_check_tables, zone_check_bins) and copies each whole before the first launch;
    area is memset; the feature lists are left out only where they are empty, and then every bin's range is empty too.
  engine_fields.hip fields_impl SRC (the index raster), DST (the labels), MID and CHUNK (the two mask planes), PP (the union-find
    parents), CONS (the sizes, which become the ranks), TABLES (the chunk sums, found, the fields table).  Index-like: the parents
    (followed as pointers), the ranks (rows of the fields table; above Z: 0) and the chunk sums (the ranks' offsets).  The raster is
    uploaded whole before the first kernel; the first mask launch writes every pixel of its plane and reads none, every morphology pass
    writes its whole destination from a whole source; the local pass writes the parent and the size of EVERY pixel before the border
    and flatten passes follow one; the count pass writes every chunk's sum before the scan reads them, and the scan writes found; the
    fields table is memset before the apply pass writes a row.
  engine_mzones.hip mzones_impl SRC (the D feature planes), DST (the labels), MID and CHUNK (the two zone planes), TABLES (cnt, lo, hi,
    status, zone_of, centres, ranked, changed, and acc: the iterations' sums, then the table).  Index-like: the labels (a label picks
    the row of every table; one above Z counts as 0 in every kernel that reads it), status (says whether a field's centres are
    fetched), zone_of (the cluster's byte in the raster, which the table pass reads back as a cluster number after checking it
    against 1..k) and the centres (compared, never followed).  Labels and features go up band by band, each band ahead of the
    statistics launch that reads it, and every later pass runs behind the last band.  cnt, lo and hi are written whole by the clear
    kernel; the start kernel writes status for EVERY row (row 0 as absent) and all k D centres of every row before an accumulate or
    update launch reads one; changed is memset in front of every iteration, acc once in front of the first (the update kernel puts
    back the zeros it took) and again in front of the table pass; the rank kernel writes zone_of and ranked for every (row, cluster)
    before the assignment reads zone_of; the assignment writes every group of its plane, a mode pass its whole destination from a
    whole source, and the table pass reads the plane the last of them wrote.
  engine_fields_split.hip split_impl SRC (the index raster), DST (the distance plane, later the labels), MID and CHUNK (the mask planes
    and the interior), VALID (the vertical distances, later the cores), PP (the growth words), CONS (the parents; behind them one
    plane that holds sizes, then the components' largest distances, then the keys, then sizes again), TABLES (the chunk sums, found,
    the changed counter, two planes of tile marks, the fields table).  Index-like: the parents (followed as pointers, and rows of the
    largest distances), the growth words (the low half is the owner: fsplit_parent_kernel reads key[] there), the key plane (what
    becomes the parent), the tile marks (which tiles a round visits), the ranks and chunk sums as in fields_impl.  The mask, morphology,
    local, border, flatten, count, scan, apply and label launches are the stages it shares with fields_impl (engine_fields.hip
    fields_mask, fields_components, fields_numbering; the tables are laid out by fields_plan), in its order.  The edge kernel writes every pixel
    of the interior, the column pass every pixel of the vertical distances and the row pass every pixel of the distance plane before
    the cores read it; the plane behind the parents is memset in front of the maxima (0), the keys (all ones) and the sizes (0); the
    core kernel writes every pixel; the seed kernel writes EVERY word (unreached: all ones) behind the second components pass, and
    an owner is a root that pass wrote; every owner's key is written by the key kernel before the parent kernel reads it; a round
    memsets the marks it writes and reads the plane the round before wrote, the first round of either growth reads none; changed is
    memset per round; the fields table is memset before the first kernel.
  engine_debug.hip s2sr_debug_mfma_ceiling MID, TABLES and s2sr_debug_rdb_persistent MID, TABLES, CHUNK: measuring prototypes, not doors; their
    buffers hold operands whose values do not matter and flags they memset themselves; no index is read from them.
"""
import numpy as np
import pytest
import torch

import diag
import doors
from diag import baseline, keep, new_engine, same
from doors import DOORS, Inputs
from s2sr import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def poisoned():
    """(config, pattern) -> an engine created, and its weights loaded, under that pattern"""
    with diag.engines_under(native.poison_pattern, native.poison) as get:
        yield get


def judged(e, ident, what):
    same(keep(DOORS[ident][1](e, Inputs())), baseline(ident), f"{ident}, {what}")


@pytest.mark.parametrize("pattern", [1, 2])
@pytest.mark.parametrize("ident", list(DOORS))
def test_fresh_under_poison(poisoned, ident, pattern):
    e = poisoned(DOORS[ident][0], pattern)
    native.poison(pattern)
    judged(e, ident, f"on an engine created under pattern {pattern}")


@pytest.mark.parametrize("ident", list(DOORS))
def test_scratch_poisoned_before_every_sighting(poisoned, ident):
    e = poisoned(DOORS[ident][0], 1)
    sightings = 3                                                     # direct launches, the graph capture, a replay
    for k in range(sightings):
        native.poison(1 + k % 2)
        torch.cuda.synchronize()
        e.poison_scratch()
        judged(e, ident, f"sighting {k + 1} behind poison_scratch, pattern {1 + k % 2}")


@pytest.mark.parametrize("ident", list(DOORS))
def test_dirty_predecessor(poisoned, ident):
    e = poisoned(DOORS[ident][0], 2)
    native.poison(0)
    fn = DOORS[ident][1]
    fn(e, Inputs(dirty=True))
    allocs = e.debug_config()["ws_allocs"]
    judged(e, ident, "behind the same call on a saturated input")
    assert e.debug_config()["ws_allocs"] == allocs, "the workspace was reallocated between the dirty call and the judged one"


def test_the_saturated_inputs_keep_type_and_shape():
    """what (c) relies on: the dirty call has the judged call's geometry"""
    for shape in ((2, 3, 4, 3), (5, 7, 3)):
        for kind in ("u8", "u16", "i16", "green"):
            a, b = getattr(Inputs(), kind)(shape, 1), getattr(Inputs(True), kind)(shape, 1)
            assert a.shape == b.shape and a.dtype == b.dtype and (b == np.iinfo(b.dtype).max).all() and not (a == b).all()


# ---- calibration: engines of their own on both sides, a calibration changes the scales of the handle it runs on -------------------------
@pytest.mark.parametrize("pattern", [1, 2])
def test_calibrate_fp8_chooses_the_same_exponents(poisoned, pattern):
    t8 = Inputs().u8((2, 37, 53, 3), 5)
    native.poison(0)
    b = new_engine("x4_fp8")
    try:
        want = b.calibrate_fp8(t8), keep(b.forward_batch_u8(t8))
    finally:
        b.close()
    native.poison(pattern)
    e = new_engine("x4_fp8")
    try:
        assert e.calibrate_fp8(t8) == want[0]                          # (a) fresh
        same(keep(e.forward_batch_u8(t8)), want[1], "forward after the calibration")
        e.poison_scratch()                                             # (b) scratch
        assert e.calibrate_fp8(t8) == want[0]
        native.poison(0)                                               # (c) dirty: a saturated calibration set first
        e.calibrate_fp8(Inputs(True).u8((2, 37, 53, 3), 5))
        allocs = e.debug_config()["ws_allocs"]
        assert e.calibrate_fp8(t8) == want[0]
        assert e.debug_config()["ws_allocs"] == allocs
        same(keep(e.forward_batch_u8(t8)), want[1], "forward after the last calibration")
    finally:
        e.close()


# ---- the controls --------------------------------------------------------------------------------------------------------------------
def _holds_pattern(e, slot, nbytes, pattern):
    """every byte of the slot, in pieces of 1 MiB"""
    for off in range(0, nbytes, 1 << 20):
        n = min(1 << 20, nbytes - off)
        got = e.scratch_peek(slot, off, n)
        want = native.poison_byte(pattern, np.arange(off, off + n))
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            return f"slot {slot}, byte {off + i}: found 0x{int(got[i]):02x}, pattern {pattern} has 0x{int(want[i]):02x}"
    return ""


@pytest.mark.parametrize("pattern", [1, 2])
def test_poison_scratch_fills_every_slot_it_reports(poisoned, pattern):
    e = poisoned("x4_hp", 1)
    native.poison(pattern)
    img16 = Inputs().u16((39, 39, 3), 3)
    e.enhance_consistent_u16(img16, mode=2, valid=np.ones((39, 39), np.uint8), tile=16, pad=3)   # scratch 0 .. 4, 6, 7
    e.postprocess_u8(Inputs().green((20, 20, 3), 1), native.pp_wow())                               # ... and 5
    filled = e.poison_scratch()
    assert set(filled) == set(range(native.SCRATCH_SLOTS)) and all(v > 0 for v in filled.values()), filled
    for slot, nbytes in filled.items():
        assert not _holds_pattern(e, slot, nbytes, pattern)
    assert not _holds_pattern(e, -1, native.TRASH_BYTES, pattern)
    with pytest.raises(native.S2srError, match="invalid argument"):        # one byte past a slot's capacity
        e.scratch_peek(0, filled[0], 1)
    with pytest.raises(native.S2srError, match="invalid argument"):
        e.scratch_peek(native.SCRATCH_SLOTS, 0, 1)
    e.enhance_u8(Inputs().u8((20, 20, 3), 1))                              # the slot the call wrote no longer holds the pattern
    assert _holds_pattern(e, 0, filled[0], pattern)


@pytest.mark.parametrize("pattern", [1, 2])
def test_a_poisoned_engine_s_trash_page_holds_the_pattern_before_any_call(poisoned, pattern):
    poisoned("x4_hp", 1)
    native.poison(pattern)
    e = native.Engine(num_block=1, precision=native.PREC_F16_HP)
    try:
        assert not _holds_pattern(e, -1, native.TRASH_BYTES, pattern)
        with pytest.raises(native.S2srError, match="invalid argument"):    # nothing allocated yet
            e.scratch_peek(0, 0, 1)
        assert e.poison_scratch() == {}
    finally:
        e.close()


def test_doors_that_consume_what_the_last_call_left_refuse_after_poison_scratch(poisoned, tmp_path):
    e = poisoned("x4_hp", 1)
    native.poison(1)
    ident = np.arange(512, dtype=np.int32)
    level = doors.png_level(Inputs())
    e.tiles_base_u8(level, ident, ident, ident, ident, fetch=False)
    e.poison_scratch()
    with pytest.raises(native.S2srError, match="did not leave a tile level"):
        e.tiles_overview_u8((2, 2), 0, 0, 1, 1, on_device=True)
    e.tiles_base_u8(level, ident, ident, ident, ident, fetch=False)
    e.poison_scratch()
    with pytest.raises(native.S2srError, match="did not leave a tile level"):
        e.tiles_write_png(2, 2, [tmp_path / f"{k}.png" for k in range(4)])
    assert not list(tmp_path.iterdir())
    img16 = Inputs().u16((37, 53, 3), 37)
    lut = np.zeros((3, 65536), np.uint8)
    e.display_hist_u16(img16)
    e.poison_scratch()
    with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
        e.display_apply_u16(None, lut, shape=(37, 53))
    with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
        e.display_hist_u16(None, shape=(37, 53))
    img = doors._dev_u8(Inputs().green((20, 24, 3), 2))
    out = torch.zeros_like(img)
    st = torch.cuda.current_stream().cuda_stream
    e.pp_band_begin_dev(20, 24, native.pp_wow(), 0, st)
    e.pp_band_hist_dev(img.data_ptr(), 0, 20, st)
    e.pp_band_lut_dev(st)
    torch.cuda.synchronize()
    e.poison_scratch()
    with pytest.raises(native.S2srError, match="took its scratch"):
        e.pp_band_rows_dev(img.data_ptr(), 0, 20, out.data_ptr(), st)
    torch.cuda.synchronize()
    assert not out.any().item()
    judged(e, "x4_hp-short_ramps-enhance_u8", "after the refusals")


def test_with_the_mode_off_poison_scratch_is_refused_and_the_engine_works(poisoned):
    e = poisoned("x4_hp", 1)
    native.poison(0)
    e.enhance_u8(Inputs().u8((20, 20, 3), 1))
    before = e.scratch_peek(0, 0, 64).copy()
    with pytest.raises(native.S2srError, match="invalid argument"):
        e.poison_scratch()
    assert np.array_equal(e.scratch_peek(0, 0, 64), before)               # nothing was filled
    judged(e, "x4_hp-short_ramps-enhance_u8", "after a refused poison_scratch")
    for bad in (-1, 3):
        with pytest.raises(native.S2srError):
            native.poison(bad)
    assert native.poison_pattern() == 0
