"""The raster passes at their limits on the GPU ("Limits the tests reach"): the code paths that the kernels' own
comments describe and that the small, mid-range rasters of the pass modules do not reach.
  A  the numbering scan of csrc/fields.hip past its first turn of 256 chunks, for s2sr_fields_segment_i16 and s2sr_fields_split_i16
  B  the split's distance transform with a band of 256 rows that has a band on both sides, and a row of three segments
  C  the management zones' pending sums beyond the 65000 pixels a wave's int32 sums may hold, under grid caps 1 and 3 and without
  D  the whole range of uint16 in the consistency pass, the band pass and the nodata fill, +-32767 in the split's edge test, and
     +-16383 over a whole zone in the index pass's zonal sums
Every comparison is byte for byte against the numpy model of the pass; every test first asserts, by arithmetic on the model's outputs
(tests/limits.py), that its input takes the path it is there for.  tests/test_limits_cpu.py holds the same arithmetic and the models at
these sizes without a GPU."""
import numpy as np
import pytest

import bands_model as bm
import consistency_model as cm
import diag
import fields_model as fm
import fields_split_model as sm
import gpu_engines
import index_model as im
import limits
import mzones_model as mm
import nodata_model as nm
from diag import same_values as same
from fields_model import HI, LO
from s2sr import native

pytestmark = pytest.mark.gpu

HP = native.PREC_F16_HP
GRID_FAMILY = "display"
SPLIT_KEYS = ("labels", "fields", "dist2", "cores")
MZ_KEYS = ("zone", "table", "centres", "status")


@pytest.fixture(scope="module")
def bare():
    with gpu_engines.bare(precision=HP) as e:                    # no pass here needs weights
        yield e


# ---- A: the scan's carry --------------------------------------------------------------------------------------------------------------------
def check_fields(e, H, W, name, kw):
    want_labels, want_fields, want_found = fm.case(H, W, name, **kw)
    labels, fields, found = e.fields_segment_i16(fm.raster(H, W, name), LO, HI, **kw)
    what = f"{H} x {W} {name} {kw}"
    assert found == want_found, f"{what}: found {found} against {want_found}"
    same(np.array(labels), want_labels, f"{what}: labels")
    same(fields, want_fields, f"{what}: fields")
    assert int(fields[:, 0].sum()) == H * W
    return np.array(labels), found


def check_split(e, H, W, name, split, kw):
    want = sm.case(H, W, name, split=split, **kw)
    labels, fields, found, dist2, cores = e.fields_split_i16(sm.raster(H, W, name), LO, HI, split=split, want=("dist2", "cores"), **kw)
    got = {"labels": np.array(labels), "fields": fields, "dist2": dist2, "cores": cores}
    what = f"{H} x {W} {name} {split} {kw}"
    assert found == want["found"], f"{what}: found {found} against {want['found']}"
    for key in SPLIT_KEYS:
        same(got[key], want[key], f"{what}: {key}")
    assert int(fields[:, 0].sum()) == H * W
    return want


@pytest.mark.parametrize("H,W,name,kw,reach", limits.FIELDS, ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in limits.FIELDS])
def test_fields_are_numbered_across_the_scan_s_turns(bare, H, W, name, kw, reach):
    """513 x 512: 257 chunks, the second turn holds one; 730 x 730: 521 chunks, three turns.  The keys of the numbered fields lie
    in every turn, so every field behind the first 262144 pixels has the carry in its number, its row of the table and its box"""
    r = limits.scan_preconditions(limits.fields_keys(H, W, name, kw), H, W, reach)
    print(f"{H} x {W} {name}: {r}")
    labels, found = check_fields(bare, H, W, name, kw)
    if name == "checker":                                          # more fields than labels: found counts them all, and a number above Z is 0
        assert found == (H * W + 1) // 2 > 65535 and int(labels.max()) == 65535
        if (H, W) == (730, 730):
            assert found == 266450 and r["carry"][1] == 2 ** 17 and r["carry"][2] == 2 ** 18


@pytest.mark.parametrize("H,W,name,split,kw,reach", limits.SPLITS, ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in limits.SPLITS])
def test_split_fields_are_numbered_across_the_scan_s_turns(bare, H, W, name, split, kw, reach):
    """the split numbers its regions behind two component labellings of its own; at 730 wide the row pass of its distance has three
    segments.  (513 x 512: the second turn's one chunk is the last row and holds no region's key; the carry shows in `found`)"""
    r = limits.scan_preconditions(limits.split_keys(H, W, name, split, kw), H, W, reach)
    print(f"{H} x {W} {name} {split}: {r}")
    check_split(bare, H, W, name, split, kw)


@pytest.mark.parametrize("cap", [1, 3])
def test_the_numbering_under_capped_grids(bare, cap):
    """the scan is one workgroup whatever the cap; the count and apply kernels around it make their trips across the turn boundary:
    257 chunks on `cap` workgroups"""
    for entry, case in limits.CAPPED:
        H, W = case[0], case[1]
        assert fm.scan_reach([0], H, W)["chunks"] == 257 and -(-257 // cap) >= 86
        with diag.under(cap):
            if entry == "fields":
                check_fields(bare, H, W, case[2], case[3])
            else:
                check_split(bare, H, W, case[2], case[3], case[4])
            launches, trips = native.grid_cap_stats()[GRID_FAMILY]
        # the most trips are the per-pixel passes': 262656 pixels, 256 a workgroup
        assert launches >= 7 and trips == -(-(-(-H * W // 256)) // cap), (entry, launches, trips)
    native.grid_cap_stats(reset=True)


# ---- B: the distance beyond two bands ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", [False, True])
def test_the_distance_with_a_band_between_two_bands(bare, both):
    """780 x 600: four bands of the column pass, three segments of the row pass.  The middle band, rows 256..511, holds pixels at the
    cap and below it, and pixels whose nearest outside pixel lies in another band (the notch from the top; with `both` also a notch
    from the bottom, so that the way back from 255 rows below finds something)"""
    H, W = 780, 600
    idx = sm.notched(H, W, both)
    want = sm.split(idx, LO, HI, split={})
    r = sm.band_reach(fm.cleaned(idx, LO, HI), want["dist2"], 1)
    print(f"notched {H} x {W}, both {both}: {r}")
    assert -(-H // sm.BAND) == 4 and -(-W // sm.SEG) == 3 and r["rows"] == (256, 512)
    assert r["capped"] > 0 and r["uncapped"] > 0 and r["above"] > 0 and r["below"] > 0 and r["other"] > 0
    assert want["dist2"][256:512].max() == 255 * 255
    if both:
        assert want["dist2"][511, 297] == (H - 21 - 511) ** 2      # straight above the lower notch
    labels, fields, found, dist2, cores = bare.fields_split_i16(idx, LO, HI, split={}, want=("dist2", "cores"))
    got = {"labels": np.array(labels), "fields": fields, "dist2": dist2, "cores": cores}
    assert found == want["found"]
    for key in SPLIT_KEYS:
        same(got[key], want[key], f"notched {H} x {W}, both {both}: {key}")


# ---- C: the pending sums ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", limits.MZ_LAYOUTS)
@pytest.mark.parametrize("names,k", limits.MZ_PARAMS, ids=["D1-k2", "D1-k3", "D4-k8"])
def test_a_wave_s_pending_sums_are_let_go_in_time(bare, names, k, lay):
    """16384 x 64: one column of 512 tiles of +32767 above and -32767 below.  Under a cap of 1 or 3 workgroups a wave meets 131072 or
    87552 pixels of one label and one value, more than 65000, and their sum passes 2^31: a kernel that did not let its pending sums go
    would wrap.  "middle": a label change meets a run that has just flushed (the flush comes after 126 tiles, the change after 128;
    a run of 128 tiles holds 65536 pixels, whose sum 2^31 - 65536 still fits, so this layout judges the order of flush and label
    change, not the wrap).  Without a cap every workgroup has one tile and nothing flushes: the baseline, against the same model.
    The table's sums (1.7 x 10^10, 5.6 x 10^14) come from the TABLE form"""
    H, W = limits.MZ_SHAPE
    feats, labels, Z = mm.inputs(H, W, names, lay)
    want = mm.case(H, W, names, lay, k=k, **limits.MZ_KW)
    assert abs(int(want["table"][1, 0, 1])) >= 2 ** 31 and want["iterations"] == 2
    for cap in limits.MZ_CAPS + (None,):
        if cap is None:
            assert mm.pending_reach(H, W)["pixels"] < mm.PENDING
            got = bare.zones_kmeans_i16(feats, labels, Z, k=k, **limits.MZ_KW)
        else:
            print(f"cap {cap}: {limits.pending_preconditions(cap)}")
            with diag.under(cap):
                got = bare.zones_kmeans_i16(feats, labels, Z, k=k, **limits.MZ_KW)
        what = f"{names} on {lay}, k {k}, cap {cap}"
        assert got["iterations"] == want["iterations"], what
        for key in MZ_KEYS:
            same(np.array(got[key]), want[key], f"{what}: {key}")
    native.grid_cap_stats(reset=True)


# ---- D: full range and saturated inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 4])
def test_the_largest_residuals_of_the_consistency_pass(bare, S):
    """q all 0 against an input of all 65535 and the reverse: e = +-n 65535 in every block, the largest the definition allows; the
    image moves from one end of the range to the other and no block is inexact"""
    for H, W in ((17, 33), (5, 300)):
        for q, v in ((0, 65535), (65535, 0)):
            sr, img = np.full((S * H, S * W, 3), q, np.uint16), np.full((H, W, 3), v, np.uint16)
            for mode in (cm.EXACT, cm.SMOOTH):
                want, bad = cm.consistency(sr, img, S, mode, 0, 65535)
                assert (want == v).all() and not bad.any()
                for band_rows in (0, 3 * S + 1):
                    got, n = bare.consistency(sr, img, mode, 0, 65535, band_rows=band_rows)
                    same(got, want, f"{H} x {W} x{S} mode {mode}: {q} towards {v}, band_rows {band_rows}")
                    assert n.tolist() == bad.tolist()


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("H,W", limits.BANDS_SHAPES)
def test_saturated_guides_and_bands(bare, H, W, S):
    """guides of 0 and 65535 alone (blocks, a half plane, per-sample noise, all white) with the band equal to the guide's block mean,
    its inverse, all 65535 and three times as steep; weights (1, 1, 1) and (255, 255, 255), r 1 and 4, eps 1 and the largest the entry
    takes, masked and not: the guide sum reaches 765 * 65535, the gain one and three in Q16, and the clip path is taken"""
    top, inexact = limits.bands_preconditions(H, W, S)
    print(f"{H} x {W} x{S}: largest |A| {top} of {bm.GAIN_LIMIT}, most inexact blocks of a case {inexact}")
    v = bm.holes(H, W, seed=7)
    for case in limits.bands_cases(H, W, S):
        name, band, w, r, eps, masked = case
        want, bad = limits.bands_modelled(H, W, S, case)[:2]
        got, n = bare.carry_band_u16(bm.saturated_band(H, W, S, name, band), S, sr=bm.saturated_scene(H, W, S, name), weights=w, r=r, eps=eps,
                                     valid=v if masked else None, fill=limits.BANDS_FILL)
        what = f"{H} x {W} x{S} guide {name} band {band} weights {w} r {r} eps {eps} masked {masked}"
        same(got, want, what)
        assert n == bad, what


@pytest.mark.parametrize("H,W", limits.SATURATED_SHAPES)
def test_the_edge_test_on_a_raster_of_plus_and_minus_32767(bare, H, W):
    """cells of 1, 3 and 8 pixels of +32767 and -32767, every pixel in the mask: the box sums and the Sobel of them at the magnitudes
    the kernel's comments bound, against thresholds at both ends of their range"""
    for cell in limits.SATURATED_CELLS:
        idx = sm.saturated(H, W, cell)
        for split in sm.SATURATED_SPLITS:
            for conn in (4, 8):
                g2 = limits.saturated_preconditions(H, W, cell, split)
                want = sm.saturated_case(H, W, cell, split, conn=conn)
                labels, fields, found, dist2, cores = bare.fields_split_i16(idx, *sm.SATURATED, split=split, want=("dist2", "cores"), conn=conn)
                got = {"labels": np.array(labels), "fields": fields, "dist2": dist2, "cores": cores}
                what = f"{H} x {W} cell {cell} {split} conn {conn} (largest gx^2 + gy^2 {g2})"
                assert found == want["found"], what
                for key in SPLIT_KEYS:
                    same(got[key], want[key], f"{what}: {key}")


@pytest.mark.parametrize("sign", [1, -1])
def test_a_lane_s_zonal_sums_at_their_largest(bare, sign):
    """csrc/index.hip: a lane adds v and v^2 of its 8 pixels in 32 bits while the label stays.  The 0 / 65535 checkerboards of
    tests/test_gpu_index.py change label with every pixel, and its constant plane holds 5000; a constant +-16383 in one zone gives
    the largest sums a lane can hold, 8 * 16383^2 = 2147221512 = 2^31 - 262136, which a wave then adds 64 times in 64 bits, and one
    histogram bin that every wave adds to as one"""
    H, W, K = 255, 257, 16383
    assert 2 ** 31 - 2 ** 19 < 8 * K * K < 2 ** 31 < 64 * 8 * K * K and (H * W) % 8 != 0
    full, none = np.full((H, W), 65535, np.uint16), np.zeros((H, W), np.uint16)
    a, b = (full, none) if sign > 0 else (none, full)
    zones = np.full((H, W), 5, np.uint16)
    v, undefined = im.index(a, b, 0, 0, K)
    assert (v == sign * K).all() and undefined == 0
    for band_rows in (0, 100):
        got = bare.index_nd_u16(a, b, K=K, zones=zones, Z=7, band_rows=band_rows, want=("index", "hist", "zonal"))
        same(got["index"], v, f"constant {sign * K}, band_rows {band_rows}: index")
        same(got["hist"], im.hist(v, K), f"constant {sign * K}, band_rows {band_rows}: hist")
        same(got["zonal"], im.zonal(v, zones, 1, 7), f"constant {sign * K}, band_rows {band_rows}: zonal")
        assert got["zonal"][5].tolist() == [H * W, sign * K * H * W, K * K * H * W] and got["undefined"] == 0


def test_the_nodata_fill_moves_samples_with_bit_15_set(bare):
    """the fill copies samples; the uint16 images of tests/test_gpu_nodata.py stay below 13000"""
    for (H, W), R in (((37, 53), 5), ((70, 300), 32)):
        valid = nm.make_mask("holes", H, W)
        img = np.random.default_rng(7 + H).integers(0, 65536, (H, W, 3)).astype(np.uint16)
        img[valid == 0] = 0
        want = nm.fill(img, valid, R)
        moved = want[valid == 0]
        assert (moved >= 32768).sum() > 100 and (want != img).any()
        same(bare.fill_nodata(img, valid, R), want, f"{H} x {W} R {R}")
