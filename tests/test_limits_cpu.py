"""The raster passes at their limits without a GPU ("Limits the tests reach"): that the cases of tests/limits.py take
the paths tests/test_gpu_limits.py runs them for -- the numbering scan past its first turn, the split's distance beyond two bands, the
management zones' pending sums beyond 65000 pixels, saturated guides and index rasters -- as arithmetic on the models' outputs; and
the models themselves at those sizes against scipy and against integer arithmetic written out by hand."""
import numpy as np
import pytest

import bands_model as bm
import consistency_model as cm
import fields_model as fm
import fields_split_model as sm
import limits
import mzones_model as mm
from fields_model import HI, LO


# ---- A ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,name,kw,reach", limits.FIELDS, ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in limits.FIELDS])
def test_the_fields_cases_carry_numbers_across_the_scan_s_turns(H, W, name, kw, reach):
    labels, fields, found = fm.case(H, W, name, **kw)
    r = limits.scan_preconditions(limits.fields_keys(H, W, name, kw), H, W, reach)
    print(f"{H} x {W} {name}: found {found}, {r}")
    assert r["turns"] == (2 if (H, W) == (513, 512) else 3)
    assert int(fields[:, 0].sum()) == H * W
    if name == "checker":                                          # more fields than labels: found counts them all, the labels stop at Z
        keys = limits.fields_keys(H, W, name, kw)
        assert found == (H * W + 1) // 2 > 65535 and int(labels.max()) == 65535 and fields[65535, 1] == keys[65534]
        assert (labels.reshape(-1)[keys[:65535]] == np.arange(1, 65536)).all() and not labels.reshape(-1)[keys[65535:]].any()
        if (H, W) == (730, 730):
            assert found == 266450 and r["carry"][1] == 2 ** 17 and r["carry"][2] == 2 ** 18
    else:
        assert found == len(fields[1:found + 1, 1]) and (np.diff(fields[1:found + 1, 1]) > 0).all()


@pytest.mark.parametrize("H,W,name,split,kw,reach", limits.SPLITS, ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in limits.SPLITS])
def test_the_split_cases_carry_numbers_across_the_scan_s_turns(H, W, name, split, kw, reach):
    want = sm.case(H, W, name, split=split, **kw)
    r = limits.scan_preconditions(limits.split_keys(H, W, name, split, kw), H, W, reach)
    print(f"{H} x {W} {name} {split}: found {want['found']}, levels {want['levels']}, {r}")
    assert int(want["fields"][:, 0].sum()) == H * W
    if W == 730:
        assert -(-W // sm.SEG) == 3                                # the row pass of the distance: three segments


@pytest.mark.parametrize("conn", [4, 8])
def test_the_fields_model_against_scipy_at_257_chunks(conn):
    ndi = pytest.importorskip("scipy.ndimage")
    H, W = 513, 512
    for name in ("blobs", "noise"):
        idx = fm.raster(H, W, name)
        labels, fields, found = fm.case(H, W, name, conn=conn)
        ref, n = ndi.label(fm.mask(idx, LO, HI), structure=np.ones((3, 3), int) if conn == 8 else None)
        assert n == found
        # the same partition: every scipy component meets one label, every label one component, and the background is the background
        pairs = np.unique(np.stack([ref.ravel(), labels.ravel().astype(np.int64)]), axis=1)
        assert pairs.shape[1] == n + 1 and (pairs[:, 0] == 0).all() and (np.sort(pairs[1, 1:]) == np.arange(1, n + 1)).all()
        assert (np.sort(pairs[0, 1:]) == np.arange(1, n + 1)).all()
        assert (fields[1:n + 1, 0] == np.bincount(labels.ravel(), minlength=n + 1)[1:]).all()
        first = np.full(n + 1, H * W, np.int64)
        np.minimum.at(first, labels.ravel(), np.arange(H * W))
        assert (fields[1:n + 1, 1] == first[1:]).all()             # the key is the smallest linear index, and the numbers ascend with it


# ---- B ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", [False, True])
def test_the_notched_rectangle_s_middle_band_looks_into_both_neighbours(both):
    ndi = pytest.importorskip("scipy.ndimage")
    H, W = 780, 600
    idx = sm.notched(H, W, both)
    I = fm.cleaned(idx, LO, HI)
    D = sm.distance2(I)
    # scipy measures to the nearest zero; beyond the raster nothing counts in either
    d = ndi.distance_transform_edt(I)
    assert (D == np.minimum(np.rint(d * d).astype(np.int64), 255 * 255) * I).all()
    r = [sm.band_reach(I, D, b) for b in range(-(-H // sm.BAND))]
    print(f"notched {H} x {W}, both {both}: {r}")
    assert len(r) == 4 and r[1]["rows"] == (256, 512)
    assert r[1]["capped"] > 0 and r[1]["uncapped"] > 0 and r[1]["above"] > 0 and r[1]["below"] > 0 and r[1]["other"] > 0
    assert D[273].max() < 255 * 255 == D[274].max() and D[274, 274] == 255 * 255      # the cap from row 274 on: 26 columns and 254 rows from the notch's corner
    if both:
        assert D[H - 275].max() == 255 * 255 > D[H - 274].max() and r[2]["capped"] == 0 and r[2]["uncapped"] > 0
        assert D[511, 297] == (H - 21 - 511) ** 2                  # straight above the lower notch: the nearest outside pixel lies in the band below
    else:
        assert (D[300:, 290:312] == 255 * 255).all()                # down to the last row: beyond the raster nothing counts


# ---- C ------------------------------------------------------------------------------------------------------------------------------------
def test_the_halves_fill_a_wave_s_pending_sums_under_either_cap():
    for cap in limits.MZ_CAPS:
        r = limits.pending_preconditions(cap)
        print(f"cap {cap}: {r}")
    r = mm.pending_reach(*limits.MZ_SHAPE)
    assert r["grid"] == 512 and r["run_tiles"] == 1 and r["pixels"] < mm.PENDING      # without a cap nothing flushes: the baseline
    H, W = limits.MZ_SHAPE
    for name in mm.HALVES:
        a = mm.raster(H, W, name)
        assert a.dtype == np.int16 and not (a == mm.NODATA).any() and len(np.unique(a)) == 2 and (a[:H // 2] == a[0, 0]).all() and (a[H // 2:] == a[-1, -1]).all()
    assert mm.raster(H, W, "halves")[0, 0] == 32767 and mm.raster(H, W, "halves")[-1, 0] == -32767
    assert (mm.raster(H, W, "-halves") == -mm.raster(H, W, "halves").astype(np.int64)).all()
    assert (mm.raster(H, W, "halves/2") == mm.raster(H, W, "halves").astype(np.int64) // 2).all()
    labels, Z = mm.layout(H, W, "middle")
    assert Z == 2 and (labels[:H // 4] == 1).all() and (labels[H // 4:3 * H // 4] == 2).all() and (labels[3 * H // 4:] == 1).all()
    late, Z = mm.layout(H, W, "late")
    assert Z == 2 and (late[:H // 4 + 96] == 1).all() and (late[H // 4 + 96:3 * H // 4] == 2).all() and (late[3 * H // 4:] == 1).all()
    # the first run of one label and one value under a cap of 1: 128 tiles fit an int32 sum by 65536, 131 do not; the flush comes at 126
    assert 128 * 512 * 32767 == 2 ** 31 - 65536 and 131 * 512 * 32767 >= 2 ** 31 and 126 * 512 > mm.PENDING - 512 >= 125 * 512


@pytest.mark.parametrize("lay", limits.MZ_LAYOUTS)
@pytest.mark.parametrize("names,k", limits.MZ_PARAMS, ids=["D1-k2", "D1-k3", "D4-k8"])
def test_the_model_on_the_halves_against_the_arithmetic_by_hand(names, k, lay):
    H, W = limits.MZ_SHAPE
    want = mm.case(H, W, names, lay, k=k, **limits.MZ_KW)
    Z, by_hand = limits.halves_by_hand(names, lay, k)
    assert want["iterations"] == 2 and want["status"].tolist() == [0] + [2] * Z
    upper = np.arange(H)[:, None] < H // 2
    assert (want["zone"] == np.where(upper, k, 1)).all()
    for l, ((n_low, n_high), (low, high), (row_low, row_high)) in enumerate(by_hand, start=1):
        assert want["centres"][l, 0].tolist() == low and want["centres"][l, k - 1].tolist() == high
        assert want["table"][l, 0].tolist() == row_low and want["table"][l, k - 1].tolist() == row_high
        assert not want["table"][l, 1:k - 1].any()
        assert n_low * 32767 >= 2 ** 31 and row_low[1] == -n_low * 32767 and row_low[2] == n_low * 32767 ** 2 and row_high[1] == n_high * 32767
    assert sum(a + b for (a, b), _, _ in by_hand) == H * W
    if lay == "one":
        assert by_hand[0][2][1][1:3] == [17179344896, 562915594207232]               # 1.7 x 10^10 and 5.6 x 10^14


# ---- D ------------------------------------------------------------------------------------------------------------------------------------
def test_the_full_range_inputs_of_the_consistency_pass_have_bit_15_set():
    for S in (2, 4):
        for kind, make in (("clip_free", cm.clip_free_input), ("saturating", cm.saturating_input)):
            sr, img = make(40, 75, S, dtype="uint16", lo=0, hi=65535)
            assert sr.dtype == img.dtype == np.uint16
            assert 0.4 < (sr >= 32768).mean() < 0.6 and 0.4 < (img >= 32768).mean() < 0.6, (S, kind)
    # the largest residuals the definition allows: the image moves from one end of the range to the other, and every block is exact
    for S in (2, 4):
        for H, W in ((17, 33), (5, 300)):
            for q, v in ((0, 65535), (65535, 0)):
                sr, img = np.full((S * H, S * W, 3), q, np.uint16), np.full((H, W, 3), v, np.uint16)
                for mode in (cm.EXACT, cm.SMOOTH):
                    out, bad = cm.consistency(sr, img, S, mode, 0, 65535)
                    assert (out == v).all() and not bad.any()


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("H,W", limits.BANDS_SHAPES)
def test_the_saturated_guides_meet_the_bounds_of_the_band_pass(H, W, S):
    top, inexact = limits.bands_preconditions(H, W, S)
    clipped = sum(limits.bands_modelled(H, W, S, c)[3] for c in limits.bands_cases(H, W, S))
    print(f"{H} x {W} x{S}: largest |A| {top} of {bm.GAIN_LIMIT}, most inexact blocks {inexact}, gains on the limit {clipped}")
    assert len(limits.bands_cases(H, W, S)) == 4 * 4 * 2 * 2 * 2 * 2
    assert top <= bm.GAIN_LIMIT
    for name in bm.SATURATED:
        q = bm.saturated_scene(H, W, S, name)
        assert set(np.unique(q).tolist()) <= {0, 65535} and q.max() == 65535
        for band in bm.SATURATED_BANDS:
            b = bm.saturated_band(H, W, S, name, band)
            assert b.dtype == np.uint16 and b.shape == (H, W)
    assert (bm.saturated_band(H, W, S, "blocks", "mean") == np.where((np.add.outer(np.arange(H), np.arange(W))) % 2 == 0, 65535, 0)).all()


@pytest.mark.parametrize("H,W", limits.SATURATED_SHAPES)
def test_the_saturated_index_rasters_meet_the_bounds_of_the_edge_test(H, W):
    for cell in limits.SATURATED_CELLS:
        for split in sm.SATURATED_SPLITS:
            g2 = limits.saturated_preconditions(H, W, cell, split)
            want = sm.saturated_case(H, W, cell, split)
            print(f"{H} x {W} cell {cell} {split}: largest gx^2 + gy^2 {g2} against {(8 * (2 * split['edge_r'] + 1) ** 2 * split['edge']) ** 2}, {want['found']} fields")
            assert int(want["fields"][:, 0].sum()) == H * W and want["found"] >= 1
            assert int(want["fields"][0, 0]) == 0 or split["edge"] < 32767           # every pixel is in the mask; only edge pixels that nothing reaches stay 0
