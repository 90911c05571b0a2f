"""The bands of a chunked whole-image call on the host: csrc/band_plan.h plan_bands through s2sr_debug_plan_bands.  Every door of
the enhance pipeline (engine_aoi.hip) takes from it which output rows a chunk of window rows makes final -- the rows the chunk loop
pastes and copies out, and for the seam-blended paste the rows whose two window rows the chunk's buffer (with the one carried in
front) must hold."""
from itertools import combinations

import numpy as np
import pytest

from s2sr import native

# PH, PW of the planned image, tile, pad, scale, output rows (scale 2: the 37 x 45 image, planned on its even-padded size and cropped)
SHAPES = [
    (53, 200, 16, 3, 4, 212),        # the three-chunk image of the GPU tests
    (100, 90, 16, 2, 4, 400),
    (130, 37, 16, 2, 4, 520),
    (39, 39, 16, 3, 4, 156),         # a shortened ramp
    (513, 513, 256, 10, 4, 2052),    # window rows 1 and 2 coincide
    (38, 46, 16, 2, 2, 74),
]


def cuts(ny):
    """every way of cutting ny window rows into 1 to 3 chunks"""
    for n in (1, 2, 3):
        for inner in combinations(range(1, ny), n - 1):
            yield [0, *inner, ny]


def planned_cuts(nx, ny, wh, ww, scale):
    """chunkings as the engine plans them (plan_chunk_rows: whole row units that fill a mosaic, sized by s2sr_debug_plan_chunks)"""
    u = 2 if scale == 2 else 1
    kx, ky = native.pick_mosaic(nx * ny, wh // u, ww // u)
    per = kx * ky
    r_min = -(-per // nx)
    units = -(-ny // r_min)
    pimg = max(1, native.mosaic_patches(per, wh // u, ww // u)[0])
    for u_max in (1, 2, 3, 16):
        for ncu in (4, 256):
            sizes = native.plan_chunks(units, u_max, r_min * nx, per, pimg, ncu)
            r0 = [0]
            for n in sizes[:-1]:
                r0.append(r0[-1] + n * r_min)
            yield r0 + [ny]


def model_bands(chunk_r0, ny, OH, last_row, off=0):
    """the rule, restated: a row is final once the last window row it reads lies in front of the chunk's end (off != 0: wrong on purpose)"""
    out, y = [], 0
    for k in range(len(chunk_r0) - 1):
        r1, yb = chunk_r0[k + 1], y
        if r1 >= ny:
            y = OH
        while y < OH and last_row[y] < r1 + off:
            y += 1
        out.append((yb, y))
    return np.array(out, np.int32)


def violations(bands, chunk_r0, OH, last_row, rows=None):
    bad = []
    n = len(chunk_r0) - 1
    if not (bands.shape == (n, 2) and bands[0, 0] == 0 and bands[-1, 1] == OH and (bands[:, 0] <= bands[:, 1]).all()
            and (bands[1:, 0] == bands[:-1, 1]).all()):
        return ["the bands do not partition [0, OH) in order"]
    for k, (yb, ye) in enumerate(bands.tolist()):
        r0, r1 = chunk_r0[k], chunk_r0[k + 1]
        if (last_row[yb:ye] >= r1).any():
            bad.append(f"band {k} holds a row whose last window row is not done")
        if k < n - 1 and ye < OH and last_row[ye] < r1:
            bad.append(f"band {k} is not maximal")
        if rows is not None:        # blend_check_band's condition: the buffer holds window rows [r0 - 1, r1), from the second chunk on
            first = r0 - (1 if k > 0 else 0)
            ab = rows[yb:ye][:, [0, 2]]
            if ab.size and (ab.min() < first or ab.max() >= r1):
                bad.append(f"band {k} reads a window row its chunk does not hold")
    return bad


def tables(PH, PW, tile, pad, scale):
    nx, ny, wh, ww, _, rm, _ = native.plan_windows(PH, PW, tile, pad, scale)
    rows, _ = native.plan_blend(PH, PW, tile, pad, scale)
    return nx, ny, wh, ww, rm[:, 0].copy(), rows


@pytest.mark.parametrize("PH,PW,tile,pad,scale,OH", SHAPES)
def test_bands_partition_the_image_are_final_maximal_and_inside_their_chunk(PH, PW, tile, pad, scale, OH):
    nx, ny, wh, ww, owner, rows = tables(PH, PW, tile, pad, scale)
    assert ny >= 2 and (np.diff(owner) >= 0).all() and (np.diff(rows[:, 2]) >= 0).all()
    seen = 0
    for chunk_r0 in list(cuts(ny)) + list(planned_cuts(nx, ny, wh, ww, scale)):
        assert chunk_r0[0] == 0 and chunk_r0[-1] == ny and all(a < b for a, b in zip(chunk_r0, chunk_r0[1:])), chunk_r0
        for last_row, tab in ((owner, None), (rows[:, 2], rows)):      # the overwrite map, the blend rows table
            bands = native.plan_bands(chunk_r0, ny, OH, last_row)
            assert np.array_equal(bands, model_bands(chunk_r0, ny, OH, last_row)), chunk_r0
            assert violations(bands, chunk_r0, OH, last_row, tab) == [], chunk_r0
        seen += 1
    assert seen >= 1 + (ny - 1) + (ny - 1) * (ny - 2) // 2 + 8


def test_the_untiled_image_is_one_band():
    nx, ny, wh, ww, _, rm, _ = native.plan_windows(28, 36, 16, 2, 4, tiled=False)
    rows, _ = native.plan_blend(28, 36, 16, 2, 4, tiled=False)
    assert (nx, ny) == (1, 1)
    for last_row in (rm[:, 0], rows[:, 2]):
        assert native.plan_bands([0, 1], 1, 112, last_row).tolist() == [[0, 112]]


def test_a_wrong_rule_fails_these_properties():
    """the control: the rule off by one in the chunk's end, either way, is caught on the shapes above"""
    caught = {+1: set(), -1: set()}
    for PH, PW, tile, pad, scale, OH in SHAPES:
        nx, ny, wh, ww, owner, rows = tables(PH, PW, tile, pad, scale)
        for chunk_r0 in cuts(ny):
            for last_row, tab in ((owner, None), (rows[:, 2], rows)):
                for off in caught:
                    caught[off].update(v.split(" ", 2)[2] for v in violations(model_bands(chunk_r0, ny, OH, last_row, off), chunk_r0, OH, last_row, tab))
    assert {"holds a row whose last window row is not done", "reads a window row its chunk does not hold"} <= caught[+1], caught
    assert "is not maximal" in caught[-1], caught


def test_plan_bands_refuses_chunks_that_do_not_cover_the_window_rows():
    last_row = np.zeros(8, np.int32)
    for bad in ([1, 2], [0, 1], [0, 2, 1, 2], [0, 0, 2]):
        with pytest.raises(native.S2srError):
            native.plan_bands(bad, 2, 8, last_row)
