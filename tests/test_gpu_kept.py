"""The hand-over between calls, pinned: what a call keeps on the device for the next call on the handle, and who may take it.

A pyramid call keeps its raster or its level, the 16-bit enhance doors and the display calls keep a uint16 image (csrc/scratch.h:
one record of kind, slot and size), and a consumer called with a NULL source takes it -- or refuses, because the record is of
another kind or size, or because a call in between asked for scratch and so voided it.  The per-family tests (display behind the
16-bit doors, levels behind levels, the refusals after poison_scratch) each see a corner; this is the cross table, on one 1-block
engine at the smallest shapes: every consumer behind every producer, asked for a matching and for a non-matching size,
  direct            the consumer returns the bytes it returns when fed the host copy of the producer's output exactly when kind
                    and size match, and refuses with its "did not leave ..." message otherwise;
  scratch_taker     one call in between that takes scratch (postprocess_u8 at 5 x 9): every consumer refuses;
  refused_calls     calls in between that are refused before any scratch request: nothing changes;
  synchronize, graph_stats   in between: nothing changes.
Each cell is printed before it is judged (pytest -s shows the table)."""
import tempfile
from pathlib import Path

import numpy as np
import pytest

import gpu_engines
from diag import keep, same
from doors import CONFIGS
from s2sr import native, tiles

pytestmark = pytest.mark.gpu

_rng = np.random.default_rng(20261019)
RGB = _rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
RASTER = _rng.integers(0, 256, (4, 4, 4), dtype=np.uint8)
OPAQUE = np.concatenate([RASTER[..., :3], np.full((4, 4, 1), 255, np.uint8)], -1)
CHILD = _rng.integers(0, 256, (1, 1, 256, 256, 4), dtype=np.uint8)
IMG16 = _rng.integers(0, 65536, (8, 8, 3), dtype=np.uint16)
LUT = _rng.integers(0, 256, (3, 65536), dtype=np.uint8)
GRID = np.stack(np.meshgrid(np.arange(2) * 4.0, np.arange(2) * 4.0), -1).astype(np.float32)   # nodes 4 apart: the identity warp

RASTER_MSG, LEVEL_MSG, U16_MSG = "did not leave a warped raster", "did not leave a tile level", "did not leave a uint16 image"


def _footprint(n_src):
    return (np.arange(256) * n_src // 256).astype(np.int32)


def _taps(n_src):
    return tiles.plan_resample_axis(256, 0.0, float(n_src), n_src, "bilinear")


def _nearest(n_src):
    """one tap of weight 1 (22 fractional bits) per sample: the sample is the source pixel itself"""
    return _footprint(n_src), np.ones(256, np.int32), np.full((256, 1), 1 << 22, np.int32)


# ---- producers: (kind, size, e -> the host copy of what stays on the device) -------------------------------------------------------
PRODUCERS = {
    "warp_bilinear_u8": ("raster", (4, 4), lambda e: e.warp_bilinear_u8(RGB, GRID, 4, 4, 4)),
    "tiles_base_u8": ("level", (1, 1), lambda e: e.tiles_base_u8(RASTER, _footprint(4), _footprint(4), _footprint(4), _footprint(4))),
    "tiles_overview_u8": ("level", (1, 1), lambda e: e.tiles_overview_u8(CHILD, 0, 0, 1, 1)),
    # (nearest taps of an opaque raster: alpha 0 or 255 as the averaged levels have it, so _write_png's way up is exact for it too)
    "tiles_resample_u8": ("level", (1, 1), lambda e: e.tiles_resample_u8(OPAQUE, _nearest(4), _nearest(4), 1, 1)),
    "enhance_u16": ("u16", (32, 32), lambda e: e.enhance_u16(IMG16)),
    "display_hist_u16": ("u16", (8, 8), lambda e: (e.display_hist_u16(IMG16), IMG16)[1]),          # (a display call keeps its upload)
    "display_apply_u16": ("u16", (8, 8), lambda e: (e.display_apply_u16(IMG16, LUT), IMG16)[1]),
}


# ---- consumers: (e, src, size) -> bytes; src None: what the call before kept -------------------------------------------------------
def _base(e, src, size):
    H, W = size
    return e.tiles_base_u8(size if src is None else src, _footprint(W), _footprint(W), _footprint(H), _footprint(H), on_device=src is None)


def _resample_raster(e, src, size):
    H, W = size
    return e.tiles_resample_u8(size if src is None else src, _taps(W), _taps(H), 1, 1, on_device=src is None)


def _overview(e, src, size):
    return e.tiles_overview_u8(size if src is None else src, 0, 0, 1, 1, on_device=src is None)


def _resample_level(e, src, size):
    cny, cnx = size
    return e.tiles_resample_u8(src, _taps(cnx * 256), _taps(cny * 256), 1, 1, level_shape=size, on_device=src is None)


def _write_png(e, src, size):
    cny, cnx = size
    if src is not None:                                   # the writer has no host door: the level goes up through an identity base
        assert np.isin(src[..., 3], (0, 255)).all() and not src[src[..., 3] == 0].any(), "an identity base would not reproduce this level"
        raster = np.ascontiguousarray(src.transpose(0, 2, 1, 3, 4).reshape(cny * 256, cnx * 256, 4))
        iy, ix = np.arange(cny * 256, dtype=np.int32), np.arange(cnx * 256, dtype=np.int32)
        e.tiles_base_u8(raster, ix, ix, iy, iy, fetch=False)
    with tempfile.TemporaryDirectory() as d:
        paths = [Path(d) / f"{k}.png" for k in range(cny * cnx)]
        wrote = e.tiles_write_png(cnx, cny, paths, skip_transparent=False).copy()
        return (wrote, *[np.frombuffer(p.read_bytes(), np.uint8) if p.exists() else np.zeros(0, np.uint8) for p in paths])


CONSUMERS = {   # name -> (kind, the sizes asked for: one that some producer leaves, one that none does (display: both are left), the call, its refusal)
    "tiles_base_u8": ("raster", ((4, 4), (4, 5)), _base, RASTER_MSG),
    "tiles_resample_u8-raster": ("raster", ((4, 4), (5, 4)), _resample_raster, RASTER_MSG),
    "tiles_overview_u8": ("level", ((1, 1), (1, 2)), _overview, LEVEL_MSG),
    "tiles_resample_u8-level": ("level", ((1, 1), (2, 1)), _resample_level, LEVEL_MSG),
    "tiles_write_png": ("level", ((1, 1), (1, 2)), _write_png, LEVEL_MSG),
    "display_hist_u16": ("u16", ((32, 32), (8, 8)), lambda e, src, size: e.display_hist_u16(src, shape=size), U16_MSG),
    "display_apply_u16": ("u16", ((32, 32), (8, 8)), lambda e, src, size: e.display_apply_u16(src, LUT, shape=size), U16_MSG),
}


def _scratch_taker(e):
    e.postprocess_u8(np.full((5, 9, 3), 90, np.uint8), native.pp_wow())


def _refused_calls(e):
    with pytest.raises(native.S2srError, match="power of two"):
        e.warp_bilinear_u8(RGB, GRID, 3, 4, 4)
    with pytest.raises(native.S2srError, match="nodata must be"):
        e.display_hist_u16(IMG16, nodata=70000)


BETWEEN = {"direct": lambda e: None, "scratch_taker": _scratch_taker, "refused_calls": _refused_calls,
           "synchronize": lambda e: e.synchronize(), "graph_stats": lambda e: e.graph_stats()}

_WANT = {}


def _want(e, pname, cname):
    """the consumer on the host copy of the producer's output: computed once, shared by every state"""
    if (pname, cname) not in _WANT:
        _, size, produce = PRODUCERS[pname]
        _WANT[pname, cname] = keep(CONSUMERS[cname][2](e, np.array(produce(e)), size))
    return _WANT[pname, cname]


@pytest.mark.parametrize("between", list(BETWEEN))
@pytest.mark.parametrize("pname", list(PRODUCERS))
def test_every_consumer_behind_this_producer(pname, between):
    e = gpu_engines.default(*CONFIGS["x4_hp"])
    pkind, psize, produce = PRODUCERS[pname]
    for cname, (ckind, sizes, call, refusal) in CONSUMERS.items():
        for size in sizes:
            takes = between != "scratch_taker" and (pkind, psize) == (ckind, size)
            want = _want(e, pname, cname) if takes else None
            produce(e)
            BETWEEN[between](e)
            print(f"{between:14s} {pname:18s} -> {cname:24s} {size}: {'bytes' if takes else 'refused'}")
            if takes:
                same(keep(call(e, None, size)), want, f"{cname} {size} behind {pname}, {between}")
            else:
                with pytest.raises(native.S2srError, match=refusal):
                    call(e, None, size)


def test_a_consumer_that_keeps_its_input_hands_it_on():
    """tiles_write_png and the display calls leave what they read: a second consumer finds it, and a third"""
    e = gpu_engines.default(*CONFIGS["x4_hp"])
    want_png, want_over = _want(e, "tiles_base_u8", "tiles_write_png"), _want(e, "tiles_base_u8", "tiles_overview_u8")
    PRODUCERS["tiles_base_u8"][2](e)
    same(keep(_write_png(e, None, (1, 1))), want_png, "the first write")
    same(keep(_write_png(e, None, (1, 1))), want_png, "the second write")
    same(keep(_overview(e, None, (1, 1))), want_over, "the overview behind both")
    want_hist, want_apply = _want(e, "enhance_u16", "display_hist_u16"), _want(e, "enhance_u16", "display_apply_u16")
    PRODUCERS["enhance_u16"][2](e)
    same(keep(e.display_hist_u16(None, shape=(32, 32))), want_hist, "hist behind enhance_u16")
    same(keep(e.display_apply_u16(None, LUT, shape=(32, 32))), want_apply, "apply behind hist")
    same(keep(e.display_hist_u16(None, shape=(32, 32))), want_hist, "hist behind apply")
