"""The doors of the library as a table: id -> (engine config, fn(engine, inputs) -> arrays).  One entry is ONE call (or the short
sequence that makes a door, such as base level + overview), on the smallest configs and shapes that take each route.  Four
modules judge every entry, each under one diagnostic mode of the library: tests/test_gpu_redzones.py (no store outside a buffer),
tests/test_gpu_poison.py (no load of bytes nobody wrote), tests/test_gpu_stall.py (no dependence on which stream runs first) and
section (c) of tests/test_gpu_gridcap.py (no dependence on the number of workgroups); tests/diag.py holds what they share.
`inputs` lets a judge ask for the same call, with the same geometry, on a saturated input (Inputs(dirty=True): all 255 / 65535 /
32767 / 1.0).  Importing this file builds the table and touches no device: inputs and models are made inside the door functions, once
per case (tests/test_doors_cpu.py; tests/golden/doors_idents.txt lists the identifiers).

The raster passes (carried band, index, zones, fields, management zones, the split, masked warp) are rows like any other.  The four
judges compare with diag.baseline, not with a model, so MODELS holds for each of these rows what the numpy model of its pass says,
and the pass's own module (tests/test_gpu_bands.py, _index, _zones, _fields, _mzones, _fields_split, _tiles_nodata) holds the baseline
to it: every mode reaches the model through the baseline, as it does for the older doors through the parity modules.

Every raster a job hands to the zone, field, management-zone and split passes lives on the SR grid, 4 x (or 2 x) the input's width: W
% 8 == 0 from an even input width, W % 8 == 4 (W % 4 == 2 at x2) from an odd one.  The kernels of these four passes pick their
load and store widths by exactly that, so WIDTHS names the shapes that the pass modules add to their own, and each pass has rows at 65
x 128 and 37 x 180 here: the red zones then watch the 16- and 8-byte stores at a ragged tile, poison the wide loads.

x2plus refuses odd tile sizes (pixel_unshuffle by 2), so its net doors run the listed shapes as the trunk grid: tiles of
2 th x 2 tw.  The 16-bit doors exist on the x4 RRDB nets only."""
import tempfile
from pathlib import Path

import numpy as np
import torch

import bands_model as bm
import display_model as dm
import fields_model as fm
import fields_split_model as sm
import index_model as im
import mzones_model as mm
import resample_model as rm
import warp_masked_model as wm
import zones_model as zm
from s2sr import geo, native, tiles

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
FILL = 0x5A                      # what a caller-owned output buffer holds before the call, on both sides of a comparison
# the widths of the SR grid: one vector group; a tile line between vector groups and a ragged bottom tile; three tile columns and a
# ragged one of a single group; W % 8 == 4 twice (4 x 45 and 4 x 17: groups of 8 and a tail of 4); W % 4 == 2, the x2 grid of 39
WIDTHS = [(5, 8), (65, 128), (33, 200), (37, 180), (1, 68), (39, 78)]


class Inputs:
    """Seeded random inputs, or (dirty) the saturated ones of the same shape and type."""

    def __init__(self, dirty=False):
        self.dirty = dirty

    def u8(self, shape, seed):
        if self.dirty:
            return np.full(shape, 255, np.uint8)
        return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)

    def u16(self, shape, seed):
        if self.dirty:
            return np.full(shape, 65535, np.uint16)
        return np.random.default_rng(seed).integers(0, 65536, shape).astype(np.uint16)

    def i16(self, shape, seed):
        if self.dirty:
            return np.full(shape, 32767, np.int16)
        return np.random.default_rng(seed).integers(-32768, 32768, shape).astype(np.int16)

    def like(self, a):
        """`a` itself (a case's pixel data), or the saturated array of its type and shape"""
        return getattr(self, {"uint8": "u8", "uint16": "u16", "int16": "i16"}[a.dtype.name])(a.shape, 0) if self.dirty else a

    def green(self, shape, seed):
        """the post-process tests' image: green at least 90, so the vegetation stage has pixels to work on"""
        img = self.u8(shape, seed)
        img[..., 1] = np.maximum(img[..., 1], 90)
        return img


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(shape, dtype=torch.uint8):
    return torch.full(shape, FILL, dtype=dtype, device="cuda")


def _back(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


DOORS = {}


def door(ident, config):
    def add(fn):
        assert ident not in DOORS, ident
        DOORS[ident] = (config, fn)
        return fn
    return add


# ---- net doors -----------------------------------------------------------------------------------------------------------------------
def _part(e, tiles_u8, job, scale):
    B, th, tw, _ = tiles_u8.shape
    x = _dev_u8(tiles_u8)
    y = torch.zeros((B, scale * th, scale * tw, 3), dtype=torch.uint8, device="cuda")
    e.forward_part_u8_dev(x.data_ptr(), B, th, tw, job, y.data_ptr(), _stream())
    return _back(y)


def _fwd_u8_dev(e, t8, S):
    B, th, tw, _ = t8.shape
    x, y = _dev_u8(t8), _out((B, S * th, S * tw, 3))
    e.forward_batch_u8_dev(x.data_ptr(), B, th, tw, y.data_ptr(), _stream())
    return _back(y)


def _fwd_u16_dev(e, t16, lo, hi):
    B, th, tw, _ = t16.shape
    x = torch.from_numpy(t16.view(np.int16).copy()).cuda()
    y = torch.full((B, 4 * th, 4 * tw, 3), 0x5A5A, dtype=torch.int16, device="cuda")
    e.forward_batch_u16_dev(x.data_ptr(), B, th, tw, y.data_ptr(), lo, hi, stream=_stream())
    return _back(y).view(np.uint16)


def _net_doors():
    for name, (_, _, S, _) in CONFIGS.items():
        for shape, (B, th, tw, job) in NET_SHAPES.items():
            if S == 2:
                th, tw = 2 * th, 2 * tw                  # the listed shape is the trunk grid (x2plus refuses odd tiles)
            dims, seed = (B, th, tw, 3), B * 10000 + th * 100 + tw
            pre = f"{name}-{shape}"
            if job:                                      # the dead-window job: B windows of a mosaic planned for `job`
                door(f"{pre}-forward_part_u8_dev", name)(lambda e, X, d=dims, s=seed, j=job, S=S: _part(e, X.u8(d, s), j, S))
                continue
            door(f"{pre}-forward_batch_u8", name)(lambda e, X, d=dims, s=seed: e.forward_batch_u8(X.u8(d, s)))
            door(f"{pre}-forward_f32", name)(lambda e, X, d=dims, s=seed: e.forward_f32(
                np.ascontiguousarray(X.u8(d, s).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))))
            door(f"{pre}-forward_batch_u8_dev", name)(lambda e, X, d=dims, s=seed, S=S: _fwd_u8_dev(e, X.u8(d, s), S))
            if not name.startswith("x4"):                # the 16-bit doors exist on the x4 RRDB nets only
                continue
            for lo, hi in (FULL, SUB):
                r = f"{lo}_{hi}"
                door(f"{pre}-forward_batch_u16-{r}", name)(lambda e, X, d=dims, s=seed, lo=lo, hi=hi: e.forward_batch_u16(X.u16(d, s + 1), lo, hi))
                door(f"{pre}-forward_batch_u16_f32-{r}", name)(
                    lambda e, X, d=dims, s=seed, lo=lo, hi=hi: e.forward_batch_u16(X.u16(d, s + 1), lo, hi, want_f32=True))
            door(f"{pre}-forward_batch_u16_dev", name)(lambda e, X, d=dims, s=seed: _fwd_u16_dev(e, X.u16(d, s + 1), *SUB))


# ---- whole-image doors ---------------------------------------------------------------------------------------------------------------
def _valid(H, W, seed):
    """a mask with holes of every size up to a band of rows; the same for the saturated input (geometry, not content)"""
    rng = np.random.default_rng(seed)
    v = (rng.random((H, W)) > 0.2).astype(np.uint8)
    v[H // 3:H // 3 + 3] = 0
    v[0, 0] = 1
    return v


def _u8_image_doors(name, case, H, W, tile, pad, full):
    g = dict(tile=tile, pad=pad)
    sh, seed, pre = (H, W, 3), 7 + 1000 * H + W, f"{name}-{case}"
    door(f"{pre}-enhance_u8", name)(lambda e, X: e.enhance_u8(X.u8(sh, seed), **g))
    door(f"{pre}-enhance_f32", name)(lambda e, X: e.enhance_f32(X.u8(sh, seed), **g))
    door(f"{pre}-enhance_job_u8", name)(lambda e, X: e.enhance_job_u8(X.u8(sh, seed), native.pp_wow(), **g))
    door(f"{pre}-blend_u8", name)(lambda e, X: e.enhance_blend_u8(X.u8(sh, seed), **g))
    door(f"{pre}-blend_u8_f32", name)(lambda e, X: e.enhance_blend_u8(X.u8(sh, seed), want_f32=True, **g))
    if not full:
        return
    door(f"{pre}-blend_u8_job", name)(lambda e, X: e.enhance_blend_u8(X.u8(sh, seed), native.pp_wow(), swap_rb=True, **g))
    door(f"{pre}-masked_u8", name)(lambda e, X: e.enhance_masked_u8(X.u8(sh, seed), _valid(H, W, seed), radius=5, out_nodata=3, **g))
    door(f"{pre}-masked_u8_blend", name)(
        lambda e, X: e.enhance_masked_u8(X.u8(sh, seed), _valid(H, W, seed), radius=5, out_nodata=3, blend=True, **g))
    for mode, what in ((1, "exact"), (2, "smooth")):
        door(f"{pre}-consistent_u8-{what}", name)(lambda e, X, m=mode: e.enhance_consistent_u8(X.u8(sh, seed), mode=m, **g))
    door(f"{pre}-consistent_u8-smooth_blend_masked", name)(
        lambda e, X: e.enhance_consistent_u8(X.u8(sh, seed), mode=2, blend=True, valid=_valid(H, W, seed), radius=5, **g))


def _u16_image_doors(name, case, H, W, tile, pad):
    g = dict(tile=tile, pad=pad)
    sh, seed, pre = (H, W, 3), H, f"{name}-{case}"
    for lo, hi in (FULL, SUB):
        r = f"{lo}_{hi}"
        door(f"{pre}-enhance_u16-{r}", name)(lambda e, X, lo=lo, hi=hi: e.enhance_u16(X.u16(sh, seed), lo, hi, **g))
        door(f"{pre}-blend_u16-{r}", name)(lambda e, X, lo=lo, hi=hi: e.enhance_blend_u16(X.u16(sh, seed), lo, hi, **g))
    door(f"{pre}-enhance_u16_f32", name)(lambda e, X: e.enhance_u16(X.u16(sh, seed), want_f32=True, **g))
    door(f"{pre}-blend_u16_f32", name)(lambda e, X: e.enhance_blend_u16(X.u16(sh, seed), want_f32=True, **g))
    door(f"{pre}-masked_u16", name)(lambda e, X: e.enhance_masked_u16(X.u16(sh, seed), _valid(H, W, seed), *SUB, radius=5, out_nodata=7, **g))
    for mode, what in ((1, "exact"), (2, "smooth")):
        door(f"{pre}-consistent_u16-{what}", name)(lambda e, X, m=mode: e.enhance_consistent_u16(X.u16(sh, seed), *SUB, mode=m, **g))


def _image_doors():
    for case, (H, W, tile, pad) in IMAGES.items():
        _u8_image_doors("x4_hp", case, H, W, tile, pad, full=True)
        _u16_image_doors("x4_hp", case, H, W, tile, pad)
    for name in ("x4_f16", "x4_fp8", "compact"):         # the other nets: the chunked and the short-ramp image, the 8-bit doors
        _u8_image_doors(name, "chunked", *IMAGES["chunked"], full=False)
        _u8_image_doors(name, "short_ramps", *IMAGES["short_ramps"], full=False)
    # x2_odd: 39 x 39 at scale 2 is the reflect-padded 40 x 40 image, tiled and untiled; 3 x 3 the smallest odd one
    _u8_image_doors("x2plus", "odd39_tiled", 39, 39, 16, 3, full=True)
    _u8_image_doors("x2plus", "odd39_untiled", 39, 39, 256, 10, full=False)
    _u8_image_doors("x2plus", "odd3", 3, 3, 256, 10, full=False)


# ---- building blocks -----------------------------------------------------------------------------------------------------------------
def _plan(e, H, W, tile, pad):
    S = e.scale
    PH, PW = (H + H % 2, W + W % 2) if S == 2 else (H, W)
    plan = native.plan_tiles(PH, PW, tile, pad, S)
    w = plan[0]
    return len(plan), w.y2 - w.y1, w.x2 - w.x1


def _cut(e, X, H, W, tile, pad):
    T, wh, ww = _plan(e, H, W, tile, pad)
    img = _dev_u8(X.u8((H, W, 3), H + W))
    buf = _out((T, wh, ww, 3))
    e.cut_windows_u8_dev(img.data_ptr(), H, W, tile, pad, 0, T, buf.data_ptr(), _stream())
    if T > 2:                                            # a part of the plan into a buffer of its own
        part = _out((T - 2, wh, ww, 3))
        e.cut_windows_u8_dev(img.data_ptr(), H, W, tile, pad, 1, T - 2, part.data_ptr(), _stream())
        return _back(buf), _back(part)
    return _back(buf)


def _stitch(e, X, H, W, tile, pad, rows):
    S = e.scale
    T, wh, ww = _plan(e, H, W, tile, pad)
    d_tiles = _dev_u8(X.u8((T, S * wh, S * ww, 3), H * W))
    out = _out((S * H, S * W, 3))
    if not rows:
        e.stitch_windows_u8_dev(d_tiles.data_ptr(), H, W, tile, pad, out.data_ptr(), _stream())
    else:                                                # bands that end on rows that are no multiple of anything, bottom band first
        cuts = [0, 1, 7, S * H // 2 + 1, S * H]
        for a, b in reversed(list(zip(cuts[:-1], cuts[1:]))):
            e.stitch_rows_u8_dev(d_tiles.data_ptr(), H, W, tile, pad, a, b, out.data_ptr(), _stream())
    return _back(out)


def _block_doors():
    for name in ("x4_hp", "x2plus"):
        for case in ("banded", "short_ramps"):
            H, W, tile, pad = IMAGES[case]
            pre = f"{name}-{case}"
            door(f"{pre}-cut_windows", name)(lambda e, X, a=(H, W, tile, pad): _cut(e, X, *a))
            door(f"{pre}-stitch_windows", name)(lambda e, X, a=(H, W, tile, pad): _stitch(e, X, *a, rows=False))
            door(f"{pre}-stitch_rows", name)(lambda e, X, a=(H, W, tile, pad): _stitch(e, X, *a, rows=True))
    H, W = 37, 53
    door("fill_nodata_u8", "x4_hp")(lambda e, X: e.fill_nodata(X.u8((H, W, 3), 21), _valid(H, W, 21), radius=6))
    door("fill_nodata_u16", "x4_hp")(lambda e, X: e.fill_nodata(X.u16((H, W, 3), 22), _valid(H, W, 22), radius=6))
    for S in (2, 4):
        for mode, what in ((1, "exact"), (2, "smooth")):
            door(f"consistency_u8-x{S}-{what}", "x4_hp")(
                lambda e, X, S=S, m=mode: e.consistency(X.u8((S * H, S * W, 3), 23), X.u8((H, W, 3), 24), mode=m, band_rows=9))
            door(f"consistency_u16-x{S}-{what}", "x4_hp")(
                lambda e, X, S=S, m=mode: e.consistency(X.u16((S * H, S * W, 3), 25), X.u16((H, W, 3), 26), mode=m, lo=SUB[0], hi=SUB[1], band_rows=9))


# ---- post-process --------------------------------------------------------------------------------------------------------------------
def _pp(grid, sigma=1.2):
    return native.PPParams(2.5, grid, sigma, 1.4, -0.4, 35, 85, 1.2, 7)


def banded(e, img, prm, hist_cuts, row_cuts, order=0, in_place=False):
    """The s2sr_pp_band_*_dev sequence on a device copy of `img`: hist over the bands of hist_cuts (given out of order on purpose),
    lut, rows over the bands of row_cuts."""
    H, W, _ = img.shape
    x = _dev_u8(img)
    y = x if in_place else torch.full_like(x, FILL)
    st = _stream()
    e.pp_band_begin_dev(H, W, prm, order, st)
    bands = list(zip(hist_cuts[:-1], hist_cuts[1:]))
    for a, b in bands[1::2] + bands[0::2]:
        e.pp_band_hist_dev(x.data_ptr(), a, b, st)
    e.pp_band_lut_dev(st)
    for a, b in zip(row_cuts[:-1], row_cuts[1:]):
        e.pp_band_rows_dev(x.data_ptr(), a, b, y.data_ptr(), st)
    return _back(y)


def _banded(e, img, prm, step):
    cuts = [*range(0, img.shape[0], step), img.shape[0]]
    return banded(e, img, prm, cuts, cuts)


def _pp_batch(e, X, B, H, W, prm):
    x = _dev_u8(X.green((B, H, W, 3), 12))
    y = _out((B, H, W, 3))
    e.postprocess_batch_u8_dev(x.data_ptr(), B, H, W, prm, y.data_ptr(), _stream())
    return _back(y)


def _postprocess_doors():
    prms = {"wow": native.pp_wow(), "farm": native.pp_farm(), "grid16_wide": _pp(16, sigma=2.7)}
    for H, W in ((67, 101), (5, 9)):
        for pn, prm in prms.items():
            pre = f"{H}x{W}-{pn}"
            door(f"postprocess_u8-{pre}", "x4_hp")(lambda e, X, a=(H, W, 3), p=prm: e.postprocess_u8(X.green(a, 10), p))
            door(f"postprocess_batch_u8_dev-{pre}", "x4_hp")(lambda e, X, a=(3, H, W), p=prm: _pp_batch(e, X, *a, p))
            door(f"pp_band_sequence-{pre}", "x4_hp")(lambda e, X, a=(H, W, 3), p=prm: _banded(e, X.green(a, 11), p, 5))
    # one pixel, a sliver, and 70 x 101 with both CLAHE grids: whole at sigma 1.2, and with the widest Gaussian the entries accept
    # (sigma < 2.75: 17 taps, 8 rows of look-ahead, more than a band) whole and in bands of 5 rows ON THE SAME IMAGE, which
    # tests/test_gpu_redzones.py holds to each other
    for H, W in ((1, 1), (3, 300), (70, 101)):
        for grid in (8, 16):
            door(f"postprocess_u8-{H}x{W}-grid{grid}", "x4_hp")(lambda e, X, a=(H, W, 3), p=_pp(grid): e.postprocess_u8(X.green(a, 13), p))
    for grid in (8, 16):
        prm = _pp(grid, sigma=2.7)
        door(f"postprocess_u8-70x101-grid{grid}_wide", "x4_hp")(lambda e, X, p=prm: e.postprocess_u8(X.green((70, 101, 3), 13), p))
        door(f"pp_band_sequence-70x101-grid{grid}_wide", "x4_hp")(lambda e, X, p=prm: _banded(e, X.green((70, 101, 3), 13), p, 5))


# ---- display -------------------------------------------------------------------------------------------------------------------------
def _display_doors():
    lut = np.random.default_rng(99).integers(0, 256, size=(3, 65536), dtype=np.uint8)

    def behind_enhance(e, X, H, W, rows):                # the device copy enhance_u16 leaves: 4H x 4W
        with e.chain_lock:
            q = np.array(e.enhance_u16(X.u16((H, W, 3), H)))
            h = e.display_hist_u16(None, band_rows=rows, shape=(4 * H, 4 * W))
            a = e.display_apply_u16(None, lut, band_rows=rows, shape=(4 * H, 4 * W))
        return q, h, a
    # 37 x 53 whole and in bands of 7 rows; 255 x 257 whole: more than one workgroup's pixels, odd on both axes
    for H, W, rows, tag in ((37, 53, 0, "bands0"), (37, 53, 7, "bands7"), (255, 257, 0, "255x257-bands0")):
        sh = (H, W, 3)
        door(f"display_hist_u16-{tag}", "x4_hp")(lambda e, X, sh=sh, r=rows: e.display_hist_u16(X.u16(sh, sh[0]), band_rows=r))
        door(f"display_hist_u16-nodata-{tag}", "x4_hp")(
            lambda e, X, sh=sh, r=rows: e.display_hist_u16(X.u16(sh, sh[0]), nodata=int(X.u16(sh, sh[0])[0, 0, 0]), band_rows=r))
        door(f"display_apply_u16-{tag}", "x4_hp")(lambda e, X, sh=sh, r=rows: e.display_apply_u16(X.u16(sh, sh[0]), lut, band_rows=r))
    door("display_behind_enhance_u16", "x4_hp")(lambda e, X: behind_enhance(e, X, 37, 53, 7))
    door("display_behind_enhance_u16-255x257-bands0", "x4_hp")(lambda e, X: behind_enhance(e, X, 255, 257, 0))


# ---- pyramid -------------------------------------------------------------------------------------------------------------------------
def _scene(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([120 + 90 * np.sin(xx / 11.0 + c) * np.cos(yy / 7.0) + rng.integers(-15, 16, (h, w)) for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


def _rgba(X, h, w, seed):
    if X.dirty:
        return np.full((h, w, 4), 255, np.uint8)
    rgba = np.concatenate([_scene(h, w, seed=seed), np.full((h, w, 1), 255, np.uint8)], -1)
    rgba[..., 3] = np.where(np.random.default_rng(seed).random((h, w)) < 0.15, 0, 255)
    return rgba


def png_level(X):
    """a 2 x 2 level of the raster's own pixels: one smooth, one noise, one half-covered and one transparent tile"""
    if X.dirty:
        return np.full((512, 512, 4), 255, np.uint8)
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[0:512, 0:512]
    rgba = np.empty((512, 512, 4), np.uint8)
    rgba[..., :3] = np.clip(120 + 80 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 23.0)[..., None] + rng.integers(-4, 5, (512, 512, 3)), 0, 255)
    rgba[:256, 256:, :3] = rng.integers(0, 256, (256, 256, 3))      # noise
    rgba[..., 3] = 255
    rgba[256:384, :256, 3] = 0                                      # half covered
    rgba[256:, 256:, 3] = 0                                         # transparent: no file
    return rgba


def png_level_5x4(X):
    """The 5 x 4 level of tests/test_gpu_tiles.py's PNG pipeline test: smooth tiles, one of noise (tile 7), a half-covered and a
    transparent one."""
    H, W = 4 * 256, 5 * 256
    if X.dirty:
        return np.full((H, W, 4), 255, np.uint8)
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[0:H, 0:W]
    rgba = np.empty((H, W, 4), np.uint8)
    rgba[..., :3] = np.clip(120 + 80 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 23.0)[..., None] + rng.integers(-4, 5, (H, W, 3)), 0, 255)
    rgba[256:512, 512:768, :3] = rng.integers(0, 256, (256, 256, 3))
    rgba[..., 3] = 255
    rgba[768:, :256, 3] = 0
    rgba[:128, 1024:, 3] = 0
    return rgba


def _pngs(e, X, level=png_level, no_path=(), **flags):
    """(the 0/1 array of files written, each tile's file bytes -- empty where there is no file); no_path: tiles given no path"""
    rgba = level(X)
    ny, nx = rgba.shape[0] // 256, rgba.shape[1] // 256
    iy, ix = np.arange(rgba.shape[0], dtype=np.int32), np.arange(rgba.shape[1], dtype=np.int32)
    e.tiles_base_u8(rgba, ix, ix, iy, iy, fetch=False)
    with tempfile.TemporaryDirectory() as d:
        paths = [None if j * nx + i in no_path else Path(d) / f"{j}_{i}.png" for j in range(ny) for i in range(nx)]
        wrote = e.tiles_write_png(nx, ny, paths, **flags).copy()
        files = [np.frombuffer(q.read_bytes(), np.uint8) if q is not None and q.exists() else np.zeros(0, np.uint8) for q in paths]
    return (wrote, *files)


def _pyramid_doors():
    @door("warp_bilinear_u8", "x4_hp")
    def warp(e, X):
        rgb = np.full((150, 211, 3), 255, np.uint8) if X.dirty else _scene(150, 211, seed=32633)
        plan = tiles.plan_warp(211, 150, geo.Placement(600000.0, 5100000.0, 2.5, 2.5), geo.CRS(32633))
        return e.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w)

    place = geo.Placement(1500017.3, 5999994.9, 3.1, 3.1)
    levels = tiles.plan_levels(place.bounds(420, 300), 12, 15)[:3]
    base = tiles.plan_base(levels[0], place, 420, 300)
    door("tiles_base_u8", "x4_hp")(lambda e, X: e.tiles_base_u8(_rgba(X, 300, 420, 2), *base))

    def overview(e, X, on_device):
        child = e.tiles_base_u8(_rgba(X, 300, 420, 2), *base)
        ox, oy = tiles.overview_offsets(levels[1], levels[0])
        return e.tiles_overview_u8(child, ox, oy, levels[1].nx, levels[1].ny, on_device=on_device)
    door("tiles_overview_u8-host_child", "x4_hp")(lambda e, X: overview(e, X, False))
    door("tiles_overview_u8-device_child", "x4_hp")(lambda e, X: overview(e, X, True))

    @door("tiles_overview_u8-two_levels", "x4_hp")
    def two_overviews(e, X):                             # the first from the host copy, the second from the level the first left on the device
        out = [np.array(e.tiles_base_u8(_rgba(X, 300, 420, 2), *base))]
        for k in (1, 2):
            ox, oy = tiles.overview_offsets(levels[k], levels[k - 1])
            out.append(np.array(e.tiles_overview_u8(out[-1], ox, oy, levels[k].nx, levels[k].ny, on_device=(k == 2))))
        return tuple(out)
    box = (-3.7, -46.0, -3.7 + 512 / 9.0, 38.1)          # tests/test_gpu_resample.py OVERZOOM
    for filt in tiles.FILTERS:
        cols = tiles.plan_resample_axis(2 * 256, box[0], box[2], rm.W, filt)
        rows = tiles.plan_resample_axis(2 * 256, box[1], box[3], rm.H, filt)
        door(f"tiles_resample_u8-{filt}", "x4_hp")(
            lambda e, X, c=cols, r=rows: e.tiles_resample_u8(np.full_like(rm.source(), 255) if X.dirty else rm.source(), c, r, 2, 2))
    door("tiles_write_png-wave_rows", "x4_hp")(lambda e, X: _pngs(e, X))
    door("tiles_write_png-row_threads", "x4_hp")(lambda e, X: _pngs(e, X, row_threads=True))
    door("tiles_write_png-host_encoder", "x4_hp")(lambda e, X: _pngs(e, X, host_encoder=True))
    door("tiles_write_png-small_groups", "x4_hp")(lambda e, X: _pngs(e, X, small_groups=True))
    # groups of 3 tiles over 20: the stream buffers regrow between groups, so buffers are freed (and their zones checked) mid-call
    door("tiles_write_png-small_groups_5x4", "x4_hp")(lambda e, X: _pngs(e, X, png_level_5x4, no_path=(7,), small_groups=True))


# ---- raster passes -------------------------------------------------------------------------------------------------------------------
# Under Inputs(dirty=True) a row keeps its geometry -- shapes, masks, zone grids, polygon tables, LUTs, parameters -- and saturates
# the pixel data only.  A counter comes back as a one-element array, a result dict as a tuple in a fixed order: diag.same views bytes.
MODELS = {}                      # ident -> () -> what the numpy model says the row returns; None for an output that has no model


def raster_door(ident, model):
    MODELS[ident] = model
    return door(ident, "x4_hp")


def _n(x):
    return np.array([x], np.uint64)


def _carry(e, X, S, rows, chain=False):
    q, b, v = bm.case(37, 45, S)
    kw = dict(lo=1000, hi=11000, r=4, eps=5, valid=v, fill=9, band_rows=rows)
    if not chain:
        got, n = e.carry_band_u16(X.like(b), S, sr=X.like(q), **kw)
        return got, _n(n)
    with e.chain_lock:                                   # the same call, then again from the guide it kept on the device
        got, n = e.carry_band_u16(X.like(b), S, sr=X.like(q), **kw)
        got = np.array(got)
        kept, m = e.carry_band_u16(X.like(b), S, sr=None, **kw)
    return got, _n(n), kept, _n(m)


def _carry_model(S, twice=False):
    want, bad = bm.modelled(37, 45, S, 1000, 11000, (1, 1, 1), 4, 5, True, 9)
    return (want, _n(bad)) * (2 if twice else 1)


def _index_case(H, W, zs, Z):
    """tests/test_gpu_index.py's call: channel 1 against a plane, offset 1000, the mask at scale 4, zones, the LUT, every output"""
    A, B, grids, lut = im.case(H, W)
    kw = dict(ca=1, offset=1000, valid=grids["valid", 4], valid_scale=4, zones=grids["zones", zs, Z], zone_scale=zs, Z=Z, lut=lut, want=im.OUTPUTS)
    return A, im.plane(B, 1, 0), kw


def _index_tuple(r):
    return tuple(np.array(r[k]) for k in im.OUTPUTS) + (_n(r["undefined"]),)


def _index(e, X, H, W, zs, Z, rows, kept=False):
    A, b, kw = _index_case(H, W, zs, Z)
    if not kept:
        return _index_tuple(e.index_nd_u16(X.like(A), X.like(b), band_rows=rows, **kw))
    with e.chain_lock:                                   # the display pass leaves A on the device as the kept image
        hist = np.array(e.display_hist_u16(X.like(A)))
        return (hist,) + _index_tuple(e.index_nd_u16(None, X.like(b), band_rows=rows, **kw))


def _index_model(H, W, zs, Z, kept=False):
    A, b, kw = _index_case(H, W, zs, Z)
    want = im.model(A[..., 1], b, 1000, 0, 10000, kw["valid"], 4, kw["zones"], zs, Z, kw["lut"])
    return ((dm.hist(A),) if kept else ()) + _index_tuple(want)


def _render_input(X, H, W):
    idx = X.i16((H, W), 1000 * H + W)
    if not X.dirty:
        idx[::5] = im.NODATA
    return idx


def _zones(e, H, W, kind, **kw):
    tabs, Z, _, _ = zm.case(H, W, kind)
    labels, area = e.zones_rasterize_u16(*tabs, Z, (H, W), **kw)          # no pixel data: the saturated call is the call
    return labels if area is None else (labels, area)


def _fields(e, X, H, W, name, **kw):
    labels, fields, found = e.fields_segment_i16(X.like(fm.raster(H, W, name)), fm.LO, fm.HI, **kw)
    return labels, fields, _n(found)


def _fields_model(H, W, name, **kw):
    labels, fields, found = fm.case(H, W, name, **kw)
    return labels, fields, _n(found)


MZ_KEYS = ("zone", "table", "centres", "status")
# management zones: tag -> (H, W, features, layout, parameters).  Two cases at 65 x 129 (one raster and two, smoothing 1 and 2); 130
# x 197 on one field with k 8 in bands of 7 rows and whole (whole: 20 tiles of 64 x 32, which a cap of 8 makes smaller; in bands of 7
# rows no launch has more than 4); one pixel; W % 8 == 0 with D 4 and k 8, and W % 8 == 4 in bands of 5 rows
MZ_ROWS = {"65x129-noise-grid16": (65, 129, "noise", "grid16", dict(smooth=1)),
           "65x129-nodata_ramp-stripes-k5": (65, 129, ("nodata", "ramp"), "stripes", dict(k=5, min_per_zone=1, smooth=2)),
           "130x197-planted_nodata-one-k8-bands7": (130, 197, ("planted", "nodata"), "one", dict(k=8, smooth=2, band_rows=7)),
           "130x197-planted_nodata-one-k8": (130, 197, ("planted", "nodata"), "one", dict(k=8, smooth=2)),
           "1x1-noise-one": (1, 1, "noise", "one", dict(k=2, min_per_zone=1)),
           "65x128-d4-grid16-k8": (65, 128, ("planted", "noise", "nodata", "extremes"), "grid16", dict(k=8, min_per_zone=1, smooth=1)),
           "37x180-noise_nodata-grid16-bands5": (37, 180, ("noise", "nodata"), "grid16", dict(smooth=2, min_per_zone=3, band_rows=5))}
EDGE, MORPH = {"edge": 150, "edge_r": 1}, dict(r_open=1, r_close=2)          # tests/test_gpu_fields_split.py
# the split: tag -> (H, W, raster, split, parameters).  Three cases at 65 x 129 (edge test, morphology, corridor); 130 x 197 (12
# growth tiles and 101 per-pixel blocks: a second trip under a cap of 8); one pixel; W % 8 == 0 and W % 8 == 4
SPLIT_ROWS = {"65x129-blobs-edge-morph": (65, 129, "blobs", EDGE, dict(conn=4, **MORPH)),
              "65x129-parcels-edge_r0": (65, 129, "parcels", {"edge": 150, "edge_r": 0}, dict(conn=8)),
              "65x129-snake-plain": (65, 129, "snake", {}, dict(conn=4)),
              "130x197-blobs-edge": (130, 197, "blobs", EDGE, dict(conn=8)),
              "1x1-ones": (1, 1, "ones", {}, {}),
              "65x128-blobs-edge-morph": (65, 128, "blobs", EDGE, dict(conn=8, min_pixels=3, **MORPH)),
              "37x180-blobs-edge": (37, 180, "blobs", EDGE, dict(conn=4))}


def _mzones_tuple(r):
    return tuple(np.array(r[k]) for k in MZ_KEYS) + (_n(r["iterations"]),)


def _mzones(e, X, H, W, features, lay, kw):
    feats, labels, Z = mm.inputs(H, W, features, lay)              # the labels are geometry: they stay under the saturated features
    return _mzones_tuple(e.zones_kmeans_i16(X.like(feats), labels, Z, **kw))


def _mzones_model(H, W, features, lay, kw):
    return _mzones_tuple(mm.case(H, W, features, lay, **{k: v for k, v in kw.items() if k != "band_rows"}))


def _split(e, X, H, W, name, split, kw):
    labels, fields, found, dist2, cores = e.fields_split_i16(X.like(sm.raster(H, W, name)), fm.LO, fm.HI, split=split, want=("dist2", "cores"), **kw)
    return labels, fields, _n(found), dist2, cores


def _split_model(H, W, name, split, kw):
    r = sm.case(H, W, name, split=split, **kw)
    return r["labels"], r["fields"], _n(r["found"]), r["dist2"], r["cores"]


def _masked_warp(e, X, then_base=False):
    """the 150 x 211 / vs = 4 case, and the base level cut from the raster it keeps: the hand-over under the modes"""
    rgb, valid, vs, plan, _ = wm.case(32633, "coarse")
    raster = wm.warp(e, X.like(rgb), valid, vs, plan)
    if not then_base:
        return raster
    raster = np.array(raster)
    lv = tiles.plan_levels(plan.placement.bounds(plan.out_w, plan.out_h), 15, 15)[0]
    return raster, e.tiles_base_u8(raster.shape[:2], *tiles.plan_base(lv, plan.placement, plan.out_w, plan.out_h), on_device=True)


def _raster_doors():
    # the carried band at 37 x 45, masked: in bands of 2 S + 1 guide rows, the S = 4 chain from the kept copy, and S = 4 whole (9
    # tiles in one launch: the only one of these that a cap of 8 makes smaller)
    for S in (2, 4):
        raster_door(f"carry_band_u16-x{S}-bands", lambda S=S: _carry_model(S))(lambda e, X, S=S: _carry(e, X, S, 2 * S + 1))
    raster_door("carry_band_u16-x4-bands-kept_chain", lambda: _carry_model(4, twice=True))(lambda e, X: _carry(e, X, 4, 9, chain=True))
    raster_door("carry_band_u16-x4-whole", lambda: _carry_model(4))(lambda e, X: _carry(e, X, 4, 0))
    # the index: the ragged shape in bands of 5 rows with zones at scale 1, Z = 65535; 255 x 257 (65535 pixels: 8 workgroups' worth,
    # a ragged last group) whole with zones at scale 4, Z = 7; from the kept copy; the rendering of a raster that exists
    for H, W, zs, Z, rows, tag in ((37, 45, 1, 65535, 5, "37x45-bands5"), (255, 257, 4, 7, 0, "255x257")):
        raster_door(f"index_nd_u16-{tag}", lambda a=(H, W, zs, Z): _index_model(*a))(lambda e, X, a=(H, W, zs, Z, rows): _index(e, X, *a))
        raster_door(f"index_render_i16-{tag}", lambda a=(H, W): im.render(_render_input(Inputs(), *a), im.case(*a)[3]))(
            lambda e, X, a=(H, W), r=rows: e.index_render_i16(_render_input(X, *a), im.case(*a)[3], band_rows=r))
    raster_door("index_nd_u16-37x45-bands5-kept", lambda: _index_model(37, 45, 1, 65535, kept=True))(
        lambda e, X: _index(e, X, 37, 45, 1, 65535, 5, kept=True))
    # zones: the scene in bands, on 4 x 5 tiles and on one pixel, the ring of 1000 vertices, and labels without area
    # (and at the widths of the SR grid: 16-byte stores across a tile line, 8-byte stores with a row tail of 4, scalar stores at x2)
    for H, W, kind, kw, tag in ((37, 45, "scene", dict(band_rows=5), "37x45-bands5"), (255, 257, "scene", {}, "255x257"), (1, 1, "scene", {}, "1x1"),
                                (255, 257, "star", {}, "255x257"), (65, 128, "scene", {}, "65x128"), (37, 180, "scene", dict(band_rows=5), "37x180-bands5"),
                                (39, 78, "scene", {}, "39x78")):
        raster_door(f"zones_rasterize_u16-{kind}-{tag}", lambda a=(H, W, kind): zm.case(*a)[2:])(lambda e, X, a=(H, W, kind), kw=kw: _zones(e, *a, **kw))
    raster_door("zones_rasterize_u16-scene-37x45-no_area", lambda: zm.case(37, 45)[2])(lambda e, X: _zones(e, 37, 45, "scene", want_area=False))
    # fields: one component through all 3 x 4 tiles, the morphology, one pixel, and more fields than Z
    # (and the morphology at the widths of the SR grid: 8-byte masks and 16-byte labels, and the scalar forms at W % 8 == 4)
    for H, W, name, kw in ((130, 197, "spiral", dict(conn=4)), (65, 129, "blobs", dict(r_open=1, r_close=2, conn=8, min_pixels=3)), (1, 1, "ones", {}),
                           (63, 65, "noise", dict(conn=8, Z=5)), (65, 128, "blobs", dict(r_open=1, r_close=2, conn=8, min_pixels=3)),
                           (37, 180, "blobs", dict(r_open=1, r_close=1, conn=4))):
        raster_door(f"fields_segment_i16-{H}x{W}-{name}", lambda a=(H, W, name), kw=kw: _fields_model(*a, **kw))(
            lambda e, X, a=(H, W, name), kw=kw: _fields(e, X, *a, **kw))
    for tag, row in MZ_ROWS.items():
        raster_door(f"zones_kmeans_i16-{tag}", lambda row=row: _mzones_model(*row))(lambda e, X, row=row: _mzones(e, X, *row))
    for tag, row in SPLIT_ROWS.items():
        raster_door(f"fields_split_i16-{tag}", lambda row=row: _split_model(*row))(lambda e, X, row=row: _split(e, X, *row))
    raster_door("warp_bilinear_masked_u8", lambda: wm.case(32633, "coarse")[4])(lambda e, X: _masked_warp(e, X))
    raster_door("warp_bilinear_masked_u8-then-base", lambda: (wm.case(32633, "coarse")[4], None))(lambda e, X: _masked_warp(e, X, then_base=True))


def owned(prefix):
    """the raster rows of one pass, for the module that holds their baselines to the model"""
    return [i for i in MODELS if i.startswith(prefix)]


_net_doors()
_image_doors()
_block_doors()
_postprocess_doors()
_display_doors()
_pyramid_doors()
_raster_doors()
