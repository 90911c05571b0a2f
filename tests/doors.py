"""The doors of the library as a table: id -> (engine config, fn(engine, inputs) -> arrays).  One entry is ONE call (or the short
sequence that makes a door, such as base level + overview), on the configs and shapes of tests/test_gpu_redzones.py: the smallest
that take each route.  tests/test_gpu_poison.py runs every entry in its three states; `inputs` lets a state ask for the same
call, with the same geometry, on a saturated input (Inputs(dirty=True): all 255 / 65535 / 1.0)."""
import tempfile
from pathlib import Path

import numpy as np
import torch

import resample_model as rm
import test_gpu_redzones as rz
from s2sr import geo, native, tiles

CONFIGS, NET_SHAPES, IMAGES, FULL, SUB = rz.CONFIGS, rz.NET_SHAPES, rz.IMAGES, rz.FULL, rz.SUB
FILL = 0x5A                      # what a caller-owned output buffer holds before the call, on both sides of a comparison


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


DOORS = {}


def door(ident, config):
    def add(fn):
        assert ident not in DOORS, ident
        DOORS[ident] = (config, fn)
        return fn
    return add


# ---- net doors -----------------------------------------------------------------------------------------------------------------------
def _fwd_u8_dev(e, t8, S):
    B, th, tw, _ = t8.shape
    x, y = rz._dev_u8(t8), _out((B, S * th, S * tw, 3))
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
                door(f"{pre}-forward_part_u8_dev", name)(lambda e, X, d=dims, s=seed, j=job, S=S: rz._part(e, X.u8(d, s), j, S))
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
    if not full:
        return
    door(f"{pre}-blend_u8_f32", name)(lambda e, X: e.enhance_blend_u8(X.u8(sh, seed), want_f32=True, **g))
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
    img = rz._dev_u8(X.u8((H, W, 3), H + W))
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
    d_tiles = rz._dev_u8(X.u8((T, S * wh, S * ww, 3), H * W))
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
def _pp_batch(e, X, B, H, W, prm):
    x = rz._dev_u8(X.green((B, H, W, 3), 12))
    y = _out((B, H, W, 3))
    e.postprocess_batch_u8_dev(x.data_ptr(), B, H, W, prm, y.data_ptr(), _stream())
    return _back(y)


def _postprocess_doors():
    prms = {"wow": native.pp_wow(), "farm": native.pp_farm(), "grid16_wide": rz._pp(16, sigma=2.7)}
    for H, W in ((67, 101), (5, 9)):
        for pn, prm in prms.items():
            pre = f"{H}x{W}-{pn}"
            door(f"postprocess_u8-{pre}", "x4_hp")(lambda e, X, a=(H, W, 3), p=prm: e.postprocess_u8(X.green(a, 10), p))
            door(f"postprocess_batch_u8_dev-{pre}", "x4_hp")(lambda e, X, a=(3, H, W), p=prm: _pp_batch(e, X, *a, p))
            door(f"pp_band_sequence-{pre}", "x4_hp")(lambda e, X, a=(H, W, 3), p=prm: rz._banded(e, X.green(a, 11), p, 5, fill=FILL))


# ---- display -------------------------------------------------------------------------------------------------------------------------
def _display_doors():
    H, W = 37, 53
    lut = np.random.default_rng(99).integers(0, 256, size=(3, 65536), dtype=np.uint8)
    sh = (H, W, 3)
    for rows in (0, 7):
        door(f"display_hist_u16-bands{rows}", "x4_hp")(lambda e, X, r=rows: e.display_hist_u16(X.u16(sh, H), band_rows=r))
        door(f"display_hist_u16-nodata-bands{rows}", "x4_hp")(
            lambda e, X, r=rows: e.display_hist_u16(X.u16(sh, H), nodata=int(X.u16(sh, H)[0, 0, 0]), band_rows=r))
        door(f"display_apply_u16-bands{rows}", "x4_hp")(lambda e, X, r=rows: e.display_apply_u16(X.u16(sh, H), lut, band_rows=r))

    @door("display_behind_enhance_u16", "x4_hp")
    def behind_enhance(e, X):                            # the device copy enhance_u16 leaves: 4H x 4W
        with e.chain_lock:
            q = rz.keep(e.enhance_u16(X.u16(sh, H)))
            h = e.display_hist_u16(None, band_rows=7, shape=(4 * H, 4 * W))
            a = e.display_apply_u16(None, lut, band_rows=7, shape=(4 * H, 4 * W))
        return q, h, a


# ---- pyramid -------------------------------------------------------------------------------------------------------------------------
def _rgba(X, h, w, seed):
    if X.dirty:
        return np.full((h, w, 4), 255, np.uint8)
    rgba = np.concatenate([rz._scene(h, w, seed=seed), np.full((h, w, 1), 255, np.uint8)], -1)
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


def _pngs(e, X, **flags):
    ident = np.arange(512, dtype=np.int32)
    e.tiles_base_u8(png_level(X), ident, ident, ident, ident, fetch=False)
    with tempfile.TemporaryDirectory() as d:
        paths = [Path(d) / f"{j}_{i}.png" for j in range(2) for i in range(2)]
        wrote = e.tiles_write_png(2, 2, paths, **flags).copy()
        files = [np.frombuffer(q.read_bytes(), np.uint8) if q.exists() else np.zeros(0, np.uint8) for q in paths]
    return (wrote, *files)


def _pyramid_doors():
    @door("warp_bilinear_u8", "x4_hp")
    def warp(e, X):
        rgb = np.full((150, 211, 3), 255, np.uint8) if X.dirty else rz._scene(150, 211, seed=32633)
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


_net_doors()
_image_doors()
_block_doors()
_postprocess_doors()
_display_doors()
_pyramid_doors()
