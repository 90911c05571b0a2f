"""Probe nets: weights that make the net an exactly known map of its input, so that every kernel that only moves data (the tile
packers and their mosaic placement, the window gather and its reflect form, the stitch forms, the channel swap, the halo and
separator zeros every conv relies on) is judged byte for byte.  Plain numpy; nothing here touches the device.

The RRDB probe: all weights zero except one tap of weight 1 per colour in conv_first (and the centre tap, weight 1, in conv_up1,
conv_up2, conv_hr, conv_last) and conv_last.bias = 0.5 / 255.  conv_body is zero, so the trunk adds exactly 0.  With the centre
tap everywhere the net is nearest-x4 of its input; with an off-centre tap in one layer it is nearest-x4 of the input shifted by
one pixel of that layer's grid, zeros coming in from outside whatever the net was given.  Values stay >= 0, so every LeakyReLU
is the identity.

Why the u8 doors are exact under it: operands 1.0 and integers <= 255 are exact in fp16 and accumulate in fp32; the one rounding
is the fp16 (or hi + lo) storage of u / 255, relative error 2^-11, at most 0.125 after the x 255.  With the 0.5 / 255 bias
trunc(y * 255) sees u + 0.5 +- 0.125: u.

The compact probe: SRVGGNetCompact adds nearest-x4 of its input to its output, so the all-zero net with last bias 0.5 / 255 is
nearest-x4; the shift probe routes the three colours through one tap of the first conv, centre taps of weight 1 in the body and
centre taps of weight 1 into all 16 sub-pixel channels of each colour: out * 255 = u + shift(u) + 0.5 (+- 0.125: one fp16
rounding of shift(u) / 255; the base u / 255 is fp32)."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from oracle import rrdbnet_ref as ref
from s2sr.weights import compact_specs, synthetic_state_dict

# the plans of tests/test_gpu_cut_stitch.py (those of test_cut_forward_stitch_equals_enhance): H, W, tile, pad
STITCH_GEOS = [(37, 45, 16, 2), (50, 41, 16, 2), (64, 65, 32, 4), (33, 70, 16, 3), (49, 48, 16, 2), (70, 36, 32, 2)]
TAP_LAYERS = ("conv_first", "conv_up1", "conv_up2", "conv_hr", "conv_last")
# the H / W at which window plans change shape, for a tile t and pad p (win = t + 2p)
def edge_sizes(t, p):
    win = t + 2 * p
    return sorted({1, 2, 3, t - 1, t, t + 1, win - 1, win, win + 1, 2 * t - 1, 2 * t, 2 * t + 1, 2 * t + p, 2 * t + 2 * p,
                   2 * t + 2 * p + 1, 3 * t + 1})


# ---- weights ------------------------------------------------------------------------------------------------------------------
def probe_state_dict(num_block, scale=4, tap_layer="conv_first", tap=(1, 1), sub=(0, 0), out_offset=(0, 0, 0), bias=0.5):
    """The RRDB probe with the shapes of synthetic_state_dict.  tap_layer / tap: the layer that carries the (ty, tx) tap (every
    other layer its centre tap).  sub = (i, j): at scale 2, conv_first reads pixel-unshuffle channel c*4 + i*2 + j.  out_offset:
    k_c / 255 added to the bias of output channel c; bias: the rounding offset in LSB (0.5 for the truncating u8 door, 0 for the
    rounding 16-bit door)."""
    assert tap_layer in TAP_LAYERS and scale in (2, 4)
    sd = OrderedDict((k, np.zeros_like(v)) for k, v in synthetic_state_dict(num_block, seed=0, scale=scale).items())
    for name in TAP_LAYERS:
        ty, tx = tap if name == tap_layer else (1, 1)
        for c in range(3):
            cin = c * 4 + sub[0] * 2 + sub[1] if (name == "conv_first" and scale == 2) else c
            sd[name + ".weight"][c, cin, ty, tx] = 1.0
    sd["conv_last.bias"][:] = (np.float64(bias) + np.asarray(out_offset, np.float64)) / 255.0
    return sd


def compact_probe_state_dict(num_conv=16, tap=None):
    """tap None: the all-zero net with last bias 0.5 / 255 (nearest-x4 through the base add).  tap (ty, tx): the shift probe,
    out * 255 = u + shift(u, tap) + 0.5."""
    sd = OrderedDict((k, np.zeros(shape, np.float32)) for k, shape in compact_specs(num_conv))
    last = 2 * num_conv + 2
    for i in range(num_conv + 1):
        sd[f"body.{2 * i + 1}.weight"][:] = 0.25          # PReLU slopes: never reached (no value is negative)
    sd[f"body.{last}.bias"][:] = 0.5 / 255.0
    if tap is not None:
        for c in range(3):
            sd["body.0.weight"][c, c, tap[0], tap[1]] = 1.0
            for i in range(1, num_conv + 1):
                sd[f"body.{2 * i}.weight"][c, c, 1, 1] = 1.0
            sd[f"body.{last}.weight"][c * 16:(c + 1) * 16, c, 1, 1] = 1.0
    return sd


# ---- images -------------------------------------------------------------------------------------------------------------------
def coded(H, W):
    """HxWx3 u8 in which any two 8-neighbours differ in every channel and every value is >= 1 (a zero would pass for a halo)."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([7 * x + 19 * y + 3, 23 * x + 11 * y + 5, 13 * x + 29 * y + 1], -1) % 256
    return np.maximum(img, 1).astype(np.uint8)


def coded_u16(H, W):
    """HxWx3 u16 whose 8-neighbours are >= 1024 levels apart in every channel, every value >= 1."""
    y, x = np.mgrid[0:H, 0:W]
    img = (np.stack([7 * x + 19 * y + 3, 23 * x + 11 * y + 5, 13 * x + 29 * y + 1], -1) * 1031) % 65536
    return np.maximum(img, 1).astype(np.uint16)


def min_neighbour_gap(img):
    """The smallest |difference| between 8-neighbours, over all channels (inf for a single pixel)."""
    a = img.astype(np.int64)
    H, W = a.shape[:2]
    gaps = [np.inf]
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        p = a[:H - dy, max(0, -dx):W - max(0, dx)]
        q = a[dy:, max(0, dx):W + min(0, dx)]
        if p.size:
            gaps.append(np.abs(p - q).min())
    return min(gaps)


# ---- the expectation ----------------------------------------------------------------------------------------------------------
def shift(a, tap):
    """What a 3x3 conv with the single tap (ty, tx) of weight 1 and zero padding makes of a [h, w, C]: out[y, x] =
    a[y + ty - 1, x + tx - 1], zero outside."""
    dy, dx = tap[0] - 1, tap[1] - 1
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ys, xs = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))
    yd, xd = slice(max(0, dy), h + min(0, dy)), slice(max(0, dx), w + min(0, dx))
    out[ys, xs] = a[yd, xd]
    return out


def up(a, k):
    return np.repeat(np.repeat(a, k, axis=0), k, axis=1)


def reflect_even(img):
    """The mod-2 rule of the scale-2 door: one reflected row / column at the bottom / right of an odd H / W."""
    H, W = img.shape[:2]
    return np.pad(img, ((0, H % 2), (0, W % 2), (0, 0)), mode="reflect") if (H % 2 or W % 2) else img


def expected(img, scale=4, tap_layer="conv_first", tap=(1, 1), sub=(0, 0), out_offset=(0, 0, 0)):
    """What the probe net makes of the integer image img [H, W, 3], as int64 [scale H, scale W, 3] (unclipped): shift on the
    tap layer's grid, nearest upsampling between the grids, the reflect pad and the sub-pixel pick at scale 2."""
    H, W = img.shape[:2]
    a = np.asarray(img).astype(np.int64)
    if scale == 2:
        a = reflect_even(a)[sub[0]::2, sub[1]::2]
    t = lambda name: tap if name == tap_layer else (1, 1)
    a = shift(a, t("conv_first"))
    a = shift(up(a, 2), t("conv_up1"))
    a = shift(up(a, 2), t("conv_up2"))
    a = shift(shift(a, t("conv_hr")), t("conv_last"))
    return a[:scale * H, :scale * W] + np.asarray(out_offset, np.int64)


def expected_u8(img, **kw):
    return np.clip(expected(img, **kw), 0, 255).astype(np.uint8)


def compact_expected(img, tap=None):
    """The compact probes on an integer image: int64 [4H, 4W, 3], unclipped."""
    a = np.asarray(img).astype(np.int64)
    return up(a, 4) if tap is None else up(a + shift(a, tap), 4)


# ---- the reference's paste ----------------------------------------------------------------------------------------------------
def paste_replay(windows_out, plan):
    """`_tile_process`'s loop over oracle.rrdbnet_ref.tile_plan: windows_out[t] [S wh, S ww, C] cropped and pasted in plan
    order, later windows overwriting.  A plan whose crops do not fit its windows raises, as the reference's slice assignment."""
    OH, OW = max(p[2][1] for p in plan), max(p[2][3] for p in plan)
    w0 = np.asarray(windows_out[0])
    out = np.zeros((OH, OW) + w0.shape[2:], w0.dtype)
    for t, (_, (top, bottom, left, right), (oy1, oy2, ox1, ox2)) in zip(windows_out, plan):
        t = np.asarray(t)
        out[oy1:oy2, ox1:ox2] = t[top:t.shape[0] - bottom, left:t.shape[1] - right]
    return out


def paste_first_wins(windows_out, plan):
    """A wrong paste: the FIRST window that covers a pixel keeps it."""
    OH, OW = max(p[2][1] for p in plan), max(p[2][3] for p in plan)
    w0 = np.asarray(windows_out[0])
    out = np.zeros((OH, OW) + w0.shape[2:], w0.dtype)
    for t, (_, (top, bottom, left, right), (oy1, oy2, ox1, ox2)) in reversed(list(zip(windows_out, plan))):
        t = np.asarray(t)
        out[oy1:oy2, ox1:ox2] = t[top:t.shape[0] - bottom, left:t.shape[1] - right]
    return out


def paste_crop_moved(windows_out, plan, dy, dx):
    """A wrong paste: every crop moved by (dy, dx) output pixels inside its window (rolled, so the shapes stay)."""
    return paste_replay([np.roll(np.asarray(t), (-dy, -dx), axis=(0, 1)) for t in windows_out], plan)


def window_tiles(T, oh, ow, seed=0):
    """[T, oh, ow, 3] u8: a hash of (window, y, x, c), so that no two windows agree over any stretch of pixels."""
    t, y, x, c = np.meshgrid(np.arange(T), np.arange(oh), np.arange(ow), np.arange(3), indexing="ij", sparse=True)
    with np.errstate(over="ignore"):
        v = (t.astype(np.uint64) * np.uint64(0x9E3779B1) + y.astype(np.uint64) * np.uint64(0x85EBCA77)
             + x.astype(np.uint64) * np.uint64(0xC2B2AE3D) + c.astype(np.uint64) * np.uint64(0x27D4EB2F) + np.uint64(seed))
        v ^= v >> np.uint64(15)
        v *= np.uint64(0x2C1B3C6D)
        v ^= v >> np.uint64(12)
    return (v & np.uint64(0xFF)).astype(np.uint8)


def plan_windows_of(img, plan):
    """The plan's input windows, cut from img with numpy slices."""
    return [img[y1:y2, x1:x2] for (y1, y2, x1, x2), _, _ in plan]


def tiled_expected(img, tile, pad, scale=4, **kw):
    """The reference's tiled route under the probe, replayed in numpy: each window through `expected` on its own (zeros come in
    at the window's sides), pasted with paste_replay.  Scale 2: the windows of the reflect-padded image, cropped at the end."""
    H, W = img.shape[:2]
    src = reflect_even(np.asarray(img)) if scale == 2 else np.asarray(img)
    plan = ref.tile_plan(src.shape[0], src.shape[1], tile, pad, scale)
    off = np.asarray(kw.pop("out_offset", (0, 0, 0)), np.int64)
    outs = [expected(w, scale=scale, **kw) for w in plan_windows_of(src, plan)]
    return paste_replay(outs, plan)[:scale * H, :scale * W] + off


def is_tiled(H, W, tile, scale=4):
    """The whole / tiled switch of RealESRGAN.enhance (strict '>', on the padded size at scale 2)."""
    if scale == 2:
        H, W = H + H % 2, W + W % 2
    return H * W > tile * tile * 4


# ---- the f32 packers ----------------------------------------------------------------------------------------------------------
def pack_f32_rule(x):
    """What the f32 packers store of x: fp16(fp32(x * 255)) -- the product rounded to fp32, then to fp16."""
    return (np.asarray(x, np.float32) * np.float32(255.0)).astype(np.float16).astype(np.float32)


def expected_p0_f32(x, geo, scale):
    """[n, 16, Hp, Wp] fp32: tap P0 for the fp32 input x [B, 3, th, tw] -- the packing rule at the positions the packer writes
    (plain images or a mosaic; at scale 2 the pixel-unshuffled order c*4 + i*2 + j on the half grid), zeros everywhere else."""
    B, _, th, tw = x.shape
    v = pack_f32_rule(x)
    if scale == 2:
        v = v.reshape(B, 3, th // 2, 2, tw // 2, 2).transpose(0, 1, 3, 5, 2, 4).reshape(B, 12, th // 2, tw // 2)
    h, w = v.shape[2:]
    p0 = np.zeros((geo["n"], 16, geo["Hp"][0], geo["Wp"][0]), np.float32)
    kx, ky = (geo["mos_kx"], geo["mos_ky"]) if geo["mos_kx"] else (1, 1)
    for t in range(B):
        i, slot = divmod(t, kx * ky)
        wy, wx = divmod(slot, kx)
        y0, x0 = 1 + wy * (h + 1), 1 + wx * (w + 1)
        p0[i, :v.shape[1], y0:y0 + h, x0:x0 + w] = v[t]
    return p0


def first_difference(got, want):
    """'' when equal, else 'N differ, first at [index]: got g, want w'."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = got != want
    if not bad.any():
        return ""
    i = tuple(np.argwhere(bad)[0].tolist())
    return f"{int(bad.sum())} of {bad.size} differ, first at {list(i)}: got {got[i]}, want {want[i]}"
