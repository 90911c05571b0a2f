"""The per-layer judge of SRVGGNetCompact IN SITU: what s2sr_debug_compact_taps returns for one batch through the production
schedule (the packed input p0, the fp16 activation behind any tapped layer over the padded extent, out_f32 / out_u8 of the same
run) against a float64 model of every layer computed from the STORED field that layer read, so one layer is what is judged and
errors do not compound.  Importable without a GPU and asserting nothing itself: `judge` returns a report, tests/
test_compact_insitu_cpu.py feeds it planted faults, tests/test_gpu_compact_insitu.py and test_gpu_compact.py feed it the device.

Rules (all derived; the only constants are tail_model.U32 and the fp16 quantum):
  layer 0          conv(p0[:3], fp16(w)) * (1/255) + b, PReLU                      csrc/conv3x3.hip EPI_CFIRST
  layer k          conv(acts[k - 1], fp16(w)) + b, PReLU                           EPI_PRELU
     bound per element: tail_model.Layer.result (stages x taps fp32 accumulator roundings of half an ulp of the running sum, two
     ulps for the epilogue) through the PReLU (slopes below 1 do not widen it) + U32 |v| for the slope multiply + half an fp16
     quantum for the store.
  the last conv    pixel_shuffle(conv(acts[num_conv], fp16(w)) + b, 4) + base, base = fp32(p0[c] * fp32(1/255)) of this LR pixel
     under all 16 sub-pixels (exact by definition: EPI_CLAST reads it from P0); bound: Layer.result + U32 |out| for the fp32 add.
     No store quantum: the output is fp32.
  out_u8           trunc(clip(fp32(out_f32 * 255), 0, 255)) of the DEVICE's out_f32: byte for byte.
  p0               channels 0..2 at live pixels are the input exactly (u8 entry: the integers; f32 entry: fp16(fp32(255 x)) bit for
     bit), channels 3..15 zero.
  zeros            every tapped activation is exactly zero outside the pixels px_live (s2sr_internal.h) admits: the halo ring, the
     round-up band, the mosaic separators.  px_live knows nothing of mos_count, so a DEAD mosaic slot (job_windows > B) is computed
     like a live window on whatever P0 holds there: its activations are judged against the model like a live window's, its p0 must
     be zero on a fresh engine, and nothing of it reaches out_f32 / out_u8 (those have B images).
Regions of the report, as test_gpu_trunk_insitu._regions: interior, last partial patch row / column (the compact convs work on
16-row x 32-column patches: 8 waves x 2 rows), image border ring, pixels next to a mosaic separator."""
from __future__ import annotations

import numpy as np

import tail_model as tm
from s2sr import weights as W

ROWS, COLS = 16, 32          # conv3x3.hip, the 8-wave form: TH = WAVES * NP = 16, TW = 32
REGIONS = ("interior", "partial", "ring", "sep")
INV255 = np.float32(1.0 / 255.0)


def num_conv_of(sd) -> int:
    return (max(int(k.split(".")[1]) for k in sd if k.startswith("body.")) - 2) // 2


def insitu_sd(nc):
    """The per-layer tests judge one layer at a time on the device's own operands, so they need no net-level stability; they do
    need both signs in every channel at every depth.  With the golden's weights (biases of 0.05, body gain 0.90) the signal 32
    layers deep is smaller than some channels' bias and 7 of the 64 pre-activation channels stay positive on any input (CPU,
    float32).  Same generator, zero-mean rows, biases of 0.01, body gain 1.0: every channel of every layer 0 .. num_conv goes
    negative (tests/test_compact_insitu_cpu.py asserts it on the batches of test_gpu_compact.test_layers_in_situ), and the PReLU
    slope vectors (0.05 .. 0.35) of all layers are distinct."""
    return W.synthetic_compact_state_dict(nc, seed=0, zero_mean=True, bias_amp=0.01, body_gain=1.0)


def insitu_tiles(seed, B, th, tw):
    """Noise tiles plus one smooth tile (ramps, a checkerboard channel, flat dark / bright corners) and one posterised tile."""
    t = np.random.default_rng(seed).integers(0, 256, (B, th, tw, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:th, 0:tw]
    g = np.stack([xx * 255 // (tw - 1), yy * 255 // (th - 1), ((xx + yy) % 2) * 255], -1).astype(np.uint8)
    g[: th // 4, : tw // 4] = 0
    g[-(th // 4):, -(tw // 4):] = 255
    t[1] = g
    if B > 2:
        t[2] = (t[2] // 64) * 85
    return t


def structured_tiles(seed, B, th, tw):
    """Noise tiles of any size; from 8 x 8 pixels on, the top-left block of tile 0 (up to 32 x 48) holds the smooth pattern of
    insitu_tiles.  Noise alone leaves channels of the first conv (no zero-mean rows there) without a negative pre-activation."""
    t = np.random.default_rng(seed).integers(0, 256, (B, th, tw, 3), dtype=np.uint8)
    if th >= 8 and tw >= 8:
        h, w = max(8, min(th // 2, 32)), min(tw, 48)
        t[0, :h, :w] = insitu_tiles(seed, 2, h, w)[1]
    return t


# ---- geometry -------------------------------------------------------------------------------------------------------------
def slots(geo, B, th, tw):
    """[(image, y0, x0)] of windows 0 .. B-1 at logical coordinates of the launch images."""
    kx, ky = (geo["mos_kx"], geo["mos_ky"]) if geo["mos_kx"] else (1, 1)
    out = []
    for t in range(B):
        i, slot = divmod(t, kx * ky)
        wy, wx = divmod(slot, kx)
        out.append((i, wy * (th + 1), wx * (tw + 1)))
    return out


def masks(geo, B, th, tw):
    """-> computed [Hm, Wm] (the pixels px_live admits, the same in every launch image), live [n, 1, Hm, Wm] (the pixels of
    windows 0 .. B-1) and the region masks [Hm, Wm] over `computed`."""
    Hm, Wm, H, Wd = geo["Hp"] - 2, geo["Wp"] - 2, geo["H"], geo["W"]
    y = np.arange(Hm)[:, None]
    x = np.arange(Wm)[None, :]
    comp = (y < H) & (x < Wd)
    if geo["mos_kx"]:
        ry, rx = geo["mos_wh"], geo["mos_ww"]
        ly, lx = y % (ry + 1), x % (rx + 1)
        comp = comp & (ly < ry) & (lx < rx)
    else:
        ly, lx, ry, rx = y + 0 * x, x + 0 * y, H, Wd
    edge = (ly == 0) | (ly == ry - 1) | (lx == 0) | (lx == rx - 1)
    img_edge = (y == 0) | (y == H - 1) | (x == 0) | (x == Wd - 1)
    part = comp & (((y >= (H // ROWS) * ROWS) & (H % ROWS != 0)) | ((x >= (Wd // COLS) * COLS) & (Wd % COLS != 0)))
    reg = {"interior": comp & ~edge & ~part, "partial": part & ~edge, "ring": comp & edge & img_edge, "sep": comp & edge & ~img_edge}
    live = np.zeros((geo["n"], 1, Hm, Wm), bool)
    for i, y0, x0 in slots(geo, B, th, tw):
        live[i, 0, y0:y0 + th, x0:x0 + tw] = True
    return comp, live, reg


def px_live_route(geo):
    """Which branch of patch_live / px_live (s2sr_internal.h) a launch with this geometry takes."""
    if not geo["mos_kx"]:
        return "no mosaic"
    return "multiply-high" if geo["mos_wh"] + 1 >= 32 and geo["mos_ww"] + 1 >= 32 else "modulo"


def expected_p0(geo, B, th, tw, tiles=None, x=None):
    """[n, 3, Hp, Wp] fp32: what the packers (csrc/pack.hip) store of the input -- u8: the integers; f32: fp16(fp32(x * 255))."""
    e = np.zeros((geo["n"], 3, geo["Hp"], geo["Wp"]), np.float32)
    if tiles is not None:
        src = np.asarray(tiles, np.uint8).transpose(0, 3, 1, 2).astype(np.float32)
    else:
        src = (np.asarray(x, np.float32) * np.float32(255.0)).astype(np.float16).astype(np.float32)
    for t, (i, y0, x0) in enumerate(slots(geo, B, th, tw)):
        e[i, :, 1 + y0:1 + y0 + th, 1 + x0:1 + x0 + tw] = src[t]
    return e


# ---- the models -------------------------------------------------------------------------------------------------------------
def model_layer(sd, layer, prev):
    """Layer `layer` (0: prev = p0; k: prev = the stored activation k - 1, padded [n, C, Hp, Wp]) -> (v, m, bound): the activation,
    the pre-activation and the bound of |stored - v| per element, at logical coordinates [n, 64, Hp - 2, Wp - 2]."""
    w, b = sd[f"body.{2 * layer}.weight"], sd[f"body.{2 * layer}.bias"]
    slope = sd[f"body.{2 * layer + 1}.weight"].astype(np.float64).reshape(1, -1, 1, 1)
    if layer == 0:
        m, _, tol = tm.model_first(prev, w, False).result(b, scale=1.0 / 255.0)
    else:
        m, _, tol = tm.model_plain64("3x3", np.asarray(prev, np.float64), w).result(b)
    v = np.where(m >= 0, m, slope * m)
    tol = tol + tm.U32 * np.abs(v)                          # the slope multiply
    return v, m, tol + tm.f16_quantum(v) / 2                # the fp16 store


def pixel_shuffle4(y):
    """[n, 16 C, H, W] -> [n, C, 4H, 4W]: channel c*16 + dy*4 + dx to colour c of (4y + dy, 4x + dx) (torch's order)."""
    n, c, H, Wd = y.shape
    return y.reshape(n, c // 16, 4, 4, H, Wd).transpose(0, 1, 4, 2, 5, 3).reshape(n, c // 16, 4 * H, 4 * Wd)


def up4(a):
    return np.repeat(np.repeat(a, 4, axis=-2), 4, axis=-1)


def model_last(act, w_eff, bias, base):
    """The tail: pixel_shuffle(conv(act, w_eff) + bias, 4) + nearest_x4(base).  act padded [n, 64, Hp, Wp]; w_eff [48, 64, 3, 3]
    fp64, the weights as the conv multiplies them (the judge passes fp16(w)); base [n, 3, Hp - 2, Wp - 2] fp64.
    -> (out, bound) [n, 3, 4 (Hp - 2), 4 (Wp - 2)]."""
    y, _, tol = tm.Layer(tm.conv3, tm.n_acc("3x3", 4)).add(np.asarray(act, np.float64), np.asarray(w_eff, np.float64)).result(bias)
    out = pixel_shuffle4(y) + up4(np.asarray(base, np.float64))
    return out, pixel_shuffle4(tol) + tm.U32 * np.abs(out)   # the fp32 add of the base


def base_of(p0):
    """fp32(p0[c] * fp32(1/255)) at logical coordinates, as EPI_CLAST computes it."""
    return (np.asarray(p0, np.float32)[:, :3, 1:-1, 1:-1] * INV255).astype(np.float64)


def quantise_f32(out_f32):
    """[B, 3, H, W] fp32 -> [B, H, W, 3] u8 with the device's arithmetic: trunc(clip(fp32(v * 255), 0, 255))."""
    q = (np.asarray(out_f32, np.float32) * np.float32(255.0)).clip(np.float32(0.0), np.float32(255.0))
    return np.ascontiguousarray(q.astype(np.uint8).transpose(0, 2, 3, 1))


# ---- the judge --------------------------------------------------------------------------------------------------------------
class Report:
    def __init__(self):
        self.rows, self.fails, self.judged = [], [], []

    def fail(self, key, msg):
        self.fails.append((key, msg))

    def keys(self):
        return {k for k, _ in self.fails}

    def worst(self):
        """worst ratio per region over all judged layers"""
        return {r: max([row[r] for row in self.rows if row.get(r) is not None], default=None) for r in REGIONS}

    def text(self, title):
        lines = [f"== {title}: worst |err| / bound per region",
                 f"{'layer':10s} " + " ".join(f"{c:>8s}" for c in REGIONS) + f" {'neg ch':>7s}"]
        for r in self.rows:
            lines.append(f"{r['name']:10s} " + " ".join(f"{r[c]:8.3f}" if r.get(c) is not None else f"{'-':>8s}" for c in REGIONS) +
                         (f" {r['neg']:7d}" if r.get("neg") is not None else f" {'-':>7s}"))
        lines += [f"FAIL {k}: {m}" for k, m in self.fails[:20]]
        return "\n".join(lines)

    def message(self):
        return "\n".join(f"{k}: {m}" for k, m in self.fails[:20])


def _row(name, ratio2d, reg, neg=None):
    """ratio2d [n, Hm, Wm] (zero where nothing is judged)"""
    row = {"name": name, "neg": neg, "worst": float(ratio2d.max()) if ratio2d.size else 0.0}
    for k, m in reg.items():
        M = np.broadcast_to(m, ratio2d.shape)
        row[k] = float(ratio2d[M].max()) if M.any() else None
    return row


def judge(geo, acts, p0, out_f32, out_u8, sd, B, th, tw, tiles=None, x=None, fresh=True, need_negative=True):
    """Judge what the hook returned for a batch of B windows of th x tw (`tiles` [B, th, tw, 3] u8 or `x` [B, 3, th, tw] fp32: the
    input, for the p0 check; neither: p0's live content is not checked).  Every tapped layer whose predecessor is tapped (layer 0:
    p0) is judged, the last conv when acts holds layer num_conv and out_f32 is given, out_u8 when both outputs are given.
    fresh: the engine had run nothing before (a dead slot's p0 is then zero).  need_negative: a judged layer without a negative
    pre-activation in every channel is a failure (its PReLU slopes went untested).  -> Report; asserts nothing."""
    nc = num_conv_of(sd)
    rep = Report()
    comp, live, reg = masks(geo, B, th, tw)
    n, Hm, Wm = geo["n"], geo["Hp"] - 2, geo["Wp"] - 2
    comp_p = np.zeros((Hm + 2, Wm + 2), bool)
    comp_p[1:-1, 1:-1] = comp
    live_p = np.zeros((n, 1, Hm + 2, Wm + 2), bool)
    live_p[:, :, 1:-1, 1:-1] = live
    if (live & ~comp).any():
        rep.fail("geometry", "windows outside the pixels the launch computes")
    # ---- p0
    if p0.shape != (n, 16, Hm + 2, Wm + 2):
        rep.fail("p0", f"shape {p0.shape}")
        return rep
    if p0[:, 3:].any():
        rep.fail("p0", f"{int((p0[:, 3:] != 0).sum())} nonzero values in channels 3..15")
    outside = ~np.broadcast_to(live_p if fresh else comp_p, (n, 3, Hm + 2, Wm + 2))
    if (p0[:, :3] != 0)[outside].any():
        rep.fail("zero p0", f"{int((p0[:, :3] != 0)[outside].sum())} nonzero values outside the {'live' if fresh else 'computed'} pixels")
    if tiles is not None or x is not None:
        want = expected_p0(geo, B, th, tw, tiles, x)
        L3 = np.broadcast_to(live_p, want.shape)
        bad = (np.ascontiguousarray(p0[:, :3]).view(np.uint32) != want.view(np.uint32)) & L3
        if bad.any():
            rep.fail("p0", f"{int(bad.sum())} live values are not the packed input (first at {np.argwhere(bad)[0].tolist()})")
    # ---- zeros outside the computed pixels, every tapped layer
    for k in sorted(acts):
        bad = (acts[k] != 0) & ~comp_p
        if bad.any():
            rep.fail(f"zero layer {k}", f"{int(bad.sum())} stores outside the live pixels (first at {np.argwhere(bad)[0].tolist()})")
    # ---- layers 0 .. num_conv
    C4 = np.broadcast_to(comp, (n, 64, Hm, Wm))
    for k in sorted(acts):
        if k != 0 and (k - 1) not in acts:
            continue
        v, m, bound = model_layer(sd, k, p0 if k == 0 else acts[k - 1])
        neg = ((m < 0) & np.broadcast_to(live, m.shape)).any(axis=(0, 2, 3))
        if need_negative and not neg.all():
            rep.fail(f"negative layer {k}", f"{int((~neg).sum())} channels without negative pre-activations (PReLU untested)")
        got = acts[k][:, :, 1:-1, 1:-1].astype(np.float64)
        ratio = np.where(C4, np.abs(got - v) / bound, 0.0)
        if (ratio > 1).any():
            rep.fail(f"layer {k}", f"off the model by {float(ratio.max()):.3g} x bound at {np.argwhere(ratio == ratio.max())[0].tolist()}")
        rep.rows.append(_row(f"layer {k}", ratio.max(axis=1), reg, int(neg.sum())))
        rep.judged.append(k)
    # ---- the last conv
    if out_f32 is not None and out_f32.shape != (B, 3, 4 * th, 4 * tw):
        rep.fail("last", f"out_f32 shape {out_f32.shape}")
    elif out_f32 is not None and nc in acts:
        last = 2 * nc + 2
        mo, bound = model_last(acts[nc], tm.split(sd[f"body.{last}.weight"])["hi"], sd[f"body.{last}.bias"], base_of(p0))
        got = np.zeros_like(mo)
        for t, (i, y0, x0) in enumerate(slots(geo, B, th, tw)):
            got[i, :, 4 * y0:4 * (y0 + th), 4 * x0:4 * (x0 + tw)] = out_f32[t]
        L = np.broadcast_to(up4(live), mo.shape)
        ratio = np.where(L, np.abs(got - mo) / bound, 0.0)
        if (ratio > 1).any():
            rep.fail("last", f"off the model by {float(ratio.max()):.3g} x bound at {np.argwhere(ratio == ratio.max())[0].tolist()}")
        if not np.isfinite(out_f32).all():
            rep.fail("last", "out_f32 is not finite")
        rep.rows.append(_row("last", ratio.reshape(n, 3, Hm, 4, Wm, 4).max(axis=(1, 3, 5)), reg))
        rep.judged.append(nc + 1)
    # ---- u8 from the device's own fp32
    if out_u8 is not None and out_f32 is not None:
        want = quantise_f32(out_f32)
        if out_u8.shape != want.shape:
            rep.fail("u8", f"out_u8 shape {out_u8.shape}")
        elif not np.array_equal(out_u8, want):
            bad = out_u8 != want
            rep.fail("u8", f"{int(bad.sum())} bytes differ from trunc(clip(out_f32 * 255)) (first at {np.argwhere(bad)[0].tolist()})")
    return rep


# ---- the shape classes tests/test_gpu_compact_insitu.py runs --------------------------------------------------------------------------
# shapes: (entry, B, th, tw, job_windows, environment, all layers)
SHAPES = {
    "tiny_1x16x32": ("u8", 1, 16, 32, 0, {}, True),                 # one patch exactly
    "tile_1x64x64": ("u8", 1, 64, 64, 0, {}, True),
    "ragged_2x37x53": ("u8", 2, 37, 53, 0, {}, True),               # 1 x 2 mosaic, period 38 x 54: the multiply-high route of px_live
    "mosaic_9x20x20": ("u8", 9, 20, 20, 0, {}, True),               # 3 x 3 mosaic, period 21: the modulo route
    "dead_7of9x20x20": ("u8", 7, 20, 20, 9, {}, True),              # the job's 3 x 3 mosaic with two dead slots
    "big_1x300x330": ("u8", 1, 300, 330, 0, {}, False),             # H % 16 and W % 32 nonzero, many patches, no mosaic
    "full_3x256x256": ("u8", 3, 256, 256, 0, {}, False),            # whole tiles: no mosaic
    "aoi_3x276x276": ("u8", 3, 276, 276, 0, {}, False),             # what enhance_u8 launches (tile 256, pad 10): 3 x 1 mosaic, multiply-high
    "mosaic_16x24x40": ("u8", 16, 24, 40, 0, {}, False),            # 2 x 8 mosaic, period 25 x 41: modulo
    "group_16x24x40": ("u8", 16, 24, 40, 0, {"S2SR_MOSAIC": "0"}, False),   # a full default group of 16 images in one launch
    "one_1x1x1": ("u8", 1, 1, 1, 0, {}, True),
    "row_1x1x9": ("u8", 1, 1, 9, 0, {}, True),
    "col_1x7x1": ("u8", 1, 7, 1, 0, {}, True),
    "f32_1x21x27": ("f32", 1, 21, 27, 0, {}, True),                 # the fp32 entry, input off the u8 grid (u8 / 255 + 1e-3)
    "f32_2x37x53": ("f32", 2, 37, 53, 0, {}, True),                 # the fp32 entry never mosaics: two images
    "f32u_2x37x53": ("f32u", 2, 37, 53, 0, {}, True),               # uniform random floats
}
# A judged layer must see a negative pre-activation in every channel (else its slopes went untested).  That is asserted where
# the CPU emulation shows it holds (test_compact_insitu_cpu.test_shape_inputs_reach_every_channel runs the same inputs, the
# large shapes on a corner).  A few pixels cannot drive 64 channels of 17 layers negative, so the degenerate sizes are judged
# without it, and so is the batch of uniform floats (noise alone leaves channels of the first conv positive; the same shape is
# guarded in f32_2x37x53).
NO_NEGATIVE_GUARD = {"one_1x1x1", "row_1x1x9", "col_1x7x1", "f32u_2x37x53"}


def shape_inputs(shape):
    """-> (keyword arguments of debug_compact_taps, keyword arguments of the judge)"""
    kind, B, th, tw, job = SHAPES[shape][:5]
    seed = sum(map(ord, shape))
    rng = np.random.default_rng(seed + 1)
    u8 = structured_tiles(seed, B, th, tw)
    if kind == "u8":
        return dict(tiles=u8, job_windows=job), dict(tiles=u8)
    if kind == "f32":
        x = (u8.transpose(0, 3, 1, 2).astype(np.float32) / 255.0 + 1e-3).clip(0, 1).astype(np.float32)
    else:
        x = rng.random((B, 3, th, tw), dtype=np.float32)
    return dict(x=x), dict(x=x)
