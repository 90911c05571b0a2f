"""Per-layer parity of the six head / tail convs (conv_first, conv_body, conv_up1, conv_up2, conv_hr, conv_last) IN SITU: one
batch through the production forward (s2sr_debug_forward_taps: forward_dev -> run_net with the handle's switches, no graph),
every tensor the tail reads or writes copied out, and each layer recomputed in fp64 by tests/tail_model.py from the STORED
input fields the GPU produced -- so each layer is checked on its own, inside the real schedule (ragged patches, odd source
sizes of the sub-pixel form, mosaic separators and dead slots, batch strides, FULL forms).

What is asserted, per layer and tap:
  * stored fields: hi == fp16(model); lo8 == e4m3(clamp((model - hi) * 2^11)); hi8 == e4m3(clamp(hi)), bit for bit.  The only
    mismatches allowed are elements whose model value lies within the accumulation tolerance of a rounding boundary of that
    field.  They are counted: hi must keep them under 1e-3 of the elements.  lo8 cannot: near lo = 0 its step is 2^-9 * 2^-11
    = 2^-20, below the fp32 accumulator's own rounding at |v| ~ 1, so 0.5-2 % of the lo8 bytes (6 % at the amplitude case)
    legitimately round the other way; each of them must still sit within tol of a boundary, and the rate is printed ("exc").
  * the value the fields carry (hi + lo8, or the f32 output) is within tol + half the field's quantum of the model at every
    live element (tol: tail_model.Layer.result -- n_acc = stages x taps fp32 accumulator roundings of half an ulp of the
    running sum, |acc| + 3 sqrt(sum of squared products), plus two ulps for the epilogue);
  * T8 (conv_body's e4m3 operand planes) bit-exact against the host re-encoding of the trunk's (hi, lo), lo_exp -> 2^11;
  * exact zeros outside the live pixels of every stored tensor (halo, round-up band, mosaic separators);
  * u8 output == trunc(clip(f32 * 255)) of the same run, byte for byte;
  * sensitivity: the hi-only model (correction terms dropped) violates the bound at >= half the elements of every
    split-operand layer -- the check would see a lost correction term.
Printed: a per-layer, per-region table (worst error / bound; interior, last partial patch row / column, image border ring,
pixels next to a mosaic separator, the four (2y+py, 2x+q) parities of the up-convs) and the fidelity columns (GPU and hi-only
model against the fp64 conv of the true operands).
"""
import numpy as np
import pytest

import gpu_engines
import tail_model as tm
from s2sr import native
from s2sr.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

HP, FAST, FP8 = native.PREC_F16_HP, native.PREC_F16, native.PREC_FP8
EXC_MAX = 1e-3      # fraction of elements allowed to differ in a stored field (all of them within tol of a rounding boundary)

# shapes: (entry, B, th, tw, job_windows)
SHAPES = {
    "full_1x16x32": ("u8", 1, 16, 32, 0),       # whole-patch (FULL) forms everywhere
    "ragged_2x37x53": ("u8", 2, 37, 53, 0),     # ragged patches, odd source sizes, batch stride
    "short_3x7x45": ("u8", 3, 7, 45, 0),        # fewer rows than a patch
    "mosaic_9x20x20": ("u8", 9, 20, 20, 0),     # 3 x 3 windows in one launch image
    "dead_7of9x20x20": ("u8", 7, 20, 20, 9),    # the job's 3 x 3 mosaic with two dead slots
    "f32_1x21x27": ("f32", 1, 21, 27, 0),       # the fp32 entry
}


def _engine(monkeypatch, precision, env, gain=1.0):
    sd = synthetic_state_dict(1, seed=0, other_gain=gain)
    return gpu_engines.fresh(monkeypatch, env, 1, precision, sd=sd), sd


def _inputs(shape, seed=0):
    kind, B, th, tw, job = SHAPES[shape]
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (B, th, tw, 3), dtype=np.uint8)
    if kind == "u8":
        return dict(tiles=u8, job_windows=job), B, th, tw
    return dict(x=(u8.transpose(0, 3, 1, 2).astype(np.float32) / 255.0 + 1e-3).clip(0, 1)), B, th, tw


# ---- geometry ------------------------------------------------------------------------------------------------------------
def _regions(geo, k, s, Hm, Wm):
    """Masks [Hm, Wm] at logical coordinates of scale index k (factor s): live pixels and their region classes."""
    H, W = geo["H"][k], geo["W"][k]
    y = np.arange(Hm)[:, None]
    x = np.arange(Wm)[None, :]
    live = (y < H) & (x < W)
    if geo["mos_kx"]:
        py, px = (geo["mos_wh"] + 1) * s, (geo["mos_ww"] + 1) * s
        ry, rx = geo["mos_wh"] * s, geo["mos_ww"] * s
        ly, lx = y % py, x % px
        live = live & (ly < ry) & (lx < rx)
    else:
        ly, lx, ry, rx = y + 0 * x, x + 0 * y, H, W
    edge = (ly == 0) | (ly == ry - 1) | (lx == 0) | (lx == rx - 1)
    img_edge = (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)
    ring = live & edge & img_edge
    sep = live & edge & ~img_edge
    part = live & (((y >= (H // 32) * 32) & (H % 32 != 0)) | ((x >= (W // 32) * 32) & (W % 32 != 0)))
    reg = {"interior": live & ~edge & ~part, "partial": part & ~edge, "ring": ring, "sep": sep}
    return live, reg


def _crop(g, Hm, Wm):
    """padded GPU tensor [n, C, Hp, Wp] -> logical [n, C, Hm, Wm]"""
    return g[:, :, 1:1 + Hm, 1:1 + Wm].astype(np.float64)


def _zero_outside(name, t, live_pad):
    bad = (t != 0) & ~live_pad[None, None]
    assert not bad.any(), f"{name}: {int(bad.sum())} nonzero elements outside the live pixels (first at {np.argwhere(bad)[0].tolist()})"


def _live_padded(geo, k, s, Hp, Wp):
    live, _ = _regions(geo, k, s, Hp - 2, Wp - 2)
    out = np.zeros((Hp, Wp), bool)
    out[1:-1, 1:-1] = live
    return out


# ---- one stored field set ------------------------------------------------------------------------------------------------
def _check_fields(rep, name, hi_g, lo_g, m, h, tol, live, reg, hp, hi8_written, parities=False):
    """hi_g [n,64,Hm,Wm] fp16 values, lo_g [n,128,Hm,Wm] (lo8 * 2^-11 | hi8) or None; m / h / tol the model."""
    L = np.broadcast_to(live[None, None], m.shape)
    ne = int(L.sum())
    exp_hi = tm.f16(m)
    qh = tm.f16_quantum(m)
    near_hi = (qh / 2 - np.abs(m - exp_hi)) <= tol
    mis_hi = (hi_g != exp_hi) & L
    unexpl = mis_hi & ~near_hi
    fails = []
    if unexpl.any():
        fails.append(f"{name} hi: {int(unexpl.sum())} mismatches away from a rounding boundary")
    exc = int(mis_hi.sum())
    bound = tol + qh / 2
    gv = hi_g
    if hp:
        lo8, hi8 = lo_g[:, :64], lo_g[:, 64:]
        r = (m - hi_g) * 2048.0
        exp_lo = tm.e4m3(r) / 2048.0
        rq = tm.e4m3_quantum(np.clip(r, -448, 448))
        near_lo = ((rq / 2 - np.abs(np.clip(r, -448, 448) - tm.e4m3(r))) <= tol * 2048.0) & (np.abs(r) <= 448)
        mis_lo = (lo8 != exp_lo) & L
        if (mis_lo & ~near_lo).any():
            fails.append(f"{name} lo8: {int((mis_lo & ~near_lo).sum())} mismatches away from a rounding boundary "
                         f"(worst |d| {float(np.abs(lo8 - exp_lo)[mis_lo & ~near_lo].max()):.3g})")
        exc_lo = int(mis_lo.sum())   # reported, not capped: see the module docstring
        if hi8_written:
            bad8 = (hi8 != tm.e4m3(hi_g)) & L
            if bad8.any():
                fails.append(f"{name} hi8: {int(bad8.sum())} bytes differ from e4m3(clamp(hi))")
        else:
            if (hi8 != 0).any():
                fails.append(f"{name} hi8: planes that are not written hold nonzero bytes")
        gv = hi_g + lo8
        bound = tol + rq / 4096.0 + np.maximum(np.abs(r) - 448.0, 0) / 2048.0
    if exc > EXC_MAX * ne:
        fails.append(f"{name}: {exc} hi boundary exceptions of {ne} elements")
    if hp:
        exc += exc_lo
    ratio = np.abs(m - gv) / bound
    if (ratio[L] > 1.0).any():
        fails.append(f"{name}: value off the model by {float(ratio[L].max()):.3g} x its bound")
    viol = float((np.abs(h - gv) > bound)[L].mean())
    rep.append(_row(name, ratio, live, reg, viol, exc / max(ne, 1), parities))
    return fails, viol


def _row(name, ratio, live, reg, viol, exc, parities):
    r = {"layer": name, "viol_hi_only": viol, "exc": exc}
    for k, msk in reg.items():
        M = np.broadcast_to(msk[None, None], ratio.shape)
        r[k] = float(ratio[M].max()) if M.any() else None
    if parities:
        for py in range(2):
            for q in range(2):
                M = np.zeros(live.shape, bool)
                M[py::2, q::2] = live[py::2, q::2]
                M = np.broadcast_to(M[None, None], ratio.shape)
                r[f"p{py}{q}"] = float(ratio[M].max()) if M.any() else None
    return r


def _print_table(title, rows, fid):
    cols = ["interior", "partial", "ring", "sep", "p00", "p01", "p10", "p11"]
    print(f"\n== {title}: worst |err| / bound per region; hi-only violation rate; boundary exceptions; fidelity vs fp64 of the true operands")
    print(f"{'layer':10s} " + " ".join(f"{c:>8s}" for c in cols) + f" {'hi-only':>8s} {'exc':>8s} {'gpu_err':>9s} {'hionly_err':>10s}")
    for r in rows:
        f = fid.get(r["layer"], (float("nan"), float("nan")))
        print(f"{r['layer']:10s} " + " ".join(f"{r[c]:8.3f}" if r.get(c) is not None else f"{'-':>8s}" for c in cols) +
              f" {r['viol_hi_only']:8.3f} {r['exc']:8.1e} {f[0]:9.2e} {f[1]:10.2e}")


# ---- the run -------------------------------------------------------------------------------------------------------------
def _run_case(monkeypatch, precision, env, shape, gain=1.0, expect_fail=False):
    e, sd = _engine(monkeypatch, precision, env, gain)
    try:
        cfg = e.debug_config()
        args, B, th, tw = _inputs(shape)
        geo, taps, of32, ou8 = e.debug_forward_taps(**args)
    finally:
        e.close()
    if shape.startswith(("mosaic", "dead")):
        kx, ky = native.pick_mosaic(SHAPES[shape][4] or B, th, tw)
        assert kx * ky > 1 and geo["mos_kx"] * geo["mos_ky"] == kx * ky
        if shape.startswith("dead"):
            assert B < kx * ky and geo["mos_count"] == B
    hp = "T8" in taps
    assert hp == (precision == HP or env.get("S2SR_FP8_TAIL") == "hp")
    upform = "phase"                       # the up-convs run in sub-pixel form
    fold = hp and cfg["last_fold"] == 1
    hi8_u3 = not fold
    W = lambda k: sd[k + ".weight"]
    Bi = lambda k: sd[k + ".bias"]
    # ---- zeros outside the live pixels, every stored tensor
    for name, t in taps.items():
        ch, k = native.TAP_SHAPE[name]
        s = (1, 2, 4)[k]
        _zero_outside(name, t, _live_padded(geo, k, s, t.shape[2], t.shape[3]))
    assert not taps["P0"][:, 3:].any(), "P0: channels 3..15 must be zero"
    rows, fid, fails, viols = [], {}, [], {}
    g1 = (taps["P0"].shape[2] - 2, taps["P0"].shape[3] - 2)
    live1, reg1 = _regions(geo, 0, 1, *g1)
    # ---- conv_first -> F (fp32)
    m, h, tol = tm.model_first(taps["P0"], W("conv_first"), hp).result(Bi("conv_first"), scale=1.0 / 255.0)
    Fg = _crop(taps["F"], *g1)
    L = np.broadcast_to(live1[None, None], m.shape)
    ratio = np.abs(m - Fg) / tol
    if (ratio[L] > 1).any():
        fails.append(f"conv_first: F off the model by {float(ratio[L].max()):.3g} x tol")
    viols["conv_first"] = float((np.abs(h - Fg) > tol)[L].mean())
    rows.append(_row("conv_first", ratio, live1, reg1, viols["conv_first"], 0.0, False))
    tv = tm.true_conv("3x3", taps["P0"][:, :3], W("conv_first")) / 255.0 + Bi("conv_first").reshape(1, -1, 1, 1)
    fid["conv_first"] = (float(np.abs(Fg - tv)[L].max()), float(np.abs(h - tv)[L].max()))
    # ---- T8: bit-exact re-encoding of the trunk
    if precision == FP8:
        assert not taps["TRUNK_LO"].any(), "fp8 trunk: conv_body's lo operand must be zero"
    if hp:
        lo8, hi8 = tm.trunk_planes(taps["TRUNK_HI"].astype(np.float64), taps["TRUNK_LO"].astype(np.float64))
        exp = np.concatenate([lo8, hi8], axis=1)
        bad = taps["T8"] != exp
        assert not bad.any(), f"T8: {int(bad.sum())} bytes differ from the re-encoded trunk (lo_exp {geo['trunk_lo_exp']})"
    # ---- the 64-channel producers
    def producer(name, src, src_lo, w, b, form, skip=None, act=True, k=0, s=1, out=None, out_lo=None, hi8_written=True):
        if hp:
            lay = tm.model_split64(form, src, src_lo[:, :64], src_lo[:, 64:], w)
        else:
            lay = tm.model_plain64(form, src, w)
        m, h, tol = lay.result(b, skip=skip, act=act)
        Hm, Wm = min(m.shape[2], out.shape[2] - 2), min(m.shape[3], out.shape[3] - 2)   # sub-pixel extent vs the 2x planes
        m, h, tol = m[:, :, :Hm, :Wm], h[:, :, :Hm, :Wm], tol[:, :, :Hm, :Wm]
        live, reg = _regions(geo, k, s, Hm, Wm)
        hg = _crop(out, Hm, Wm)
        lg = _crop(out_lo, Hm, Wm) if hp else None
        f, v = _check_fields(rows, name, hg, lg, m, h, tol, live, reg, hp, hi8_written, parities=form != "3x3")
        fails.extend(f)
        viols[name] = v
        xt = src + (src_lo[:, :64] if hp else 0)
        tv = tm.true_conv("3x3" if form == "3x3" else "up3", xt, w)[:, :, :Hm, :Wm] + np.asarray(b, np.float64).reshape(1, -1, 1, 1)
        if skip is not None:
            tv = tv + skip
        if act:
            tv = tm.lrelu(tv)
        Lm = np.broadcast_to(live[None, None], m.shape)
        gv = hg + (lg[:, :64] if hp else 0)
        fid[name] = (float(np.abs(gv - tv)[Lm].max()), float(np.abs(h - tv)[Lm].max()))
        return Hm, Wm

    f64 = lambda a: a.astype(np.float64)
    producer("conv_body", f64(taps["TRUNK_HI"]), f64(taps["T8"]) if hp else None, W("conv_body"), Bi("conv_body"), "3x3",
             skip=Fg, act=False, out=taps["U0"], out_lo=taps.get("U0LO"))
    producer("conv_up1", f64(taps["U0"]), f64(taps["U0LO"]) if hp else None, W("conv_up1"), Bi("conv_up1"), upform,
             k=1, s=2, out=taps["U1"], out_lo=taps.get("U1LO"))
    producer("conv_up2", f64(taps["U1"]), f64(taps["U1LO"]) if hp else None, W("conv_up2"), Bi("conv_up2"), upform,
             k=2, s=4, out=taps["U2"], out_lo=taps.get("U2LO"))
    H4, W4 = producer("conv_hr", f64(taps["U2"]), f64(taps["U2LO"]) if hp else None, W("conv_hr"), Bi("conv_hr"), "3x3",
                      k=2, s=4, out=taps["U3"], out_lo=taps.get("U3LO"), hi8_written=hi8_u3)
    # ---- conv_last -> f32 / u8 outputs
    x3 = f64(taps["U3"])
    if hp:
        lay = tm.model_split64("3x3", x3, f64(taps["U3LO"][:, :64]), f64(taps["U3LO"][:, 64:]), W("conv_last"),
                               stages=6 if fold else 8, fold=fold)
    else:
        lay = tm.model_plain64("3x3", x3, W("conv_last"))
    m, h, tol = lay.result(Bi("conv_last"))
    xt = x3 + (f64(taps["U3LO"][:, :64]) if hp else 0)
    tv = tm.true_conv("3x3", xt, W("conv_last")) + Bi("conv_last").reshape(1, -1, 1, 1).astype(np.float64)
    kx, ky = max(geo["mos_kx"], 1), max(geo["mos_ky"], 1)
    oh, ow = 4 * th, 4 * tw

    def win(a, t):
        n, sl = divmod(t, kx * ky)
        wy, wx = divmod(sl, kx)
        y0, x0 = wy * 4 * (th + 1), wx * 4 * (tw + 1)
        return a[n, :, y0:y0 + oh, x0:x0 + ow]
    r_all, rh_all, tv_err, h_err = [], [], 0.0, 0.0
    for t in range(B):
        mt, ht, tt, vt = win(m, t), win(h, t), win(tol, t), win(tv, t)
        r_all.append(np.abs(mt - of32[t]) / tt)
        rh_all.append(np.abs(ht - of32[t]) > tt)
        tv_err = max(tv_err, float(np.abs(of32[t] - vt).max()))
        h_err = max(h_err, float(np.abs(ht - vt).max()))
    ratio = np.stack(r_all)
    if (ratio > 1).any():
        fails.append(f"conv_last: f32 output off the model by {float(ratio.max()):.3g} x tol")
    viols["conv_last"] = float(np.mean(rh_all))
    ones = np.ones((oh, ow), bool)
    _, regl = _regions({"H": [0, 0, oh], "W": [0, 0, ow], "mos_kx": 0}, 2, 4, oh, ow)
    rows.append(_row("conv_last", ratio, ones, regl, viols["conv_last"], 0.0, False))
    fid["conv_last"] = (tv_err, h_err)
    want_u8 = np.clip(of32.astype(np.float32) * np.float32(255.0), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)
    assert np.array_equal(ou8, want_u8), f"u8 output differs from trunc(clip(f32 * 255)) at {int((ou8 != want_u8).sum())} bytes"
    # ---- report, region coverage, sensitivity
    _print_table(f"{shape} prec={precision} env={env} gain={gain}", rows, fid)
    # every region class this geometry has was checked somewhere in the tail
    for r in rows:
        if r["layer"] in ("conv_up1", "conv_up2"):
            assert all(r[p] is not None for p in ("p00", "p01", "p10", "p11")), r
    seen = {c for r in rows for c in ("interior", "partial", "ring", "sep") if r.get(c) is not None}
    want = {"interior", "ring"} | ({"sep"} if shape.startswith(("mosaic", "dead")) else set()) | ({"partial"} if th % 32 or tw % 32 else set())
    assert want <= seen, (want, seen)
    if expect_fail:
        return fails, viols, fid
    assert not fails, "\n".join(fails)
    if hp:
        for name, v in viols.items():
            print(f"sensitivity {name}: hi-only model violates the bound at {v:.3f} of the elements")
            assert v >= 0.5, (name, v)
    return fails, viols, fid


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tail_hp(monkeypatch, shape):
    _run_case(monkeypatch, HP, {}, shape)


def test_tail_hp_generic_forms(monkeypatch):
    """the same data as the FULL case through the generic (px_live) forms"""
    _run_case(monkeypatch, HP, {"S2SR_F16_FULL": "0"}, "full_1x16x32")


@pytest.mark.parametrize("shape", ["full_1x16x32", "ragged_2x37x53", "mosaic_9x20x20"])
def test_tail_hp_last_8_stages(monkeypatch, shape):
    _run_case(monkeypatch, HP, {"S2SR_LAST_FOLD": "0"}, shape)


@pytest.mark.parametrize("shape", ["full_1x16x32", "ragged_2x37x53", "dead_7of9x20x20"])
def test_tail_fast(monkeypatch, shape):
    _run_case(monkeypatch, FAST, {}, shape)


@pytest.mark.parametrize("shape", ["ragged_2x37x53", "mosaic_9x20x20"])
def test_tail_fp8(monkeypatch, shape):
    _run_case(monkeypatch, FP8, {}, shape)


@pytest.mark.parametrize("shape", ["ragged_2x37x53", "short_3x7x45"])
def test_tail_fp8_hp_tail(monkeypatch, shape):
    _run_case(monkeypatch, FP8, {"S2SR_FP8_TAIL": "hp"}, shape)


def test_tail_hp_amplitude_past_448(monkeypatch):
    """Head / tail weights scaled up until tail activations pass 448, where the hi8 (and lo8) clamps take over: the model
    (clamps included) must still hold.  The fidelity columns record what the clamp costs."""
    fails, viols, fid = _run_case(monkeypatch, HP, {}, "ragged_2x37x53", gain=8.0)


def test_tail_negative_control_no_wlo(monkeypatch):
    """The model without the e4m3 w_lo * 2^11 term of the split-operand convs (the GPU unchanged): the parity check of every
    layer that reads it (conv_body, up1, up2, hr) must fail -- proof that the check sees a lost correction term."""
    split = tm.split

    def no_wlo(w):
        s = split(w)
        s["lo8"] = np.zeros_like(s["lo8"])
        return s
    monkeypatch.setattr(tm, "split", no_wlo)
    fails, _, _ = _run_case(monkeypatch, HP, {}, "ragged_2x37x53", expect_fail=True)
    print("negative control failures:\n" + "\n".join(fails))
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        assert any(f.startswith(name) for f in fails), (name, fails)
