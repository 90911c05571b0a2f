"""Per-RDB parity of the RRDB trunk IN SITU: one batch through the production forward (s2sr_debug_trunk_taps: forward_dev ->
run_net with the handle's weights and switches, no graph), the trunk fields copied out at every RDB boundary of a range, and
every conv recomputed in fp64 by tests/trunk_model.py from the STORED fields it read -- inside the real schedule: the production
weight packs and bias offsets, the D / Tr (fp16) and D8 / Xh (fp8) buffer rotations, the RRDB skip, the entry conversion, and
the kernel forms launch_conv_trunk / launch_conv_trunk_f8 pick for the launch (each launch's form is recorded and printed).

What is asserted, per conv and field:
  * stored fields match the model bit for bit: fp16 hi and growth planes == fp16(model); lo == e4m3(clamp((model - hi) *
    2^lo_exp)); fp8 growth / x planes == e4m3(clamp(model * 2^e)).  The only mismatches allowed sit within the accumulation
    tolerance of a rounding boundary; fewer than EXC_MAX of a case's hi, growth and fp8-plane elements may be such exceptions
    (lo and fp8 Xh exceptions are printed, not capped: see UNCAPPED);
  * the value a field carries (hi + lo, or the e4m3 value) is within tol + half its quantum (+ what a clamp cuts off);
  * the entry conversion bit-exact (fp16 path: conv_first's fp16 lo -> e4m3 at 2^lo_exp; fp8: Xh -> the x planes), and the
    skip a rdb3 reads equals the stored input of its RRDB when that boundary is in the range;
  * every trunk field is exactly zero outside the live pixels (halo ring, round-up band, mosaic separators) at every boundary;
  * the hook's outputs equal forward_batch_u8 / forward_f32 of the same handle byte for byte (the taps do not change the run).
Dead mosaic slots are computed like live windows (px_live does not exclude them): they are checked against the model.
Printed: per case, per conv, the worst |err| / bound per region (interior, last partial patch row / column, image border
ring, pixels next to a mosaic separator) and the exception rates; and the kernel forms the launches took.
"""
import numpy as np
import pytest

import gpu_engines
import trunk_model as tm
from trunk_forms import PRODUCTION_FORMS
from s2sr import native
from s2sr.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

HP, FAST, FP8 = native.PREC_F16_HP, native.PREC_F16, native.PREC_FP8
EXC_MAX = 1e-3      # fraction of the hi / growth / fp8-plane elements of a case allowed to differ (all within tol of a rounding boundary)
# Capped per case and field kind (all the RDBs' fields of that kind together): one 16 x 32 field of 16k elements measured up to
# 1.7e-3 on its own, the kinds together 5-8e-4.  Reported, not capped: the fp16 path's lo (its step near 0 is below the fp32
# accumulator's rounding) and the fp8 path's fp16 Xh (the fp8 MFMA's accumulation, trunk_model.F8_ACC, is as coarse as its step).
UNCAPPED = {"fp16 lo", "fp8 Xh"}
WINO_TOL = 256.0    # the row-Winograd form rounds transformed fp16 operands: its conv1-4 are held to a bound 256x wider (its worst
                    # element measured 247x the fp32-rounding bound; the other fp16 forms stay within 0.12x)

# shapes: (entry, B, th, tw, job_windows)
SHAPES = {
    "tiny_1x16x32": ("u8", 1, 16, 32, 0),
    "tile_1x64x64": ("u8", 1, 64, 64, 0),           # one whole tile: 8x32 patches, FULL=1, two planes per stage
    "ragged_2x37x53": ("u8", 2, 37, 53, 0),         # ragged windows, two per launch image (a mosaic): 8x32 generic form
    "mosaic_9x20x20": ("u8", 9, 20, 20, 0),         # 3 x 3 windows per launch image: 8x32 generic form
    "dead_7of9x20x20": ("u8", 7, 20, 20, 9),        # the job's mosaic with dead slots
    "r16_1x300x330": ("u8", 1, 300, 330, 0),        # 96 <= n32 < 192: 16x32 patches, FULL=3
    "f16_1x320x320": ("u8", 1, 320, 320, 0),        # 16x32 patches, FULL=1
    "m16_9x100x100": ("u8", 9, 100, 100, 0),        # 16x32 patches, generic (mosaic)
    "full_3x256x256": ("u8", 3, 256, 256, 0),       # 32x32 patches, FULL=1; conv5 16x32
    "r32_2x300x330": ("f32", 2, 300, 330, 0),       # 32x32 patches, FULL=3 (the f32 entry: no mosaic)
    "m32_20x100x100": ("u8", 20, 100, 100, 0),      # 5 x 4 windows, n32 208: 32x32 patches, generic (mosaic)
    "aoi_3x276x276": ("u8", 3, 276, 276, 0),        # mosaic of 276-pixel windows (tile 256, pad 10): 32x32 patches, FULL=2
    "f32_1x21x27": ("f32", 1, 21, 27, 0),           # the fp32 entry
}

_SEEN_FORMS = set()


def _key(f):
    return (f["kernel"], f["ct"], f["rows"], f["ring"], f["full"], f["pl"], f["prod"], f["npl"], f["epi"])


def _engine(monkeypatch, precision, env, nb, gain, other_gain=1.0):
    sd = synthetic_state_dict(nb, seed=0, body_gain=gain, other_gain=other_gain)
    return gpu_engines.fresh(monkeypatch, env, nb, precision, sd=sd), sd


def _inputs(shape, seed=0):
    kind, B, th, tw, job = SHAPES[shape]
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (B, th, tw, 3), dtype=np.uint8)
    if kind == "u8":
        return dict(tiles=u8, job_windows=job), u8
    return dict(x=(u8.transpose(0, 3, 1, 2).astype(np.float32) / 255.0 + 1e-3).clip(0, 1)), None


def _regions(geo, Hm, Wm):
    """masks [Hm, Wm] at logical coordinates: live pixels and their region classes"""
    H, W = geo["H"], geo["W"]
    y = np.arange(Hm)[:, None]
    x = np.arange(Wm)[None, :]
    live = (y < H) & (x < W)
    if geo["mos_kx"]:
        py, px, ry, rx = geo["mos_wh"] + 1, geo["mos_ww"] + 1, geo["mos_wh"], geo["mos_ww"]
        ly, lx = y % py, x % px
        live = live & (ly < ry) & (lx < rx)
    else:
        ly, lx, ry, rx = y + 0 * x, x + 0 * y, H, W
    edge = (ly == 0) | (ly == ry - 1) | (lx == 0) | (lx == rx - 1)
    img_edge = (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)
    part = live & (((y >= (H // 32) * 32) & (H % 32 != 0)) | ((x >= (W // 32) * 32) & (W % 32 != 0)))
    reg = {"interior": live & ~edge & ~part, "partial": part & ~edge, "ring": live & edge & img_edge, "sep": live & edge & ~img_edge}
    return live, reg


def _c(a):
    """padded [.., Hp, Wp] -> logical [.., Hp - 2, Wp - 2], fp64"""
    return a[..., 1:-1, 1:-1].astype(np.float64)


class _Report:
    def __init__(self, live, reg):
        self.live, self.reg, self.rows, self.fails = live, reg, [], []
        self.worst, self.agg, self.need = {}, {}, {}

    def finish(self):
        for kind, (e, n) in self.agg.items():
            if e > EXC_MAX * n:
                self.fails.append(f"{kind}: boundary exceptions {e / n:.2e} of the elements")

    def add(self, name, c, capped, kind):
        ex = float(c["exc"].sum()) / max(c["n"], 1)
        if c["bad"].any():
            self.fails.append(f"{name}: {int(c['bad'].sum())} mismatches away from a rounding boundary")
        if capped:
            a = self.agg.setdefault(kind, [0, 0])
            a[0], a[1] = a[0] + int(c["exc"].sum()), a[1] + c["n"]
        r = c["ratio"]
        worst = float(r.max())
        if worst > 1.0:
            self.fails.append(f"{name}: value off the model by {worst:.3g} x its bound")
        row = {"name": name, "exc": ex, "worst": worst}
        for k, m in self.reg.items():
            M = np.broadcast_to(m, r.shape)
            row[k] = float(r[M].max()) if M.any() else None
        self.rows.append(row)
        self.need[kind] = max(self.need.get(kind, 0.0), c["need"])
        w = self.worst.setdefault(kind, [0.0, 0.0])
        w[0], w[1] = max(w[0], worst), max(w[1], ex)

    def print(self, title):
        cols = ["interior", "partial", "ring", "sep"]
        print(f"\n== {title}: worst |err| / bound per region; boundary exception rate")
        print(f"{'field':28s} " + " ".join(f"{c:>8s}" for c in cols) + f" {'exc':>9s}")
        for r in self.rows:
            print(f"{r['name']:28s} " + " ".join(f"{r[c]:8.3f}" if r.get(c) is not None else f"{'-':>8s}" for c in cols) + f" {r['exc']:9.2e}")
        print("per kind (worst ratio, worst exception rate of one field): " + ", ".join(f"{k} {v[0]:.3f} / {v[1]:.1e}" for k, v in sorted(self.worst.items())))
        print("per kind, all fields (exception rate): " + ", ".join(f"{k} {e / max(n, 1):.1e}" for k, (e, n) in sorted(self.agg.items())))
        print("per kind, largest share of the accumulation tolerance an element used: " +
              ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.need.items())))


def _run(monkeypatch, precision, env, shape, nb=1, first=0, count=3, gain=0.3, calibrate=False, forms=None, wino=False, other_gain=1.0):
    e, sd = _engine(monkeypatch, precision, env, nb, gain, other_gain)
    try:
        args, u8 = _inputs(shape)
        if calibrate:
            e.calibrate_fp8(u8)
        geo, F, fl, of32, ou8 = e.debug_trunk_taps(first, count, **args)
        # the taps do not change the run: the same handle's plain forward gives the same bytes
        if SHAPES[shape][4] == 0:
            if u8 is not None:
                assert np.array_equal(e.forward_batch_u8(u8), ou8), "hook u8 output differs from forward_batch_u8"
            else:
                assert np.array_equal(e.forward_f32(args["x"]), of32), "hook f32 output differs from forward_f32"
    finally:
        e.close()
    fp8 = precision == FP8
    assert geo["fp8"] == int(fp8)
    Hm, Wm = F["x_hi"].shape[-2] - 2, F["x_hi"].shape[-1] - 2
    live, reg = _regions(geo, Hm, Wm)
    lp = np.zeros((Hm + 2, Wm + 2), bool)
    lp[1:-1, 1:-1] = live
    # ---- zeros outside the live pixels, every field at every boundary
    for name in ("x_hi", "x_lo", "growth", "skip_hi", "skip_lo"):
        bad = (F[name] != 0) & ~lp
        assert not bad.any(), f"{name}: {int(bad.sum())} nonzero elements outside the live pixels (first at {np.argwhere(bad)[0].tolist()})"
    # ---- entry conversion
    if first == 0:
        if fp8:
            want = tm.enc_e4m3(F["x_hi"][0].astype(np.float64), geo["x_exp"])
        else:
            want = tm.enc_e4m3(F["entry_lo"].astype(np.float64), geo["lo_exp"])
        bad = F["x_lo"][0] != want
        assert not bad.any(), f"entry conversion: {int(bad.sum())} elements differ"
    rep = _Report(live, reg)
    le, xe, ge = geo["lo_exp"], geo["x_exp"], geo["g_exp"]
    for j in range(count):
        g = first + j
        blk, r = divmod(g, 3)
        pre = f"body.{blk}.rdb{r + 1}."
        Wt = lambda k: sd[pre + f"conv{k}.weight"]
        Bi = lambda k: sd[pre + f"conv{k}.bias"]
        xh, xl, gr = F["x_hi"][j].astype(np.float64), F["x_lo"][j].astype(np.float64), F["growth"][j].astype(np.float64)
        xin = xl if fp8 else xh
        for k in range(1, 5):
            m, tol = tm.conv14(xin, gr, k, Wt(k), Bi(k), "f8" if fp8 else "f16")
            st = _c(gr[:, 32 * (k - 1):32 * k])
            c = tm.check_e4m3(st, m, tol, live, ge) if fp8 else tm.check_f16(st, m, tol * (WINO_TOL if wino else 1.0), live)
            kind = "fp8 growth" if fp8 else "fp16 growth"
            rep.add(f"rdb{g} conv{k} x{k}", c, not wino and kind not in UNCAPPED, kind)
        skip = None
        if r == 2:
            sk = F["skip_hi"][j].astype(np.float64) + (0 if fp8 else F["skip_lo"][j].astype(np.float64))
            skip = sk
            if j >= 2:   # the RRDB's input boundary is in the range: the skip is that stored trunk
                assert np.array_equal(F["skip_hi"][j], F["x_hi"][j - 2]), f"rdb{g}: skip hi is not the RRDB's input"
                if not fp8:
                    assert np.array_equal(F["skip_lo"][j], F["x_lo"][j - 2]), f"rdb{g}: skip lo is not the RRDB's input"
        m, tol = tm.conv5(xin, xh if fp8 else xh + xl, gr, Wt(5), Bi(5), "f8" if fp8 else "f16", skip=skip)
        hi_next, lo_next = _c(F["x_hi"][j + 1]), _c(F["x_lo"][j + 1])
        rep.add(f"rdb{g} conv5 {'Xh' if fp8 else 'hi'}", tm.check_f16(hi_next, m, tol, live), not fp8, "fp8 Xh" if fp8 else "fp16 hi")
        if fp8:
            rep.add(f"rdb{g} conv5 x8", tm.check_e4m3(lo_next, m, tol, live, xe), True, "fp8 x planes")
        else:
            rep.add(f"rdb{g} conv5 lo", tm.check_e4m3(lo_next, m - hi_next, tol, live, le), False, "fp16 lo")
    # ---- forms
    for j, f5 in enumerate(fl):
        for k, f in enumerate(f5):
            assert f["kernel"] != 0, f"rdb{first + j} conv{k + 1}: no kernel form recorded"
            _SEEN_FORMS.add(_key(f))
    uniq = sorted({(k + 1 if k < 4 else 5, _key(f)) for f5 in fl for k, f in enumerate(f5)})
    title = (f"{shape} prec={precision} env={env} nb={nb} rdbs=[{first},{first + count}) gain={gain}/{other_gain} lo_exp={le} "
             f"x_exp={xe} g_exp={ge}")
    rep.finish()
    rep.print(title)
    print("forms (conv, (kernel, ct, rows, ring, full, pl, prod, npl, epi)): " + ", ".join(str(u) for u in uniq))
    if forms is not None:
        got = {_key(f) for f5 in fl for f in f5}
        assert forms <= got, (forms, got)
    assert not rep.fails, "\n".join(rep.fails[:20])
    return geo, F


# ---- wiring: every conv of a 23-block net ---------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [HP, FAST, FP8], ids=["hp", "fast", "fp8"])
def test_trunk_wiring_all_69_rdbs(monkeypatch, precision):
    """num_block 23 on a tiny shape, all 69 RDBs tapped: the pack and bias offsets of all 345 convs, the buffer rotations"""
    _run(monkeypatch, precision, {}, "tiny_1x16x32", nb=23, first=0, count=69)


# ---- HP: one case per production conv1-4 form (the form record shows which one ran) ----------------------------------------
_F16_CASES = [   # (shape, forms that must show up, whole RRDB tapped)
    ("tile_1x64x64", {(1, 1, 8, 3, 1, 2, 0, 0, 0), (1, 2, 8, 2, 0, 2, 0, 0, 1), (1, 2, 8, 2, 0, 2, 0, 0, 2)}, True),
    ("ragged_2x37x53", {(1, 1, 8, 7, 0, 1, 0, 0, 0)}, True),
    ("f32_1x21x27", {(1, 1, 8, 3, 3, 2, 0, 0, 0)}, True),
    ("mosaic_9x20x20", {(1, 1, 8, 7, 0, 1, 0, 0, 0)}, True),
    ("dead_7of9x20x20", None, True),
    ("r16_1x300x330", {(1, 1, 16, 5, 3, 1, 0, 0, 0)}, False),
    ("f16_1x320x320", {(1, 1, 16, 5, 1, 1, 0, 0, 0)}, False),
    ("m16_9x100x100", {(1, 1, 16, 5, 0, 1, 0, 0, 0)}, False),
    ("full_3x256x256", {(1, 1, 32, 3, 1, 1, 0, 0, 0), (1, 2, 16, 4, 0, 1, 0, 0, 1), (1, 2, 16, 4, 0, 1, 0, 0, 2)}, True),
    ("r32_2x300x330", {(1, 1, 32, 3, 3, 1, 0, 0, 0)}, False),
    ("m32_20x100x100", {(1, 1, 32, 3, 0, 1, 0, 0, 0)}, False),
    ("aoi_3x276x276", {(1, 1, 32, 3, 2, 1, 0, 0, 0)}, False),
]


@pytest.mark.parametrize("shape,forms,rrdb", _F16_CASES, ids=[c[0] for c in _F16_CASES])
def test_trunk_hp_forms(monkeypatch, shape, forms, rrdb):
    # a whole RRDB (both conv5 epilogues: rdb1 / rdb2 and rdb3 with the skip) on the small shapes and on one big batch (the 16x32
    # conv5 form); the other big shapes tap rdb3 of block 0 only (their conv1-4 form is the point, and the fp64 model is slow)
    _run(monkeypatch, HP, {}, shape, first=0 if rrdb else 2, count=3 if rrdb else 1, forms=forms)


def test_trunk_aoi_window_mosaic_is_the_smallest_full2_job():
    """the 276-pixel-window case is the smallest job whose launch takes the FULL=2 form: fewer windows do not mosaic"""
    assert native.pick_mosaic(3, 276, 276)[0] * native.pick_mosaic(3, 276, 276)[1] > 1
    for b in (1, 2):
        assert native.pick_mosaic(b, 276, 276) == (1, 1)


# ---- edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo_exp", ["6", "18"])
def test_trunk_hp_lo_exp_clamp(monkeypatch, lo_exp):
    """S2SR_LO_EXP at both ends of its range, with the trunk driven to |x| ~ 10-14 (conv_first's weights 8x, body_gain 1.0;
    fp64 oracle on these inputs: 10-28 % of the trunk at |x| >= 4).  The stored lo is v - fp16(v), at most half an fp16 ulp of v,
    so the clamp at 448 * 2^-18 = 1.7e-3 needs |v| >= 4: at lo_exp 18 it must bite (asserted: stored |lo| at the clamp value), and
    the model, clamp included, must still hold.  At lo_exp 6 the clamp sits at 7, out of reach of any fp16 trunk below 2^14: that
    end checks the coarse encoding only."""
    le = int(lo_exp)
    geo, F = _run(monkeypatch, HP, {"S2SR_LO_EXP": lo_exp}, "ragged_2x37x53", nb=2, first=0, count=6, gain=1.0, other_gain=8.0)
    assert geo["lo_exp"] == le
    at = np.abs(F["x_lo"][1:]) == np.float32(np.ldexp(448.0, -le))     # boundaries 1..: lo written by conv5
    print(f"lo_exp {le}: stored lo at the clamp {float(at.mean()):.3e} of the elements")
    if le == 18:
        assert at.mean() > 1e-3, "the conv5 lo clamp did not bite: the case does not test it"


@pytest.mark.parametrize("shape", ["ragged_2x37x53", "full_3x256x256"])
def test_trunk_fast(monkeypatch, shape):   # the big shape: rdb3 of block 0 only (its forms are those of the HP case)
    _run(monkeypatch, FAST, {}, shape, first=0 if shape.startswith("ragged") else 2, count=3 if shape.startswith("ragged") else 1)


def test_trunk_f32_entry(monkeypatch):
    _run(monkeypatch, HP, {}, "f32_1x21x27")


# ---- fp8 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["ragged_2x37x53", "mosaic_9x20x20", "full_3x256x256"])
def test_trunk_fp8(monkeypatch, shape):
    big = shape.startswith("full")
    _run(monkeypatch, FP8, {}, shape, first=2 if big else 0, count=1 if big else 3)


def test_trunk_fp8_saturation(monkeypatch):
    """x / growth scales raised until growth planes saturate at 448: the model's clamp must reproduce the stored bytes"""
    _run(monkeypatch, FP8, {"S2SR_FP8_XEXP": "6", "S2SR_FP8_GEXP": "12"}, "ragged_2x37x53", gain=1.0)


def test_trunk_fp8_saturation_is_reached(monkeypatch):
    e, _ = _engine(monkeypatch, FP8, {"S2SR_FP8_XEXP": "6", "S2SR_FP8_GEXP": "12"}, 1, 1.0)
    try:
        args, _ = _inputs("ragged_2x37x53")
        geo, F, _, _, _ = e.debug_trunk_taps(0, 3, **args)
    finally:
        e.close()
    sat = np.abs(F["growth"]) == np.float32(np.ldexp(448.0, -geo["g_exp"]))
    print(f"saturated growth elements: {float(sat.mean()):.3e}")
    assert sat.any(), "no growth plane reached 448: the saturation case does not test the clamp"


def test_trunk_fp8_calibrated(monkeypatch):
    _run(monkeypatch, FP8, {}, "ragged_2x37x53", calibrate=True)


def test_trunk_forms_cover_the_dispatcher():
    """run last in this module: the union of the recorded forms holds every instantiation the shipped dispatcher picks"""
    if not _SEEN_FORMS:
        pytest.skip("no case of this module ran in this session")
    missing = PRODUCTION_FORMS - _SEEN_FORMS
    print("recorded forms: " + ", ".join(str(f) for f in sorted(_SEEN_FORMS)))
    assert not missing, f"production forms no case reached: {sorted(missing)}"
