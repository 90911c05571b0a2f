"""The in-situ judge of the compact nets (tests/compact_insitu.py) judged itself, without a GPU.  "Taps" are built on the CPU with
the device's number formats (the recipe of compact_model.forward_emulated: fp16 weights and stored activations, fp32
accumulation, bias, slopes and base add) and laid out as s2sr_debug_compact_taps lays them out -- padded planes, a window
mosaic with separators and a dead slot -- under an explicit geometry.  The judge must pass them, and must FAIL each planted fault
(a wrong layer's slopes / bias / weights, a lane-group slip of the slopes, a wrong sub-pixel or colour order in the tail, a wrong
base, a wrong u8 rounding or byte order, a store on a separator or in the round-up band, a store 0.75 fp16 quanta off), each one
flagged at the layer it was planted in and nowhere else: the evidence that the GPU tests would notice a subtly wrong kernel.
Also here: the tail model against the pinned checker, and the weights of the in-situ tests (every channel of every layer sees
negative pre-activations, all slope vectors differ)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import compact_insitu as ci
import compact_model as cm
import tail_model as tm
from s2sr import weights as W

NC = 16


# ---- the hook's layout on the CPU ----------------------------------------------------------------------------------------------
def _roundup32(v):
    return (v + 31) // 32 * 32


def make_geo(B, th, tw, kx=0, ky=0, plan=None):
    """The geometry dict of the hook: B windows as mosaics of kx x ky (0: no mosaic) inside the planes of the job's `plan`
    mosaic (kx, ky; default: the same)."""
    if not kx:
        return dict(n=B, H=th, W=tw, Hp=_roundup32(th) + 2, Wp=_roundup32(tw) + 2, mos_kx=0, mos_ky=0, mos_wh=0, mos_ww=0, mos_count=0)
    pkx, pky = plan or (kx, ky)
    return dict(n=-(-B // (kx * ky)), H=ky * (th + 1) - 1, W=kx * (tw + 1) - 1, Hp=_roundup32(pky * (th + 1) - 1) + 2,
                Wp=_roundup32(pkx * (tw + 1) - 1) + 2, mos_kx=kx, mos_ky=ky, mos_wh=th, mos_ww=tw, mos_count=B)


def _r16(t):
    return t.half().float()


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


def _params(sd, k):
    """(weight, bias, slopes) of layer k; the last conv (k = num_conv + 1) has no slopes"""
    return sd[f"body.{2 * k}.weight"], sd[f"body.{2 * k}.bias"], sd.get(f"body.{2 * k + 1}.weight")


def emu_tail(act, p0, w, b, geo, B, th, tw, inv=ci.INV255, base_shift=0):
    """EPI_CLAST on the CPU: [B, 3, 4 th, 4 tw] fp32 from the stored activation and p0 (padded planes)."""
    y = F.conv2d(_f32(act), _r16(_f32(w)), _f32(b))
    base = _f32(np.roll(p0, base_shift, axis=3)[:, :3, 1:-1, 1:-1]) * torch.tensor(inv, dtype=torch.float32)
    full = (F.pixel_shuffle(y, 4) + F.interpolate(base, scale_factor=4, mode="nearest")).numpy()
    return np.stack([full[i, :, 4 * y0:4 * (y0 + th), 4 * x0:4 * (x0 + tw)] for i, y0, x0 in ci.slots(geo, B, th, tw)])


def emulate(sd, geo, B, th, tw, tiles=None, x=None, params=_params, tamper=None, tail=None):
    """-> (acts {0 .. num_conv}, p0, out_f32, out_u8) in the hook's layout.  params(sd, k): the (weight, bias, slopes) layer k runs
    on; tamper(k, act, prev) -> act: a fault in the stored activation of layer k (later layers read it); tail: keyword
    arguments of emu_tail."""
    nc = ci.num_conv_of(sd)
    comp, _, _ = ci.masks(geo, B, th, tw)
    keep = _f32(comp.astype(np.float32))
    p0 = np.zeros((geo["n"], 16, geo["Hp"], geo["Wp"]), np.float32)
    p0[:, :3] = ci.expected_p0(geo, B, th, tw, tiles, x)
    acts, prev = {}, p0
    for k in range(nc + 1):
        w, b, s = params(sd, k)
        if k == 0:
            y = F.conv2d(_f32(p0[:, :3]), _r16(_f32(w))) * torch.tensor(ci.INV255) + _f32(b).view(1, -1, 1, 1)
        else:
            y = F.conv2d(_f32(prev), _r16(_f32(w)), _f32(b))
        a = F.pad(_r16(F.prelu(y, _f32(s))) * keep, (1, 1, 1, 1)).numpy()
        if tamper is not None:
            a = tamper(k, a, prev)
        acts[k] = prev = a
    w, b, _ = params(sd, nc + 1)
    out = emu_tail(acts[nc], p0, w, b, geo, B, th, tw, **(tail or {}))
    return acts, p0, out, ci.quantise_f32(out)


def _u8(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


GEOS = {                                               # name: (B, th, tw, geo)
    "plain": (1, 16, 32, make_geo(1, 16, 32)),
    "ragged": (2, 21, 37, make_geo(2, 21, 37)),                                        # H % 16 and W % 32 nonzero, two patches
    "mosaic": (4, 9, 11, make_geo(4, 9, 11, 2, 2)),
    "mosaic_dead": (3, 9, 11, make_geo(3, 9, 11, 2, 2)),                               # slot 3 is dead
    "submosaic": (2, 9, 11, make_geo(2, 9, 11, 2, 1, plan=(3, 3))),                    # a remainder row inside the job's planes
}
_SD = {}


def _sd(nc=NC):
    if nc not in _SD:
        _SD[nc] = ci.insitu_sd(nc)
    return _SD[nc]


# ---- (a) the judge passes the emulation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,entry", [(n, "u8") for n in GEOS] + [("plain", "f32"), ("ragged", "f32")])     # the f32 entry never mosaics
def test_judge_passes_the_emulation(name, entry):
    B, th, tw, geo = GEOS[name]
    sd = _sd()
    tiles = _u8(3, B, th, tw, 3)
    kw = dict(tiles=tiles) if entry == "u8" else dict(x=np.random.default_rng(4).random((B, 3, th, tw), dtype=np.float32))
    acts, p0, out, o8 = emulate(sd, geo, B, th, tw, **kw)
    rep = ci.judge(geo, acts, p0, out, o8, sd, B, th, tw, need_negative=False, **kw)
    print(rep.text(f"{name} {entry}"))
    assert rep.judged == list(range(NC + 2)) and not rep.fails, rep.message()
    if name.startswith("mosaic"):
        assert rep.rows[3]["sep"] is not None and rep.rows[-1]["sep"] is not None
    if name == "ragged":
        assert rep.rows[3]["partial"] is not None
    # eight taps with a gap: only layers with a tapped predecessor are judged
    sub = {k: acts[k] for k in (0, 1, 4, 5, 6, 9, 15, 16)}
    rep = ci.judge(geo, sub, p0, out, o8, sd, B, th, tw, need_negative=False, **kw)
    assert rep.judged == [0, 1, 5, 6, 16, 17] and not rep.fails, rep.message()
    rep = ci.judge(geo, {k: acts[k] for k in (3, 4)}, p0, out, None, sd, B, th, tw, need_negative=False, **kw)
    assert rep.judged == [4] and not rep.fails


def test_dead_slot_is_judged_like_a_live_window():
    B, th, tw, geo = GEOS["mosaic_dead"]
    sd = _sd()
    tiles = _u8(5, B, th, tw, 3)
    acts, p0, out, o8 = emulate(sd, geo, B, th, tw, tiles=tiles)
    comp, live, _ = ci.masks(geo, B, th, tw)
    dead = comp & ~live[0, 0]
    assert dead.sum() == th * tw and acts[5][0, :, 1:-1, 1:-1][:, dead].any()          # the dead slot holds prelu(bias) and what follows
    a = {k: v.copy() for k, v in acts.items()}
    y, x = np.argwhere(dead)[7]
    a[5][0, 9, y + 1, x + 1] *= 1.01
    rep = ci.judge(geo, a, p0, out, o8, sd, B, th, tw, tiles=tiles, need_negative=False)
    assert rep.keys() >= {"layer 5"}
    p = p0.copy()                                     # a stale input pixel in the dead slot: a failure on a fresh engine only
    p[0, 1, y + 1, x + 1] = 7.0
    acts2, _, out2, o82 = emulate(sd, geo, B, th, tw, tiles=tiles)
    assert ci.judge(geo, acts2, p, out2, o82, sd, B, th, tw, tiles=tiles, need_negative=False).keys() >= {"zero p0"}
    assert "zero p0" not in ci.judge(geo, acts2, p, out2, o82, sd, B, th, tw, tiles=tiles, need_negative=False, fresh=False).keys()


# ---- (b) planted faults ----------------------------------------------------------------------------------------------------------------
K = 6                        # the body conv the layer faults are planted in


def _with(k, f):
    """params: layer k runs on f(sd) instead of its own (weight, bias, slopes)"""
    def params(sd, layer):
        w, b, s = _params(sd, layer)
        return f(sd, w, b, s) if layer == k else (w, b, s)
    return params


def _dydx(a):
    """48 rows as if dy and dx were exchanged: row c*16 + dy*4 + dx takes row c*16 + dx*4 + dy"""
    return np.ascontiguousarray(a.reshape((3, 4, 4) + a.shape[1:]).swapaxes(1, 2).reshape(a.shape))


def _rgb(a):
    return np.ascontiguousarray(a.reshape((3, 16) + a.shape[1:])[::-1].reshape(a.shape))


def _off_model(quanta, layer=K):
    """tamper: one element of layer `layer` stored `quanta` fp16 quanta off the judge's own model value -- the element where the
    accumulation tolerance is smallest against the quantum"""
    def tamper(k, a, prev):
        if k != layer:
            return a
        v, _, bound = ci.model_layer(_sd(), k, prev)
        q = tm.f16_quantum(v)
        B, th, tw, geo = GEOS["mosaic_dead"]
        _, live, _ = ci.masks(geo, B, th, tw)
        score = np.where(np.broadcast_to(live, v.shape), (bound - q / 2) / q, np.inf)
        i = np.unravel_index(np.argmin(score), score.shape)
        assert score[i] < 0.2, "no element whose accumulation tolerance is below a fifth of its fp16 quantum"
        a = a.astype(np.float64)
        a[i[0], i[1], i[2] + 1, i[3] + 1] = v[i] + quanta * q[i]
        return a.astype(np.float32)
    return tamper


def _poke(layer, where):
    def tamper(k, a, prev):
        if k == layer:
            a = a.copy()
            a[(0, 13) + where] = 0.25
        return a
    return tamper


def _swap_bytes(o8):
    o = o8.copy()
    run = o[1, 5, 8:12].reshape(-1)                   # the 12 bytes of LR pixel (1, 2) of window 1, HR row 5
    j = int(np.argmax(run[1:] != run[0])) + 1
    assert run[j] != run[0]
    run[0], run[j] = run[j], run[0]
    o[1, 5, 8:12] = run.reshape(4, 3)
    return o


# name: (emulate keywords, post-processing of (acts, p0, out, o8), the keys the judge must report -- exactly)
FAULTS = {
    "slopes of layer k+1": (dict(params=_with(K, lambda sd, w, b, s: (w, b, _params(sd, K + 1)[2]))), None, {f"layer {K}"}),
    "bias of layer k+1": (dict(params=_with(K, lambda sd, w, b, s: (w, _params(sd, K + 1)[1], s))), None, {f"layer {K}"}),
    "weights rolled by one output channel": (dict(params=_with(K, lambda sd, w, b, s: (np.roll(w, 1, axis=0), b, s))), None, {f"layer {K}"}),
    "slopes off by 4 channels": (dict(params=_with(K, lambda sd, w, b, s: (w, b, np.roll(s, 4)))), None, {f"layer {K}"}),
    "slopes of layer 1 at layer 0": (dict(params=_with(0, lambda sd, w, b, s: (w, b, _params(sd, 1)[2]))), None, {"layer 0"}),
    "last conv dy / dx exchanged": (dict(params=_with(NC + 1, lambda sd, w, b, s: (_dydx(w), _dydx(b), s))), None, {"last"}),
    "last conv weight rows dy / dx exchanged, bias right": (dict(params=_with(NC + 1, lambda sd, w, b, s: (_dydx(w), b, s))), None, {"last"}),
    "colour planes 0 and 2 exchanged": (dict(params=_with(NC + 1, lambda sd, w, b, s: (_rgb(w), _rgb(b), s))), None, {"last"}),
    "base from fp16(1/255)": (dict(tail=dict(inv=np.float32(np.float16(1.0 / 255.0)))), None, {"last"}),
    "base of the pixel to the left": (dict(tail=dict(base_shift=1)), None, {"last"}),
    "u8 rounded to nearest": ({}, lambda a, p, o, o8: (a, p, o, _rint_u8(o)), {"u8"}),
    "two bytes of a 12-byte run exchanged": ({}, lambda a, p, o, o8: (a, p, o, _swap_bytes(o8)), {"u8"}),
    "a value on a separator": (dict(tamper=_poke(K, (1 + 9, 1 + 4))), None, {f"zero layer {K}"}),
    "a value on the separator column": (dict(tamper=_poke(K, (1 + 3, 1 + 11))), None, {f"zero layer {K}"}),
    "a stale value in the round-up band": (dict(tamper=_poke(K, (1 + 25, 1 + 6))), None, {f"zero layer {K}"}),
    "a stale value in the halo ring": (dict(tamper=_poke(K, (0, 5))), None, {f"zero layer {K}"}),
    "a store 0.75 fp16 quanta off": (dict(tamper=_off_model(0.75)), None, {f"layer {K}"}),
    "a store 0.25 fp16 quanta off (inside the bound)": (dict(tamper=_off_model(0.25)), None, set()),
    "a store -0.25 fp16 quanta off (inside the bound)": (dict(tamper=_off_model(-0.25)), None, set()),
    "an input pixel one level off": ({}, lambda a, p, o, o8: (a, _bump(p), o, o8), {"p0", "layer 0", "last"}),
    "a value in p0 channel 3": ({}, lambda a, p, o, o8: (a, _ch3(p), o, o8), {"p0"}),
}


def _rint_u8(out_f32):
    return np.rint((out_f32 * np.float32(255)).clip(0, 255)).astype(np.uint8).transpose(0, 2, 3, 1)


def _bump(p0):
    p = p0.copy()
    p[0, 1, 1 + 4, 1 + 5] += 1.0
    return p


def _ch3(p0):
    p = p0.copy()
    p[0, 3, 1 + 4, 1 + 5] = 1.0
    return p


@pytest.mark.parametrize("fault", list(FAULTS))
def test_judge_catches(fault):
    kw, post, want = FAULTS[fault]
    B, th, tw, geo = GEOS["mosaic_dead"]
    sd = _sd()
    tiles = ci.insitu_tiles(11, B, th, tw)
    res = emulate(sd, geo, B, th, tw, tiles=tiles, **kw)
    if post:
        res = post(*res)
    rep = ci.judge(geo, *res, sd, B, th, tw, tiles=tiles, need_negative=False)
    worst = {r["name"]: r["worst"] for r in rep.rows}
    print(f"{fault}: {'caught as ' + ', '.join(sorted(rep.keys())) if rep.fails else 'passes'}"
          f" (worst ratio {max(worst.values()):.3g} at {max(worst, key=worst.get)})")
    assert rep.keys() == want, rep.message()


def test_f32_entry_p0_is_held_bit_for_bit():
    B, th, tw, geo = GEOS["ragged"]
    sd = _sd()
    x = np.random.default_rng(8).random((B, 3, th, tw), dtype=np.float32)
    acts, p0, out, o8 = emulate(sd, geo, B, th, tw, x=x)
    lv = p0[:, :3, 1:1 + th, 1:1 + tw]
    assert (lv != np.rint(lv)).mean() > 0.4                                            # off the u8 grid
    p = p0.copy()
    i = np.unravel_index(np.argmax(p[:, :3]), p[:, :3].shape)
    p[i] = np.nextafter(np.float16(p[i]), np.float16(0)).astype(np.float32)            # one fp16 step: fp16(trunc) instead of round
    a2, _, out2, o82 = emulate(sd, geo, B, th, tw, x=x)
    assert "p0" in ci.judge(geo, a2, p, out2, o82, sd, B, th, tw, x=x, need_negative=False).keys()


def test_missing_negative_pre_activations_are_reported():
    B, th, tw, geo = 1, 1, 1, make_geo(1, 1, 1)
    sd = _sd()
    tiles = _u8(1, 1, 1, 1, 3)
    res = emulate(sd, geo, B, th, tw, tiles=tiles)
    rep = ci.judge(geo, *res, sd, B, th, tw, tiles=tiles)
    assert any(k.startswith("negative layer") for k in rep.keys())                      # one pixel cannot drive 64 channels negative
    assert all(k.startswith("negative layer") for k in rep.keys()), rep.message()
    assert not ci.judge(geo, *res, sd, B, th, tw, tiles=tiles, need_negative=False).fails


# ---- the tail model against the pinned checker ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [16, 32])
def test_tail_model_reproduces_the_checker(golden_dir, nc):
    """compact_model.layer for layers 0 .. num_conv, then the judge's model_last with the raw float64 weights and the input itself
    as the base == compact_model.forward (float64) on the g10 golden's input, to 1e-12: the sub-pixel order, the base placement
    and the conv of the new model are the pinned checker's."""
    g = np.load(golden_dir / "g10_compact.npz")
    sd = W.synthetic_compact_state_dict(nc, seed=0)
    x = torch.from_numpy(g["net_u8"]).permute(0, 3, 1, 2).double() / 255.0
    h = x
    for i in range(nc + 1):
        h = cm.layer(h, sd, i)
    last = 2 * nc + 2
    out, bound = ci.model_last(F.pad(h, (1, 1, 1, 1)).numpy(), sd[f"body.{last}.weight"].astype(np.float64), sd[f"body.{last}.bias"], x.numpy())
    ref = cm.forward(x, sd).numpy()
    assert out.shape == ref.shape and float(np.abs(out - ref).max()) <= 1e-12
    assert float(np.abs(ref - g[f"net_c{nc}"]).max()) <= 1e-6
    assert bound.shape == out.shape and (bound > 0).all() and float(bound.max()) < 1e-4   # fp32-accumulation class, far below TOL


# ---- the weights and inputs of the in-situ tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,B,th,tw", [(32, 2, 40, 56), (16, 5, 37, 45)])
def test_insitu_weights_reach_every_channel(nc, B, th, tw):
    """float32 emulation of the two batches of test_gpu_compact.test_layers_in_situ: every one of the 64 channels has a negative
    pre-activation at every layer 0 .. num_conv, so every PReLU slope is exercised; and no two layers share a slope vector, a bias
    or a weight row closely enough for a swap to hide below a quantum."""
    for depth in (16, 32):
        sd = ci.insitu_sd(depth)
        x = _f32(ci.insitu_tiles(nc + B, B, th, tw).transpose(0, 3, 1, 2))
        h = None
        for k in range(depth + 1):
            w, b, s = _params(sd, k)
            if k == 0:
                y = F.conv2d(x, _r16(_f32(w)), None, padding=1) * torch.tensor(ci.INV255) + _f32(b).view(1, -1, 1, 1)
            else:
                y = F.conv2d(h, _r16(_f32(w)), _f32(b), padding=1)
            assert bool((y < 0).flatten(2).any(dim=2).any(dim=0).all()), f"num_conv {depth} layer {k}: a channel without negative pre-activations"
            h = _r16(F.prelu(y, _f32(s)))
        slopes = np.stack([sd[f"body.{2 * k + 1}.weight"] for k in range(depth + 1)])
        assert slopes.min() >= 0.05 and slopes.max() <= 0.35
        d = np.abs(slopes[:, None] - slopes[None]).max(axis=2) + np.eye(depth + 1)
        assert d.min() > 0.1, "two layers with nearly the same slope vector"
        assert np.abs(slopes - np.roll(slopes, 4, axis=1)).max(axis=1).min() > 0.1


def _negative_everywhere(sd, x, margin=0):
    """float32 emulation of layers 0 .. num_conv on x [B, 3, H, W] (values as packed): -> the first layer with a channel that has
    no negative pre-activation, or None.  margin: pixels at the bottom / right that are left out (a crop's inexact border)."""
    h, depth = None, ci.num_conv_of(sd)
    for k in range(depth + 1):
        w, b, s = _params(sd, k)
        if k == 0:
            y = F.conv2d(x, _r16(_f32(w)), None, padding=1) * torch.tensor(ci.INV255) + _f32(b).view(1, -1, 1, 1)
        else:
            y = F.conv2d(h, _r16(_f32(w)), _f32(b), padding=1)
        yy = y[:, :, :y.shape[2] - margin, :y.shape[3] - margin]
        if not bool((yy < 0).flatten(2).any(dim=2).any(dim=0).all()):
            return k
        h = _r16(F.prelu(y, _f32(s)))
    return None


def test_shape_inputs_reach_every_channel():
    """The inputs of compact_insitu.SHAPES on which the GPU test demands negative pre-activations in every channel of every
    judged layer do have them (float32 emulation; windows of a mosaic are independent images).  Shapes above 96 x 96 are run on the
    top-left 96 x 96 of their windows and counted on its 63 x 63 corner, which 33 convs from the cut cannot reach."""
    for shape, (kind, B, th, tw, job, env, every) in ci.SHAPES.items():
        if shape in ci.NO_NEGATIVE_GUARD:
            continue
        _, kw = ci.shape_inputs(shape)
        if "tiles" in kw:
            x = _f32(kw["tiles"].transpose(0, 3, 1, 2))
        else:
            x = _f32(ci.expected_p0(make_geo(B, th, tw), B, th, tw, x=kw["x"])[:, :, 1:1 + th, 1:1 + tw])
        margin = 0
        if th > 96 and tw > 96:
            x, margin = x[:, :, :96, :96], 33
        bad = _negative_everywhere(ci.insitu_sd(16 if every else 32), x, margin)
        assert bad is None, f"{shape}: layer {bad} has a channel without negative pre-activations"


def test_f32_packing_rounding_on_and_off_the_u8_grid():
    """The f32 entries store fp16(fp32(255 x)): the product rounded to fp32, then to fp16 (csrc/pack.hip pins it; a fused multiply
    and convert rounds the exact product once).  On the u8 grid (x = fp32(u / 255), what every RRDB test and golden feeds) both
    roundings give u exactly, so pinning it moves no RRDB output; off the grid they differ at ties of the fp32 product, as for
    the value the device test met."""
    u = np.arange(256)
    x = (u.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    twice = (x * np.float32(255.0)).astype(np.float16)
    once = (x.astype(np.float64) * 255.0).astype(np.float16)
    assert np.array_equal(twice.astype(np.float64), u) and np.array_equal(once.astype(np.float64), u)
    x = np.array([0.21868873], np.float32)
    assert float((x * np.float32(255.0)).astype(np.float16)[0]) == 55.75 and float((x.astype(np.float64) * 255.0).astype(np.float16)[0]) == 55.78125
    geo = make_geo(1, 1, 1)
    assert ci.expected_p0(geo, 1, 1, 1, x=np.broadcast_to(x.reshape(1, 1, 1, 1), (1, 3, 1, 1)))[0, 0, 1, 1] == 55.75
