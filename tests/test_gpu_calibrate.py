"""s2sr_calibrate_fp8 against the tensors it reduces.

The call runs the calibration tiles through the production forward with the measuring pass's scales (x 2^0, growth 2^2), takes the
largest |x| of the fp16 trunk (absmax_f16_kernel) and the largest |x_k| of the e4m3 growth planes (absmax_e4m3_kernel, its own
decoder) over every RDB boundary and every launch image, measures a kind again 8x wider when it reaches the pass's ceiling, and turns
each maximum m into floor(log2(448 / (m * headroom))).  s2sr_debug_trunk_taps returns exactly those tensors of the same forward, so
the reference here is exact: a second handle created with the measuring pass's scales, never calibrated, tapped at every boundary,
the maxima taken in numpy, the ladder followed on fresh handles.

The call returns exponents, not maxima.  Each maximum is pinned by a pair of headrooms around its own boundary: with
k = floor(log2(448 / m)) and hb = 448 / (m 2^k) in [1, 2), headroom hb (1 - EPS) must give k and hb (1 + EPS) must give k - 1
(hb (1 - EPS) < 1: 2 hb and k - 1, k - 2).  A measured maximum that is off by more than EPS = 2^-9, relatively, fails one side: an
fp16 maximum is exact, an e4m3 step is 2^-4, and a maximum over the wrong planes, the first launch image only or a mis-decoded
binade is off by far more (the conditions that make this so are asserted per case: _assert_sensitive).

Every test prints the tapped maxima, boundary 0's own maximum and the exponents it got before it asserts.
"""
import numpy as np
import pytest

import gpu_engines
from s2sr import native
from s2sr.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

FP8 = native.PREC_FP8
EPS = 2.0 ** -9
MEASURE_X, MEASURE_G = 0, 2          # the measuring pass's first scales (s2sr_calibrate_fp8: mx = 0, mg = 2)
F32 = np.float32

# conv_first.weight / .bias times these.  The trunk is positively homogeneous up to the body's 0.01 biases, so its maxima follow
# the factor.  An fp64 model of the seeded one-block trunk on the 3 x 64 x 64 tiles gives m_x 1.53 (boundary 0: 1.27) and m_g 0.32;
# the tests assert, from the taps, the conditions each factor is chosen for (pass counts, finite fp16 values).
LADDER_FACTOR = 512.0      # m_x ~ 780 in [439, 3512), m_g ~ 163 in [110, 878): both kinds need the second pass (2^-3 / 2^-1), not the third
                           # (m_x / m_g ~ 4.7 with these weights, so growth cannot reach its ceiling without x reaching its own)
REFUSE_FACTOR = 24576.0    # m_x ~ 37500: at the third pass's ceiling for x (>= 0.98 * 28672), below fp16's 65504; m_g ~ 7850 >= 0.98 * 7168


def _tiles(B, th, tw, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, th, tw, 3), dtype=np.uint8)


def _hot_tiles(hot):
    """three 64 x 64 tiles: one full-range tile in slot `hot`, the others the same tile at an eighth of its range"""
    t = _tiles(1, 64, 64, 5)[0]
    out = np.stack([t // 8] * 3)
    out[hot] = t
    return out


def _sd(nb, first_gain=1.0, late_gain=1.0):
    sd = synthetic_state_dict(nb, seed=0)
    for k in ("conv_first.weight", "conv_first.bias"):
        sd[k] = sd[k] * F32(first_gain)
    for k in ("body.0.rdb2.conv4.weight", "body.0.rdb2.conv4.bias"):      # late_gain: the last growth conv of one RDB louder (CASES)
        sd[k] = sd[k] * F32(late_gain)
    return sd


# name -> (num_block, conv_first factor, conv4 factor, tiles, launch images n, index of the image that must hold both maxima or None)
CASES = {
    "n3_3x64x64": (1, 1.0, 1.0, lambda: _tiles(3, 64, 64, 0), 3, None),        # three launch images: the per-image loop of the growth max
    "ragged_2x37x53": (1, 1.0, 1.0, lambda: _tiles(2, 37, 53, 1), 1, None),    # ragged two-window mosaic, one launch image
    "mosaic_9x20x20": (1, 1.0, 1.0, lambda: _tiles(9, 20, 20, 2), 1, None),    # 3 x 3 mosaic with separators
    "hot1_3x64x64": (1, 8.0, 1.0, lambda: _hot_tiles(1), 3, 1),                # a maximum only launch image 1 reaches
    "hot2_3x64x64": (1, 8.0, 1.0, lambda: _hot_tiles(2), 3, 2),                # ... only launch image 2
    "nb2_3x64x64": (2, 1.0, 1.0, lambda: _tiles(3, 64, 64, 3), 3, None),       # six RDBs accumulate into the same two floats
    # the seeded weights put the growth maximum into x1 of every case above (x1 .. x4: 0.32, 0.20, 0.19, 0.14), so a max over the
    # first two growth planes only would pass them all: rdb2's conv4 times 4 moves the maximum into x4 (asserted)
    "late_3x64x64": (1, 1.0, 4.0, lambda: _tiles(3, 64, 64, 0), 3, None),
    "ladder_3x64x64": (1, LADDER_FACTOR, 1.0, lambda: _tiles(3, 64, 64, 0), 3, None),   # both maxima reach the first pass's ceiling, not the second's
}

_REF = {}


def _tap(monkeypatch, sd, nb, tiles, xe, ge):
    """maxima of one uncalibrated forward at scales 2^xe / 2^ge, from the trunk taps of a handle of its own"""
    e = gpu_engines.fresh(monkeypatch, {"S2SR_FP8_XEXP": str(xe), "S2SR_FP8_GEXP": str(ge)}, nb, FP8, sd=sd)
    try:
        cfg = e.debug_config()
        assert (cfg["fp8_x_exp"], cfg["fp8_g_exp"]) == (xe, ge)
        geo, F, _, _, _ = e.debug_trunk_taps(0, 3 * nb, tiles=tiles)
    finally:
        e.close()
    assert (geo["x_exp"], geo["g_exp"]) == (xe, ge)
    ax, ag = np.abs(F["x_hi"]), np.abs(F["growth"])
    assert np.isfinite(ax).all() and np.isfinite(ag).all(), "inf / NaN in the trunk: the case's factor is wrong"
    return {"n": geo["n"], "xe": xe, "ge": ge, "m_x": F32(ax.max()), "m_g": F32(ag.max()), "b0": F32(ax[0].max()),
            "x_img": ax.max(axis=(0, 2, 3, 4)), "g_img": ag.max(axis=(0, 2, 3, 4)),
            "x_bnd": ax.max(axis=(1, 2, 3, 4)),
            "g_conv": ag.reshape(ag.shape[0], ag.shape[1], 4, 32, -1).max(axis=(0, 1, 3, 4))}     # x1 .. x4


def _ceiling(m, e):
    """s2sr_calibrate_fp8's "this maximum reached the pass's ceiling" rule, in float32 as the product evaluates it"""
    return F32(m) >= F32(0.98) * F32(np.ldexp(448.0, -e))


def reference(monkeypatch, nb, gain, tiles, late=1.0):
    """the product's ladder on tapped maxima -> (passes, clipped): passes = the tapped maxima of each measuring pass"""
    sd = _sd(nb, gain, late)
    mx, mg, passes = MEASURE_X, MEASURE_G, []
    for attempt in range(3):
        t = _tap(monkeypatch, sd, nb, tiles, mx, mg)
        passes.append(t)
        cx, cg = _ceiling(t["m_x"], mx), _ceiling(t["m_g"], mg)
        if not (cx or cg) or attempt == 2:
            return passes, bool(cx or cg)
        mx, mg = mx - 3 * int(cx), mg - 3 * int(cg)


def _ref(monkeypatch, name):
    if name not in _REF:
        nb, gain, late, mk, n, hot = CASES[name]
        tiles = mk()
        passes, clipped = reference(monkeypatch, nb, gain, tiles, late)
        _REF[name] = (tiles, passes, clipped)
        for t in passes:
            print(f"{name}: pass at 2^{t['xe']} / 2^{t['ge']}: m_x {t['m_x']:.6g} (boundary 0 alone {t['b0']:.6g}, {t['b0'] / t['m_x']:.3f} of it; "
                  f"per boundary {np.array2string(t['x_bnd'], precision=4)}), m_g {t['m_g']:.6g}; per image x {np.array2string(t['x_img'], precision=4)} "
                  f"g {np.array2string(t['g_img'], precision=4)}; growth per conv x1..x4 {np.array2string(t['g_conv'], precision=4)}")
    return _REF[name]


def pick(m, headroom):
    """s2sr_calibrate_fp8's `pick`, in float32"""
    k = int(np.floor(np.log2(F32(448.0) / (F32(m) * F32(headroom)))))
    return max(-8, min(12, k))


def near_power_of_two(m, headroom):
    """448 / (m headroom) less than EPS away, relatively, from a power of two: floor(log2) may fall either way"""
    r = 448.0 / (float(F32(m)) * float(F32(headroom)))
    f = r / 2.0 ** np.floor(np.log2(r))          # [1, 2)
    return f < 1.0 + EPS or f > 2.0 * (1.0 - EPS)


def bracket(m):
    """-> [(headroom, expected exponent)] at both sides of the boundary of maximum m"""
    m = float(F32(m))
    k = int(np.floor(np.log2(448.0 / m)))
    hb = 448.0 / (m * 2.0 ** k)
    assert 1.0 <= hb < 2.0
    if hb * (1.0 - EPS) < 1.0:
        k, hb = k - 1, 2.0 * hb
    assert -8 < k - 1 and k < 12, "the clamp of the exponent would hide the bracket"
    return [(hb * (1.0 - EPS), k), (hb * (1.0 + EPS), k - 1)]


def _assert_sensitive(name, t):
    """what makes a wrong reduction fail a bracket in this case (conditions of the case, not measurements of the product)"""
    n, hot = CASES[name][4], CASES[name][5]
    assert t["n"] == n, (t["n"], n)
    if name.startswith("late"):     # the growth maximum sits in the planes of x3 / x4: a max over x1 / x2 only is low
        assert t["g_conv"][:2].max() * (1.0 + 4.0 * EPS) < t["g_conv"][2:].max() == t["m_g"], t["g_conv"]
    if hot is not None:     # every other launch image stays clear of both maxima: a max over image 0 only, or one that skips an image, is low
        for kind, per, m in (("x", t["x_img"], t["m_x"]), ("growth", t["g_img"], t["m_g"])):
            assert int(np.argmax(per)) == hot, (kind, per)
            others = np.delete(per, hot).max()
            assert others * (1.0 + 4.0 * EPS) < m, f"{kind}: another launch image comes within {4 * EPS:.1e} of image {hot}'s maximum"


@pytest.mark.parametrize("name", list(CASES))
def test_exponents_bracket_the_tapped_maxima(monkeypatch, name):
    nb, gain, late = CASES[name][:3]
    tiles, passes, clipped = _ref(monkeypatch, name)
    assert not clipped, "the reference ladder ends at its ceiling: this case belongs to the refusal test"
    t = passes[-1]
    if name.startswith("ladder"):
        assert len(passes) == 2 and t["ge"] == MEASURE_G - 3, \
            f"the factor does not drive the ladder's second pass for growth alone: {[(p['xe'], p['ge'], p['m_x'], p['m_g']) for p in passes]}"
    else:
        assert len(passes) == 1
    _assert_sensitive(name, t)
    e = gpu_engines.fresh(monkeypatch, {}, nb, FP8, sd=_sd(nb, gain, late))
    try:
        for kind, m, other in (("x", t["m_x"], t["m_g"]), ("growth", t["m_g"], t["m_x"])):
            for headroom, want in bracket(m):
                xe, ge = e.calibrate_fp8(tiles, headroom=headroom)
                cfg = e.debug_config()
                got, got_other = (xe, ge) if kind == "x" else (ge, xe)
                print(f"{name}: {kind} bracket, headroom {headroom:.6f}: x_exp {xe} g_exp {ge} (expected {kind} {want}, other {pick(other, headroom)})")
                assert (cfg["fp8_x_exp"], cfg["fp8_g_exp"]) == (xe, ge), "the handle does not carry the exponents the call returned"
                assert got == want == pick(m, headroom), (kind, headroom, got, want)
                if not near_power_of_two(other, headroom):
                    assert got_other == pick(other, headroom), (kind, "other kind", headroom, got_other, pick(other, headroom))
    finally:
        e.close()


def test_calibration_drops_captured_graphs_and_restores_replay(monkeypatch):
    """captured launches carry the exponents of their capture: after a calibration the next forward must compute with the new ones
    (bytes of a handle created with them), replays must resume, and a weight load puts the create-time exponents back"""
    name = "n3_3x64x64"
    nb = CASES[name][0]
    tiles, passes, _ = _ref(monkeypatch, name)
    t = passes[-1]
    e = gpu_engines.fresh(monkeypatch, {}, nb, FP8)
    try:
        cfg0 = e.debug_config()
        before = e.forward_batch_u8(tiles).copy()
        assert np.array_equal(e.forward_batch_u8(tiles), before)
        c0, r0 = e.graph_stats()
        assert c0 >= 1 and r0 >= 1, "no graph was captured and replayed before the calibration: the case does not test the drop"
        headroom = 8.0
        xe, ge = e.calibrate_fp8(tiles, headroom=headroom)
        assert not near_power_of_two(t["m_x"], headroom) and not near_power_of_two(t["m_g"], headroom)
        assert (xe, ge) == (pick(t["m_x"], headroom), pick(t["m_g"], headroom))
        assert xe != cfg0["fp8_x_exp"] and ge != cfg0["fp8_g_exp"], "the calibrated exponents equal the old ones: a stale graph would not show"
        after = e.forward_batch_u8(tiles).copy()
        again = e.forward_batch_u8(tiles).copy()
        c1, r1 = e.graph_stats()
        cfg1 = e.debug_config()
        f = gpu_engines.fresh(monkeypatch, {"S2SR_FP8_XEXP": str(xe), "S2SR_FP8_GEXP": str(ge)}, nb, FP8)
        try:
            want = f.forward_batch_u8(tiles).copy()
        finally:
            f.close()
        assert not np.array_equal(want, before), "both pairs of exponents give the same bytes: a stale graph would not show"
        assert np.array_equal(after, want), "the forward behind the calibration did not run with the calibrated exponents"
        assert np.array_equal(again, want)
        assert cfg1["graphs_on"] == cfg0["graphs_on"] == 1
        assert c1 > c0 and r1 > r0, "graph replay did not resume behind the calibration"
        e.load_state_dict(_sd(nb))
        cfg2 = e.debug_config()
        assert (cfg2["fp8_x_exp"], cfg2["fp8_g_exp"]) == (cfg0["fp8_x_exp"], cfg0["fp8_g_exp"])
        assert np.array_equal(e.forward_batch_u8(tiles), before)
    finally:
        e.close()


def test_refusal_restores_the_exponents(monkeypatch):
    """activations that still reach the third pass's ceiling (every fp16 value finite): the call fails, the handle keeps the exponents
    and the bytes from before the call"""
    nb, tiles = 1, _tiles(3, 64, 64, 0)
    passes, clipped = reference(monkeypatch, nb, REFUSE_FACTOR, tiles)
    for t in passes:
        print(f"refusal: pass at 2^{t['xe']} / 2^{t['ge']}: m_x {t['m_x']:.6g} (boundary 0 alone {t['b0']:.6g}), m_g {t['m_g']:.6g}")
    assert len(passes) == 3 and clipped, "the factor does not keep the maxima at the third pass's ceiling"
    env = {"S2SR_FP8_XEXP": "1", "S2SR_FP8_GEXP": "4"}      # neither the defaults nor any pass's scales
    e = gpu_engines.fresh(monkeypatch, env, nb, FP8, sd=_sd(nb, REFUSE_FACTOR))
    try:
        before = e.forward_batch_u8(tiles).copy()
        assert np.array_equal(e.forward_batch_u8(tiles), before)
        with pytest.raises(native.S2srError, match="ceiling"):
            e.calibrate_fp8(tiles)
        cfg = e.debug_config()
        assert (cfg["fp8_x_exp"], cfg["fp8_g_exp"]) == (1, 4) and cfg["graphs_on"] == 1
        assert np.array_equal(e.forward_batch_u8(tiles), before)
        geo, _, _, _, ou8 = e.debug_trunk_taps(0, 1, tiles=tiles)       # eagerly, no graph: the exponents themselves, not a replay
        assert (geo["x_exp"], geo["g_exp"]) == (1, 4) and np.array_equal(ou8, before)
    finally:
        e.close()
