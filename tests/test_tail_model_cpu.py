"""CPU checks of the host model behind test_gpu_tail.py (tests/tail_model.py): a wrong model is caught here, not on a GPU."""
import numpy as np
import pytest

import tail_model as tm
from s2sr import native


def _decode(b):
    b = np.asarray(b, np.int64)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, np.ldexp(m.astype(np.float64), -9), np.ldexp((8 + m).astype(np.float64), e - 10))
    return np.where(b & 0x80, -v, v)


def test_e4m3_rounding_and_clamp_match_the_library_encoder():
    """tail_model.e4m3 == s2sr_debug_f32_to_e4m3 (the packers' encoder) on random values over every binade, the exact
    midpoints between neighbouring codes (ties to even), the subnormal range, and past 448 (saturation, never NaN)."""
    lib = native.load_library()
    rng = np.random.default_rng(0)
    codes = _decode(np.arange(0, 0x7F))                      # every finite non-negative code
    mids = (codes[:-1] + codes[1:]) / 2
    vals = np.concatenate([
        np.ldexp(rng.uniform(1, 2, 4000), rng.integers(-14, 10, 4000)),
        codes, mids, np.nextafter(mids.astype(np.float32), np.float32(np.inf)), np.nextafter(mids.astype(np.float32), np.float32(0)),
        rng.uniform(0, 2.0 ** -6, 500), [447.9, 448.0, 455.9, 456.0, 463.9, 464.0, 500.0, 1e6],
    ]).astype(np.float32)
    vals = np.concatenate([vals, -vals])
    got = _decode([lib.s2sr_debug_f32_to_e4m3(float(v)) for v in vals])
    want = tm.e4m3(vals.astype(np.float64))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(vals[i]), float(got[i]), float(want[i])) for i in bad[:8]]


def test_phase_form_is_conv_on_nearest_2x():
    """The sub-pixel kernels (pack_conv_weights_phase_f8hp's sums) on the source image == a 3x3 conv on its nearest-2x, in
    fp64.  Weights on a 2^-12 grid below 1 so the fp32 sums are exact; odd source sizes."""
    rng = np.random.default_rng(1)
    w = (rng.integers(-2048, 2048, (5, 4, 3, 3)) / 4096.0).astype(np.float32)
    for H, W in ((7, 9), (4, 5), (1, 3)):
        x = np.pad(rng.standard_normal((2, 4, H, W)), ((0, 0), (0, 0), (1, 1), (1, 1)))
        a = tm.conv_phase(x, tm.phase_weights(w))
        b = tm.conv_up3(x, w)
        assert a.shape == b.shape == (2, 5, 2 * H, 2 * W)
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)


@pytest.mark.parametrize("form", ["3x3", "phase"])
def test_split_model_converges_to_the_fp64_conv(form):
    """x = fp16 hi + a residual carried as e4m3(lo * 2^11), weights fp32: the hi-only model is off by the dropped terms
    (~2^-12 relative), each correction term brings it closer (x_lo * w_hi, then x_hi * w_lo), the full split model sits at the e4m3 level of the corrections
    (~2^-16 relative) -- and the folded form (fp16 w_lo) at least as close."""
    rng = np.random.default_rng(2)
    v = rng.standard_normal((1, 64, 10, 12))
    hi = tm.f16(v)
    lo8, hi8 = tm.out_planes(v, hi)
    xp = lambda a: np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)))
    w = (rng.standard_normal((64, 64, 3, 3)) / 24).astype(np.float32)
    ref = tm.true_conv("3x3" if form == "3x3" else "up3", xp(hi + lo8), w)
    ref_v = tm.true_conv("3x3" if form == "3x3" else "up3", xp(v), w)
    s = tm.split_any(tm.weights_for(form, w))
    op = tm.op_for(form)
    e0 = np.abs(op(xp(hi), s["hi"]) - ref).max()
    e1 = np.abs(op(xp(hi), s["hi"]) + op(xp(lo8), s["hi8"]) - ref).max()
    L = tm.model_split64(form, xp(hi), xp(lo8), xp(hi8), w)
    e2 = np.abs(L.main + L.corr - ref).max()
    Lf = tm.model_split64(form, xp(hi), xp(lo8), xp(hi8), w, stages=6, fold=True)
    e3 = np.abs(Lf.main + Lf.corr - ref).max()
    scale = np.abs(ref).max()
    assert e0 > 2.0 ** -14 * scale and e1 < e0 and e2 < e1 / 8 and e2 < 2.0 ** -15 * scale and e3 <= 1.5 * e2, (e0, e1, e2, e3, scale)
    # the stored residual itself is within e4m3's half quantum of the true one: the model of the whole stack stays close
    assert np.abs(ref - ref_v).max() < 2.0 ** -14 * scale


def test_layer_tolerance_is_below_the_lost_correction():
    """The per-element tolerance (tail_model.Layer.result) must be far below what a lost correction term costs, or the
    GPU test's sensitivity assertion could not hold: on unit-scale data the dropped terms exceed it at most elements."""
    rng = np.random.default_rng(3)
    v = rng.standard_normal((1, 64, 16, 16))
    hi = tm.f16(v)
    lo8, hi8 = tm.out_planes(v, hi)
    xp = lambda a: np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)))
    w = (rng.standard_normal((64, 64, 3, 3)) / 24).astype(np.float32)
    m, h, tol = tm.model_split64("3x3", xp(hi), xp(lo8), xp(hi8), w).result(np.zeros(64))
    assert np.mean(np.abs(m - h) > tol) > 0.8
