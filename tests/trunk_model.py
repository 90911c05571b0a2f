"""Host model (fp64) of the 345 RRDB trunk convs as the production kernels compute them (csrc/conv_trunk.hip, csrc/pack.hip),
for the per-RDB parity tests in test_gpu_trunk_insitu.py.  Every conv reads the STORED fields the GPU produced (the taps of
s2sr_debug_trunk_taps), so each conv is checked on its own and errors do not compound.

fp16 path (conv_trunk_f16; S2SR_PREC_F16 / F16_HP, one-wave-per-SIMD trunk).  The trunk x travels as (hi, lo): hi fp16, lo as
e4m3 planes holding lo * 2^lo_exp.  Weights: fp16(w) (pack_trunk_f16_kernel).  Operand of conv k: cat[x_hi, x_1..x_{k-1}].
  conv1-4 (EPI_LRELU, conv_trunk.hip epilogue ~770-790): the bias is the first MFMA's C operand, then LeakyReLU on the fp32 sum:
      x_k = fp16(lrelu(conv + b))
  conv5 (EPI_RDB5 / EPI_RDB5_RRDB, ~790-880): bv = fp32(0.2 * b); t = hi + lo (exact in fp32);
      v = fma(acc, 0.2, t + bv);  rdb3: v = fma(v, 0.2, skip_hi + skip_lo)  (the RRDB's input, read as a (hi, lo) pair)
      stored hi = fp16(v) (RNE); d = v - hi (exact, one v_fma_mix_f32); stored lo = e4m3(clamp(d, +-448 * 2^-lo_exp) * 2^lo_exp)
      (v_cvt_scalef32_pk_fp8_f32 with the scale 2^-lo_exp: it divides by the scale)
  entry (xh_to_fp8_kernel, pack.hip): boundary 0's lo = e4m3(clamp(T * 2^lo_exp, +-448)) of conv_first's fp16 lo T.
fp8 path (conv_trunk_f8; S2SR_PREC_FP8).  The trunk x is fp16 (Xh) plus its e4m3 image at 2^x_exp (the D8 x planes); the
growth planes are e4m3 at 2^g_exp.  Weights: per output channel k_co with max|w_co| * 2^k_co in [224, 448), stored
e4m3(w * 2^k_co) (pack_conv_weights_f8 / pack_trunk_f8_kernel); the MFMA's scale_a takes 2^-k_co back out.
  conv1-4 (~1515-1534): the accumulator comes out scaled by 2^g_exp (scale_a carries + g_exp, the bias C operand is b * 2^g_exp):
      stored = e4m3(clamp(lrelu(conv + b) * 2^g_exp, +-448))                 (med3 clamp, then v_cvt_pk_fp8_f32, RNE)
  conv5 (~1536-1563): acc = conv (unscaled); v = fma(acc, 0.2, Xh_in + fp32(0.2 * b)); rdb3: v = fma(v, 0.2, Xh_skip)
      stored Xh = fp16(v); stored x planes = e4m3(clamp(v * 2^x_exp, +-448)) -- of the fp32 v, not of its fp16 rounding
  entry: boundary 0's x planes = e4m3(clamp(Xh * 2^x_exp, +-448)).

Tolerance (tail_model.Layer): n_acc fp32 roundings of the running sum (one per MFMA: 9 taps x 16-channel stages for fp16,
9 taps x pair-steps of 64 channels for fp8), each of half an ulp of |acc| + 3 sqrt(sum of squared products), plus two ulps of
the result for the epilogue; conv5 scales that by 0.2 (0.04 for rdb3) and adds its own fused roundings.
"""
from __future__ import annotations

import numpy as np

import tail_model as tm
from tail_model import e4m3, e4m3_quantum, f16, f16_quantum, lrelu  # noqa: F401  (re-exported for the tests)

U32 = tm.U32
# The block-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4) does not sum its 64 products into an fp32 accumulator the way the
# fp16 MFMA does.  Measured in situ (test_gpu_trunk_insitu.py prints, per case, the largest share of the tolerance an element
# used): the worst fp8 element needs 21x the fp32-rounding bound (the saturation case; 12-17x at the default scales), against
# 0.12x for the fp16 path's conv1-4.  The fp8 accumulation bound therefore uses the next power of two, 32x: a unit roundoff of
# 2^-19 per MFMA instead of 2^-24 (16x would reject the measured elements; the bound stays far below an e4m3 quantum).
F8_ACC = 2.0 ** -19 / U32


def f8_weights(w):
    """pack_conv_weights_f8: (e4m3(w * 2^k) * 2^-k, k[cout]) with max|w_co| * 2^k_co in [224, 448)."""
    w = np.asarray(w, np.float32).astype(np.float64)
    m = np.abs(w).reshape(w.shape[0], -1).max(axis=1)
    k = np.zeros(w.shape[0], np.int64)
    nz = m > 0
    k[nz] = np.floor(np.log2(448.0 / m[nz])).astype(np.int64)
    for _ in range(2):
        k = np.where(nz & (np.ldexp(m, k) >= 448.0), k - 1, k)
        k = np.where(nz & (np.ldexp(m, k + 1) < 448.0), k + 1, k)
    k = np.clip(k, -100, 100)
    s = np.ldexp(1.0, k).reshape(-1, 1, 1, 1)
    return e4m3(w * s) / s, k


def _operand(x, growth, k):
    """cat[x, x_1..x_{k-1}] of padded fields: x [n, 64, Hp, Wp], growth [n, 128, Hp, Wp] (x1..x4, 32 channels each)"""
    return np.concatenate([x, growth[:, :32 * (k - 1)]], axis=1)


def conv14(x, growth, k, w, b, path, exact=False):
    """conv k (1..4) of an RDB on the stored operands -> (model value lrelu(conv + b) [n, 32, H, W], tol).  path 'f16' or 'f8'
    (x: the x planes' values, growth: the e4m3 planes' values); exact: fp64 weights (no operand rounding)."""
    xin = _operand(x, growth, k)
    cin = xin.shape[1]
    if exact:
        wq = np.asarray(w, np.float64)
    else:
        wq = f16(w) if path == "f16" else f8_weights(w)[0]
    n_acc = 9 * (cin // 16 if path == "f16" else (cin // 32 + 1) // 2)
    L = tm.Layer(tm.conv3, n_acc).add(xin, wq)
    m, _, tol = L.result(b, act=True)
    return m, tol * (F8_ACC if path == "f8" else 1.0)


def conv5(x_in, res, growth, w, b, path, skip=None, exact=False):
    """conv5 of an RDB: operand cat[x_in, x1..x4] (fp16 path: x_in = hi; fp8 path: the x planes' values), `res` the trunk value
    the residual adds (fp16 path: hi + lo; fp8 path: Xh), `skip` the rdb3 skip value (fp16 path: skip hi + lo; fp8: Xh) or
    None; all padded.  -> (v [n, 64, H, W], tol)"""
    xin = _operand(x_in, growth, 5)
    cin = xin.shape[1]
    if exact:
        wq = np.asarray(w, np.float64)
    else:
        wq = f16(w) if path == "f16" else f8_weights(w)[0]
    n_acc = 9 * (cin // 16 if path == "f16" else (cin // 32 + 1) // 2)
    L = tm.Layer(tm.conv3, n_acc).add(xin, wq)
    res = res[:, :, 1:-1, 1:-1]
    bv = np.asarray(np.float32(0.2) * np.asarray(b, np.float32), np.float64)
    m, _, tol = L.result(bv if not exact else 0.2 * np.asarray(b, np.float64), scale=0.2, skip=res)
    tol = tol * (F8_ACC if path == "f8" else 1.0)
    tol = tol + U32 * np.abs(res)                 # t + bv rounded once more
    if skip is not None:
        s = skip[:, :, 1:-1, 1:-1]
        m = 0.2 * m + s
        tol = 0.2 * tol + 2 * U32 * np.abs(m)
    return m, tol


# ---- stored-field encoders (what the epilogues write, from a model value) ------------------------------------------------
def enc_f16(v):
    return f16(v)


def enc_e4m3(v, e):
    """e4m3(clamp(v * 2^e, +-448)), returned as the value (* 2^-e), as the tap decoders return it"""
    return np.ldexp(e4m3(np.ldexp(v, e)), -e)


def enc_lo(v, hi, lo_exp):
    """the fp16 path's lo: e4m3(clamp(v - hi, +-448 * 2^-lo_exp) * 2^lo_exp) as its value"""
    return enc_e4m3(v - hi, lo_exp)


# ---- the check: stored field against the model ---------------------------------------------------------------------------
def check_f16(stored, m, tol, live):
    """fp16 field.  -> dict: bad (mismatch away from a rounding boundary), exc (any mismatch), ratio |m - stored| / (tol + q/2),
    need: the largest multiple of tol an element needs to pass (<= 1: all pass -- the accumulation error seen, in units of tol)"""
    L = np.broadcast_to(live, m.shape)
    want = f16(m)
    q = f16_quantum(m)
    near = (q / 2 - np.abs(m - want)) <= tol
    mis = (stored != want) & L
    need = np.maximum(np.abs(m - stored) - q / 2, np.where(mis, q / 2 - np.abs(m - want), 0.0)) / tol
    return {"bad": mis & ~near, "exc": mis, "ratio": np.where(L, np.abs(m - stored) / (tol + q / 2), 0.0), "n": int(L.sum()),
            "need": float(need[L].max()) if L.any() else 0.0}


def check_e4m3(stored, v, tol, live, e):
    """e4m3 field holding e4m3(clamp(v * 2^e, +-448)) (value returned, * 2^-e).  Same dict as check_f16; the value bound adds
    half the field's quantum and what the clamp cuts off."""
    L = np.broadcast_to(live, v.shape)
    r = np.ldexp(v, e)
    rt = np.ldexp(tol, e)
    rc = np.clip(r, -448.0, 448.0)
    want = np.ldexp(e4m3(r), -e)
    q = e4m3_quantum(rc)
    near = (q / 2 - np.abs(rc - e4m3(rc))) <= rt
    mis = (stored != want) & L
    bound = tol + np.ldexp(q / 2 + np.maximum(np.abs(r) - 448.0, 0.0), -e)
    need = np.maximum(np.abs(v - stored) - (bound - tol), np.where(mis, np.ldexp(q / 2 - np.abs(rc - e4m3(rc)), -e), 0.0)) / tol
    return {"bad": mis & ~near, "exc": mis, "ratio": np.where(L, np.abs(v - stored) / bound, 0.0), "n": int(L.sum()),
            "need": float(need[L].max()) if L.any() else 0.0}


def flagged(c):
    """elements the check rejects (a mismatch away from a rounding boundary, or a value off the model beyond its bound)"""
    return c["bad"] | (c["ratio"] > 1.0)
