"""Host model (fp64) of the six head / tail convs as the production kernels compute them (csrc/conv3x3.hip, csrc/pack.hip),
for the per-layer parity tests in test_gpu_tail.py.  Every layer reads the STORED input fields the GPU produced (the taps of
s2sr_debug_forward_taps), so each layer is checked on its own and errors do not compound.

Operand formats (split-operand / "hp" tail, S2SR_PREC_F16_HP or S2SR_FP8_TAIL=hp):
  w_hi = fp16(w), w_lo = w - w_hi (exact in fp32)                         pack_conv_weights / pack_f8hp_taps (conv3x3.hip)
  e4m3 weight planes: e4m3(w_hi) and e4m3(w_lo * 2^11)                   pack_f8hp_taps, f32_to_e4m3
  activation planes of a 64-channel output v (fp32 accumulator):         conv3x3.hip epilogue, HPO branch
    hi = fp16(v); lo8 = e4m3(clamp((v - hi) * 2^11, +-448)); hi8 = e4m3(clamp(hi, +-448))
  conv_body's planes from the trunk (hi, lo as stored):                  trunk_to_fp8_kernel (pack.hip)
    lo8 = e4m3(clamp(lo * 2^11, +-448)) (e4m3 lo at 2^lo_exp: decoded, * 2^(11 - lo_exp), clamped, re-encoded); hi8 as above

Layer arithmetic (x_hi: fp16 field, lo8 / hi8: the e4m3 fields' values, lo8 already * 2^-11):
  conv_first  hp:   (conv(P0, w_hi) + conv(P0, fp16(w_lo))) * (1/255) + b           load_weights_locked nseg 2, EPI_FIRST
              fast: conv(P0, w_hi) * (1/255) + b
  cin-64 split (body, up1, up2, hr, last 8-stage):
              conv(x_hi, w_hi) + conv(lo8, e4m3(w_hi)) + conv(hi8, e4m3(w_lo * 2^11) * 2^-11) + b
              body: + F (EPI_BODY); up / hr: lrelu (EPI_LRELU)
  conv_last folded (6 stages, S2SR_LAST_FOLD=1): conv(x_hi, w_hi) + conv(x_hi, fp16(w_lo)) + conv(lo8, e4m3(w_hi)) + b
              (pack_f8hp_taps fold: w_lo as fp16 in couts 8..10, EPI_LAST o3 = acc[c] + acc[8 + c])
  up1 / up2 sub-pixel form: nearest-2x then 3x3 == for output parity (py, q) a 2x2 kernel on the source image whose taps are
              the sums (in double, stored as fp32) of the 3x3 taps that land on the same source pixel
              (pack_conv_weights_phase_f8hp); that fp32 kernel is then split as above
  fast / fp8 tail: conv(x_hi, fp16(w)) + b (+ F, lrelu as above), the up-convs on fp16(phase kernel)
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as Fn

U32 = 2.0 ** -24     # unit roundoff of the fp32 accumulator


def f16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def e4m3(a):
    """OCP e4m3fn value of a (round to nearest even, subnormals in steps of 2^-9, saturating at +-448): the values
    f32_to_e4m3 (conv3x3.hip) and the device conversions behind a +-448 clamp produce."""
    a = np.clip(np.asarray(a, np.float64), -448.0, 448.0)
    return np.sign(a) * np.minimum(np.rint(np.abs(a) / e4m3_quantum(a)) * e4m3_quantum(a), 448.0)


def e4m3_quantum(a):
    """Spacing of e4m3 values at |a| (2^-9 in the subnormal range)."""
    m = np.abs(np.asarray(a, np.float64))
    _, e = np.frexp(np.where(m > 0, m, 1.0))
    return np.ldexp(1.0, np.maximum(e - 1, -6) - 3)


def f16_quantum(a):
    m = np.abs(np.asarray(a, np.float64))
    _, e = np.frexp(np.where(m > 0, m, 1.0))
    return np.ldexp(1.0, np.maximum(e - 1, -14) - 10)


def lrelu(v):
    return np.where(v >= 0, v, 0.2 * v)


def split(w):
    """fp32 weights -> the operands the packers make of them."""
    w = np.asarray(w, np.float32).astype(np.float64)
    hi = f16(w)
    lo = w - hi
    return {"hi": hi, "lo16": f16(lo), "hi8": e4m3(hi), "lo8": e4m3(lo * 2048.0) / 2048.0, "lo": lo, "w": w}


def phase_weights(w):
    """pack_conv_weights_phase_f8hp: {(py, q): [cout, cin, 2, 2] fp32} -- tap (a, b) of parity (py, q) reads source pixel
    (y + py - 1 + a, x + q - 1 + b) and carries the double sum of the 3x3 taps (dy, dx) with floor((py + dy - 1) / 2) == py - 1 + a."""
    w = np.asarray(w, np.float32).astype(np.float64)
    out = {}
    for py in range(2):
        for q in range(2):
            k = np.zeros(w.shape[:2] + (2, 2))
            for dy in range(3):
                for dx in range(3):
                    a = (py + dy - 1) // 2 - py + 1
                    b = (q + dx - 1) // 2 - q + 1
                    k[:, :, a, b] += w[:, :, dy, dx]
            out[(py, q)] = k.astype(np.float32)
    return out


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def conv3(xp, w):
    """3x3 conv of a PADDED tensor [n, C, Hp, Wp] (halo included) -> [n, Cout, Hp-2, Wp-2] at logical (y, x)."""
    return Fn.conv2d(_t(xp), _t(w)).numpy()


def conv_phase(xp, w4):
    """Sub-pixel form on a padded SOURCE tensor -> [n, Cout, 2(Hp-2), 2(Wp-2)] at logical 2x coordinates."""
    n, _, Hp, Wp = xp.shape
    co = next(iter(w4.values())).shape[0]
    out = np.zeros((n, co, 2 * (Hp - 2), 2 * (Wp - 2)))
    for (py, q), k in w4.items():
        out[:, :, py::2, q::2] = Fn.conv2d(_t(xp[:, :, py:py + Hp - 1, q:q + Wp - 1]), _t(k)).numpy()
    return out


def conv_up3(xp, w):
    """nearest-2x, then 3x3 (the upsample-on-load form) on a padded source -> logical 2x coordinates."""
    x = xp[:, :, 1:-1, 1:-1]
    u = np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)
    return conv3(np.pad(u, ((0, 0), (0, 0), (1, 1), (1, 1))), w)


class Layer:
    """One conv as a sum of product terms conv(x_i, w_i) plus bias (and a post-op).  Everything is fp64; `terms` hold the
    correction terms separately so the hi-only model (corrections dropped) comes from the same pass."""

    def __init__(self, op, n_acc):
        self.op, self.n_acc = op, n_acc
        self.main, self.corr, self.sq = 0.0, 0.0, 0.0

    def add(self, x, w, correction=False):
        y = self.op(x, w)
        if correction:
            self.corr = self.corr + y
        else:
            self.main = self.main + y
        self.sq = self.sq + self.op(x * x, _wmap(w, lambda a: a * a))
        return self

    def result(self, bias, scale=1.0, skip=None, act=False):
        """-> (model, hi-only model, tolerance).  Tolerance: the fp32 accumulator is rounded once per MFMA (n_acc = stages x
        taps of the launch), each time by at most half an ulp of the running sum; the running sum is bounded by |acc| plus
        three standard deviations of a random walk over the products (3 * sqrt(sum of squares)).  Plus the epilogue's own
        roundings (scale, bias, skip: 2 ulps of the result)."""
        b = np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
        acc = (self.main + self.corr) * scale
        run = np.abs(acc) + 3.0 * np.sqrt(self.sq) * scale
        tol = U32 * (self.n_acc + 2) * run
        m = acc + b
        h = self.main * scale + b
        if skip is not None:
            m = m + skip
            h = h + skip
        tol = tol + 2 * U32 * np.abs(m)
        if act:
            m, h = lrelu(m), lrelu(h)
        return m, h, tol


def op_for(form):
    return {"3x3": conv3, "phase": conv_phase, "up3": conv_up3}[form]


def weights_for(form, w):
    """the fp32 kernel the packer splits: the 3x3 weights, or the sub-pixel kernels"""
    return phase_weights(w) if form == "phase" else np.asarray(w, np.float32)


def _wmap(ws, f):
    return {k: f(v) for k, v in ws.items()} if isinstance(ws, dict) else f(ws)


def split_any(wk):
    if isinstance(wk, dict):
        s = {k: split(v) for k, v in wk.items()}
        return {f: {k: s[k][f] for k in s} for f in ("hi", "lo16", "hi8", "lo8", "lo", "w")}
    return split(wk)


def n_acc(form, stages):
    return stages * (4 if form == "phase" else 9)


def model_split64(form, x_hi, lo8, hi8, w, stages=8, fold=False):
    """cin-64 split-operand conv (8 stages; conv_last folded: 6).  x_hi / lo8 / hi8 padded [n, 64, Hp, Wp]."""
    s = split_any(weights_for(form, w))
    L = Layer(op_for(form), n_acc(form, stages))
    L.add(x_hi, s["hi"])
    if fold:
        L.add(x_hi, s["lo16"], True)
    else:
        L.add(hi8, s["lo8"], True)
    L.add(lo8, s["hi8"], True)
    return L


def model_plain64(form, x_hi, w):
    """fp16 tail (fast mode, fp8 mode): one pass of 4 stages over x_hi with fp16 weights."""
    s = split_any(weights_for(form, w))
    return Layer(op_for(form), n_acc(form, 4)).add(x_hi, s["hi"])


def model_first(p0, w, hp):
    s = split(w)
    L = Layer(conv3, 9 * (2 if hp else 1))
    L.add(p0[:, :3], s["hi"][:, :3])
    if hp:
        L.add(p0[:, :3], s["lo16"][:, :3], True)
    return L


def true_conv(form, x, w):
    """fp64 conv of the true operands (fidelity column)"""
    w = np.asarray(w, np.float32).astype(np.float64)
    return (conv3 if form == "3x3" else conv_up3)(x, w)


def trunk_planes(hi, lo):
    """trunk_to_fp8_kernel: conv_body's e4m3 operands from the trunk (hi fp16, lo the value stored) -> (lo8 * 2^-11, hi8)"""
    return e4m3(lo * 2048.0) / 2048.0, e4m3(hi)


def out_planes(v, hi):
    """the epilogue's e4m3 planes of a 64-channel output: lo8 (* 2^-11) from the value and its stored fp16 hi, hi8 from hi"""
    return e4m3((v - hi) * 2048.0) / 2048.0, e4m3(hi)
