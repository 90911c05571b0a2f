"""CPU checks of the host model behind test_gpu_trunk_insitu.py (tests/trunk_model.py): a wrong model is caught here, not on a
GPU.  The sensitivity cases prove that the in-situ check sees single-conv defects that the whole-net bounds (3e-4 HP, 2.5e-3
fast, 1e-2 fp8) cannot: each defect below moves the net's output by 1e-5 .. 1.2e-3 only."""
import numpy as np
import pytest
import torch

import trunk_model as tm
from oracle import rrdbnet_ref as ref
from s2sr import native
from s2sr.weights import synthetic_state_dict


def _decode(b):
    b = np.asarray(b, np.int64)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, np.ldexp(m.astype(np.float64), -9), np.ldexp((8 + m).astype(np.float64), e - 10))
    return np.where(b & 0x80, -v, v)


@pytest.fixture(scope="module")
def sd():
    return synthetic_state_dict(23, seed=0)


def test_f8_weights_match_the_library_packer():
    """trunk_model.f8_weights == s2sr_debug_pack_f8: the per-cout exponent and every e4m3 weight byte's value"""
    lib = native.load_library()
    rng = np.random.default_rng(0)
    for cin, cout in ((64, 32), (160, 32), (192, 64)):
        w = (rng.standard_normal((cout, cin, 3, 3)) * rng.uniform(1e-3, 2.0, size=(cout, 1, 1, 1))).astype(np.float32)
        out = np.zeros(lib.s2sr_debug_pack_f8_bytes(cin, cout), np.uint8)
        ws = np.zeros(64, np.int32)
        assert lib.s2sr_debug_pack_f8(w.ctypes.data, cin, cout, out.ctypes.data, ws.ctypes.data) == 0
        npad, ct = ((cin // 32) + 1) & ~1, (cout + 31) // 32
        got = _decode(out).reshape(npad, 9, ct, 2, 32, 16).transpose(2, 4, 0, 3, 5, 1).reshape(ct * 32, npad * 32, 9)[:cout, :cin]
        wq, k = tm.f8_weights(w)
        assert np.array_equal(127 - ws[:cout], k)
        assert np.array_equal(got * np.ldexp(1.0, -k)[:, None, None], wq.reshape(cout, cin, 9))


@pytest.mark.parametrize("e", [-3, 3, 5, 12, 18])
def test_scaled_e4m3_encoder_matches_the_library(e):
    """enc_e4m3(v, e) == e4m3 of the library encoder at v * 2^e (clamp at 448 included), as a value * 2^-e"""
    lib = native.load_library()
    rng = np.random.default_rng(e + 10)
    v = np.concatenate([np.ldexp(rng.uniform(-2, 2, 3000), rng.integers(-30, 8, 3000) - e), [0.0, np.ldexp(500.0, -e)]])
    v = v.astype(np.float32)
    got = np.ldexp(_decode([lib.s2sr_debug_f32_to_e4m3(float(np.ldexp(np.float64(x), e))) for x in v]), -e)
    assert np.array_equal(got, tm.enc_e4m3(v.astype(np.float64), e))


def _pad(a):
    return np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)))


def _rdb_exact(x, sd, pre):
    g = np.zeros((x.shape[0], 128) + x.shape[2:])
    for k in range(1, 5):
        m, _ = tm.conv14(x, g, k, sd[pre + f"conv{k}.weight"], sd[pre + f"conv{k}.bias"], "f16", exact=True)
        g[:, 32 * (k - 1):32 * k, 1:-1, 1:-1] = m
    return g


def test_model_chained_over_an_rrdb_is_the_oracle(sd):
    """no rounding (fp64 operands): conv14 / conv5 chained over one RRDB == oracle.rrdbnet_ref.rrdb_forward in fp64"""
    rng = np.random.default_rng(3)
    x0 = _pad(rng.standard_normal((2, 64, 9, 11)))
    x, skip = x0, x0
    for r in range(3):
        pre = f"body.5.rdb{r + 1}."
        g = _rdb_exact(x, sd, pre)
        m, _ = tm.conv5(x, x, g, sd[pre + "conv5.weight"], sd[pre + "conv5.bias"], "f16", skip=skip if r == 2 else None, exact=True)
        x = _pad(m)
    tsd = {k: torch.from_numpy(v.astype(np.float64)) for k, v in sd.items() if k.startswith("body.5.")}
    want = ref.rrdb_forward(torch.from_numpy(x0[:, :, 1:-1, 1:-1]), tsd, "body.5").numpy()
    np.testing.assert_allclose(x[:, :, 1:-1, 1:-1], want, rtol=0, atol=1e-12)


# ---- sensitivity ---------------------------------------------------------------------------------------------------------
def _fields(x_hi, x_lo, ws, lo_exp=12, skip=None, swap12=False, drop_lo=False):
    """what a GPU running this RDB with the weights `ws` ({k: (w, b)}) stores: growth [n, 128, Hp, Wp], conv5 (hi, lo)"""
    g = np.zeros((x_hi.shape[0], 128) + x_hi.shape[2:])
    for k in range(1, 5):
        m, _ = tm.conv14(x_hi, g, k, *ws[k], "f16")
        g[:, 32 * (k - 1):32 * k, 1:-1, 1:-1] = tm.f16(m)
    g5 = np.concatenate([g[:, 32:64], g[:, :32], g[:, 64:]], axis=1) if swap12 else g
    m, _ = tm.conv5(x_hi, x_hi if drop_lo else x_hi + x_lo, g5, *ws[5], "f16", skip=skip)
    hi = tm.f16(m)
    return g, hi, tm.enc_lo(m, hi, lo_exp)


def _flag_rates(x_hi, x_lo, ws, stored, skip=None, lo_exp=12):
    """the in-situ check of test_gpu_trunk_insitu, with the correct weights `ws`, on the stored fields -> {field: rejected share}"""
    g, hi, lo = stored
    live = np.ones(hi.shape[2:], bool)
    out = {}
    for k in range(1, 5):
        m, tol = tm.conv14(x_hi, g, k, *ws[k], "f16")
        out[f"x{k}"] = float(tm.flagged(tm.check_f16(g[:, 32 * (k - 1):32 * k, 1:-1, 1:-1], m, tol, live)).mean())
    m, tol = tm.conv5(x_hi, x_hi + x_lo, g, *ws[5], "f16", skip=skip)
    f = tm.flagged(tm.check_f16(hi, m, tol, live)) | tm.flagged(tm.check_e4m3(lo, m - hi, tol, live, lo_exp))
    out["x"] = float(f.mean())
    return out


def _trunk(seed, shape=(1, 64, 12, 12), lo_exp=12):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape)
    hi = tm.f16(v)
    return _pad(hi), _pad(tm.enc_lo(v, hi, lo_exp))


def _ws(sd, pre):
    return {k: (sd[pre + f"conv{k}.weight"], sd[pre + f"conv{k}.bias"]) for k in range(1, 6)}


def _defect(ws, k, wf=None, bf=None):
    d = dict(ws)
    w, b = ws[k]
    d[k] = (wf(w) if wf else w, bf(b) if bf else b)
    return d


DEFECTS = {   # name: (RDB, {field: ...} affected, how the GPU's weights / wiring differ)
    "bias_rolled": ("body.11.rdb2.", "x3", dict(k=3, bf=lambda b: np.roll(b, 1))),
    "bias_dropped": ("body.0.rdb1.", "x1", dict(k=1, bf=lambda b: 0 * b)),
    "conv5_weights_1pct": ("body.22.rdb3.", "x", dict(k=5, wf=lambda w: (w * np.float32(1.01)).astype(np.float32))),
    "taps_flipped": ("body.11.rdb2.", "x3", dict(k=3, wf=lambda w: np.ascontiguousarray(w[:, :, ::-1, :]))),
    "x1_x2_swapped": ("body.11.rdb2.", "x", dict(swap12=True)),
    "lo_dropped": ("body.3.rdb1.", "x", dict(drop_lo=True)),
    "neighbour_weights": ("body.7.rdb1.", "x2", dict(neighbour=2)),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_check_flags_single_conv_defects(sd, name):
    """The check applied to fields stored by a defective RDB (one defect at a time) rejects at least half of the affected
    field's elements; fields stored by a correct RDB pass (no element rejected)."""
    pre, field, how = DEFECTS[name]
    ws = _ws(sd, pre)
    x_hi, x_lo = _trunk(7)
    skip = None
    if pre.endswith("rdb3."):
        s_hi, s_lo = _trunk(8)
        skip = s_hi + s_lo
    clean = _flag_rates(x_hi, x_lo, ws, _fields(x_hi, x_lo, ws, skip=skip), skip=skip)
    assert all(v == 0.0 for v in clean.values()), clean
    how = dict(how)
    kw = {k: how.pop(k) for k in ("swap12", "drop_lo") if k in how}
    if "neighbour" in how:
        k = how.pop("neighbour")
        blk = int(pre.split(".")[1])
        nxt = _ws(sd, f"body.{blk}.rdb2.")
        bad_ws = _defect(ws, k, wf=lambda w: nxt[k][0], bf=lambda b: nxt[k][1])
    elif how:
        bad_ws = _defect(ws, **how)
    else:
        bad_ws = ws
    rates = _flag_rates(x_hi, x_lo, ws, _fields(x_hi, x_lo, bad_ws, skip=skip, **kw), skip=skip)
    print(f"{name}: rejected share per field {rates}")
    assert rates[field] >= 0.5, (name, field, rates)
