"""Carrying an extra band to the SR grid (csrc/bands.hip), restated in numpy: int64 throughout.

S the scale (2 or 4), n = S S; q the guide, a uint16 image [S H, S W, 3] a 16-bit door produced; b the band [H, W]; lo < hi the
band's own range; w the three guide weights (0..255, Wt their sum); r the window radius; eps the regulariser in squared sample
units; valid an optional mask [H, W] (non-zero: valid); fill what invalid blocks are written with.
  guide    I[Y, X] = floor((w0 q0 + w1 q1 + w2 q2) / Wt); G[y, x] = floor(blocksum(I) / n); p = clip(b, lo, hi)
  coeffs   per valid pixel, over the valid pixels of the window [y - r, y + r] x [x - r, x + r] cut at the border: N, SG, Sp, SGG,
           SGp; cov = N SGp - SG Sp, var = N SGG - SG SG; A = clip(floor((cov << 16) / (var + N N eps)), -(4 << 16), 4 << 16);
           C = floor(((Sp << 16) - A SG) / N); invalid pixels: A = C = 0
  apply    A and C interpolated bilinearly between input-pixel centres with the consistency pass's weights (consistency_model._axis),
           an invalid neighbour replaced by the pixel itself; den = 4 S S;
           g0 = floor((Abar I + Cbar + (den << 15)) / (den << 16)); g = clip(g0, lo, hi)
  exact    the consistency pass's exact step towards n p; invalid blocks = fill
  inexact  the valid blocks whose final sum differs from n p"""
import functools

import numpy as np

import consistency_model as cm

GAIN_LIMIT = 4 << 16


def guide(q, w):
    """I: int64 [S H, S W]"""
    q = np.asarray(q).astype(np.int64)
    w = [int(x) for x in w]
    assert q.ndim == 3 and q.shape[2] == 3 and all(0 <= x <= 255 for x in w) and sum(w) >= 1
    return (w[0] * q[..., 0] + w[1] * q[..., 1] + w[2] * q[..., 2]) // sum(w)


def block_mean(I, S):
    return cm.block_sums(I[..., None], S)[..., 0] // (S * S)


def window_sum(a, r):
    """the sum of a over [y - r, y + r] x [x - r, x + r] cut at the border"""
    H, W = a.shape
    c = np.zeros((H + 1, W + 1), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]


def coefficients(G, p, m, r, eps):
    """-> (A, C, cov): int64 [H, W]; m the 0 / 1 mask"""
    Gm, pm = G * m, p * m
    N, SG, Sp = window_sum(m, r), window_sum(Gm, r), window_sum(pm, r)
    SGG, SGp = window_sum(Gm * G, r), window_sum(Gm * p, r)
    cov, var = N * SGp - SG * Sp, N * SGG - SG * SG
    assert (var >= 0).all() and np.abs(cov).max(initial=0) < 2 ** 46          # cov << 16 stays inside int64
    Ns = np.where(m != 0, N, 1)
    A = np.clip(np.floor_divide(cov << 16, var + Ns * Ns * eps), -GAIN_LIMIT, GAIN_LIMIT)
    C = np.floor_divide((Sp << 16) - A * SG, Ns)
    return np.where(m != 0, A, 0), np.where(m != 0, C, 0), cov


def interpolate(a, m, S):
    """the undivided bilinear sum of a [H, W] on the output grid: int64 [S H, S W]; an invalid neighbour is the pixel itself"""
    H, W = a.shape
    y0, y1, a0, a1 = cm._axis(H, S)
    x0, x1, b0, b1 = cm._axis(W, S)
    a0, a1, b0, b1 = a0[:, None], a1[:, None], b0[None, :], b1[None, :]
    own = a[y0][:, x0]
    at = lambda yy, xx: np.where(m[yy][:, xx] != 0, a[yy][:, xx], own)
    return a0 * (b0 * own + b1 * at(y0, x1)) + a1 * (b0 * at(y1, x0) + b1 * at(y1, x1))


def carry(q, b, S, lo, hi, w=(1, 1, 1), r=2, eps=1, valid=None, fill=0, parts=False):
    """-> (the carried band uint16 [S H, S W], inexact); parts: (that, inexact, a dict of the intermediates)"""
    b = np.asarray(b)
    H, W = b.shape
    n, den = S * S, 4 * S * S
    assert S in (2, 4) and 0 <= lo < hi <= 65535 and 1 <= r <= 4 and eps >= 1 and 0 <= fill <= 65535
    assert np.asarray(q).shape == (S * H, S * W, 3)
    m = np.ones((H, W), np.int64) if valid is None else (np.asarray(valid) != 0).astype(np.int64)
    I = guide(q, w)
    G = block_mean(I, S)
    p = np.clip(b.astype(np.int64), lo, hi)
    A, C, cov = coefficients(G, p, m, r, int(eps))
    Abar, Cbar = interpolate(A, m, S), interpolate(C, m, S)
    lin = Abar * I + Cbar
    g = np.clip((lin + (den << 15)) >> (den.bit_length() - 1 + 16), lo, hi)
    g = cm.exact_step(g[..., None], p[..., None], S, lo, hi)[..., 0]
    inexact = int(((cm.block_sums(g[..., None], S)[..., 0] != n * p) & (m != 0)).sum())
    out = np.where(cm._up(m, S) != 0, g, fill).astype(np.uint16)
    if parts:
        return out, inexact, dict(I=I, G=G, p=p, A=A, C=C, cov=cov, Abar=Abar, Cbar=Cbar, lin=lin)
    return out, inexact


def default_eps(lo, hi):
    return max(1, ((hi - lo) >> 8) ** 2)


# ---- the inputs of the tests --------------------------------------------------------------------------------------------------------
def scene(H, W, S, seed=0):
    """a uint16 guide [S H, S W, 3] with structure at every scale: two sinusoids and noise around mid-range, well inside 0..65535"""
    rng = np.random.default_rng(seed + 31 * H + W + 7 * S)
    yy, xx = np.mgrid[0:H * S, 0:W * S] / float(S)
    chans = [22000 + 9000 * np.sin(xx / 3.1 + c) * np.cos(yy / 2.3) + 5000 * np.sin((xx + 2 * yy) / 9.0 + 2 * c)
             + rng.integers(-1500, 1501, xx.shape) for c in range(3)]
    return np.clip(np.stack(chans, -1), 0, 65535).astype(np.uint16)


SATURATED = ("blocks", "half", "noise", "full")
SATURATED_BANDS = ("mean", "inverse", "full", "steep")


@functools.lru_cache(maxsize=None)
def saturated_scene(H, W, S, name):
    """a uint16 guide [S H, S W, 3] of 0 and 65535 alone: "blocks" alternates per input pixel, "half" is a half plane whose edge cuts
    a column of blocks, "noise" draws every sample of every channel, "full" is all 65535"""
    yy, xx = np.mgrid[0:H * S, 0:W * S]
    if name == "blocks":
        on = (yy // S + xx // S) % 2 == 0
    elif name == "half":
        on = xx >= (W * S) // 2 + 1
    elif name == "noise":
        on = np.random.default_rng(17 * H + W + 3 * S).integers(0, 2, (H * S, W * S, 3)) != 0
    elif name == "full":
        on = np.ones((H * S, W * S), bool)
    else:
        raise KeyError(name)
    q = np.where(on if on.ndim == 3 else on[..., None].repeat(3, 2), 65535, 0).astype(np.uint16)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def saturated_band(H, W, S, name, band):
    """a band for saturated_scene(H, W, S, name): the block mean of the guide under weights (1, 1, 1), 65535 minus it, all 65535, or
    ("steep") three times the block mean's distance from mid-range, clipped: a gain of 3 where the guide has grey block means"""
    G = block_mean(guide(saturated_scene(H, W, S, name), (1, 1, 1)), S)
    b = {"mean": G, "inverse": 65535 - G, "full": np.full_like(G, 65535), "steep": np.clip(3 * G - 65535, 0, 65535)}[band].astype(np.uint16)
    b.setflags(write=False)
    return b


def affine_band(q, S, alpha, beta, w=(1, 1, 1)):
    """(the band: the rounded block mean of alpha I + beta, the truth alpha I + beta on the output grid as float)"""
    t = alpha * guide(q, w).astype(np.float64) + beta
    H, W = t.shape[0] // S, t.shape[1] // S
    return np.rint(t.reshape(H, S, W, S).mean(axis=(1, 3))).astype(np.int64), t


def stray_band(q, S, seed=0):
    """a uint16 band that follows the guide loosely inside 2500..10000, with noise, and strays outside 1000..11000 in places"""
    rng = np.random.default_rng(seed)
    G = block_mean(guide(q, (1, 1, 1)), S)
    b = G // 4 + 800 + rng.integers(-900, 901, G.shape)
    out = rng.random(G.shape)
    b = np.where(out < 0.06, rng.integers(0, 1000, G.shape), np.where(out > 0.94, rng.integers(11001, 30000, G.shape), b))
    return np.clip(b, 0, 65535).astype(np.uint16)


def holes(H, W, seed):
    """a mask with holes of every size, a band of rows among them, and an isolated valid pixel where the image has room for one"""
    rng = np.random.default_rng(seed)
    v = (rng.random((H, W)) > 0.25).astype(np.uint8)
    if H >= 9:
        v[H // 3:H // 3 + 2] = 0
    if H >= 5 and W >= 5:
        v[H - 4:H, W - 4:W] = 0
        v[H - 2, W - 2] = 1
    v[0, 0] = 1
    return v


@functools.lru_cache(maxsize=None)
def case(H, W, S):
    """(guide, band straying outside 1000..11000, mask): made once per shape and scale"""
    q = scene(H, W, S, seed=5)
    return q, stray_band(q, S, seed=6), holes(H, W, seed=7)


@functools.lru_cache(maxsize=None)
def modelled(H, W, S, lo, hi, w, r, eps, masked, fill=0):
    """carry() on case(H, W, S): made once per parameter set"""
    q, b, v = case(H, W, S)
    return carry(q, b, S, lo, hi, w=w, r=r, eps=eps, valid=v if masked else None, fill=fill)
