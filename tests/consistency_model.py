"""The radiometric consistency pass (csrc/consistency.hip), restated in numpy: int64 throughout.

Per channel: S the scale (2 or 4), n = S S; q the quantised image [S H, S W, 3]; v = clip(img, lo, hi) the input the net saw;
sum[y, x] the sum of q over block [S y, S y + S) x [S x, S x + S); e = n v - sum.
  exact   k = floor(e / n), r = e - n k; block sample (i, j) gets d = k + (rank[i][j] < r); q' = clip(q + d, lo, hi)
  smooth  e interpolated bilinearly between input-pixel centres with edge replication; d = floor((num + den / 2) / den),
          den = 4 S S n; q' = clip(q + d, lo, hi)
  mode 1  exact; mode 2  smooth, the sums again, exact on what remains
  inexact[c] = the blocks of channel c whose final sum differs from n v"""
import numpy as np

EXACT, SMOOTH = 1, 2
RANK = {2: np.array([[0, 2], [3, 1]], np.int64),
        4: np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.int64)}


def block_sums(q, S):
    """[S H, S W, C] -> int64 [H, W, C]"""
    q = np.asarray(q).astype(np.int64)
    H, W, C = q.shape[0] // S, q.shape[1] // S, q.shape[2]
    assert q.shape[:2] == (H * S, W * S)
    return q.reshape(H, S, W, S, C).sum(axis=(1, 3))


def _up(a, S):
    return np.repeat(np.repeat(a, S, axis=0), S, axis=1)


def exact_step(q, v, S, lo, hi):
    n = S * S
    e = n * v - block_sums(q, S)
    k = np.floor_divide(e, n)
    r = e - n * k
    assert (r >= 0).all() and (r < n).all()
    rank = np.tile(RANK[S], v.shape[:2])[..., None]
    return np.clip(q + _up(k, S) + (rank < _up(r, S)), lo, hi)


def _axis(N, S):
    """per output coordinate: the input coordinate, its neighbour, and their weights"""
    o = np.arange(N * S)
    y, i = o // S, o % S
    t = 2 * i + 1 - S
    nb = np.clip(y + np.sign(t), 0, N - 1)
    w1 = np.abs(t)
    return y, nb, 2 * S - w1, w1


def smooth_delta(e, S):
    """The smooth step's d for a residual plane e [H, W, C]: int64 [S H, S W, C]."""
    H, W = e.shape[:2]
    y0, y1, a0, a1 = _axis(H, S)
    x0, x1, b0, b1 = _axis(W, S)
    a0, a1 = a0[:, None, None], a1[:, None, None]
    b0, b1 = b0[None, :, None], b1[None, :, None]
    at = lambda yy, xx: e[yy][:, xx]
    num = a0 * (b0 * at(y0, x0) + b1 * at(y0, x1)) + a1 * (b0 * at(y1, x0) + b1 * at(y1, x1))
    assert np.abs(num).max(initial=0) < 2 ** 31 - 2 ** 12          # the device's int32
    den = 4 * S * S * S * S
    return np.floor_divide(num + den // 2, den)


def smooth_step(q, v, S, lo, hi):
    e = S * S * v - block_sums(q, S)
    return np.clip(q + smooth_delta(e, S), lo, hi)


def consistency(sr, img, S, mode, lo=0, hi=255, swap=False):
    """-> (the consistent image in sr's dtype, inexact int64 [3]).  swap: image channel c belongs to input channel 2 - c."""
    assert S in (2, 4) and mode in (EXACT, SMOOTH)
    sr, img = np.asarray(sr), np.asarray(img)
    q = sr.astype(np.int64)
    v = np.clip(img.astype(np.int64), lo, hi)
    if swap:
        v = v[:, :, ::-1]
    assert q.shape == (v.shape[0] * S, v.shape[1] * S, 3)
    if mode == SMOOTH:
        q = smooth_step(q, v, S, lo, hi)
    q = exact_step(q, v, S, lo, hi)
    inexact = (block_sums(q, S) != S * S * v).sum(axis=(0, 1))
    return q.astype(sr.dtype), inexact.astype(np.int64)


# ---- the two inputs of the tests ---------------------------------------------------------------------------------------------------
def clip_free_input(H, W, S, seed=0, dtype="uint8", lo=0, hi=255):
    """(sr, img): img uniform in [lo + 32, hi - 31), sr = repeat(img, S) + noise uniform in [-24, 24] (for uint8: [32, 224)).
    A corrected sample is img + (noise - the block's mean noise) + (d - the block's mean d) + a rank bit; a block's mean of
    independent noise stays within a few units of 0 and d varies by a few units inside a block, so the excursion stays near the
    noise's 24, inside the margin of 31 -- for these seeded draws, which is what the tests assert through the model (the bound is
    not a worst case: one sample at +24 among fifteen at -24 would reach +45).
    For uint16, img also holds values on both sides of [lo, hi] in one corner: they clamp to lo / hi, sr there is the clamped
    value itself, and one ring of blocks around the corner carries no noise, so the smooth step has nothing to spread into
    samples that sit on a limit."""
    rng = np.random.default_rng(1000 * H + W + 7 * S + seed)
    img = rng.integers(lo + 32, hi - 31, size=(H, W, 3))
    noise = rng.integers(-24, 25, size=(H * S, W * S, 3))
    if dtype == "uint16" and H * W > 1:
        hh, ww = max(1, H // 3), max(1, W // 3)
        below = max(lo - 90, 0)
        img[:hh, :ww] = below + rng.integers(0, 2, size=(hh, ww, 3)) * (hi + 500 - below)      # lo - 90, or hi + 500
        noise[:(hh + 1) * S, :(ww + 1) * S] = 0
    sr = _up(np.clip(img, lo, hi), S) + noise
    return sr.astype(dtype), img.astype(dtype)


def saturating_input(H, W, S, seed=0, dtype="uint8", lo=0, hi=255):
    """(sr, img): img uniform over [lo, hi], noise in [-40, 40] (scaled to the range), pre-clipped: blocks near the ends stay inexact."""
    rng = np.random.default_rng(2000 * H + W + 7 * S + seed)
    img = rng.integers(lo, hi + 1, size=(H, W, 3))
    a = max(40, (hi - lo) * 40 // 255)
    sr = np.clip(_up(img, S) + rng.integers(-a, a + 1, size=(H * S, W * S, 3)), lo, hi)
    return sr.astype(dtype), img.astype(dtype)
