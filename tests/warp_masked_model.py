"""numpy model of the masked bilinear warp (csrc/tiles.hip warp_bilinear_masked_kernel) and the scenes and masks its
tests share (tests/test_tiles_nodata_cpu.py, tests/test_gpu_tiles_nodata.py).

Source pixel (y, x) is valid iff valid[y // vs, x // vs] != 0.  For one output pixel the source coordinates, the coverage test and
the four edge-replicated taps are the plain warp's (oracle/tiles_ref.py warp_bilinear, restated here from the kernel, not imported:
the all-valid test ties the two).  Then
  outside the source                    (0, 0, 0, 0)
  all four taps valid                   the plain lerp chain
  no tap valid                          (0, 0, 0, 0)
  some valid                            w00 = (1-fx)(1-fy), w10 = fx(1-fy), w01 = (1-fx)fy, w11 = fx fy; ws = the valid ones summed
                                        in that order; ws < 0.5: (0, 0, 0, 0); else (sum of w p over the valid taps) / ws, + 0.5,
                                        truncated; alpha 255
every float32 operation rounded on its own.  An invalid tap's weight enters as +0: x + 0 = x and 0 * p = 0 exactly for the
non-negative finite values here, so "summed over the valid taps" and "summed over all four with the invalid weights zeroed" are
the same numbers."""
import functools

import numpy as np

from s2sr import geo, tiles

f32 = np.float32

# the three scenes of tests/test_gpu_tiles.py::test_warp_bit_exact
SCENES = [(32633, (600000.0, 5100000.0)), (32733, (300000.0, 6200000.0)), (4326, (13.3, 52.6))]


def scene(h, w, seed=0):
    """the synthetic image of tests/test_gpu_tiles.py (_scene), restated: a test module is nobody's library"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([120 + 90 * np.sin(xx / 11.0 + c) * np.cos(yy / 7.0) + rng.integers(-15, 16, (h, w)) for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


def plan_for(epsg, origin, h=150, w=211):
    px = 2.5 if epsg != 4326 else 2.5e-5
    return tiles.plan_warp(w, h, geo.Placement(origin[0], origin[1], px, px), geo.CRS(epsg))


def identity_grid(h, w, step=4, shift=(0.0, 0.0)):
    """node grid of the warp that maps output pixel (oy, ox) to source (ox + shift[0], oy + shift[1]): for hand-made cases"""
    gh, gw = (h - 1 + step - 1) // step + 1, (w - 1 + step - 1) // step + 1
    gx, gy = np.meshgrid(np.arange(gw) * float(step) + shift[0], np.arange(gh) * float(step) + shift[1])
    return np.stack([gx, gy], -1).astype(np.float32)


def mask_mixed(h, w, seed=1):
    """vs = 1: 20 % random holes, a 3-row band, and a diagonal edge that leaves about 30 % invalid"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    v = (rng.random((h, w)) >= 0.2)
    v[h // 3:h // 3 + 3] = False
    v &= (xx / w + yy / h) < diagonal_cut(0.30)
    return v.astype(np.uint8)


def diagonal_cut(fraction):
    """t with area{x + y >= t in the unit square} = fraction (fraction <= 0.5): the corner triangle has area (2 - t)^2 / 2"""
    return 2.0 - np.sqrt(2.0 * fraction)


def mask_diagonal(h, w, fraction=0.30):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx / w + yy / h) < diagonal_cut(fraction)).astype(np.uint8)


def mask_coarse(h, w, vs, seed=2):
    """[ceil(h / vs), ceil(w / vs)]: random holes (25 %) and an invalid corner block"""
    rng = np.random.default_rng(seed)
    mh, mw = -(-h // vs), -(-w // vs)
    v = (rng.random((mh, mw)) >= 0.25)
    v[-mh // 4:, -mw // 3:] = False
    return v.astype(np.uint8)


def repaint(rgb, valid, vs, how, seed=3):
    """the raster with its invalid pixels holding 0, 255 or random bytes"""
    up = np.repeat(np.repeat(valid != 0, vs, axis=0), vs, axis=1)[:rgb.shape[0], :rgb.shape[1]]
    out = rgb.copy()
    if how == "random":
        junk = np.random.default_rng(seed).integers(0, 256, rgb.shape, dtype=np.uint8)
        out[~up] = junk[~up]
    else:
        out[~up] = how
    return out


def _add(a, b):
    return (a + b).astype(f32)


def _mul(a, b):
    return (a * b).astype(f32)


def _sub(a, b):
    return (a - b).astype(f32)


def warp_bilinear_masked(rgb, valid, vs, grid, step, out_h, out_w):
    rgb, valid = np.asarray(rgb), np.asarray(valid)
    H, W = rgb.shape[:2]
    assert valid.shape == (-(-H // vs), -(-W // vs)), (valid.shape, H, W, vs)
    gh, gw = grid.shape[:2]
    oy, ox = np.mgrid[0:out_h, 0:out_w]
    gi, gj = oy // step, ox // step
    gi1, gj1 = np.minimum(gi + 1, gh - 1), np.minimum(gj + 1, gw - 1)
    inv = f32(1.0) / f32(step)
    fi, fj = _mul((oy - gi * step).astype(f32), inv), _mul((ox - gj * step).astype(f32), inv)
    g = grid.astype(f32)

    def node(k):
        a, b, c, d = g[gi, gj, k], g[gi, gj1, k], g[gi1, gj, k], g[gi1, gj1, k]
        t0, t1 = _add(a, _mul(_sub(b, a), fj)), _add(c, _mul(_sub(d, c), fj))
        return _add(t0, _mul(_sub(t1, t0), fi))

    u, v = node(0), node(1)
    inside = (u >= f32(-0.5)) & (u <= f32(W) - f32(0.5)) & (v >= f32(-0.5)) & (v <= f32(H) - f32(0.5))
    xf, yf = np.floor(u), np.floor(v)
    fx, fy = _sub(u, xf), _sub(v, yf)
    xi, yi = np.where(inside, xf, 0).astype(np.int64), np.where(inside, yf, 0).astype(np.int64)
    x0, x1 = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1)
    y0, y1 = np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
    ok = valid != 0
    k00, k10, k01, k11 = ok[y0 // vs, x0 // vs], ok[y0 // vs, x1 // vs], ok[y1 // vs, x0 // vs], ok[y1 // vs, x1 // vs]
    every, some = k00 & k10 & k01 & k11, k00 | k10 | k01 | k11
    gx, gy = _sub(f32(1.0), fx), _sub(f32(1.0), fy)
    zero = f32(0.0)
    w00, w10 = np.where(k00, _mul(gx, gy), zero), np.where(k10, _mul(fx, gy), zero)
    w01, w11 = np.where(k01, _mul(gx, fy), zero), np.where(k11, _mul(fx, fy), zero)
    ws = _add(_add(_add(w00, w10), w01), w11)
    mixed = inside & some & ~every & (ws >= f32(0.5))
    plain = inside & every
    safe = np.where(mixed, ws, f32(1.0))
    src = rgb.astype(f32)
    out = np.zeros((out_h, out_w, 4), np.uint8)
    for k in range(3):
        p00, p10, p01, p11 = src[y0, x0, k], src[y0, x1, k], src[y1, x0, k], src[y1, x1, k]
        t = _add(p00, _mul(_sub(p10, p00), fx))
        b = _add(p01, _mul(_sub(p11, p01), fx))
        lerp = _add(t, _mul(_sub(b, t), fy))
        s = _add(_add(_add(_mul(w00, p00), _mul(w10, p10)), _mul(w01, p01)), _mul(w11, p11))
        val = np.where(plain, lerp, (s / safe).astype(f32))
        out[..., k] = np.where(plain | mixed, _add(val, f32(0.5)).astype(np.int64), 0)
    out[..., 3] = np.where(plain | mixed, 255, 0)
    return out


# ---- the cases of the GPU tests: 150 x 211 scenes under six masks ------------------------------------------------------------------------
H, W = 150, 211


@functools.lru_cache(maxsize=None)
def case(epsg, kind):
    """(rgb, valid, vs, plan, the model's raster) of one scene and mask"""
    origin = dict(SCENES)[epsg]
    rgb, plan = scene(H, W, seed=epsg), plan_for(epsg, origin)
    valid, vs = {"mixed": (mask_mixed(H, W), 1), "coarse": (mask_coarse(H, W, 4), 4), "none": (np.zeros((H, W), np.uint8), 1),
                 "thirds": (mask_coarse(H, W, 3, seed=4), 3),                   # no power of two: the cell index by division
                 "every3": (np.ones((50, 71), np.uint8), 3),
                 "every": (np.ones((38, 53), np.uint8), 4)}[kind]
    want = warp_bilinear_masked(rgb, valid, vs, plan.grid, plan.step, plan.out_h, plan.out_w)
    return rgb, valid, vs, plan, want


def warp(e, rgb, valid, vs, plan):
    """the entry on a case"""
    return e.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w, valid=valid, valid_scale=vs)
