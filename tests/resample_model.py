"""numpy int64 restatement of the resampled tile levels' pixel arithmetic (csrc/resample.hip): premultiply
on load, horizontal pass, vertical pass over the 8-bit intermediate, un-premultiply on store.  It takes tap tables and does not
build them (s2sr.tiles.plan_resample_axis does; the CPU test pins planner + this model to Pillow)."""
import numpy as np

SRC_RASTER, SRC_LEVEL = 0, 1
H, W = 37, 53


def source(seed=1) -> np.ndarray:
    """The tests' 37 x 53 RGBA source: noise over a smooth field, opaque but for a 4 x 4 hole and a 4 x 10 patch of random alpha."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    src = np.empty((H, W, 4), np.uint8)
    src[..., :3] = np.clip(120 + 90 * np.sin(xx / 5.0)[..., None] * np.cos(yy / 3.0)[..., None] + rng.integers(-40, 41, (H, W, 3)), 0, 255)
    src[..., 3] = 255
    src[10:14, 20:24, 3] = 0
    src[20:24, 5:15, 3] = rng.integers(0, 256, (4, 10))
    return src


def mosaic(level: np.ndarray) -> np.ndarray:
    """[ny, nx, 256, 256, 4] tiles -> [ny*256, nx*256, 4] pixels."""
    ny, nx = level.shape[:2]
    return level.transpose(0, 2, 1, 3, 4).reshape(ny * 256, nx * 256, 4)


def _pass(px: np.ndarray, first, count, coef) -> np.ndarray:
    """px [R, N, 4] int64, tables along axis 1 -> [R, n_out, 4] in 0..255."""
    first, count, coef = np.asarray(first, np.int64), np.asarray(count, np.int64), np.asarray(coef, np.int64)
    acc = np.full((px.shape[0], first.size, 4), 1 << 21, np.int64)
    for t in range(coef.shape[1]):
        used = t < count
        idx = np.where(used, first + t, 0)
        acc += np.where(used, coef[:, t], 0)[None, :, None] * px[:, idx, :]
    assert np.abs(acc).max() < 2 ** 31                      # what the entry's overflow bound promises the device
    return np.clip(acc >> 22, 0, 255)


def resample_pixels(src: np.ndarray, cols, rows) -> np.ndarray:
    """Steps 1-4 on a plain pixel array: [H, W, 4] uint8, not premultiplied -> [len(rows), len(cols), 4] uint8."""
    p = src.astype(np.int64)
    a = p[..., 3:4]
    m = p[..., :3] * a + 128
    p = np.concatenate([((m >> 8) + m) >> 8, a], -1)                                  # 1: premultiply
    h = _pass(p, *cols[:3])                                                           # 2: horizontal, stored as 8 bits
    v = _pass(h.transpose(1, 0, 2), *rows[:3]).transpose(1, 0, 2)                     # 3: vertical
    a = v[..., 3:4]
    c = np.where((a == 0) | (a == 255), v[..., :3], np.minimum(255, (255 * v[..., :3]) // np.maximum(a, 1)))   # 4: un-premultiply
    return np.concatenate([c, a], -1).astype(np.uint8)


def apply_tables(src_rgba: np.ndarray, src_kind: int, cols, rows, nx: int, ny: int) -> np.ndarray:
    """src_rgba: [H, W, 4] (SRC_RASTER) or [cny, cnx, 256, 256, 4] (SRC_LEVEL) uint8, not premultiplied; cols / rows:
    (first, count, coef[, K]) of nx*256 / ny*256 samples -> the level [ny, nx, 256, 256, 4] uint8."""
    out = resample_pixels(mosaic(src_rgba) if src_kind == SRC_LEVEL else src_rgba, cols, rows)
    assert out.shape[:2] == (ny * 256, nx * 256)
    return np.ascontiguousarray(out.reshape(ny, 256, nx, 256, 4).transpose(0, 2, 1, 3, 4))


def pillow_resize(src_rgba: np.ndarray, box, size, filter: str, opaque_rgb: bool = False) -> np.ndarray:
    """PIL.Image.resize(size, filter, box=box) of the source lying in a transparent plane -> [size[1], size[0], 4] uint8.
    Pillow refuses a box that leaves its image, so the source is pasted into a transparent canvas that holds the box plus the
    filter's support, and the box moves with it (by whole pixels: the arithmetic does not change).
    opaque_rgb: the source's colours go through Pillow's three-channel path (mode RGB on a black canvas) and its coverage through
    the one-channel path; Pillow's own RGBa -> RGBA conversion then divides the colours by the coverage."""
    from PIL import Image
    flt = {"lanczos": Image.Resampling.LANCZOS, "cubic": Image.Resampling.BICUBIC, "bilinear": Image.Resampling.BILINEAR}[filter]
    h, w = src_rgba.shape[:2]
    x0, y0, x1, y1 = box
    scale = max((x1 - x0) / size[0], (y1 - y0) / size[1], 1.0)
    pad = int(np.ceil(3.0 * scale)) + 2
    left, top = int(np.floor(min(x0, 0))) - pad, int(np.floor(min(y0, 0))) - pad
    right, bottom = int(np.ceil(max(x1, w))) + pad, int(np.ceil(max(y1, h))) + pad
    canvas = np.zeros((bottom - top, right - left, 4), np.uint8)
    canvas[-top:-top + h, -left:-left + w] = src_rgba
    moved = (x0 - left, y0 - top, x1 - left, y1 - top)
    if not opaque_rgb:
        return np.asarray(Image.fromarray(canvas, "RGBA").resize(size, flt, box=moved))
    assert (src_rgba[..., 3] == 255).all()
    rgb = np.asarray(Image.fromarray(np.ascontiguousarray(canvas[..., :3]), "RGB").resize(size, flt, box=moved))
    cov = np.asarray(Image.fromarray(np.ascontiguousarray(canvas[..., 3]), "L").resize(size, flt, box=moved))
    pre = Image.frombytes("RGBa", size, np.dstack([rgb, cov]).tobytes())
    return np.asarray(pre.convert("RGBA"))
