"""The seam-blended stitch, restated in numpy from oracle.rrdbnet_ref.tile_plan alone (include/s2sr.h, s2sr_enhance_blend_*).

Per axis (rows: the windows of the plan's first column; columns: those of its first row), with s the scale, n the axis length in
LR pixels and [start_k, end_k) the input interval of window k:
  owner(o)   the last window in plan order whose paste interval contains output coordinate o (the overwrite rule)
  seams      S_1 < ... < S_m: where owner(o) and owner(o - 1) have different input intervals; S_0 = 0, S_{m+1} = s n
  r_j        min(pad s, (S_j - S_{j-1}) // 2, (S_{j+1} - S_j) // 2)
  ramp       o in [S_j - r_j, S_j + r_j): a = owner(S_j - 1), b = owner(S_j), ia = o - s start_a, ib = o - s start_b,
             w = float32(2 (o - S_j + r_j) + 1) / float32(4 r_j), the weight of b
  elsewhere  a = b = owner(o), w = 0
A table row is {a, ia, b, ib, num, den}; windows are numbered by their distinct input intervals (coincident windows of the plan
run once).  Plain numpy; nothing here touches the device."""
from __future__ import annotations

import functools

import numpy as np

from oracle import rrdbnet_ref as ref


def axis_windows(plan, tile, PW, axis):
    """[(start, end, o1, o2)] along axis 0 (rows: the plan's first column) or 1 (columns: its first row)."""
    nx = (PW + tile - 1) // tile
    picked = plan[::nx] if axis == 0 else plan[:nx]
    return [(r[0][2 * axis], r[0][2 * axis + 1], r[2][2 * axis], r[2][2 * axis + 1]) for r in picked]


def axis_table(wins, n, s, pad):
    """-> (table [s n, 6] int64, starts of the distinct windows, seams [(S, r)])."""
    N = s * n
    owner = np.full(N, -1)
    for k, (_, _, o1, o2) in enumerate(wins):
        owner[o1:o2] = k
    assert (owner >= 0).all()
    starts = []
    for st, _, _, _ in wins:
        if not starts or starts[-1] != st:
            starts.append(st)
    idx = {st: i for i, st in enumerate(starts)}
    assert len(idx) == len(starts)
    st_of = np.array([wins[k][0] for k in owner])
    S = [o for o in range(1, N) if st_of[o] != st_of[o - 1]]
    bounds = [0] + S + [N]
    tab = np.zeros((N, 6), np.int64)
    tab[:, 0] = tab[:, 2] = [idx[v] for v in st_of]
    tab[:, 1] = tab[:, 3] = np.arange(N) - s * st_of
    tab[:, 5] = 1
    seams = []
    for j in range(1, len(bounds) - 1):
        Sj = bounds[j]
        r = min(pad * s, (Sj - bounds[j - 1]) // 2, (bounds[j + 1] - Sj) // 2)
        seams.append((Sj, r))
        sa, sb = st_of[Sj - 1], st_of[Sj]
        for o in range(Sj - r, Sj + r):
            tab[o] = (idx[sa], o - s * sa, idx[sb], o - s * sb, 2 * (o - Sj + r) + 1, 4 * r)
    return tab, starts, seams


@functools.lru_cache(maxsize=None)
def axis_plan(n, tile, pad, s):
    """The table of an axis of length n (the other axis does not enter)."""
    plan = ref.tile_plan(n, n, tile, pad, s)
    tab, starts, seams = axis_table(axis_windows(plan, tile, n, 0), n, s, pad)
    tab.setflags(write=False)
    return tab, tuple(starts), tuple(seams)


def tables(PH, PW, tile, pad, s):
    """-> (rows [s PH, 6], cols [s PW, 6], row starts, column starts) of the PH x PW image the window job is planned on."""
    plan = ref.tile_plan(PH, PW, tile, pad, s)
    rows, ys, _ = axis_table(axis_windows(plan, tile, PW, 0), PH, s, pad)
    cols, xs, _ = axis_table(axis_windows(plan, tile, PW, 1), PW, s, pad)
    return rows, cols, ys, xs


def distinct_rects(PH, PW, tile, pad, s):
    """The distinct windows' input rectangles (y1, y2, x1, x2), row-major, and for every planned window its index among them."""
    plan = ref.tile_plan(PH, PW, tile, pad, s)
    _, _, ys, xs = tables(PH, PW, tile, pad, s)
    wh, ww = plan[0][0][1] - plan[0][0][0], plan[0][0][3] - plan[0][0][2]
    rects = [(y, y + wh, x, x + ww) for y in ys for x in xs]
    of_plan = [ys.index(r[0][0]) * len(xs) + xs.index(r[0][2]) for r in plan]
    return rects, of_plan


def weights(tab):
    return tab[:, 4].astype(np.float32) / tab[:, 5].astype(np.float32)      # one correctly rounded fp32 division


def blend(windows_f32, rows, cols, nx):
    """windows_f32 [ny nx, oh, ow, C] float32 (the distinct windows' outputs, row-major) -> [len(rows), len(cols), C] float32:
    top = A + wx (B - A), bot = C + wx (D - C), v = top + wy (bot - top), each operation rounded to float32, terms of weight 0
    left out."""
    w = np.asarray(windows_f32)
    assert w.dtype == np.float32
    wy, wx = weights(rows)[:, None, None], weights(cols)[None, :, None]

    def take(ry, rx):
        return w[rows[:, ry][:, None] * nx + cols[:, rx][None, :], rows[:, ry + 1][:, None], cols[:, rx + 1][None, :]]

    def lerp(p, q, t):
        return np.where(t == 0, p, p + t * (q - p)).astype(np.float32)

    top = lerp(take(0, 0), take(0, 2), wx)
    bot = lerp(take(2, 0), take(2, 2), wx)
    return lerp(top, bot, wy)


def in_ramp(rows, cols):
    """[len(rows), len(cols)] bool: the pixels inside a row ramp or a column ramp."""
    return (rows[:, 4] != 0)[:, None] | (cols[:, 4] != 0)[None, :]


# ---- two wrong models (the controls of the device test) ------------------------------------------------------------------------
def reversed_weights(tab):
    """The cross-fade run backwards: b weighs 1 - w."""
    t = np.array(tab)
    ramp = t[:, 4] != 0
    t[ramp, 4] = t[ramp, 5] - t[ramp, 4]
    return t


def shifted_ramp(tab, ext):
    """Every ramp moved one pixel up the axis (where both windows still cover it): entry o is entry o - 1 one pixel further into
    its windows; the pixel a ramp leaves falls back to its owner a."""
    t = np.array(tab)
    for o in range(len(tab) - 1, 0, -1):
        p = tab[o - 1]
        if p[4] != 0 and p[1] + 1 < ext and p[3] + 1 < ext:
            t[o] = (p[0], p[1] + 1, p[2], p[3] + 1, p[4], p[5])
        if p[4] != 0 and (o < 2 or tab[o - 2][4] == 0):
            t[o - 1] = (p[0], p[1], p[0], p[1], 0, 1)
    return t


def quant_u8(v):
    """The reference's rule as conv_last applies it: trunc(clip(fp32(v * 255), 0, 255))."""
    return np.clip(np.asarray(v, np.float32) * np.float32(255.0), 0, 255).astype(np.uint8)
