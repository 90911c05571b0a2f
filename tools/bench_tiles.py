#!/usr/bin/env python3
"""XYZ pyramid timing on one GPU: a 4096x4096 SR raster (UTM, 2.5 m) -> EPSG:3857 -> z10..18 tiles -> PNG files, the levels
kept on the device and encoded there.  Reports the engine calls and the kernel time from the HIP-event statistics.  The raster
is smooth + noise like an SR output (on pure noise every tile goes to the host encoder: stored blocks).

    bench_tiles.py [side] [--resampling average|lanczos|cubic|bilinear] [--min-zoom 10] [--max-zoom 18]

--resampling: "average" = tiles_base / tiles_overview (the default), a filter = tiles_resample_u8 for every level (csrc/resample.hip:
the deepest level from the raster, the others 2:1 from the level below); the bytes the two resample passes move are printed next
to their time."""
import argparse
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sentinel2-super-resolution-poc_amd"))
import numpy as np  # noqa: E402

from s2sr import geo, native, tiles  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=4096)
ap.add_argument("--resampling", default="average", choices=("average",) + tiles.FILTERS)
ap.add_argument("--min-zoom", type=int, default=10)
ap.add_argument("--max-zoom", type=int, default=18)
args = ap.parse_args()
side, resampling = args.side, args.resampling
e = native.Engine(num_block=1)
rng = np.random.default_rng(0)
yy, xx = np.mgrid[0:side, 0:side]
rgb = np.clip(np.stack([110 + 70 * np.sin(xx / 93.0 + c) * np.cos(yy / 67.0) for c in range(3)], -1) + rng.integers(-6, 7, (side, side, 3)), 0, 255).astype(np.uint8)
src = geo.Placement(600000.0, 5100000.0, 2.5, 2.5)
t0 = time.perf_counter()
plan = tiles.plan_warp(side, side, src, geo.CRS(32633))
t_plan = time.perf_counter() - t0
e.warp_bilinear_u8(rgb[:64, :64], plan.grid[:8, :8], plan.step, 32, 32)      # warm-up
e.set_profiling(1)
e.reset_kernel_stats()
t0 = time.perf_counter()
warped = e.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w)
t_warp = time.perf_counter() - t0
k_warp = e.kernel_stats()["misc"]["total_ms"]
levels = tiles.plan_levels(plan.placement.bounds(plan.out_w, plan.out_h), args.min_zoom, args.max_zoom)
import tempfile  # noqa: E402
out_dir = Path(tempfile.mkdtemp())
for warm in (True, False):
    e.reset_kernel_stats()
    t_lv = t_png = 0.0
    k_lv = k_png = 0.0
    ntiles = nfiles = 0
    prev = None
    moved = 0.0             # resample: bytes the two passes move, each byte once (source window + intermediate written, intermediate read + level written)
    for lv in levels:
        t0 = time.perf_counter()
        if resampling != "average":
            if prev is None:
                cols, rows = tiles.plan_resample_level(lv, tiles.level_box(lv, plan.placement), plan.out_w, plan.out_h, resampling)
                e.tiles_resample_u8(warped, cols, rows, lv.nx, lv.ny, fetch=False)
            else:
                cols, rows = tiles.plan_resample_level(lv, tiles.overview_box(lv, prev), prev.nx * 256, prev.ny * 256, resampling)
                e.tiles_resample_u8(None, cols, rows, lv.nx, lv.ny, level_shape=(prev.ny, prev.nx), on_device=True, fetch=False)
            used_c, used_r = cols[1] > 0, rows[1] > 0
            n_r = int((rows[0] + rows[1])[used_r].max() - rows[0][used_r].min()) if used_r.any() else 0
            n_c = int((cols[0] + cols[1])[used_c].max() - cols[0][used_c].min()) if used_c.any() else 0
            inter = n_r * lv.nx * 256 * 4
            moved += n_r * n_c * 4 + 2 * inter + lv.nx * lv.ny * 262144
        elif prev is None:
            e.tiles_base_u8(warped, *tiles.plan_base(lv, plan.placement, plan.out_w, plan.out_h), fetch=False)
        else:
            ox, oy = tiles.overview_offsets(lv, prev)
            e.tiles_overview_u8((prev.ny, prev.nx), ox, oy, lv.nx, lv.ny, on_device=True, fetch=False)
        t1 = time.perf_counter()
        k0 = e.kernel_stats()["misc"]["total_ms"]
        paths = [f"{out_dir}/{int(warm)}/{lv.zoom}/{lv.tminx + i}/{geo.xyz_row(lv.tmaxy - j, lv.zoom)}.png" for j in range(lv.ny) for i in range(lv.nx)]
        wrote = e.tiles_write_png(lv.nx, lv.ny, paths)
        t2 = time.perf_counter()
        k1 = e.kernel_stats()["misc"]["total_ms"]
        t_lv += t1 - t0
        t_png += t2 - t1
        k_png += k1 - k0
        ntiles += lv.nx * lv.ny
        nfiles += int(wrote.sum())
        prev = lv
    k_lv = e.kernel_stats()["misc"]["total_ms"] - k_png
import shutil  # noqa: E402
shutil.rmtree(out_dir, ignore_errors=True)
opx = plan.out_h * plan.out_w
print(f"source {side}x{side} -> EPSG:3857 {plan.out_w}x{plan.out_h}; plan {t_plan*1e3:.1f} ms")
print(f"warp: call {t_warp*1e3:.1f} ms (kernel {k_warp:.3f} ms = {opx*(4+12)/k_warp/1e6:.0f} GB/s at 16 B per output px)")
print(f"pyramid z{args.max_zoom}..{args.min_zoom} ({resampling}): {ntiles} tiles on the device, level kernels {k_lv:.3f} ms (calls {t_lv*1e3:.1f} ms); "
      f"whole pyramid {(t_lv + t_png)*1e3:.0f} ms")
if resampling != "average":
    print(f"resample passes: {moved/1e6:.0f} MB moved at one pass per byte = {moved/k_lv/1e6:.0f} GB/s over the level-kernel time")
print(f"PNG files: {nfiles} written in {t_png*1e3:.0f} ms; the two encoder kernels {k_png:.3f} ms = {ntiles*262144*2/k_png/1e6:.0f} GB/s at one read of the tile per kernel")
