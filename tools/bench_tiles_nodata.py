#!/usr/bin/env python3
"""What the validity mask costs the reprojection warp, on one MI355X, one process, one weightless engine.  One JSON line.

tools/bench_tiles.py's raster (4096 x 4096 smooth + noise, UTM 2.5 m -> EPSG:3857) through warp_bilinear_u8 three ways: plain,
with a mask that is valid everywhere (the price of asking: four mask bytes per pixel and the all-valid test), and with a diagonal
edge that leaves 30 % of the source invalid (the mixed branch along the edge, the early out behind it).  The mask is the job's:
input resolution, valid_scale = 4.  `--warmup` calls each, then `--runs` timed calls, ALTERNATING (plain, all-valid, edge, then
rotated).  Two clocks per call: the kernel between its HIP events (the engine's profiling mode brackets the one launch) and the
host clock around the call (upload of 50 MB + the mask, kernel, 70 MB back).  The yardstick is the plain warp in the same process.

    python tools/bench_tiles_nodata.py [--runs 5] [--warmup 2] [--size 4096] [--out profiles/tiles_nodata_bench_line.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (str(REPO / "sentinel2-super-resolution-poc_amd"), str(REPO)):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from s2sr import geo, native, tiles  # noqa: E402

VS = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    S = a.size
    eng = native.Engine(num_block=1)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:S, 0:S]
    rgb = np.clip(np.stack([110 + 70 * np.sin(xx / 93.0 + c) * np.cos(yy / 67.0) for c in range(3)], -1) + rng.integers(-6, 7, (S, S, 3)),
                  0, 255).astype(np.uint8)
    plan = tiles.plan_warp(S, S, geo.Placement(600000.0, 5100000.0, 2.5, 2.5), geo.CRS(32633))
    M = -(-S // VS)
    my, mx = np.ogrid[:M, :M]
    all_valid = np.ones((M, M), np.uint8)
    edge = ((my + mx) * 1000 >= 775 * M).astype(np.uint8)          # the corner below y + x = 0.775: 0.775^2 / 2 = 30 % invalid
    warp = lambda **kw: eng.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w, **kw)      # noqa: E731
    legs = {"plain": lambda: warp(), "masked_all_valid": lambda: warp(valid=all_valid, valid_scale=VS),
            "masked_edge_30pct": lambda: warp(valid=edge, valid_scale=VS)}
    names = list(legs)
    same_bytes = bool(np.array_equal(legs["plain"](), legs["masked_all_valid"]()))
    alpha0 = {n: round(float((np.asarray(legs[n]())[..., 3] == 0).mean()), 4) for n in names}
    eng.set_profiling(1)

    def clock(fn):
        eng.reset_kernel_stats()
        t0 = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t0) * 1e3
        st = eng.kernel_stats()["misc"]
        assert int(st["launches"]) == 1, st
        return ms, float(st["total_ms"])

    for _ in range(a.warmup):
        for n in names:
            legs[n]()
    t = {n: [] for n in names}
    for i in range(a.runs):
        for k in range(len(names)):
            n = names[(i + k) % len(names)]
            t[n].append(clock(legs[n]))
    eng.set_profiling(0)
    eng.close()
    opx = float(plan.out_h) * plan.out_w

    def leg(v):
        call, kern = [x[0] for x in v], [x[1] for x in v]
        km = statistics.median(kern)
        return {"kernel_ms_per_run": [round(x, 4) for x in kern], "kernel_ms_median": round(km, 4),
                "kernel_spread_pct": round(100.0 * (max(kern) - min(kern)) / km, 2),
                "kernel_gb_s": round((opx * 16.0) / (km / 1e3) / 1e9, 1),          # 4 B out + 12 B of taps per output pixel, as the engine counts it
                "call_ms_per_run": [round(x, 3) for x in call], "call_ms_median": round(statistics.median(call), 3),
                "call_spread_pct": round(100.0 * (max(call) - min(call)) / statistics.median(call), 2)}

    res = {"metric": "tiles_nodata_warp", "size": S, "raster": [plan.out_h, plan.out_w], "valid_scale": VS, "runs": a.runs, "warmup": a.warmup,
           "invalid_share_edge": round(float((edge == 0).mean()), 4), "alpha0_share": alpha0, "all_valid_equals_plain_bytes": same_bytes}
    for n in names:
        res[n] = leg(t[n])
    for clk in ("kernel", "call"):
        base = res["plain"][f"{clk}_ms_median"]
        res[f"all_valid_over_plain_{clk}"] = round(res["masked_all_valid"][f"{clk}_ms_median"] / base, 4)
        res[f"edge_over_plain_{clk}"] = round(res["masked_edge_30pct"][f"{clk}_ms_median"] / base, 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
