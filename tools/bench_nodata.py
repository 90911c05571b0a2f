#!/usr/bin/env python3
"""What the nodata-aware enhance costs next to the default door, on one MI355X, one process, one 23-block HP engine.  One JSON line.

A 4096 x 4096 image through enhance_u8, through enhance_masked_u8 with a mask that is valid everywhere (the fill and the mask
kernels run and find nothing to do: the price of asking) and through enhance_masked_u8 with a diagonal swath edge that leaves
about 30 % of the pixels invalid.  All -> 16384 x 16384 x 3 u8, host to host, a host clock around calls that end in a device
synchronise.  Each gets `--warmup` calls, then `--runs` timed calls, ALTERNATING (u8, all-valid, edge, then rotated), so clock drift
and the neighbours on the host hit all three alike.  The yardstick is enhance_u8 in the same process.  The fill and mask kernels
are also timed on their own by HIP events (the engine's profiling mode), in calls outside the timed ones.

    python tools/bench_nodata.py [--runs 5] [--warmup 2] [--size 4096] [--radius 32] [--out profiles/nodata_bench_line.json]
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

from s2sr import native  # noqa: E402
from s2sr.synth import synthetic_tiles  # noqa: E402
from s2sr.weights import synthetic_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=23)
    ap.add_argument("--radius", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: at least 5 timed runs")
    eng = native.Engine(num_block=a.blocks, precision=native.PREC_F16_HP)
    eng.load_state_dict(synthetic_state_dict(a.blocks, seed=0))
    S = a.size
    reps = -(-S // 1024)
    img = np.ascontiguousarray(np.tile(synthetic_tiles(1, 1024, seed=99)[0], (reps, reps, 1))[:S, :S])
    yy, xx = np.ogrid[:S, :S]
    all_valid = np.ones((S, S), np.uint8)
    edge = ((yy + xx) * 1000 >= 775 * S).astype(np.uint8)          # the corner below y / S + x / S = 0.775: 0.775^2 / 2 = 30 %
    img_edge = np.array(img)
    img_edge[edge == 0] = 0                                        # the raster as a file holds it
    legs = {"enhance_u8": lambda: eng.enhance_u8(img),
            "masked_all_valid": lambda: eng.enhance_masked_u8(img, all_valid, radius=a.radius),
            "masked_edge_30pct": lambda: eng.enhance_masked_u8(img_edge, edge, radius=a.radius)}
    names = list(legs)

    def clock(fn):
        t0 = time.perf_counter()
        o = fn()
        ms = (time.perf_counter() - t0) * 1e3
        assert o.shape == (4 * S, 4 * S, 3) and o.dtype == np.uint8
        return ms

    for _ in range(a.warmup):
        for n in names:
            legs[n]()
    t = {n: [] for n in names}
    for i in range(a.runs):
        for k in range(len(names)):
            n = names[(i + k) % len(names)]
            t[n].append(clock(legs[n]))
    opx = 16.0 * S * S

    def leg(v):
        med = statistics.median(v)
        return {"ms_per_run": [round(x, 1) for x in v], "ms_median": round(med, 1), "ms_min": round(min(v), 1),
                "spread_pct": round(100.0 * (max(v) - min(v)) / med, 2), "sr_mp_s": round(opx / (med / 1e3) / 1e6, 1)}

    res = {"metric": "nodata_door", "blocks": a.blocks, "precision": "hp", "size": S, "radius": a.radius, "runs": a.runs, "warmup": a.warmup,
           "invalid_share_edge": round(float((edge == 0).mean()), 4)}
    for n in names:
        res[n] = leg(t[n])
    base = res["enhance_u8"]["ms_median"]
    res["all_valid_over_u8"] = round(res["masked_all_valid"]["ms_median"] / base, 4)
    res["edge_over_u8"] = round(res["masked_edge_30pct"]["ms_median"] / base, 4)
    # the two kernels by HIP events: every launch of the two families bracketed, one call per mask
    eng.set_profiling(1)
    for n in names[1:]:
        eng.reset_kernel_stats()
        legs[n]()
        st = eng.kernel_stats()
        res[n]["kernel_ms"] = {k: {"launches": int(st[k]["launches"]), "total_ms": round(float(st[k]["total_ms"]), 3)}
                               for k in ("nodata_fill", "nodata_mask")}
    eng.set_profiling(0)
    eng.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
