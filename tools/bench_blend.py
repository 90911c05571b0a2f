#!/usr/bin/env python3
"""What the seam-blended stitch costs next to the default door, on one MI355X, one process, one 23-block HP engine.  One JSON line.

A 4096 x 4096 image through enhance_u8 and through enhance_blend_u8 (both -> 16384 x 16384 x 3 u8), host to host, a host clock
around calls that end in a device synchronise.  Both get `--warmup` calls, then `--runs` timed calls each, ALTERNATING (u8, blend,
u8, ...), so clock drift and the neighbours on the host hit both alike.  The blend route is the 16-bit door's: the windows' fp32
tiles are written and read again by the paste kernel (12 + 12 B per output pixel against the u8 door's 3 + 3); inside the ramps
the kernel reads a second (row or column ramp) or four (where they cross) windows, and one window row per chunk is copied
forward on the device.

    python tools/bench_blend.py [--runs 5] [--warmup 2] [--size 4096] [--out profiles/blend_bench_line.json]
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
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: at least 5 timed runs")
    eng = native.Engine(num_block=a.blocks, precision=native.PREC_F16_HP)
    eng.load_state_dict(synthetic_state_dict(a.blocks, seed=0))
    S = a.size
    reps = -(-S // 1024)
    img = np.ascontiguousarray(np.tile(synthetic_tiles(1, 1024, seed=99)[0], (reps, reps, 1))[:S, :S])

    def clock(fn):
        t0 = time.perf_counter()
        o = fn(img)
        ms = (time.perf_counter() - t0) * 1e3
        assert o.shape == (4 * S, 4 * S, 3) and o.dtype == np.uint8
        return ms

    for _ in range(a.warmup):
        eng.enhance_u8(img)
        eng.enhance_blend_u8(img)
    t8, tb = [], []
    for i in range(a.runs):
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            (tb if which else t8).append(clock(eng.enhance_blend_u8 if which else eng.enhance_u8))
    opx = 16.0 * S * S

    def leg(t):
        med = statistics.median(t)
        return {"ms_per_run": [round(v, 1) for v in t], "ms_median": round(med, 1), "ms_min": round(min(t), 1),
                "spread_pct": round(100.0 * (max(t) - min(t)) / med, 2), "sr_mp_s": round(opx / (med / 1e3) / 1e6, 1)}

    res = {"metric": "blend_door", "blocks": a.blocks, "precision": "hp", "size": S, "runs": a.runs, "warmup": a.warmup,
           "enhance_u8": leg(t8), "enhance_blend_u8": leg(tb)}
    res["blend_over_u8"] = round(res["enhance_blend_u8"]["ms_median"] / res["enhance_u8"]["ms_median"], 4)
    # the pixels inside a ramp, from the plan: the share of output rows / columns with a weight
    rows, cols = native.plan_blend(S, S, 256, 10)
    fy, fx = float((rows[:, 4] != 0).mean()), float((cols[:, 4] != 0).mean())
    res["ramp_pixel_share"] = round(fy + fx - fy * fx, 4)
    # bytes beyond the u8 route, from shapes: fp32 tiles written + read (the windows' output incl. halos is (276/256)^2 of the image
    # at the default plan) against u8 tiles written + read, plus the second / fourth window read inside the ramps
    halo = (276.0 / 256.0) ** 2 if S * S > 256 * 256 * 4 else 1.0
    res["extra_device_GB_estimate"] = round(opx * 3 * (halo * (4 + 4 - 1 - 1) + 4 * (fy + fx + fy * fx)) / 1e9, 2)
    eng.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
