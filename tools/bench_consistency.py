#!/usr/bin/env python3
"""What the radiometric consistency pass costs next to the plain doors, on one MI355X, one process, one 23-block HP
engine.  One JSON line.

A 4096 x 4096 image through enhance_u8 and through enhance_consistent_u8 in both modes, and the same for the 16-bit pair
(enhance_u16 / enhance_consistent_u16): -> 16384 x 16384 x 3, host to host, a host clock around calls that end in a device
synchronise.  Each leg gets `--warmup` calls, then `--runs` timed calls, ALTERNATING (the legs in order, then rotated), so clock
drift and the neighbours on the host hit all alike; medians are reported.  The yardstick of a consistent leg is the plain door of
its sample type in the same process; the spread of this kind of measurement is 0.3-0.4 % (profiles/blend_bench_line.json).
The pass's kernels are also timed on their own by HIP events (the engine's profiling mode: every launch of the family
bracketed), in calls outside the timed ones, next to a device-to-device copy of an image of the same bytes timed by events in
the same run: by bytes the pass moves ~2x what the copy moves in mode 1 (read + write, plus 1 / 16 for the input) and ~3x in
mode 2 (the residual launch reads the image once more).

    python tools/bench_consistency.py [--runs 5] [--warmup 2] [--size 4096] [--out profiles/consistency_bench_line.json]
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


def copy_ms(nbytes: int, reps: int = 7):
    """Median time of a device-to-device copy of nbytes, by events."""
    import torch
    a = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    ms = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return statistics.median(ms[2:])


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
    img16 = img.astype(np.uint16) * 40 + 100                        # 100 .. 10300, the 16-bit tests' range
    lo, hi = 100, 10300
    legs = {"enhance_u8": lambda: eng.enhance_u8(img),
            "consistent_u8_exact": lambda: eng.enhance_consistent_u8(img, 1)[0],
            "consistent_u8_smooth": lambda: eng.enhance_consistent_u8(img, 2)[0],
            "enhance_u16": lambda: eng.enhance_u16(img16, lo, hi),
            "consistent_u16_exact": lambda: eng.enhance_consistent_u16(img16, lo, hi, 1)[0],
            "consistent_u16_smooth": lambda: eng.enhance_consistent_u16(img16, lo, hi, 2)[0]}
    names = list(legs)

    def clock(fn):
        t0 = time.perf_counter()
        o = fn()
        ms = (time.perf_counter() - t0) * 1e3
        assert o.shape == (4 * S, 4 * S, 3)
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

    res = {"metric": "consistency_door", "blocks": a.blocks, "precision": "hp", "size": S, "runs": a.runs, "warmup": a.warmup}
    for n in names:
        res[n] = leg(t[n])
    for n in names:
        if n.startswith("consistent"):
            base = res["enhance_u8" if "_u8_" in n else "enhance_u16"]["ms_median"]
            res[n]["over_plain"] = round(res[n]["ms_median"] / base, 4)
    # the pass's kernels by HIP events (every launch bracketed), one call per leg, and the copy of the same bytes
    eng.set_profiling(1)
    for n in names:
        if not n.startswith("consistent"):
            continue
        eng.reset_kernel_stats()
        _, bad = (eng.enhance_consistent_u8(img, 1 + n.endswith("smooth")) if "_u8_" in n else
                  eng.enhance_consistent_u16(img16, lo, hi, 1 + n.endswith("smooth")))
        st = eng.kernel_stats()["consistency"]
        res[n]["kernel"] = {"launches": int(st["launches"]), "total_ms": round(float(st["total_ms"]), 3)}
        res[n]["inexact_blocks"] = [int(v) for v in bad]
    eng.set_profiling(0)
    eng.close()
    for esz, tag in ((1, "u8"), (2, "u16")):
        c = copy_ms(int(opx) * 3 * esz)
        res[f"copy_{tag}_ms"] = round(c, 3)
        for mode in ("exact", "smooth"):
            k = res[f"consistent_{tag}_{mode}"]["kernel"]
            k["over_copy"] = round(k["total_ms"] / c, 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
