#!/usr/bin/env python3
"""What carrying one extra band to the SR grid costs next to the 16-bit door, on one MI355X, one process, one
23-block HP engine.  One JSON line.

A 4096 x 4096 uint16 image through enhance_u16 alone, and through enhance_u16 followed by one carry_band_u16 from the device copy
(-> 16384 x 16384 x 3 and one 16384 x 16384 band, host to host, a host clock around calls that end in a device synchronise).  Each
leg gets `--warmup` calls, then `--runs` timed calls, ALTERNATING, medians reported; a leg's spread is (max - min) / median of its
timed calls.  The pass's two kernels are also timed on their own by HIP events (the engine's profiling mode: every launch of the
family bracketed), in a call outside the timed ones, next to a device-to-device copy of the band's output bytes timed by events in
the same run: by bytes the pass reads the guide twice (6 bytes per output sample each time, plus the halo of the coefficient
tiles) and writes 2, so ~7x what that copy moves one way.

--plain-only: the enhance_u16 leg alone (it needs nothing of the pass: the yardstick for a build without it).

    python tools/bench_bands.py [--runs 5] [--warmup 2] [--size 4096] [--out profiles/bands_bench_line.json]
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
    ap.add_argument("--plain-only", action="store_true", help="time enhance_u16 alone")
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
    rng = np.random.default_rng(5)
    band = (img16.sum(axis=2) // 4 + rng.integers(0, 400, (S, S))).astype(np.uint16)       # a band that follows the image loosely
    blo, bhi = int(band.min()), int(band.max())
    eps = max(1, ((bhi - blo) >> 8) ** 2)

    def plain():
        return eng.enhance_u16(img16, lo, hi)

    def with_band():
        with eng.chain_lock:
            out = eng.enhance_u16(img16, lo, hi)
            g, bad = eng.carry_band_u16(band, 4, lo=blo, hi=bhi, eps=eps)
        assert g.shape == (4 * S, 4 * S)
        return out

    legs = {"enhance_u16": plain} if a.plain_only else {"enhance_u16": plain, "enhance_u16_one_band": with_band}
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

    res = {"metric": "bands_door", "blocks": a.blocks, "precision": "hp", "size": S, "runs": a.runs, "warmup": a.warmup}
    for n in names:
        res[n] = leg(t[n])
    if not a.plain_only:
        res["enhance_u16_one_band"]["over_plain"] = round(res["enhance_u16_one_band"]["ms_median"] / res["enhance_u16"]["ms_median"], 4)
        res["band_ms"] = round(res["enhance_u16_one_band"]["ms_median"] - res["enhance_u16"]["ms_median"], 1)
        # the pass's kernels by HIP events (every launch bracketed), one call, and the copy of the band's output bytes
        with eng.chain_lock:
            eng.enhance_u16(img16, lo, hi)
            eng.set_profiling(1)
            eng.reset_kernel_stats()
            _, bad = eng.carry_band_u16(band, 4, lo=blo, hi=bhi, eps=eps)
            st = eng.kernel_stats()["bands"]
            eng.set_profiling(0)
        res["kernel"] = {"launches": int(st["launches"]), "total_ms": round(float(st["total_ms"]), 3)}
        res["band_range"], res["eps"], res["inexact_blocks"] = [blo, bhi], eps, int(bad)
    eng.close()
    if not a.plain_only:
        c = copy_ms(int(opx) * 2)
        res["copy_band_ms"] = round(c, 3)
        res["kernel"]["over_copy"] = round(res["kernel"]["total_ms"] / c, 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
