#!/usr/bin/env python3
"""What an NDVI on the SR grid costs next to the 16-bit door and one carried band, on one MI355X, one process, one
23-block HP engine.  One JSON line.

A 4096 x 4096 uint16 image through enhance_u16 alone; through enhance_u16 and one carry_band_u16 from the device copy; and through
both followed by index_nd_u16(a=None) -- the carried band against a channel of the device copy, with the int16 raster, its RGBA
rendering and its histogram coming back (-> 16384 x 16384, host to host, a host clock around calls that end in a device
synchronise).  Each leg gets `--warmup` calls, then `--runs` timed calls, ALTERNATING, medians reported; a leg's spread is
(max - min) / median of its timed calls.  The index call alone is also clocked (the carried band leaves the device and comes back:
its host round trip is most of the call), and the pass's kernel is timed on its own by HIP events (the engine's profiling mode,
every launch bracketed) in calls outside the timed ones, in four forms -- the raster alone, + RGBA, + histogram, + zonal sums --
next to device-to-device copies, timed by events in the same run, that move the same bytes (4 B/px read, 2 B/px written, 4 B/px more
with the RGBA: a copy of n bytes moves 2 n).

--plain-only: the enhance_u16 leg alone (it needs nothing of the pass: the yardstick for a build without it).

    python tools/bench_index.py [--runs 5] [--warmup 2] [--size 4096] [--out profiles/index_bench_line.json]
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
    K = 10000
    last = {}

    def plain():
        return eng.enhance_u16(img16, lo, hi)

    def with_band():
        with eng.chain_lock:
            out = eng.enhance_u16(img16, lo, hi)
            g, bad = eng.carry_band_u16(band, 4, lo=blo, hi=bhi, eps=eps)
        assert g.shape == (4 * S, 4 * S)
        return out

    def with_ndvi():
        from s2sr import index as xi
        if "lut" not in last:
            last["lut"] = xi.ramp_lut(xi.ramp_for("vegetation", K))
        with eng.chain_lock:
            out = eng.enhance_u16(img16, lo, hi)
            g, bad = eng.carry_band_u16(band, 4, lo=blo, hi=bhi, eps=eps)
            t0 = time.perf_counter()
            r = eng.index_nd_u16(None, g, ca=0, offset=0, K=K, lut=last["lut"], want=("index", "hist", "rgba"))
            last.setdefault("index_call_ms", []).append((time.perf_counter() - t0) * 1e3)
        assert r["index"].shape == (4 * S, 4 * S) and int(r["hist"].sum()) + r["undefined"] == 16 * S * S
        return out

    legs = {"enhance_u16": plain} if a.plain_only else {"enhance_u16": plain, "enhance_u16_one_band": with_band, "enhance_u16_one_band_ndvi": with_ndvi}
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
    last.pop("index_call_ms", None)
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

    res = {"metric": "index_door", "blocks": a.blocks, "precision": "hp", "size": S, "runs": a.runs, "warmup": a.warmup}
    for n in names:
        res[n] = leg(t[n])
    if not a.plain_only:
        res["enhance_u16_one_band_ndvi"]["over_one_band"] = round(res["enhance_u16_one_band_ndvi"]["ms_median"] / res["enhance_u16_one_band"]["ms_median"], 4)
        res["ndvi_ms"] = round(res["enhance_u16_one_band_ndvi"]["ms_median"] - res["enhance_u16_one_band"]["ms_median"], 1)
        res["index_call_ms"] = {"per_run": [round(x, 1) for x in last["index_call_ms"]], "median": round(statistics.median(last["index_call_ms"]), 1)}
        # the pass's kernel by HIP events (every launch bracketed), one call per form
        zones = np.zeros((S // 16, S // 16), np.uint16)
        zones[S // 64:S // 32, S // 64:S // 24] = 1
        zones[S // 40:, S // 30:] = 2
        forms = {"index": dict(want=("index",)), "index_rgba": dict(want=("index", "rgba")), "index_rgba_hist": dict(want=("index", "rgba", "hist")),
                 "index_rgba_hist_zonal": dict(want=("index", "rgba", "hist", "zonal"), zones=zones, zone_scale=64, Z=2)}
        res["kernel"] = {}
        with eng.chain_lock:
            eng.enhance_u16(img16, lo, hi)
            g = np.array(eng.carry_band_u16(band, 4, lo=blo, hi=bhi, eps=eps)[0])
            for name, kw in forms.items():
                eng.set_profiling(1)
                eng.reset_kernel_stats()
                eng.index_nd_u16(None, g, ca=0, K=K, lut=last["lut"], **kw)
                st = eng.kernel_stats()["index"]
                eng.set_profiling(0)
                res["kernel"][name] = {"launches": int(st["launches"]), "total_ms": round(float(st["total_ms"]), 3)}
    eng.close()
    if not a.plain_only:
        for name, moved in (("index", 6.0), ("index_rgba", 10.0)):
            c = copy_ms(int(opx * moved / 2))
            res["kernel"][name]["copy_same_bytes_ms"] = round(c, 3)
            res["kernel"][name]["over_copy"] = round(res["kernel"][name]["total_ms"] / c, 3)
        for name in ("index_rgba_hist", "index_rgba_hist_zonal"):
            res["kernel"][name]["over_copy"] = round(res["kernel"][name]["total_ms"] / res["kernel"]["index_rgba"]["copy_same_bytes_ms"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
