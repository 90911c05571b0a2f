#!/usr/bin/env python3
"""What management zones (integer k-means inside every field) cost on one MI355X, one process, one engine without
weights.  One JSON line.

The raster is 16384 x 16384 (`--size`): the synthetic NDVI of 128 x 128 noisy fields of tools/bench_fields.py, segmented by the
engine with that tool's parameters, so the labels are the 16384 fields a job would find.  A second feature for D = 2 is the same
scene under another seed.  k = 3, min_per_zone 10, at most 32 iterations; D in (1, 2) x smooth in (0, 1).  `--warmup` calls, then
`--runs` timed calls, medians, per configuration:

  kernels       the pass's launches by HIP events (the engine's profiling mode, every launch bracketed): their sum, the split by
                stage (statistics, iterations, final assign, smoothing, table; native.Engine.mzones_stage_ms), the iterations run and
                the time of one (an assign-and-accumulate launch plus the centre update, a launch over 3 x 16385 cells), next to
                a device-to-device copy, timed by events in the same run, of the (2 D + 2) bytes per pixel that launch reads
                (a copy of n bytes moves 2 n)
  call          zones_kmeans_i16 host to host: the upload, the kernels, one host wait per iteration, the raster and the tables on
                their way out, by a host clock
  trace         the k labels_trace_u16 calls of where(zone == id, labels, 0) (host code), D = 1 and smooth 1 only
  sklearn       KMeans(n_clusters=3, random_state=42, n_init=10) on `--sklearn-fields` of the same fields one after the other, as
                the reference's per-polygon loop runs it, and that time scaled to all fields: for scale only, where scikit-learn is
                importable

    python tools/bench_mzones.py [--runs 5] [--warmup 2] [--size 16384] [--out profiles/mzones_bench_line.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (str(REPO / "sentinel2-super-resolution-poc_amd"), str(REPO), str(REPO / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from bench_fields import copy_ms, scene  # noqa: E402
from s2sr import native  # noqa: E402

K_ZONES = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--sklearn-fields", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: at least 5 timed runs")
    S = a.size
    eng = native.Engine(num_block=1, precision=native.PREC_F16_HP)
    feats = np.stack([scene(S), scene(S, seed=11)])
    labels, fields, found = eng.fields_segment_i16(feats[0], 3000, 32767, r_open=1, r_close=2, conn=4, min_pixels=800)
    labels, fields = np.array(labels), np.array(fields)
    assert 0 < found <= 65535
    kw = dict(k=K_ZONES, iters=32, min_per_zone=10)
    res = {"metric": "zones_kmeans", "size": S, "fields": int(found), "parameters": kw, "runs": a.runs, "warmup": a.warmup, "configs": {}}

    def leg(v):
        med = statistics.median(v)
        return {"ms_per_run": [round(x, 2) for x in v], "ms_median": round(med, 2), "ms_min": round(min(v), 2),
                "spread_pct": round(100.0 * (max(v) - min(v)) / med, 2)}

    last = None
    for D in (1, 2):
        for smooth in (0, 1):
            call = lambda: eng.zones_kmeans_i16(feats[:D], labels, found, smooth=smooth, **kw)       # noqa: E731
            for _ in range(a.warmup):
                call()
            host = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                r = call()
                host.append((time.perf_counter() - t0) * 1e3)
            ms, stages = [], {name: [] for name in native.MZONES_STAGES}
            for _ in range(a.runs):
                eng.set_profiling(1)
                eng.reset_kernel_stats()
                r = call()
                per = eng.mzones_stage_ms()
                st = eng.kernel_stats()["index"]
                eng.set_profiling(0)
                ms.append(float(st["total_ms"]))
                for name, (t, _) in per.items():
                    stages[name].append(t)
            assert sum(n for _, n in per.values()) == int(st["launches"])
            split = {name: {"ms_median": round(statistics.median(v), 3), "launches": per[name][1]} for name, v in stages.items()}
            status = np.asarray(r["status"])
            entry = {"call": leg(host), "kernels": dict(leg(ms), launches=int(st["launches"]), stages=split), "iterations": r["iterations"],
                     "zoned": int((status == 2).sum()), "skipped": int((status == 1).sum()),
                     "zone_pixels": [int(v) for v in np.asarray(r["table"])[:, :, 0].sum(axis=0)]}
            entry["kernels"]["iteration_ms"] = round(split["iterations"]["ms_median"] / r["iterations"], 3)
            res["configs"][f"D{D}_smooth{smooth}"] = entry
            if D == 1 and smooth == 1:
                last = np.array(r["zone"])
    tr = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        rings = [eng.labels_trace_u16(np.where(last == j, labels, 0).astype(np.uint16), found) for j in range(1, K_ZONES + 1)]
        tr.append((time.perf_counter() - t0) * 1e3)
    res["trace"] = dict(leg(tr), vertices=int(sum(len(x[0]) for x in rings)), rings=int(sum(len(x[2]) for x in rings)))
    eng.close()
    for D in (1, 2):
        c = copy_ms((2 * D + 2) * S * S)
        for smooth in (0, 1):
            kern = res["configs"][f"D{D}_smooth{smooth}"]["kernels"]
            kern["copy_same_bytes_ms"] = round(c, 3)
            kern["iteration_over_copy"] = round(kern["iteration_ms"] / c, 3)
    try:
        from sklearn.cluster import KMeans
        n = min(a.sklearn_fields, found)
        t0 = time.perf_counter()
        for l in range(1, n + 1):
            x0, y0, x1, y1 = (int(v) for v in fields[l, 2:6])
            inside = labels[y0:y1, x0:x1] == l
            v = feats[0, y0:y1, x0:x1][inside & (feats[0, y0:y1, x0:x1] != -32768)]
            if len(v) >= K_ZONES * 10:
                KMeans(n_clusters=K_ZONES, random_state=42, n_init=10).fit_predict(v.reshape(-1, 1).astype(np.float64))
        dt = (time.perf_counter() - t0) * 1e3
        res["sklearn"] = {"fields": n, "ms": round(dt, 1), "ms_per_field": round(dt / n, 2), "ms_scaled_to_all_fields": round(dt / n * found, 0)}
    except ImportError:
        res["sklearn"] = None
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
