#!/usr/bin/env python3
"""What segmenting an index raster into fields costs on one MI355X, one process, one engine without weights.
One JSON line.

The raster is 16384 x 16384 (`--size`): a synthetic NDVI of 128 x 128 fields of jittered extent, 0.6 inside and 0.1 between them,
with Gaussian noise of 0.08 on every pixel, speckle, and nodata holes.  `--warmup` calls, then `--runs` timed calls, medians:

  kernels       the pass's launches by HIP events (the engine's profiling mode, every launch bracketed): their sum, and the split
                by stage (mask and morphology, local, border, flatten, the numbering's count, scan and apply, labels and boxes;
                native.Engine.fields_stage_ms), for the job's default parameters, with the morphology off and under conn 8; next to
                a device-to-device copy, timed by events in the same run, of the bytes the call must move (2 B/px of index in,
                2 B/px of labels out; a copy of n bytes moves 2 n)
  call          fields_segment_i16 host to host: the upload, the kernels, labels and fields on their way out, by a host clock
  trace         labels_trace_u16 of those labels (host code)
  index_zonal   index_nd_u16 with zonal sums from those labels (two uint16 planes from the host, `want=("zonal",)`): what a job pays
                once more per index
  scipy         scipy.ndimage.label of the raw threshold mask (no open, no close, no size filter) on the host, for scale only, where scipy is importable

    python tools/bench_fields.py [--runs 5] [--warmup 2] [--size 16384] [--out profiles/fields_bench_line.json]
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

K = 10000


def scene(S: int, n: int = 128, seed: int = 7) -> np.ndarray:
    """-> int16 [S, S]: n x n noisy fields"""
    rng = np.random.default_rng(seed)
    step = S // n
    idx = np.full((S, S), 0.1 * K, np.float32)
    for i in range(n):
        for j in range(n):
            a, b, c, d = rng.integers(step // 16, step // 5, 4)
            idx[i * step + a:(i + 1) * step - b, j * step + c:(j + 1) * step - d] = 0.6 * K
    for y0 in range(0, S, 2048):                                  # the noise in bands: no second full-size float array
        idx[y0:y0 + 2048] += rng.normal(0.0, 0.08 * K, idx[y0:y0 + 2048].shape).astype(np.float32)
    out = np.clip(np.rint(idx), -K, K).astype(np.int16)
    del idx
    holes = rng.integers(0, S, (S // 8, 2))
    for y, x in holes:
        out[y:y + 3, x:x + 3] = -32768
    return out


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
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: at least 5 timed runs")
    S = a.size
    eng = native.Engine(num_block=1, precision=native.PREC_F16_HP)
    idx = scene(S)
    kw = dict(r_open=1, r_close=2, conn=4, min_pixels=800)
    res = {"metric": "fields_segment", "size": S, "lo": 3000, "parameters": kw, "runs": a.runs, "warmup": a.warmup}

    def call(**over):
        return eng.fields_segment_i16(idx, 3000, 32767, **dict(kw, **over))

    def leg(v):
        med = statistics.median(v)
        return {"ms_per_run": [round(x, 2) for x in v], "ms_median": round(med, 2), "ms_min": round(min(v), 2),
                "spread_pct": round(100.0 * (max(v) - min(v)) / med, 2)}

    def by_events(**over):
        ms, stages = [], {name: [] for name in native.FIELDS_STAGES}
        for _ in range(a.runs):
            eng.set_profiling(1)
            eng.reset_kernel_stats()
            call(**over)
            per = eng.fields_stage_ms()
            st = eng.kernel_stats()["index"]
            eng.set_profiling(0)
            ms.append(float(st["total_ms"]))
            for name, (t, _) in per.items():
                stages[name].append(t)
        assert sum(n for _, n in per.values()) == int(st["launches"])
        split = {name: {"ms_median": round(statistics.median(v), 3), "launches": per[name][1]} for name, v in stages.items()}
        return dict(leg(ms), launches=int(st["launches"]), stages=split)

    for _ in range(a.warmup):
        call()
    host = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        labels, fields, found = call()
        host.append((time.perf_counter() - t0) * 1e3)
    labels, fields = np.array(labels), np.array(fields)
    assert int(fields[:, 0].sum()) == S * S and 0 < found <= 65535
    res["found"] = int(found)
    res["fields"] = {"unlabelled": int(fields[0, 0]), "pixels_min": int(fields[1:found + 1, 0].min()), "pixels_max": int(fields[1:found + 1, 0].max())}
    res["call"] = leg(host)
    res["kernels"] = by_events()
    res["kernels_without_morphology"] = by_events(r_open=0, r_close=0)
    res["kernels_conn8"] = by_events(conn=8)
    tr = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        xy, ring_start, ring_label = eng.labels_trace_u16(labels, found)
        tr.append((time.perf_counter() - t0) * 1e3)
    res["trace"] = dict(leg(tr), vertices=int(len(xy)), rings=int(len(ring_label)))
    rng = np.random.default_rng(3)
    pa = rng.integers(0, 10000, (S, S), dtype=np.uint16)
    pb = rng.integers(0, 10000, (S, S), dtype=np.uint16)
    zon = []
    for _ in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        r = eng.index_nd_u16(pa, pb, zones=labels, Z=found, want=("zonal",))
        zon.append((time.perf_counter() - t0) * 1e3)
    assert int(r["zonal"][:, 0].sum()) + r["undefined"] == S * S
    res["index_zonal_call"] = leg(zon[a.warmup:])
    eng.close()
    del pa, pb
    c = copy_ms(2 * S * S)
    res["kernels"]["copy_same_bytes_ms"] = round(c, 3)
    res["kernels"]["over_copy"] = round(res["kernels"]["ms_median"] / c, 3)
    try:
        from scipy import ndimage
        t0 = time.perf_counter()
        _, n = ndimage.label((idx >= 3000) & (idx != -32768))
        res["scipy_label_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["scipy_components_of_the_raw_mask"] = int(n)
    except ImportError:
        res["scipy_label_ms"] = None
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
