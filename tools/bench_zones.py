#!/usr/bin/env python3
"""What rasterising field polygons to zone labels costs on one MI355X, one process, one engine without weights.
One JSON line.

The label grid is 16384 x 16384 (`--size`).  The scene is a jittered mesh of 128 x 128 four-cornered fields with shared vertices
over the middle 94 % of the grid, behind one polygon of 2000 vertices around the whole scene (first in the list: the fields win).
`--warmup` calls, then `--runs` timed calls, medians:

  kernel        the pass's launches by HIP events (the engine's profiling mode, every launch bracketed), next to a device-to-device
                copy, timed by events in the same run, of the bytes the kernel writes (2 B/px; a copy of n bytes moves 2 n)
  call          zones_rasterize_u16 host to host: the tables' checks, the binning, the uploads, the kernel and the labels' way
                out, by a host clock; next to the binning-free part a caller pays today, a plain host-to-device upload of a label
                raster of that size (pageable and page-locked)
  index_zonal   index_nd_u16 with zonal sums from those labels (two uint16 planes from the host, `want=("zonal",)`)

    python tools/bench_zones.py [--runs 5] [--warmup 2] [--size 16384] [--out profiles/zones_bench_line.json]
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


def scene(S: int, n: int = 128, around: int = 2000, seed: int = 7):
    """-> (xy, ring_start, feat_start, label, Z): the polygon around everything (label Z), then n x n jittered quadrilaterals"""
    rng = np.random.default_rng(seed)
    U = 256 * S
    lo, hi = int(0.03 * U), int(0.97 * U)
    step = (hi - lo) // n
    gx, gy = np.meshgrid(lo + step * np.arange(n + 1), lo + step * np.arange(n + 1))
    jx, jy = (rng.integers(-(step // 3), step // 3 + 1, gx.shape) for _ in range(2))
    jx[:, [0, -1]] = 0
    jy[[0, -1], :] = 0
    vx, vy = gx + jx, gy + jy
    a = 2 * np.pi * np.arange(around) / around
    ring0 = np.stack([np.round(U / 2 + 0.8 * U * np.cos(a)), np.round(U / 2 + 0.8 * U * np.sin(a))], 1).astype(np.int32)
    quads = np.stack([np.stack([vx[:-1, :-1], vy[:-1, :-1]], -1), np.stack([vx[:-1, 1:], vy[:-1, 1:]], -1),
                      np.stack([vx[1:, 1:], vy[1:, 1:]], -1), np.stack([vx[1:, :-1], vy[1:, :-1]], -1)], 2).reshape(-1, 2).astype(np.int32)
    xy = np.ascontiguousarray(np.concatenate([ring0, quads]))
    F = 1 + n * n
    ring_start = np.concatenate([[0], around + 4 * np.arange(n * n + 1)]).astype(np.int32)
    feat_start = np.arange(F + 1, dtype=np.int32)
    label = np.concatenate([[F], 1 + np.arange(n * n)]).astype(np.uint16)
    return xy, ring_start, feat_start, label, F


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


def upload_ms(labels: np.ndarray, pinned: bool, runs: int, warmup: int):
    """Median host time of a host-to-device upload of the label raster, synchronised."""
    import torch
    src = torch.from_numpy(labels.view(np.int16))
    if pinned:
        src = src.pin_memory()
    dst = torch.empty(src.shape, dtype=src.dtype, device="cuda")
    ms = []
    for _ in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    del dst, src
    torch.cuda.empty_cache()
    return statistics.median(ms[warmup:])


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
    xy, ring_start, feat_start, label, Z = scene(S)
    res = {"metric": "zones_rasterize", "size": S, "features": int(len(label)), "vertices": int(len(xy)), "runs": a.runs, "warmup": a.warmup}

    def call():
        return eng.zones_rasterize_u16(xy, ring_start, feat_start, label, Z, (S, S))

    def leg(v):
        med = statistics.median(v)
        return {"ms_per_run": [round(x, 2) for x in v], "ms_median": round(med, 2), "ms_min": round(min(v), 2),
                "spread_pct": round(100.0 * (max(v) - min(v)) / med, 2)}

    for _ in range(a.warmup):
        call()
    host, kern = [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        out, area = call()
        host.append((time.perf_counter() - t0) * 1e3)
    labels, area = np.array(out), np.array(area)
    assert int(area.sum()) == S * S and int(area[0]) == 0 and int(area[Z]) > 0 and int((area[1:Z] > 0).sum()) == Z - 1
    for _ in range(a.runs):                                        # the kernel by events, in calls outside the timed ones
        eng.set_profiling(1)
        eng.reset_kernel_stats()
        call()
        st = eng.kernel_stats()["index"]
        eng.set_profiling(0)
        kern.append(float(st["total_ms"]))
    res["kernel"] = dict(leg(kern), launches=int(st["launches"]))
    bare = []
    for _ in range(a.runs):                                        # ... and without the area counters
        eng.set_profiling(1)
        eng.reset_kernel_stats()
        eng.zones_rasterize_u16(xy, ring_start, feat_start, label, Z, (S, S), want_area=False)
        bare.append(float(eng.kernel_stats()["index"]["total_ms"]))
        eng.set_profiling(0)
    res["kernel_without_area"] = leg(bare)
    res["call"] = leg(host)
    res["area"] = {"unlabelled": int(area[0]), "around": int(area[Z]), "fields_min": int(area[1:Z].min()), "fields_max": int(area[1:Z].max())}
    # the index call with zonal sums from these labels
    rng = np.random.default_rng(3)
    pa = rng.integers(0, 10000, (S, S), dtype=np.uint16)
    pb = rng.integers(0, 10000, (S, S), dtype=np.uint16)
    zon = []
    for i in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        r = eng.index_nd_u16(pa, pb, zones=labels, Z=Z, want=("zonal",))
        zon.append((time.perf_counter() - t0) * 1e3)
    assert int(r["zonal"][:, 0].sum()) + r["undefined"] == S * S
    res["index_zonal_call"] = leg(zon[a.warmup:])
    eng.close()
    del pa, pb
    c = copy_ms(2 * S * S)
    res["kernel"]["copy_same_bytes_ms"] = round(c, 3)
    res["kernel"]["over_copy"] = round(res["kernel"]["ms_median"] / c, 3)
    res["upload_pageable_ms"] = round(upload_ms(labels, False, a.runs, a.warmup), 2)
    res["upload_pinned_ms"] = round(upload_ms(labels, True, a.runs, a.warmup), 2)
    res["call"]["over_upload_pageable"] = round(res["call"]["ms_median"] / res["upload_pageable_ms"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
