#!/usr/bin/env python3
"""What cutting touching fields apart costs on one MI355X, one process, one engine without weights.  One JSON line.

Two rasters of 16384 x 16384 (`--size`), each a synthetic NDVI of 128 x 128 noisy fields:
  apart      tools/bench_fields.py's scene: fields of jittered extent, 0.6 inside and 0.1 between them, noise of 0.08, nodata holes;
             split with the defaults (core 0.5, 2 pixels, no edge test)
  touching   every field fills its whole cell, so the raster is ONE blob of the mask: the fields alternate between 0.5 and 0.7 like
             a chess board, noise of 0.03, the same holes; split with an edge test of 0.04 index units per pixel behind a 3 x 3 box sum
`--warmup` calls, then `--runs` timed calls, medians:

  kernels    fields_split_i16's launches by HIP events (the engine's profiling mode, every launch bracketed): their sum, the split by
             stage with the launches of each (native.Engine.fields_split_stage_ms) and the rounds the two growths took; next to
             fields_segment_i16 on the same raster in the same process, and to a device-to-device copy, timed by events in the same
             run, of the bytes the call must move (2 B/px of index in, 2 B/px of labels out; a copy of n bytes moves 2 n)
  call       fields_split_i16 and fields_segment_i16 host to host: the upload, the kernels, labels and fields on their way out
  found      the fields with and without the split

    python tools/bench_fields_split.py [--runs 5] [--warmup 2] [--size 16384] [--out profiles/fields_split_bench_line.json]
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

from bench_fields import K, copy_ms, scene  # noqa: E402
from s2sr import native  # noqa: E402


def touching(S: int, n: int = 128, seed: int = 7) -> np.ndarray:
    """-> int16 [S, S]: n x n fields that fill their cells"""
    rng = np.random.default_rng(seed)
    step = S // n
    cell = (np.arange(S) // step)
    idx = np.where((cell[:, None] + cell[None, :]) % 2 == 0, 0.5 * K, 0.7 * K).astype(np.float32)
    for y0 in range(0, S, 2048):
        idx[y0:y0 + 2048] += rng.normal(0.0, 0.03 * K, idx[y0:y0 + 2048].shape).astype(np.float32)
    out = np.clip(np.rint(idx), -K, K).astype(np.int16)
    del idx
    for y, x in rng.integers(0, S, (S // 8, 2)):
        out[y:y + 3, x:x + 3] = -32768
    return out


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
    kw = dict(r_open=1, r_close=2, conn=4, min_pixels=800)
    res = {"metric": "fields_split", "size": S, "lo": 3000, "parameters": kw, "runs": a.runs, "warmup": a.warmup}

    def leg(v):
        med = statistics.median(v)
        return {"ms_per_run": [round(x, 2) for x in v], "ms_median": round(med, 2), "ms_min": round(min(v), 2),
                "spread_pct": round(100.0 * (max(v) - min(v)) / med, 2)}

    def by_events(call, stage_ms, names):
        ms, stages, rounds = [], {name: [] for name in names}, []
        for _ in range(a.runs):
            eng.set_profiling(1)
            eng.reset_kernel_stats()
            call()
            per = stage_ms()
            st = eng.kernel_stats()["index"]
            eng.set_profiling(0)
            ms.append(float(st["total_ms"]))
            for name in names:
                stages[name].append(per[name][0])
            rounds.append(per.get("rounds"))
        assert sum(per[name][1] for name in names) == int(st["launches"])
        split = {name: {"ms_median": round(statistics.median(v), 3), "launches": per[name][1]} for name, v in stages.items()}
        out = dict(leg(ms), launches=int(st["launches"]), stages=split)
        if rounds[0] is not None:
            out["growth_rounds_per_run"] = [list(r) for r in rounds]       # they may differ: a workgroup may meet its neighbour's round or the one before
        return out

    def host(call):
        for _ in range(a.warmup):
            call()
        v = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            r = call()
            v.append((time.perf_counter() - t0) * 1e3)
        return leg(v), r

    c = None
    for name, make, split in (("apart", scene, {"core_q": 500, "core_px": 2, "edge": 0, "edge_r": 1}),
                              ("touching", touching, {"core_q": 500, "core_px": 2, "edge": 400, "edge_r": 1})):
        idx = make(S)
        plain = lambda: eng.fields_segment_i16(idx, 3000, 32767, **kw)
        cut = lambda: eng.fields_split_i16(idx, 3000, 32767, split=split, **kw)
        one = {"split": split}
        one["call_segment"], (_, fields0, found0) = host(plain)
        one["call_split"], (_, fields1, found1) = host(cut)
        assert int(fields0[:, 0].sum()) == int(fields1[:, 0].sum()) == S * S
        one["found_segment"], one["found_split"] = int(found0), int(found1)
        n = min(int(found1), 65535)
        one["fields_split"] = {"unlabelled": int(fields1[0, 0]), "pixels_min": int(fields1[1:n + 1, 0].min()) if n else 0,
                               "pixels_max": int(fields1[1:n + 1, 0].max()) if n else 0}
        one["kernels_segment"] = by_events(plain, eng.fields_stage_ms, native.FIELDS_STAGES)
        one["kernels_split"] = by_events(cut, eng.fields_split_stage_ms, native.FSPLIT_STAGES)
        res[name] = one
        del idx
    eng.close()
    c = copy_ms(2 * S * S)
    res["copy_same_bytes_ms"] = round(c, 3)
    for name in ("apart", "touching"):
        res[name]["split_over_copy"] = round(res[name]["kernels_split"]["ms_median"] / c, 2)
        res[name]["segment_over_copy"] = round(res[name]["kernels_segment"]["ms_median"] / c, 2)
        res[name]["split_over_segment"] = round(res[name]["kernels_split"]["ms_median"] / res[name]["kernels_segment"]["ms_median"], 2)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
