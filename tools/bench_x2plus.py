#!/usr/bin/env python3
"""RealESRGAN_x2plus against x4 at equal output, in one process.  Prints one JSON line.

Batch leg: x4 on B x 256^2 and x2plus on B x 512^2 tiles (both hp, 23 blocks, u8 -> u8 on the device): the same B x 1024^2 output
pixels per step and the same trunk geometry.  After a warm-up of each shape the two alternate step by step; each step is timed
with HIP events on the launch stream around a device synchronise.  Then one profiled step of each (s2sr kernel statistics: the
pack_u8 and conv_first rows, and their share of the step).
AOI leg: a 2048^2 image through enhance_u8 at scale 2 against a 1024^2 image at scale 4 (both 4096^2 out), host to host.

    python tools/bench_x2plus.py [--steps 20] [--warmup 3] [--batch 32] [--only 2|4] [--no-aoi]
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
import torch  # noqa: E402

from s2sr import native  # noqa: E402
from s2sr.synth import synthetic_tiles  # noqa: E402
from s2sr.weights import synthetic_state_dict  # noqa: E402

LEGS = {4: 256, 2: 512}          # scale -> input tile: 1024^2 out, 256^2 trunk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--only", type=int, choices=(2, 4), default=0, help="run one scale only (a profiler run)")
    ap.add_argument("--no-aoi", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    side = torch.cuda.Stream(device=dev)        # a real stream: graphs replay on it
    torch.cuda.set_stream(side)
    st = side.cuda_stream
    B = a.batch
    scales = [a.only] if a.only else [4, 2]
    legs = {}
    for s in scales:
        e = native.Engine(num_block=23, precision=native.PREC_F16_HP, scale=s)
        e.load_state_dict(synthetic_state_dict(23, seed=0, scale=s))
        size = LEGS[s]
        x = torch.from_numpy(synthetic_tiles(B, size, seed=1234)).to(dev)
        out = torch.empty((B, size * s, size * s, 3), dtype=torch.uint8, device=dev)
        legs[s] = (e, x, out, size)

    def step(s):
        e, x, out, size = legs[s]
        e.forward_batch_u8_dev(x.data_ptr(), B, size, size, out.data_ptr(), st)

    for s in scales:
        for _ in range(a.warmup):
            step(s)
    torch.cuda.synchronize()
    ms = {s: [] for s in scales}
    for i in range(a.steps):
        for s in (scales if i % 2 == 0 else scales[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(side)
            step(s)
            e1.record(side)
            e1.synchronize()
            ms[s].append(e0.elapsed_time(e1))
    res = {"metric": "x2plus_vs_x4", "batch": B, "steps": a.steps, "warmup": a.warmup, "precision": "hp", "num_block": 23,
           "out_px_per_step": B * 1024 * 1024}
    for s in scales:
        med = statistics.median(ms[s])
        res[f"x{s}"] = {"tile": LEGS[s], "step_ms_median": round(med, 3), "step_ms_min": round(min(ms[s]), 3),
                        "step_ms_max": round(max(ms[s]), 3), "sr_mp_s": round(B * 1024 * 1024 / (med / 1e3) / 1e6, 1)}
    if len(scales) == 2:
        res["ratio_x2_over_x4"] = round(res["x2"]["sr_mp_s"] / res["x4"]["sr_mp_s"], 4)
    # one profiled step of each (events around every launch: its times are not the step's; the shares are)
    for s in scales:
        e = legs[s][0]
        e.set_profiling(1)
        e.reset_kernel_stats()
        step(s)
        torch.cuda.synchronize()
        kst = e.kernel_stats()
        e.set_profiling(0)
        tot = sum(v["total_ms"] for v in kst.values())
        rows = {k: {"launches": v["launches"], "ms": round(v["total_ms"], 4), "GB": round(v["bytes"] / 1e9, 4)}
                for k, v in kst.items() if k in ("pack_u8", "conv_first")}
        res[f"x{s}"]["kstats"] = rows
        res[f"x{s}"]["launches"] = {k: v["launches"] for k, v in kst.items() if v["launches"]}
        res[f"x{s}"]["pack_plus_first_share"] = round((kst["pack_u8"]["total_ms"] + kst["conv_first"]["total_ms"]) / tot, 5) if tot else None
    if len(scales) == 2:
        res["same_launch_counts"] = res["x2"]["launches"] == res["x4"]["launches"]
    if not a.no_aoi and not a.only:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        aoi = {}
        for s, side_px in ((4, 1024), (2, 2048)):
            e = legs[s][0]
            img = synthetic_tiles(1, side_px, seed=99)[0]
            e.enhance_u8(img)                                        # warm-up: workspace, graphs
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                o = e.enhance_u8(img)
                t.append((time.perf_counter() - t0) * 1e3)
            assert o.shape == (4096, 4096, 3)
            med = statistics.median(t)
            aoi[f"x{s}"] = {"in": side_px, "ms_median": round(med, 2), "out_mp_s": round(4096 * 4096 / (med / 1e3) / 1e6, 1)}
        aoi["ratio_x2_over_x4"] = round(aoi["x2"]["out_mp_s"] / aoi["x4"]["out_mp_s"], 4)
        res["aoi_4096_out"] = aoi
    for s in scales:
        legs[s][0].close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
