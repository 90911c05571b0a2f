#!/usr/bin/env python3
"""SRVGGNetCompact (realesr-general-x4v3 shape, num_conv 32; --num-conv 16: realesr-animevideov3) on one MI355X.  One JSON line.

Batch leg: B x 256^2 u8 tiles -> B x 1024^2 u8 on the device (forward_batch_u8_dev on a real stream, graphs replay), timed per
step with HIP events around a device synchronise; `--repeats` repeats of `--steps` steps give the spread.  Group sweep: the same
leg with launch groups of 4 / 8 / 16 / 32 images (two 64-channel fp16 tensors of a group: 67 / 134 / 268 / 537 MB against an
Infinity Cache of ~256 MB), the groups interleaved step by step so clock drift hits all alike.  AOI leg: a 4096 x 4096 image
through enhance_u8, host to host.  Kernel statistics: one profiled step (HIP events around every launch), per family time and
the achieved FLOP/s and bytes/s from the algorithmic counts.

    python tools/bench_compact.py [--steps 20] [--warmup 3] [--batch 32] [--repeats 3] [--num-conv 32] [--no-aoi] [--no-sweep]
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
from s2sr.weights import synthetic_compact_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--num-conv", type=int, default=32, choices=(16, 32))
    ap.add_argument("--no-aoi", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--no-kstats", action="store_true", help="a profiler run: the timed steps only")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(side)
    st = side.cuda_stream
    B, nc = a.batch, a.num_conv
    sd = synthetic_compact_state_dict(nc, seed=0)
    x = torch.from_numpy(synthetic_tiles(B, 256, seed=1234)).to(dev)
    out = torch.empty((B, 1024, 1024, 3), dtype=torch.uint8, device=dev)

    def make(group):
        e = native.Engine(num_block=nc, precision=native.PREC_F16_HP, arch="compact", group=group)
        e.load_state_dict(sd)
        return e

    def timed(e):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(side)
        e.forward_batch_u8_dev(x.data_ptr(), B, 256, 256, out.data_ptr(), st)
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    mp = lambda ms: round(B * 1024 * 1024 / (ms / 1e3) / 1e6, 1)
    res = {"metric": "compact_sr", "num_conv": nc, "batch": B, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
           "out_px_per_step": B * 1024 * 1024}
    eng = make(0)
    res["default_group"] = eng.group_images()
    for _ in range(a.warmup):
        timed(eng)
    reps = []
    for _ in range(a.repeats):
        ms = [timed(eng) for _ in range(a.steps)]
        reps.append(statistics.median(ms))
    res["tiles_32x256"] = {"step_ms_median_per_repeat": [round(v, 3) for v in reps], "sr_mp_s_per_repeat": [mp(v) for v in reps],
                           "sr_mp_s": mp(statistics.median(reps)), "spread_pct": round(100.0 * (max(reps) - min(reps)) / statistics.median(reps), 2)}
    if not a.no_sweep:
        groups = [g for g in (4, 8, 16, 32) if g <= B]
        engs = {g: make(g) for g in groups}
        for g in groups:
            for _ in range(a.warmup):
                timed(engs[g])
        ms = {g: [] for g in groups}
        for i in range(a.steps):
            for g in (groups if i % 2 == 0 else groups[::-1]):
                ms[g].append(timed(engs[g]))
        res["group_sweep"] = {str(g): {"step_ms_median": round(statistics.median(ms[g]), 3), "step_ms_min": round(min(ms[g]), 3),
                                       "sr_mp_s": mp(statistics.median(ms[g])),
                                       "act_tensors_MB": round(g * 2 * 4 * 258 * 258 * 32 / 1e6, 1)} for g in groups}
        for e in engs.values():
            e.close()
    if not a.no_kstats:
        eng.set_profiling(1)
        eng.reset_kernel_stats()
        eng.forward_batch_u8_dev(x.data_ptr(), B, 256, 256, out.data_ptr(), st)
        torch.cuda.synchronize()
        kst = eng.kernel_stats()
        eng.set_profiling(0)
        res["kstats"] = {k: {"launches": v["launches"], "ms": round(v["total_ms"], 4), "TFLOP_s": round(v["flops"] / (v["total_ms"] / 1e3) / 1e12, 1),
                             "TB_s": round(v["bytes"] / (v["total_ms"] / 1e3) / 1e12, 3), "GFLOP": round(v["flops"] / 1e9, 2),
                             "GB": round(v["bytes"] / 1e9, 3)} for k, v in kst.items() if v["launches"] and v["total_ms"] > 0}
    if not a.no_aoi:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        img = synthetic_tiles(1, 1024, seed=99)[0]
        img = np.ascontiguousarray(np.tile(img, (4, 4, 1)))           # 4096 x 4096 in, 16384 x 16384 out
        eng.enhance_u8(img)
        t = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            o = eng.enhance_u8(img)
            t.append((time.perf_counter() - t0) * 1e3)
        assert o.shape == (16384, 16384, 3)
        med = statistics.median(t)
        res["enhance_4096"] = {"ms_per_repeat": [round(v, 1) for v in t], "ms_median": round(med, 1),
                               "sr_mp_s": round(16384 * 16384 / (med / 1e3) / 1e6, 1)}
    eng.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
