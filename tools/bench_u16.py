#!/usr/bin/env python3
"""What the 16-bit door costs next to the 8-bit one, on one MI355X, one process, one 23-block HP engine.  One JSON line.

AOI leg: a 4096 x 4096 image through enhance_u8 (-> 16384 x 16384 x 3 u8) and the same-size uint16 image through enhance_u16
(-> u16), host to host, a host clock around calls that end in a device synchronise.  Both get `--warmup` calls, then `--runs`
timed calls each, ALTERNATING (u8, u16, u8, ...), so clock drift and the neighbours on the host hit both alike.  The 16-bit
route writes the windows' fp32 tiles and reads them again in the fused paste + quantise kernel: 12 + 12 B per output pixel
against the u8 door's 3 + 3, and copies 6 B per output pixel to the host instead of 3.

Headline leg: forward_batch_u8_dev on 32 x 256^2 tiles (device to device, HIP events), the figure bench.py reports -- to show
that the 8-bit path did not move against the parent commit measured the same day on the same box.

    python tools/bench_u16.py [--runs 5] [--warmup 2] [--size 4096] [--steps 10] [--out profiles/u16_bench_line.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=23)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: at least 5 timed runs")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    eng = native.Engine(num_block=a.blocks, precision=native.PREC_F16_HP)
    eng.load_state_dict(synthetic_state_dict(a.blocks, seed=0))
    S = a.size
    reps = -(-S // 1024)
    img8 = np.ascontiguousarray(np.tile(synthetic_tiles(1, 1024, seed=99)[0], (reps, reps, 1))[:S, :S])
    # the same scene at 12 bits of radiometry (Sentinel-2's), range = the image's own min / max as app.wow_sr picks it
    img16 = (img8.astype(np.uint16) << 4) | (img8.astype(np.uint16) >> 4)
    lo, hi = int(img16.min()), int(img16.max())

    def run8():
        return eng.enhance_u8(img8)

    def run16():
        return eng.enhance_u16(img16, lo, hi)

    def clock(fn):
        t0 = time.perf_counter()
        o = fn()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, o.shape, o.dtype

    for _ in range(a.warmup):
        run8()
        run16()
    t8, t16 = [], []
    for i in range(a.runs):
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            ms, shape, dt = clock(run16 if which else run8)
            assert shape == (4 * S, 4 * S, 3) and dt == (np.uint16 if which else np.uint8)
            (t16 if which else t8).append(ms)
    opx = 16.0 * S * S

    def leg(t):
        med = statistics.median(t)
        return {"ms_per_run": [round(v, 1) for v in t], "ms_median": round(med, 1), "ms_min": round(min(t), 1),
                "spread_pct": round(100.0 * (max(t) - min(t)) / med, 2), "sr_mp_s": round(opx / (med / 1e3) / 1e6, 1)}

    res = {"metric": "u16_door", "blocks": a.blocks, "precision": "hp", "size": S, "runs": a.runs, "warmup": a.warmup,
           "value_range": [lo, hi], "enhance_u8": leg(t8), "enhance_u16": leg(t16)}
    res["u16_over_u8"] = round(res["enhance_u16"]["ms_median"] / res["enhance_u8"]["ms_median"], 4)
    # bytes the 16-bit route moves beyond the u8 one, from shapes: fp32 tiles written + read (the windows' output incl. halos is
    # (276/256)^2 of the image at the default plan) against u8 tiles written + read, and the wider image out
    halo = (276.0 / 256.0) ** 2 if S * S > 256 * 256 * 4 else 1.0
    res["extra_device_GB_estimate"] = round(opx * 3 * halo * (4 + 4 - 1 - 1) / 1e9 + opx * 3 * (2 - 1) / 1e9, 2)
    res["extra_host_copy_GB"] = round(opx * 3 * (2 - 1) / 1e9 + S * S * 3 / 1e9, 2)

    # headline: 32 x 256^2 u8 tiles, device to device on a side stream (graphs replay), HIP events
    B = 32
    side = torch.cuda.Stream(device=dev)
    x = torch.from_numpy(synthetic_tiles(B, 256, seed=1234)).to(dev)
    out = torch.empty((B, 1024, 1024, 3), dtype=torch.uint8, device=dev)

    def step():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(side)
        eng.forward_batch_u8_dev(x.data_ptr(), B, 256, 256, out.data_ptr(), side.cuda_stream)
        e1.record(side)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(3):
        step()
    ms = [step() for _ in range(a.steps)]
    med = statistics.median(ms)
    res["forward_batch_u8_32x256"] = {"steps": a.steps, "step_ms_median": round(med, 3), "step_ms_min": round(min(ms), 3),
                                      "spread_pct": round(100.0 * (max(ms) - min(ms)) / med, 2),
                                      "sr_mp_s": round(B * 1024 * 1024 / (med / 1e3) / 1e6, 1)}
    eng.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
