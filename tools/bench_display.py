#!/usr/bin/env python3
"""What the display rendering of a 16-bit product costs, on one MI355X, one process.  One JSON line.

The image is the x4 product of a `--size` x `--size` AOI (default 4096: 16384 x 16384 x 3 uint16, 1.6 GB).  `--warmup` calls, then
`--runs` timed calls each (a host clock around calls that end in a device synchronise) of

  (a) host_image   display_hist_u16 + display_apply_u16 from a host image (render_u16: one upload, the 8-bit image back);
  (b) device_copy  the same two passes from the device copy enhance_u16 left (one enhance_u16 of a `--blocks`-block net in front,
                   not timed: the display calls leave the copy in place);
  (c) host_minmax  the host route used before, rasterio_lite._to_u8 on the same array (float64 numpy, global min-max).

Next to them each kernel's bytes over time from the handle's HIP-event statistics (profiling on in a separate pass, so that the
event pairs stay out of the timed calls), against the 6.3 TB/s device copy rate DESIGN.md quotes.

    python tools/bench_display.py [--runs 5] [--warmup 2] [--size 4096] [--blocks 1] [--out profiles/display_bench_line.json]
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

from s2sr import display, native  # noqa: E402
from s2sr import rasterio_lite as rio  # noqa: E402
from s2sr.synth import synthetic_tiles  # noqa: E402
from s2sr.weights import synthetic_state_dict  # noqa: E402

COPY_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--skip-host", action="store_true", help="leave out (c), the float64 host route (6.4 GB of temporaries at the default size)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    eng = native.Engine(num_block=a.blocks, precision=native.PREC_F16_HP)
    eng.load_state_dict(synthetic_state_dict(a.blocks, seed=0))
    S = a.size
    reps = -(-S // 1024)
    img8 = np.ascontiguousarray(np.tile(synthetic_tiles(1, 1024, seed=99)[0], (reps, reps, 1))[:S, :S])
    lr16 = (img8.astype(np.uint16) << 4) | (img8.astype(np.uint16) >> 4)       # 12 bits of radiometry, as tools/bench_u16.py
    lo, hi = int(lr16.min()), int(lr16.max())
    sr16 = eng.enhance_u16(lr16, lo, hi)                                       # the product; its copy stays on the device
    OH, OW = sr16.shape[:2]
    sr16 = np.array(sr16)                                                      # an ordinary (pageable) array, as a file reader hands over
    stretch = display.Stretch()

    def clock(what, fn, n_warm, n):
        for _ in range(n_warm):
            fn()
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(t)
        print(f"[bench_display] {what}: median {med:.1f} ms of {n}", file=sys.stderr, flush=True)
        return {"ms_per_run": [round(v, 1) for v in t], "ms_median": round(med, 1), "ms_min": round(min(t), 1),
                "spread_pct": round(100.0 * (max(t) - min(t)) / med, 2)}

    # (b) first: the device copy is there
    dev = clock("device_copy", lambda: display.render_u16(None, stretch, eng, shape=(OH, OW)), a.warmup, a.runs)
    hist_only = clock("device_copy_hist_only", lambda: eng.display_hist_u16(None, shape=(OH, OW)), 1, a.runs)
    host = clock("host_image", lambda: display.render_u16(sr16, stretch, eng), a.warmup, a.runs)
    res = {"metric": "display_u16", "size": S, "image": [OH, OW, 3], "runs": a.runs, "warmup": a.warmup,
           "host_image": host, "device_copy": dev, "device_copy_hist_only": hist_only}
    if not a.skip_host:
        res["host_minmax"] = clock("host_minmax", lambda: rio._to_u8(sr16, 0.0), 1, a.runs)
        res["host_image_over_host_minmax"] = round(host["ms_median"] / res["host_minmax"]["ms_median"], 4)
    samples = float(OH) * OW * 3
    res["host_link_GB"] = {"in": round(samples * 2 / 1e9, 2), "out": round(samples / 1e9, 2)}
    res["host_image_GB_s"] = round(samples * 3 / 1e9 / (host["ms_median"] / 1e3), 1)

    # kernel times by HIP events, separately: from the device copy (nothing else runs), then under a host image's copies
    for name, fn in (("kernels_device_copy", lambda: display.render_u16(None, stretch, eng, shape=(OH, OW))),
                     ("kernels_host_image", lambda: display.render_u16(sr16, stretch, eng))):
        if name == "kernels_device_copy":
            eng.enhance_u16(lr16, lo, hi)
        eng.set_profiling(1)
        eng.reset_kernel_stats()
        for _ in range(3):
            fn()
        st = eng.kernel_stats()
        eng.set_profiling(0)
        out = {}
        for k in ("display_hist", "display_apply"):
            v = st[k]
            tbs = v["bytes"] / 1e12 / (v["total_ms"] / 1e3) if v["total_ms"] > 0 else 0.0
            out[k] = {"launches": int(v["launches"]), "ms_per_image": round(v["total_ms"] / 3, 3), "algorithmic_TB_s": round(tbs, 3),
                      "of_copy_rate": round(tbs / COPY_TBS, 3)}
        res[name] = out
    eng.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
