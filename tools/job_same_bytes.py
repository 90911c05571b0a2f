#!/usr/bin/env python3
"""SHA-256 of every file a fixed list of process_wow_sr / process_farm_sr jobs writes: one `job file sha256` line per file and, per
job, one line for its metadata JSON with the timestamp and the temporary directory taken out of the text (key order stays in).
Seeded 37 x 45 four-band inputs, synthetic weights, one process.  Run it on two commits and compare the lines: a change of the job
path that moves no byte leaves every line as it was (profiles/job_record_same_bytes.txt).

    python tools/job_same_bytes.py > lines.txt
"""
from __future__ import annotations

import builtins
import hashlib
import os
import re
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (str(REPO / "sentinel2-super-resolution-poc_amd"), str(REPO)):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from s2sr import rasterio_lite as rio  # noqa: E402
from s2sr.weights import synthetic_state_dict  # noqa: E402

H, W = 37, 45
S16 = dict(enhance_crops=False, bit_depth=16)
STRETCH = {"p_lo": 2.0, "p_hi": 98.0, "linked": False}
INDICES = ["ndvi", {"name": "rb", "a": 1, "b": 3, "offset": 100}]
JOBS = [                                         # (name, function, input, keywords; "zones": the label file's path is filled in)
    ("wow-8-crops", "wow", "u8", dict()),
    ("wow-8-plain", "wow", "u8", dict(enhance_crops=False)),
    ("wow-8-seam-blend", "wow", "u8", dict(seam_blend=True)),
    ("wow-8-nodata-tag", "wow", "u16", dict(nodata="tag")),
    ("wow-8-consistency", "wow", "u8", dict(consistency="exact")),
    ("wow-16-plain", "wow", "u16", dict(S16)),
    ("wow-16-display-crops", "wow", "u16", dict(S16, enhance_crops=True, display=STRETCH)),
    ("wow-16-extra-bands-all", "wow", "u16", dict(S16, extra_bands="all")),
    ("wow-16-indices-zones", "wow", "u16", dict(S16, indices=INDICES, zones=True)),
    ("wow-16-everything", "wow", "u16", dict(S16, enhance_crops=True, display=STRETCH, seam_blend=True, nodata="tag", fill_radius=9,
                                             consistency="smooth", extra_bands=[4], extra_weights=(2, 1, 1), indices=INDICES,
                                             index_offset=50, zones=True)),
    ("farm", "farm", "u8", dict()),
    ("farm-seam-blend-consistency", "farm", "u8", dict(seam_blend=True, consistency="smooth")),
]


def main():
    tmp = Path(tempfile.mkdtemp())
    os.environ["S2SR_MODEL_DIR"] = str(tmp / "models")
    os.environ.pop("S2SR_PRECISION", None)
    (tmp / "models").mkdir()
    for name, nb in (("realesrgan_anime", 6), ("realesrgan_x4", 23)):
        torch.save({"params_ema": {k: torch.from_numpy(v) for k, v in synthetic_state_dict(nb, seed=0).items()}}, tmp / "models" / f"{name}.pth")
    rng = np.random.default_rng(2034)
    four = rng.integers(1000, 4000, size=(H, W, 4)).astype(np.uint16)
    four[..., 3] = (four[..., :3].sum(axis=2) // 2 + rng.integers(0, 300, (H, W))).astype(np.uint16)
    four[5:9, 7:30] = 0                          # never measured
    four[20, 20, :3] = 0
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0),
                      rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633)})
    rio.write_geotiff_u16(tmp / "u16.tif", four, geo, nodata=0)
    rio.write_geotiff_rgb(tmp / "u8.tif", rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), geo)
    zones = np.zeros((H, W), np.uint16)
    zones[10:30, 5:25], zones[12:20, 30:44] = 1, 3
    rio.write_geotiff_u16(tmp / "zones.tif", zones[..., None], geo)

    from app.farm_sr import process_farm_sr
    from app.wow_sr import process_wow_sr
    real_print = print
    for name, fn, src, kw in JOBS:
        kw = dict(kw)
        if kw.get("zones"):
            kw["zones"] = tmp / "zones.tif"
        if fn == "wow":
            kw.setdefault("model", "realesrgan_anime")
        out = tmp / name
        builtins.print = lambda *a, **k: None    # (the job functions narrate on stdout)
        try:
            (process_wow_sr if fn == "wow" else process_farm_sr)(tmp / f"{src}.tif", out, **kw)
        finally:
            builtins.print = real_print
        for f in sorted(out.iterdir()):
            if f.name.endswith("_metadata.json"):
                text = re.sub(r'"timestamp": "[0-9_]+"', '"timestamp": ""', f.read_text().replace(str(tmp), ""))
                print(f"{name} {f.name} (normalised) {hashlib.sha256(text.encode()).hexdigest()}", flush=True)
            else:
                print(f"{name} {f.name} {hashlib.sha256(f.read_bytes()).hexdigest()}", flush=True)


if __name__ == "__main__":
    main()
