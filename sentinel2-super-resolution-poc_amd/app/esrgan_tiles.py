"""Drop-in for the reference module `app.esrgan_tiles` (reference server/app/esrgan_tiles.py:23-193): Real-ESRGAN x4 followed by a
high-zoom Lanczos tile pyramid (z18-20 by default), both on the GPU through libs2sr.so.

    python -m app.esrgan_tiles [--input PATH] [--output-dir PATH] [--min-zoom 18] [--max-zoom 20]

The pyramid is an over-zoom (a 2.5 m raster shown at 0.6 / 0.3 / 0.15 m per tile pixel), which is why the job asks for Lanczos:
under "average" every source pixel would come out as a square of up to 17 x 17 tile pixels.
"""
from __future__ import annotations

import logging
import sys
from datetime import datetime
from pathlib import Path
from typing import Optional

from app.tiling import get_raster_info, process_raster_to_tiles
from app.wow_sr import apply_wow_sr

logger = logging.getLogger("esrgan_tiles")

TILE_TEMPLATE = "/tiles_esrgan/{z}/{x}/{y}.png"


def run_esrgan_and_tiles(input_path: Path, output_dir: Path, min_zoom: int = 18, max_zoom: int = 20, enhance_crops: bool = True,
                         skip_sr: bool = False, sr_output: Optional[Path] = None, nodata=None) -> dict:
    """<output_dir>/sr_esrgan/<stem>_esrgan_x4.tif through apply_wow_sr (skip_sr: `sr_output` is taken as that file), then
    <output_dir>/tiles_esrgan/{z}/{x}/{y}.png + tileset.json, Lanczos, reprojected first when the raster is not EPSG:3857 (the
    warped raster is written next to the SR output as <stem>_3857.tif; the pyramid reads its device copy).  A failing step is
    recorded in the result's "steps" and the result returned: nothing is raised.
    nodata (None, an integer, or "tag"): the SR step runs as a nodata job and the pyramid is transparent over
    the pixels that were never measured -- cut with the input's own mask at the SR scale, or, with skip_sr, with the mask the
    value gives on the SR raster."""
    from s2sr.nodata import DEFAULT_FILL_RADIUS, check_args
    check_args(nodata, DEFAULT_FILL_RADIUS)
    input_path, output_dir = Path(input_path), Path(output_dir)
    mask_kw = {} if nodata is None else {"nodata": nodata}
    results = {"timestamp": datetime.now().strftime("%Y%m%d_%H%M%S"), "input": str(input_path), "min_zoom": min_zoom,
               "max_zoom": max_zoom, "steps": []}
    sr_dir, tiles_dir = output_dir / "sr_esrgan", output_dir / "tiles_esrgan"
    sr_dir.mkdir(parents=True, exist_ok=True)
    tiles_dir.mkdir(parents=True, exist_ok=True)
    sr_tif = Path(sr_output) if sr_output is not None else None

    if not skip_sr:
        logger.info("Step 1/2: Real-ESRGAN x4 super-resolution")
        sr_tif = sr_dir / f"{input_path.stem}_esrgan_x4.tif"
        try:
            out, sr_metadata = apply_wow_sr(input_path=input_path, output_path=sr_tif, enhance_crops=enhance_crops, **mask_kw)
            sr_tif = Path(out)
            if nodata is not None:      # the job's own mask, read at the SR scale; the SR GeoTIFF declares the value
                from app.wow_sr import input_mask
                mask_kw = {"valid": input_mask(input_path, nodata), "valid_scale": int(sr_metadata["scale"]), "nodata": "tag"}
            results["steps"].append({"step": 1, "name": "Real-ESRGAN SR", "status": "completed", "output": str(sr_tif),
                                     "metadata": sr_metadata})
        except Exception as e:      # noqa: BLE001 -- the job's contract: a failed step is reported, not raised
            logger.error("SR failed: %s", e)
            results["steps"].append({"step": 1, "name": "Real-ESRGAN SR", "status": "failed", "error": str(e)})
            return results
    else:
        logger.info("Skipping SR (using existing output)")
        results["steps"].append({"step": 1, "name": "Real-ESRGAN SR", "status": "skipped", "output": str(sr_tif)})

    logger.info("Step 2/2: tiles z%d-%d", min_zoom, max_zoom)
    try:
        if sr_tif is None:
            raise ValueError("skip_sr needs sr_output: the SR raster to cut the tiles from")
        info = get_raster_info(sr_tif)
        logger.info("SR image: %dx%d pixels, CRS: %s", info.width, info.height, info.crs)
        metadata = process_raster_to_tiles(sr_tif, tiles_dir, min_zoom=min_zoom, max_zoom=max_zoom, resampling="lanczos",
                                           tile_template=TILE_TEMPLATE, **mask_kw)
        tile_count = sum(1 for _ in tiles_dir.rglob("*.png"))
        results["steps"].append({"step": 2, "name": "Tile Generation", "status": "completed", "output_dir": str(tiles_dir),
                                 "tile_count": tile_count, "zoom_levels": list(range(min_zoom, max_zoom + 1)), "metadata": metadata})
    except Exception as e:          # noqa: BLE001
        logger.error("Tile generation failed: %s", e)
        results["steps"].append({"step": 2, "name": "Tile Generation", "status": "failed", "error": str(e)})
        return results

    results.update(status="completed", sr_output=str(sr_tif), tiles_dir=str(tiles_dir), tile_count=tile_count)
    logger.info("Real-ESRGAN + high-zoom tiles complete: %s, %d tiles at z%d-%d", tiles_dir, tile_count, min_zoom, max_zoom)
    return results


def main(argv=None) -> int:
    import argparse

    ap = argparse.ArgumentParser(description="Real-ESRGAN enhanced tiles at zoom 18-20 (MI355X)")
    ap.add_argument("--input", "-i", help="input GeoTIFF; default: the newest *.tif under <output-dir>/source")
    ap.add_argument("--output-dir", "-o", default="/app/data")
    ap.add_argument("--min-zoom", type=int, default=18)
    ap.add_argument("--max-zoom", type=int, default=20)
    ap.add_argument("--no-enhance", action="store_true", help="skip the crop-visibility post-process")
    ap.add_argument("--skip-sr", action="store_true", help="only cut tiles from an existing SR output")
    ap.add_argument("--sr-output", help="the existing SR output (required with --skip-sr)")
    ap.add_argument("--nodata", type=lambda s: s if s == "tag" else int(s), default=None,
                    help="the value of the pixels that were never measured, or \"tag\" (the file's GDAL_NODATA): filled in front of the "
                         "net, transparent in the tiles")
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    if a.input:
        input_path = Path(a.input)
        if not input_path.exists():
            logger.error("Input file not found: %s", input_path)
            return 1
    else:
        found = sorted((Path(a.output_dir) / "source").glob("*.tif"), key=lambda q: q.stat().st_mtime)
        if not found:
            logger.error("No GeoTIFF files found in %s: specify --input", Path(a.output_dir) / "source")
            return 1
        input_path = found[-1]
    sr_output = None
    if a.skip_sr:
        if not a.sr_output or not Path(a.sr_output).exists():
            logger.error("--skip-sr needs --sr-output, an existing SR raster")
            return 1
        sr_output = Path(a.sr_output)
    result = run_esrgan_and_tiles(input_path, Path(a.output_dir), min_zoom=a.min_zoom, max_zoom=a.max_zoom,
                                  enhance_crops=not a.no_enhance, skip_sr=a.skip_sr, sr_output=sr_output,
                                  **({} if a.nodata is None else {"nodata": a.nodata}))
    if result.get("status") == "completed":
        logger.info("View tiles at %s", TILE_TEMPLATE)
        return 0
    logger.error("Pipeline failed: %s", result["steps"][-1].get("error"))
    return 1


if __name__ == "__main__":
    sys.exit(main())
