"""Reprojection to Web Mercator and XYZ tile generation on the GPU: the same module surface as the
reference's GDAL helpers (reference server/app/tiling.py: RasterInfo :14-25, get_raster_info :28-99,
reproject_to_web_mercator :102-135, generate_xyz_tiles :138-186, create_tileset_metadata :189-224,
process_raster_to_tiles :227-275), without gdalinfo / gdalwarp / gdal2tiles.py subprocesses.

Scope: 8-bit RGB rasters (what the SR path writes) in UTM (EPSG:326xx / 327xx), EPSG:4326 or
EPSG:3857, north-up.  Resampling definitions are this build's (s2sr/tiles.py, csrc/tiles.hip);
GDAL is not available to compare against, see DESIGN.md.  The pyramid is cut with "average" (the
default, what tiling.py:138-186 passes) or with "lanczos" / "cubic" / "bilinear" (what the SR-to-tiles
job passes, reference esrgan_tiles.py:138; csrc/resample.hip, Pillow's arithmetic).
"""
from __future__ import annotations

import json
import logging
import struct
import threading
import zlib
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np
from PIL import Image

from s2sr import geo, native, tiles
from s2sr import rasterio_lite as rio
from s2sr import tiff_lite

logger = logging.getLogger("tiling")

_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def filter_sub_rgba(tiles_arr: np.ndarray) -> np.ndarray:
    """[..., 256, 256, 4] uint8 -> [..., 256, 1 + 1024]: every row behind its PNG filter byte (type 1, Sub, bpp = 4; wraps modulo
    256).  Vectorised over the leading axes: the pyramid filters 8 tiles per call inside the encoder threads (per tile the numpy
    calls are interpreter overhead; a whole z18 level in one call is 3 GB through one thread, 3x slower than either)."""
    lead, (h, w, _) = tiles_arr.shape[:-3], tiles_arr.shape[-3:]
    rows = tiles_arr.reshape(lead + (h, w * 4))
    raw = np.empty(lead + (h, w * 4 + 1), np.uint8)
    raw[..., 0] = 1
    raw[..., 1:5] = rows[..., :4]
    np.subtract(rows[..., 4:], rows[..., :-4], out=raw[..., 5:])
    return raw


def _png_from_filtered(raw: np.ndarray, level: int, strategy: int) -> bytes:
    h, w = raw.shape[0], (raw.shape[1] - 1) // 4

    def chunk(kind: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return (_PNG_SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
            chunk(b"IDAT", co.compress(raw.tobytes()) + co.flush()) + chunk(b"IEND", b""))


def encode_png_rgba(tile: np.ndarray, level: int = 1, strategy: int = zlib.Z_RLE) -> bytes:
    """256x256x4 uint8 -> PNG bytes (8-bit RGBA, Sub filter on every row, one IDAT).  The defaults (level 1 + Z_RLE, the fast
    end of deflate, what cv2.imwrite uses) go through the native encoder (csrc/pngenc.hip, ~3x zlib on tile data, GIL released:
    tiles are encoded on a thread pool; gdal2tiles uses --processes 4 for this); other settings through zlib."""
    if level == 1 and strategy == zlib.Z_RLE:
        return native.png_encode(tile)
    return _png_from_filtered(filter_sub_rgba(tile), level, strategy)

_ENGINES: dict = {}                 # device index -> (engine, lock of its pyramid chain)
_ENGINES_LOCK = threading.Lock()


def _engine_and_lock():
    """The pyramid engine of the GPU this job was admitted to (app.sr_routes.GpuAdmission sets the thread's device; default:
    LOCAL_RANK, as everywhere in app.*) and the lock that keeps one pyramid chain at a time on it.  A weightless handle is enough
    for the pyramid kernels (raises without a gfx950 GPU)."""
    from app.cnn_super_resolution import current_device_index
    dev = current_device_index()
    with _ENGINES_LOCK:
        if dev not in _ENGINES:
            _ENGINES[dev] = (native.Engine(num_block=1, device=dev), threading.RLock())
        return _ENGINES[dev]


def _engine() -> native.Engine:
    return _engine_and_lock()[0]


@dataclass
class RasterInfo:
    """Information about a raster file (field for field the reference's dataclass)."""
    path: Path
    crs: str
    bounds: list          # [west, south, east, north] in native CRS
    bounds_4326: list     # [west, south, east, north] in EPSG:4326
    width: int
    height: int
    bands: int
    dtype: str


_GDAL_TYPE = {"uint8": "Byte", "uint16": "UInt16", "int16": "Int16", "uint32": "UInt32", "int32": "Int32",
              "float32": "Float32", "float64": "Float64"}


def _read(path: Path):
    # a raster this process wrote a moment ago and nobody touched since (a job's sr_tif, main.py:347-359) comes from memory
    hit = rio.recall_written(path)
    arr, tags = hit if hit is not None else tiff_lite.read_tiff(path)
    place = geo.placement_from_tags(tags)
    if place is None:
        raise ValueError(f"{path}: no north-up georeferencing (tiepoint + pixel scale) in the GeoTIFF tags")
    epsg = geo.epsg_from_geokeys(tags.get(rio.TAG_GEOKEYS))
    return arr, tags, place, geo.CRS(epsg if epsg else 4326)      # the reference defaults to EPSG:4326 too (:49)


def get_raster_info(raster_path: Path) -> RasterInfo:
    raster_path = Path(raster_path)
    arr, _tags, place, crs = _read(raster_path)
    h, w, b = arr.shape
    west, south, east, north = place.bounds(w, h)
    t = np.linspace(0.0, 1.0, 21)
    ex = np.concatenate([west + (east - west) * t, np.full(21, east), east - (east - west) * t, np.full(21, west)])
    ey = np.concatenate([np.full(21, north), north - (north - south) * t, np.full(21, south), south + (north - south) * t])
    lon, lat = crs.to_lonlat(ex, ey)
    return RasterInfo(path=raster_path, crs=str(crs), bounds=[west, south, east, north],
                      bounds_4326=[float(lon.min()), float(lat.min()), float(lon.max()), float(lat.max())],
                      width=w, height=h, bands=b, dtype=_GDAL_TYPE.get(arr.dtype.name, arr.dtype.name))


def _mercator_tags(place: geo.Placement) -> rio.GeoRef:
    return rio.GeoRef({rio.TAG_PIXEL_SCALE: (place.dx, place.dy, 0.0),
                       rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, place.x0, place.y0, 0.0),
                       rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 3857)})


def _rgb_u8(arr: np.ndarray, stretch=None) -> np.ndarray:
    """Bands 1-3 (the single band three times) as the 8-bit image the warp and the pyramid take: the reference's global min-max
    (rasterio_lite._to_u8), or -- a uint16 raster with `stretch` (s2sr.display.Stretch or a dict of its fields) -- its display
    rendering, made on the device (pass the `limits` of a job's metadata to get the rendering of the job's PNG)."""
    rgb = arr[..., :3] if arr.shape[2] >= 3 else np.repeat(arr[..., :1], 3, axis=2)
    if stretch is None or arr.dtype != np.uint16:
        return rio._to_u8(rgb, 0.0)
    from s2sr.display import render_u16
    eng, lock = _engine_and_lock()
    with lock:
        return render_u16(np.ascontiguousarray(rgb), stretch, eng)[0]


def _check_mask_args(nodata, valid, valid_scale) -> None:
    """The refusals of the nodata arguments, before a file is read: nodata None, an integer or "tag" (s2sr.nodata.check_args);
    valid_scale an integer of at least 1."""
    from s2sr.nodata import DEFAULT_FILL_RADIUS, check_args
    check_args(nodata, DEFAULT_FILL_RADIUS)
    if isinstance(valid_scale, bool) or not isinstance(valid_scale, (int, np.integer)) or valid_scale < 1:
        raise ValueError(f"valid_scale {valid_scale!r}: an integer of at least 1")


def _mask_of(arr: np.ndarray, tags: dict, path, nodata, valid, valid_scale: int):
    """The mask a nodata-transparent pyramid is cut with -> (valid uint8 or None, its scale, the nodata value or None).
    nodata: an integer, or "tag" = the file's GDAL_NODATA tag (ValueError when it has none); the mask is then
    s2sr.nodata.mask_from_value on bands 1-3 of the raster AS READ (before _rgb_u8's stretch), scale 1.  valid: the caller's own
    mask, [ceil(H / valid_scale), ceil(W / valid_scale)]; it wins over the value (at 8 bits a measured pixel can equal it)."""
    from s2sr.nodata import mask_from_value
    value = None
    if nodata is not None:
        value = rio.resolve_nodata(nodata, rio.GeoRef({}, tiff_lite.parse_nodata(tags.get(tiff_lite.GDAL_NODATA))), path)
    if valid is not None:
        return native.warp_mask(arr.shape[:2] + (3,), valid, valid_scale), int(valid_scale), value
    if value is None:
        return None, 1, None
    raw = arr[..., :3] if arr.shape[2] >= 3 else np.repeat(arr[..., :1], 3, axis=2)
    return mask_from_value(raw, value), 1, value


def _ramp_source(arr: np.ndarray, ramp, path, stretch, nodata, valid):
    """A single-band int16 index raster through a colour ramp -> (rgb uint8 [H, W, 3], the mask of the masked warp:
    the rendering's alpha, scale 1).  ramp: a name of s2sr.index.RAMPS (its values at K = 10000), a list of (value, r, g, b) stops,
    or a ready LUT uint8 [65536][4].  Rendered on the device (native.Engine.index_render_i16); nodata (-32768) comes out 0, 0, 0, 0."""
    from s2sr import index as xi
    if stretch is not None or nodata is not None or valid is not None:
        raise ValueError("ramp renders an index raster, whose nodata is its own -32768: stretch, nodata and valid do not go with it")
    if arr.dtype != np.int16 or arr.shape[2] != 1:
        raise ValueError(f"{path}: ramp needs a single-band int16 raster, got {arr.shape[2]} band(s) of {arr.dtype}")
    lut = ramp if isinstance(ramp, np.ndarray) else xi.ramp_lut(xi.ramp_for(ramp))
    eng, lock = _engine_and_lock()
    with lock:
        rgba = np.array(eng.index_render_i16(np.ascontiguousarray(arr[..., 0]), lut))      # (out of the pinned pool, which the warp reuses)
    rgb = np.ascontiguousarray(rgba[..., :3])
    return rgb, native.warp_mask(rgb.shape, rgba[..., 3], 1)


def _u8_nodata(value) -> Optional[int]:
    """What the 8-bit <stem>_3857.tif holds in its alpha-0 pixels and declares in GDAL_NODATA: the value where a byte can hold it,
    0 otherwise (a 16-bit product's value above 255 under a display stretch); None: no value known, the file as ever."""
    if value is None:
        return None
    return int(value) if value == int(value) and 0 <= value <= 255 else 0


def _rgb_with_nodata(rgba: np.ndarray, fill: int) -> np.ndarray:
    """the RGB(A) raster whose alpha-0 pixels hold `fill`: colour is already 0 there (the warp's contract), so 0 costs nothing"""
    if fill == 0:
        return rgba
    rgb = np.ascontiguousarray(rgba[..., :3])
    rgb[rgba[..., 3] == 0] = fill
    return rgb


def _masked_rgba(rgb: np.ndarray, mask: Optional[np.ndarray], vs: int) -> np.ndarray:
    """A raster that is on the EPSG:3857 grid already: alpha 255 (x mask), RGB zeroed where invalid"""
    h, w = rgb.shape[:2]
    rgba = np.empty((h, w, 4), np.uint8)
    rgba[..., :3] = rgb
    rgba[..., 3] = 255
    if mask is not None:
        from s2sr.nodata import upsample_mask
        rgba[upsample_mask(mask, vs)[:h, :w] == 0] = 0
    return rgba


def reproject_to_web_mercator(input_path: Path, output_path: Path, resample_method: str = "bilinear", stretch=None, nodata=None) -> Path:
    """Writes an RGB GeoTIFF on the EPSG:3857 grid (pixels outside the source are black; the tile
    generator recomputes coverage from the geometry, so no alpha band is stored).  stretch: see _rgb_u8.
    nodata (None, an integer, or "tag"): the input's pixels that hold the value are left out of the bilinear taps,
    and the file carries the GDAL_NODATA tag and holds the value wherever nothing valid was warped to, the wedges outside the
    source included -- generate_xyz_tiles(nodata="tag") then cuts a pyramid that is transparent there."""
    if resample_method != "bilinear":
        raise ValueError("only bilinear resampling is implemented (the reference never passes anything else)")
    _check_mask_args(nodata, None, 1)
    input_path, output_path = Path(input_path), Path(output_path)
    arr, tags, place, crs = _read(input_path)
    mask, vs, value = _mask_of(arr, tags, input_path, nodata, None, 1)
    rgb = _rgb_u8(arr, stretch)
    plan = tiles.plan_warp(rgb.shape[1], rgb.shape[0], place, crs)
    eng, lock = _engine_and_lock()
    with lock:                   # the engine's scratch holds a pyramid chain's previous level (see _cut_pyramid)
        out = eng.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w, **({} if mask is None else {"valid": mask, "valid_scale": vs}))
    output_path.parent.mkdir(parents=True, exist_ok=True)
    fill = _u8_nodata(value)
    if fill is None:
        rio.write_geotiff_rgb(output_path, np.ascontiguousarray(out[..., :3]), _mercator_tags(plan.placement))
    else:
        rio.write_geotiff_rgb(output_path, np.ascontiguousarray(_rgb_with_nodata(out, fill)[..., :3]), _mercator_tags(plan.placement), nodata=fill)
    logger.info("Reprojection complete: %s", output_path)
    return output_path


LAST_STATS: dict = {}        # where the last process_raster_to_tiles / generate_xyz_tiles call spent its time (seconds; tools/bench_job.py)


RESAMPLINGS = ("average",) + tiles.FILTERS


def _check_tile_args(tile_size: int, resampling: str) -> None:
    if tile_size != 256:
        raise ValueError(f"tile_size {tile_size!r}: 256-pixel tiles are what is implemented")
    if resampling not in RESAMPLINGS:
        raise ValueError(f"resampling {resampling!r}: one of {', '.join(RESAMPLINGS)} (the reference passes average for its pyramids and "
                         "lanczos for the SR-to-tiles job)")


def _cut_pyramid(rgba: np.ndarray, place: geo.Placement, output_dir: Path, min_zoom: int, max_zoom: int, on_device: bool = False,
                 resampling: str = "average") -> None:
    """RGBA raster on the EPSG:3857 grid -> z/x/y.png files (deepest zoom from the raster, the others from their children).
    The levels never leave the device as pixels: each is computed from the previous one's device copy and its PNG files are encoded
    there (s2sr_tiles_write_png: token statistics and bit emission are kernels, the Huffman codes come from the host in between;
    chunk framing, CRC and the file writes run on native host threads).  on_device: `rgba` is what the caller's warp call just left on
    the engine (the caller holds the engine's lock across both): the base level reads that copy.  r04, same 12.8k-tile pyramid: levels fetched and deflated
    by zlib on a Python pool 1.9 s -> native host encoder, one call per 8 tiles 0.6 s -> encoded on the device (this).
    resampling: "average" = footprint means (tiles_base / tiles_overview); a filter of tiles.FILTERS = the deepest level resampled
    from the raster and every shallower one 2:1 from the level below it, across its tile borders (tiles_resample_u8); alpha is
    then fractional along the raster's edge."""
    import time
    _check_tile_args(256, resampling)
    h, w = rgba.shape[:2]
    output_dir.mkdir(parents=True, exist_ok=True)
    eng, lock = _engine_and_lock()
    levels = tiles.plan_levels(place.bounds(w, h), min_zoom, max_zoom)
    prev_lv = None
    t_dev = t_png = 0.0
    # the levels of one pyramid chain through the engine's device copy of the previous level: one pyramid at a time per engine
    with lock:
        for lv in levels:
            t0 = time.perf_counter()
            if resampling != "average":
                if prev_lv is None:
                    cols, rows = tiles.plan_resample_level(lv, tiles.level_box(lv, place), w, h, resampling)
                    eng.tiles_resample_u8(rgba, cols, rows, lv.nx, lv.ny, on_device=on_device, fetch=False)
                else:
                    cols, rows = tiles.plan_resample_level(lv, tiles.overview_box(lv, prev_lv), prev_lv.nx * geo.TILE, prev_lv.ny * geo.TILE,
                                                           resampling)
                    eng.tiles_resample_u8(None, cols, rows, lv.nx, lv.ny, level_shape=(prev_lv.ny, prev_lv.nx), on_device=True, fetch=False)
            elif prev_lv is None:
                eng.tiles_base_u8(rgba, *tiles.plan_base(lv, place, w, h), fetch=False, on_device=on_device)
            else:
                ox, oy = tiles.overview_offsets(lv, prev_lv)
                eng.tiles_overview_u8((prev_lv.ny, prev_lv.nx), ox, oy, lv.nx, lv.ny, on_device=True, fetch=False)
            t1 = time.perf_counter()
            # <output_dir>/<z>/<x>/<y>.png; tiles outside the raster (alpha 0 everywhere) get no file
            eng.tiles_write_png_xyz(lv.nx, lv.ny, output_dir, lv.zoom, lv.tminx, [geo.xyz_row(lv.tmaxy - j, lv.zoom) for j in range(lv.ny)])
            prev_lv = lv
            t_dev += t1 - t0
            t_png += time.perf_counter() - t1
    LAST_STATS.update(pyramid_level_kernels=t_dev, pyramid_png_on_device_and_files=t_png)


def generate_xyz_tiles(input_path: Path, output_dir: Path, min_zoom: int = 10, max_zoom: int = 16, tile_size: int = 256,
                       resampling: str = "average", nodata=None, valid=None, valid_scale: int = 1, ramp=None) -> Path:
    """z/x/y.png (XYZ row order, RGBA) for every tile of zooms min..max that holds data.  nodata / valid / valid_scale: the pixels
    the pyramid leaves transparent (see _mask_of).  ramp: a single-band int16 index raster through a colour ramp,
    transparent over its nodata (see _ramp_source)."""
    _check_tile_args(tile_size, resampling)
    _check_mask_args(nodata, valid, valid_scale)
    input_path, output_dir = Path(input_path), Path(output_dir)
    arr, tags, place, crs = _read(input_path)
    if crs.epsg != 3857:
        raise ValueError(f"{input_path}: {crs}, tiles are cut from an EPSG:3857 raster (reproject_to_web_mercator first)")
    if ramp is not None:
        rgb, mask = _ramp_source(arr, ramp, input_path, None, nodata, valid)
        rgba = _masked_rgba(rgb, mask, 1)
    else:
        mask, vs, _value = _mask_of(arr, tags, input_path, nodata, valid, valid_scale)
        rgba = _masked_rgba(arr[..., :3] if arr.shape[2] >= 3 else np.repeat(arr[..., :1], 3, axis=2), mask, vs)
    _cut_pyramid(rgba, place, output_dir, min_zoom, max_zoom, resampling=resampling)
    logger.info("Tile generation complete: %s", output_dir)
    return output_dir


def create_tileset_metadata(tiles_dir: Path, bounds_4326: list, min_zoom: int, max_zoom: int,
                            tile_template: str = "/tiles/{z}/{x}/{y}.png") -> dict:
    metadata = {"bounds": bounds_4326, "minzoom": min_zoom, "maxzoom": max_zoom, "tileTemplate": tile_template,
                "attribution": "Sentinel-2 SR via UP42", "format": "png", "tileSize": 256}
    tiles_dir = Path(tiles_dir)
    tiles_dir.mkdir(parents=True, exist_ok=True)
    (tiles_dir / "tileset.json").write_text(json.dumps(metadata, indent=2))
    return metadata


def process_raster_to_tiles(input_path: Path, tiles_dir: Path, min_zoom: int = 10, max_zoom: int = 16, resampling: str = "average",
                            tile_template: str = "/tiles/{z}/{x}/{y}.png", stretch=None, nodata=None, valid=None,
                            valid_scale: int = 1, ramp=None) -> dict:
    """Check the CRS, reproject if needed, cut the pyramid, write tileset.json.  stretch (uint16 rasters; ignored for uint8): the
    8-bit image is the raster's display rendering instead of the global min-max, see _rgb_u8.
    nodata (None, an integer, or "tag") / valid, valid_scale (the caller's own mask, which wins; see _mask_of): the pyramid is
    transparent over the pixels that were never measured -- a raster that needs reprojecting goes through the
    masked warp, one that is EPSG:3857 already gets alpha 255 x mask and RGB 0 where invalid; with a value known <stem>_3857.tif
    carries the GDAL_NODATA tag and holds the value in every alpha-0 pixel.  Without them every file is what it always was.
    ramp (see _ramp_source): the raster is a single-band int16 index; it is rendered through the colour ramp on the
    device, the rendering's alpha is the mask of the masked warp, and the pyramid is cut as for any nodata-transparent raster."""
    import time
    _check_tile_args(256, resampling)
    _check_mask_args(nodata, valid, valid_scale)
    input_path, tiles_dir = Path(input_path), Path(tiles_dir)
    LAST_STATS.clear()
    t0 = time.perf_counter()
    arr, tags, place, crs = _read(input_path)
    if ramp is not None:
        rgb, mask = _ramp_source(arr, ramp, input_path, stretch, nodata, valid)
        vs, value = 1, None
    else:
        mask, vs, value = _mask_of(arr, tags, input_path, nodata, valid, valid_scale)
    h, w, b = arr.shape
    west, south, east, north = place.bounds(w, h)
    t = np.linspace(0.0, 1.0, 21)
    ex = np.concatenate([west + (east - west) * t, np.full(21, east), east - (east - west) * t, np.full(21, west)])
    ey = np.concatenate([np.full(21, north), north - (north - south) * t, np.full(21, south), south + (north - south) * t])
    lon, lat = crs.to_lonlat(ex, ey)
    bounds_4326 = [float(lon.min()), float(lat.min()), float(lon.max()), float(lat.max())]
    if ramp is None:
        rgb = _rgb_u8(arr, stretch)
    t1 = time.perf_counter()
    LAST_STATS["read"] = t1 - t0
    side, err = None, []
    eng, lock = _engine_and_lock()
    with lock:                   # one pyramid chain at a time per engine; held from the warp to the base level that reads its device copy
        if crs.epsg != 3857:
            # the warped raster is written next to the input like the reference does (<stem>_3857.tif, :251-252),
            # but the pyramid is cut from the array in hand, with the coverage mask of the warp as alpha
            plan = tiles.plan_warp(w, h, place, crs)
            t2 = time.perf_counter()
            rgba = eng.warp_bilinear_u8(rgb, plan.grid, plan.step, plan.out_h, plan.out_w, **({} if mask is None else {"valid": mask, "valid_scale": vs}))
            t3 = time.perf_counter()
            place = plan.placement
            LAST_STATS.update(warp_plan=t2 - t1, warp_call=t3 - t2)
            fill = _u8_nodata(value)

            def write_3857():            # next to the pyramid, not in front of it: its strips fill the CPUs the device calls leave idle
                try:
                    out_3857 = input_path.parent / f"{input_path.stem}_3857.tif"
                    if fill is None:
                        rio.write_geotiff_rgb(out_3857, rgba, _mercator_tags(plan.placement))   # alpha dropped per strip
                    else:                # (the pyramid reads the warp's device copy: the host raster is this thread's)
                        rio.write_geotiff_rgb(out_3857, _rgb_with_nodata(rgba, fill), _mercator_tags(plan.placement), nodata=fill)
                except BaseException as e:      # noqa: BLE001 -- surfaced below: a failed writer fails the call
                    err.append(e)
            side = threading.Thread(target=write_3857)
            side.start()
        elif mask is not None:
            rgba = _masked_rgba(rgb, mask, vs)
        else:
            rgba = np.dstack([rgb, np.full((h, w), 255, np.uint8)])
        t4 = time.perf_counter()
        try:
            _cut_pyramid(np.ascontiguousarray(rgba), place, tiles_dir, min_zoom, max_zoom, on_device=side is not None, resampling=resampling)
        finally:
            if side is not None:
                t5 = time.perf_counter()
                side.join()
                LAST_STATS["wait_for_3857_tif"] = time.perf_counter() - t5      # what the warped raster's file still needs behind the pyramid
    if err:
        raise err[0]
    LAST_STATS["pyramid"] = time.perf_counter() - t4
    return create_tileset_metadata(tiles_dir, bounds_4326, min_zoom, max_zoom, tile_template=tile_template)
