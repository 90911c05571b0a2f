"""Drop-in for the reference module `app.wow_sr` (reference server/app/wow_sr.py): Real-ESRGAN x4
followed by the crop-visibility post-process, both on the GPU through libs2sr.so."""
from __future__ import annotations

import json
import threading
from datetime import datetime
from pathlib import Path
from typing import Tuple

import numpy as np

from app.cnn_super_resolution import RealESRGAN
from app.job_options import JobOptions
from s2sr import native

_PP_LOCK = threading.Lock()
_PP_ENGINE = {}


def _pp_engine(device_index: int = None) -> native.Engine:
    """Handle used for post-process only (it needs no weights); one per GPU, shared by all jobs
    (s2sr_postprocess_u8 holds the handle's lock from upload to download)."""
    if device_index is None:
        from app.cnn_super_resolution import current_device_index
        device_index = current_device_index()
    with _PP_LOCK:
        if device_index not in _PP_ENGINE:
            _PP_ENGINE[device_index] = native.Engine(num_block=1, device=device_index)
        return _PP_ENGINE[device_index]


def _enhance_for_crops(img: np.ndarray) -> np.ndarray:
    """CLAHE(2.5, 8x8) on L -> unsharp (sigma 1.2, 1.4/-0.4) -> saturation x1.2 on hue 36..84
    (reference wow_sr.py:187-209): HxWx3 uint8 RGB -> same, one fused GPU pass sequence."""
    return _pp_engine().postprocess_u8(img, native.pp_wow())


def _alpha_of(valid, scale: int) -> dict:
    """What a PNG writer gets of a nodata job's mask (a job without one: nothing, the call as ever)."""
    return {} if valid is None else {"valid": valid, "valid_scale": scale}


def _nodata_block(value, valid: np.ndarray, fill_radius: int) -> dict:
    """The metadata of a nodata job."""
    return {"value": value, "invalid_pixels": int(valid.size - np.count_nonzero(valid)), "fill_radius": int(fill_radius)}


def read_masked(input_path: Path, nodata, bit_depth: int = 8):
    """A nodata job's input and its mask, one definition for the job and for whoever needs the job's mask again (the tiler of a
    transparent_tiles job, app.sr_routes) -> (image, GeoRef, valid uint8 [H, W], the nodata value).  bit_depth 8: the 8-bit image
    of rio.read_rgb_u8_nodata (mask from the raster AS STORED); 16: the raw uint16 raster, the value an integer in 0..65535."""
    from s2sr import rasterio_lite as rio
    from s2sr.nodata import mask_from_value
    input_path = Path(input_path)
    if bit_depth != 16:
        return rio.read_rgb_u8_nodata(input_path, nodata)
    try:
        img, georef = rio.read_rgb_raw(input_path)
    except ValueError as e:
        raise ValueError(f"bit_depth=16 needs a uint16 GeoTIFF: {e}") from e
    if img.dtype != np.uint16:
        raise ValueError(f"bit_depth=16 needs a uint16 GeoTIFF, {input_path} holds {img.dtype}")
    if nodata is None:               # (the 16-bit job without the option reads its file here too: no mask, no value)
        return img, georef, None, None
    value = rio.resolve_nodata(nodata, georef, input_path)
    if not 0 <= value <= 65535 or value != int(value):
        raise ValueError(f"nodata {value!r}: a uint16 raster takes an integer in 0..65535")
    return img, georef, mask_from_value(img, value), value


def input_mask(input_path: Path, nodata, bit_depth: int = 8) -> np.ndarray:
    """The mask a nodata job derives from its input file (uint8 [H, W] at the INPUT resolution, 1 = valid)."""
    return read_masked(input_path, nodata, bit_depth)[2]


def _apply_wow_sr16(input_path: Path, output_path: Path, model: str, enhance_crops: bool, o: JobOptions) -> Tuple[Path, dict]:
    """bit_depth=16 of apply_wow_sr (o: the job's options, checked; its fields are named below): a uint16 GeoTIFF read raw,
    value_range = the image's own (min, max) -- the reference's min-max (wow_sr.py:67-73) minus its quantisation to 8 bits -- the
    net fed BGR as ever (:85,94), RealESRGAN.product16, RGB back, a uint16 GeoTIFF out.  Without `display`: no PNG (the encoder is 8-bit) and no crop-visibility post-process (OpenCV's 8-bit
    arithmetic).  With it (s2sr.display.Stretch or a dict of its fields): the output's display rendering, made on the device from
    the output's copy there, is written as the PNG, after the crop-visibility post-process when enhance_crops; the GeoTIFF stays raw.
    nodata (an integer, or "tag"): see apply_wow_sr; the value range is that of the valid pixels (s2sr.nodata.valid_range), the
    GeoTIFF declares the value, the PNG (with `display`) carries the mask as alpha, and the stretch leaves the value out of its
    statistics unless it names a nodata of its own.
    extra_bands ("all" or band numbers from 4 on): those bands of the file are carried to the output grid against the
    super-resolved image (RealESRGAN.product16(extra=...)), each with its own min-max over the valid pixels as its range, and the
    GeoTIFF holds 3 + k bands: RGB as without the option, then the carried bands in the order given.  extra_weights: the guide
    weights in R, G, B terms (None: 1, 1, 1).
    indices, index_offset, zones (s2sr/index.py): spectral indices on the output grid -- a list of preset names
    ("ndvi", "ndwi", "ndre", "savi"), presets with their bands named ({"preset": "ndre", "nir": 4, "rededge": 5}) or definitions
    ({"name", "a", "b", "offset", "L", "K"}; a, b: 1-based bands of the file).  Bands 1-3 are read from the job's final uint16
    product on the device (behind the consistency pass), bands from 4 on are carried for the index whether or not extra_bands
    lists them (only listed bands go into the product GeoTIFF), and the job's nodata mask is the index's.  index_offset: the DN
    offset of a definition that names none.  Per index the job writes <stem>_<name>.tif (int16, GDAL_NODATA -32768) and
    <stem>_<name>.png (its RGBA rendering through the index's colour ramp); zones (the path of a single-band uint8 / uint16 label
    GeoTIFF on the input or the output grid, or such an array) adds a per-zone table.  The metadata gains "indices", and only then.
    zones may also be field polygons (s2sr/zones.py): a GeoJSON source -- the path of a .geojson / .json file, a parsed
    FeatureCollection, Feature or geometry, or a list of those -- or {"geojson": source, "property": name}.  They are projected onto
    the output grid, rasterised on the job's engine in front of the net, and the labels then travel as a caller's array does; the
    job also writes <stem>_zones.tif (uint16, GDAL_NODATA 0, the product's georeference) and the metadata gains "zones", and only then.
    zones may also be {"segment": {"index": name, "min": 0.3, "max": None, "open": 1, "close": 2, "connectivity": 4, "min_area_ha": 0.5}}
    (s2sr/fields.py): the fields are the connected components of the thresholded, opened and closed raster of the named
    index; the job writes <stem>_zones.tif as above and <stem>_fields.geojson (one Feature per field, lon / lat).
    With "split": True or {"core": 0.5, "core_px": 2, "edge": None, "edge_smooth": 1} inside "segment"  touching fields
    are cut apart around the cores of their distance transform, optionally along gradient ridges of the index; the files are the same
    files, and metadata["zones"]["parameters"] gains "split", and only then.
    zones may also be {"manage": {"index": name or names, "k": 3, "iterations": 32, "min_per_zone": 10, "smooth": 1, "polygons": True},
    "fields": any of the values above} (s2sr/mzones.py): `fields` is handled exactly as that value is without "manage";
    the pixels of every field are then split into k zones by the named index rasters (integer k-means on the job's engine), and the job
    writes <stem>_mzones.tif (uint8, GDAL_NODATA 0, the product's georeference), with polygons <stem>_mzones.geojson (one Feature per
    field and zone), and metadata["zones"]["management"]."""
    import dataclasses

    from s2sr import rasterio_lite as rio
    from s2sr.display import Stretch
    stretch = None if o.display is None else Stretch.of(o.display)
    from s2sr import mzones as xm
    manage = None
    if xm.is_manage(o.zones):          # management zones: from here on `zones` is the value of "fields", handled as ever
        manage = {"option": o.zones}
        o = dataclasses.replace(o, zones=o.zones["fields"])

    input_path = Path(input_path)
    print(f"\nWOW Super-Resolution ({model}, 16-bit)\n   Input: {input_path}")
    img, georef, valid, value = read_masked(input_path, o.nodata, 16)
    extra = numbers = defs = None
    if o.extra_bands is not None or o.indices is not None:
        from s2sr import bands as xb
        try:
            every, _ = rio.read_bands_raw(input_path)
        except ValueError as e:
            raise ValueError(f"{'extra_bands' if o.extra_bands is not None else 'indices'} needs a GeoTIFF whose bands share one uint16 layout: {e}") from e
        listed = [] if o.extra_bands is None else xb.select_bands(o.extra_bands, every.shape[2])
        numbers = list(listed)                                    # the carried bands: the listed ones, then what only an index reads
        if o.indices is not None:
            from s2sr import index as xi
            defs = xi.resolve(o.indices, o.index_offset, every.shape[2])
            numbers += [b for b in xi.carried_bands(defs) if b not in numbers]
            from s2sr import zones as xz
            from s2sr import fields as xf
            segmenting = xf.is_segment(o.zones)                            # fields from the job's own index raster, below
            polygons = o.zones is not None and not segmenting and xz.is_geojson(o.zones)   # rasterised through the job's engine, below
            label = None if o.zones is None or polygons or segmenting else xi.check_zones(rio.read_bands_raw(o.zones)[0] if isinstance(o.zones, (str, Path)) else o.zones,
                                                                             img.shape[:2], 4)
        if numbers:
            extra = np.ascontiguousarray(every[:, :, [b - 1 for b in numbers]])
        del every
        w_rgb = xb.check_args(4, 0, 65535, xb.WEIGHTS if o.extra_weights is None else o.extra_weights)["weights"]
    from s2sr.nodata import valid_range
    lo, hi = valid_range(img, valid)
    call = {} if valid is None else {"valid": valid, "nodata": value, "fill_radius": o.fill_radius}
    tagged = {} if valid is None else {"nodata": value}                                  # what the GeoTIFF writers get
    esrgan = RealESRGAN(model_name=model, tile_size=256, **o.passed("RealESRGAN"))
    if extra is not None:            # the device copy is BGR: the guide weights go in reversed
        call.update(extra=extra, extra_weights=w_rgb[::-1])
    burnt = seg = None
    if manage is not None:             # its refusals before the net runs; the GeoJSON needs the raster's place
        manage["params"] = xm.resolve(manage["option"], defs)
        if manage["params"]["polygons"]:
            xf.placement_of(None if georef is None else georef.scaled(esrgan.scale))
    if defs is not None and segmenting:    # every refusal of the option before the net runs; the size in pixels of the output grid
        xf.placement_of(None if georef is None else georef.scaled(esrgan.scale))      # the GeoJSON needs the raster's place
        size = georef.scaled(esrgan.scale).pixel_size
        seg = {"params": xf.resolve(o.zones, defs, None if size is None else abs(float(size[0]) * float(size[1])))}
    if defs is not None and polygons:      # field polygons: labels on the output grid, in front of the net; they travel as a caller's array does
        burnt = xz.rasterize(esrgan._engine, o.zones, georef, img.shape[:2], esrgan.scale)
        label = (burnt["labels"], 1, burnt["Z"])
    if defs is not None:             # file band 1, 2, 3 is channel 2, 1, 0 of the device copy; a band from 4 on is one of the carried
        side = lambda b: ("img", 3 - b) if b <= 3 else ("extra", numbers.index(b))
        ramps = [xi.ramp_for(xi.DEFAULT_RAMP.get(d["preset"], "diverging"), d["K"]) for d in defs]
        zoned = {} if label is None else {"zones": label[0], "zone_scale": label[1], "Z": label[2]}
        call["indices"] = [dict(a=side(d["a"]), b=side(d["b"]), offset=d["offset"], L=d["L"], K=d["K"], lut=xi.ramp_lut(r), **zoned)
                           for d, r in zip(defs, ramps)]
    if stretch is not None:
        # the device copy is BGR like the net's input: explicit per-band limits go in reversed, the info's come back reversed
        call["display"] = stretch if stretch.limits is None else dataclasses.replace(stretch, limits=stretch.limits[::-1])
    got = esrgan.product16(np.ascontiguousarray(img[:, :, ::-1]), value_range=(lo, hi), **call)
    display_rgb, info, carried, carried_rec, found = None, None, got.carried, got.carried_record, got.indices
    if stretch is not None:
        display_rgb = np.ascontiguousarray(got.display[:, :, ::-1])
        info = dict(got.info, limits=got.info["limits"][::-1])
        if enhance_crops:
            print("   Stage 2/2: Crop visibility enhancement (on the display image)...")
            display_rgb = _enhance_for_crops(display_rgb)
    output_rgb = np.ascontiguousarray(got.out16[:, :, ::-1])
    scale = esrgan.scale
    inexact = None if o.consistency is None else got.inexact_blocks[::-1]      # (the net's image is B, G, R)
    if seg is not None:              # segment the named raster, then each index's per-zone sums from host arrays: the segment call voided the kept image
        seg.update(xf.segment(esrgan._engine, found[seg["params"]["index"]]["index"], seg["params"]))
        for d, r in zip(call["indices"], found):
            r["zonal"] = xf.zonal(esrgan._engine, d, got.out16, carried, valid, seg["labels"], seg["found"])
        label = (seg["labels"], 1, seg["found"])
    if manage is not None:           # k-means inside every field on the named index rasters (host arrays: the call voids the kept image)
        mz_labels = np.asarray(label[0]) if label[1] == 1 else \
            np.repeat(np.repeat(np.asarray(label[0]), label[1], axis=0), label[1], axis=1)[:got.out16.shape[0], :got.out16.shape[1]]
        mz_labels = np.ascontiguousarray(mz_labels.astype(np.uint16))
        params = manage["params"]
        manage["result"] = xm.run(esrgan._engine, [found[i]["index"] for i in params["indices"]], mz_labels, label[2], params)
        if params["polygons"]:
            manage["rings"] = xm.trace(esrgan._engine, manage["result"]["zone"], mz_labels, label[2], params["k"])
    del esrgan
    final_output = Path(output_path).with_suffix(".tif")
    final_output.parent.mkdir(parents=True, exist_ok=True)
    if carried is not None and defs is not None:                  # only the listed bands go into the product
        carried = carried[..., :len(listed)] if listed else None
        carried_rec = None if carried is None else {k: (v[:len(listed)] if k in ("ranges", "eps", "inexact") else v) for k, v in carried_rec.items()}
        numbers = listed
    if carried is None:
        rio.write_geotiff_rgb16(final_output, output_rgb, georef.scaled(scale), **tagged)
    else:
        rio.write_geotiff_u16(final_output, np.concatenate([output_rgb, carried], axis=2), georef.scaled(scale), **tagged)
    if display_rgb is not None:
        rio.write_png(final_output.with_suffix(".png"), display_rgb, **_alpha_of(valid, scale))
    crops = display_rgb is not None and enhance_crops
    metadata = {
        "input_file": str(input_path),
        "output_file": str(final_output),
        "scale": scale,
        "pipeline": "Real-ESRGAN x4 (16-bit)",
        "stages": [{"model": model, "scale": scale, "purpose": "GAN upscaling"}] +
                  ([{"post_processing": "Enhanced", "purpose": "Crop visibility"}] if crops else []),
        "enhancements": ["CLAHE local contrast", "Unsharp mask", "Vegetation boost"] if crops else [],
        "original_size": list(img.shape[:2]),
        "output_size": list(output_rgb.shape[:2]),
        "original_resolution_m": 10.0,
        "effective_resolution_m": 10.0 / scale,
        "optimized_for": "z18_crop_visibility",
        "bit_depth": 16,
        "value_range": [lo, hi],
    }
    if o.seam_blend:
        metadata["seam_blend"] = True
    if info is not None:
        metadata["display"] = info
    if valid is not None:
        metadata["nodata"] = _nodata_block(value, valid, o.fill_radius)
    if o.consistency is not None:      # the GeoTIFF is the consistent product; the display image and its crop step are renderings of it
        from s2sr.consistency import metadata_block
        metadata["consistency"] = metadata_block(o.consistency, inexact)
    if carried_rec is not None:
        metadata["extra_bands"] = xb.metadata_block(numbers, carried_rec["ranges"], w_rgb, carried_rec["r"], carried_rec["eps"], carried_rec["inexact"])
    if defs is not None:
        out_geo = georef.scaled(scale)
        metadata["indices"] = []
        for d, ramp, r in zip(defs, ramps, found):
            tif = final_output.with_name(f"{final_output.stem}_{d['name']}.tif")
            rio.write_geotiff_i16(tif, r["index"], out_geo, nodata=xi.NODATA)
            rio.write_png(tif.with_suffix(".png"), r["rgba"])
            stats = xi.stats_from_hist(r["hist"], d["K"], pixel_size=out_geo.pixel_size)
            metadata["indices"].append(xi.metadata_entry(d, r["undefined"], stats, ramp, {"tif": str(tif), "png": str(tif.with_suffix(".png"))},
                                                         None if label is None else xi.zonal_table(r["zonal"], d["K"])))
        if burnt is not None:
            ztif = final_output.with_name(f"{final_output.stem}_zones.tif")
            rio.write_geotiff_u16(ztif, burnt["labels"][..., None], out_geo, nodata=0)
            metadata["zones"] = xz.metadata_block(burnt["source"], burnt["features"], burnt["table"], burnt["dropped"], burnt["grid"], 1, ztif,
                                                  burnt["area"], out_geo.pixel_size)
        if seg is not None:
            ztif = final_output.with_name(f"{final_output.stem}_zones.tif")
            rio.write_geotiff_u16(ztif, seg["labels"][..., None], out_geo, nodata=0)
            tables = {e["name"]: e["zones"] for e in metadata["indices"]}
            gj = xf.write_geojson(final_output.with_name(f"{final_output.stem}_fields.geojson"),
                                  xf.to_geojson(xf.polygons(seg["rings"], seg["fields"]), out_geo, out_geo.pixel_size, tables))
            metadata["zones"] = xf.metadata_block(seg["params"], seg["found"], seg["fields"], seg["labels"].shape, ztif, gj, out_geo.pixel_size)
        if manage is not None:
            mtif = final_output.with_name(f"{final_output.stem}_mzones.tif")
            rio.write_geotiff_u8(mtif, manage["result"]["zone"][..., None], out_geo, nodata=0)
            rows = xm.zone_rows(manage["result"]["table"], manage["result"]["status"], manage["params"], out_geo.pixel_size)
            mgj = None
            if manage["params"]["polygons"]:
                mgj = xm.write_geojson(final_output.with_name(f"{final_output.stem}_mzones.geojson"), xm.to_geojson(manage["rings"], rows, out_geo))
            metadata.setdefault("zones", {})["management"] = xm.metadata_block(manage["params"], manage["result"], rows, mtif, mgj)
    return final_output, metadata


def apply_wow_sr(input_path: Path, output_path: Path, enhance_crops: bool = True,
                 model: str = "realesrgan_x4", bit_depth: int = 8, seam_blend: bool = False, display=None, nodata=None,
                 fill_radius: int = 32, consistency=None, extra_bands=None, extra_weights=None, indices=None, index_offset: int = 0,
                 zones=None) -> Tuple[Path, dict]:
    """Reference wow_sr.py:28-184 -- same outputs (GeoTIFF and/or PNG) and metadata dict.  bit_depth=16 (not in the reference): a
    uint16 GeoTIFF goes through the net without the 8-bit squeeze and comes back as a uint16 GeoTIFF (_apply_wow_sr16).
    display (bit_depth=16 only; a s2sr.display.Stretch or a dict of its fields): the job also writes the PNG, from the output's
    display rendering (percentile stretch); enhance_crops then runs on that image; the metadata gains "display", and only then.
    seam_blend (not in the reference): the tiled stitch cross-fades the window overlaps (RealESRGAN(seam_blend=True)); the metadata
    gains "seam_blend": true, and only then.
    nodata (not in the reference): None, an integer, or "tag" = the file's GDAL_NODATA tag (a ValueError if it
    has none).  A pixel whose bands 1-3 all equal it was never measured: it is filled from its nearest valid neighbour within
    fill_radius (1..64) in front of the net, the post-process runs on the filled image, and the outputs say which pixels they
    are -- the GeoTIFF carries the GDAL_NODATA tag and the value in those pixels, the PNG is RGBA with alpha 255 x mask.  The
    metadata gains "nodata": {"value", "invalid_pixels", "fill_radius"}, and only then.
    consistency (not in the reference): None, "exact" or "smooth" -- the block means of the super-resolved image
    reproduce the input pixels (RealESRGAN(consistency=...)).  The metadata gains "consistency": {"mode", "inexact_blocks": [r, g,
    b]}, and only then; with enhance_crops the block also says "applied_before": "post_process" -- the crop-visibility step
    changes radiometry on purpose, so the written 8-bit image is consistent only up to it.
    extra_bands, extra_weights (bit_depth=16 only; not in the reference): see _apply_wow_sr16.  The GeoTIFF gains
    the carried bands behind R, G, B and the metadata "extra_bands": {"bands", "ranges", "weights_rgb", "r", "eps", "gain_limit",
    "inexact_blocks"}, and only then.
    indices, index_offset, zones (bit_depth=16 only; not in the reference): see _apply_wow_sr16.  Two files per index
    next to the GeoTIFF and "indices" in the metadata, and only then."""
    from s2sr import rasterio_lite as rio

    o = JobOptions(seam_blend=seam_blend, bit_depth=bit_depth, display=display, nodata=nodata, fill_radius=fill_radius, consistency=consistency,
                   extra_bands=extra_bands, extra_weights=extra_weights, indices=indices, index_offset=index_offset, zones=zones)
    o.check(enhance_crops)
    if bit_depth == 16:
        return _apply_wow_sr16(input_path, output_path, model, enhance_crops, o)

    model_display = {"realesrgan_x4": "Real-ESRGAN x4",
                     "realesrgan_anime": "Real-ESRGAN Anime 6B (text/plates)",
                     "realesrgan_x2plus": "Real-ESRGAN x2plus (5 m)",
                     "realesr_general_x4v3": "Real-ESRGAN general-x4v3 (compact)",
                     "realesr_general_wdn_x4v3": "Real-ESRGAN general-wdn-x4v3 (compact, denoising)",
                     "realesr_animevideov3": "Real-ESRGAN animevideov3 (compact)"}.get(model, model)
    print(f"\nWOW Super-Resolution ({model_display} + Enhanced)\n   Input: {input_path}")
    input_path = Path(input_path)
    valid = value = None
    if nodata is None:
        img, georef = rio.read_rgb_u8(input_path)           # u8 RGB (min-max normalised if >255, :67-73)
    else:
        img, georef, valid, value = read_masked(input_path, nodata)
    # the 8-bit image's invalid pixels get the value where it is one of its own, 0 otherwise (the mask is the truth: alpha, metadata)
    out_nodata = value if valid is not None and 0 <= value <= 255 and value == int(value) else 0
    original_shape = img.shape[:2]

    pipeline_stages = []
    print(f"   Stage 1/2: {model_display} (GAN upscaling)...")
    esrgan = RealESRGAN(model_name=model, tile_size=256, **o.passed("RealESRGAN"))
    # RGB2BGR -> enhance -> BGR2RGB -> _enhance_for_crops (:85-110) as ONE native call: the 16x image crosses PCIe once
    if enhance_crops:
        print("   Stage 2/2: Crop visibility enhancement...")
    if valid is not None:
        output_rgb = esrgan.enhance_job(img, native.pp_wow() if enhance_crops else None, valid=valid, nodata=int(out_nodata), fill_radius=fill_radius)
    elif hasattr(esrgan, "enhance_job"):
        output_rgb = esrgan.enhance_job(img, native.pp_wow() if enhance_crops else None)
    else:      # an operator with the reference's interface only: the reference's own sequence
        output_rgb = np.ascontiguousarray(esrgan.enhance(np.ascontiguousarray(img[:, :, ::-1]))[:, :, ::-1])   # the net is fed BGR (:85,94)
        if enhance_crops:
            output_rgb = _enhance_for_crops(output_rgb)
    scale = esrgan.scale
    inexact = None if consistency is None else esrgan.last_inexact_blocks
    del esrgan
    pipeline_stages.append({"model": model, "scale": scale, "purpose": "GAN upscaling"})
    if enhance_crops:
        pipeline_stages.append({"post_processing": "Enhanced", "purpose": "Crop visibility"})
    final_shape = output_rgb.shape[:2]

    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    output_png = output_path.with_suffix(".png")
    if georef is not None:
        final_output = output_path.with_suffix(".tif")
        # the two encoders side by side (both are thread pools over strips / bands of the same array)
        rio.write_outputs(output_rgb, output_png, final_output, georef.scaled(scale), remember=True,       # pixel size / scale (:128-135)
                          **dict({} if valid is None else {"nodata": out_nodata}, **_alpha_of(valid, scale)))
    else:
        final_output = output_png
        rio.write_png(output_png, output_rgb, **_alpha_of(valid, scale))

    metadata = {
        "input_file": str(input_path),
        "output_file": str(final_output),
        "scale": scale,
        "pipeline": "Real-ESRGAN x4 + Enhanced",
        "stages": pipeline_stages,
        "enhancements": (["CLAHE local contrast", "Unsharp mask", "Vegetation boost"] if enhance_crops else []),
        "original_size": list(original_shape),
        "output_size": list(final_shape),
        "original_resolution_m": 10.0,
        "effective_resolution_m": 10.0 / scale,
        "optimized_for": "z18_crop_visibility",
    }
    if seam_blend:
        metadata["seam_blend"] = True
    if valid is not None:
        metadata["nodata"] = _nodata_block(value, valid, fill_radius)
    if consistency is not None:
        from s2sr.consistency import metadata_block
        metadata["consistency"] = metadata_block(consistency, inexact, "post_process" if enhance_crops else None)
    return final_output, metadata


def process_wow_sr(input_tif: Path, output_dir: Path, enhance_crops: bool = True,
                   model: str = "realesrgan_x4", bit_depth: int = 8, seam_blend: bool = False, display=None, nodata=None,
                   fill_radius: int = 32, consistency=None, extra_bands=None, extra_weights=None, indices=None, index_offset: int = 0,
                   zones=None) -> dict:
    """Reference wow_sr.py:212-266 -- file naming, metadata JSON and result dict schema.  bit_depth=16: see apply_wow_sr (no PNG:
    "sr_png" is None -- unless `display` is given: the PNG is the output's display rendering).  seam_blend, nodata, fill_radius,
    consistency, extra_bands, extra_weights, indices, index_offset, zones: see apply_wow_sr; "outputs" gains "indices": {name: {"tif",
    "png"}} with indices, and only then."""
    o = JobOptions(seam_blend=seam_blend, bit_depth=bit_depth, display=display, nodata=nodata, fill_radius=fill_radius, consistency=consistency,
                   extra_bands=extra_bands, extra_weights=extra_weights, indices=indices, index_offset=index_offset, zones=zones)
    o.check(enhance_crops)       # before anything is created
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    base_name = Path(input_tif).stem
    wow_tif = output_dir / f"{base_name}_wow_sr.tif"
    png = wow_tif.with_suffix(".png")
    # (tests patch apply_wow_sr with the reference's signature: a plain job names nothing beyond it)
    _, sr_metadata = apply_wow_sr(input_path=input_tif, output_path=wow_tif, enhance_crops=enhance_crops, model=model, **o.passed("apply_wow_sr"))
    if bit_depth == 16 and display is None:
        png = None   # (a PNG an earlier 8-bit job left under this name is not this job's output)
    result = {
        "timestamp": datetime.now().strftime("%Y%m%d_%H%M%S"),
        "input": str(input_tif),
        "outputs": {"sr_tif": str(wow_tif) if wow_tif.exists() else None,
                    "sr_png": str(png) if png is not None and png.exists() else None},
        "sr_metadata": sr_metadata,
    }
    if indices is not None:
        result["outputs"]["indices"] = {e["name"]: dict(e["files"]) for e in sr_metadata.get("indices", [])}
    if "file" in sr_metadata.get("zones", {}):       # field polygons were rasterised: the label raster the job wrote
        result["outputs"]["zones_tif"] = sr_metadata["zones"]["file"]
        if sr_metadata["zones"].get("geojson"):      # the fields were segmented from the image
            result["outputs"]["fields_geojson"] = sr_metadata["zones"]["geojson"]
    if "management" in sr_metadata.get("zones", {}):      # management zones inside the fields
        result["outputs"]["management_tif"] = sr_metadata["zones"]["management"]["file"]
        if sr_metadata["zones"]["management"].get("geojson"):
            result["outputs"]["management_geojson"] = sr_metadata["zones"]["management"]["geojson"]
    with open(output_dir / f"{base_name}_wow_sr_metadata.json", "w") as f:
        json.dump(result, f, indent=2)
    return result


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="WOW Super-Resolution (MI355X)")
    ap.add_argument("input")
    ap.add_argument("-o", "--output", default="./wow_sr_output")
    ap.add_argument("--no-enhance", action="store_true")
    a = ap.parse_args()
    print(process_wow_sr(Path(a.input), Path(a.output), enhance_crops=not a.no_enhance)["outputs"])
