"""The keyword ladders of the job path, restated as plain functions from the hand-written `**({...} if ... else {})` groups that
app/job_options.py replaced.

Transcribed from the last commit that carried them (20344e9); the line references are to that commit's app/sr_routes.py,
app/wow_sr.py and app/farm_sr.py.  tests/test_job_options_cpu.py holds JobOptions.passed to this model over every on/off
combination of the options.  Each function answers the keywords its seam's call got beyond the reference's arguments; `o` is any
object with the twelve option attributes."""


def run_wow_job(o):
    """start_wow_sr -> background_tasks.add_task(run_wow_job, ...), sr_routes.py:396-405"""
    return {**({"seam_blend": True} if o.seam_blend else {}),
            **({"bit_depth": o.bit_depth} if o.bit_depth != 8 else {}),
            **({"display": o.display} if o.display is not None else {}),
            **({"nodata": o.nodata, "fill_radius": o.fill_radius} if o.nodata is not None else {}),
            **({"consistency": o.consistency} if o.consistency is not None else {}),
            **({"extra_bands": o.extra_bands} if o.extra_bands is not None else {}),
            **({"transparent_tiles": True} if o.transparent_tiles else {}),
            **({"indices": o.indices, "index_offset": o.index_offset} if o.indices is not None else {})}


def process_wow_sr(o):
    """run_wow_job -> process_wow_sr, sr_routes.py:262-275"""
    extra = {"seam_blend": True} if o.seam_blend else {}
    if o.bit_depth != 8:
        extra["bit_depth"] = o.bit_depth
    if o.display is not None:
        extra["display"] = o.display
    if o.nodata is not None:
        extra.update(nodata=o.nodata, fill_radius=o.fill_radius)
    if o.consistency is not None:
        extra["consistency"] = o.consistency
    if o.extra_bands is not None:
        extra["extra_bands"] = o.extra_bands
    if o.indices is not None:
        extra.update(indices=o.indices, index_offset=o.index_offset)
    return extra


def apply_wow_sr(o):
    """process_wow_sr -> apply_wow_sr, wow_sr.py:371-389 (bit_depth is 8 or 16 there: _check_bit_depth ran first)"""
    blend = {"seam_blend": True} if o.seam_blend else {}
    if o.nodata is not None:
        blend.update(nodata=o.nodata, fill_radius=o.fill_radius)
    if o.consistency is not None:
        blend["consistency"] = o.consistency
    if o.extra_bands is not None:
        blend["extra_bands"] = o.extra_bands
        if o.extra_weights is not None:
            blend["extra_weights"] = o.extra_weights
    if o.indices is not None:
        blend.update(indices=o.indices, index_offset=o.index_offset, zones=o.zones)
    if o.bit_depth == 16:
        if o.display is not None:
            blend["display"] = o.display
        blend["bit_depth"] = 16
    return blend


def operator(o):
    """RealESRGAN(...), wow_sr.py:124-125, 300-301 and farm_sr.py:64-65; start_super_resolution -> run_sr_job -> process_farm_sr ->
    apply_farm_sr, sr_routes.py:313-314, 237-238 and farm_sr.py:106-107: the same two groups everywhere"""
    return {**({"seam_blend": True} if o.seam_blend else {}),
            **({"consistency": o.consistency} if o.consistency is not None else {})}


SEAMS = {"run_wow_job": run_wow_job, "process_wow_sr": process_wow_sr, "apply_wow_sr": apply_wow_sr, "RealESRGAN": operator,
         "run_sr_job": operator, "process_farm_sr": operator, "apply_farm_sr": operator}
