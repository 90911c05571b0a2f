"""Host-side policy of management zones: a job's `zones` option in its "manage" form, the per-zone rows in index
units and hectares, the class names, the GeoJSON of the zones and the "management" block of a job's metadata.  numpy only.  The
device work -- int16 index rasters and uint16 labels to a uint8 zone raster, integer k-means inside every field -- is
csrc/mzones.hip behind native.Engine.zones_kmeans_i16; the rings are csrc/ring_trace.h behind native.Engine.labels_trace_u16.

A job's `zones` option takes, besides a label raster, field polygons (s2sr/zones.py) and {"segment": ...} (s2sr/fields.py):
  {"manage": {"index": "ndvi" | ["ndvi", "ndre"], "k": 3, "iterations": 32, "min_per_zone": 10, "smooth": 1, "polygons": True},
   "fields": <any value zones takes otherwise>}
index names one to four of the job's indices, the first ranks the zones (zone 1 is its lowest class); k is the number of zones per
field (2..8), iterations the most Lloyd iterations (1..64; the pass stops at a fixed point), min_per_zone the pixels per zone a field
needs to be zoned at all (a field of fewer than k min_per_zone pixels is skipped), smooth the passes of the 3 x 3 mode filter (0..4),
polygons whether the zones are also traced and written as GeoJSON.  `fields` says where the fields come from and is handled exactly
as that value is handled without "manage".
Defaults: k 3 and min_per_zone 10 (the reference's KMeans(n_clusters=3) and its 10 pixels per zone), iterations 32, smooth 1,
polygons True.  The start centres lie on the diagonal of a field's value box and there is one start, not ten.  What k = 3, that
start and the smoothing do on real scenes is unmeasured; DESIGN.md 7.11 has what one synthetic sample showed."""
from __future__ import annotations

import math

import numpy as np

from . import fields as xf

KEYS = ("index", "k", "iterations", "min_per_zone", "smooth", "polygons")
DEFAULTS = {"k": 3, "iterations": 32, "min_per_zone": 10, "smooth": 1, "polygons": True}
MAX_INDICES = 4
RANGES = {"k": (2, 8), "iterations": (1, 64), "smooth": (0, 4)}


def is_manage(value) -> bool:
    """whether a job's `zones` value is the manage form"""
    return isinstance(value, dict) and "manage" in value


def class_names(k: int) -> list:
    """the reference's names: low / medium / high for three zones, zone_<id> otherwise"""
    return ["low", "medium", "high"] if k == 3 else [f"zone_{j}" for j in range(1, k + 1)]


def check_option(option) -> dict:
    """The refusals that need nothing but the option, as ValueError -> the manage fields with the defaults filled in and "index" as
    a list: "manage" without "fields", an unknown key, an index that is no name or list of one to four distinct names, k,
    iterations or smooth out of range, min_per_zone below 1, polygons that is no bool."""
    if not is_manage(option):
        raise ValueError(f"zones: {option!r} is no {{\"manage\": ..., \"fields\": ...}} option")
    extra = set(option) - {"manage", "fields"}
    if extra:
        raise ValueError(f"zones: unknown field(s) {sorted(extra)} next to \"manage\"")
    if "fields" not in option or option["fields"] is None:
        raise ValueError("zones: \"manage\" needs \"fields\": a label raster, field polygons or {\"segment\": ...}")
    if is_manage(option["fields"]):
        raise ValueError("zones: \"fields\" of \"manage\" cannot be a \"manage\" option itself")
    m = option["manage"]
    if not isinstance(m, dict):
        raise ValueError(f"zones: \"manage\" takes a dict of {', '.join(KEYS)}, got {m!r}")
    unknown = set(m) - set(KEYS)
    if unknown:
        raise ValueError(f"zones: manage has unknown key(s) {sorted(unknown)}; known are {', '.join(KEYS)}")
    p = dict(DEFAULTS, **m)
    index = p.get("index")
    names = [index] if isinstance(index, str) else list(index) if isinstance(index, (list, tuple)) else None
    if not names or not all(isinstance(n, str) for n in names):
        raise ValueError(f"zones: manage needs \"index\", the name of one of the job's indices or a list of them, got {index!r}")
    if len(names) > MAX_INDICES:
        raise ValueError(f"zones: manage takes at most {MAX_INDICES} indices, got {len(names)}")
    if len(set(names)) != len(names):
        raise ValueError(f"zones: manage index {names} names an index twice")
    p["index"] = names
    for key, (lo, hi) in RANGES.items():
        if isinstance(p[key], bool) or not isinstance(p[key], int) or not lo <= p[key] <= hi:
            raise ValueError(f"zones: manage {key} {p[key]!r}: an integer in {lo}..{hi}")
    if isinstance(p["min_per_zone"], bool) or not isinstance(p["min_per_zone"], int) or p["min_per_zone"] < 1:
        raise ValueError(f"zones: manage min_per_zone {p['min_per_zone']!r}: an integer >= 1")
    if not isinstance(p["polygons"], bool):
        raise ValueError(f"zones: manage polygons {p['polygons']!r}: True or False")
    return p


def check_index(p, index_defs) -> list:
    """the places of the option's indices among the job's (s2sr.index.resolve's list); ValueError when one is not among them"""
    have = [d["name"] for d in index_defs]
    for n in p["index"]:
        if n not in have:
            raise ValueError(f"zones: manage index {n!r} is not among the job's indices {have}")
    return [have.index(n) for n in p["index"]]


def resolve(option, index_defs) -> dict:
    """A job's manage option -> {"indices" (their places in index_defs), "names", "K" (one per index), "k", "iterations",
    "min_per_zone", "smooth", "polygons"}.  ValueError: check_option's, an index that is not among the job's."""
    p = check_option(option)
    at = check_index(p, index_defs)
    return {"indices": at, "names": list(p["index"]), "K": [int(index_defs[i]["K"]) for i in at], "k": p["k"], "iterations": p["iterations"],
            "min_per_zone": p["min_per_zone"], "smooth": p["smooth"], "polygons": p["polygons"]}


def run(engine, rasters, labels, Z: int, params) -> dict:
    """The named int16 index rasters and the uint16 labels through `engine` (native.Engine) with resolve()'s params -> the entry's
    dict, every array a copy of the engine's own: they outlive its next call."""
    with engine.chain_lock:          # the call voids what the engine kept: not between another job's door and its readers
        r = engine.zones_kmeans_i16(np.stack([np.asarray(a) for a in rasters]), labels, int(Z), k=params["k"], iters=params["iterations"],
                                    min_per_zone=params["min_per_zone"], smooth=params["smooth"])
        return {key: (np.array(v) if isinstance(v, np.ndarray) else int(v)) for key, v in r.items()}


def zone_rows(table, status, params, pixel_size=None) -> list:
    """The per-field rows: [{"label", "zones": [{"zone_id", "zone_class", "pixels", "area_ha", <name>: {"mean", "std"} or None, ...}]}]
    for the zoned fields (status 2), every zone id listed, one without a pixel too.  table: int64 [Z + 1][k][1 + 2 D]; mean and std
    per index in index units, as s2sr.index.zonal_table computes them; area_ha None without a pixel size."""
    ha = None if pixel_size is None else abs(float(pixel_size[0]) * float(pixel_size[1])) / 10000.0
    names = class_names(params["k"])
    rows = []
    for l in np.flatnonzero(np.asarray(status) == 2).tolist():
        zones = []
        for j in range(params["k"]):
            t = [int(v) for v in table[l][j]]
            n = t[0]
            z = {"zone_id": j + 1, "zone_class": names[j], "pixels": n, "area_ha": None if ha is None else n * ha}
            for d, (name, K) in enumerate(zip(params["names"], params["K"])):
                s, q = t[1 + 2 * d], t[2 + 2 * d]
                z[name] = None if n == 0 else {"mean": s / (n * K), "std": math.sqrt(max(n * q - s * s, 0)) / (n * K)}
            zones.append(z)
        rows.append({"label": l, "zones": zones})
    return rows


def trace(engine, zone, labels, Z: int, k: int) -> list:
    """per zone id 1..k the tracer's rings (xy, ring_start, ring_label) around where(zone == id, labels, 0)"""
    labels = np.asarray(labels)
    return [engine.labels_trace_u16(np.where(np.asarray(zone) == j, labels, 0).astype(np.uint16), int(Z)) for j in range(1, k + 1)]


def to_geojson(rings_by_zone, rows, georef) -> dict:
    """trace()'s rings and zone_rows()'s rows -> a FeatureCollection in lon / lat (RFC 7946), one Feature per (field, zone) that
    holds a pixel, ordered by field, then zone: label, zone_id, zone_class, pixels, area_ha and, per index, {"mean", "std"}.  The
    rings are grouped by s2sr.fields.polygons and placed by s2sr.fields.to_geojson.  ValueError: a raster without placement tags
    or with a CRS geo.CRS does not support."""
    by = {(r["label"], z["zone_id"]): z for r in rows for z in r["zones"]}
    Z = max([r["label"] for r in rows], default=0)
    features = []
    for j, rings in enumerate(rings_by_zone, start=1):
        pixels = np.zeros((Z + 1, 6), np.int64)
        for (l, zid), z in by.items():
            if zid == j:
                pixels[l, 0] = z["pixels"]
        held = sorted(set(np.asarray(rings[2]).tolist()))
        polys = [p for p in xf.polygons(rings, pixels) if p["label"] in held]
        for f in xf.to_geojson(polys, georef)["features"]:
            z = by[f["properties"]["label"], j]
            props = {"label": f["properties"]["label"]}
            props.update(z)
            features.append({"type": "Feature", "id": f"{props['label']}-{j}", "properties": props, "geometry": f["geometry"]})
    features.sort(key=lambda f: (f["properties"]["label"], f["properties"]["zone_id"]))
    return {"type": "FeatureCollection", "features": features}


def metadata_block(params, result, rows, file, geojson) -> dict:
    """the "management" block of a job's "zones" metadata.  params: resolve()'s; result: the entry's dict; rows: zone_rows()'s"""
    status = np.asarray(result["status"])
    return {"parameters": {"index": list(params["names"]), "K": list(params["K"]), "k": params["k"], "iterations": params["iterations"],
                           "min_per_zone": params["min_per_zone"], "smooth": params["smooth"], "polygons": params["polygons"]},
            "classes": class_names(params["k"]), "iterations": int(result["iterations"]), "zoned": int((status == 2).sum()),
            "skipped": int((status == 1).sum()), "fields": rows, "file": None if file is None else str(file),
            "geojson": None if geojson is None else str(geojson)}


write_geojson = xf.write_geojson
