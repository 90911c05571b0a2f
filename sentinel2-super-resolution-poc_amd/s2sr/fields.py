"""Host-side policy of fields from the image: a job's `zones` option in its "segment" form, index units and hectares
turned into the integers of the device pass, the rings of the labels grouped into polygons, the GeoJSON of the fields and the "zones"
block of a job's metadata.  numpy only.  The device work -- an int16 index raster to uint16 labels and the fields table -- is
csrc/fields.hip behind native.Engine.fields_segment_i16; the rings are csrc/ring_trace.h behind native.Engine.labels_trace_u16.

A job's `zones` option takes, besides a label raster and field polygons (s2sr/zones.py):
  {"segment": {"index": "ndvi", "min": 0.3, "max": None, "open": 1, "close": 2, "connectivity": 4, "min_area_ha": 0.5}}
index names one of the job's indices; min / max are in index units (None: no bound on that side); open / close are the radii of the
morphological open and close in output pixels (0..8); min_pixels may be given instead of min_area_ha, one of the two must be.
Defaults: min 0.3, max None, open 1, close 2, connectivity 4.  What these defaults do on real scenes is unmeasured.

One more key cuts touching fields apart (native.Engine.fields_split_i16):
  "split": True | {"core": 0.5, "core_px": 2, "edge": None, "edge_smooth": 1}
core in (0, 1]: a core pixel lies at least that fraction of its blob's largest distance from the blob's outside, and at least
core_px pixels (0..255); edge: a gradient of the index, in index units per output pixel, above which a pixel is a field boundary
(None: no such test); edge_smooth: the radius of the box sum in front of the gradient (0..4).  True takes these defaults.  Without
the key nothing changes, byte for byte."""
from __future__ import annotations

import json
import math
from pathlib import Path

import numpy as np

from . import geo

MAX_LABELS = 65535
KEYS = ("index", "min", "max", "open", "close", "connectivity", "min_area_ha", "min_pixels", "split")
SPLIT_KEYS = ("core", "core_px", "edge", "edge_smooth")
SPLIT_DEFAULTS = {"core": 0.5, "core_px": 2, "edge": None, "edge_smooth": 1}
DEFAULTS = {"min": 0.3, "max": None, "open": 1, "close": 2, "connectivity": 4}
LIMIT = 32767                     # the index values a bound may name: -32768 is nodata


def is_segment(value) -> bool:
    """whether a job's `zones` value is the segment form"""
    return isinstance(value, dict) and "segment" in value


def check_split(value) -> dict:
    """the "split" value of a segment option -> its fields with the defaults filled in; ValueError: neither True nor a dict, an
    unknown key, core outside (0, 1], core_px outside 0..255, a non-positive or non-finite edge, edge_smooth outside 0..4"""
    if value is True:
        return dict(SPLIT_DEFAULTS)
    if not isinstance(value, dict):
        raise ValueError(f"zones: segment split {value!r}: True, or a dict of {', '.join(SPLIT_KEYS)}")
    unknown = set(value) - set(SPLIT_KEYS)
    if unknown:
        raise ValueError(f"zones: segment split has unknown key(s) {sorted(unknown)}; known are {', '.join(SPLIT_KEYS)}")
    p = dict(SPLIT_DEFAULTS, **value)
    if isinstance(p["core"], bool) or not isinstance(p["core"], (int, float)) or not math.isfinite(p["core"]) or not 0 < p["core"] <= 1:
        raise ValueError(f"zones: segment split core {p['core']!r}: a fraction in (0, 1]")
    if round(1000 * p["core"]) < 1:
        raise ValueError(f"zones: segment split core {p['core']!r}: below a thousandth")
    if isinstance(p["core_px"], bool) or not isinstance(p["core_px"], int) or not 0 <= p["core_px"] <= 255:
        raise ValueError(f"zones: segment split core_px {p['core_px']!r}: an integer in 0..255 pixels")
    if p["edge"] is not None and (isinstance(p["edge"], bool) or not isinstance(p["edge"], (int, float)) or not math.isfinite(p["edge"]) or p["edge"] <= 0):
        raise ValueError(f"zones: segment split edge {p['edge']!r}: a positive number of index units per pixel, or None")
    if isinstance(p["edge_smooth"], bool) or not isinstance(p["edge_smooth"], int) or not 0 <= p["edge_smooth"] <= 4:
        raise ValueError(f"zones: segment split edge_smooth {p['edge_smooth']!r}: a radius in 0..4 pixels")
    return p


def check_option(option) -> dict:
    """The refusals that need neither the job's indices nor its pixel size, as ValueError -> the option's fields with the defaults
    filled in: an unknown key, min > max, a radius outside 0..8, a connectivity other than 4 or 8, both size options or neither."""
    if not is_segment(option):
        raise ValueError(f"zones: {option!r} is no {{\"segment\": ...}} option")
    if set(option) != {"segment"}:
        raise ValueError(f"zones: unknown field(s) {sorted(set(option) - {'segment'})} next to \"segment\"")
    seg = option["segment"]
    if not isinstance(seg, dict):
        raise ValueError(f"zones: \"segment\" takes a dict of {', '.join(KEYS)}, got {seg!r}")
    unknown = set(seg) - set(KEYS)
    if unknown:
        raise ValueError(f"zones: segment has unknown key(s) {sorted(unknown)}; known are {', '.join(KEYS)}")
    p = dict(DEFAULTS, **seg)
    if not isinstance(p.get("index"), str):
        raise ValueError(f"zones: segment needs \"index\", the name of one of the job's indices, got {p.get('index')!r}")
    for k in ("min", "max"):
        if p[k] is not None and (isinstance(p[k], bool) or not isinstance(p[k], (int, float)) or not math.isfinite(p[k])):
            raise ValueError(f"zones: segment {k} {p[k]!r}: a number in index units, or None")
    if p["min"] is not None and p["max"] is not None and p["min"] > p["max"]:
        raise ValueError(f"zones: segment min {p['min']} > max {p['max']}")
    for k in ("open", "close"):
        if isinstance(p[k], bool) or not isinstance(p[k], int) or not 0 <= p[k] <= 8:
            raise ValueError(f"zones: segment {k} {p[k]!r}: a radius in 0..8 pixels")
    if p["connectivity"] not in (4, 8) or isinstance(p["connectivity"], bool):
        raise ValueError(f"zones: segment connectivity {p['connectivity']!r}: 4 or 8")
    area, pixels = p.get("min_area_ha"), p.get("min_pixels")
    if (area is None) == (pixels is None):
        raise ValueError("zones: segment needs exactly one of min_area_ha and min_pixels")
    if area is not None and (isinstance(area, bool) or not isinstance(area, (int, float)) or not math.isfinite(area) or area <= 0):
        raise ValueError(f"zones: segment min_area_ha {area!r}: a positive number of hectares")
    if pixels is not None and (isinstance(pixels, bool) or not isinstance(pixels, int) or pixels < 1):
        raise ValueError(f"zones: segment min_pixels {pixels!r}: an integer >= 1")
    if "split" in p:
        p["split"] = check_split(p["split"])
    return p


def check_index(p, index_defs) -> int:
    """the place of the option's index among the job's (s2sr.index.resolve's list); ValueError when it is not one of them"""
    names = [d["name"] for d in index_defs]
    if p["index"] not in names:
        raise ValueError(f"zones: segment index {p['index']!r} is not among the job's indices {names}")
    return names.index(p["index"])


def resolve(option, index_defs, pixel_area_m2) -> dict:
    """A job's segment option -> the integers of the device pass: {"index" (its place in index_defs), "name", "K", "lo", "hi", "r_open",
    "r_close", "conn", "min_pixels"} with lo = round(K min), hi = round(K max), both kept inside -32767..32767, and min_pixels =
    ceil(10000 min_area_ha / pixel_area_m2); only when the option has "split", also "split": {"core_q": round(1000 core), "core_px",
    "edge": 0 or round(K edge) kept inside 1..32767, "edge_r"}.  index_defs: s2sr.index.resolve's list.  ValueError: check_option's, an index that is
    not among the job's, min_area_ha for a raster without a pixel size."""
    p = check_option(option)
    at = check_index(p, index_defs)
    K = int(index_defs[at]["K"])
    lo = -LIMIT if p["min"] is None else min(max(int(round(K * p["min"])), -LIMIT), LIMIT)
    hi = LIMIT if p["max"] is None else min(max(int(round(K * p["max"])), -LIMIT), LIMIT)
    if lo > hi:
        raise ValueError(f"zones: segment min {p['min']} > max {p['max']} in units of 1 / {K}")
    if p.get("min_pixels") is not None:
        min_pixels = int(p["min_pixels"])
    else:
        if pixel_area_m2 is None or not pixel_area_m2 > 0:
            raise ValueError("zones: segment min_area_ha needs a raster with a pixel size; pass min_pixels")
        min_pixels = max(1, math.ceil(10000.0 * float(p["min_area_ha"]) / float(pixel_area_m2)))
    out = {"index": at, "name": p["index"], "K": K, "lo": lo, "hi": hi, "r_open": p["open"], "r_close": p["close"], "conn": p["connectivity"],
           "min_pixels": min_pixels}
    if "split" in p:
        sp = p["split"]
        out["split"] = {"core_q": int(round(1000 * sp["core"])), "core_px": sp["core_px"],
                        "edge": 0 if sp["edge"] is None else max(1, min(LIMIT, int(round(K * sp["edge"])))), "edge_r": sp["edge_smooth"]}
    return out


def segment(engine, idx, params) -> dict:
    """An int16 index raster through `engine` (native.Engine) with resolve()'s params -> {"labels" uint16 [H, W], "fields" int64
    [found + 1][6], "found", "rings": (xy, ring_start, ring_label)}.  The labels are a copy of the engine's own: they outlive its
    next call.  With "split" among the params the fields are native.Engine.fields_split_i16's.  ValueError: no field found, more
    than 65535 fields."""
    kw = dict(r_open=params["r_open"], r_close=params["r_close"], conn=params["conn"], min_pixels=params["min_pixels"], Z=MAX_LABELS)
    with engine.chain_lock:          # the call voids what the engine kept: not between another job's door and its readers
        if "split" in params:        # touching fields cut apart
            labels, fields, found = engine.fields_split_i16(idx, params["lo"], params["hi"], split=params["split"], **kw)
        else:
            labels, fields, found = engine.fields_segment_i16(idx, params["lo"], params["hi"], **kw)
        labels = np.array(labels)
    if found < 1:
        raise ValueError(f"zones: segment found no field of at least {params['min_pixels']} pixels with {params['name']} in "
                         f"[{params['lo'] / params['K']}, {params['hi'] / params['K']}]")
    if found > MAX_LABELS:
        raise ValueError(f"zones: segment found {found} fields, more than the {MAX_LABELS} labels a uint16 raster holds: raise the minimum area")
    return {"labels": labels, "fields": fields[:found + 1].copy(), "found": found, "rings": engine.labels_trace_u16(labels, found)}


def zonal(engine, d, out16, carried, valid, labels, Z: int):
    """The per-zone sums (int64 [Z + 1][3]) of one index of a job from host arrays: d is the index's record of
    RealESRGAN.product16 (a, b either ("img", channel of out16) or ("extra", i), offset, L, K), out16 and carried the job's
    product, valid its mask on the input grid or None."""
    (ka, ca), (kb, cb) = d["a"], d["b"]
    a = out16 if ka == "img" else np.ascontiguousarray(carried[..., ca])
    b = np.ascontiguousarray(out16[..., cb]) if kb == "img" else np.ascontiguousarray(carried[..., cb])
    with engine.chain_lock:
        r = engine.index_nd_u16(a, b, ca=ca if ka == "img" else 0, cb=0, offset=d.get("offset", 0), L=d.get("L", 0), K=d.get("K", 10000), valid=valid,
                                valid_scale=4, zones=labels, zone_scale=1, Z=int(Z), want=("zonal",))
        return np.array(r["zonal"])


def _area2(ring) -> int:
    """twice the signed area with y down: negative for an exterior (counterclockwise on a north-up map)"""
    x, y = ring[:, 0].astype(np.int64), ring[:, 1].astype(np.int64)
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def _holds(ring, px: float, py: float) -> bool:
    """even-odd: the vertical edges right of the point whose span holds py (the point has half-integer coordinates, the ring integer ones)"""
    x, y = ring[:, 0], ring[:, 1]
    xn, yn = np.roll(x, -1), np.roll(y, -1)
    crossing = (x == xn) & (x > px) & (np.minimum(y, yn) < py) & (np.maximum(y, yn) > py)
    return bool(int(crossing.sum()) & 1)


def polygons(rings, fields) -> list:
    """The tracer's rings (xy, ring_start, ring_label) grouped per label -> [{"label", "pixels", "bbox", "polygons": [[exterior, hole,
    ...], ...]}] for the labels 1 .. len(fields) - 1, rings as int arrays [n, 2] of pixel corners, not closed.  A ring of negative
    signed area (y down) is an exterior; every hole goes with the smallest exterior of its label that encloses it -- judged at the
    centre of the label's pixel above the hole's first vertex.  A label with several exteriors has several polygons."""
    xy, ring_start, ring_label = (np.asarray(v) for v in rings)
    by = {}
    for k, l in enumerate(ring_label.tolist()):
        by.setdefault(l, []).append(xy[ring_start[k]:ring_start[k + 1]])
    out = []
    for l in range(1, len(fields)):
        ext, holes = [], []
        for ring in by.get(l, []):
            a2 = _area2(ring)
            (ext if a2 < 0 else holes).append((abs(a2), ring))
        ext.sort(key=lambda e: e[0])                              # the smallest enclosing exterior is the first that holds the point
        polys = [[ring] for _, ring in ext]
        for _, ring in holes:
            px, py = float(ring[0, 0]) + 0.5, float(ring[0, 1]) - 0.5
            owner = next((i for i, (_, e) in enumerate(ext) if _holds(e, px, py)), None)
            if owner is None:
                raise ValueError(f"fields: a hole of label {l} lies in none of its exteriors")
            polys[owner].append(ring)
        order = sorted(range(len(polys)), key=lambda i: (int(polys[i][0][0, 1]), int(polys[i][0][0, 0])))      # by start vertex
        out.append({"label": l, "pixels": int(fields[l][0]), "bbox": [int(v) for v in fields[l][2:6]], "polygons": [polys[i] for i in order]})
    return out


def placement_of(georef):
    """-> (geo.Placement, geo.CRS) of a raster's GeoRef; ValueError for a raster without placement tags or with a CRS geo.CRS does
    not support: what the job asks before the net runs"""
    from .rasterio_lite import TAG_GEOKEYS
    tags = getattr(georef, "tags", None) or {}
    place = geo.placement_from_tags(tags)
    epsg = geo.epsg_from_geokeys(tags.get(TAG_GEOKEYS))
    if place is None or epsg is None:
        raise ValueError("fields: the raster has no georeference (placement tags and an EPSG code) to place the polygons with")
    crs = geo.CRS(epsg)
    crs.kind                                                      # ValueError for an unsupported CRS
    return place, crs


def to_geojson(polys, georef, pixel_size=None, tables=None) -> dict:
    """polygons()'s list -> a FeatureCollection in lon / lat (RFC 7946): every corner through the raster's placement (georef: the
    s2sr.rasterio_lite.GeoRef of the label grid) and geo.CRS.to_lonlat; rings closed, exteriors counterclockwise.  Each Feature
    carries label, pixels, area_ha (None without a pixel size), bbox (the pixel box x0, y0, x1, y1, half-open) and, per index of
    tables = {name: s2sr.index.zonal_table's rows}, {name: {"mean", "std"}}.  ValueError: a raster without placement tags or with
    a CRS geo.CRS does not support."""
    place, crs = placement_of(georef)
    ha = None if pixel_size is None else abs(float(pixel_size[0]) * float(pixel_size[1])) / 10000.0

    def lonlat(ring):
        lon, lat = crs.to_lonlat(place.x0 + ring[:, 0].astype(np.float64) * place.dx, place.y0 - ring[:, 1].astype(np.float64) * place.dy)
        pts = [[float(a), float(b)] for a, b in zip(np.atleast_1d(lon), np.atleast_1d(lat))]
        return pts + [pts[0]]
    by_zone = {name: {r["zone"]: r for r in rows} for name, rows in (tables or {}).items()}
    features = []
    for f in polys:
        props = {"label": f["label"], "pixels": f["pixels"], "area_ha": None if ha is None else f["pixels"] * ha, "bbox": f["bbox"]}
        for name, rows in by_zone.items():
            r = rows.get(f["label"])
            props[name] = None if r is None else {"mean": r["mean"], "std": r["std"]}
        coords = [[lonlat(ring) for ring in poly] for poly in f["polygons"]]
        geometry = {"type": "Polygon", "coordinates": coords[0]} if len(coords) == 1 else {"type": "MultiPolygon", "coordinates": coords}
        features.append({"type": "Feature", "id": f["label"], "properties": props, "geometry": geometry})
    return {"type": "FeatureCollection", "features": features}


def metadata_block(params, found: int, fields, grid, file, geojson, pixel_size) -> dict:
    """the "zones" block of a job that segmented its fields.  params: resolve()'s; fields: int64 [found + 1][6]; pixel_size: the
    output pixel's (x, y) in metres (or None: no hectares).  "parameters" carries "split" only when the params do."""
    ha = None if pixel_size is None else abs(float(pixel_size[0]) * float(pixel_size[1])) / 10000.0
    rows = [{"label": l, "pixels": int(fields[l][0]), "area_ha": None if ha is None else int(fields[l][0]) * ha, "bbox": [int(v) for v in fields[l][2:6]]}
            for l in range(1, len(fields))]
    return {"source": "segment", "parameters": {k: params[k] for k in ("name", "K", "lo", "hi", "r_open", "r_close", "conn", "min_pixels", "split") if k in params},
            "found": int(found), "unlabelled": int(fields[0][0]), "labels": rows, "grid": [int(grid[0]), int(grid[1])], "zone_scale": 1,
            "file": None if file is None else str(file), "geojson": None if geojson is None else str(geojson)}


def write_geojson(path, collection) -> Path:
    path = Path(path)
    with open(path, "w") as f:
        json.dump(collection, f)
    return path
