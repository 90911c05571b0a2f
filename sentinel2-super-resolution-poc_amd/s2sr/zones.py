"""Host-side policy of field polygons as zones: reading GeoJSON, projecting its vertices onto the label grid of a
job, quantising them, numbering the labels, and the "zones" block of a job's metadata.  numpy only.  The device work -- features
made of rings to a uint16 label raster and the pixels per label -- is csrc/zones.hip, behind native.Engine.zones_rasterize_u16.

A job's `zones` option takes, besides a label raster (an array, or the path of a label GeoTIFF; s2sr/index.py check_zones):
  a GeoJSON source    the path of a .geojson / .json file, a parsed FeatureCollection, a Feature, a bare geometry, or a list of those
  {"geojson": source, "property": name}    features that share the property's value share a label

Coordinates are lon / lat (RFC 7946); a legacy `crs` member that names an EPSG code geo.CRS supports is honoured.  Only vertices
are projected: an edge is the straight segment between its projected ends on the label grid (DESIGN.md 7.9 says what that costs).
The rasteriser's rule gives a pixel to the feature that holds its centre, and a pixel on a shared edge to one neighbour; how that
treats real field boundaries is unmeasured."""
from __future__ import annotations

import json
import re
from pathlib import Path
from typing import Optional

import numpy as np

from . import geo

SUB = 256                         # coordinate units per label pixel
COORD_MAX = 2 ** 29
MAX_LABELS = 65535
_SUFFIXES = (".geojson", ".json")
_GEOMETRIES = ("Polygon", "MultiPolygon")


def is_geojson(value) -> bool:
    """whether a job's `zones` value is a GeoJSON source (or the dict that wraps one), not a label raster"""
    if isinstance(value, dict):
        return True
    if isinstance(value, (str, Path)):
        return Path(value).suffix.lower() in _SUFFIXES
    return isinstance(value, (list, tuple)) and len(value) > 0 and all(isinstance(v, (dict, str, Path)) and is_geojson(v) for v in value)


def split_option(value):
    """a job's GeoJSON `zones` value -> (source, property name or None)"""
    if isinstance(value, dict) and "geojson" in value:
        unknown = set(value) - {"geojson", "property"}
        if unknown:
            raise ValueError(f"zones: unknown field(s) {sorted(unknown)} next to \"geojson\"")
        prop = value.get("property")
        if prop is not None and not isinstance(prop, str):
            raise ValueError(f"zones: \"property\" must be a property's name, got {prop!r}")
        return value["geojson"], prop
    return value, None


def _epsg_of_crs_member(crs) -> int:
    """the EPSG code of a legacy GeoJSON `crs` member (GeoJSON 2008: {"type": "name", "properties": {"name": ...}})"""
    name = crs.get("properties", {}).get("name") if isinstance(crs, dict) and crs.get("type") == "name" else None
    if not isinstance(name, str):
        raise ValueError(f"zones: the crs member {crs!r} is not a named CRS")
    if re.fullmatch(r"urn:ogc:def:crs:OGC:[\d.]*:CRS84", name):
        return 4326
    m = re.fullmatch(r"(?:urn:ogc:def:crs:EPSG:[\d.]*:|EPSG:)(\d+)", name)
    if not m:
        raise ValueError(f"zones: the crs {name!r} names no EPSG code")
    epsg = int(m.group(1))
    geo.CRS(epsg).kind                                            # ValueError for a CRS geo.py does not know
    return epsg


def _rings_of(geometry, index: int) -> list:
    kind = geometry.get("type") if isinstance(geometry, dict) else None
    if kind not in _GEOMETRIES:
        raise ValueError(f"zones: feature {index} has geometry type {kind!r}; Polygon and MultiPolygon are handled")
    polys = [geometry.get("coordinates")] if kind == "Polygon" else geometry.get("coordinates")
    rings = []
    try:
        for poly in polys:
            for ring in poly:
                pts = [(float(p[0]), float(p[1])) for p in ring]
                if len(pts) > 1 and pts[0] == pts[-1]:
                    pts.pop()                                     # the closing vertex: the edge last -> first is implied
                if len(pts) < 3:
                    raise ValueError(f"zones: feature {index} has a ring of fewer than 3 distinct vertices")
                rings.append(pts)
    except (TypeError, IndexError):
        raise ValueError(f"zones: feature {index} has malformed {kind} coordinates") from None
    return rings


def read(source) -> list:
    """A GeoJSON source -> [{"index", "rings": [[(x, y), ...], ...], "properties", "id", "epsg"}], one per Feature, in the file's
    order.  source: the path of a .geojson / .json file, a parsed FeatureCollection, a Feature, a bare geometry, or a list of
    those.  ValueError: a geometry that is no Polygon / MultiPolygon (with the feature's index and type), a crs member that
    names anything but an EPSG code geo.CRS supports, anything that is no GeoJSON."""
    out = []

    def take(obj, epsg):
        if isinstance(obj, (str, Path)):
            path = Path(obj)
            if path.suffix.lower() not in _SUFFIXES:
                raise ValueError(f"zones: {path} is no .geojson / .json file")
            with open(path) as f:
                obj = json.load(f)
        if isinstance(obj, (list, tuple)):
            for o in obj:
                take(o, epsg)
            return
        if not isinstance(obj, dict) or "type" not in obj:
            raise ValueError(f"zones: {type(obj).__name__} is no GeoJSON object")
        if obj.get("crs") is not None:
            epsg = _epsg_of_crs_member(obj["crs"])
        kind = obj["type"]
        if kind == "FeatureCollection":
            feats = obj.get("features")
            if not isinstance(feats, list):
                raise ValueError("zones: a FeatureCollection without a list of features")
            for f in feats:
                if not isinstance(f, dict) or f.get("type") != "Feature":
                    raise ValueError(f"zones: feature {len(out)} of the collection is no Feature")
                take(f, epsg)
        elif kind == "Feature":
            props = obj.get("properties") or {}
            out.append({"index": len(out), "rings": _rings_of(obj.get("geometry"), len(out)), "properties": props, "id": obj.get("id"), "epsg": epsg})
        else:
            out.append({"index": len(out), "rings": _rings_of(obj, len(out)), "properties": {}, "id": None, "epsg": epsg})

    take(source, 4326)
    if not out:
        raise ValueError("zones: the source holds no feature")
    return out


def labels_of(features, prop: Optional[str] = None):
    """-> (label per feature, [{"label", "id" or "value", "features"}]).  Default: a feature's place in the file plus 1.  With a
    property name: the features that share the property's value share a label, numbered by first appearance."""
    if prop is None:
        if len(features) > MAX_LABELS:
            raise ValueError(f"zones: {len(features)} features are more than the {MAX_LABELS} labels a uint16 raster holds")
        return [f["index"] + 1 for f in features], [{"label": f["index"] + 1, "id": f["id"], "features": 1} for f in features]
    seen, labels, table = {}, [], []
    for f in features:
        if prop not in f["properties"]:
            raise ValueError(f"zones: feature {f['index']} has no property {prop!r}")
        v = f["properties"][prop]
        key = json.dumps(v, sort_keys=True)
        if key not in seen:
            if len(seen) == MAX_LABELS:
                raise ValueError(f"zones: the property {prop!r} takes more than {MAX_LABELS} values")
            seen[key] = len(seen) + 1
            table.append({"label": seen[key], "value": v, "features": 0})
        labels.append(seen[key])
        table[seen[key] - 1]["features"] += 1
    return labels, table


def quantise(p):
    """label-grid coordinates (pixels, float64) -> units of 1 / 256 pixel: floor(256 p + 0.5)"""
    return np.floor(SUB * np.asarray(p, np.float64) + 0.5)


def to_grid(features, georef, in_shape, scale: int, zone_scale: int = 1) -> dict:
    """Features of read() -> the rasteriser's tables on the label grid of ceil(scale H / zone_scale) x ceil(scale W / zone_scale)
    of an input raster of in_shape = (H, W) placed by georef (s2sr.rasterio_lite.GeoRef): each vertex through geo.CRS.from_lonlat
    and the raster's placement, quantised as floor(256 p + 0.5) in float64.  A feature whose bounding box misses the grid is
    dropped and counted.  -> {"xy", "ring_start", "feat_start", "kept" (the features' indices), "dropped", "grid"}.
    ValueError: a raster without placement tags or with a CRS geo.CRS does not support, a coordinate beyond +-2^29 (or not
    finite) on a feature that meets the grid."""
    from .rasterio_lite import TAG_GEOKEYS
    tags = getattr(georef, "tags", None) or {}
    place = geo.placement_from_tags(tags)
    epsg = geo.epsg_from_geokeys(tags.get(TAG_GEOKEYS))
    if place is None or epsg is None:
        raise ValueError("zones: the input raster has no georeference (placement tags and an EPSG code) to put the polygons on")
    crs = geo.CRS(epsg)
    crs.kind                                                      # ValueError for an unsupported CRS
    scale, zone_scale = int(scale), int(zone_scale)
    if scale < 1 or zone_scale < 1:
        raise ValueError("zones: scale and zone_scale must be >= 1")
    H, W = in_shape
    GH, GW = -(-scale * H // zone_scale), -(-scale * W // zone_scale)
    xy, ring_start, feat_start, kept, dropped = [], [0], [0], [], 0
    for f in features:
        rings = []
        for ring in f["rings"]:
            a = np.asarray(ring, np.float64)
            lon, lat = (a[:, 0], a[:, 1]) if f["epsg"] == 4326 else geo.CRS(f["epsg"]).to_lonlat(a[:, 0], a[:, 1])
            x, y = (a[:, 0], a[:, 1]) if f["epsg"] == epsg else crs.from_lonlat(lon, lat)
            px = (np.asarray(x, np.float64) - place.x0) / place.dx * scale / zone_scale
            py = (place.y0 - np.asarray(y, np.float64)) / place.dy * scale / zone_scale
            rings.append(np.stack([quantise(px), quantise(py)], axis=1))
        q = np.concatenate(rings)
        if not np.isfinite(q).all():
            raise ValueError(f"zones: feature {f['index']} has a vertex that does not project to a finite position")
        if q[:, 0].max() < 0 or q[:, 0].min() >= SUB * GW or q[:, 1].max() < 0 or q[:, 1].min() >= SUB * GH:
            dropped += 1
            continue
        if np.abs(q).max() > COORD_MAX:
            raise ValueError(f"zones: feature {f['index']} meets the grid and reaches beyond +-2^29 units of 1 / 256 pixel ({np.abs(q).max():.0f})")
        for r in rings:
            xy.append(r.astype(np.int32))
            ring_start.append(ring_start[-1] + len(r))
        feat_start.append(len(ring_start) - 1)
        kept.append(f["index"])
    return {"xy": np.concatenate(xy).reshape(-1, 2) if xy else np.zeros((0, 2), np.int32), "ring_start": np.array(ring_start, np.int32),
            "feat_start": np.array(feat_start, np.int32), "kept": kept, "dropped": dropped, "grid": (GH, GW)}


def metadata_block(source, features, table, dropped: int, grid, zone_scale: int, file, area, pixel_size) -> dict:
    """the "zones" block of a job's metadata.  table: labels_of()'s; area: uint64 [Z + 1] from the rasteriser; pixel_size: the
    output pixel's (x, y) in metres (or None: no hectares)."""
    ha = None if pixel_size is None else abs(float(pixel_size[0]) * float(pixel_size[1])) * zone_scale * zone_scale / 10000.0
    rows = []
    for t in table:
        px = int(area[t["label"]]) if t["label"] < len(area) else 0
        rows.append(dict(t, pixels=px, area_ha=None if ha is None else px * ha))
    return {"source": str(source) if isinstance(source, (str, Path)) else "inline", "features": int(features), "labels": rows, "dropped": int(dropped),
            "grid": [int(grid[0]), int(grid[1])], "zone_scale": int(zone_scale), "file": None if file is None else str(file)}


def rasterize(engine, value, georef, in_shape, scale: int, zone_scale: int = 1, band_rows: int = 0) -> dict:
    """A job's GeoJSON `zones` value through `engine` (native.Engine) -> {"labels" uint16 [GH, GW], "Z", "area", "table", "features",
    "dropped", "grid", "source"}.  The labels are a copy of the engine's own: they outlive its next call."""
    source, prop = split_option(value)
    feats = read(source)
    labels, table = labels_of(feats, prop)
    g = to_grid(feats, georef, in_shape, scale, zone_scale)
    Z = max(labels)
    if not g["kept"]:
        raise ValueError(f"zones: none of the {len(feats)} features meets the raster")
    lab = np.array([labels[i] for i in g["kept"]], np.uint16)
    with engine.chain_lock:          # the call voids what the engine kept: not between another job's door and its readers
        out, area = engine.zones_rasterize_u16(g["xy"], g["ring_start"], g["feat_start"], lab, Z, g["grid"], band_rows=band_rows)
        out = np.array(out)
    return {"labels": out, "Z": Z, "area": area, "table": table, "features": len(feats), "dropped": g["dropped"], "grid": g["grid"], "source": source}
