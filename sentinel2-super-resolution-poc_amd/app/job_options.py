"""What a caller may ask of a job beyond the reference's signature, as one record (none of it is in the reference): the public job
functions keep their keywords, build a JobOptions at their top and hand the record inwards.  Three things live here and nowhere
else: the refusals (`check`), the keywords each call seam passes on (`passed`), and the route's way in (`from_request`).

| field             | default | meaning                                                                                   | travels when        |
|-------------------|---------|-------------------------------------------------------------------------------------------|---------------------|
| seam_blend        | False   | cross-fade the window overlaps of the tiled stitch                                        | true                |
| bit_depth         | 8       | 16: a uint16 GeoTIFF through the net in its own units                                     | not 8               |
| display           | None    | 16-bit jobs: the stretch (s2sr.display.Stretch or its fields) of the 8-bit rendering      | given               |
| nodata            | None    | the value of the pixels never measured, or "tag"                           | given               |
| fill_radius       | 32      | how far they are filled from their valid neighbours in front of the net (1..64)           | nodata is given     |
| consistency       | None    | "exact" or "smooth": block means reproduce the input pixels               | given               |
| extra_bands       | None    | 16-bit jobs: "all" or band numbers from 4 on, carried to the SR grid      | given               |
| extra_weights     | None    | the guide weights of extra_bands in R, G, B terms                                         | both are given      |
| indices           | None    | 16-bit jobs: spectral indices on the SR grid (s2sr/index.py)               | given               |
| index_offset      | 0       | the DN offset of the index definitions that name none                                     | indices are given   |
| zones             | None    | a label raster (path or array), field polygons or {"segment": ...} for per-zone tables;   | indices are given   |
|                   |         | {"manage": ..., "fields": one of those} adds management zones (s2sr/mzones.py)            |                     |
|                   |         | "split" inside "segment" cuts touching fields apart (s2sr/fields.py)      |                     |
| transparent_tiles | False   | the tile pyramid shows the map through the job's nodata pixels            | true                |

A callee with the reference's signature (tests patch such stand-ins in) must keep working for a job that asks for nothing: an option
crosses a seam only when it was given, and only on the seams whose callee knows it (SEAMS)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

# (the fields that travel together, when they travel)
_TRAVELS = (
    (("seam_blend",), lambda o: o.seam_blend),
    (("bit_depth",), lambda o: o.bit_depth != 8),
    (("display",), lambda o: o.display is not None),
    (("nodata", "fill_radius"), lambda o: o.nodata is not None),
    (("consistency",), lambda o: o.consistency is not None),
    (("extra_bands",), lambda o: o.extra_bands is not None),
    (("extra_weights",), lambda o: o.extra_bands is not None and o.extra_weights is not None),
    (("transparent_tiles",), lambda o: o.transparent_tiles),
    (("indices", "index_offset", "zones"), lambda o: o.indices is not None),
)
_FLAGS = ("seam_blend", "transparent_tiles")          # passed as True, whatever truthy value the caller gave

_OPERATOR = ("seam_blend", "consistency")
_PROCESS = ("seam_blend", "bit_depth", "display", "nodata", "fill_radius", "consistency", "extra_bands", "indices", "index_offset")
# callee -> the options it knows
SEAMS = {
    "run_wow_job": _PROCESS + ("transparent_tiles",),                         # the route's background task
    "process_wow_sr": _PROCESS,                                               # run_wow_job has no extra_weights and no zones
    "apply_wow_sr": _PROCESS + ("extra_weights", "zones"),
    "run_sr_job": _OPERATOR,
    "process_farm_sr": _OPERATOR,
    "apply_farm_sr": _OPERATOR,
    "RealESRGAN": _OPERATOR,
}


@dataclass(frozen=True, eq=False)
class JobOptions:
    seam_blend: bool = False
    bit_depth: int = 8
    display: object = None
    nodata: object = None
    fill_radius: int = 32
    consistency: Optional[str] = None
    extra_bands: object = None
    extra_weights: object = None
    indices: object = None
    index_offset: int = 0
    zones: object = None
    transparent_tiles: bool = False

    @classmethod
    def from_request(cls, request) -> "JobOptions":
        """The options of an app.sr_routes.WowRequest (it has no extra_weights and no zones) or SRRequest."""
        return cls(**{name: getattr(request, name) for name in cls.__dataclass_fields__ if hasattr(request, name)})

    def passed(self, seam: str) -> dict:
        """The keywords the call of `seam` (a key of SEAMS) gets beyond the reference's arguments: {} for a job that asks for nothing."""
        knows = SEAMS[seam]
        kw = {name: True if name in _FLAGS else getattr(self, name)
              for names, travels in _TRAVELS if travels(self) for name in names if name in knows}
        if seam == "apply_wow_sr" and self.bit_depth != 16:
            kw.pop("display", None)      # (display belongs to the 16-bit call; `check` has refused the pair before this seam)
        return kw

    def check_option(self, name: str, band_count: Optional[int] = None) -> None:
        """The refusals of one option that no other option has a say in, as ValueError (a bad stretch may be a TypeError).
        band_count: the input file's, when it is at hand -- extra_bands and indices are then checked against it."""
        if name == "nodata":
            from s2sr.nodata import check_args
            check_args(self.nodata, self.fill_radius)
        elif name == "consistency":
            from s2sr.consistency import check_args
            check_args(self.consistency)
        elif name == "display":
            from s2sr.display import Stretch
            Stretch.of(self.display)
        elif name == "extra_bands":      # without the file: the form, numbers below 4, repeats
            from s2sr import bands as xb
            xb.select_bands(self.extra_bands, band_count)
            xb.check_args(4, 0, 65535, xb.WEIGHTS if self.extra_weights is None else self.extra_weights)
        elif name == "indices":          # without the file: presets, names, bands, K, L, offsets
            from s2sr.index import resolve
            resolve(self.indices, self.index_offset, band_count)
        else:
            raise KeyError(name)

    def check(self, enhance_crops: bool, band_count: Optional[int] = None) -> None:
        """Every refusal of a job's options, before anything is created."""
        self.check_option("nodata")
        self.check_option("consistency")
        if self.nodata is not None and self.nodata != "tag" and not 0 <= int(self.nodata) <= 65535:
            # (compared with the bands as stored: an 8-bit job of a uint16 raster names the uint16 value)
            raise ValueError(f"nodata {self.nodata!r}: an integer in 0..65535")
        if self.bit_depth not in (8, 16):
            raise ValueError(f"bit_depth {self.bit_depth!r}: 8 or 16")
        if self.extra_bands is not None:
            if self.bit_depth != 16:
                raise ValueError("extra_bands are carried on the 16-bit path: pass bit_depth=16 (an 8-bit job has no uint16 image to guide them)")
            self.check_option("extra_bands", band_count)
        elif self.extra_weights is not None:
            raise ValueError("extra_weights are the guide weights of extra_bands: pass extra_bands")
        if self.indices is not None:
            if self.bit_depth != 16:
                raise ValueError("indices are computed on the 16-bit path: pass bit_depth=16 (an 8-bit job has no uint16 product to take them from)")
            self.check_option("indices", band_count)
            from s2sr import fields as xf
            from s2sr import mzones as xm
            zones = self.zones
            if xm.is_manage(zones):            # management zones: its own refusals, then `fields` as the value it is
                from s2sr.index import resolve
                xm.check_index(xm.check_option(zones), resolve(self.indices, self.index_offset, band_count))
                zones = zones["fields"]
            if xf.is_segment(zones):           # (that its index is among the job's: s2sr.fields.resolve, with the definitions at hand)
                from s2sr.index import resolve
                xf.check_index(xf.check_option(zones), resolve(self.indices, self.index_offset, band_count))
        elif self.zones is not None or self.index_offset != 0:
            raise ValueError("zones and index_offset belong to indices: pass indices")
        if self.display is not None:
            if self.bit_depth != 16:
                raise ValueError("display is the 8-bit rendering of a 16-bit job: pass bit_depth=16 (an 8-bit job's image is its display image)")
            self.check_option("display")
        elif self.bit_depth == 16 and enhance_crops:
            raise ValueError("bit_depth=16 has no crop-visibility post-process (it is OpenCV's 8-bit arithmetic by definition): pass enhance_crops=False, "
                             "or display=... to run it on the display image")
