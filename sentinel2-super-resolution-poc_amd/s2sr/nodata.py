"""Host-side helpers of the nodata-aware enhance: the mask of a raster whose invalid pixels carry a nodata value,
the mask of the enhanced image, and the value range of a 16-bit raster over its valid pixels.  The device work -- the fill in front
of the net, the mask behind everything -- is in csrc/nodata.hip, behind native.Engine.enhance_masked_*."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

DEFAULT_FILL_RADIUS = 32        # policy: what it does to edge ringing with real checkpoints is unmeasured


def mask_from_value(img: np.ndarray, nodata) -> np.ndarray:
    """uint8 [H, W], 1 = valid: a pixel of HxWx3 `img` is invalid iff all three bands equal `nodata`."""
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"expected HxWx3 image, got shape {img.shape}")
    return (~(img == nodata).all(axis=2)).astype(np.uint8)


def upsample_mask(valid: np.ndarray, scale: int) -> np.ndarray:
    """uint8 [scale H, scale W]: output pixel (Y, X) is valid iff input pixel (Y // scale, X // scale) is."""
    valid = np.asarray(valid)
    if valid.ndim != 2 or int(scale) < 1:
        raise ValueError(f"expected an [H, W] mask and a positive scale, got shape {valid.shape}, scale {scale}")
    v = (valid != 0).astype(np.uint8)
    return np.repeat(np.repeat(v, int(scale), axis=0), int(scale), axis=1)


def valid_range(img16: np.ndarray, valid: Optional[np.ndarray]) -> Tuple[int, int]:
    """(lo, hi) = the min and max of `img16` over its valid pixels (valid None: all), made a range the 16-bit door takes
    (lo < hi): a constant raster gets (v - 1, v), or (0, 1) for v == 0; a raster without a valid pixel (0, 1)."""
    img16 = np.asarray(img16)
    px = img16 if valid is None else img16[np.asarray(valid) != 0]
    if px.size == 0:
        return 0, 1
    lo, hi = int(px.min()), int(px.max())
    if hi == lo:                      # a constant raster: any range that contains it
        lo, hi = (lo - 1, hi) if hi > 0 else (0, 1)
    return lo, hi


def check_args(nodata, fill_radius, what: str = "nodata") -> None:
    """The refusals every layer above the engine shares (before anything is created): nodata None, an integer or "tag";
    fill_radius an integer in 1..64."""
    if nodata is not None and nodata != "tag" and (isinstance(nodata, bool) or not isinstance(nodata, (int, np.integer))):
        raise ValueError(f"{what} {nodata!r}: None, an integer or \"tag\" (the file's GDAL_NODATA tag)")
    if isinstance(fill_radius, bool) or not isinstance(fill_radius, (int, np.integer)) or not 1 <= int(fill_radius) <= 64:
        raise ValueError(f"fill_radius {fill_radius!r}: an integer in 1..64")
