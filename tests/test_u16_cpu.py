"""The 16-bit door, the parts that need no GPU: the channel split the packer rests on, the uint16 GeoTIFF writer / raw reader,
and the argument checks of bit_depth=16."""
import numpy as np
import pytest

from s2sr import rasterio_lite as rio
from s2sr import tiff_lite
from tiff_fixture import write_tiff

GEO = {rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0),
       rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 500000.0, 4000000.0, 0.0),
       rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32636)}


@pytest.mark.parametrize("lo,hi", [(0, 65535), (0, 255), (1000, 11000), (65534, 65535), (0, 1), (137, 40000)])
def test_channel_split_is_exact_in_fp16(lo, hi):
    """d = clamp(v, lo, hi) - lo = 256 dh + dl: dl (0..255) and 256 dh (0..65280) are fp16 numbers, and their sum -- what
    conv_first's fp32 accumulator sees through the doubled weight set -- is d.  All 65536 input values."""
    v = np.arange(65536, dtype=np.int64)
    d = np.clip(v, lo, hi) - lo
    dl, dh256 = d & 0xFF, d & 0xFF00
    assert dl.max() <= 255 and dh256.max() <= 65280 < 65504          # fp16's largest finite value
    h_l, h_h = dl.astype(np.float16), dh256.astype(np.float16)
    assert np.isfinite(h_l).all() and np.isfinite(h_h).all()
    assert np.array_equal(h_l.astype(np.int64), dl) and np.array_equal(h_h.astype(np.int64), dh256)
    assert np.array_equal((h_l.astype(np.float32) + h_h.astype(np.float32)).astype(np.int64), d)
    assert d.min() == 0 and d.max() == hi - lo
    if hi - lo < 256:          # the case the bit-identity with the u8 door rests on: the high channels are exact zeros
        assert not dh256.any()


@pytest.mark.parametrize("H,W,rps", [(33, 47, 64), (130, 61, 64), (5, 3, 64), (64, 64, 64), (65, 7, 16), (1, 1, 64)])
def test_write_geotiff_rgb16_roundtrip(tmp_path, H, W, rps):
    """Odd sizes, fewer rows than one strip, exactly one strip, several strips with a short last one."""
    rng = np.random.default_rng(H * 1000 + W)
    rgb = rng.integers(0, 65536, (H, W, 3), dtype=np.uint16)
    rgb[0, 0] = (0, 65535, 256)
    p = tmp_path / "a16.tif"
    rio.write_geotiff_rgb16(p, rgb, rio.GeoRef(GEO), rows_per_strip=rps)
    arr, tv = tiff_lite.read_tiff(p)
    assert arr.dtype == np.uint16 and arr.shape == (H, W, 3) and np.array_equal(arr, rgb)
    assert tuple(tv[258]) == (16, 16, 16) and tuple(tv[259]) == (5,) and p.read_bytes()[:2] == b"II"
    for t, want in GEO.items():
        assert tuple(tv[t]) == tuple(want), t
    raw, g2 = rio.read_rgb_raw(p)
    assert raw.dtype == np.uint16 and np.array_equal(raw, rgb) and g2.pixel_size == (10.0, 10.0)
    assert g2.scaled(4).pixel_size == (2.5, 2.5) and g2.tags[rio.TAG_GEOKEYS] == GEO[rio.TAG_GEOKEYS]


def test_write_geotiff_rgb16_refuses_other_arrays(tmp_path):
    for bad in (np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint16), np.zeros((4, 4, 4), np.uint16), np.zeros((4, 4, 3), np.float32)):
        with pytest.raises(ValueError):
            rio.write_geotiff_rgb16(tmp_path / "bad.tif", bad, rio.GeoRef({}))
    assert not (tmp_path / "bad.tif").exists()


def test_read_rgb_raw_returns_the_stored_values(tmp_path):
    rng = np.random.default_rng(4)
    geo = [(rio.TAG_PIXEL_SCALE, 12, (10.0, 10.0, 0.0)), (rio.TAG_TIEPOINT, 12, (0.0, 0.0, 0.0, 5e5, 4e6, 0.0))]
    for B in (3, 4, 1):
        a = rng.integers(0, 65536, (21, 34, B), dtype=np.uint16)
        p = tmp_path / f"b{B}.tif"
        write_tiff(p, a, extra=geo)
        raw, g = rio.read_rgb_raw(p)
        assert raw.dtype == np.uint16 and raw.shape == (21, 34, 3) and raw.flags["C_CONTIGUOUS"]
        want = a[..., :3] if B >= 3 else np.repeat(a, 3, axis=2)
        assert np.array_equal(raw, want) and g.pixel_size == (10.0, 10.0)
        # the 8-bit reader squeezes the same file (values above 255): the raw one must not
        u8, _ = rio.read_rgb_u8(p)
        assert u8.dtype == np.uint8
    with pytest.raises(ValueError):
        rio.read_rgb_raw(tmp_path / "nothing.png")
    (tmp_path / "junk.tif").write_bytes(b"II*\0junk")
    with pytest.raises(ValueError):
        rio.read_rgb_raw(tmp_path / "junk.tif")


def test_bit_depth_argument_checks_need_no_device(tmp_path):
    from app.wow_sr import apply_wow_sr, process_wow_sr
    rgb16 = np.random.default_rng(5).integers(100, 4000, (12, 16, 3)).astype(np.uint16)
    src16 = tmp_path / "s16.tif"
    rio.write_geotiff_rgb16(src16, rgb16, rio.GeoRef(GEO))
    src8 = tmp_path / "s8.tif"
    rio.write_geotiff_rgb(src8, (rgb16 >> 4).astype(np.uint8), rio.GeoRef(GEO))
    # the post-process is 8-bit arithmetic: refused before anything is read or created
    with pytest.raises(ValueError, match="enhance_crops"):
        process_wow_sr(src16, tmp_path / "o1", enhance_crops=True, bit_depth=16)
    with pytest.raises(ValueError, match="enhance_crops"):
        apply_wow_sr(src16, tmp_path / "o1" / "x.tif", bit_depth=16)
    assert not (tmp_path / "o1").exists()
    # a non-uint16 input
    with pytest.raises(ValueError, match="uint16"):
        process_wow_sr(src8, tmp_path / "o2", enhance_crops=False, bit_depth=16)
    png = tmp_path / "s.png"
    rio.write_png(png, (rgb16 >> 4).astype(np.uint8))
    with pytest.raises(ValueError, match="uint16"):
        process_wow_sr(png, tmp_path / "o3", enhance_crops=False, bit_depth=16)
    with pytest.raises(ValueError, match="bit_depth"):
        process_wow_sr(src16, tmp_path / "o4", enhance_crops=False, bit_depth=12)
