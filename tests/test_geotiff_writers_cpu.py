"""The GeoTIFF writers of s2sr/rasterio_lite.py, one strip writer under four doors, held to the bytes the three separate writers
wrote: SHA-256 of every file in tests/golden/geotiff_writer_digests.txt, recorded from the last commit with the three copies.

    python tests/test_geotiff_writers_cpu.py > tests/golden/geotiff_writer_digests.txt

records the table through the public writers, so it runs on any commit."""
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden" / "geotiff_writer_digests.txt"
H, W, ROWS = 70, 33, 64                        # two strips, the last one ragged
NODATA = (None, 0, -32768, 0.5)


def _georef():
    from s2sr import rasterio_lite as rio
    return rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0),
                       rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 500000.0, 4000000.0, 0.0),
                       rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32636),
                       rio.TAG_GEOASCII: "WGS 84 / UTM zone 36N|"})


def _cases():
    """name -> (writer name, array)"""
    rng = np.random.default_rng(20344)
    u8 = lambda c: rng.integers(0, 256, size=(H, W, c), dtype=np.uint8)                       # noqa: E731
    u16 = lambda c: rng.integers(0, 65536, size=(H, W, c)).astype(np.uint16)                  # noqa: E731
    return {
        "rgb-u8x3": ("write_geotiff_rgb", u8(3)),
        "rgb-u8x4-alpha-dropped": ("write_geotiff_rgb", u8(4)),
        "rgb-u8x3-zeros": ("write_geotiff_rgb", np.zeros((H, W, 3), np.uint8)),
        "rgb16-u16x3": ("write_geotiff_rgb16", u16(3)),
        "rgb16-u16x3-zeros": ("write_geotiff_rgb16", np.zeros((H, W, 3), np.uint16)),
        "u16-x3": ("write_geotiff_u16", u16(3)),
        "u16-x1": ("write_geotiff_u16", u16(1)),
        "u16-x2": ("write_geotiff_u16", u16(2)),
        "u16-x5": ("write_geotiff_u16", u16(5)),
        "u16-x5-zeros": ("write_geotiff_u16", np.zeros((H, W, 5), np.uint16)),
        "i16-2d": ("write_geotiff_i16", rng.integers(-32768, 32768, size=(H, W)).astype(np.int16)),
        "i16-2d-zeros": ("write_geotiff_i16", np.zeros((H, W), np.int16)),
    }


def _digests(tmp: Path):
    from s2sr import rasterio_lite as rio
    out = {}
    for name, (writer, a) in _cases().items():
        for nodata in NODATA:
            p = tmp / f"{name}.tif"
            getattr(rio, writer)(p, a, _georef(), rows_per_strip=ROWS, nodata=nodata)
            out[f"{name} nodata={nodata}"] = hashlib.sha256(p.read_bytes()).hexdigest()
    return out


def test_every_writer_writes_the_recorded_bytes(tmp_path):
    want = dict(line.rsplit(" ", 1) for line in GOLDEN.read_text().splitlines() if line and not line.startswith("#"))
    got = _digests(tmp_path)
    assert set(got) == set(want) and len(got) == 12 * 4
    assert [k for k in got if got[k] != want[k]] == []
    assert len(set(got.values())) == len(got)               # (no two cases are the same file: every case and every tag counts)


def test_u16_with_three_bands_is_rgb16(tmp_path):
    from s2sr import rasterio_lite as rio
    a = _cases()["rgb16-u16x3"][1]
    for nodata in NODATA:
        rio.write_geotiff_rgb16(tmp_path / "a.tif", a, _georef(), rows_per_strip=ROWS, nodata=nodata)
        rio.write_geotiff_u16(tmp_path / "b.tif", a, _georef(), rows_per_strip=ROWS, nodata=nodata)
        assert (tmp_path / "a.tif").read_bytes() == (tmp_path / "b.tif").read_bytes()
    back, geo = rio.read_bands_raw(tmp_path / "b.tif")
    assert np.array_equal(back, a) and geo.nodata == 0.5


@pytest.mark.parametrize("name", ["rgb-u8x3", "rgb16-u16x3", "u16-x5", "i16-2d"])
def test_a_failing_strip_leaves_no_file_behind(tmp_path, monkeypatch, name):
    import threading

    from s2sr import native, rasterio_lite as rio
    writer, a = _cases()[name]
    real, calls, lock = native.tiff_lzw_encode, [], threading.Lock()

    class Boom(Exception):
        pass

    def second_strip_fails(data):
        with lock:
            calls.append(len(data))
            n = len(calls)
        if n == 2:
            raise Boom("strip 2")
        return real(data)
    monkeypatch.setattr(native, "tiff_lzw_encode", second_strip_fails)
    p = tmp_path / "out.tif"
    with pytest.raises(Boom, match="strip 2"):
        getattr(rio, writer)(p, a, _georef(), rows_per_strip=ROWS)
    assert len(calls) == 2 and not p.exists() and list(tmp_path.iterdir()) == []


if __name__ == "__main__":
    import tempfile
    for p in (str(REPO / "sentinel2-super-resolution-poc_amd"), str(REPO)):
        if p not in sys.path:
            sys.path.insert(0, p)
    print("# SHA-256 of the files the GeoTIFF writers write for tests/test_geotiff_writers_cpu.py's seeded arrays (70 x 33, 64 rows per")
    print("# strip), recorded from commit 20344e9 (the last with three separate writers) by `python tests/test_geotiff_writers_cpu.py`.")
    print("# <case> nodata=<value> <sha256>")
    with tempfile.TemporaryDirectory() as d:
        for k, v in _digests(Path(d)).items():
            print(k, v)
