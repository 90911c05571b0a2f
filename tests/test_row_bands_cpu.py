"""The row bands of the raster passes (csrc/row_bands.h: band_of and the row_bands iterable every banded loop and copy_rows walk)
without a GPU: tests/native/row_bands_main.cpp does the arithmetic under ASan / UBSan.  The GPU side is the band-row independence
tests of the pass modules and the four door matrices."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent


def test_row_bands_under_address_and_ub_sanitizers(tmp_path):
    """For every H in 1..70 and rows in 1..H + 2 the bands are ordered, disjoint and cover exactly [0, H), all but the last have
    `rows` rows, there are ceil(H / rows) of them and `last` is set on the final one alone; H = 0x7fffffff in bands of 0x40000000
    rows (ceil gives two; 0x3fffffff rows give three) where an int sum would wrap; band_of: a positive band_rows wins and is
    clamped to H, otherwise budget / row_bytes clamped to [1, H], a row above the budget gives 1."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "row_bands"
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", str(REPO / "sentinel2-super-resolution-poc_amd" / "csrc"),
                        str(REPO / "tests" / "native" / "row_bands_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
