"""The red-zone mode's host logic (csrc/redzone.h: registry of zoned allocations, the zone pattern, check / re-fill / sticky
record) without a GPU: the device is reached through two callbacks, which tests/native/redzone_main.cpp points at exact-size heap
blocks.  The GPU side is tests/test_gpu_redzones.py."""
import shutil
import subprocess
from pathlib import Path

import pytest

from s2sr import native

REPO = Path(__file__).resolve().parent.parent


def test_redzone_registry_under_address_and_ub_sanitizers(tmp_path):
    """Register, check and free in every order; damage at the first and last byte of each zone, zeros and shifted copies;
    re-fill after a report; the sticky record after a free; a pointer that was never registered; Z = 0; workspace planes --
    under ASan / UBSan, so a fill or read-back that leaves a zone is itself reported."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "redzone"
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", str(REPO / "sentinel2-super-resolution-poc_amd" / "csrc"),
                        str(REPO / "tests" / "native" / "redzone_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


def test_zone_size_must_be_a_multiple_of_4096():
    """s2sr_debug_redzone is host arithmetic until the next allocation: 0 and multiples of 4096 are taken, everything else is
    refused (a pointer handed out must keep hipMalloc's alignment).  Ends with the zone size it found (S2SR_REDZONE may have set one)."""
    lib = native.load_library()
    before = native.redzone_bytes()
    try:
        for bad in (1, 4095, 4097, 65536 + 256, -4096):
            assert lib.s2sr_debug_redzone(bad) == -1, bad
            with pytest.raises(native.S2srError):
                native.redzone(bad)
            assert native.redzone_bytes() == before
        for good in (4096, 65536, 0):
            assert lib.s2sr_debug_redzone(good) == 0 and native.redzone_bytes() == good
    finally:
        native.redzone(before)
