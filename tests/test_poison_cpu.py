"""The poison mode's host logic (csrc/redzone.h namespace poison: the two patterns, the chunked fill, the read-back) without a
GPU: the device is reached through two callbacks, which tests/native/poison_main.cpp points at exact-size heap blocks.  The GPU
side is tests/test_gpu_poison.py."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from s2sr import native

REPO = Path(__file__).resolve().parent.parent


def test_poison_fill_under_address_and_ub_sanitizers(tmp_path):
    """Both patterns at every size around the chunk boundaries, on exact-size blocks and inside a guarded frame; the first wrong
    byte is the one reported; the mode off writes nothing; a failing write is reported; a fill between red zones leaves them
    whole -- under ASan / UBSan, so a fill or read-back that leaves the caller's bytes is itself reported."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "poison"
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", str(REPO / "sentinel2-super-resolution-poc_amd" / "csrc"),
                        str(REPO / "tests" / "native" / "poison_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


def test_pattern_must_be_0_1_or_2():
    """s2sr_debug_poison is host arithmetic until the next allocation.  Ends with the pattern it found (S2SR_POISON may have set one)."""
    lib = native.load_library()
    before = native.poison_pattern()
    try:
        for bad in (-1, 3, 255):
            assert lib.s2sr_debug_poison(bad) == -1, bad
            with pytest.raises(native.S2srError):
                native.poison(bad)
            assert native.poison_pattern() == before
        for good in (1, 2, 0):
            assert lib.s2sr_debug_poison(good) == 0 and native.poison_pattern() == good
    finally:
        native.poison(before)


def test_the_python_pattern_is_the_library_header_s():
    """native.poison_byte restates poison::byte_at for the GPU controls: never zero, 0xFF for pattern 1, and for pattern 2 the
    red zones' front pattern with its period of 65536."""
    i = np.arange(3 * 65536)
    assert (native.poison_byte(1, i) == 0xFF).all()
    p = native.poison_byte(2, i)
    want = ((i * 167 + (i >> 8) * 13 + 0x5B) & 0xFF) | 1
    assert p.dtype == np.uint8 and (p == want).all() and (p != 0).all() and np.array_equal(p[:65536], p[65536:2 * 65536])
    assert len(np.unique(p)) > 64
