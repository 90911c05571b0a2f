"""The scratch slots' book-keeping (csrc/scratch.h: capacity per slot, the one record of what the last call kept, the taken-input
guard, the void rule) without a GPU: memory is reached through two callbacks, which tests/native/scratch_main.cpp points at
exact-size heap blocks.  The GPU side is tests/test_gpu_kept.py and the three door matrices."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent


def test_scratch_book_under_address_and_ub_sanitizers(tmp_path):
    """A request within capacity moves nothing, a larger one frees the old block once; any request voids the kept record and only
    the run's slot closes a banded run; take refuses a wrong kind or size and leaves the record; keep restores it behind the
    call's own requests; a taken slot is not regrown; the all-slots void -- under ASan / UBSan, so a double free, a leak or a
    use after release is itself reported."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "scratch"
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", str(REPO / "sentinel2-super-resolution-poc_amd" / "csrc"),
                        str(REPO / "tests" / "native" / "scratch_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
