"""The grid cap without a GPU: the setter, the getter and the counter are host arithmetic; the header, the library and native.py
state the same constants; and every .hip file whose kernels stride over gridDim.x computes its launch grids through the helper
of csrc/s2sr_internal.h, the documented exceptions listed here with one reason each."""
import ctypes as C
import re
from pathlib import Path

import pytest

from s2sr import native

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "sentinel2-super-resolution-poc_amd" / "csrc"
HEADER = (REPO / "include" / "s2sr.h").read_text()

# .hip files whose kernels hold `+= gridDim.x` or `+= (size_t)gridDim.x` and whose launches are NOT capped: one reason each
EXCEPTIONS = {
    "ceiling.hip": "a measuring instrument: its fill kernel is launched at a fixed grid and its result is a rate, not bytes a door returns",
}
# files with no such stride that must stay away from the helper: a workgroup is the work item, or workgroups wait for each other
NEVER_CAPPED = {
    "pngdev.hip": "one workgroup per tile: blockIdx.x is the tile",
    "persist.hip": "its workgroups hand planes to each other through flags: all must be resident",
    "stall.hip": "one wave that lets time pass",
    "ceiling.hip": EXCEPTIONS["ceiling.hip"],
}
HELPERS = ("capped_grid(", "stride_grid(", "persistent_grid(")


def _code(text):
    """the source without its // comments and string literals"""
    out = []
    for line in text.splitlines():
        line = re.sub(r'"(?:[^"\\]|\\.)*"', '""', line)
        out.append(line.split("//")[0])
    return "\n".join(out)


def test_abi_of_the_setter_the_getter_and_the_counter():
    lib = native.load_library()
    assert int(re.search(r"#define S2SR_DEBUG_GRID_CAP_MAX (\d+)", HEADER).group(1)) == native.GRID_CAP_MAX == 1048576
    assert int(re.search(r"#define S2SR_GRID_CAP_FAMILIES (\d+)", HEADER).group(1)) == native.GRID_CAP_FAMILIES
    for name in ("s2sr_debug_grid_cap", "s2sr_debug_grid_cap_workgroups", "s2sr_debug_grid_cap_stats", "s2sr_debug_grid_cap_stats_reset",
                 "s2sr_debug_grid_cap_family"):
        assert name in native.EXPORTED_SYMBOLS and re.search(rf"\b{name}\(", HEADER), name
    before = native.grid_cap_workgroups()
    try:
        for good in (0, 1, 3, 8, 16, native.GRID_CAP_MAX, 0):
            assert lib.s2sr_debug_grid_cap(good) == 0 and native.grid_cap_workgroups() == good
        native.grid_cap(5)
        for bad in (-1, -8, native.GRID_CAP_MAX + 1, 2 ** 31 - 1, -2 ** 31):
            assert lib.s2sr_debug_grid_cap(bad) == -1, bad
            with pytest.raises(native.S2srError):
                native.grid_cap(bad)
            assert native.grid_cap_workgroups() == 5, "a refused value moved the cap"
    finally:
        native.grid_cap(before)
    # the families: named, distinct, NULL past the last; the counter is at zero in a process that launched nothing
    fams = native.grid_cap_families()
    assert len(fams) == len(set(fams)) == native.GRID_CAP_FAMILIES and lib.s2sr_debug_grid_cap_family(len(fams)) is None
    assert lib.s2sr_debug_grid_cap_family(-1) is None
    assert {"conv", "trunk_f16", "trunk_f8", "pack", "tiles", "resample", "display", "nodata", "consistency", "bands", "postprocess"} == set(fams)
    native.grid_cap_stats(reset=True)
    assert all(v == (0, 0) for v in native.grid_cap_stats().values())
    a, n = (C.c_int64 * native.GRID_CAP_FAMILIES)(), C.c_int32(0)
    assert lib.s2sr_debug_grid_cap_stats(a, a, native.GRID_CAP_FAMILIES - 1, C.byref(n)) != 0      # too little room: refused
    assert lib.s2sr_debug_grid_cap_stats(None, a, native.GRID_CAP_FAMILIES, C.byref(n)) != 0


def test_the_families_of_the_library_are_the_enum_of_the_internal_header():
    text = (CSRC / "s2sr_internal.h").read_text()
    enum = re.search(r"enum GridFam : int \{([^}]*)\}", text).group(1)
    names = [n.strip() for n in enum.split(",") if n.strip()]
    assert names[-1] == "GF_COUNT" and len(names) - 1 == native.GRID_CAP_FAMILIES
    listed = re.search(r"kGridFamName\[GF_COUNT\] = \{([^}]*)\}", text).group(1)
    assert tuple(re.findall(r'"(\w+)"', listed)) == native.grid_cap_families()
    assert [n[3:].lower() for n in names[:-1]] == list(native.grid_cap_families())


def _strided_files():
    out = {}
    for path in sorted(CSRC.glob("*.hip")):
        code = _code(path.read_text())
        if re.search(r"\+=\s*(\(size_t\)\s*)?gridDim\.x", code) or re.search(r"=\s*gridDim\.x\s*;", code):
            out[path.name] = code
    return out


def test_every_kernel_that_strides_over_its_grid_is_launched_through_the_helper():
    """`i += gridDim.x ...`, `t += gridDim.x`, and the conv kernels' `nwg = gridDim.x` (their patch loop strides by nwg)"""
    files = _strided_files()
    assert {"pack.hip", "tiles.hip", "resample.hip", "display.hip", "nodata.hip", "consistency.hip", "bands.hip", "postprocess.hip",
            "conv3x3.hip", "conv_trunk.hip"} <= set(files), sorted(files)
    for name, code in files.items():
        if name in EXCEPTIONS or name in NEVER_CAPPED:
            continue
        assert any(h in code for h in HELPERS), f"{name}: a kernel strides over gridDim.x and no launch grid goes through {HELPERS}"
        # every launch of a kernel that strides over its grid stands in a function that takes the grid from the helper
        launches = 0
        for m in re.finditer(r"hipLaunchKernelGGL\(\(?([\w:]+)", code):
            kernel = m.group(1)
            if kernel == "kern":                                  # the conv launchers: the instantiation is chosen above the launch
                strided = True
            else:
                at = re.search(rf"__global__[^;{{]*?\b{kernel}\(", code)
                assert at, f"{name}: the kernel {kernel} of a launch was not found"
                body = code[at.start():]
                strided = "gridDim.x" in body[:body.index("\n}\n")]
            if not strided:
                continue
            launches += 1
            fn = code[code.rfind("\n}\n", 0, m.start()) + 1:code.index(";", m.end())]      # the function so far, and the launch statement
            assert any(h in fn for h in HELPERS + ("grid_for(", "tile_grid(")), f"{name}: {kernel} strides over its grid; its launch does not go through the helper"
        assert launches, name
    for name in EXCEPTIONS:
        assert name in files, f"{name} no longer strides over gridDim.x: take it off the list"


def test_the_uncapped_files_stay_away_from_the_helper():
    for name, why in NEVER_CAPPED.items():
        code = _code((CSRC / name).read_text())
        assert not any(h in code for h in HELPERS), f"{name} must not be capped ({why})"
    # the one file that both caps and must not: the CLAHE histogram / LUT and the blur launches take tile counts, not the helper
    pp = _code((CSRC / "postprocess.hip").read_text())
    for kernel in ("clahe_hist_kernel", "clahe_lut_kernel", "clahe_hist_rows_kernel", "sharpen_veg_kernel"):
        for m in re.finditer(rf"hipLaunchKernelGGL\({kernel}[^;]*;", pp):
            assert not any(h in m.group(0) for h in HELPERS), m.group(0)
    assert pp.count("stride_grid(") == 4                       # clahe_apply / clahe_apply4, whole batches and row bands


def test_grid_for_of_each_file_is_the_helper():
    for name, fam in (("pack.hip", "GF_PACK"), ("tiles.hip", "GF_TILES"), ("resample.hip", "GF_RESAMPLE")):
        code = _code((CSRC / name).read_text())
        m = re.search(r"inline int grid_for\([^)]*\)\s*\{([^}]*)\}", code)
        assert m and "stride_grid(" in m.group(1) and fam in m.group(1), name
    assert "S2SR_DIAG_GRID" not in (CSRC / "conv3x3.hip").read_text()          # folded into the cap


def test_the_helper_keeps_the_conv_grids_a_multiple_of_eight():
    """the arithmetic of capped_grid restated: what a cap of c gives a persistent grid, a tile grid and a histogram grid"""
    def capped(grid, cap, quantum=1):
        if not cap:
            return grid
        if quantum > 1:
            cap = max(quantum, cap & ~(quantum - 1))
        return min(grid, cap)
    text = _code((CSRC / "s2sr_internal.h").read_text())
    body = text[text.index("static inline int capped_grid("):]
    body = body[:body.index("\n}\n")]
    assert "cap & ~(quantum - 1)" in body and "if (!cap) return grid;" in body and "if (cap >= grid) return grid;" in body
    assert "memory_order_relaxed" in body
    assert re.search(r"capped_grid\(ntiles < grid \? \(ntiles \+ 7\) & ~7 : grid, ntiles, fam, 8\)", text)
    for c, want in ((1, 8), (7, 8), (8, 8), (9, 8), (15, 8), (16, 16), (23, 16), (1 << 20, 256)):
        assert capped(256, c, 8) == want
    assert capped(16, 8, 8) == 8 and capped(8, 16, 8) == 8 and capped(9, 3) == 3 and capped(2, 3) == 2 and capped(9, 0) == 9
