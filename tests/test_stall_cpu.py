"""The stall mode without a GPU: every ordering event of the engine goes through the three wrappers of csrc/engine_internal.h,
every site they name is in use, the droppable sites of the header are the ones the entry accepts, and the entries refuse what
they should before they touch a device."""
import re
from pathlib import Path

import pytest

from s2sr import native

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "sentinel2-super-resolution-poc_amd" / "csrc"
RAW = ("hipStreamWaitEvent(", "hipEventRecord(", "hipEventSynchronize(")
# where the raw calls may stand: the wrappers themselves, and the timing events, which order nothing
ALLOWED = {
    "engine_internal.h": {"ev_record", "ev_stream_wait", "ev_host_wait", "Scope"},
    "engine.hip": {"span_begin", "span_end"},
    "engine_debug.hip": {"s2sr_debug_mfma_ceiling", "s2sr_debug_bench_conv", "s2sr_debug_rdb_persistent"},
}
def _sources():
    return sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.h")))


def _code(line):
    """the line without its // comment and without string literals"""
    line = re.sub(r'"(?:[^"\\]|\\.)*"', '""', line)
    return line.split("//")[0]


def _enclosing(lines, i):
    """the function or struct whose body holds line i: the nearest line above that starts a definition in column 0"""
    for j in range(i, -1, -1):
        line = _code(lines[j])
        if not re.match(r"[A-Za-z_]", line) or re.match(r"(namespace|using|extern|typedef|template)\b", line):
            continue
        m = re.match(r"struct\s+(\w+)", line) or re.search(r"(\w+)\s*\(", line)
        if m:
            return m.group(1)
    return None


def test_ordering_events_go_through_the_wrappers():
    found = {}
    for path in _sources():
        lines = path.read_text().splitlines()
        for i, line in enumerate(lines):
            if any(r in _code(line) for r in RAW):
                found.setdefault(path.name, set()).add(_enclosing(lines, i))
                assert _enclosing(lines, i) in ALLOWED.get(path.name, set()), \
                    f"{path.name}:{i + 1}: a raw event call in {_enclosing(lines, i)}(): use ev_record / ev_stream_wait / ev_host_wait (engine_internal.h)"
    # the list above is no wider than the code: every allowed function still holds a raw call (engine_debug.hip: by its e0 / e1 pairs)
    assert found == ALLOWED, found
    debug = (CSRC / "engine_debug.hip").read_text()
    for m in re.finditer(r"hipEventRecord\((\w+),", debug):
        assert m.group(1) in ("e0", "e1"), m.group(0)


def _sites():
    text = (CSRC / "engine_internal.h").read_text()
    body = text[text.index("enum Site {"):]
    body = body[:body.index("};")]
    names = re.findall(r"^\s*(SITE_[A-Z0-9_]+)", body, re.M)
    assert names and names[-1] == "SITE_COUNT"
    return names[:-1]


def test_every_site_is_used():
    sites = _sites()
    assert len(sites) == len(set(sites))
    text = "".join(p.read_text() for p in _sources())
    calls = re.findall(r"ev_(record|stream_wait|host_wait)\(h, [^;]*?(SITE_[A-Z0-9_]+)\)", text)
    used = {s for _, s in calls}
    assert used == set(sites), (sorted(set(sites) - used), sorted(used - set(sites)))
    # a site that is waited for is recorded somewhere
    for s in used:
        assert ("record", s) in calls and (("stream_wait", s) in calls or ("host_wait", s) in calls), s


def test_droppable_sites_of_the_headers_are_the_ones_the_entry_accepts():
    sites = _sites()
    text = (CSRC / "engine_internal.h").read_text()
    listed = re.search(r"kDroppableSites\[\] = \{([^}]*)\}", text).group(1).replace(" ", "").split(",")
    header = (REPO / "include" / "s2sr.h").read_text()
    public = {name: int(v) for name, v in re.findall(r"#define S2SR_(SITE_[A-Z0-9_]+) (\d+)", header)}
    assert set(public) == set(listed)
    assert all(sites.index(n) == v for n, v in public.items())
    assert sorted(public.values()) == sorted(native.DROPPABLE_SITES)
    assert (native.SITE_BATCH_GROUP_D2H, native.SITE_CHUNK_BAND_D2H, native.SITE_DISPLAY_BAND_D2H, native.SITE_COPY_TO_HOST) == tuple(
        public[n] for n in ("SITE_BATCH_GROUP_D2H", "SITE_CHUNK_BAND_D2H", "SITE_DISPLAY_BAND_D2H", "SITE_COPY_TO_HOST"))
    # the header says, site by site, why each droppable one cannot send a load or store anywhere
    why = text[text.index("The negative control (s2sr_debug_delay_drop)"):text.index("inline constexpr int kDroppableSites")]
    for n in listed:
        assert re.search(rf"//\s+{n}\s+\S", why), n
    before = native.delay_dropped()
    try:
        accepted = []
        for site in range(-4, len(sites) + 4):
            try:
                native.delay_drop(site)
                accepted.append(site)
            except native.S2srError:
                pass
        assert accepted == sorted([-1] + list(public.values()))
    finally:
        native.delay_drop(before)


def test_the_mode_is_off_by_default_and_refuses_bad_arguments():
    assert native.delay_mode() == (0, 0) and native.delay_dropped() == -1
    header = (REPO / "include" / "s2sr.h").read_text()
    assert int(re.search(r"#define S2SR_DEBUG_STALL_MAX_USEC (\d+)", header).group(1)) == native.STALL_MAX_USEC == 20000
    for mode, usec in ((1, 0), (2, 0), (4, 100), (-1, 100), (1, native.STALL_MAX_USEC + 1), (3, -1), (0, 5)):
        if (mode, usec) == (0, 5):
            native.delay(mode, usec)                                     # off with a length on record is still off
            assert native.delay_mode()[0] == 0
            native.delay(0)
            continue
        with pytest.raises(native.S2srError):
            native.delay(mode, usec)
    assert native.delay_mode() == (0, 0)
    lib = native.load_library()
    assert lib.s2sr_debug_stall(None, 0, None, 100) != 0 and lib.s2sr_debug_stream_touch(None, 0, None, 1) != 0   # no handle: refused


def test_the_stall_kernel_is_plain_cxx_with_a_hard_cap():
    """one wave, the constant-rate counter, a sleep between reads, an iteration cap, no memory and no inline assembly"""
    src = (CSRC / "stall.hip").read_text()
    kernel = src[src.index("__global__ void"):]
    kernel = kernel[:kernel.index("\n}\n")]
    assert "wall_clock64()" in kernel and "__builtin_amdgcn_s_sleep(" in kernel and "i < cap" in kernel
    assert "asm" not in src.replace("assembl", "") and "*" not in "".join(_code(l) for l in kernel.split("{", 1)[1].splitlines())    # no pointer is read or written
    assert "stall_kernel<<<dim3(1), dim3(64)" in src
