"""Which kernel instantiation a conv launch takes (csrc/conv_forms.h: kTrunkForms, kTailForms and the picks) without a GPU:
tests/native/conv_forms_main.cpp prints the tables and the pick of every query of a sweep, built stand-alone under the address and
undefined-behaviour sanitizers, and the picks are held to tests/forms_model.py, the plain-Python restatement of the if-ladders the
tables replaced.  The GPU side is the form record of test_gpu_trunk_insitu.py and the hook tests of test_gpu_trunk.py."""
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest

import forms_model as fm
from trunk_forms import PRODUCTION_FORMS

REPO = Path(__file__).resolve().parent.parent

# the sweep of conv_forms_main.cpp, in its nesting order
NS = (1, 2, 3, 6, 9, 16, 20, 32)
HW = (8, 16, 20, 32, 37, 53, 64, 96, 100, 192, 256, 276, 300, 320, 330, 553, 1024)
MOS = ((0, 0, 0, 0), (277, 276, 277, 276), (21, 20, 21, 20), (101, 100, 101, 100))
REST = list(itertools.product((False, True), (False, True), (1, 2), (0, 1, 2, 3), (False, True), (2, 4, 6), range(13)))   # small8, f16_full, ct, epi, fp8, nstage, hook
TAIL_REST = list(itertools.product(HW, HW, range(4), (False, True), (False, True), (False, True)))   # H, W, m, f16_full, slope, src_lo
PHASE_REST = list(itertools.product(HW, HW, range(4), (False, True)))                                # H, W, m, f16_full


@pytest.fixture(scope="module")
def native_out(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("conv_forms") / "conv_forms"
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", str(REPO / "sentinel2-super-resolution-poc_amd" / "csrc"),
                        str(REPO / "tests" / "native" / "conv_forms_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower() and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("ok\n"), (r.stdout[-500:], r.stderr[-3000:])
    out = {"T": {}, "R": {}, "L": {}, "G": {}, "C": {}, "P": {}}
    for line in r.stdout.splitlines()[:-1]:
        tag, *f = line.split()
        if tag in "TRL":
            out[tag][int(f[0])] = tuple(int(v) for v in f[1:])
        else:
            out[tag][tuple(int(v) for v in f[:-1])] = f[-1]
    return out


def _trunk_key(row):
    """a kTrunkForms row (kernel, ct, rows, ring, full, pl, prod, npl, epi, hook) as the form record's key"""
    return row[:9]


def _decode(codes, rows, refusals):
    return [refusals[c] if c in refusals else rows[ord(c) - ord("A")] for c in codes]


def test_tables_have_the_instantiations_of_the_library_once_each(native_out):
    T, L = native_out["T"], native_out["L"]
    assert sorted(T) == list(range(21)) and sorted(L) == list(range(25))
    assert len({_trunk_key(r) for r in T.values()}) == 21 and len(set(L.values())) == 25
    assert sum(r[0] == 1 and r[1] == 1 for r in T.values()) == 11 and sum(r[0] == 1 and r[1] == 2 for r in T.values()) == 6
    assert sum(r[0] == 2 for r in T.values()) == 4
    # a hook number names one row per (kernel, ct, epi) class; the documented numbers (include/s2sr.h) and no others
    hooks = {}
    for r in T.values():
        if r[9]:
            assert hooks.setdefault((r[0], r[1], r[8], r[9]), r) is r
    assert {k[3] for k in hooks if k[:2] == (1, 1)} == {1, 2, 5, 6, 7, 8, 10}
    for epi in (1, 2):
        assert {k[3] for k in hooks if k[:3] == (1, 2, epi)} == {1, 5, 10}
    assert not [k for k in hooks if k[0] == 2]
    # the record a launch leaves: the row's fields, wgl 0, loe 1 on the fp16 kernel, 4 MFMA waves
    for i, r in T.items():
        assert native_out["R"][i] == r[:7] + (0, 1 if r[0] == 1 else 0, 4) + r[7:9]


def test_trunk_pick_equals_the_ladders_over_the_sweep(native_out):
    """The full cross N x H x W x mosaic x switches x (ct, epi) x precision x nstage x hook: 9,248 geometries x 2,496 queries.  The
    ladders read a geometry through six booleans (forms_model.trunk_geometry), so the model's answers are computed once per class."""
    rows = {i: _trunk_key(r) for i, r in native_out["T"].items()}
    G = native_out["G"]
    assert len(G) == len(NS) * len(HW) ** 2 * len(MOS)
    expected, reached, classes = {}, set(), set()
    for (N, H, W, m), codes in G.items():
        geo = fm.trunk_geometry(N, H, W, MOS[m])
        if geo not in expected:
            expected[geo] = [fm.trunk_ladder(geo, *rest) for rest in REST]
        got = _decode(codes, rows, {"-": fm.NOT_SUPPORTED, "!": fm.INVALID})
        if got != expected[geo]:
            k = next(i for i in range(len(REST)) if got[i] != expected[geo][i])
            pytest.fail(f"N {N} H {H} W {W} mosaic {MOS[m]} (small8, f16_full, ct, epi, fp8, nstage, hook) {REST[k]}: "
                        f"picked {got[k]}, the ladders {expected[geo][k]}")
        reached.update(g for g in got if g != fm.NOT_SUPPORTED)
        classes.add(geo)
    assert reached == set(rows.values()), "a row no query of the sweep reaches"
    # both sides of every threshold, with and without a mosaic, whole and ragged, on and off the 277 / 276 mosaic
    for k in range(6):
        assert {c[k] for c in classes} == {False, True}
    assert any(fm.NOT_SUPPORTED in e for e in expected.values())


def test_default_picks_are_the_production_forms(native_out):
    rows = {i: _trunk_key(r) for i, r in native_out["T"].items()}
    default = [k for k, rest in enumerate(REST) if rest[0] and rest[1] and rest[6] == 0]
    seen = set()
    for codes in native_out["G"].values():
        seen.update(rows[ord(codes[k]) - ord("A")] for k in default if codes[k] not in "-!")
    assert seen == PRODUCTION_FORMS
    rest = {r for r in native_out["T"].values() if _trunk_key(r) not in PRODUCTION_FORMS}
    assert rest == {(1, 1, 8, 7, 1, 1, 0, 0, 0, 8), (1, 2, 8, 5, 0, 1, 0, 0, 1, 5), (1, 2, 8, 5, 0, 1, 0, 0, 2, 5)}


# what the comments of test_gpu_trunk_insitu.SHAPES promise, for the shapes whose launch geometry the comment states:
# (N, H, W, mosaic) -> (rows, full, pl) of conv1-4 (and conv5's rows where the comment names them)
def _mosaic(kx, ky, w):
    return (1, ky * (w + 1) - 1, kx * (w + 1) - 1, (w + 1, w, w + 1, w))


SHAPE_PROMISES = {
    "tile_1x64x64": ((1, 64, 64, MOS[0]), (8, 1, 2), None),
    "mosaic_9x20x20": (_mosaic(3, 3, 20), (8, 0, 1), None),
    "r16_1x300x330": ((1, 300, 330, MOS[0]), (16, 3, 1), None),
    "f16_1x320x320": ((1, 320, 320, MOS[0]), (16, 1, 1), None),
    "full_3x256x256": ((3, 256, 256, MOS[0]), (32, 1, 1), 16),
    "r32_2x300x330": ((2, 300, 330, MOS[0]), (32, 3, 1), None),
    "m32_20x100x100": (_mosaic(5, 4, 100), (32, 0, 1), None),
}


@pytest.mark.parametrize("shape", sorted(SHAPE_PROMISES))
def test_insitu_shape_comments_hold(native_out, shape):
    (N, H, W, mos), (rows, full, pl), conv5_rows = SHAPE_PROMISES[shape]
    if shape == "m32_20x100x100":
        assert ((W + 31) // 32) * ((H + 31) // 32) * N == 208       # "n32 208"
    if mos in MOS and H in HW and W in HW and N in NS:              # a geometry of the native sweep: the native pick itself
        T = native_out["T"]
        codes = native_out["G"][(N, H, W, MOS.index(mos))]
        pick = lambda ct, epi: T[ord(codes[REST.index((True, True, ct, epi, False, 4, 0))]) - ord("A")]   # noqa: E731
    else:                                                            # the model the sweep holds the native pick to
        pick = lambda ct, epi: fm.trunk_pick(N, H, W, mos, True, True, ct, epi, False, 4, 0)             # noqa: E731
    r = pick(1, fm.EPI_LRELU)
    assert (r[0], r[2], r[4], r[5]) == (1, rows, full, pl)
    if conv5_rows:
        assert pick(2, fm.EPI_RDB5)[2] == conv5_rows and pick(2, fm.EPI_RDB5_RRDB)[2] == conv5_rows


def test_tail_and_phase_picks_equal_the_ladders(native_out):
    # a kTailForms row (form, ct, epi, up, waves, np, ring, hpo, occ, f8, ph, full) as launch_t's argument list
    rows = {i: (r[1], r[2], bool(r[3]), r[4], r[5], r[6], r[7], r[8], bool(r[9]), r[10], bool(r[11])) for i, r in native_out["L"].items()}
    refusals = {"-": fm.NOT_SUPPORTED, "!": fm.INVALID}
    reached = set()
    assert sorted(f for (f,) in native_out["C"]) == list(range(-1, 18))
    for (form,), codes in native_out["C"].items():
        got = _decode(codes, rows, refusals)
        want = [fm.tail_pick(form, H, W, MOS[m][0], full, slope, lo) for H, W, m, full, slope, lo in TAIL_REST]
        assert got == want, form
        # the row serves the form it was asked for
        assert all(native_out["L"][ord(c) - ord("A")][0] == form for c in codes if c != "!")
        reached.update(g for g in got if g != fm.INVALID)
    assert sorted(native_out["P"]) == [(py, f8) for py in (-1, 0, 1, 2) for f8 in (0, 1)]
    for (py, f8), codes in native_out["P"].items():
        got = _decode(codes, rows, refusals)
        assert got == [fm.phase_pick(py, bool(f8), H, W, MOS[m][0], full) for H, W, m, full in PHASE_REST], (py, f8)
        assert all(native_out["L"][ord(c) - ord("A")][0] == fm.CF_NONE for c in codes if c != "!")
        reached.update(g for g in got if g != fm.INVALID)
    assert reached == set(rows.values()), "a row no query of the sweep reaches"
