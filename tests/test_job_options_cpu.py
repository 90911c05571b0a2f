"""app/job_options.py held to what the job path did before it: the keywords that cross every call seam (tests/job_options_model.py,
the hand-written ladders transcribed), and the refusals -- the ValueErrors of the job functions and the 400s of /api/wow, recorded
in tests/golden/job_option_refusals.txt from the last commit without the record.

    python tests/test_job_options_cpu.py > tests/golden/job_option_refusals.txt

records the table through the public seams (process_wow_sr and the route), so it runs on any commit."""
import itertools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden" / "job_option_refusals.txt"

# ---- a. the ladders -------------------------------------------------------------------------------------------------------------
GROUPS = [                                      # every state of every option group; the first of each is "not asked for"
    [{}, {"seam_blend": True}],
    [{}, {"bit_depth": 16}],
    [{}, {"display": {"p_lo": 2.0, "p_hi": 98.0}}],
    [{}, {"nodata": 0}, {"nodata": "tag", "fill_radius": 7}],
    [{}, {"consistency": "smooth"}],
    [{}, {"extra_bands": "all"}, {"extra_bands": [4], "extra_weights": (2, 1, 1)}, {"extra_weights": (2, 1, 1)}],
    [{}, {"indices": ["ndvi"]}, {"indices": ["ndvi"], "zones": "zones.tif"}, {"indices": ["ndvi"], "index_offset": 1000},
     {"indices": ["ndvi"], "zones": "zones.tif", "index_offset": 1000}, {"index_offset": 1000}, {"zones": "zones.tif"}],
    [{}, {"transparent_tiles": True}],
]
COMBOS = [{k: v for part in parts for k, v in part.items()} for parts in itertools.product(*GROUPS)]


def test_every_seam_passes_the_keywords_the_hand_written_ladders_passed():
    from app.job_options import SEAMS, JobOptions
    from job_options_model import SEAMS as MODEL
    assert set(SEAMS) == set(MODEL) and len(COMBOS) == 2 * 2 * 2 * 3 * 2 * 4 * 7 * 2
    for kw in COMBOS:
        o = JobOptions(**kw)
        for seam, ladder in MODEL.items():
            assert o.passed(seam) == ladder(o), (seam, kw)
    for seam in MODEL:                          # a job that asks for nothing: the reference's call, at every seam
        assert JobOptions().passed(seam) == {}
        assert JobOptions(fill_radius=7, extra_weights=(2, 1, 1), index_offset=5, zones="z.tif").passed(seam) == {}     # riders alone do not travel


def test_the_record_is_frozen_and_reads_a_request():
    import dataclasses

    from app.job_options import JobOptions
    from app.sr_routes import SRRequest, WowRequest
    with pytest.raises(dataclasses.FrozenInstanceError):
        JobOptions().seam_blend = True
    assert [f.name for f in dataclasses.fields(JobOptions)] == [
        "seam_blend", "bit_depth", "display", "nodata", "fill_radius", "consistency", "extra_bands", "extra_weights", "indices",
        "index_offset", "zones", "transparent_tiles"]
    assert dataclasses.asdict(JobOptions.from_request(WowRequest())) == dataclasses.asdict(JobOptions())
    o = JobOptions.from_request(WowRequest(bit_depth=16, nodata="tag", fill_radius=5, indices=["ndvi"], index_offset=1000, transparent_tiles=True))
    assert (o.bit_depth, o.nodata, o.fill_radius, o.indices, o.index_offset, o.transparent_tiles) == (16, "tag", 5, ["ndvi"], 1000, True)
    o = JobOptions.from_request(SRRequest(seam_blend=True, consistency="exact"))
    assert o.passed("run_sr_job") == {"seam_blend": True, "consistency": "exact"}


# ---- b. the refusals ------------------------------------------------------------------------------------------------------------
# name -> (enhance_crops, options).  One per raise of the old _check_bit_depth, then pairs whose refusals compete.
CHECKS = {
    "nodata-form": (True, dict(nodata=1.5)),
    "fill-radius": (True, dict(nodata=0, fill_radius=0)),
    "fill-radius-without-nodata": (True, dict(fill_radius=99)),
    "consistency": (True, dict(consistency="both")),
    "nodata-range": (True, dict(nodata=70000)),
    "nodata-negative": (False, dict(nodata=-1, bit_depth=16)),
    "bit-depth": (True, dict(bit_depth=12)),
    "extra-bands-8-bit": (True, dict(extra_bands="all")),
    "extra-bands-form": (False, dict(bit_depth=16, extra_bands="some")),
    "extra-bands-below-4": (False, dict(bit_depth=16, extra_bands=[3])),
    "extra-bands-twice": (False, dict(bit_depth=16, extra_bands=[4, 4])),
    "extra-bands-empty": (False, dict(bit_depth=16, extra_bands=[])),
    "extra-weights-zero": (False, dict(bit_depth=16, extra_bands=[4], extra_weights=(0, 0, 0))),
    "extra-weights-alone": (False, dict(bit_depth=16, extra_weights=(1, 1, 1))),
    "indices-8-bit": (True, dict(indices=["ndvi"])),
    "indices-unknown-preset": (False, dict(bit_depth=16, indices=["nope"])),
    "indices-empty": (False, dict(bit_depth=16, indices=[])),
    "indices-offset": (False, dict(bit_depth=16, indices=["ndvi"], index_offset=-1)),
    "zones-alone": (False, dict(bit_depth=16, zones="zones.tif")),
    "index-offset-alone": (True, dict(index_offset=1000)),
    "display-8-bit": (True, dict(display={})),
    "display-percentiles": (True, dict(bit_depth=16, display={"p_lo": 90.0, "p_hi": 10.0})),
    "display-unknown-field": (True, dict(bit_depth=16, display={"stretch": 1})),
    "crops-16-bit": (True, dict(bit_depth=16)),
    # competing refusals: the order of the checks
    "order-fill-radius-before-consistency": (True, dict(nodata=0, fill_radius=0, consistency="both")),
    "order-nodata-range-before-bit-depth": (True, dict(nodata=70000, bit_depth=12)),
    "order-extra-bands-before-indices-before-display": (True, dict(extra_bands="all", indices=["ndvi"], display={})),
    "order-indices-before-crops": (True, dict(bit_depth=16, indices=["nope"])),
    "order-extra-weights-before-display": (True, dict(extra_weights=(1, 1, 1), display={})),
}

# name -> the JSON body of POST /api/wow (input_file, unless given as None: a 4-band uint16 GeoTIFF) -- every 400 of the route, pairs that compete, and what
# the route lets through to the job (200: the job then fails with the job functions' message)
ROUTES = {
    "bit-depth": {"bit_depth": 12},
    "display-8-bit": {"display": {}},
    "display-percentiles": {"bit_depth": 16, "display": {"p_lo": 90.0, "p_hi": 10.0}},
    "display-unknown-field": {"bit_depth": 16, "display": {"stretch": 1}},
    "nodata-form": {"nodata": "none"},
    "fill-radius": {"nodata": 0, "fill_radius": 0},
    "transparent-tiles": {"transparent_tiles": True},
    "consistency": {"consistency": "both"},
    "extra-bands-8-bit": {"extra_bands": "all"},
    "extra-bands-below-4": {"bit_depth": 16, "extra_bands": [3]},
    "extra-bands-not-in-file": {"bit_depth": 16, "extra_bands": [9]},
    "indices-8-bit": {"indices": ["ndvi"]},
    "indices-unknown-preset": {"bit_depth": 16, "indices": ["nope"]},
    "indices-not-in-file": {"bit_depth": 16, "indices": [{"preset": "ndre", "nir": 4, "rededge": 9}]},
    "index-offset-alone": {"index_offset": 1000},
    "order-bit-depth-before-display": {"bit_depth": 12, "display": {}},
    "order-display-before-nodata": {"display": {}, "nodata": "none"},
    "order-nodata-before-transparent-before-consistency": {"nodata": "none", "transparent_tiles": True, "consistency": "both"},
    "order-transparent-before-consistency": {"transparent_tiles": True, "consistency": "both"},
    "order-consistency-before-extra-bands": {"consistency": "both", "extra_bands": "all"},
    "order-extra-bands-before-indices": {"bit_depth": 16, "extra_bands": [3], "indices": ["nope"]},
    "passes-extra-bands-no-file": {"bit_depth": 16, "extra_bands": [9], "input_file": None},
    "passes-nodata-range": {"nodata": 70000},
    "passes-crops-16-bit": {"bit_depth": 16},
}


def _raised(fn):
    try:
        fn()
    except Exception as e:                      # noqa: BLE001 -- the type is part of the record
        return type(e).__name__, str(e)
    return "-", None


def _route_answers(tmp: Path):
    """-> {name: (status, detail, the job's message or None)} of ROUTES through TestClient, with no tiler, as test_app_cpu does"""
    from fastapi.testclient import TestClient

    from app.sr_routes import create_app
    from s2sr import rasterio_lite as rio
    src = tmp / "four_bands.tif"
    rio.write_geotiff_u16(src, np.random.default_rng(5).integers(0, 4000, size=(6, 7, 4)).astype(np.uint16), rio.GeoRef({}))
    c = TestClient(create_app(tmp / "data", tiler=False))
    out = {}
    for name, body in ROUTES.items():
        body = {"input_file": str(src), **body}
        r = c.post("/api/wow", json={k: v for k, v in body.items() if v is not None})
        msg = None
        if r.status_code == 200:
            msg = c.get(f"/api/sr/{r.json()['job_id']}").json()["message"]
        out[name] = (r.status_code, r.json().get("detail"), msg)
    return out


def _golden():
    rows = [line.rstrip("\n").split("\t") for line in GOLDEN.read_text().splitlines() if line and not line.startswith("#")]
    return {(r[0], r[1]): tuple(json.loads(x) for x in r[2:]) for r in rows}


def test_check_raises_the_recorded_refusals():
    from app.job_options import JobOptions
    want = _golden()
    assert {k[1] for k in want if k[0] == "check"} == set(CHECKS)
    for name, (crops, kw) in CHECKS.items():
        got = _raised(lambda: JobOptions(**kw).check(crops))
        assert got == want["check", name] and got[0] != "-", name
    # with the file's band count, what the route refuses with the file at hand
    for name in ("extra-bands-not-in-file", "indices-not-in-file"):
        kw = {k: v for k, v in ROUTES[name].items()}
        assert _raised(lambda: JobOptions(**kw).check(False, 4)) == ("ValueError", want["route", name][1]), name
        JobOptions(**kw).check(False)


def test_the_job_functions_refuse_the_same_before_anything_is_created(tmp_path):
    from app import wow_sr
    want = _golden()
    for name, (crops, kw) in CHECKS.items():
        for fn in (wow_sr.process_wow_sr, wow_sr.apply_wow_sr):
            assert _raised(lambda: fn(tmp_path / "none.tif", tmp_path / "out" / name, crops, **kw)) == want["check", name], (name, fn.__name__)
    assert not (tmp_path / "out").exists()


def test_api_wow_answers_the_recorded_statuses_and_details(tmp_path):
    want = _golden()
    got = _route_answers(tmp_path)
    assert {k[1] for k in want if k[0] == "route"} == set(ROUTES)
    for name in ROUTES:
        assert got[name] == want["route", name], name
    assert sum(1 for v in got.values() if v[0] == 400) >= 20 and all(v[0] in (200, 400) for v in got.values())


if __name__ == "__main__":
    import tempfile
    for p in (str(REPO / "sentinel2-super-resolution-poc_amd"), str(REPO)):
        if p not in sys.path:
            sys.path.insert(0, p)
    from app import wow_sr
    print("# The refusals of a job's options, recorded from commit 20344e9 (the last with _check_bit_depth and the route's own checks)")
    print("# by `python tests/test_job_options_cpu.py`.  Tab-separated; every field behind the name is JSON.")
    print("# check <name> <exception type> <message>          -- process_wow_sr(<no file>, <dir>, enhance_crops, **CHECKS[name])")
    print("# route <name> <status> <detail> <job message>     -- POST /api/wow with ROUTES[name]")
    with tempfile.TemporaryDirectory() as d:
        for name, (crops, kw) in CHECKS.items():
            print("\t".join(["check", name] + [json.dumps(x) for x in _raised(lambda: wow_sr.process_wow_sr(Path(d) / "none.tif", Path(d) / "out", crops, **kw))]))
        for name, row in _route_answers(Path(d)).items():
            print("\t".join(["route", name] + [json.dumps(x) for x in row]))
