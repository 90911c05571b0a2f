"""Spectral indices on the GPU (include/s2sr.h: s2sr_index_nd_u16, s2sr_index_render_i16; csrc/index.hip): byte for
byte against tests/index_model.py, the independence of band_rows, the chain behind the 16-bit door's kept image, every refusal,
the launch and trip arithmetic under caps 1 and 3, and the job with its two files per index and its map tiles.  The entries under red
zones, poison, stalls and cap 8: their rows of tests/doors.py, whose baselines this module holds to the model.

The pass's capped launches are counted in the grid-cap family "display" (the launcher families are a closed list that
tests/test_gridcap_cpu.py spells out; DESIGN.md 7.8 says why the pass shares one)."""
import json

import numpy as np
import pytest

import diag
import doors
import gpu_engines
import index_model as im
from diag import same_values as same
from index_model import case, model, plane
from s2sr import index as xi
from s2sr import native

pytestmark = pytest.mark.gpu

HP = native.PREC_F16_HP
# the ragged shape, one pixel, a sliver, two tiles down and across, and 65535 pixels: 8 workgroups' worth, a ragged last group
SHAPES = [(37, 45), (1, 1), (3, 70), (33, 17), (255, 257)]
PARAMS = [(0, 0, 10000), (1000, 0, 10000), (1000, 5000, 15000), (0, 0, 1), (0, 65535, 16383)]
PLANES = [(1, 0), (3, 0), (3, 1), (3, 2)]                          # (channels per pixel, the channel read)
GRID_FAMILY = "display"


@pytest.fixture(scope="module")
def bare():
    with gpu_engines.bare(precision=HP) as e:                    # the entries need no weights
        yield e


def same_result(got, want, what):
    assert got["undefined"] == want["undefined"], f"{what}: undefined {got['undefined']} against {want['undefined']}"
    for k in ("index", "hist", "rgba", "zonal"):
        if k in got:
            same(got[k], want[k], f"{what}: {k}")


def keep(r):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in r.items()}


MASKS = [None, 1, 4]
ZONES = [None, (1, 1), (4, 7), (1, 65535), (4, 1), (1, 7), (4, 65535)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_byte_for_byte_against_the_model(bare, H, W):
    """every (ac, ca) x (bc, cb) x (offset, L, K), all outputs together; masks and zones rotate so that every mask state meets
    every zone state and every parameter set"""
    A, B, grids, lut = case(H, W)
    n = undefined = 0
    for ac, ca in PLANES:
        for bc, cb in PLANES:
            for offset, L, K in PARAMS:
                vs = MASKS[n % 3]
                zn = ZONES[(n // 3 + n) % 7]
                n += 1
                valid = None if vs is None else grids["valid", vs]
                zones, zs, Z = (None, 1, 0) if zn is None else (grids["zones", zn[0], zn[1]], zn[0], zn[1])
                want = model(A[..., ca], B[..., cb], offset, L, K, valid, vs or 1, zones, zs, Z, lut)
                got = bare.index_nd_u16(plane(A, ac, ca), plane(B, bc, cb), ca=ca, cb=cb, offset=offset, L=L, K=K, valid=valid, valid_scale=vs or 1,
                                        zones=zones, zone_scale=zs, Z=Z, lut=lut,
                                        want=("index", "hist", "rgba") + (("zonal",) if zones is not None else ()))
                same_result(got, want, f"{H} x {W} a {ac}:{ca} b {bc}:{cb} ({offset}, {L}, {K}) mask {vs} zones {zn}")
                if offset == 1000 and L == 0:
                    undefined += want["undefined"]
    if H * W > 1:
        assert undefined > 0                                     # the d == 0 path was taken


def test_masks_times_zones(bare):
    """the full product of mask states and zone states on the ragged shape"""
    H, W = 37, 45
    A, B, grids, lut = case(H, W)
    for vs in MASKS:
        for zn in ZONES:
            valid = None if vs is None else grids["valid", vs]
            zones, zs, Z = (None, 1, 0) if zn is None else (grids["zones", zn[0], zn[1]], zn[0], zn[1])
            want = model(A[..., 0], B[..., 1], 1000, 0, 10000, valid, vs or 1, zones, zs, Z, lut)
            got = bare.index_nd_u16(A, B, ca=0, cb=1, offset=1000, valid=valid, valid_scale=vs or 1, zones=zones, zone_scale=zs, Z=Z, lut=lut,
                                    want=("index", "hist", "rgba") + (("zonal",) if zones is not None else ()))
            same_result(got, want, f"mask {vs} zones {zn}")


def test_each_output_alone_and_all_together(bare):
    H, W = 33, 17
    A, B, grids, lut = case(H, W)
    a, b = plane(A, 1, 0), plane(B, 3, 2)
    kw = dict(cb=2, offset=1000, L=5000, K=15000, valid=grids["valid", 4], valid_scale=4, zones=grids["zones", 4, 7], zone_scale=4, Z=7, lut=lut)
    want = model(a, B[..., 2], 1000, 5000, 15000, grids["valid", 4], 4, grids["zones", 4, 7], 4, 7, lut)
    for outs in (("index",), ("hist",), ("rgba",), ("zonal",), (), ("index", "hist", "rgba", "zonal"), ("hist", "zonal"), ("index", "rgba")):
        got = bare.index_nd_u16(a, b, want=outs, **(kw if "zonal" in outs else dict(kw, zones=None, Z=0)))
        assert set(got) == set(outs) | {"undefined"}
        same_result(got, want, f"outputs {outs}")                # (no output at all still counts the undefined pixels)


def test_the_offset_band_takes_the_undefined_path(bare):
    """DNs in 900..1199 at offset 1000: both planes at or below the offset give d == 0"""
    rng = np.random.default_rng(4)
    a, b = (rng.integers(900, 1200, (37, 45)).astype(np.uint16) for _ in range(2))
    want = model(a, b, 1000, 0, 10000, None, 1, None, 1, 0, case(37, 45)[3])
    got = bare.index_nd_u16(a, b, offset=1000, lut=case(37, 45)[3], want=("index", "hist", "rgba"))
    same_result(got, want, "900..1199 at offset 1000")
    assert got["undefined"] > 0 and got["undefined"] == int((got["index"] == im.NODATA).sum())
    assert int(got["hist"].sum()) + got["undefined"] == 37 * 45
    assert not got["rgba"][got["index"] == im.NODATA].any()


def test_a_constant_plane_is_one_bin_and_one_zone(bare):
    H, W = 255, 257
    lut = case(H, W)[3]
    a, b = np.full((H, W), 3000, np.uint16), np.full((H, W), 1000, np.uint16)
    zones = np.full((H, W), 5, np.uint16)
    want = model(a, b, 0, 0, 10000, None, 1, zones, 1, 7, lut)
    got = bare.index_nd_u16(a, b, zones=zones, Z=7, lut=lut, want=("index", "hist", "rgba", "zonal"))
    same_result(got, want, "constant planes")
    assert got["hist"][5000 + 10000] == H * W and np.count_nonzero(got["hist"]) == 1
    assert got["zonal"][5].tolist() == [H * W, 5000 * H * W, 5000 * 5000 * H * W] and not got["zonal"][[0, 1, 2, 3, 4, 6, 7]].any()


@pytest.mark.parametrize("flip", [0, 1])
def test_the_checkerboards(bare, flip):
    """0 / 65535 checkerboards at K = 16383: the widest numerator of the definition, with L = 65535 and without"""
    H, W = 33, 70
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.where((yy + xx + flip) & 1, 65535, 0).astype(np.uint16)
    b = (65535 - a).astype(np.uint16)
    lut = case(37, 45)[3]
    zones = ((yy + xx) & 1).astype(np.uint16) + 1
    for L in (65535, 0):
        want = model(a, b, 0, L, 16383, None, 1, zones, 1, 2, lut)
        got = bare.index_nd_u16(a, b, L=L, K=16383, zones=zones, Z=2, lut=lut, want=("index", "hist", "rgba", "zonal"))
        same_result(got, want, f"checkerboard {flip}, L {L}")
        assert set(np.unique(got["index"]).tolist()) == {-im.value(65535, 0, 0, L, 16383)[0], im.value(65535, 0, 0, L, 16383)[0]}


def test_band_rows_do_not_change_a_byte(bare):
    H, W = 37, 45
    A, B, grids, lut = case(H, W)
    kw = dict(ca=1, cb=0, offset=1000, valid=grids["valid", 4], valid_scale=4, zones=grids["zones", 1, 7], zone_scale=1, Z=7, lut=lut,
              want=("index", "hist", "rgba", "zonal"))
    want = model(A[..., 1], B[..., 0], 1000, 0, 10000, grids["valid", 4], 4, grids["zones", 1, 7], 1, 7, lut)
    for rows in (0, 1, 3, H - 1):
        same_result(bare.index_nd_u16(A, plane(B, 1, 0), band_rows=rows, **kw), want, f"band_rows {rows}")
        same(bare.index_render_i16(want["index"], lut, band_rows=rows), want["rgba"], f"render, band_rows {rows}")


def test_render_equals_the_fused_rgba(bare):
    for H, W in SHAPES:
        A, B, grids, lut = case(H, W)
        got = keep(bare.index_nd_u16(A, B, ca=2, cb=2, offset=1000, valid=grids["valid", 1], lut=lut, want=("index", "rgba")))
        same(bare.index_render_i16(got["index"], lut), got["rgba"], f"{H} x {W}")
    lut2 = np.random.default_rng(8).integers(0, 256, (65536, 4)).astype(np.uint8)          # a LUT that holds something at nodata
    idx = np.random.default_rng(9).integers(-32768, 32768, (33, 17)).astype(np.int16)
    idx[::5] = im.NODATA
    same(bare.index_render_i16(idx, lut2), im.render(idx, lut2), "any int16 value through any LUT")
    for bad in (idx.astype(np.uint16), idx[0]):
        with pytest.raises(TypeError):
            bare.index_render_i16(bad, lut2)
    with pytest.raises(ValueError):
        bare.index_render_i16(idx, lut2[:, :3])


def test_kept_image_chain():
    """enhance_u16, a carried band, two indices from the device copy, then the display pass on the same copy; an unrelated call in
    between makes a=None refuse, and the engine answers again"""
    e = gpu_engines.default(1, HP)
    H, W = 9, 11
    rng = np.random.default_rng(3)
    img = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
    nir = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    lut = case(37, 45)[3]
    with e.chain_lock:
        q = np.array(e.enhance_u16(img, tile=16, pad=3))
        g = np.array(e.carry_band_u16(nir, 4)[0])
        r1 = keep(e.index_nd_u16(None, g, ca=2, lut=lut, want=("index", "hist", "rgba")))
        r2 = keep(e.index_nd_u16(None, g, ca=0, offset=1000, L=5000, K=15000, band_rows=7, want=("index", "hist")))
        hist = e.display_hist_u16(None, shape=(4 * H, 4 * W))
        r3 = keep(e.index_nd_u16(None, g, ca=2, lut=lut, want=("index", "hist", "rgba")))      # behind a display call too
    assert np.array_equal(hist, e.display_hist_u16(q))
    same_result(r1, model(q[..., 2], g, 0, 0, 10000, None, 1, None, 1, 0, lut), "a=None, channel 2")
    same_result(r2, model(q[..., 0], g, 1000, 5000, 15000, None, 1, None, 1, 0, lut), "a=None, channel 0")
    same_result(r3, r1, "a=None behind the display pass")
    same_result(keep(e.index_nd_u16(q, g, ca=2, lut=lut, want=("index", "hist", "rgba"))), r1, "the explicit image")
    with e.chain_lock:
        e.enhance_u16(img, tile=16, pad=3)
        e.enhance_u8(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8))
        with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
            e.index_nd_u16(None, g, ca=2)
        e.enhance_u16(img, tile=16, pad=3)
        with pytest.raises(native.S2srError, match="did not leave a uint16 image"):
            e.index_nd_u16(None, g[:-1], ca=2)                              # another size
        with pytest.raises(native.S2srError, match="outside its image"):
            e.index_nd_u16(None, g, ca=3)
        same_result(keep(e.index_nd_u16(None, g, ca=2, lut=lut, want=("index", "hist", "rgba"))), r1, "after the refusals the kept image still serves")


# (argument, value) overrides of one good raw call; each must return -1 before the device is touched
REFUSALS = [dict(K=0), dict(K=16384), dict(K=-1), dict(L=-1), dict(L=65536), dict(offset=-1), dict(offset=65536), dict(ac=2), dict(ac=0), dict(bc=4),
            dict(ca=3), dict(ca=-1), dict(cb=1), dict(cb=-1), dict(valid_scale=0), dict(zone_scale=0), dict(zonal=None), dict(zones=None),
            dict(Z=0), dict(Z=65536), dict(lut=None), dict(b=None), dict(H=0), dict(W=-1), dict(band_rows=-1), dict(a=None),
            dict(out=None, hist=None, zonal=None, zones=None, rgba=None, undefined=None)]


def test_every_refusal_returns_minus_one_and_leaves_the_next_call_intact(bare):
    H, W = 3, 70
    A, B, grids, lut = case(H, W)
    b1 = plane(B, 1, 1)
    valid, zones = grids["valid", 4], grids["zones", 4, 7]
    want = model(A[..., 2], b1, 1000, 0, 10000, valid, 4, zones, 4, 7, lut)
    good = dict(ca=2, offset=1000, valid=valid, valid_scale=4, zones=zones, zone_scale=4, Z=7, lut=lut, want=("index", "hist", "rgba", "zonal"))
    lib = native.load_library()
    out, hist, zonal = np.zeros((H, W), np.int16), np.zeros(20001, np.uint64), np.zeros((8, 3), np.int64)
    rgba, und = np.zeros((H, W, 4), np.uint8), np.zeros(1, np.uint64)
    base = dict(a=A, ac=3, ca=2, b=b1, bc=1, cb=0, H=H, W=W, offset=1000, L=0, K=10000, valid=valid, valid_scale=4, zones=zones, zone_scale=4, Z=7,
                lut=lut, band_rows=0, out=out, hist=hist, zonal=zonal, rgba=rgba, undefined=und)
    order = list(base)
    p = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
    assert lib.s2sr_index_nd_u16(bare._h, *[p(base[k]) for k in order]) == 0
    same(out, want["index"], "the raw call")
    same(zonal, want["zonal"], "the raw call")
    for kw in REFUSALS:                               # (a=None: the good call before it uploaded a host image, which is not kept)
        args = dict(base, **kw)
        assert lib.s2sr_index_nd_u16(bare._h, *[p(args[k]) for k in order]) == -1, kw
        same_result(bare.index_nd_u16(A, b1, **good), want, f"after the refusal of {kw}")
    for kw in (dict(idx=None), dict(lut=None), dict(rgba=None), dict(H=0), dict(W=0), dict(band_rows=-1)):
        r = dict(idx=want["index"], H=H, W=W, lut=lut, band_rows=0, rgba=rgba)
        r.update(kw)
        assert lib.s2sr_index_render_i16(bare._h, *[p(r[k]) for k in ("idx", "H", "W", "lut", "band_rows", "rgba")]) == -1, kw
        same(bare.index_render_i16(want["index"], lut), want["rgba"], f"after the render refusal of {kw}")
    # the Python layer's own refusals
    with pytest.raises(TypeError):
        bare.index_nd_u16(A.astype(np.int16), b1)
    for bad in (dict(valid=valid[:-1] if valid.shape[0] > 1 else valid[:, :-1], valid_scale=4), dict(zones=zones[:, :-1], zone_scale=4, Z=7, want=("zonal",)),
                dict(lut=lut[:, :3]), dict(want=("ndvi",))):
        with pytest.raises(ValueError):
            bare.index_nd_u16(A, b1, **bad)
    with pytest.raises(ValueError):
        bare.index_nd_u16(A[:-1], b1)
    same_result(bare.index_nd_u16(A, b1, **good), want, "after the Python refusals")


@pytest.mark.parametrize("ident", doors.owned("index_"))
def test_the_door_table_s_baseline_is_the_model(ident):
    """tests/doors.py's rows of this pass: the red-zone, poison, stall and grid-cap matrices hold every mode to diag.baseline, and
    this holds the baseline to the model, sample for sample"""
    same(diag.baseline(ident), doors.MODELS[ident](), ident)


@pytest.mark.parametrize("cap", [1, 3])
def test_under_capped_grids(bare, cap):
    """the same bytes, and the trips are what ceil(items / cap) says: 65535 pixels are 8192 groups of 8, 8 workgroups' worth of 1024"""
    H, W = 255, 257
    A, B, grids, lut = case(H, W)
    b1 = plane(B, 1, 2)
    for zn, outs in (((4, 7), ("index", "hist", "rgba", "zonal")), (None, ("index", "rgba")), ((1, 65535), ("zonal",)), (None, ("hist",))):
        zones, zs, Z = (None, 1, 0) if zn is None else (grids["zones", zn[0], zn[1]], zn[0], zn[1])
        kw = dict(ca=0, offset=1000, valid=grids["valid", 4], valid_scale=4, zones=zones, zone_scale=zs, Z=Z, lut=lut, want=outs)
        want = model(A[..., 0], b1, 1000, 0, 10000, grids["valid", 4], 4, zones, zs, Z, lut)
        with diag.under(cap):
            got = keep(bare.index_nd_u16(A, b1, **kw))
            launches, trips = native.grid_cap_stats()[GRID_FAMILY]
            ren = np.array(bare.index_render_i16(want["index"], lut))
            launches2, trips2 = native.grid_cap_stats()[GRID_FAMILY]
        same_result(got, want, f"cap {cap}, outputs {outs}")
        same(ren, want["rgba"], f"render under cap {cap}")
        items = -(-(-(-H * W // 8)) // 1024)
        assert (launches, trips) == (1, -(-items // cap)), (launches, trips, items)
        assert (launches2, trips2) == (2, max(trips, -(-(-(-(H * W) // 8) // 256) // cap)))       # the render: blocks of 256 lanes
    native.grid_cap_stats(reset=True)
    bare.index_nd_u16(A, b1, want=("index",))
    assert native.grid_cap_stats()[GRID_FAMILY] == (0, 0)             # off means off


def test_the_pass_has_a_kernel_family(bare):
    A, B, grids, lut = case(33, 17)
    bare.set_profiling(1)
    try:
        bare.reset_kernel_stats()
        bare.index_nd_u16(A, B, lut=lut, want=("index", "hist", "rgba"), band_rows=11)
        bare.index_render_i16(np.zeros((33, 17), np.int16), lut)
        bare.synchronize()
        st = bare.kernel_stats()
    finally:
        bare.set_profiling(0)
    assert st["index"]["launches"] == 4 and st["index"]["total_ms"] > 0, st["index"]
    assert st["index"]["bytes"] == 33 * 17 * 10.0 + 33 * 17 * 6.0
    assert all(v["launches"] == 0 for k, v in st.items() if k != "index")


# ---- the Python seam, the job and the map --------------------------------------------------------------------------------------------------
def _patch_weights(monkeypatch, tmp_path, nb_by_name):
    """Seeded synthetic checkpoints where the drop-in looks for them (tests/test_gpu_app.py)."""
    import torch

    from s2sr.weights import synthetic_state_dict
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir(exist_ok=True)
    for name, nb in nb_by_name.items():
        sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(nb, seed=0).items()}
        torch.save({"params_ema": sd}, tmp_path / "models" / f"{name}.pth")


def _tree(d):
    return {str(q.relative_to(d)): q.read_bytes() for q in sorted(d.rglob("*.png"))}


def test_the_wow_job_writes_indices_and_the_tiler_renders_them(monkeypatch, tmp_path):
    from PIL import Image

    import app.tiling as tiling
    from app.wow_sr import process_wow_sr
    from s2sr import rasterio_lite as rio
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    H, W = 37, 45
    rng = np.random.default_rng(52)
    four = rng.integers(1000, 4000, size=(H, W, 4)).astype(np.uint16)
    four[..., 3] = (four[..., :3].sum(axis=2) // 2 + rng.integers(0, 300, (H, W))).astype(np.uint16)     # a band that follows the guide loosely
    four[5:9, 7:30] = 0                                              # never measured
    four[20, 20, :3] = 0
    valid = (four[..., :3] != 0).any(axis=2).astype(np.uint8)
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0),
                      rio.TAG_GEOKEYS: (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32633)})
    src = tmp_path / "scene4.tif"
    rio.write_geotiff_u16(src, four, geo, nodata=0)
    zones = np.zeros((H, W), np.uint8)
    zones[10:30, 5:25], zones[12:20, 30:44] = 1, 3
    rio.write_geotiff_u16(tmp_path / "zones.tif", zones.astype(np.uint16)[..., None], geo)
    common = dict(enhance_crops=False, model="realesrgan_anime", bit_depth=16, nodata=0)
    base = process_wow_sr(src, tmp_path / "base", extra_bands=[4], **common)
    none = process_wow_sr(src, tmp_path / "none", extra_bands=[4], indices=None, **common)
    spec = ["ndvi", {"preset": "savi", "offset": 1000}, {"name": "gr", "a": 2, "b": 1, "K": 100}]
    res = process_wow_sr(src, tmp_path / "idx", extra_bands=[4], indices=spec, index_offset=0, zones=tmp_path / "zones.tif", **common)
    lean = process_wow_sr(src, tmp_path / "lean", indices=["ndvi"], **common)                       # band 4 carried for the index only
    plain = process_wow_sr(src, tmp_path / "plain", **common)
    # without the option: the same files and metadata
    strip = lambda d: {k: v for k, v in d.items() if k not in ("indices", "output_file")}
    for other in (none, res):
        assert open(other["outputs"]["sr_tif"], "rb").read() == open(base["outputs"]["sr_tif"], "rb").read()
        assert strip(other["sr_metadata"]) == strip(base["sr_metadata"])
    assert "indices" not in none["sr_metadata"] and "indices" not in none["outputs"] and set(none["outputs"]) == set(base["outputs"])
    assert sorted(p.name for p in (tmp_path / "none").iterdir()) == sorted(p.name for p in (tmp_path / "base").iterdir())
    assert open(lean["outputs"]["sr_tif"], "rb").read() == open(plain["outputs"]["sr_tif"], "rb").read()
    assert "extra_bands" not in lean["sr_metadata"] and strip(lean["sr_metadata"]) == strip(plain["sr_metadata"])
    # the files per index, against the model on the job's own product
    prod, g2 = rio.read_bands_raw(res["outputs"]["sr_tif"])
    assert prod.shape == (4 * H, 4 * W, 4)
    meta = res["sr_metadata"]["indices"]
    assert [m["name"] for m in meta] == ["ndvi", "savi", "gr"] and set(res["outputs"]["indices"]) == {"ndvi", "savi", "gr"}
    assert json.load(open(tmp_path / "idx" / "scene4_wow_sr_metadata.json"))["sr_metadata"]["indices"] == json.loads(json.dumps(meta))
    label = np.repeat(np.repeat(zones, 4, 0), 4, 1)
    for m, (a, b, off, L, K, ramp) in zip(meta, [(3, 0, 0, 0, 10000, "vegetation"), (3, 0, 1000, 5000, 15000, "vegetation"), (1, 0, 0, 0, 100, "diverging")]):
        tif, png = (tmp_path / "idx" / f"scene4_wow_sr_{m['name']}{ext}" for ext in (".tif", ".png"))
        assert tif.exists() and png.exists() and m["files"] == {"tif": str(tif), "png": str(png)}
        arr, g = rio.read_bands_raw(tif)
        assert arr.dtype == np.int16 and arr.shape == (4 * H, 4 * W, 1) and g.nodata == -32768 and g.pixel_size == (2.5, 2.5)
        want, und = im.index(prod[..., a], prod[..., b], off, L, K, valid, 4)
        same(arr[..., 0], want, f"{m['name']}: the TIFF against the model on the job's product")
        assert (m["a"], m["b"], m["offset"], m["L"], m["K"], m["undefined"], m["nodata"]) == (a + 1, b + 1, off, L, K, und, -32768)
        stops = xi.ramp_for(ramp, K)
        assert m["ramp"] == [list(s) for s in stops]
        rgba = np.asarray(Image.open(png))
        same(rgba, im.render(want, im.ramp_lut(stops)), f"{m['name']}: the PNG")
        assert np.array_equal(rgba[..., 3] != 0, want != im.NODATA)
        assert np.array_equal(rgba[..., 3] != 0, np.repeat(np.repeat(valid, 4, 0), 4, 1) != 0) or und > 0       # the alpha is the mask
        assert m["statistics"] == xi.stats_from_hist(im.hist(arr[..., 0], K), K, pixel_size=(2.5, 2.5))
        z = im.zonal(want, label, 1, 3)
        assert m["zones"] == xi.zonal_table(z, K) and [r["zone"] for r in m["zones"]] == [0, 1, 3]
    assert "zones" not in lean["sr_metadata"]["indices"][0]
    lean_arr, _ = rio.read_bands_raw(lean["outputs"]["indices"]["ndvi"]["tif"])
    same(lean_arr, rio.read_bands_raw(res["outputs"]["indices"]["ndvi"]["tif"])[0], "ndvi with and without band 4 in the product")
    # the map: the index TIFF through its ramp against the model's rendering through the existing masked path
    ndvi_tif = tmp_path / "idx" / "scene4_wow_sr_ndvi.tif"
    idx = rio.read_bands_raw(ndvi_tif)[0][..., 0]
    for ramp in ("vegetation", [(-10000, 0, 0, 255), (0, 9, 9, 9), (10000, 255, 0, 0)]):
        tag = ramp if isinstance(ramp, str) else "stops"
        tiling.process_raster_to_tiles(ndvi_tif, tmp_path / f"tiles_{tag}", min_zoom=14, max_zoom=16, ramp=ramp)
        host = im.render(idx, im.ramp_lut(xi.ramp_for(ramp)))
        d = tmp_path / f"host_{tag}"
        d.mkdir()
        rio.write_geotiff_rgb(d / "ndvi.tif", np.ascontiguousarray(host[..., :3]), g2)
        tiling.process_raster_to_tiles(d / "ndvi.tif", d / "tiles", min_zoom=14, max_zoom=16, valid=(host[..., 3] != 0).astype(np.uint8))
        got, want_tree = _tree(tmp_path / f"tiles_{tag}"), _tree(d / "tiles")
        assert got and got == want_tree, f"ramp {tag}: {len(got)} tile files against {len(want_tree)}"
        assert json.load(open(tmp_path / f"tiles_{tag}" / "tileset.json")) == json.load(open(d / "tiles" / "tileset.json"))
    seen = [np.asarray(Image.open(q)) for q in (tmp_path / "tiles_vegetation" / "16").glob("*/*.png")]
    assert any((t[..., 3] == 0).any() and (t[..., 3] == 255).any() for t in seen)                   # transparent over the nodata
    with pytest.raises(ValueError, match="single-band int16"):
        tiling.process_raster_to_tiles(res["outputs"]["sr_tif"], tmp_path / "never", ramp="vegetation")


def test_enhance16_runs_every_pairing_of_planes(monkeypatch, tmp_path):
    """image x carried, carried x image (run exchanged and mirrored back), image x image, carried x carried, with a display rendering"""
    import app.cnn_super_resolution as m
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    H, W = 20, 26
    rng = np.random.default_rng(7)
    img = rng.integers(100, 4000, (H, W, 3)).astype(np.uint16)
    extra = rng.integers(100, 4000, (H, W, 2)).astype(np.uint16)
    zones = rng.integers(0, 4, (H, W)).astype(np.uint16)
    lut = xi.ramp_lut(xi.ramp_for("diverging"))
    e = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)
    pairs = [(("img", 1), ("extra", 0)), (("extra", 0), ("img", 2)), (("img", 0), ("img", 2)), (("extra", 1), ("extra", 0))]
    spec = [dict(a=a, b=b, offset=500, L=0, K=10000, lut=lut, zones=zones, zone_scale=4, Z=3) for a, b in pairs]
    out16, carried, found = e.enhance16(img, value_range=(100, 4000), extra=extra, indices=spec)
    out16 = np.array(out16)
    assert np.array_equal(out16, np.array(e.enhance16(img, value_range=(100, 4000))))
    src = {"img": out16, "extra": carried}
    for (a, b), r in zip(pairs, found):
        want = model(src[a[0]][..., a[1]], src[b[0]][..., b[1]], 500, 0, 10000, None, 1, zones, 4, 3, lut)
        same_result(r, want, f"{a} against {b}")
    o2, disp, info, c2, f2 = e.enhance16(img, value_range=(100, 4000), extra=extra, indices=spec, display=dict(p_lo=2.0, p_hi=98.0))
    d0 = e.enhance16(img, value_range=(100, 4000), display=dict(p_lo=2.0, p_hi=98.0))
    assert np.array_equal(o2, out16) and np.array_equal(c2, carried) and np.array_equal(disp, d0[1]) and info == d0[2]
    for r, r0 in zip(f2, found):
        same_result(r, r0, "with the display rendering in the chain")
    with pytest.raises(ValueError, match="indices"):
        e.enhance16(img, indices=[dict(a=("extra", 0), b=("img", 0))])                            # no carried band to name
    with pytest.raises(ValueError, match="indices"):
        e.enhance16(img, extra=extra, indices=[dict(a=("img", 3), b=("img", 0))])


def _frozen(x):
    """a call's result out of the pinned pool the next call reuses, arrays as (dtype, shape, bytes) so that == is byte equality"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return {k: _frozen(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_frozen(v) for v in x]
    return x


def test_enhance16_is_the_flattened_product16(monkeypatch, tmp_path):
    """The form table of RealESRGAN.enhance16 over all eight combinations of display / extra / indices: the tuple's length and
    order, every member byte-equal to the same field of product16 on the same arguments, out16 that of the plain call, and
    last_extra / last_inexact_blocks the record's carried_record / inexact_blocks.  The index is image x carried with a LUT
    wherever bands are carried; without `extra` such an index is refused (no carried band to name), so it is image x image there."""
    import itertools

    import app.cnn_super_resolution as m
    monkeypatch.delenv("S2SR_PRECISION", raising=False)
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    H, W = 20, 26
    rng = np.random.default_rng(11)
    img = rng.integers(100, 4000, (H, W, 3)).astype(np.uint16)
    extra = rng.integers(100, 4000, (H, W, 2)).astype(np.uint16)
    spec = [dict(a=("img", 1), b=("extra", 1), offset=500, L=0, K=10000, lut=xi.ramp_lut(xi.ramp_for("diverging")))]
    asked = {"display": dict(p_lo=2.0, p_hi=98.0), "extra": extra, "indices": spec}
    lone = [dict(spec[0], b=("img", 2))]            # without `extra` there is no carried band to name: the index reads two image channels
    fields = {"display": ("display", "info"), "extra": ("carried",), "indices": ("indices",)}
    assert m.Product16._fields == ("out16", "display", "info", "carried", "carried_record", "indices", "inexact_blocks")
    for consistency in (None, "exact"):
        e = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256, **({} if consistency is None else {"consistency": consistency}))
        plain = _frozen(e.enhance16(img, value_range=(100, 4000)))
        assert plain[:2] == ("uint16", (4 * H, 4 * W, 3))                                      # a bare array
        for on in itertools.product((False, True), repeat=3):
            kw = {k: asked[k] for k, use in zip(("display", "extra", "indices"), on) if use}
            if "indices" in kw and "extra" not in kw:
                kw["indices"] = lone
            order = ["out16"] + [f for k in ("display", "extra", "indices") if k in kw for f in fields[k]]
            e.last_extra = None
            got = e.enhance16(img, value_range=(100, 4000), **kw)
            got = [_frozen(got)] if isinstance(got, np.ndarray) else _frozen(got)
            seen_extra, seen_inexact = _frozen(e.last_extra), e.last_inexact_blocks
            p = e.product16(img, value_range=(100, 4000), **kw)
            rec = {f: _frozen(getattr(p, f)) for f in m.Product16._fields}
            assert len(got) == len(order), (kw.keys(), len(got))
            for f, member in zip(order, got):
                assert member == rec[f], (sorted(kw), f)
            assert got[0] == plain, sorted(kw)
            assert [f for f in m.Product16._fields if rec[f] is None] == \
                [f for f in m.Product16._fields if f not in order + ["carried_record"] * ("extra" in kw) + ["inexact_blocks"] * (consistency is not None)]
            assert seen_extra == rec["carried_record"] == _frozen(e.last_extra)
            assert seen_inexact == p.inexact_blocks == e.last_inexact_blocks and (consistency is None) == (p.inexact_blocks is None)
            if "indices" in kw:
                assert set(rec["indices"][0]) == {"index", "hist", "undefined", "rgba"}
            if "display" in kw:
                assert rec["display"][:2] == ("uint8", (4 * H, 4 * W, 3)) and isinstance(p.info, dict)
