"""Carrying an extra band to the SR grid without a GPU: the properties of the definition on its numpy model
(tests/bands_model.py), the N-band GeoTIFF writer and reader, and the refusals of the job.  The GPU side is tests/test_gpu_bands.py.
(tests/test_bands_cpu.py is about something else: the row bands of a chunked whole-image call.)"""
import numpy as np
import pytest

import bands_model as bm
import consistency_model as cm
from s2sr import bands, native
from s2sr import rasterio_lite as rio
from tiff_fixture import write_tiff

H, W = 37, 45
GAINS = [(0.5, 3000), (1.5, -8000), (-0.8, 40000)]      # the negative one is what a multiplicative injection gets wrong


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("alpha,beta", GAINS)
def test_an_affine_band_comes_back_within_two_levels(S, alpha, beta):
    q = bm.scene(H, W, S)
    b, truth = bm.affine_band(q, S, alpha, beta)
    assert b.min() >= 0 and b.max() <= 65535
    out, inexact = bm.carry(q, b.astype(np.uint16), S, 0, 65535, eps=1)
    err = np.abs(out.astype(np.float64) - truth).max()
    print(f"x{S} gain {alpha}: max error {err:.2f} levels")
    assert err <= 2.0
    assert inexact == 0


@pytest.mark.parametrize("S", [2, 4])
def test_block_sums_are_n_p_unless_a_sample_clips(S):
    q = bm.scene(H, W, S)
    n = S * S
    b, _ = bm.affine_band(q, S, 0.7, 5000)
    out, inexact = bm.carry(q, b.astype(np.uint16), S, 0, 65535, eps=bm.default_eps(0, 65535))
    assert inexact == 0 and np.array_equal(cm.block_sums(out[..., None], S)[..., 0], n * b)
    # the band's own min-max as the range: samples around the extremes clip, their blocks stay inexact
    lo, hi = int(b.min()), int(b.max())
    out, inexact = bm.carry(q, b.astype(np.uint16), S, lo, hi, eps=bm.default_eps(lo, hi))
    assert 0 < inexact < H * W
    assert out.min() >= lo and out.max() <= hi
    assert inexact == int((cm.block_sums(out[..., None], S)[..., 0] != n * b).sum())
    # data straying outside the range is clamped to it first
    stray = bm.stray_band(q, S, seed=1)
    out, inexact = bm.carry(q, stray, S, 1000, 11000, eps=5)
    assert 0 < inexact < H * W and out.min() >= 1000 and out.max() <= 11000


@pytest.mark.parametrize("S", [2, 4])
def test_default_eps_beats_nearest_neighbour_by_an_order_of_magnitude(S):
    q = bm.scene(H, W, S)
    b, truth = bm.affine_band(q, S, 0.7, 5000)
    lo, hi = int(b.min()), int(b.max())
    out, _ = bm.carry(q, b.astype(np.uint16), S, lo, hi, eps=bm.default_eps(lo, hi))
    rms = lambda a: float(np.sqrt(((a - truth) ** 2).mean()))
    ours, nearest = rms(out.astype(np.float64)), rms(cm._up(b, S).astype(np.float64))
    print(f"x{S}: rms {ours:.1f} against nearest neighbour's {nearest:.1f}")
    assert ours * 10 < nearest


@pytest.mark.parametrize("S", [2, 4])
def test_masks(S):
    q = bm.scene(H, W, S)
    b = bm.stray_band(q, S, seed=2)
    v = bm.holes(H, W, seed=3)
    assert v[H - 2, W - 2] and not v[H - 3:H, W - 3:W].sum() > 1          # the isolated valid pixel
    out, inexact = bm.carry(q, b, S, 1000, 11000, r=2, eps=5, valid=v, fill=4242)
    up = cm._up(v, S) != 0
    assert (out[~up] == 4242).all()
    # garbage under the invalid pixels changes nothing on the valid blocks
    rng = np.random.default_rng(9)
    b2 = np.where(v != 0, b, rng.integers(0, 65536, b.shape)).astype(np.uint16)
    q2 = np.where(up[..., None], q, rng.integers(0, 65536, q.shape)).astype(np.uint16)
    out2, inexact2 = bm.carry(q2, b2, S, 1000, 11000, r=2, eps=5, valid=v, fill=4242)
    assert np.array_equal(out, out2) and inexact == inexact2
    # the isolated pixel: no neighbour to learn from, a flat block of p
    p = int(np.clip(b[H - 2, W - 2], 1000, 11000))
    assert (out[(H - 2) * S:(H - 1) * S, (W - 2) * S:(W - 1) * S] == p).all()
    # an all-valid mask is no mask
    a, na = bm.carry(q, b, S, 1000, 11000, valid=np.ones((H, W), np.uint8))
    c, nc = bm.carry(q, b, S, 1000, 11000)
    assert np.array_equal(a, c) and na == nc


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("flip", [False, True])
def test_the_extremes_stay_inside_int64(S, flip):
    """the 0 / 65535 checkerboards at r = 4, band with or against the guide: cov << 16 and Abar I + Cbar recomputed with Python
    integers equal the int64 model's"""
    h, w, r = 11, 13, 4
    yy, xx = np.mgrid[0:h, 0:w]
    board = ((yy + xx) % 2) * 65535
    # columns 0..3 checkered, the rest half and half: the largest covariance a window can hold lies in between
    board[:, 4:] = np.where(xx[:, 4:] % 2 == 0, 65535, 0)
    q = np.repeat(cm._up(board, S)[..., None], 3, axis=2).astype(np.uint16)
    b = (65535 - board if flip else board).astype(np.uint16)
    out, inexact, parts = bm.carry(q, b, S, 0, 65535, r=r, eps=1, parts=True)
    G, p = [[int(x) for x in row] for row in parts["G"]], [[int(x) for x in row] for row in parts["p"]]
    top = 0
    for y in range(h):
        for x in range(w):
            win = [(j, i) for j in range(max(0, y - r), min(h, y + r + 1)) for i in range(max(0, x - r), min(w, x + r + 1))]
            N, SG, Sp = len(win), sum(G[j][i] for j, i in win), sum(p[j][i] for j, i in win)
            SGG, SGp = sum(G[j][i] ** 2 for j, i in win), sum(G[j][i] * p[j][i] for j, i in win)
            cov, var = N * SGp - SG * Sp, N * SGG - SG * SG
            assert abs(cov << 16) < 2 ** 63 and int(parts["cov"][y, x]) == cov
            A = max(-bm.GAIN_LIMIT, min(bm.GAIN_LIMIT, (cov << 16) // (var + N * N)))
            C = ((Sp << 16) - A * SG) // N
            assert (int(parts["A"][y, x]), int(parts["C"][y, x])) == (A, C)
            top = max(top, abs(cov << 16).bit_length())
            assert abs(C).bit_length() <= 36
    print(f"x{S}: cov << 16 needs {top} bits")
    assert 55 <= top <= 60
    A, C, I = parts["A"].astype(object), parts["C"].astype(object), parts["I"].astype(object)
    ones = np.ones((h, w), np.int64)
    lin = bm.interpolate(A, ones, S) * I + bm.interpolate(C, ones, S)
    assert all(abs(int(v)) < 2 ** 62 for v in lin.ravel())
    assert np.array_equal(lin.astype(np.int64), parts["lin"])
    assert int(np.abs(parts["Abar"]).max()) <= 4 * S * S * bm.GAIN_LIMIT


def test_defaults_and_argument_checks():
    assert bands.default_eps(0, 65535) == 255 ** 2 == bm.default_eps(0, 65535) and bands.default_eps(10, 200) == 1
    a = bands.check_args(4, 1000, 11000)
    assert a == dict(S=4, lo=1000, hi=11000, weights=(1, 1, 1), r=2, eps=39 ** 2, fill=0, band_rows=0)
    for kw in (dict(S=3), dict(lo=5, hi=5), dict(lo=-1), dict(hi=65536), dict(weights=(0, 0, 0)), dict(weights=(256, 0, 0)), dict(weights=(1, 1)),
               dict(weights=(0.5, 1, 1)), dict(r=0), dict(r=5), dict(eps=0), dict(eps=2 ** 31), dict(fill=-1), dict(fill=65536), dict(band_rows=-1)):
        with pytest.raises(ValueError):
            bands.check_args(**{**dict(S=4, lo=0, hi=65535), **kw})
    assert bands.band_range(np.array([[5, 9], [7, 1]], np.uint16)) == (1, 9)
    assert bands.band_range(np.array([[5, 9], [7, 1]], np.uint16), np.array([[1, 0], [1, 0]])) == (5, 7)
    assert bands.band_range(np.full((2, 2), 65535, np.uint16)) == (65534, 65535) and bands.band_range(np.zeros((2, 2), np.uint16)) == (0, 1)
    assert bands.select_bands("all", 6) == [4, 5, 6] and bands.select_bands([5, 4], 5) == [5, 4]
    for bad, count in (("all", 3), ([3], 5), ([6], 5), ([4, 4], 5), ("some", 5), ([], 5), ([4.5], 5), (4, 5), ([True], 5)):
        with pytest.raises(ValueError):
            bands.select_bands(bad, count)
    assert "s2sr_carry_band_u16" in native.EXPORTED_SYMBOLS
    assert native.load_library().s2sr_carry_band_u16(None, None, None, 1, 1, 4, 0, 65535, None, 2, 1, None, 0, 0, None, None) == -1


# ---- the N-band GeoTIFF ------------------------------------------------------------------------------------------------------------
GEO = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 600000.0, 5100000.0, 0.0),
                  rio.TAG_GEOKEYS: (1, 1, 0, 1, 3072, 0, 1, 32633)})


@pytest.mark.parametrize("B", [1, 3, 4, 7])
def test_geotiff_round_trip(tmp_path, B):
    rng = np.random.default_rng(B)
    arr = rng.integers(0, 65536, (37, 29, B)).astype(np.uint16)              # 37 rows: the last strip is ragged at 16 rows per strip
    for rows, nodata in ((16, None), (64, 77)):
        path = tmp_path / f"b{B}_{rows}.tif"
        rio.write_geotiff_u16(path, arr, GEO, nodata=nodata, rows_per_strip=rows)
        back, geo = rio.read_bands_raw(path)
        assert back.dtype == np.uint16 and np.array_equal(back, arr)
        assert geo.pixel_size == (10.0, 10.0) and geo.nodata == nodata
        if B >= 3:
            rgb, _ = rio.read_rgb_raw(path)
            assert np.array_equal(rgb, arr[..., :3])
    if B == 3:
        rio.write_geotiff_rgb16(tmp_path / "rgb16.tif", arr, GEO, 64, 77)
        assert (tmp_path / "rgb16.tif").read_bytes() == (tmp_path / "b3_64.tif").read_bytes()
    for bad in (arr.astype(np.uint8), arr[..., 0], arr.astype(np.float32)):
        with pytest.raises(ValueError):
            rio.write_geotiff_u16(tmp_path / "bad.tif", bad, GEO)
    assert not (tmp_path / "bad.tif").exists()
    with pytest.raises(ValueError):
        rio.read_bands_raw(tmp_path / "x.png")


# ---- the job's refusals: all of them before a device is looked for -----------------------------------------------------------------
def _four_bands(path, dtype=np.uint16, B=4):
    rng = np.random.default_rng(1)
    arr = rng.integers(0, 200 if dtype == np.uint8 else 4000, (12, 14, B)).astype(dtype)
    write_tiff(path, arr)
    return arr


def test_the_job_refuses_before_it_looks_for_a_device(tmp_path, monkeypatch):
    from app import wow_sr

    def no_device(*a, **k):
        raise AssertionError("the refusal came after the operator was created")
    monkeypatch.setattr(wow_sr, "RealESRGAN", no_device)
    src = tmp_path / "four.tif"
    _four_bands(src)
    out = tmp_path / "out"
    cases = [
        (dict(extra_bands="all"), "bit_depth=16"),                                         # an 8-bit job
        (dict(extra_bands="all", bit_depth=8), "bit_depth=16"),
        (dict(extra_bands=[3], bit_depth=16), "below 4"),
        (dict(extra_bands=[4, 5], bit_depth=16), "not in the file"),
        (dict(extra_bands=[4, 4], bit_depth=16), "twice"),
        (dict(extra_bands="every", bit_depth=16), "all"),
        (dict(extra_bands=[], bit_depth=16), "no band"),
        (dict(extra_bands="all", extra_weights=(0, 0, 0), bit_depth=16), "weights"),
        (dict(extra_weights=(1, 1, 1), bit_depth=16), "extra_bands"),
    ]
    for kw, why in cases:
        with pytest.raises(ValueError, match=why):
            wow_sr.process_wow_sr(src, out, enhance_crops=False, **kw)
    three = tmp_path / "three.tif"
    _four_bands(three, B=3)
    with pytest.raises(ValueError, match="no band"):
        wow_sr.process_wow_sr(three, out, enhance_crops=False, bit_depth=16, extra_bands="all")
    # bands that differ in dtype: the fourth sample declared 8 bits wide
    mixed = tmp_path / "mixed.tif"
    raw = bytearray(src.read_bytes())
    import struct
    at = raw.find(struct.pack("<4H", 16, 16, 16, 16))
    assert at > 0
    raw[at:at + 8] = struct.pack("<4H", 16, 16, 16, 8)
    mixed.write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="bit depth"):
        wow_sr.process_wow_sr(mixed, out, enhance_crops=False, bit_depth=16, extra_bands="all")
    eight = tmp_path / "eight.tif"
    _four_bands(eight, np.uint8)
    with pytest.raises(ValueError, match="uint16"):
        wow_sr.process_wow_sr(eight, out, enhance_crops=False, bit_depth=16, extra_bands="all")
    assert not list(out.glob("*.tif"))


def test_the_route_refuses_with_400(tmp_path):
    from fastapi.testclient import TestClient

    from app.sr_routes import create_app
    src = tmp_path / "four.tif"
    _four_bands(src)
    client = TestClient(create_app(tmp_path / "data", tiler=False))
    for body in (dict(extra_bands="all"), dict(extra_bands=[3], bit_depth=16), dict(extra_bands=[9], bit_depth=16), dict(extra_bands="some", bit_depth=16)):
        r = client.post("/api/wow", json=dict(input_file=str(src), auto_fetch=False, **body))
        assert r.status_code == 400, (body, r.status_code, r.text)
