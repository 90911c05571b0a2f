"""s2sr/display.py (percentile limits, stretch LUT: the policy between the two device passes of the display rendering, DESIGN.md
7.3) pinned to the from-scratch model of tests/display_model.py, plus the CPU-side seams: exported symbols, the job's refusals."""
import functools

import numpy as np
import pytest

import display_model as M
from s2sr import display as D
from s2sr import native

PCTS = [(0, 100), (2, 98), (0.01, 99.99)]


@functools.lru_cache(maxsize=None)
def image(kind):
    """The inputs the tests share (never written to)."""
    rng = np.random.default_rng(7)
    if kind == "full":
        a = rng.integers(0, 65536, size=(61, 47, 3))
    elif kind == "narrow":
        a = rng.integers(1000, 3001, size=(61, 47, 3))
        a[..., 1] += 500                                         # the bands differ: linked and unlinked limits differ
    elif kind == "const":
        a = np.broadcast_to(np.array([700, 700, 9]), (5, 6, 3))
    elif kind == "zero":
        a = np.zeros((4, 4, 3))
    elif kind == "nodata":
        a = np.full((6, 5, 3), 321)
    elif kind == "one":
        a = np.array([[[5, 60000, 0]]])
    elif kind == "two":                                          # two values, one of them the nodata value
        a = np.where(rng.random((30, 31, 3)) < 0.3, 321, 40000)
    a = np.ascontiguousarray(a).astype(np.uint16)
    a.setflags(write=False)
    return a


NODATA = {"nodata": 321, "two": 321}


@functools.lru_cache(maxsize=None)
def model_lut(lims, gamma):
    return M.lut([list(p) for p in lims], gamma)


@pytest.mark.parametrize("kind", ["full", "narrow", "const", "zero", "nodata", "one", "two"])
@pytest.mark.parametrize("linked", [True, False])
@pytest.mark.parametrize("p", PCTS)
def test_limits_equal_the_sorted_sample_model(kind, linked, p):
    img, nd = image(kind), NODATA.get(kind)
    st = D.Stretch(p_lo=p[0], p_hi=p[1], linked=linked, nodata=nd)
    h = M.hist(img, nd)
    got = D.limits_from_hist(h, st)
    want = M.limits(img, p[0], p[1], linked, nd)
    assert got == want, (got, want)
    assert all(0 <= lo < hi <= 65535 for lo, hi in got)
    if kind == "nodata":
        assert h.sum() == 0 and got == [[0, 1]] * 3               # every sample left out
    if kind == "one" and not linked:
        assert got == [[4, 5], [59999, 60000], [0, 1]]
    if p == (0, 100) and kind in ("full", "narrow") and not linked:
        assert got == [[int(img[..., c].min()), int(img[..., c].max())] for c in range(3)]


@pytest.mark.parametrize("lims", [((0, 65535),) * 3, ((1000, 3000), (1500, 3500), (0, 1)), ((4, 5), (65534, 65535), (123, 40000)),
                                  ((0, 2), (10, 13), (100, 355))])
def test_lut_gamma_1_is_the_integer_formula_everywhere(lims):
    got = D.build_lut([list(p) for p in lims], 1.0)
    assert got.dtype == np.uint8 and got.shape == (3, 65536)
    assert np.array_equal(got, model_lut(lims, 1.0))
    for c, (lo, hi) in enumerate(lims):
        assert (got[c, : lo + 1] == 0).all() and (got[c, hi:] == 255).all()
    # round half up: 3 steps over 255 -> 1/3 -> 85, 2/3 -> 170; x - lo = 1 of 2 -> 127.5 -> 128
    assert list(D.build_lut([[10, 13]] * 3)[0, 10:14]) == [0, 85, 170, 255]
    assert D.build_lut([[0, 2]] * 3)[0, 1] == 128


def test_lut_gamma_2_2():
    lims = [[1000, 3000], [0, 65535], [4, 5]]
    got = D.build_lut(lims, 2.2)
    for c, (lo, hi) in enumerate(lims):
        assert (got[c, : lo + 1] == 0).all() and (got[c, hi:] == 255).all()
        assert (np.diff(got[c].astype(np.int16)) >= 0).all()
    # by hand: t = 0.5 -> 255 * 0.5 ** (1 / 2.2) = 186.08 -> 186; t = 0.25 -> 135.79 -> 136; t = 0.01 -> 31.44 -> 31
    assert got[0, 2000] == 186 and got[0, 1500] == 136 and got[0, 1020] == 31
    # t = 1 / 65535 -> 255 * 0.00646 = 1.65 -> 2; t = 0.75 -> 223.74 -> 224
    assert got[1, 1] == 2 and got[1, 49151] == 224
    for c, x in [(0, 1001), (0, 2999), (0, 2345), (1, 32768), (1, 65534), (1, 7)]:
        assert got[c, x] == M.lut_entry(x, *lims[c], 2.2)
    assert (got >= D.build_lut(lims, 1.0)).all()                   # gamma > 1 brightens


def test_refusals():
    for bad in [dict(p_lo=2.005), dict(p_hi=97.123), dict(p_lo=50, p_hi=50), dict(p_lo=60, p_hi=40), dict(p_lo=-1), dict(p_hi=100.01),
                dict(gamma=0), dict(gamma=-1.0), dict(gamma=float("nan")), dict(nodata=65536), dict(nodata=-1), dict(limits=[[5, 5]] * 3),
                dict(limits=[1, 2, 3])]:
        with pytest.raises(ValueError):
            D.Stretch(**bad)
    with pytest.raises(ValueError):
        D.Stretch.of({"percentile": 2})
    with pytest.raises(ValueError):
        D.build_lut([[0, 1]] * 3, 0.0)
    with pytest.raises(ValueError):
        D.limits_from_hist(np.zeros((3, 256), np.uint64), D.Stretch())
    s = D.Stretch.of({"p_lo": 0.01, "p_hi": 99.99, "linked": False, "limits": [7, 9]})
    assert s.basis_points == (1, 9999) and s.limits == [[7, 9]] * 3
    assert D.Stretch().info([[1, 2]] * 3) == {"p_lo": 2.0, "p_hi": 98.0, "linked": True, "gamma": 1.0, "nodata": None, "limits": [[1, 2]] * 3}


class _HostEngine:
    """The two device passes in numpy: render_u16's policy and call protocol without a GPU."""

    def __init__(self):
        self.calls, self.left = [], None

    def display_hist_u16(self, img, nodata=-1, band_rows=0, shape=None):
        self.calls.append(("hist", img is None))
        if img is not None:
            self.left = img
        assert self.left.shape[:2] == tuple(shape)
        return M.hist(self.left, None if nodata < 0 else nodata)

    def display_apply_u16(self, img, lut, band_rows=0, shape=None):
        self.calls.append(("apply", img is None))
        if img is not None:
            self.left = img
        assert self.left.shape[:2] == tuple(shape)
        return M.apply(self.left, lut)


@pytest.mark.parametrize("kind,kw", [("narrow", {}), ("narrow", {"linked": False, "p_lo": 0, "p_hi": 100}), ("two", {"nodata": 321, "linked": False}),
                                     ("const", {"linked": False})])
def test_render_equals_the_model_and_uploads_once(kind, kw):
    img, eng = image(kind), _HostEngine()
    out, info = D.render_u16(img, kw, eng)
    want, lims = M.render(img, **kw)
    assert out.dtype == np.uint8 and np.array_equal(out, want) and info["limits"] == lims
    assert eng.calls == [("hist", False), ("apply", True)]        # the apply pass reads the histogram pass' upload
    # explicit limits: no histogram pass; the device copy: no upload at all
    eng2 = _HostEngine()
    out2, info2 = D.render_u16(img, dict(kw, limits=lims), eng2)
    assert np.array_equal(out2, want) and info2 == info and eng2.calls == [("apply", False)]
    out3, _ = D.render_u16(None, kw, eng2, shape=img.shape[:2])
    assert np.array_equal(out3, want) and eng2.calls[1:] == [("hist", True), ("apply", True)]
    with pytest.raises(ValueError):
        D.render_u16(None, kw, eng2)
    with pytest.raises(ValueError):
        D.render_u16(img.astype(np.uint8), kw, eng2)


def test_symbols_are_exported():
    assert "s2sr_display_hist_u16" in native.EXPORTED_SYMBOLS and "s2sr_display_apply_u16" in native.EXPORTED_SYMBOLS
    lib = native.load_library()
    assert hasattr(lib, "s2sr_display_hist_u16") and hasattr(lib, "s2sr_display_apply_u16")


def test_job_refuses_display_on_an_8_bit_job_before_anything_is_created(tmp_path):
    from app.wow_sr import apply_wow_sr, process_wow_sr
    out = tmp_path / "never"
    with pytest.raises(ValueError, match="bit_depth=16"):
        process_wow_sr(tmp_path / "missing.tif", out, enhance_crops=False, bit_depth=8, display={"p_lo": 2, "p_hi": 98})
    with pytest.raises(ValueError, match="bit_depth=16"):
        apply_wow_sr(tmp_path / "missing.tif", out / "x.tif", enhance_crops=False, display={})
    with pytest.raises(ValueError, match="basis points"):
        process_wow_sr(tmp_path / "missing.tif", out, enhance_crops=False, bit_depth=16, display={"p_lo": 2.005})
    with pytest.raises(ValueError, match="enhance_crops"):       # today's refusal stays: no display image, no post-process
        process_wow_sr(tmp_path / "missing.tif", out, enhance_crops=True, bit_depth=16)
    assert not out.exists()
