"""GPU parity of the post-process kernels (through s2sr_postprocess_u8) against the numpy
oracle: every stage is integer / fixed-point or a fixed sequence of float32 operations, so
the bar is BIT-EXACT."""
import numpy as np
import pytest

from doors import banded
from oracle import postprocess_ref as pp
from s2sr import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = native.Engine(num_block=1)
    yield e
    e.close()


def _imgs():
    rng = np.random.default_rng(4)
    out = []
    # smooth green-dominant field-like image (exercises the hue 36..84 branch), cf. SURVEY 8d
    base = rng.integers(0, 256, (96, 128, 3)).astype(np.float32)
    k = np.ones((5, 5), np.float32) / 25
    sm = np.stack([np.convolve(base[..., c].ravel(), np.ones(25) / 25, "same").reshape(96, 128) for c in range(3)], -1)
    g = np.clip(sm * np.array([0.5, 1.0, 0.45]) + np.array([20, 60, 10]), 0, 255).astype(np.uint8)
    out.append(("green", g))
    out.append(("noise", rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)))
    out.append(("ragged", rng.integers(0, 256, (67, 101, 3), dtype=np.uint8)))      # CLAHE pads both dims
    out.append(("half_ragged", rng.integers(0, 256, (64, 100, 3), dtype=np.uint8)))  # one dim divisible
    out.append(("flat", np.full((40, 48, 3), 100, np.uint8)))
    grad = np.zeros((128, 256, 3), np.uint8)
    grad[..., 0] = np.arange(256)[None, :]
    grad[..., 1] = (np.arange(128) * 2)[:, None]
    grad[..., 2] = 255 - np.arange(256)[None, :]
    out.append(("gradient", grad))
    return out


@pytest.mark.parametrize("name,img", _imgs())
def test_stages_bit_exact(eng, name, img):
    P = native.PPParams
    cases = {
        "clahe": (P(2.5, 8, 1.2, 1.4, -0.4, 35, 85, 1.2, 1), lambda x: pp.local_contrast(x, 2.5, 8)),
        "clahe3": (P(3.0, 8, 1.0, 1.0, 0.0, 35, 85, 1.0, 1), lambda x: pp.local_contrast(x, 3.0, 8)),
        "unsharp_wow": (P(2.5, 8, 1.2, 1.4, -0.4, 35, 85, 1.2, 2), lambda x: pp.unsharp(x, 1.2, 1.4, -0.4)),
        "unsharp_farm": (P(2.5, 8, 1.5, 2.2, -1.2, 35, 85, 1.3, 2), lambda x: pp.unsharp(x, 1.5, 2.2, -1.2)),
        "veg12": (P(2.5, 8, 1.2, 1.4, -0.4, 35, 85, 1.2, 4), lambda x: pp.vegetation(x, 1.2)),
        "veg13": (P(2.5, 8, 1.2, 1.4, -0.4, 35, 85, 1.3, 4), lambda x: pp.vegetation(x, 1.3)),
        "wow": (native.pp_wow(), pp.enhance_for_crops),
        "farm": (native.pp_farm(), pp.farm_postprocess),
    }
    for cname, (prm, fn) in cases.items():
        got = eng.postprocess_u8(img, prm)
        exp = fn(img)
        d = np.abs(got.astype(np.int16) - exp.astype(np.int16))
        assert d.max() == 0, f"{name}/{cname}: {int((d > 0).sum())} bytes differ, max {int(d.max())}"


def test_all_hsv_and_lab_values(eng):
    """Every (hue, sat) pair at two values, and a dense RGB lattice: exhaustive over the LUT domains."""
    h, s = np.meshgrid(np.arange(180), np.arange(256), indexing="ij")
    for v in (255, 131):
        hsv = np.stack([h, s, np.full_like(h, v)], -1).astype(np.uint8)
        rgb = pp.hsv2rgb_u8(hsv)
        for gain, prm in ((1.2, native.pp_wow()), (1.3, native.pp_farm())):
            prm.stages = 4
            assert np.array_equal(eng.postprocess_u8(rgb, prm), pp.vegetation(rgb, gain))
    r, g, b = np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 5), np.arange(0, 256, 5), indexing="ij")
    lat = np.stack([r, g, b], -1).reshape(52 * 4, 13 * 52, 3).astype(np.uint8)
    prm = native.pp_wow()
    prm.stages = 1
    assert np.array_equal(eng.postprocess_u8(lat, prm), pp.local_contrast(lat, 2.5, 8))


def test_wow_on_sr_sized_image(eng):
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
    img[..., 1] = np.maximum(img[..., 1], 90)
    assert np.array_equal(eng.postprocess_u8(img, native.pp_wow()), pp.enhance_for_crops(img))


def test_radius3_tiny_and_misaligned_batch(eng):
    """The restructured sharpen kernel: radius 3 (sigma 1.0), an image smaller than the blur radius,
    and a batch whose images start at odd byte offsets (dword staging of interior tiles)."""
    import torch

    P = native.PPParams
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (70, 210, 3), dtype=np.uint8)
    prm = P(3.0, 8, 1.0, 2.5, -1.5, 35, 85, 1.3, 2)          # apply_unsharp_mask(strength=1.5, radius=1.0)
    assert np.array_equal(eng.postprocess_u8(img, prm), pp.unsharp(img, 1.0, 2.5, -1.5))
    tiny = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)
    for sigma, a, b in ((1.2, 1.4, -0.4), (1.5, 2.2, -1.2)):
        prm = P(2.5, 8, sigma, a, b, 35, 85, 1.2, 2)
        assert np.array_equal(eng.postprocess_u8(tiny, prm), pp.unsharp(tiny, sigma, a, b))
    batch = rng.integers(0, 256, (3, 35, 203, 3), dtype=np.uint8)   # 21315 bytes per image: odd offsets
    batch[..., 1] = np.maximum(batch[..., 1], 100)
    x = torch.from_numpy(batch).cuda()
    y = torch.empty_like(x)
    for prm, fn in ((native.pp_wow(), pp.enhance_for_crops), (native.pp_farm(), pp.farm_postprocess)):
        eng.postprocess_batch_u8_dev(x.data_ptr(), 3, 35, 203, prm, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        for i in range(3):
            assert np.array_equal(got[i], fn(batch[i])), f"image {i}"
    # a view that starts 1 byte into its buffer: the first dword of the first row straddles the start
    flat = torch.empty(1 + 35 * 203 * 3, dtype=torch.uint8, device="cuda")
    flat[1:] = torch.from_numpy(batch[0].ravel()).cuda()
    out = torch.empty(35 * 203 * 3, dtype=torch.uint8, device="cuda")
    eng.postprocess_batch_u8_dev(flat.data_ptr() + 1, 1, 35, 203, native.pp_wow(), out.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(35, 203, 3), pp.enhance_for_crops(batch[0]))


def test_full_pipelines_on_tiny_and_thin_images(eng):
    """Images smaller than the CLAHE grid / the blur radius, 1-pixel wide or high: every stage pads by
    reflection (more than one bounce) and must still match the oracle bit for bit."""
    rng = np.random.default_rng(13)
    for shape in ((1, 1, 3), (1, 9, 3), (7, 1, 3), (3, 5, 3), (8, 8, 3), (9, 17, 3), (2, 300, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        img[..., 1] = np.maximum(img[..., 1], 90)
        for prm, fn in ((native.pp_wow(), pp.enhance_for_crops), (native.pp_farm(), pp.farm_postprocess)):
            got = eng.postprocess_u8(img, prm)
            assert np.array_equal(got, fn(img)), shape


def test_banded_postprocess_gives_the_bytes_of_the_whole_image(eng):
    """The band-wise route an AOI's mosaic takes (engine_aoi.hip enhance_locked, s2sr/dist.py: CLAHE histograms counted as the bands are
    stitched, LUTs behind the last band, apply + sharpen band by band in front of the copy out) against the whole-image launch:
    ragged sizes (both CLAHE paddings, the reflected rows counted into the last tile row from whichever band holds them), images
    smaller than the grid (padding that bounces more than once), bands that are no multiple of any tile, one-row bands, in place,
    BGR bytes and the swap on the way out, the farm constants, single stages."""
    rng = np.random.default_rng(31)
    P = native.PPParams
    cases = [((257, 301), [0, 40, 41, 130, 200, 257], [0, 33, 100, 101, 257]),
             ((256, 512), [0, 256], [0, 64, 128, 256]),
             ((67, 101), [0, 10, 60, 67], [0, 67]),
             ((131, 64), [0, 1, 2, 3, 120, 131], [0, 7, 14, 131]),
             ((5, 9), [0, 2, 5], [0, 1, 5]),          # smaller than the 8x8 grid and than the blur radius
             ((9, 17), [0, 9], [0, 4, 9]),
             ((1, 40), [0, 1], [0, 1])]
    for (H, W), hc, rc in cases:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        img[..., 1] = np.maximum(img[..., 1], 90)
        for prm in (native.pp_wow(), native.pp_farm()):
            want = eng.postprocess_u8(img, prm)
            assert np.array_equal(banded(eng, img, prm, hc, rc), want), (H, W, "rgb")
            assert np.array_equal(banded(eng, img, prm, hc, rc, in_place=True), want), (H, W, "in place")
            bgr = np.ascontiguousarray(img[:, :, ::-1])
            got = banded(eng, bgr, prm, hc, rc, native.PP_ORDER_BGR, in_place=True)
            assert np.array_equal(got[:, :, ::-1], want), (H, W, "bgr in, bgr out")
            got = banded(eng, bgr, prm, hc, rc, native.PP_ORDER_BGR | native.PP_ORDER_SWAP_OUT)
            assert np.array_equal(got, want), (H, W, "bgr in, rgb out")
            got = banded(eng, img, prm, hc, rc, native.PP_ORDER_SWAP_OUT)
            assert np.array_equal(got[:, :, ::-1], want), (H, W, "rgb in, bgr out")
    img = rng.integers(0, 256, (150, 203, 3), dtype=np.uint8)
    for stages in (1, 2, 3, 4, 5, 6):
        prm = P(2.5, 8, 1.2, 1.4, -0.4, 35, 85, 1.2, stages)
        assert np.array_equal(banded(eng, img, prm, [0, 70, 150], [0, 31, 150], in_place=True), eng.postprocess_u8(img, prm)), stages
    # misuse is refused, not computed: rows before the LUTs, bands out of order
    import torch
    x = torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda")
    eng.pp_band_begin_dev(64, 64, native.pp_wow(), 0, 0)
    with pytest.raises(native.S2srError):
        eng.pp_band_rows_dev(x.data_ptr(), 0, 32, x.data_ptr(), 0)
    eng.pp_band_hist_dev(x.data_ptr(), 0, 64, 0)
    eng.pp_band_lut_dev(0)
    with pytest.raises(native.S2srError):
        eng.pp_band_rows_dev(x.data_ptr(), 32, 64, x.data_ptr(), 0)
    eng.pp_band_rows_dev(x.data_ptr(), 0, 64, x.data_ptr(), 0)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def weng():
    """a handle with weights (s2sr_enhance_job_u8 runs the net) whose scratch only ever serves 64 x 64 post-process work"""
    from s2sr.weights import synthetic_state_dict
    e = native.Engine(num_block=1)
    e.load_state_dict(synthetic_state_dict(1, seed=0))
    yield e
    e.close()


def _take_batch_dev(e, img, prm):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(img[:40, :48])).cuda()
    y = torch.empty_like(x)
    e.postprocess_batch_u8_dev(x.data_ptr(), 1, 40, 48, prm, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


# calls that take the scratch area a banded run keeps its histograms, LUTs and CLAHE'd rows in.  Each works on the run's 64 x 64
# pixels or fewer (an enhance job's output is 4 x its input), so the area is never regrown.
_TAKERS = {
    "postprocess_u8": lambda e, img, prm: e.postprocess_u8(img, prm),
    "postprocess_batch_u8_dev": _take_batch_dev,
    "enhance_job_u8": lambda e, img, prm: e.enhance_job_u8(img[:16, :16], prm),
}


@pytest.mark.parametrize("taker", list(_TAKERS))
def test_banded_run_is_void_once_its_scratch_is_taken(weng, taker):
    """Another post-process on the handle between begin and the last rows band overwrites the run's state: the run's next call must
    fail (it used to pass `open && !lut` and answer with wrong bytes), and a complete run afterwards gives the whole image's bytes."""
    import torch
    rng = np.random.default_rng(47)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    img[..., 1] = np.maximum(img[..., 1], 90)
    prm = native.pp_wow()
    want = weng.postprocess_u8(img, prm)
    assert np.array_equal(want, pp.enhance_for_crops(img))
    x = torch.from_numpy(img).cuda()
    y = torch.empty_like(x)
    st = torch.cuda.current_stream().cuda_stream
    # taken while the histograms are being counted
    weng.pp_band_begin_dev(64, 64, prm, 0, st)
    weng.pp_band_hist_dev(x.data_ptr(), 0, 32, st)
    torch.cuda.synchronize()
    _TAKERS[taker](weng, img, prm)
    with pytest.raises(native.S2srError, match="took its scratch"):
        weng.pp_band_hist_dev(x.data_ptr(), 32, 64, st)
    with pytest.raises(native.S2srError, match="took its scratch"):
        weng.pp_band_lut_dev(st)
    assert np.array_equal(banded(weng, img, prm, [0, 32, 64], [0, 32, 64]), want)
    # taken between two finishing bands
    weng.pp_band_begin_dev(64, 64, prm, 0, st)
    weng.pp_band_hist_dev(x.data_ptr(), 0, 64, st)
    weng.pp_band_lut_dev(st)
    weng.pp_band_rows_dev(x.data_ptr(), 0, 32, y.data_ptr(), st)
    torch.cuda.synchronize()
    _TAKERS[taker](weng, img, prm)
    with pytest.raises(native.S2srError, match="took its scratch"):
        weng.pp_band_rows_dev(x.data_ptr(), 32, 64, y.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(banded(weng, img, prm, [0, 32, 64], [0, 32, 64]), want)


def test_gpu_against_cv2_golden(eng, golden_dir):
    """With tests/golden/g9_cv2_postprocess.npz present (tools/make_cv2_golden.py, run where cv2 is installed): the HIP
    post-process against OpenCV's own output of the reference's call chain, end to end, within 2 LSB per byte at >= 99 % of the
    bytes (the kernels are bit-exact against the oracle, which test_oracle_against_cv2_golden holds to cv2 stage by stage;
    composed, a 1-LSB difference in the blur input moves the sharpened value by up to its weight).  Skipped when absent."""
    f = golden_dir / "g9_cv2_postprocess.npz"
    if not f.exists():
        pytest.skip("no cv2 golden (run tools/make_cv2_golden.py where opencv-contrib-python>=4.8.0 is installed)")
    g = np.load(f)
    for name in sorted({k.split(".")[0] for k in g.files if k.endswith(".img")}):
        for tag, prm in (("wow", native.pp_wow()), ("farm", native.pp_farm())):
            got = eng.postprocess_u8(g[f"{name}.img"], prm)
            d = np.abs(got.astype(np.int16) - g[f"{name}.{tag}.final"].astype(np.int16))
            print(f"GPU vs cv2 {g['cv2_version']} {name}/{tag}: max |d| {int(d.max())}, identical {np.mean(d == 0):.5f}, within 2 LSB {np.mean(d <= 2):.5f}")
            assert np.mean(d <= 2) >= 0.99, (name, tag)
