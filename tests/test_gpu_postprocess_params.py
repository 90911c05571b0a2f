"""The post-process kernels at every parameter a caller can reach, not only the wow / farm sets of test_gpu_postprocess.py:
`s2sr_pp_params` is caller-supplied and the drop-ins `apply_unsharp_mask(img, strength, radius)` /
`enhance_local_contrast(img, clip_limit, grid_size)` pass their arguments straight into it.  Radii 1, 2, 6, 7, 8 take the generic
sharpen kernel (radii 3, 4, 5 have forms of their own), CLAHE grids other than 8 move the padding rule, the histogram split, the
neighbour clamp and the band path's tile-row arithmetic, clip limits 0 / tiny / huge take the no-clip, floor-to-1 and
nothing-clips branches.  Everything runs through the same entries (postprocess_u8, postprocess_batch_u8_dev, the pp_band_*_dev
sequence) against oracle/postprocess_ref.py, and the bar is the one of that module: BIT-EXACT, no tolerance anywhere."""
import numpy as np
import pytest

from doors import banded
from oracle import postprocess_ref as pp
from s2sr import native

pytestmark = pytest.mark.gpu

P = native.PPParams
MAX_KSIZE = 17          # postprocess.hip: 2 * MAXR + 1; sigma >= 2.75 asks OpenCV for more taps and is refused


def _ksize(sigma):
    return int(np.rint(6 * sigma + 1)) | 1


# sigma -> the OpenCV kernel width it must give (asserted in the tests, so that a list edit cannot silently move a case onto another
# kernel): 3, 5, 13, 15, 17 take the generic sharpen kernel, 7 the radius-3 form as a control
SIGMAS = {0.3: 3, 0.5: 5, 0.84: 7, 2.0: 13, 2.3: 15, 2.7: 17}
WEIGHTS = ((2.5, -1.5), (1.4, -0.4), (1.0, 0.0))
CLIPS = (2.5, 0.0, 0.01, 40.0, 1000.0)


@pytest.fixture(scope="module")
def eng():
    e = native.Engine(num_block=1)
    yield e
    e.close()


def _img(seed, H, W):
    img = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[..., 1] = np.maximum(img[..., 1], 90)        # green-heavy: the vegetation mask has pixels to work on
    return img


# 70 x 101: ragged in both dimensions, 3 x 4 tiles of the generic kernel; 64 x 64: divisible by every power-of-two grid; 33 x 32 and
# 32 x 33: one pixel past a 32-tile; 3 x 5 and 1 x 9: smaller than every radius, more than one reflection
IMGS = {f"{H}x{W}": _img(100 + i, H, W) for i, (H, W) in enumerate(((70, 101), (64, 64), (128, 192), (33, 32), (32, 33), (3, 5), (1, 9)))}


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not np.array_equal(got, want):
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        raise AssertionError(f"{what}: {int((d > 0).sum())} of {d.size} bytes differ, max {int(d.max())}")


def _unsharp_then(img, sigma, a, b, stages, gain=1.3):
    out = pp.unsharp(img, sigma, a, b)
    return pp.vegetation(out, gain) if stages & 4 else out


# ---- the generic sharpen kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", list(SIGMAS))
def test_unsharp_every_radius(eng, sigma):
    """Stage 2 alone and stages 2|4 at kernel widths 3..17 on every image: the generic kernel's horizontal and vertical passes, its
    reflect-then-clamp staging and the 32-pixel tile edges."""
    assert _ksize(sigma) == SIGMAS[sigma] <= MAX_KSIZE
    for name, img in IMGS.items():
        for a, b in WEIGHTS:
            for stages in (2, 6):
                got = eng.postprocess_u8(img, P(2.5, 8, sigma, a, b, 35, 85, 1.3, stages))
                _same(got, _unsharp_then(img, sigma, a, b, stages), f"sigma {sigma} {name} weights {a}/{b} stages {stages}")


@pytest.mark.parametrize("sigma", list(SIGMAS))
def test_unsharp_every_radius_batch(eng, sigma):
    """... through postprocess_batch_u8_dev: three 35 x 203 images (21315 bytes each: odd offsets), and a view that starts one
    byte into its buffer."""
    import torch
    assert _ksize(sigma) == SIGMAS[sigma]
    batch = np.stack([_img(200 + i, 35, 203) for i in range(3)])
    x = torch.from_numpy(batch).cuda()
    y = torch.empty_like(x)
    flat = torch.empty(1 + 35 * 203 * 3, dtype=torch.uint8, device="cuda")
    flat[1:] = x[1].reshape(-1)
    out = torch.empty(35 * 203 * 3, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for a, b in WEIGHTS:
        for stages in (2, 6):
            prm = P(2.5, 8, sigma, a, b, 35, 85, 1.3, stages)
            want = [_unsharp_then(batch[i], sigma, a, b, stages) for i in range(3)]
            eng.postprocess_batch_u8_dev(x.data_ptr(), 3, 35, 203, prm, y.data_ptr(), st)
            eng.postprocess_batch_u8_dev(flat.data_ptr() + 1, 1, 35, 203, prm, out.data_ptr(), st)
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            for i in range(3):
                _same(got[i], want[i], f"sigma {sigma} weights {a}/{b} stages {stages} image {i}")
            _same(out.cpu().numpy().reshape(35, 203, 3), want[1], f"sigma {sigma} weights {a}/{b} stages {stages} offset view")


@pytest.mark.parametrize("sigma", list(SIGMAS))
def test_unsharp_every_radius_banded(eng, sigma):
    """... through the banded sequence (the kernel's y_begin / y_end form): one-row bands, a band one row past a tile, an image
    smaller than the radius; in place, out of place, BGR bytes swapped on the way out.  Each equals the whole image and the oracle."""
    assert _ksize(sigma) == SIGMAS[sigma]
    for name, rc in (("70x101", [0, 1, 33, 34, 70]), ("3x5", [0, 1, 3])):
        img = IMGS[name]
        hc = [0, img.shape[0]]
        bgr = np.ascontiguousarray(img[:, :, ::-1])
        for a, b in WEIGHTS:
            for stages in (2, 6):
                prm = P(2.5, 8, sigma, a, b, 35, 85, 1.3, stages)
                what = f"sigma {sigma} {name} weights {a}/{b} stages {stages}"
                want = _unsharp_then(img, sigma, a, b, stages)
                _same(eng.postprocess_u8(img, prm), want, what + " whole")
                _same(banded(eng, img, prm, hc, rc), want, what + " banded")
                _same(banded(eng, img, prm, hc, rc, in_place=True), want, what + " banded in place")
                _same(banded(eng, bgr, prm, hc, rc, native.PP_ORDER_BGR | native.PP_ORDER_SWAP_OUT), want, what + " banded bgr in, rgb out")


# ---- CLAHE grids and clip limits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2, 3, 4, 7, 16, 64])
def test_clahe_every_grid_and_clip(eng, grid):
    """Stage 1: the two-dimension padding rule, the histogram split (grid 64: 4096 tiles, one workgroup each), the neighbour clamp
    (grid 1: every neighbour is the tile itself), tiles of 2 x 2 pixels; clip 0 (no clipping), 0.01 (floors to the `clip < 1 -> 1`
    branch at small tiles), 40 and 1000 (little or nothing clips)."""
    for name in ("70x101", "64x64", "128x192", "3x5", "1x9"):
        img = IMGS[name]
        for clip in CLIPS:
            got = eng.postprocess_u8(img, P(clip, grid, 1.0, 1.0, 0.0, 35, 85, 1.0, 1))
            _same(got, pp.local_contrast(img, clip, grid), f"grid {grid} clip {clip} {name}")


@pytest.mark.parametrize("grid", [1, 3, 16, 64])
def test_clahe_grids_banded(eng, grid):
    """The band path's "which tile rows does this band touch" arithmetic at one tile row, a non-power-of-two grid, tiles smaller
    than a band and 2 x 2-pixel tiles (70 x 101 pads to 128 x 128 at grid 64: the padding is wider than what one reflection
    reaches from the last rows).  Stage 1 alone, and all stages with a non-product blur so that the apply pass runs 6 rows ahead."""
    img = IMGS["70x101"]
    hc, rc = [0, 1, 2, 40, 69, 70], [0, 9, 70]
    for clip in CLIPS:
        for stages, prm in ((1, P(clip, grid, 1.0, 1.0, 0.0, 35, 85, 1.0, 1)), (7, P(clip, grid, 2.0, 2.2, -1.2, 30, 90, 1.5, 7))):
            what = f"grid {grid} clip {clip} stages {stages}"
            want = pp.postprocess(img, clip, grid, prm.blur_sigma, prm.w_img, prm.w_blur, prm.hue_lo, prm.hue_hi, prm.sat_gain, stages)
            _same(eng.postprocess_u8(img, prm), want, what + " whole")
            _same(banded(eng, img, prm, hc, rc), want, what + " banded")
            _same(banded(eng, img, prm, hc, rc, in_place=True), want, what + " banded in place")


def test_clahe_grid16_batch(eng):
    """Three images at grid 16: image i's LUTs start at i * grid * grid * 256."""
    import torch
    batch = np.stack([_img(300 + i, 70, 101) for i in range(3)])
    x = torch.from_numpy(batch).cuda()
    y = torch.empty_like(x)
    for clip in (2.5, 0.0):
        eng.postprocess_batch_u8_dev(x.data_ptr(), 3, 70, 101, P(clip, 16, 1.0, 1.0, 0.0, 35, 85, 1.0, 1), y.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        for i in range(3):
            _same(got[i], pp.local_contrast(batch[i], clip, 16), f"clip {clip} image {i}")


def _wow_still_right(eng):
    img = IMGS["64x64"]
    _same(eng.postprocess_u8(img, native.pp_wow()), pp.enhance_for_crops(img), "wow after a refusal")


def _no_run_open(eng, x):
    with pytest.raises(native.S2srError, match="no banded post-process open"):
        eng.pp_band_hist_dev(x.data_ptr(), 0, 1, 0)


@pytest.mark.parametrize("grid", [0, 65])
def test_grid_outside_1_to_64_is_refused(eng, grid):
    import torch
    img = IMGS["64x64"]
    x = torch.from_numpy(img).cuda()
    y = torch.empty_like(x)
    for stages in (1, 7):
        prm = P(2.5, grid, 1.2, 1.4, -0.4, 35, 85, 1.2, stages)
        with pytest.raises(native.S2srError):
            eng.postprocess_u8(img, prm)
        with pytest.raises(native.S2srError):
            eng.postprocess_batch_u8_dev(x.data_ptr(), 1, 64, 64, prm, y.data_ptr(), 0)
        with pytest.raises(native.S2srError):
            eng.pp_band_begin_dev(64, 64, prm, 0, 0)
        _no_run_open(eng, x)
    _wow_still_right(eng)


# ---- vegetation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 180), (-1, 180), (100, 20), (84, 86)])
def test_vegetation_hue_bounds_and_gains(eng, lo, hi):
    """Every (hue, sat) pair at v = 255 with masks that take every hue but 0, every hue, none, and hue 85 alone; gains that zero
    the saturation, keep it, saturate it and go negative (clipped to 0)."""
    h, s = np.meshgrid(np.arange(180), np.arange(256), indexing="ij")
    rgb = pp.hsv2rgb_u8(np.stack([h, s, np.full_like(h, 255)], -1).astype(np.uint8))
    for gain in (0.0, 1.0, 2.5, -1.0):
        got = eng.postprocess_u8(rgb, P(2.5, 8, 1.2, 1.4, -0.4, lo, hi, gain, 4))
        _same(got, pp.vegetation(rgb, gain, lo, hi), f"hue {lo}..{hi} gain {gain}")


# ---- stage masks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", [0, 3, 5, 6])
def test_stage_masks_whole_image(eng, stages):
    """The masks the whole-image entry never ran, at a parameter set that is neither wow's nor farm's."""
    for name in ("70x101", "128x192"):
        img = IMGS[name]
        got = eng.postprocess_u8(img, P(3.0, 4, 2.0, 2.2, -1.2, 30, 90, 1.5, stages))
        _same(got, pp.postprocess(img, 3.0, 4, 2.0, 2.2, -1.2, 30, 90, 1.5, stages), f"stages {stages} {name}")
        if stages == 0:
            _same(got, img, f"stages 0 {name} is the input")


# ---- the drop-in functions --------------------------------------------------------------------------------------------------
def test_farm_dropins_at_other_arguments():
    from app.farm_sr import apply_unsharp_mask, enhance_local_contrast
    img = IMGS["70x101"]
    _same(apply_unsharp_mask(img, 1.5, 2.0), pp.unsharp(img, 2.0, 2.5, -1.5), "apply_unsharp_mask(1.5, 2.0): ksize 13")
    _same(apply_unsharp_mask(img, 0.7, 0.5), pp.unsharp(img, 0.5, 1.7, -0.7), "apply_unsharp_mask(0.7, 0.5): ksize 5")
    _same(enhance_local_contrast(img, 4.0, 4), pp.local_contrast(img, 4.0, 4), "enhance_local_contrast(4.0, 4)")
    with pytest.raises(native.S2srError, match="blur_sigma must be > 0 and < 2.75"):
        apply_unsharp_mask(img, 1.5, 3.0)
    _same(apply_unsharp_mask(img, 1.5, 2.7), pp.unsharp(img, 2.7, 2.5, -1.5), "apply_unsharp_mask(1.5, 2.7) after the refusal")


# ---- the sigma limit --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weng():
    """a handle with weights: s2sr_enhance_job_u8 runs the net"""
    from s2sr.weights import synthetic_state_dict
    e = native.Engine(num_block=1)
    e.load_state_dict(synthetic_state_dict(1, seed=0))
    yield e
    e.close()


@pytest.mark.parametrize("sigma", [2.75, 3.0, float("inf"), 0.0, -1.0, float("nan")])
def test_sigma_the_device_cannot_compute_is_refused(weng, sigma):
    """OpenCV's kernel for sigma >= 2.75 is 19 taps or more, the device holds 17: no entry may answer with the bytes of a kernel
    cut short (sigma 3.0 used to come back as a 17-tap blur with return code 0).  Neither is there a kernel for sigma <= 0 or NaN
    (cv2.GaussianBlur((0, 0), sigma) raises).  After each refusal the handle works, and no banded run is left open."""
    import torch
    if sigma >= 2.75:
        assert _ksize(min(sigma, 1e6)) > MAX_KSIZE
    img = IMGS["64x64"]
    x = torch.from_numpy(img).cuda()
    y = torch.empty_like(x)
    st = torch.cuda.current_stream().cuda_stream
    for stages in (2, 7):
        prm = P(2.5, 8, sigma, 2.5, -1.5, 35, 85, 1.3, stages)
        with pytest.raises(native.S2srError, match="blur_sigma must be > 0 and < 2.75.*17 taps"):
            weng.postprocess_u8(img, prm)
        _wow_still_right(weng)
        with pytest.raises(native.S2srError, match="blur_sigma must be > 0 and < 2.75.*17 taps"):
            weng.postprocess_batch_u8_dev(x.data_ptr(), 1, 64, 64, prm, y.data_ptr(), st)
        _wow_still_right(weng)
        # a run that is open when another begin is refused does not survive it either
        weng.pp_band_begin_dev(64, 64, native.pp_wow(), 0, st)
        with pytest.raises(native.S2srError, match="blur_sigma must be > 0 and < 2.75.*17 taps"):
            weng.pp_band_begin_dev(64, 64, prm, 0, st)
        _no_run_open(weng, x)
        with pytest.raises(native.S2srError, match="no banded post-process open"):
            weng.pp_band_lut_dev(st)
        _same(banded(weng, img, native.pp_wow(), [0, 32, 64], [0, 32, 64]), pp.enhance_for_crops(img), "banded wow after a refusal")
        with pytest.raises(native.S2srError, match="blur_sigma must be > 0 and < 2.75.*17 taps"):
            weng.enhance_job_u8(img[:16, :16], prm)
        _wow_still_right(weng)
    # the stage is what is refused, not the field: without bit 1 the sigma is not looked at
    _same(weng.postprocess_u8(img, P(2.5, 8, sigma, 2.5, -1.5, 35, 85, 1.3, 5)),
          pp.vegetation(pp.local_contrast(img, 2.5, 8), 1.3), "stages 5 ignores the sigma")


def test_widest_sigma_computes_through_every_entry(weng):
    """sigma 2.7 (17 taps, the last one computed) through the four entries that refuse 2.75."""
    import torch
    assert _ksize(2.7) == MAX_KSIZE
    img = IMGS["64x64"]
    prm = P(2.5, 8, 2.7, 2.5, -1.5, 35, 85, 1.3, 2)
    want = pp.unsharp(img, 2.7, 2.5, -1.5)
    _same(weng.postprocess_u8(img, prm), want, "postprocess_u8")
    x = torch.from_numpy(img).cuda()
    y = torch.empty_like(x)
    weng.postprocess_batch_u8_dev(x.data_ptr(), 1, 64, 64, prm, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same(y.cpu().numpy(), want, "postprocess_batch_u8_dev")
    _same(banded(weng, img, prm, [0, 64], [0, 7, 64]), want, "banded")
    small = img[:16, :16]
    sr = weng.enhance_job_u8(small, None)
    _same(weng.enhance_job_u8(small, prm), pp.unsharp(sr, 2.7, 2.5, -1.5), "enhance_job_u8")


@pytest.mark.parametrize("a,b", [(2.0, 0.0), (2.2, -1.2)])
def test_one_tap_kernel_still_weighs(eng, a, b):
    """sigma 0.05: ksize 1, GaussianBlur returns the image and addWeighted(img, a, img, b) still runs.  With weights that sum to 1
    that is the image again; with (2.0, 0.0) it is twice the image, saturated (the kernel used to store the centre pixel
    unweighted)."""
    import torch
    assert _ksize(0.05) == 1
    for name in ("70x101", "3x5"):
        img = IMGS[name]
        H, W, _ = img.shape
        for stages in (2, 6):
            prm = P(2.5, 8, 0.05, a, b, 35, 85, 1.3, stages)
            want = _unsharp_then(img, 0.05, a, b, stages)
            if stages == 2:
                exact = np.clip(np.rint(img.astype(np.float32) * np.float32(a) + img.astype(np.float32) * np.float32(b)), 0, 255)
                assert np.array_equal(want, exact.astype(np.uint8))
            what = f"{name} weights {a}/{b} stages {stages}"
            _same(eng.postprocess_u8(img, prm), want, what)
            x = torch.from_numpy(img).cuda()
            y = torch.empty_like(x)
            eng.postprocess_batch_u8_dev(x.data_ptr(), 1, H, W, prm, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            _same(y.cpu().numpy(), want, what + " batch")
            _same(banded(eng, img, prm, [0, H], [0, 1, H], in_place=True), want, what + " banded")
