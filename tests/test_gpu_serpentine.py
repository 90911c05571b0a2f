"""Launch order: a conv launch that walks its patches back to front (ConvParams::dbg bit 0, tile -> ntiles - 1 - tile) writes exactly the
bytes of the front-to-back launch, kernel by kernel through the per-layer hooks and end to end through engines created with and
without the order (S2SR_SERPENTINE).

The shapes are the smallest at which the mapping can go wrong: more patches than the 256 workgroups with a ragged last round, so
the DMA cursor crosses a patch boundary inside a workgroup, the conv5 operand prefetch and the epilogue have to agree with it on the
mapped index, and some workgroups own one patch more than others.  Every comparison is np.array_equal: the patch index is mapped,
a patch's arithmetic and accumulation order are not.
"""
import numpy as np
import pytest
import torch

from s2sr import native
from s2sr.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

K14, K5, K5R, F14, F5 = (native.TRUNK_F16_CONV14, native.TRUNK_F16_CONV5, native.TRUNK_F16_CONV5_RRDB, native.TRUNK_F8_CONV14,
                         native.TRUNK_F8_CONV5)


@pytest.fixture(scope="module")
def eng():
    e = native.Engine(num_block=1, precision=native.PREC_F16_HP)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng8():
    e = native.Engine(num_block=1, precision=native.PREC_FP8)
    yield e
    e.close()


def _h(a):
    return a.astype(np.float16).astype(np.float32)


def _rand(rng, N, Cin, Cout, H, W):
    x = _h(rng.standard_normal((N, Cin, H, W)).astype(np.float32))
    w = _h((rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32))
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    return x, w, b


def _conv5_operands(eng, rng, N, H, W):
    x, w, b = _rand(rng, N, 192, 64, H, W)
    le = eng.debug_config()["lo_exp"]
    lo = (rng.integers(-7, 8, size=(N, 64, H, W)) * 2.0 ** (-4 - le)).astype(np.float32)
    skip = _h(rng.standard_normal((N, 64, H, W)).astype(np.float32))
    return x, w, b, lo, skip


@pytest.fixture(scope="module")
def conv5_case(eng):
    """N=5, 128x256: 320 patches of 16x32, with the forward results of the generic form (shared, never modified)."""
    x, w, b, lo, skip = _conv5_operands(eng, np.random.default_rng(51), 5, 128, 256)
    fwd = eng.debug_conv_trunk(K5, x, w, b, lo=lo, form=1)
    fwd_rr = eng.debug_conv_trunk(K5R, x, w, b, lo=lo, skip=skip, form=1)
    assert np.abs(fwd).max() > 0 and not np.array_equal(fwd, fwd_rr)
    return x, w, b, lo, skip, fwd, fwd_rr


# 32x32 patches (form 2, and its whole-patch form 6): N=9, 128x256 -> 288 patches; 16x32 patches (form 1, whole-patch 7): N=5 -> 320
@pytest.mark.parametrize("form,N", [(2, 9), (6, 9), (1, 5), (7, 5)])
def test_f16_conv14_backwards_same_bytes(eng, form, N):
    x, w, b = _rand(np.random.default_rng(140 + form), N, 160, 32, 128, 256)
    fwd = eng.debug_conv_trunk(K14, x, w, b, form=form)
    assert np.abs(fwd).max() > 0
    assert np.array_equal(eng.debug_conv_trunk(K14, x, w, b, form=form, backwards=True), fwd)


def test_f16_conv5_backwards_same_bytes(eng, conv5_case):
    """conv5 and the conv5 that closes an RRDB on the 16x32 form: backwards gives the bytes of forwards."""
    x, w, b, lo, skip, fwd, fwd_rr = conv5_case
    assert np.array_equal(eng.debug_conv_trunk(K5, x, w, b, lo=lo, form=1, backwards=True), fwd)
    assert np.array_equal(eng.debug_conv_trunk(K5R, x, w, b, lo=lo, skip=skip, form=1, backwards=True), fwd_rr)


def test_f16_ragged_launch_backwards(eng):
    """6 x 96x190, ragged in x (190 = 5 x 32 + 30): the generic forms walk it backwards to the same bytes -- 216 patches of 16x32
    (form 1: one ragged round), 432 of 8x32 (form 5: two rounds).  (conv5 has no whole-patch form that would have to refuse
    this launch: measured and not kept)"""
    N, H, W = 6, 96, 190
    rng = np.random.default_rng(96190)
    x, w, b, lo, skip = _conv5_operands(eng, rng, N, H, W)
    for form in (1, 5):
        assert np.array_equal(eng.debug_conv_trunk(K5, x, w, b, lo=lo, form=form, backwards=True), eng.debug_conv_trunk(K5, x, w, b, lo=lo, form=form))
        assert np.array_equal(eng.debug_conv_trunk(K5R, x, w, b, lo=lo, skip=skip, form=form, backwards=True),
                              eng.debug_conv_trunk(K5R, x, w, b, lo=lo, skip=skip, form=form))
    x, w, b = _rand(rng, N, 160, 32, H, W)
    assert np.array_equal(eng.debug_conv_trunk(K14, x, w, b, form=1, backwards=True), eng.debug_conv_trunk(K14, x, w, b, form=1))
    with pytest.raises(native.S2srError):       # conv1-4's whole-patch form refuses a ragged launch in either direction
        eng.debug_conv_trunk(K14, x, w, b, form=7, backwards=True)


def test_fp8_trunk_backwards_same_bytes(eng8):
    """The fp8 conv1-4 (N=9, 128x256) and conv5 (N=5) kernels; operands on the e4m3 grid of the handle's scales."""
    cfg = eng8.debug_config()
    rng = np.random.default_rng(8)

    def grid(shape, exp):       # representable e4m3 values at scale 2^exp
        return (rng.integers(-8, 9, size=shape) * 2.0 ** (-exp)).astype(np.float32)

    N, H, W = 9, 128, 256
    x = np.concatenate([grid((N, 64, H, W), cfg["fp8_x_exp"]), grid((N, 96, H, W), cfg["fp8_g_exp"])], axis=1)
    _, w, b = _rand(rng, 1, 160, 32, 1, 1)
    fwd = eng8.debug_conv_trunk(F14, x, w, b)
    assert np.abs(fwd).max() > 0
    assert np.array_equal(eng8.debug_conv_trunk(F14, x, w, b, backwards=True), fwd)
    N = 5
    x = np.concatenate([_h(grid((N, 64, H, W), cfg["fp8_x_exp"])), grid((N, 128, H, W), cfg["fp8_g_exp"])], axis=1)
    _, w, b = _rand(rng, 1, 192, 64, 1, 1)
    y, aux = eng8.debug_conv_trunk(F5, x, w, b)
    yb, auxb = eng8.debug_conv_trunk(F5, x, w, b, backwards=True)
    assert np.abs(y).max() > 0
    assert np.array_equal(yb, y) and np.array_equal(auxb, aux)


@pytest.mark.parametrize("upsample", [False, True])
def test_conv3x3_backwards_same_bytes(eng, upsample):
    """conv3x3.hip's loader and epilogue through s2sr_debug_conv (16x32 patches, 256 workgroups): 7 images of 96x200 output pixels
    = 6 x 7 x 7 = 294 patches, ragged in x; with nearest-2x on load from 48x100 sources."""
    rng = np.random.default_rng(33 + upsample)
    s = 2 if upsample else 1
    x, w, b = _rand(rng, 7, 32, 64, 96 // s, 200 // s)
    fwd = eng.debug_conv(x, w, b, upsample=upsample, act=True)
    assert np.abs(fwd).max() > 0
    assert np.array_equal(eng.debug_conv(x, w, b, upsample=upsample, act=True, backwards=True), fwd)


# ---- end to end: engines that differ in the launch order only

NB = 6
# turn masks (engine_internal.h serp_bit): nothing, the shipped default, and single kinds that the default may not exercise alone --
# conv_hr (the split-operand conv3x3 form) and both row-parity launches of the sub-pixel up-convs
ORDERS = {"front_to_back": "0", "default": None, "hr_only": "0x80", "up_only": "0x10060"}


@pytest.fixture(scope="module")
def engines():
    mp = pytest.MonkeyPatch()
    sd = synthetic_state_dict(NB, seed=0)
    es = {}
    try:
        for name, val in ORDERS.items():
            if val is None:
                mp.delenv("S2SR_SERPENTINE", raising=False)
            else:
                mp.setenv("S2SR_SERPENTINE", val)
            e = native.Engine(num_block=NB, precision=native.PREC_F16_HP)
            e.load_state_dict(sd)
            es[name] = e
    finally:
        mp.undo()
    yield es
    for e in es.values():
        e.close()


def test_order_switch_took(engines):
    masks = {k: e.debug_config()["serpentine"] for k, e in engines.items()}
    assert masks["front_to_back"] == 0 and masks["hr_only"] == 0x80 and masks["up_only"] == 0x10060, masks
    assert masks["default"] != 0, "the shipped order turns launches round; S2SR_SERPENTINE=0 is the off switch"


def test_batch_same_bytes_in_every_order(engines):
    """20 tiles of 128x128, launch groups of 16 and 4 images: 320 conv1-4 patches of 32x32 over the job, 512 conv5 patches of 16x32 in the
    16-image launch, thousands in the HR convs: more than one round everywhere."""
    tiles = np.random.default_rng(20).integers(0, 256, size=(20, 128, 128, 3), dtype=np.uint8)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    x = torch.from_numpy(tiles).to(dev)
    outs = {}
    for name, e in engines.items():
        y = torch.zeros((20, 512, 512, 3), dtype=torch.uint8, device=dev)
        e.forward_batch_u8_dev(x.data_ptr(), 20, 128, 128, y.data_ptr(), st)
        torch.cuda.synchronize()
        outs[name] = y.cpu().numpy()
    ref = outs["front_to_back"]
    assert ref.std() > 1.0
    for name, got in outs.items():
        assert np.array_equal(got, ref), name


def test_mosaic_image_same_bytes_in_every_order(engines):
    """One 300x300 image through enhance_u8 with the 256 / 10 window plan: the mosaic path of the same schedule."""
    img = np.random.default_rng(300).integers(0, 256, size=(300, 300, 3), dtype=np.uint8)
    ref = np.array(engines["front_to_back"].enhance_u8(img, tile=256, pad=10))
    assert ref.shape == (1200, 1200, 3) and ref.std() > 1.0
    for name, e in engines.items():
        assert np.array_equal(np.array(e.enhance_u8(img, tile=256, pad=10)), ref), name
