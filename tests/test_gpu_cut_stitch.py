"""The multi-GPU building blocks alone, through torch device tensors: s2sr_cut_windows_u8_dev against numpy slices of a coded
image, s2sr_stitch_windows_u8_dev / s2sr_stitch_rows_u8_dev against the reference's paste loop (probe_model.paste_replay) on
window-coded tiles.  No forward runs here: tests/test_gpu_net.py's test_cut_forward_stitch_equals_enhance compares these entries
with s2sr_enhance_u8, which runs the same kernels; tests/test_probe_cpu.py shows that these inputs tell a wrong paste from the
right one."""
import numpy as np
import pytest
import torch

import gpu_engines
import probe_model as pm
from oracle import rrdbnet_ref as ref
from s2sr import native

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module", params=[4, 2])
def engine(request):
    with pytest.MonkeyPatch.context() as mp:
        e = gpu_engines.fresh(mp, {}, 1, native.PREC_F16_HP, scale=request.param, sd=pm.probe_state_dict(1, scale=request.param))
    yield e
    e.close()


def _padded(img, scale):
    return pm.reflect_even(img) if scale == 2 else img


def _same(got, want, what):
    d = pm.first_difference(got, want)
    assert not d, f"{what}: {d}"


def test_cut_windows_equal_numpy_slices(engine):
    S = engine.scale
    geos = pm.STITCH_GEOS + [(17, 53, 16, 2), (19, 60, 16, 2), (3, 40, 16, 2)]       # + duplicate window rows, H < win, a 3-pixel side
    for H, W, t, p in geos:
        if S == 2 and min(H, W) < 2:
            continue
        img = pm.coded(H, W)
        src = _padded(img, S)
        plan = native.plan_tiles(src.shape[0], src.shape[1], t, p, S)
        rplan = ref.tile_plan(src.shape[0], src.shape[1], t, p, S)
        assert [(w.y1, w.y2, w.x1, w.x2) for w in plan] == [r[0] for r in rplan]
        want = np.stack(pm.plan_windows_of(src, rplan))
        T, wh, ww, _ = want.shape
        d_img = torch.from_numpy(img).cuda()
        n = T * wh * ww * 3
        ranges = [(0, T)] + ([(0, 1), (1, T - 1), (T // 2, T - T // 2), (T - 1, 1)] if T > 1 else [])
        for first, count in ranges:
            buf = torch.full((n + 1,), SENTINEL, dtype=torch.uint8, device="cuda")
            engine.cut_windows_u8_dev(d_img.data_ptr(), H, W, t, p, first, count, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            m = count * wh * ww * 3
            _same(got[:m].reshape(count, wh, ww, 3), want[first:first + count], (S, H, W, t, p, first, count))
            assert (got[m:] == SENTINEL).all(), (S, H, W, t, p, first, count, "bytes behind the last window were written")
        with pytest.raises(native.S2srError, match="window range exceeds the plan"):
            engine.cut_windows_u8_dev(d_img.data_ptr(), H, W, t, p, 1, T, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)


def _bands(OH, seed):
    """Band splits at arbitrary rows: one-row bands, boundaries that are no multiple of 4, the rest in uneven pieces."""
    rng = np.random.default_rng(seed)
    cuts = {0, OH, 1, 2, min(OH, 7), OH - 1, OH - 3}
    cuts |= set(int(v) for v in rng.integers(1, OH, size=5))
    cuts = sorted(c for c in cuts if 0 <= c <= OH)
    return list(zip(cuts[:-1], cuts[1:]))


def test_stitch_equals_the_reference_paste(engine):
    """Six geometries in turn, twice (the four-entry map LRU recycles): the whole paste, and the paste band by band into a
    sentinel-filled image -- every band writes its own rows and no others."""
    S = engine.scale
    st = lambda: torch.cuda.current_stream().cuda_stream
    cases = []
    for H, W, t, p in pm.STITCH_GEOS:
        PH, PW = (H + H % 2, W + W % 2) if S == 2 else (H, W)
        plan = ref.tile_plan(PH, PW, t, p, S)
        (y1, y2, x1, x2) = plan[0][0]
        tiles = pm.window_tiles(len(plan), S * (y2 - y1), S * (x2 - x1), seed=H * 1000 + W)
        cases.append((H, W, t, p, torch.from_numpy(tiles).cuda(), pm.paste_replay(tiles, plan)[:S * H, :S * W]))
    for rnd in range(2):
        for H, W, t, p, d_tiles, want in cases:
            OH, OW = S * H, S * W
            out = torch.full((OH * OW * 3 + 1,), SENTINEL, dtype=torch.uint8, device="cuda")
            engine.stitch_windows_u8_dev(d_tiles.data_ptr(), H, W, t, p, out.data_ptr(), st())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            _same(got[:-1].reshape(OH, OW, 3), want, (S, H, W, t, p, "whole", rnd))
            assert got[-1] == SENTINEL
            # bands, in an order that is not top to bottom; the image keeps the sentinel wherever no band has been yet
            bands = _bands(OH, H + W + rnd)
            order = np.random.default_rng(rnd).permutation(len(bands))
            out.fill_(SENTINEL)
            model = np.full((OH, OW, 3), SENTINEL, np.uint8)
            for k, b in enumerate(order):
                oy0, oy1 = bands[b]
                engine.stitch_rows_u8_dev(d_tiles.data_ptr(), H, W, t, p, oy0, oy1, out.data_ptr(), st())
                model[oy0:oy1] = want[oy0:oy1]
                if k in (0, len(order) // 2):             # (every intermediate state would be a copy per band)
                    torch.cuda.synchronize()
                    _same(out.cpu().numpy()[:-1].reshape(OH, OW, 3), model, (S, H, W, t, p, "band", oy0, oy1, rnd))
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            _same(got[:-1].reshape(OH, OW, 3), want, (S, H, W, t, p, "bands", rnd))
            assert got[-1] == SENTINEL
