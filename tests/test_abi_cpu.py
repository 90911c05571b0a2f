"""CPU-side checks of the native boundary: the library loads, exports every symbol that
include/s2sr.h declares, the pure host function s2sr_plan_tiles matches the reference's
window plans, and the product path fails loudly without a GPU (no fallback)."""
import re
from pathlib import Path

import numpy as np
import pytest

from s2sr import native

REPO = Path(__file__).resolve().parent.parent


def test_library_exports_every_declared_symbol():
    lib = native.load_library()
    header = (REPO / "include" / "s2sr.h").read_text()
    declared = set(re.findall(r"\b(s2sr_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/s2sr.h but not exported"
    assert declared == set(native.EXPORTED_SYMBOLS)
    assert b"gfx950" in lib.s2sr_version()


def test_gpu_tests_clear_exactly_the_switches_s2sr_create_reads():
    """tests/gpu_engines.py creates default engines with SWITCHES cleared: a switch s2sr_create reads and the list lacks would
    leak a test's environment into a cached handle; a name the list has and nothing reads is rot."""
    import gpu_engines

    src = (REPO / "sentinel2-super-resolution-poc_amd" / "csrc" / "engine.hip").read_text()
    body = src[src.index("int s2sr_create("):]
    body = body[:body.index("\n}\n")]                       # up to the function's closing brace in column 0
    read = re.findall(r'getenv\("(S2SR_[A-Z0-9_]+)"\)', body)
    assert read, "no getenv call parsed in s2sr_create"
    assert len(read) == len(set(read)) and len(gpu_engines.SWITCHES) == len(set(gpu_engines.SWITCHES))
    assert set(read) == set(gpu_engines.SWITCHES)


def test_expected_blob_size():
    lib = native.load_library()
    assert lib.s2sr_expected_blob_floats(23) == 16_697_987
    from s2sr.weights import num_params, num_params_compact
    assert lib.s2sr_expected_blob_floats(6) == num_params(6)
    # the layer table behind the sizes (csrc/engine.hip layer_table) against the state dicts' own arithmetic
    for nb in (1, 6, 23):
        for scale in (2, 4):
            assert native.expected_blob_floats_cfg(nb, scale) == num_params(nb, scale)
    for n in (16, 32):
        assert native.expected_blob_floats_cfg(n, 4, "compact") == num_params_compact(n)
    # ... and the configurations it refuses
    assert native.expected_blob_floats_cfg(8, 4, "compact") == 0
    assert native.expected_blob_floats_cfg(6, 3) == 0 and native.expected_blob_floats_cfg(16, 3, "compact") == 0
    for arch in (native.ARCH_RRDB, native.ARCH_COMPACT):
        cfg = native._Config(16, 32, 32, 4, native.PREC_F16, 0, 0, arch)      # num_feat 32
        assert lib.s2sr_expected_blob_floats_cfg(cfg) == 0


def test_plan_tiles_matches_reference_golden(golden_dir):
    g = np.load(golden_dir / "g6_tile_plans.npz")
    for key in g.files:
        h, w = map(int, key.split("x"))
        ts, tp = (16, 2) if (h, w) == (37, 45) else (256, 10)
        if h * w <= ts * ts * 4:
            continue   # whole-image branch: no plan
        wins = native.plan_tiles(h, w, ts, tp, 4)
        rects = np.array([(q.y1, q.y2, q.x1, q.x2) for q in wins], dtype=np.int32)
        assert np.array_equal(rects, g[key]), key


def test_plan_tiles_matches_oracle_everywhere():
    from oracle import rrdbnet_ref as ref
    rng = np.random.default_rng(5)
    cases = [(513, 512), (530, 600), (1024, 1024), (200, 1400), (276, 1000), (4096, 4096), (257, 1025)]
    cases += [(int(a), int(b)) for a, b in rng.integers(1, 1500, size=(40, 2))]
    for (h, w) in cases:
        for ts, tp in ((256, 10), (16, 2), (64, 0), (100, 7)):
            wins = native.plan_tiles(h, w, ts, tp, 4)
            exp = ref.tile_plan(h, w, ts, tp, 4)
            got = [((q.y1, q.y2, q.x1, q.x2), (q.crop_top, q.crop_bottom, q.crop_left, q.crop_right),
                    (q.oy1, q.oy2, q.ox1, q.ox2)) for q in wins]
            assert got == exp, (h, w, ts, tp)


def test_no_gpu_means_loud_failure():
    if native.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(native.S2srError):
        native.Engine(num_block=1)


def test_e4m3_encoder_matches_torch():
    """The weight packer's fp8 encoder (OCP e4m3fn, RNE, saturating) against torch's float8_e4m3fn
    on a sweep that covers subnormals, ties and every binade up to the finite maximum."""
    import torch

    lib = native.load_library()
    rng = np.random.default_rng(0)
    vals = np.concatenate([
        np.array([0.0, -0.0, 2.0 ** -10, 2.0 ** -9, 1.5 * 2.0 ** -9, 2.0 ** -6, 1.0625, 1.1875, 447.9, 448.0], np.float32),
        (rng.standard_normal(4000) * np.exp2(rng.integers(-12, 9, 4000))).astype(np.float32),
        np.ldexp(np.arange(8, 17, dtype=np.float32) + 0.5, -3),           # exact ties between neighbours
    ])
    vals = vals[np.abs(vals) <= 448.0]
    want = torch.from_numpy(vals).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = np.array([lib.s2sr_debug_f32_to_e4m3(float(v)) for v in vals], np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(vals[i]), hex(got[i]), hex(want[i])) for i in bad[:5]]
    assert lib.s2sr_debug_f32_to_e4m3(1e9) == 0x7E and lib.s2sr_debug_f32_to_e4m3(-1e9) == 0xFE   # saturate, never NaN
    assert lib.s2sr_debug_f32_to_e4m3(float("nan")) == 0x7F


def _e4m3_decode(b: np.ndarray) -> np.ndarray:
    """OCP e4m3fn bytes -> float (bias 7, subnormals, no infinities, 0x7f/0xff = NaN)."""
    b = b.astype(np.int32)
    sign = np.where(b & 0x80, -1.0, 1.0)
    e = (b >> 3) & 0xF
    m = b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10))
    v = np.where((b & 0x7F) == 0x7F, np.nan, v)
    return sign * v


def test_fp8_trunk_weight_packer_host():
    """pack_conv_weights_f8 (S2SR_PREC_FP8), host side: per-output-channel power-of-two scales put each row's maximum
    into e4m3's top binade, the packed bytes decode back to the weights within e4m3's half-ulp, odd plane counts get an
    all-zero phantom plane, and the byte order is [plane][tap][ct][16-B half][cout row][16 channels]."""
    lib = native.load_library()
    rng = np.random.default_rng(5)
    for cin, cout in ((64, 32), (96, 32), (160, 32), (192, 64)):
        w = (rng.standard_normal((cout, cin, 3, 3)) * rng.uniform(1e-3, 2.0, size=(cout, 1, 1, 1))).astype(np.float32)
        w[3, 5, 1, 1] = 0.0
        nb = lib.s2sr_debug_pack_f8_bytes(cin, cout)
        nreal, ct = cin // 32, (cout + 31) // 32
        npad = (nreal + 1) & ~1
        assert nb == npad * 9 * ct * 1024
        out = np.zeros(nb, np.uint8)
        ws = np.zeros(64, np.int32)
        assert lib.s2sr_debug_pack_f8(w.ctypes.data, cin, cout, out.ctypes.data, ws.ctypes.data) == 0
        k = 127 - ws[:cout]
        m = np.abs(w).reshape(cout, -1).max(axis=1)
        top = m * 2.0 ** k
        assert np.all((top >= 224) & (top < 448)), (top.min(), top.max())
        assert np.all(ws[cout:] == 127)
        dec = _e4m3_decode(out).reshape(npad, 9, ct, 2, 32, 16)
        assert not np.isnan(dec).any()
        # [plane][tap][ct][h16][row][j] -> w[co = ct*32 + row][ci = 32*plane + 16*h16 + j][tap]
        got = dec.transpose(2, 4, 0, 3, 5, 1).reshape(ct * 32, npad * 32, 9)[:cout]
        if npad > nreal:
            assert np.all(got[:, nreal * 32:] == 0) and np.all(out.reshape(npad, -1)[nreal:] == 0)
        scaled = w.reshape(cout, cin, 9) * (2.0 ** k)[:, None, None]
        err = np.abs(got[:, :cin] - scaled)
        # half an ulp of e4m3 at the value's binade (3 mantissa bits), 2^-10 in the subnormal range
        ulp = np.maximum(2.0 ** (np.floor(np.log2(np.maximum(np.abs(scaled), 2.0 ** -6))) - 3), 2.0 ** -9)
        assert np.all(err <= ulp / 2 + 1e-12)
        assert got[3, 5, 4] == 0


def test_hidden_asm_loads_are_not_touched_before_their_wait(tmp_path):
    """The conv kernels' residual loads are inline asm (invisible to hipcc's waitcnt pass); tools/check_asm_loads.py reads
    the device assembly and fails on any instruction that touches such a load's destination registers before the wait that
    covers it -- the pattern behind r01's faulting 4-wave variant -- and (r03) on any non-MFMA read of an inline-asm MFMA's
    destination inside the XDL-write -> VALU-read distance (passes + 3 wait states; hipcc pads nothing around an asm MFMA and
    had hoisted accumulator reads above the epilogue's s_nop pair).  Compiles the conv sources to assembly (~1.5 min)."""
    import os
    import subprocess
    import sys
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not Path(hipcc).exists():
        pytest.skip("no hipcc")
    csrc = REPO / "sentinel2-super-resolution-poc_amd" / "csrc"
    for src in ("conv_trunk.hip", "conv3x3.hip"):
        asm = tmp_path / (src + ".s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", str(csrc / src), "-o", str(asm)], check=True, stderr=subprocess.DEVNULL)
        # --cfg: + the control-flow rule (every path from a hidden load to its first vmcnt wait; test below)
        r = subprocess.run([sys.executable, str(REPO / "tools" / "check_asm_loads.py"), "--cfg", str(asm)], capture_output=True, text=True)
        assert r.returncode == 0 and "0 hazard(s)" in r.stdout, r.stdout[-2000:]
        if src == "conv_trunk.hip":      # the check has something to check (conv3x3.hip has no hidden loads left)
            assert asm.read_text().count("global_load_dwordx2 a[") + asm.read_text().count("global_load_dwordx4 a[") > 0


def test_hidden_asm_load_before_fp8_loader_branch_is_caught(tmp_path):
    """The guard for r04's GPU fault (profiles/r04_latency_anatomy.txt section 3: inline-asm bias requests issued in front of a
    loader wave's role branch; on the loader's side their destination registers were dead, the compiler handed them to DMA
    offsets, the landing loads overwrote those -- an aborted GPU test).  tools/check_asm_loads.py --cfg follows every path of the
    control-flow graph from each hidden load to the first vmcnt wait on that path and reports any touch of the destination on the
    way; no counting, hence no false positives from infeasible paths.  Shown here to (a) pass on conv_trunk.hip as it is and (b)
    FIRE on r04's placement, rebuilt in a scratch copy in the shipped loader-wave form (conv_trunk_f8's conv1-4 kernels): a hidden
    request planted in front of the marked role branch and consumed on the compute side behind a vmcnt wait."""
    import os
    import shutil
    import subprocess
    import sys
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not Path(hipcc).exists():
        pytest.skip("no hipcc")
    csrc = REPO / "sentinel2-super-resolution-poc_amd" / "csrc"
    work = tmp_path / "pkg" / "csrc"
    work.mkdir(parents=True)
    (tmp_path / "include").mkdir()
    shutil.copy(REPO / "include" / "s2sr.h", tmp_path / "include" / "s2sr.h")
    shutil.copy(csrc / "s2sr_internal.h", work / "s2sr_internal.h")
    shutil.copy(csrc / "conv_forms.h", work / "conv_forms.h")       # s2sr_internal.h includes it
    src = (csrc / "conv_trunk.hip").read_text()
    role = "    // ---- the loader wave (PROD): the whole workgroup's DMA schedule, one barrier per pair-step like everybody else   [role-branch]"
    compute = "    // ---- fragment addresses: per-lane base + immediate.  b0 / b1 = logical 16-B halves 0 / 1 of pixel (row, pcol + dx)"
    assert src.count(role) == 1 and src.count(compute) == 1 and src.index(role) < src.index(compute)
    request = ("    // [hidden-request begin]\n"
               "    const f32x4 probe = asm_load16v((const char*)(p.bias + (tid & 31)));\n"
               "    // [hidden-request end]\n")
    land = ("    asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n"
            "    asm volatile(\"\" ::\"v\"(probe));\n")
    old = src.replace(role, request + role).replace(compute, land + compute)

    def hazards(text, name):
        (work / "conv_trunk.hip").write_text(text)
        asm = tmp_path / (name + ".s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S",
                        "--cuda-device-only", str(work / "conv_trunk.hip"), "-o", str(asm)], check=True, stderr=subprocess.DEVNULL)
        r = subprocess.run([sys.executable, str(REPO / "tools" / "check_asm_loads.py"), "--cfg", str(asm)], capture_output=True, text=True)
        return r.returncode, r.stdout

    rc, out = hazards(src, "head")
    assert rc == 0 and "0 hazard(s)" in out, out[-2000:]
    rc, out = hazards(old, "r04_placement")
    print(out[-3000:])
    assert rc == 1 and "with no vmcnt wait in between" in out, out[-2000:]
    # ... in the loader-wave form (conv_trunk_f8<1, 4, 6, EPI_LRELU, NPL, PROD = 1>), nowhere else
    lines = [l for l in out.splitlines() if "touches" in l]
    assert lines and all(re.search(r"conv_trunk_f8ILi1ELi4ELi6ELi0ELi[04]ELi1EE", l) for l in lines), out[-2000:]


def test_enhance_chunk_plan_properties():
    """The chunk plan of a tiled s2sr_enhance_u8 (engine_aoi.hip plan_chunk_sizes through s2sr_debug_plan_chunks; host arithmetic,
    no device): every row unit is covered once, no chunk exceeds the workspace limit, the last chunk (whose band copy is exposed)
    is small, the middle piece is at most 5x the last, and the plan is the one the measurements
    were made with -- 4096x4096 at 256/10 (16 row units of 16 windows, 4x4 mosaics of 1225 patches, 256 workgroups) goes as
    10 + 5 + 1 (whole workgroup rounds: 48 + 24 + 5 of 76.6), 2048x2048 (4 units of 2 rows) as 3 + 1."""
    from s2sr import native
    assert native.plan_chunks(16, 16, 16, 16, 1225, 256) == [10, 5, 1]
    assert native.plan_chunks(4, 4, 16, 16, 1225, 256) == [3, 1]
    assert native.plan_chunks(1, 16, 16, 16, 1225, 256) == [1]
    assert native.plan_chunks(0, 16, 16, 16, 1225, 256) == []
    rng = np.random.default_rng(5)
    for _ in range(300):
        units = int(rng.integers(1, 200)); u_max = int(rng.integers(1, 40)); uw = int(rng.integers(1, 64))
        per = int(rng.choice([1, 4, 8, 16, 64])); pimg = int(rng.integers(1, 5000)); ncu = int(rng.choice([64, 256, 304]))
        sz = native.plan_chunks(units, u_max, uw, per, pimg, ncu)
        assert sum(sz) == units and all(1 <= u <= u_max for u in sz), (units, u_max, sz)
        assert sz[-1] <= 3
        if len(sz) >= 2:
            assert sz[-2] <= 5 * sz[-1] or sz[-2] == u_max or len(sz) == 2   # the middle piece is bounded by 5x the last (or it is a front piece)
        # front pieces are as large as the workspace allows: at most one of them is not full
        front = sz[:-2] if len(sz) > 2 else []
        assert sum(1 for u in front if u != u_max) <= 1


# H, W of the planned image, tile, pad, scale, tiled -- and what the reference's plan does there
WINDOW_JOBS = [
    (34, 36, 16, 2, 4, True),        # the last two window rows and the last two window columns coincide
    (34, 45, 16, 2, 4, True),        # rows coincide, columns do not
    (37, 35, 16, 2, 4, True),        # columns coincide, rows do not
    (37, 45, 16, 2, 4, True),        # nothing coincides (the golden size)
    (100, 90, 16, 2, 4, True),       # 7 x 6 planned -> 6 x 6 distinct
    (53, 200, 16, 3, 4, True),       # 4 x 13 -> 3 x 13
    (513, 512, 256, 10, 4, True),    # window rows 1 and 2 coincide
    (38, 46, 16, 2, 2, True),        # a 37 x 45 image at scale 2, padded to even sizes
    (28, 36, 16, 2, 4, False),       # untiled: the image is its own window
]


@pytest.mark.parametrize("H,W,ts,tp,scale,tiled", WINDOW_JOBS)
def test_window_job_equals_the_references_paste(H, W, ts, tp, scale, tiled):
    """The window job both enhance doors run (engine_aoi.hip plan_window_job through s2sr_debug_plan_windows; host arithmetic, no
    device) against the reference's paste loop replayed in numpy: in plan order every window writes (its origin, the row inside
    its output, the column inside its output) into its paste rectangle, later windows overwriting earlier ones.  The job forwards
    each distinct rectangle once, so its maps must name, for every output pixel, a window with that origin and those offsets."""
    from oracle import rrdbnet_ref as ref
    plan = ref.tile_plan(H, W, ts, tp, scale) if tiled else [((0, H, 0, W), (0, 0, 0, 0), (0, scale * H, 0, scale * W))]
    big = 1 << 20
    origin = np.full((scale * H, scale * W), -1, np.int64)
    row, col = origin.copy(), origin.copy()
    for (y1, y2, x1, x2), (top, _, left, _), (oy1, oy2, ox1, ox2) in plan:
        origin[oy1:oy2, ox1:ox2] = y1 * big + x1
        row[oy1:oy2, ox1:ox2] = (np.arange(oy1, oy2) - oy1 + top)[:, None]
        col[oy1:oy2, ox1:ox2] = (np.arange(ox1, ox2) - ox1 + left)[None, :]
    assert origin.min() >= 0                                        # the reference's plan covers the image
    nx, ny, wh, ww, rects, rm, cm = native.plan_windows(H, W, ts, tp, scale, tiled)
    assert rm.shape == (scale * H, 2) and cm.shape == (scale * W, 2) and rm.min() >= 0 and cm.min() >= 0
    distinct = {p[0] for p in plan}
    assert nx * ny == len(distinct)
    if tiled:
        assert rects.shape == (nx * ny, 4) and len({tuple(r) for r in rects.tolist()}) == nx * ny
        assert np.all(rects[:, 1] - rects[:, 0] == wh) and np.all(rects[:, 3] - rects[:, 2] == ww)
        assert {tuple(r) for r in rects.tolist()} == distinct
    else:
        assert rects.shape == (0, 4) and (nx, ny, wh, ww) == (1, 1, H, W)
        rects = np.array([[0, H, 0, W]], np.int32)
    assert rm[:, 0].max() < ny and cm[:, 0].max() < nx
    win = rm[:, 0][:, None] * nx + cm[:, 0][None, :]                # the window each output pixel is pasted from
    assert np.array_equal(rects[win, 0].astype(np.int64) * big + rects[win, 2], origin)
    assert np.array_equal(np.broadcast_to(rm[:, 1][:, None], row.shape), row)
    assert np.array_equal(np.broadcast_to(cm[:, 1][None, :], col.shape), col)


def test_window_mosaic_choice():
    """pick_mosaic (engine.hip) through s2sr_debug_pick_mosaic / s2sr_debug_mosaic_patches: the reference's default 276-pixel
    windows (tile 256 + 2 x pad 10, cnn_super_resolution.py:244-257) travel 4 x 4 per launch image (1107 -> 1120 of patch extent:
    280 x 280 per window instead of 288 x 288); windows that are multiples of the 32-pixel patch, single windows and sizes where
    the separators eat the gain (532-pixel windows) stay one per image; a mosaic is never wider than 8 windows or ~1280 pixels and
    never holds more windows than there are.  The choice is made on what is LAUNCHED -- full mosaics plus one smaller mosaic for
    the remainder (r03 ADVICE: 17 windows as two 4 x 4 mosaics launched 2450 patches against 1377 for plain images): for every
    B the launched patches are at most the plain ones."""
    from s2sr import native
    assert native.pick_mosaic(256, 276, 276) == (4, 4)
    assert native.pick_mosaic(16, 276, 276) == (4, 4)
    assert native.pick_mosaic(3, 276, 276) == (3, 1)
    assert native.pick_mosaic(1, 276, 276) == (1, 1)
    assert native.pick_mosaic(64, 256, 256) == (1, 1)
    assert native.pick_mosaic(64, 532, 532) == (1, 1)
    r32 = lambda v: (v + 31) // 32
    for B in range(1, 65):                    # the ADVICE's examples: 5, 9, 17, 20, 25 windows of 276
        launched, plain = native.mosaic_patches(B, 276, 276)
        assert plain == B * 81 and launched <= plain, (B, launched, plain)
        kx, ky = native.pick_mosaic(B, 276, 276)
        if kx * ky > 1:
            assert launched <= 0.98 * plain, (B, kx, ky, launched, plain)
        if B % 16 == 0:
            assert (kx, ky) == (4, 4), (B, kx, ky)
        # the launched figure is full mosaics + one remainder mosaic of ceil(rem / kx) rows (one row: cut to its windows)
        per = kx * ky
        full, rem = divmod(B, per)
        exp = full * r32(ky * 277 - 1) * r32(kx * 277 - 1)
        if rem and per > 1:
            rky = min(-(-rem // kx), ky)
            rkx = rem if rky == 1 else kx
            exp += r32(rky * 277 - 1) * r32(rkx * 277 - 1)
        assert launched == (exp if per > 1 else plain), (B, kx, ky, launched, exp)
    assert native.mosaic_patches(17, 276, 276) == (1225 + 81, 17 * 81)
    assert native.mosaic_patches(25, 276, 276)[0] <= 1225 + 3 * 35 * 9 + 1     # 16 + 9: one 4 x 4 and a 4 x 3 (9 of its 12 slots used)
    rng = np.random.default_rng(6)
    for _ in range(300):
        B, th, tw = int(rng.integers(1, 400)), int(rng.integers(1, 700)), int(rng.integers(1, 700))
        kx, ky = native.pick_mosaic(B, th, tw)
        launched, plain = native.mosaic_patches(B, th, tw)
        assert launched <= plain
        assert 1 <= kx <= 8 and 1 <= ky <= 8
        if kx * ky > 1:
            assert kx * ky <= B
            assert kx * (tw + 1) - 1 <= 1280 + tw and ky * (th + 1) - 1 <= 1280 + th
            assert launched <= 0.98 * plain                           # it pays
