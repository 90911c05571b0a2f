"""GPU end-to-end through the reference-shaped Python seam (app.*)."""
import json

import numpy as np
import pytest
import torch

from oracle import postprocess_ref as pp
from oracle import rrdbnet_ref as ref
from s2sr import native
from s2sr import rasterio_lite as rio
from s2sr.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu


def _patch_weights(monkeypatch, tmp_path, nb_by_name):
    """Write seeded synthetic checkpoints where the reference looks for them (<dir>/<name>.pth)."""
    monkeypatch.setenv("S2SR_MODEL_DIR", str(tmp_path / "models"))
    (tmp_path / "models").mkdir(exist_ok=True)
    for name, nb in nb_by_name.items():
        sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(nb, seed=0).items()}
        torch.save({"params_ema": sd}, tmp_path / "models" / f"{name}.pth")


def test_realesrgan_class_matches_oracle(monkeypatch, tmp_path):
    import app.cnn_super_resolution as m
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    e = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)
    assert (e.scale, e.tile_size, e.tile_pad, e.model_name) == (4, 256, 10, "realesrgan_anime")
    img = np.random.default_rng(2).integers(0, 256, (40, 56, 3), dtype=np.uint8)
    out = e.enhance(img)
    exp = ref.enhance(img, ref.to_torch_sd(synthetic_state_dict(6, seed=0)), 6)
    d = np.abs(out.astype(np.int16) - exp.astype(np.int16))
    assert out.shape == (160, 224, 3) and d.max() <= 1 and (d == 0).mean() > 0.95
    with pytest.raises(TypeError):
        e.enhance(img.astype(np.float32))
    # a second object reuses the cached engine (construct-per-job is free)
    e2 = m.RealESRGAN(model_name="realesrgan_anime")
    assert e2._engine is e._engine


def test_process_wow_and_farm_sr(monkeypatch, tmp_path):
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6, "realesrgan_x4": 23})
    from app.farm_sr import apply_unsharp_mask, enhance_local_contrast, enhance_vegetation, process_farm_sr
    from app.wow_sr import _enhance_for_crops, process_wow_sr
    rgb = np.random.default_rng(3).integers(0, 256, (24, 32, 3), dtype=np.uint8)
    rgb[..., 1] = np.maximum(rgb[..., 1], 100)
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)})
    src = tmp_path / "scene.tif"
    rio.write_geotiff_rgb(src, rgb, geo)

    res = process_wow_sr(src, tmp_path / "wow", enhance_crops=True, model="realesrgan_anime")
    assert set(res) == {"timestamp", "input", "outputs", "sr_metadata"}
    meta = res["sr_metadata"]
    assert meta["original_size"] == [24, 32] and meta["output_size"] == [96, 128] and meta["scale"] == 4
    assert meta["enhancements"] == ["CLAHE local contrast", "Unsharp mask", "Vegetation boost"]
    out, g4 = rio.read_rgb_u8(res["outputs"]["sr_tif"])
    assert out.shape == (96, 128, 3) and g4.pixel_size == (2.5, 2.5)
    assert json.load(open(tmp_path / "wow" / "scene_wow_sr_metadata.json"))["sr_metadata"] == meta
    # expected pixels: oracle net on BGR, back to RGB, oracle post-process; u8 net output may
    # differ by 1 LSB, so compare the post-process on the library's own SR image instead
    png, _ = rio.read_rgb_u8(res["outputs"]["sr_png"])
    assert np.array_equal(png, out)
    res2 = process_wow_sr(src, tmp_path / "wow2", enhance_crops=False, model="realesrgan_anime")
    sr_plain, _ = rio.read_rgb_u8(res2["outputs"]["sr_tif"])
    assert np.array_equal(pp.enhance_for_crops(sr_plain), out)
    assert np.array_equal(_enhance_for_crops(sr_plain), out)
    exp_sr = ref.enhance(np.ascontiguousarray(rgb[:, :, ::-1]), ref.to_torch_sd(synthetic_state_dict(6, seed=0)), 6)[:, :, ::-1]
    assert np.abs(sr_plain.astype(np.int16) - exp_sr.astype(np.int16)).max() <= 1

    resf = process_farm_sr(src, tmp_path / "farm", scale=4)          # /api/sr path: 23-block net + farm constants
    farm, _ = rio.read_rgb_u8(resf["outputs"]["sr_tif"])
    assert farm.shape == (96, 128, 3) and resf["sr_metadata"]["model"] == "RealESRGAN_farm_x4"
    with pytest.raises(ValueError, match="Unknown model"):
        process_farm_sr(src, tmp_path / "farm2", scale=2)             # reference: job fails with this message
    # stand-alone farm helpers == oracle stages
    assert np.array_equal(apply_unsharp_mask(sr_plain, 1.2, 1.5), pp.unsharp(sr_plain, 1.5, 2.2, -1.2))
    assert np.array_equal(enhance_local_contrast(sr_plain, 2.5, 8), pp.local_contrast(sr_plain, 2.5, 8))
    assert np.array_equal(enhance_vegetation(sr_plain), pp.vegetation(sr_plain, 1.3))


def test_http_wow_and_sr_jobs(monkeypatch, tmp_path):
    """POST /api/wow and /api/sr end to end on the GPU path; poll GET /api/sr/{job_id}."""
    from fastapi.testclient import TestClient
    from app.sr_routes import create_app
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_x4": 23})
    rgb = np.random.default_rng(5).integers(0, 256, (20, 28, 3), dtype=np.uint8)
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)})
    (tmp_path / "data" / "source").mkdir(parents=True)
    src = tmp_path / "data" / "source" / "s2.tif"
    rio.write_geotiff_rgb(src, rgb, geo)
    tiled = []
    c = TestClient(create_app(tmp_path / "data", tiler=lambda tif, d: tiled.append((tif, d))))
    r = c.post("/api/wow", json={"auto_fetch": False})           # newest GeoTIFF in source/
    assert r.status_code == 200 and r.json()["status"] == "queued"
    st = c.get(f"/api/sr/{r.json()['job_id']}").json()           # TestClient runs background tasks before returning
    assert st["status"] == "completed", st
    assert st["result"]["sr_metadata"]["output_size"] == [80, 112] and st["result"]["tiles_dir"].endswith("tiles_wow")
    out, _ = rio.read_rgb_u8(st["result"]["outputs"]["sr_tif"])
    assert out.shape == (80, 112, 3)
    r2 = c.post("/api/sr", json={"input_file": str(src), "scale": 4, "model": "edsr"})
    st2 = c.get(f"/api/sr/{r2.json()['job_id']}").json()
    assert st2["status"] == "completed" and st2["result"]["sr_metadata"]["model"] == "RealESRGAN_farm_x4"
    import time
    time.sleep(1.1)          # job ids have 1-second resolution (reference main.py:411): avoid the collision
    r3 = c.post("/api/sr", json={"input_file": str(src), "scale": 2})        # accepted by validation, fails in the job
    st3 = c.get(f"/api/sr/{r3.json()['job_id']}").json()
    assert st3["status"] == "failed" and "Unknown model" in st3["message"]
    assert len(tiled) == 2 and set(c.get("/api/sr").json()["jobs"]) >= {r.json()["job_id"]}


def test_concurrent_jobs_share_one_engine(monkeypatch, tmp_path):
    """The reference runs /api/wow and /api/sr jobs from Starlette worker threads with no gate
    (main.py:66,602,670-675): several threads construct RealESRGAN and call enhance at once.  They
    share the cached native engine, which serialises calls per handle; results must equal the
    serial ones (different shapes force workspace / graph turnover between calls)."""
    import threading

    import app.cnn_super_resolution as m
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    rng = np.random.default_rng(12)
    imgs = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((40, 56, 3), (33, 47, 3), (64, 64, 3), (40, 56, 3))]
    serial = [m.RealESRGAN(model_name="realesrgan_anime").enhance(im) for im in imgs]
    results = [[None] * len(imgs) for _ in range(4)]
    errors = []

    def worker(tid):
        try:
            for rep in range(2):
                for i in ((np.arange(len(imgs)) + tid) % len(imgs)):
                    results[tid][i] = m.RealESRGAN(model_name="realesrgan_anime").enhance(imgs[i])
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for tid in range(4):
        for i in range(len(imgs)):
            assert np.array_equal(results[tid][i], serial[i]), (tid, i)


def test_two_engines_capture_and_regrow_on_two_threads():
    """Two handles on two threads, as the x4 and the anime-6B engines are under Starlette's pool (main.py:602,670-675): while one
    captures a hipGraph the other allocates and clears a bigger workspace, uploads stitch maps, loads weights.  None of that may
    touch the legacy stream: the runtime refuses hipMemset / hipMemcpy while any stream of the process captures ("would make
    the legacy stream depend on a capturing blocking stream") and voids the capture with it -- found by tools/soak_jobs.py."""
    import threading
    rng = np.random.default_rng(21)
    shapes = [(40, 56), (64, 64), (33, 47), (90, 70), (128, 96), (50, 140), (160, 160), (200, 120)]
    imgs = [rng.integers(0, 256, (*s, 3), dtype=np.uint8) for s in shapes]
    sd = synthetic_state_dict(1, seed=4)
    ref = native.Engine(num_block=1, precision=native.PREC_F16_HP)
    ref.load_state_dict(sd)
    serial = [ref.enhance_u8(im, tile=32, pad=4) for im in imgs]
    ref.close()
    errors, captures = [], [0, 0]
    barrier = threading.Barrier(2)

    def worker(tid):
        try:
            barrier.wait(10)
            for rep in range(3):
                e = native.Engine(num_block=1, precision=native.PREC_F16_HP)     # a fresh handle: every shape is a new capture
                e.load_state_dict(sd)                                           # and most of them a bigger workspace
                order = range(len(imgs)) if tid == 0 else reversed(range(len(imgs)))
                for i in order:
                    for again in range(2):                                      # graphs are captured at the second sighting
                        if not np.array_equal(e.enhance_u8(imgs[i], tile=32, pad=4), serial[i]):
                            errors.append((tid, rep, i, "pixels differ"))
                captures[tid] += e.graph_stats()[0]
                e.close()
        except Exception as ex:                      # noqa: BLE001
            errors.append((tid, repr(ex)))

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errors, errors[:4]
    assert min(captures) > 0, captures


def test_capture_voided_by_another_runtime_user_is_recovered():
    """Another user of the HIP runtime in the process (here: a thread in torch.cuda.synchronize / allocator traffic) voids a graph
    capture in progress -- the library's gate cannot see it -- and the runtime leaves the stream unusable.  The host-facing calls
    replace the stream and run again: no error reaches the caller, the bytes are the serial ones, and after three voided
    captures the handle stops capturing.  (The other thread's own call fails with hipErrorStreamCaptureUnsupported while a
    capture is open: runtime behaviour, INTEGRATION.md "Threads".)"""
    import threading
    rng = np.random.default_rng(5)
    sd = synthetic_state_dict(1, seed=4)
    imgs = [rng.integers(0, 256, (40 + 8 * i, 56 + 4 * i, 3), dtype=np.uint8) for i in range(30)]
    ref = native.Engine(num_block=1, precision=native.PREC_F16_HP)
    ref.load_state_dict(sd)
    serial = [ref.enhance_u8(im, tile=32, pad=4) for im in imgs]
    ref.close()
    stop = threading.Event()
    refused = [0]

    def pest():
        while not stop.is_set():
            try:
                torch.cuda.synchronize()
                torch.empty(1 << 20, device="cuda")
            except Exception:                      # noqa: BLE001 -- the runtime refuses these while a capture is open
                refused[0] += 1
    t = threading.Thread(target=pest)
    t.start()
    try:
        e = native.Engine(num_block=1, precision=native.PREC_F16_HP)
        e.load_state_dict(sd)
        for rep in range(3):
            for i, im in enumerate(imgs):
                assert np.array_equal(e.enhance_u8(im, tile=32, pad=4), serial[i]), (rep, i)
    finally:
        stop.set()
        t.join()
    assert np.array_equal(e.enhance_u8(imgs[0], tile=32, pad=4), serial[0])
    e.close()


def test_concurrent_postprocess_jobs_share_one_handle():
    """The app keeps ONE post-process handle per GPU (app.wow_sr._pp_engine) and the reference runs jobs
    from concurrent worker threads (main.py:247-368, 629-675): 4 threads x different images of different
    sizes through `_enhance_for_crops` / the farm functions must each get their own pixels back
    (s2sr_postprocess_u8 holds the handle's lock from the upload to the download)."""
    import threading
    from app.farm_sr import apply_unsharp_mask
    from app.wow_sr import _enhance_for_crops
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in [(96, 128), (200, 64), (128, 128), (333, 77)]]
    for im in imgs:
        im[..., 1] = np.maximum(im[..., 1], 80)
    serial = [(_enhance_for_crops(im), apply_unsharp_mask(im, 1.2, 1.5)) for im in imgs]
    for a, im in zip(serial, imgs):
        assert np.array_equal(a[0], pp.enhance_for_crops(im))
    errors = []
    barrier = threading.Barrier(len(imgs))

    def worker(i):
        try:
            barrier.wait(10)
            for _ in range(25):
                a = _enhance_for_crops(imgs[i])
                b = apply_unsharp_mask(imgs[i], 1.2, 1.5)
                if not (np.array_equal(a, serial[i][0]) and np.array_equal(b, serial[i][1])):
                    errors.append(i)
                    return
        except Exception as e:                      # noqa: BLE001
            errors.append((i, repr(e)))

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(len(imgs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errors, errors


def test_http_enhance_upload_runs_on_gpu(monkeypatch, tmp_path):
    """/api/enhance end to end (main.py:544-675): PNG upload -> admission -> anime model on the GPU ->
    job table `completed` with the wow result schema."""
    from fastapi.testclient import TestClient
    from app.sr_routes import create_app
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    rgb = np.random.default_rng(8).integers(0, 256, (20, 28, 3), dtype=np.uint8)
    png = tmp_path / "plate.png"
    rio.write_png(png, rgb)
    b = "BoUnD"
    body = (f'--{b}\r\nContent-Disposition: form-data; name="model"\r\n\r\nrealesrgan_anime\r\n'
            f'--{b}\r\nContent-Disposition: form-data; name="image"; filename="plate.png"\r\n'
            f'Content-Type: image/png\r\n\r\n').encode() + png.read_bytes() + f"\r\n--{b}--\r\n".encode()
    c = TestClient(create_app(tmp_path / "data", tiler=False, devices=[0]))
    r = c.post("/api/enhance", content=body, headers={"content-type": f"multipart/form-data; boundary={b}"})
    assert r.status_code == 200 and r.json()["model"] == "realesrgan_anime"
    st = c.get(f"/api/sr/{r.json()['job_id']}").json()
    assert st["status"] == "completed", st
    out, _ = rio.read_rgb_u8(st["result"]["outputs"]["sr_png"])
    exp = ref.enhance(np.ascontiguousarray(rgb[:, :, ::-1]), ref.to_torch_sd(synthetic_state_dict(6, seed=0)), 6)
    exp = pp.enhance_for_crops(np.ascontiguousarray(exp[:, :, ::-1]))
    d = np.abs(out.astype(np.int16) - exp.astype(np.int16))
    assert out.shape == (80, 112, 3) and np.mean(d == 0) > 0.9


def test_http_enhance_on_the_references_upload_matches_its_recorded_result(monkeypatch, tmp_path, golden_dir):
    """The reference's recorded /api/enhance job replayed on the GPU: its own upload (576x432, decoded pixels in
    g8_real_image.npz, re-encoded losslessly as PNG) with model realesrgan_anime -> the job's `result` must have the recorded
    metadata JSON's keys, value types and non-path values (tests/golden/ref_wow_sr_metadata_anime.json, written by the
    reference's process_wow_sr, wow_sr.py:243-259), and the SR pixels must be the reference net's (through the oracle's
    post-process: the net output may differ by 1 LSB, which CLAHE / unsharp amplify)."""
    import json
    from fastapi.testclient import TestClient
    from app.sr_routes import create_app
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    want = json.loads((golden_dir / "ref_wow_sr_metadata_anime.json").read_text())
    g8 = np.load(golden_dir / "g8_real_image.npz")
    rgb = np.ascontiguousarray(g8["img_bgr"][:, :, ::-1])
    png = tmp_path / "1758691019_vin.png"
    rio.write_png(png, rgb)
    b = "BoUnD"
    body = (f'--{b}\r\nContent-Disposition: form-data; name="model"\r\n\r\nrealesrgan_anime\r\n'
            f'--{b}\r\nContent-Disposition: form-data; name="image"; filename="1758691019_vin.png"\r\n'
            f'Content-Type: image/png\r\n\r\n').encode() + png.read_bytes() + f"\r\n--{b}--\r\n".encode()
    c = TestClient(create_app(tmp_path / "data", tiler=False, devices=[0]))
    r = c.post("/api/enhance", content=body, headers={"content-type": f"multipart/form-data; boundary={b}"})
    assert r.status_code == 200, r.text
    st = c.get(f"/api/sr/{r.json()['job_id']}").json()
    assert st["status"] == "completed", st
    got = st["result"]

    def shape(v):
        if isinstance(v, dict):
            return {k: shape(x) for k, x in v.items()}
        if isinstance(v, list):
            return [shape(x) for x in v]
        return type(v).__name__
    assert list(got) == list(want) and shape(got) == shape(want) and got["outputs"]["sr_tif"] is None
    for k, v in want["sr_metadata"].items():
        if k not in ("input_file", "output_file"):
            assert got["sr_metadata"][k] == v, k
    out, _ = rio.read_rgb_u8(got["outputs"]["sr_png"])
    assert list(out.shape[:2]) == want["sr_metadata"]["output_size"] == [2304, 1728]
    # pixels: the recorded windows of the reference net's u8 output (BGR), post-processed by the oracle on the WHOLE image is
    # not available (the fixture holds windows), so check the SR stage alone through the class, then the job's own composition
    import app.cnn_super_resolution as m
    sr = m.RealESRGAN(model_name="realesrgan_anime").enhance(g8["img_bgr"])
    for (y, x), wq in zip(g8["full_win_yx"], g8["full_win_u8_b6"]):
        assert np.abs(sr[y:y + 64, x:x + 64].astype(np.int16) - wq.astype(np.int16)).max() <= 1
    assert np.array_equal(out, pp.enhance_for_crops(np.ascontiguousarray(sr[:, :, ::-1])))


def test_farm_sr_on_fp8_trunk(monkeypatch, tmp_path):
    """BASELINE.json configs[4]: the /api/sr variant (process_farm_sr) selected onto the fp8 trunk by
    S2SR_FARM_PRECISION=fp8; pixels stay within the mode's measured tolerance of the default-precision job."""
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_x4": 23})
    from app.farm_sr import process_farm_sr
    rgb = np.random.default_rng(4).integers(0, 256, (24, 32, 3), dtype=np.uint8)
    src = tmp_path / "scene.tif"
    rio.write_geotiff_rgb(src, rgb, rio.GeoRef({rio.TAG_PIXEL_SCALE: (10.0, 10.0, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)}))
    a = process_farm_sr(src, tmp_path / "hp", scale=4)
    monkeypatch.setenv("S2SR_FARM_PRECISION", "fp8")
    b = process_farm_sr(src, tmp_path / "f8", scale=4)
    ia, _ = rio.read_rgb_u8(a["outputs"]["sr_tif"])
    ib, _ = rio.read_rgb_u8(b["outputs"]["sr_tif"])
    d = np.abs(ia.astype(np.int16) - ib.astype(np.int16))
    print(f"farm_sr fp8 vs hp: max {d.max()} LSB, identical {np.mean(d == 0):.4f}")
    # the farm post-process (CLAHE + unsharp 2.2/-1.2) amplifies the 1-3 LSB differences of the two nets on this noise image
    assert ia.shape == ib.shape == (96, 128, 3) and not np.array_equal(ia, ib) and d.max() <= 48 and d.mean() < 3.0
    import app.cnn_super_resolution as m
    assert len({k[2] for k in m._ENGINES}) >= 2          # two engines: default precision and fp8


def test_bench_two_ranks_rehearsal(tmp_path):
    """bench.py's N > 1 control flow (weight broadcast from rank 0, double-buffered steps with the all-gather on a
    communication stream, max-over-ranks timing, one JSON line from rank 0) with TWO ranks on this one GPU: RCCL refuses two
    ranks on one device, so the rehearsal runs the collectives over gloo (S2SR_BENCH_BACKEND / S2SR_BENCH_SAME_DEVICE are
    rehearsal knobs the driver never sets).  Real N > 1 RCCL runs need a multi-GPU node."""
    import os
    import socket
    import subprocess
    import sys
    from pathlib import Path
    repo = Path(__file__).resolve().parent.parent
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, S2SR_BENCH_SAME_DEVICE="1", S2SR_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", S2SR_BENCH_AOI="1024")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(repo / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--full"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=str(repo))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert "RCCL all-gather" in d["config"]["workload"] and "cpu_baseline" not in d
    assert d["roofline"]["timed_pass"]["graph_replays"] >= 1
    # the strong-scaling AOI leg (configs[2]): one 1024x1024 image over the two ranks, 16 windows in blocks of 8, host image on rank 0
    ao = d["aoi_strong_scaling"]
    assert ao["n_gpus"] == 2 and ao["scaling"] == "strong" and ao["value"] > 0 and ao["rccl_ranks_seen"] == 2
    assert "blocks of 8 per rank" in ao["workload"]
    # ... and in the flavour the reference requests by default (enhance_crops=True: band histograms, LUTs, finish in row bands)
    assert ao["enhance_crops"]["value"] > 0 and ao["enhance_crops"]["seconds"] > 0


def test_bench_plain_run_dumps_the_last_steps_outputs(tmp_path):
    """A plain bench.py run prints the headline line alone (no stats pass, no legs behind it), times exactly --steps steps, and
    --dump-outputs writes what its last step computed: the first whole SR tile and the seeded sample of every output byte, both
    float32, equal to the engine's own output on the same seeded tiles and weights."""
    import subprocess
    import sys
    from pathlib import Path
    from s2sr.synth import synthetic_tiles
    repo = Path(__file__).resolve().parent.parent
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(repo / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=str(repo))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "f16" and d["higher_is_better"] is True
    assert not {"roofline", "secondary", "cpu_baseline"} & set(d)
    tile0 = np.load(out_dir / "sr_tile0.npy")
    sample = np.load(out_dir / "sr_sample.npy")
    assert tile0.dtype == sample.dtype == np.float32 and tile0.shape == (1024, 1024, 3) and sample.shape == (4_000_000,)
    assert tile0.nbytes + sample.nbytes <= 64 << 20
    e = native.Engine(num_block=23, device=0, precision=native.PREC_F16_HP)
    e.load_state_dict(synthetic_state_dict(23, seed=0))
    want = e.forward_batch_u8(synthetic_tiles(4, 256, seed=1234)).copy()
    e.close()
    assert np.array_equal(tile0, want[0].astype(np.float32))
    idx = np.sort(np.random.default_rng(0).integers(0, want.size, size=4_000_000))
    assert np.array_equal(sample, want.reshape(-1)[idx].astype(np.float32))


def test_job_result_beyond_2_gib(monkeypatch, tmp_path):
    """Maximum sizes: a 2816 x 16384 AOI (704 windows of the 256 / 10 plan) gives an 11264 x 65536 x 3 result of 2.21 GB -- byte offsets
    past 2^31 in the stitch, the band-wise swaps, histograms, apply + sharpen and the copies out.  Checked through what does not depend
    on the size: (1) windows see only their own 276 x 276 pixels, so the job of the bottom-right 1792 x 4096 crop (small offsets
    everywhere) gives the same bytes away from the crop's own top / left windows; (2) the band-wise post-process of the job equals
    the whole-image launch of s2sr_postprocess_u8 on the plain job's result."""
    import app.cnn_super_resolution as m
    from s2sr import native
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    e = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)
    H, W, y0, x0 = 2816, 16384, 1024, 12288
    rng = np.random.default_rng(77)
    rgb = rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)     # blocky: statistics of an image, cheap to draw
    rgb += rng.integers(0, 8, (H, W, 3), dtype=np.uint8)
    rgb[..., 1] = np.maximum(rgb[..., 1], 90)
    big = e.enhance_job(rgb, None)
    assert big.shape == (4 * H, 4 * W, 3) and big.nbytes > 2 ** 31
    small = e.enhance_job(np.ascontiguousarray(rgb[y0:, x0:]), None)
    assert np.array_equal(big[4 * (y0 + 256):, 4 * (x0 + 256):], small[4 * 256:, 4 * 256:])
    assert big[-1, -1].tolist() == small[-1, -1].tolist() and int(big[4 * (y0 + 256):].max()) > 0
    del small
    prm = native.pp_wow()
    got = e.enhance_job(rgb, prm)
    want = e._engine.postprocess_u8(big, prm)
    assert np.array_equal(got, want)


def test_enhance_job_equals_the_separate_steps(monkeypatch, tmp_path):
    """s2sr_enhance_job_u8 (RealESRGAN.enhance_job: RGB in, RGB2BGR, the net, BGR2RGB, the post-process, RGB out -- one upload, one
    download) gives the bytes of the reference's own sequence (wow_sr.py:85-110: cvtColor, enhance, cvtColor, _enhance_for_crops)
    run as separate calls -- on the whole-image branch, on the tiled branch (banded copies off: the post-process is image-global),
    with the wow and the farm constants and without a post-process; and the PNG / GeoTIFF written side by side decode to it."""
    import app.cnn_super_resolution as m
    from s2sr import native
    _patch_weights(monkeypatch, tmp_path, {"realesrgan_anime": 6})
    e = m.RealESRGAN(model_name="realesrgan_anime", tile_size=256)
    rng = np.random.default_rng(21)
    # whole image; 3 x 3 windows of 276 with shifted edges; 6 x 5 windows in several chunks: the band-wise finish (swap per band,
    # histograms per band, the image finished and copied out in two finishing bands)
    for (H, W) in ((96, 130), (540, 610), (1300, 1100)):
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        rgb[..., 1] = np.maximum(rgb[..., 1], 90)
        sr_rgb = np.ascontiguousarray(e.enhance(np.ascontiguousarray(rgb[:, :, ::-1]))[:, :, ::-1])
        assert np.array_equal(e.enhance_job(rgb, None), sr_rgb), (H, W)
        for prm in (native.pp_wow(), native.pp_farm()):
            want = e._engine.postprocess_u8(sr_rgb, prm)
            got = e.enhance_job(rgb, prm)
            assert np.array_equal(got, want), (H, W, prm.blur_sigma)
    # the same chunked job into a PAGEABLE result (S2SR_PINNED_OUT=0 / a pool at its cap): the finishing bands travel through the
    # library's pinned staging slices instead of one DMA each -- same bytes
    native.pinned_pool.on = False
    try:
        paged = e.enhance_job(rgb, native.pp_farm())
    finally:
        native.pinned_pool.on = True
    assert np.array_equal(paged, got)
    geo = rio.GeoRef({rio.TAG_PIXEL_SCALE: (2.5, 2.5, 0.0), rio.TAG_TIEPOINT: (0.0, 0.0, 0.0, 5e5, 4e6, 0.0)})
    rio.write_outputs(got, tmp_path / "o.png", tmp_path / "o.tif", geo)
    back, g = rio.read_rgb_u8(tmp_path / "o.tif")
    assert np.array_equal(back, got) and g.pixel_size == (2.5, 2.5)
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "o.png").convert("RGB")), got)
