#!/usr/bin/env python3
"""SHA-256 of every output of the routes that run the whole-image pipeline of engine_aoi.hip: one `route dtype shape sha256` line
each.  Seeded inputs, synthetic weights, 1-block HP and F16 handles plus one x2plus and one compact handle, one process.  Run it on
two builds of the library (S2SR_LIB names the one to load) and compare the lines: a host-side change of the pipeline leaves every
line as it was (profiles/enhance_pipeline_same_bytes.txt).

    python tools/enhance_same_bytes.py > lines.txt
"""
from __future__ import annotations

import hashlib
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (str(REPO / "sentinel2-super-resolution-poc_amd"), str(REPO)):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from s2sr import native  # noqa: E402
from s2sr.weights import synthetic_compact_state_dict, synthetic_state_dict  # noqa: E402

IMAGES = [(28, 36, 256, 10), (100, 90, 16, 2), (53, 200, 16, 3), (34, 36, 16, 2)]   # untiled; one chunk; three chunks; coinciding rows
CHUNKED = IMAGES[2]
RANGES = [(0, 65535), (1000, 11000)]


def say(route, a):
    a = np.ascontiguousarray(a)
    print(f"{route} {a.dtype} {a.shape} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def image8(H, W):
    return np.random.default_rng(7 + 1000 * H + W).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def image16(H, W, hi):
    return np.random.default_rng(11 + 1000 * H + W).integers(0, 13000 if hi < 65535 else 65536, size=(H, W, 3)).astype(np.uint16)


def default_doors(name, e):
    for H, W, t, p in IMAGES:
        img, tag = image8(H, W), f"{name} {H}x{W} {t}/{p}"
        say(f"{tag} enhance_u8", e.enhance_u8(img, tile=t, pad=p))
        say(f"{tag} enhance_f32", e.enhance_f32(img, tile=t, pad=p))
        say(f"{tag} tile_process_f32", e.tile_process_f32(img, tile=t, pad=p))
        say(f"{tag} enhance_u8 again", e.enhance_u8(img, tile=t, pad=p))
    H, W, t, p = CHUNKED
    for what, prm in (("plain", None), ("wow", native.pp_wow()), ("farm", native.pp_farm())):
        say(f"{name} job {what}", e.enhance_job_u8(image8(H, W), prm, tile=t, pad=p))
    say(f"{name} job wow one chunk", e.enhance_job_u8(image8(100, 90), native.pp_wow(), tile=16, pad=2))
    say(f"{name} job wow untiled", e.enhance_job_u8(image8(28, 36), native.pp_wow()))
    for H, W, t, p in IMAGES[:3]:
        for lo, hi in RANGES:
            img, tag = image16(H, W, hi), f"{name} {H}x{W} {t}/{p} u16 {lo}-{hi}"
            q, f = e.enhance_u16(img, lo, hi, tile=t, pad=p, want_f32=True)
            say(f"{tag} both.u16", q)
            say(f"{tag} both.f32", f)
            say(f"{tag} u16 only", e.enhance_u16(img, lo, hi, tile=t, pad=p))
            say(f"{tag} u16 only again", e.enhance_u16(img, lo, hi, tile=t, pad=p))
    rng = np.random.default_rng(3)
    say(f"{name} forward_batch_u8 40x32x32", e.forward_batch_u8(rng.integers(0, 256, size=(40, 32, 32, 3), dtype=np.uint8)))
    say(f"{name} forward_batch_u8 40x24x40 (mosaic)", e.forward_batch_u8(rng.integers(0, 256, size=(40, 24, 40, 3), dtype=np.uint8)))
    # the multi-GPU building blocks: the reference's 42 windows of 100 x 90 at 16 / 2, cut, forwarded and stitched on device buffers
    H, W, t, p = IMAGES[1]
    st = torch.cuda.current_stream().cuda_stream
    d_img = torch.from_numpy(image8(H, W)).cuda()
    d_win = torch.zeros((42, 20, 20, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((42, 80, 80, 3), dtype=torch.uint8, device="cuda")
    d_sr = torch.zeros((4 * H, 4 * W, 3), dtype=torch.uint8, device="cuda")
    e.cut_windows_u8_dev(d_img.data_ptr(), H, W, t, p, 0, 42, d_win.data_ptr(), st)
    e.forward_batch_u8_dev(d_win.data_ptr(), 42, 20, 20, d_out.data_ptr(), st)
    e.stitch_windows_u8_dev(d_out.data_ptr(), H, W, t, p, d_sr.data_ptr(), st)
    torch.cuda.synchronize()
    say(f"{name} cut_windows", d_win.cpu().numpy())
    say(f"{name} cut+forward+stitch", d_sr.cpu().numpy())


def blend_doors(name, e):
    for H, W, t, p in IMAGES[1:3]:
        img, tag = image8(H, W), f"{name} {H}x{W} {t}/{p} blend_u8"
        u8, f = e.enhance_blend_u8(img, tile=t, pad=p, want_f32=True)
        say(f"{tag} both.u8", u8)
        say(f"{tag} both.f32", f)
        say(f"{tag} u8 only", e.enhance_blend_u8(img, tile=t, pad=p))
    H, W, t, p = CHUNKED
    img = image8(H, W)
    say(f"{name} blend job swap_rb", e.enhance_blend_u8(img, swap_rb=True, tile=t, pad=p))
    for what, prm in (("wow", native.pp_wow()), ("farm", native.pp_farm())):
        say(f"{name} blend job {what}", e.enhance_blend_u8(img, prm, swap_rb=True, tile=t, pad=p))
        say(f"{name} blend {what} no swap", e.enhance_blend_u8(img, prm, tile=t, pad=p))
    for H, W, t, p in IMAGES[1:3]:
        for lo, hi in RANGES:
            img, tag = image16(H, W, hi), f"{name} {H}x{W} {t}/{p} blend_u16 {lo}-{hi}"
            q, f = e.enhance_blend_u16(img, lo, hi, tile=t, pad=p, want_f32=True)
            say(f"{tag} both.u16", q)
            say(f"{tag} both.f32", f)
            say(f"{tag} u16 only", e.enhance_blend_u16(img, lo, hi, tile=t, pad=p))
    # the fall-throughs: no ramp (pad 0), and an image the switch leaves whole
    for H, W, kw in ((53, 200, dict(tile=16, pad=0)), (28, 36, dict())):
        img, tag = image8(H, W), f"{name} {H}x{W} blend fall-through {kw.get('tile', 256)}/{kw.get('pad', 10)}"
        u8, f = e.enhance_blend_u8(img, want_f32=True, **kw)
        say(f"{tag} both.u8", u8)
        say(f"{tag} both.f32", f)
        say(f"{tag} job wow", e.enhance_blend_u8(img, native.pp_wow(), swap_rb=True, **kw))
        q, f = e.enhance_blend_u16(image16(H, W, 65535), want_f32=True, **kw)
        say(f"{tag} u16 both.u16", q)
        say(f"{tag} u16 both.f32", f)
        say(f"{tag} u16 only", e.enhance_blend_u16(image16(H, W, 65535), **kw))


def display(name, e):
    """the 8-bit rendering from the copy enhance_u16 / enhance_blend_u16 leave on the device"""
    H, W, t, p = CHUNKED
    img = image16(H, W, 65535)
    lut = (np.arange(65536, dtype=np.uint32) >> 8).astype(np.uint8)
    lut = np.ascontiguousarray(np.stack([lut, 255 - lut, lut // 2]))
    for door in ("enhance_u16", "enhance_blend_u16"):
        getattr(e, door)(img, tile=t, pad=p)
        say(f"{name} display_hist after {door}", e.display_hist_u16(None, shape=(4 * H, 4 * W)))
        getattr(e, door)(img, tile=t, pad=p)
        say(f"{name} display_apply after {door}", e.display_apply_u16(None, lut, shape=(4 * H, 4 * W)))


def main():
    for name, prec in (("hp", native.PREC_F16_HP), ("f16", native.PREC_F16)):
        e = native.Engine(num_block=1, precision=prec)
        e.load_state_dict(synthetic_state_dict(1, seed=0))
        default_doors(name, e)
        blend_doors(name, e)
        display(name, e)
        e.close()
        e = native.Engine(num_block=1, precision=prec, scale=2)
        e.load_state_dict(synthetic_state_dict(1, seed=0, scale=2))
        for t, p in ((16, 2), (256, 10)):
            say(f"{name} x2plus 37x45 {t}/{p} enhance_u8", e.enhance_u8(image8(37, 45), tile=t, pad=p))
            say(f"{name} x2plus 37x45 {t}/{p} enhance_f32", e.enhance_f32(image8(37, 45), tile=t, pad=p))
        u8, f = e.enhance_blend_u8(image8(37, 45), tile=16, pad=2, want_f32=True)
        say(f"{name} x2plus 37x45 16/2 blend_u8 both.u8", u8)
        say(f"{name} x2plus 37x45 16/2 blend_u8 both.f32", f)
        say(f"{name} x2plus 37x45 16/2 blend_u8 u8 only", e.enhance_blend_u8(image8(37, 45), tile=16, pad=2))
        e.close()
    e = native.Engine(num_block=16, precision=native.PREC_F16_HP, arch="compact")
    e.load_state_dict(synthetic_compact_state_dict(16, seed=0))
    H, W, t, p = CHUNKED
    say("compact 53x200 16/3 enhance_u8", e.enhance_u8(image8(H, W), tile=t, pad=p))
    say("compact 53x200 16/3 blend_u8", e.enhance_blend_u8(image8(H, W), tile=t, pad=p))
    e.close()


if __name__ == "__main__":
    main()
