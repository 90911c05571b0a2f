"""SRVGGNetCompact (realesr-general-x4v3, realesr-general-wdn-x4v3, realesr-animevideov3) on the CPU, written from its definition
with torch's own operators on the raw state-dict arrays:

    h   = PReLU_64(conv3x3(x, 3 -> 64))                      body.0, body.1
    h   = PReLU_64(conv3x3(h, 64 -> 64))   x num_conv        body.2 .. body.{2 num_conv + 1}
    y   = conv3x3(h, 64 -> 48)                               body.{2 num_conv + 2}
    out = pixel_shuffle(y, 4) + nearest_upsample(x, 4)

plus `RealESRGAN.enhance` / `_tile_process` around it on the reference's window plan (oracle.rrdbnet_ref.tile_plan) and
`forward_emulated`, the same net with the device's number formats.  The checker of the compact library paths;
tests/test_compact_cpu.py pins it to tests/golden/g10_compact.npz, which tools/make_golden_compact.py wrote with a separately
written nn.Module driven through the reference's own enhance / _tile_process."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rrdbnet_ref as ref

UPSCALE = 4


def num_conv_of(sd) -> int:
    last = max(int(k.split(".")[1]) for k in sd if k.startswith("body."))
    return (last - 2) // 2


def _t(a, dtype) -> torch.Tensor:
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a.detach().cpu()).to(dtype)


def layer(h: torch.Tensor, sd, i: int, dtype=torch.float64) -> torch.Tensor:
    """Conv i (0 = the first conv, 1..num_conv the body convs) followed by its PReLU; i = num_conv + 1 is the last conv (no
    activation)."""
    nc = num_conv_of(sd)
    y = F.conv2d(h.to(dtype), _t(sd[f"body.{2 * i}.weight"], dtype), _t(sd[f"body.{2 * i}.bias"], dtype), stride=1, padding=1)
    return y if i == nc + 1 else F.prelu(y, _t(sd[f"body.{2 * i + 1}.weight"], dtype))


@torch.no_grad()
def forward(x: torch.Tensor, sd, dtype=torch.float64) -> torch.Tensor:
    """[N,3,H,W] float in [0,1] -> [N,3,4H,4W] (`dtype` arithmetic throughout)."""
    nc = num_conv_of(sd)
    x = x.to(dtype)
    h = x
    for i in range(nc + 2):
        h = layer(h, sd, i, dtype)
    return F.pixel_shuffle(h, UPSCALE) + F.interpolate(x, scale_factor=UPSCALE, mode="nearest")


def _r16(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


@torch.no_grad()
def forward_emulated(x_u8: torch.Tensor, sd) -> torch.Tensor:
    """The device's arithmetic on the CPU: [N,3,H,W] holding exact integers 0..255 -> [N,3,4H,4W] float32.  Weights and every
    stored activation rounded to fp16, fp32 accumulation, fp32 bias / slope / base add; the first conv runs on the integers and
    scales by 1/255 in fp32 behind the accumulation, the base is x * (1/255) in fp32 (csrc/conv3x3.hip EPI_CFIRST / EPI_CLAST)."""
    nc = num_conv_of(sd)
    f32 = torch.float32
    x = x_u8.to(f32)
    inv = torch.tensor(1.0 / 255.0, dtype=f32)
    w0 = _r16(_t(sd["body.0.weight"], f32))
    h = F.conv2d(x, w0, None, padding=1) * inv + _t(sd["body.0.bias"], f32).view(1, -1, 1, 1)
    h = _r16(F.prelu(h, _t(sd["body.1.weight"], f32)))
    for i in range(1, nc + 1):
        y = F.conv2d(h, _r16(_t(sd[f"body.{2 * i}.weight"], f32)), _t(sd[f"body.{2 * i}.bias"], f32), padding=1)
        h = _r16(F.prelu(y, _t(sd[f"body.{2 * i + 1}.weight"], f32)))
    last = 2 * nc + 2
    y = F.conv2d(h, _r16(_t(sd[f"body.{last}.weight"], f32)), _t(sd[f"body.{last}.bias"], f32), padding=1)
    return F.pixel_shuffle(y, UPSCALE) + F.interpolate(x * inv, scale_factor=UPSCALE, mode="nearest")


@torch.no_grad()
def tile_process(x: torch.Tensor, sd, tile_size: int = 256, tile_pad: int = 10, dtype=torch.float64, fwd=None) -> torch.Tensor:
    """`_tile_process`: windows of ref.tile_plan(..., scale=4), hard crop, later windows overwrite."""
    fwd = fwd or (lambda t: forward(t, sd, dtype))
    n, c, h, w = x.shape
    out = None
    for (y1, y2, x1, x2), (top, bottom, left, right), (oy1, oy2, ox1, ox2) in ref.tile_plan(h, w, tile_size, tile_pad, UPSCALE):
        t = fwd(x[:, :, y1:y2, x1:x2])
        if out is None:
            out = torch.zeros((n, c, UPSCALE * h, UPSCALE * w), dtype=t.dtype)
        out[:, :, oy1:oy2, ox1:ox2] = t[:, :, top:t.shape[2] - bottom, left:t.shape[3] - right]
    return out


@torch.no_grad()
def enhance_float(img_u8: np.ndarray, sd, tile_size: int = 256, tile_pad: int = 10, force_tiled: bool = False,
                  emulated: bool = False) -> np.ndarray:
    """HxWx3 u8 -> 4Hx4Wx3 before quantisation (float64; float32 with `emulated`): whole image when H*W <= tile^2*4, else (or
    with force_tiled: `_tile_process` alone) the windows."""
    H, W, _ = img_u8.shape
    xi = torch.from_numpy(np.ascontiguousarray(img_u8)).permute(2, 0, 1).unsqueeze(0)
    if emulated:
        x, fwd = xi.to(torch.float32), (lambda t: forward_emulated(t, sd))
    else:
        x, fwd = xi.to(torch.float64) / 255.0, (lambda t: forward(t, sd))
    o = tile_process(x, sd, tile_size, tile_pad, fwd=fwd) if (force_tiled or H * W > tile_size * tile_size * 4) else fwd(x)
    return o[0].permute(1, 2, 0).numpy()


def quantise(out: np.ndarray) -> np.ndarray:
    """(out*255).clip(0,255).astype(uint8): truncation, as RealESRGAN.enhance."""
    return (out * 255.0).clip(0, 255).astype(np.uint8)


def enhance(img_u8: np.ndarray, sd, tile_size: int = 256, tile_pad: int = 10, emulated: bool = False) -> np.ndarray:
    """`RealESRGAN.enhance`: HxWx3 u8 -> 4Hx4Wx3 u8."""
    return quantise(enhance_float(img_u8, sd, tile_size, tile_pad, emulated=emulated))


def gpu_test_images():
    """The u8 images tests/test_gpu_compact.py runs through forward_batch_u8 / enhance_u8 / tile_process_f32 (seeded)."""
    rng = np.random.default_rng(77)
    return {"batch": rng.integers(0, 256, size=(3, 40, 56, 3), dtype=np.uint8),
            "whole": rng.integers(0, 256, size=(300, 420, 3), dtype=np.uint8),
            "tiled": rng.integers(0, 256, size=(700, 900, 3), dtype=np.uint8)}


def u8_cap_check(a_u8, b_u8, cap):
    d = np.abs(a_u8.astype(np.int16) - b_u8.astype(np.int16))
    return int(d.max()), float((d > 0).mean()), bool(d.max() <= 1 and (d > 0).mean() <= cap)
