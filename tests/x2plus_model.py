"""RealESRGAN_x2plus on the CPU: the oracle's x4 net (oracle/rrdbnet_ref.py) composed with `F.pixel_unshuffle(x, 2)`, the
reference's window plan at scale 2, RealESRGANer's mod-2 reflect pad and the crop back to 2H x 2W.

The checker for the scale-2 library paths (tests/test_x2plus_cpu.py pins it to tests/golden/g9_x2plus.npz, which the reference's
own classes wrote; the reflect pad has no reference counterpart and is pinned here only)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rrdbnet_ref as ref


def forward(x: torch.Tensor, sd, num_block: int) -> torch.Tensor:
    """[N,3,H,W] float, H and W even -> [N,3,2H,2W]: RRDBNet(num_in_ch=12, scale=4) on pixel_unshuffle(x, 2)."""
    return ref.rrdbnet_forward(F.pixel_unshuffle(x, 2), sd, num_block, 4)


def tile_process(x: torch.Tensor, sd, num_block: int, tile_size: int = 256, tile_pad: int = 10) -> torch.Tensor:
    """`_tile_process` at scale 2: windows of ref.tile_plan(..., scale=2), later windows overwrite."""
    n, c, h, w = x.shape
    out = torch.zeros((n, c, 2 * h, 2 * w))
    for (y1, y2, x1, x2), (top, bottom, left, right), (oy1, oy2, ox1, ox2) in ref.tile_plan(h, w, tile_size, tile_pad, 2):
        t = forward(x[:, :, y1:y2, x1:x2], sd, num_block)
        out[:, :, oy1:oy2, ox1:ox2] = t[:, :, top:t.shape[2] - bottom, left:t.shape[3] - right]
    return out


def reflect_pad(x: torch.Tensor) -> torch.Tensor:
    """RealESRGANer's mod-2 rule: one reflected row / column at the bottom / right of an odd H / W."""
    h, w = x.shape[2:]
    return F.pad(x, (0, w % 2, 0, h % 2), mode="reflect") if (h % 2 or w % 2) else x


@torch.no_grad()
def enhance_float(img_u8: np.ndarray, sd, num_block: int, tile_size: int = 256, tile_pad: int = 10,
                  force_tiled: bool = False) -> np.ndarray:
    """HxWx3 u8 -> 2Hx2Wx3 float32 before quantisation: reflect pad, whole image when Hp*Wp <= tile^2*4 (strict '>' on the padded
    sizes, as RealESRGAN.enhance), else (or with force_tiled: `_tile_process` alone) the windows; cropped to 2H x 2W."""
    H, W, _ = img_u8.shape
    x = reflect_pad(torch.from_numpy(img_u8.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0))
    hp, wp = x.shape[2:]
    if force_tiled or hp * wp > tile_size * tile_size * 4:
        o = tile_process(x, sd, num_block, tile_size, tile_pad)
    else:
        o = forward(x, sd, num_block)
    return o[0, :, :2 * H, :2 * W].permute(1, 2, 0).numpy()


def enhance(img_u8: np.ndarray, sd, num_block: int, tile_size: int = 256, tile_pad: int = 10) -> np.ndarray:
    """`RealESRGAN.enhance` at scale 2: HxWx3 u8 -> 2Hx2Wx3 u8 (truncating quantisation)."""
    return (enhance_float(img_u8, sd, num_block, tile_size, tile_pad) * 255.0).clip(0, 255).astype(np.uint8)


def expected_p0(tiles, geo):
    """The unshuffled integers at the positions the packer writes (plain images or a mosaic), zeros everywhere else."""
    B, th, tw, _ = tiles.shape
    n, Hp, Wp = geo["n"], geo["Hp"][0], geo["Wp"][0]
    p0 = np.zeros((n, 16, Hp, Wp), np.float64)
    un = torch.nn.functional.pixel_unshuffle(torch.from_numpy(tiles.transpose(0, 3, 1, 2).astype(np.float64)), 2).numpy()
    kx, ky = (geo["mos_kx"], geo["mos_ky"]) if geo["mos_kx"] else (1, 1)
    h, w = th // 2, tw // 2
    for t in range(B):
        i, slot = divmod(t, kx * ky)
        wy, wx = divmod(slot, kx)
        y0, x0 = 1 + wy * (h + 1), 1 + wx * (w + 1)
        p0[i, :12, y0:y0 + h, x0:x0 + w] = un[t]
    return p0
