#!/usr/bin/env python3
"""Generate tests/golden/g9_x2plus.npz (RealESRGAN_x2plus) by running the REFERENCE implementation in this container.

Same recipe as tools/make_golden.py: the reference's `RRDBNet` and `RealESRGAN` (server/app/cnn_super_resolution.py) are imported
with an empty `cv2` stub, seeded weights of this repo's generator (`synthetic_state_dict(..., scale=2)`) are loaded with
`load_state_dict(strict=True)`, and nothing of the reference's text is copied.

RealESRGAN_x2plus is basicsr's RRDBNet(num_in_ch=3, scale=2), which runs `F.pixel_unshuffle(x, 2)` and then the x4 net with a
12-channel conv_first.  The reference's own class spells that as `RRDBNet(num_in_ch=12, scale=4)` applied to the unshuffled
image; that is the model here.  `RealESRGAN.enhance` and `_tile_process` are called unbound on a duck-typed object whose `.model`
is that composition and whose `.scale` is 2.  The odd-size reflect pad has no counterpart in the reference (it never runs x2):
only tests/x2plus_model.py pins it.

Fixtures are DATA only: inputs and expected outputs.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sentinel2-super-resolution-poc_amd"))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/server")
sys.modules.setdefault("cv2", types.ModuleType("cv2"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from app.cnn_super_resolution import RRDBNet, RealESRGAN  # noqa: E402
from s2sr.weights import synthetic_state_dict  # noqa: E402

OUT = REPO / "tests" / "golden"
torch.set_num_threads(8)


def make_net(num_block, seed=0):
    net = RRDBNet(num_in_ch=12, num_out_ch=3, num_feat=64, num_block=num_block, num_grow_ch=32, scale=4)
    sd = synthetic_state_dict(num_block, seed=seed, scale=2)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return net.eval()


class Unshuffled(torch.nn.Module):
    """RealESRGAN_x2plus: pixel_unshuffle by 2, then the 12-channel net."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        return self.net(F.pixel_unshuffle(x, 2))


class Wrapper:
    """Duck-typed stand-in for a constructed RealESRGAN (its __init__ downloads weights)."""

    def __init__(self, model, tile_size, tile_pad):
        self.model, self.scale, self.device = model, 2, torch.device("cpu")
        self.tile_size, self.tile_pad = tile_size, tile_pad
        self._tile_process = lambda img: RealESRGAN._tile_process(self, img)


@torch.no_grad()
def main():
    g = np.random.Generator(np.random.PCG64(9))
    out = {}
    # the net on F.pixel_unshuffle of a [2, 3, 24, 32] input (u8 / 255, as the x4 goldens), 1 / 2 / 23 blocks
    u = g.integers(0, 256, size=(2, 24, 32, 3), dtype=np.uint8)
    x = (u.astype(np.float32) / 255.0).transpose(0, 3, 1, 2).copy()
    out["net_u8"], out["net_x"] = u, x
    for nb in (1, 2, 23):
        out[f"net_b{nb}"] = Unshuffled(make_net(nb))(torch.from_numpy(x)).numpy()
    # RealESRGAN.enhance, whole-image branch: 40 x 56 u8, 23 blocks, tile_size 256
    img = g.integers(0, 256, size=(40, 56, 3), dtype=np.uint8)
    m23 = Unshuffled(make_net(23))
    out["enh_img"] = img
    out["enh_u8"] = RealESRGAN.enhance(Wrapper(m23, 256, 10), img)
    xt = torch.from_numpy(img.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    out["enh_f32"] = m23(xt).squeeze(0).permute(1, 2, 0).numpy()
    # _tile_process, tile_size 16, tile_pad 2 on 38 x 46 (float input), 1-block net
    timg = g.integers(0, 256, size=(38, 46, 3), dtype=np.uint8)
    out["tiled_img"] = timg
    tt = torch.from_numpy(timg.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    out["tiled_f32"] = Wrapper(Unshuffled(make_net(1)), 16, 2)._tile_process(tt).numpy()
    path = OUT / "g9_x2plus.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
