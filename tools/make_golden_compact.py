#!/usr/bin/env python3
"""Generate tests/golden/g10_compact.npz (SRVGGNetCompact: realesr-general-x4v3 / realesr-animevideov3 shapes).

The reference tree holds no SRVGGNetCompact, so unlike g9 the NET of this golden cannot come from the reference's classes.  It is
written here a second time, independently of tests/compact_model.py (which is functional code on the raw arrays): an `nn.Module`
of `nn.ModuleList([nn.Conv2d, nn.PReLU, ...])`, `nn.PixelShuffle` and `F.interpolate(mode="nearest")`, loaded with
`load_state_dict(strict=True)` from this repo's seeded generator (`synthetic_compact_state_dict`) and run in float64.  What does
come from the reference is everything around the net: its own `RealESRGAN.enhance` and `_tile_process`
(server/app/cnn_super_resolution.py) are called unbound on a duck-typed object whose `.model` is that module, as
tools/make_golden_x2plus.py does.  Nothing of the reference's text is copied.

    python tools/make_golden_compact.py --reference <path to the reference checkout>

Fixtures are DATA only: inputs, expected outputs and the SHA-256 of the seeded weight blobs (not the weights: 4.8 MB).
"""
from __future__ import annotations

import argparse
import hashlib
import sys
import types
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.dont_write_bytecode = True

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

OUT = REPO / "tests" / "golden"
torch.set_num_threads(8)


class CompactNet(nn.Module):
    """SRVGGNetCompact(3, 3, 64, num_conv, upscale=4, act_type="prelu"), float64."""

    def __init__(self, num_conv):
        super().__init__()
        self.body = nn.ModuleList([nn.Conv2d(3, 64, 3, 1, 1), nn.PReLU(num_parameters=64)])
        for _ in range(num_conv):
            self.body.append(nn.Conv2d(64, 64, 3, 1, 1))
            self.body.append(nn.PReLU(num_parameters=64))
        self.body.append(nn.Conv2d(64, 3 * 16, 3, 1, 1))
        self.upsampler = nn.PixelShuffle(4)

    def forward(self, x):
        x = x.double()
        out = x
        for m in self.body:
            out = m(out)
        return self.upsampler(out) + F.interpolate(x, scale_factor=4, mode="nearest")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (its server/ directory is imported)")
    args = ap.parse_args()
    sys.path.insert(0, str(REPO / "sentinel2-super-resolution-poc_amd"))
    from s2sr.weights import flatten_state_dict, synthetic_compact_state_dict
    for name in [k for k in sys.modules if k == "app" or k.startswith("app.")]:
        del sys.modules[name]
    sys.path.insert(0, str(Path(args.reference) / "server"))
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from app.cnn_super_resolution import RealESRGAN   # the REFERENCE's class (its path was put in front)
    assert Path(sys.modules["app.cnn_super_resolution"].__file__).resolve().is_relative_to(Path(args.reference).resolve())

    def make_net(num_conv, seed=0):
        net = CompactNet(num_conv).double()
        sd = synthetic_compact_state_dict(num_conv, seed=seed)
        net.load_state_dict({k: torch.from_numpy(v.copy()).double() for k, v in sd.items()}, strict=True)
        return net.eval(), sd

    class Wrapper:
        """Duck-typed stand-in for a constructed RealESRGAN (its __init__ downloads weights)."""

        def __init__(self, model, tile_size, tile_pad):
            self.model, self.scale, self.device = model, 4, torch.device("cpu")
            self.tile_size, self.tile_pad = tile_size, tile_pad
            self._tile_process = lambda img: RealESRGAN._tile_process(self, img)

    with torch.no_grad():
        g = np.random.Generator(np.random.PCG64(10))
        out = {}
        u = g.integers(0, 256, size=(1, 20, 24, 3), dtype=np.uint8)
        x = (u.astype(np.float32) / 255.0).transpose(0, 3, 1, 2).copy()
        out["net_u8"], out["net_x"] = u, x
        for nc in (16, 32):
            net, sd = make_net(nc)
            out[f"net_c{nc}"] = net(torch.from_numpy(x)).numpy().astype(np.float32)
            out[f"blob_sha256_c{nc}"] = np.array(hashlib.sha256(flatten_state_dict(sd).tobytes()).hexdigest())
        # RealESRGAN.enhance, whole-image branch: 28 x 36 u8, 32 convs, tile_size 256 (the golden's largest image)
        net32, _ = make_net(32)
        img = g.integers(0, 256, size=(28, 36, 3), dtype=np.uint8)
        out["enh_img"] = img
        out["enh_u8"] = RealESRGAN.enhance(Wrapper(net32, 256, 10), img)
        # _tile_process, tile_size 8, tile_pad 2 on 22 x 26, 16 convs; and enhance's tiled branch on the same image (22*26 > 8*8*4)
        net16, _ = make_net(16)
        timg = g.integers(0, 256, size=(22, 26, 3), dtype=np.uint8)
        out["tiled_img"] = timg
        tt = torch.from_numpy(timg.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
        out["tiled_f32"] = Wrapper(net16, 8, 2)._tile_process(tt).numpy().astype(np.float32)
        out["tiled_enh_u8"] = RealESRGAN.enhance(Wrapper(net16, 8, 2), timg)
    path = OUT / "g10_compact.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
