"""Weight handling for the RRDBNet x4 / x2 path and the SRVGGNetCompact x4 path: canonical conv order, state-dict <-> flat
fp32 blob, and the deterministic synthetic-weight generator used by tests and bench.

The reference stores weights as a torch state-dict whose keys are fixed by
`RRDBNet.__init__` (reference server/app/cnn_super_resolution.py:125-136, keys
`conv_first.*`, `body.{i}.rdb{1,2,3}.conv{1..5}.*`, `conv_body.*`, `conv_up1.*`,
`conv_up2.*`, `conv_hr.*`, `conv_last.*`; 702 tensors for 23 blocks).  The native
library takes ONE flat little-endian fp32 blob: for every conv in `conv_specs()`
order, `weight[Cout,Cin,3,3]` (OIHW, row-major) followed by `bias[Cout]`.  The
library re-packs that blob itself (fp16 MFMA fragment order) -- nothing here knows
about device layouts.

No pretrained weights exist offline, so `synthetic_state_dict`
produces seeded weights of the exact RealESRGAN_x4plus / anime_6B shapes from a
splitmix64 counter stream.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Iterable, List, Tuple

import numpy as np

NUM_FEAT = 64
NUM_GROW = 32

# reference server/app/cnn_super_resolution.py:28-45 (model table; URLs are not used here,
# there is no network path in this build)
MODEL_TABLE = {
    "realesrgan_x4": {"scale": 4, "channels": 64, "blocks": 23, "num_in_ch": 3},
    "realesrgan_anime": {"scale": 4, "channels": 64, "blocks": 6, "num_in_ch": 3},
    # RealESRGAN_x2plus: basicsr RRDBNet(num_in_ch=3, scale=2) = pixel_unshuffle(x, 2), a 12-channel conv_first, then the x4 body
    # and tail on the half grid.  Not in the drop-in's MODELS (the reference's table); app.cnn_super_resolution.EXTRA_MODELS
    "realesrgan_x2plus": {"scale": 2, "channels": 64, "blocks": 23, "num_in_ch": 3},
    # SRVGGNetCompact(num_feat=64, num_conv, upscale=4, act_type="prelu"): Real-ESRGAN's small models ("arch": "compact";
    # entries without the key are RRDBNet).  The wdn twin is the denoise end of `dni` (denoise_strength).
    "realesr_general_x4v3": {"scale": 4, "channels": 64, "arch": "compact", "num_conv": 32, "num_in_ch": 3},
    "realesr_general_wdn_x4v3": {"scale": 4, "channels": 64, "arch": "compact", "num_conv": 32, "num_in_ch": 3},
    "realesr_animevideov3": {"scale": 4, "channels": 64, "arch": "compact", "num_conv": 16, "num_in_ch": 3},
}


def first_conv_cin(scale: int) -> int:
    """Input channels of conv_first: 3, or 12 at scale 2 (the channels of pixel_unshuffle(x, 2))."""
    if scale not in (2, 4):
        raise ValueError(f"scale {scale}: the native path runs scale 4 and RealESRGAN_x2plus (scale 2)")
    return 12 if scale == 2 else 3


def conv_specs(num_block: int, num_feat: int = NUM_FEAT, num_grow: int = NUM_GROW,
               num_in_ch: int = 3, num_out_ch: int = 3) -> List[Tuple[str, int, int, bool]]:
    """Canonical conv order: list of (state-dict prefix, Cin, Cout, is_body).

    Order == module registration order in the reference (`cnn_super_resolution.py:125-136`),
    which is also the order of `state_dict()` keys.
    """
    specs: List[Tuple[str, int, int, bool]] = [("conv_first", num_in_ch, num_feat, False)]
    for b in range(num_block):
        for r in (1, 2, 3):
            for k in range(1, 6):
                cin = num_feat + (k - 1) * num_grow
                cout = num_grow if k < 5 else num_feat
                specs.append((f"body.{b}.rdb{r}.conv{k}", cin, cout, True))
    specs.append(("conv_body", num_feat, num_feat, False))
    specs.append(("conv_up1", num_feat, num_feat, False))
    specs.append(("conv_up2", num_feat, num_feat, False))
    specs.append(("conv_hr", num_feat, num_feat, False))
    specs.append(("conv_last", num_feat, num_out_ch, False))
    return specs


def num_params(num_block: int, scale: int = 4) -> int:
    return sum(ci * co * 9 + co for _, ci, co, _ in conv_specs(num_block, num_in_ch=first_conv_cin(scale)))


# ----------------------------------------------------------------------------------------
# splitmix64 counter stream
# ----------------------------------------------------------------------------------------
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(seed: int, start: int, count: int) -> np.ndarray:
    """Outputs `start .. start+count-1` of the splitmix64 stream seeded with `seed` (uint64)."""
    with np.errstate(over="ignore"):
        n = np.arange(start + 1, start + count + 1, dtype=np.uint64)
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + n * _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    return z


def _uniform(seed: int, start: int, count: int) -> np.ndarray:
    """float64 uniform in [-1, 1) from the top 53 bits."""
    z = splitmix64(seed, start, count)
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0


def synthetic_state_dict(num_block: int = 23, seed: int = 0, body_gain: float = 0.3,
                         other_gain: float = 1.0, bias_amp: float = 0.01, scale: int = 4
                         ) -> "OrderedDict[str, np.ndarray]":
    """Seeded weights with RealESRGAN shapes (numpy fp32, state-dict key order).

    weights ~ U(-a, a), a = gain * sqrt(1 / (9 * Cin)); body (RDB) convs use `body_gain`
    (0.3 -- mirrors ESRGAN's scaled-down residual-branch init), the rest `other_gain`;
    biases ~ U(-bias_amp, bias_amp).  One contiguous counter stream, tensors consumed in
    `conv_specs` order (weight then bias), so any prefix of the net is reproducible.
    scale=2: RealESRGAN_x2plus shapes (conv_first.weight [64, 12, 3, 3]; the stream runs on from there).
    """
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    pos = 0
    for name, cin, cout, is_body in conv_specs(num_block, num_in_ch=first_conv_cin(scale)):
        a = (body_gain if is_body else other_gain) * np.sqrt(1.0 / (9.0 * cin))
        n_w = cout * cin * 9
        sd[name + ".weight"] = (_uniform(seed, pos, n_w) * a).astype(np.float32).reshape(cout, cin, 3, 3)
        pos += n_w
        sd[name + ".bias"] = (_uniform(seed, pos, cout) * bias_amp).astype(np.float32)
        pos += cout
    return sd


# ----------------------------------------------------------------------------------------
# SRVGGNetCompact: a flat nn.ModuleList `body` of conv / PReLU alternating, then the last conv
# ----------------------------------------------------------------------------------------
COMPACT_UPSCALE = 4


def compact_specs(num_conv: int = 32, num_feat: int = NUM_FEAT, num_in_ch: int = 3, num_out_ch: int = 3,
                  upscale: int = COMPACT_UPSCALE) -> List[Tuple[str, Tuple[int, ...]]]:
    """State-dict order of SRVGGNetCompact: list of (key, shape).  body.0 = first conv, body.1 = its PReLU (64 slopes),
    then conv / PReLU alternating `num_conv` times, last conv body.{2*num_conv+2} with num_out_ch * upscale^2 outputs."""
    specs: List[Tuple[str, Tuple[int, ...]]] = []
    cin = num_in_ch
    for i in range(num_conv + 1):
        specs.append((f"body.{2 * i}.weight", (num_feat, cin, 3, 3)))
        specs.append((f"body.{2 * i}.bias", (num_feat,)))
        specs.append((f"body.{2 * i + 1}.weight", (num_feat,)))
        cin = num_feat
    last = 2 * num_conv + 2
    specs.append((f"body.{last}.weight", (num_out_ch * upscale * upscale, num_feat, 3, 3)))
    specs.append((f"body.{last}.bias", (num_out_ch * upscale * upscale,)))
    return specs


def num_params_compact(num_conv: int = 32) -> int:
    return int(sum(int(np.prod(shape)) for _, shape in compact_specs(num_conv)))


def infer_arch(keys: Iterable[str]) -> Tuple[str, int]:
    """("rrdb", num_block) or ("compact", num_conv) from state-dict keys: a flat `body.<i>.weight` list without `conv_first`
    is SRVGGNetCompact, its num_conv from the largest index (2 * num_conv + 2)."""
    keys = list(keys)
    if "conv_first.weight" not in keys and "body.0.weight" in keys:
        last = max(int(k.split(".")[1]) for k in keys if k.startswith("body."))
        if last < 4 or last % 2:
            raise ValueError(f"compact state dict: last body index {last} is not 2 * num_conv + 2")
        return "compact", (last - 2) // 2
    return "rrdb", infer_num_block(keys)


def synthetic_compact_state_dict(num_conv: int = 32, seed: int = 0, body_gain: float = 0.90, first_gain: float = 1.0,
                                 last_gain: float = 0.3, bias_amp: float = 0.05, slope_lo: float = 0.05, slope_hi: float = 0.35,
                                 zero_mean: bool = False) -> "OrderedDict[str, np.ndarray]":
    """Seeded SRVGGNetCompact weights on the splitmix64 stream, tensors consumed in `compact_specs` order.

    Conv weights ~ U(-a, a) with the Kaiming-uniform bound a = gain * sqrt(6 / (9 * Cin)) (first / body / last gains), biases
    ~ U(-bias_amp, bias_amp), PReLU slopes ~ U(slope_lo, slope_hi).  The body gain decides whether 33 layers of fp16
    activations stay inside the project's tolerance (tests/test_compact_cpu.py guards it): at 1.0 the activations grow layer
    by layer, well below 0.9 the body's contribution fades.  zero_mean: every output channel of a 64 -> 64 conv has the mean of
    its 576 weights removed -- PReLU outputs have a positive mean that such a sum turns into a per-channel offset, and 32 layers
    deep the offset keeps some channels' pre-activations one-signed; without it every channel sees both signs at every depth
    (the per-layer device tests want negative pre-activations in every channel)."""
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    pos = 0
    specs = compact_specs(num_conv)
    last_w = specs[-2][0]
    for key, shape in specs:
        n = int(np.prod(shape))
        u = _uniform(seed, pos, n)
        pos += n
        if len(shape) == 4:
            gain = first_gain if key == "body.0.weight" else (last_gain if key == last_w else body_gain)
            v = u * (gain * np.sqrt(6.0 / (9.0 * shape[1])))
            if zero_mean and shape[1] == 64 and key != last_w:
                v = v.reshape(shape[0], -1)
                v = v - v.mean(axis=1, keepdims=True)
        elif key.endswith(".bias"):
            v = u * bias_amp
        else:
            v = slope_lo + (u + 1.0) * 0.5 * (slope_hi - slope_lo)
        sd[key] = v.astype(np.float32).reshape(shape)
    return sd


def dni(sd_a, sd_b, strength: float) -> "OrderedDict[str, np.ndarray]":
    """Deep network interpolation (Real-ESRGAN's denoise_strength): strength * a + (1 - strength) * b per key, fp32.
    Upstream calls it as dni(x4v3, wdn_x4v3, denoise_strength)."""
    strength = float(strength)
    if not (0.0 <= strength <= 1.0):
        raise ValueError(f"dni strength {strength} outside [0, 1]")
    if set(sd_a.keys()) != set(sd_b.keys()):
        raise ValueError("dni: the two state dicts have different keys")
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    s, r = np.float32(strength), np.float32(1.0 - strength)
    for k in sd_a.keys():
        a = np.asarray(_to_numpy(sd_a[k]), dtype=np.float32)
        b = np.asarray(_to_numpy(sd_b[k]), dtype=np.float32)
        if a.shape != b.shape:
            raise ValueError(f"dni: {k} has shapes {a.shape} and {b.shape}")
        out[k] = a.copy() if strength == 1.0 else (b.copy() if strength == 0.0 else (s * a + r * b).astype(np.float32))
    return out


def _flatten_compact(sd, num_conv: int | None) -> np.ndarray:
    arch, nc = infer_arch(sd.keys())
    if arch != "compact":
        raise KeyError("state_dict mismatch: not a SRVGGNetCompact state dict (no flat body.<i>.weight list)")
    if num_conv is None:
        num_conv = nc
    specs = compact_specs(num_conv)
    expected = {k for k, _ in specs}
    missing = sorted(expected - set(sd.keys()))
    unexpected = sorted(set(sd.keys()) - expected)
    if missing or unexpected:
        raise KeyError(f"state_dict mismatch: missing={missing[:4]}... unexpected={unexpected[:4]}...")
    parts = []
    for key, shape in specs:
        t = _to_numpy(sd[key])
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{key}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        parts.append(np.ascontiguousarray(t, dtype=np.float32).ravel())
    return np.concatenate(parts)


def infer_num_block(keys: Iterable[str]) -> int:
    blocks = {int(k.split(".")[1]) for k in keys if k.startswith("body.")}
    return (max(blocks) + 1) if blocks else 0


def select_params(obj):
    """`params_ema` -> `params` -> bare state-dict (reference cnn_super_resolution.py:205-209)."""
    if isinstance(obj, dict):
        if "params_ema" in obj:
            return obj["params_ema"]
        if "params" in obj:
            return obj["params"]
    return obj


def infer_scale(sd) -> int:
    """2 when conv_first reads 12 channels (RealESRGAN_x2plus), else 4."""
    w = sd.get("conv_first.weight")
    return 2 if w is not None and len(w.shape) == 4 and w.shape[1] == 12 else 4


def flatten_state_dict(sd: Dict[str, "np.ndarray"], num_block: int | None = None, scale: int | None = None,
                       arch: str | None = None) -> np.ndarray:
    """State-dict (numpy arrays or torch tensors) -> the flat fp32 blob of the C ABI.

    `arch` (None: from the keys, `infer_arch`): "compact" = SRVGGNetCompact, `num_block` then carries num_conv and the blob
    is the flat `body` list in `compact_specs` order (conv weight, conv bias, slopes, ...).

    Raises KeyError / ValueError on missing, unexpected or mis-shaped tensors -- the same
    failures `load_state_dict(strict=True)` reports (reference cnn_super_resolution.py:211).
    `scale` (None: from conv_first's shape) picks the layout: 2 = RealESRGAN_x2plus (conv_first 12 -> 64).
    """
    if arch is None:
        arch = infer_arch(sd.keys())[0]
    if arch == "compact":
        return _flatten_compact(sd, num_block)
    if arch != "rrdb":
        raise ValueError(f"unknown arch {arch!r}")
    if num_block is None:
        num_block = infer_num_block(sd.keys())
    if scale is None:
        scale = infer_scale(sd)
    specs = conv_specs(num_block, num_in_ch=first_conv_cin(scale))
    expected = {p + s for p, _, _, _ in specs for s in (".weight", ".bias")}
    missing = sorted(expected - set(sd.keys()))
    unexpected = sorted(set(sd.keys()) - expected)
    if missing or unexpected:
        raise KeyError(f"state_dict mismatch: missing={missing[:4]}... unexpected={unexpected[:4]}...")
    parts = []
    for name, cin, cout, _ in specs:
        w = _to_numpy(sd[name + ".weight"])
        b = _to_numpy(sd[name + ".bias"])
        if w.shape != (cout, cin, 3, 3) or b.shape != (cout,):
            raise ValueError(f"{name}: expected weight {(cout, cin, 3, 3)} bias {(cout,)}, "
                             f"got {w.shape} {b.shape}")
        parts.append(np.ascontiguousarray(w, dtype=np.float32).ravel())
        parts.append(np.ascontiguousarray(b, dtype=np.float32).ravel())
    return np.concatenate(parts)


def _to_numpy(t) -> np.ndarray:
    if isinstance(t, np.ndarray):
        return t
    return t.detach().to("cpu").float().numpy()
