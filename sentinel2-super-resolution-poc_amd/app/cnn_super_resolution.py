"""Drop-in for the reference module `app.cnn_super_resolution`
(reference server/app/cnn_super_resolution.py): same public names, constructor arguments,
attributes and error behaviour, but every pixel is computed by libs2sr.so on an MI355X.

    RealESRGAN(scale=4, device=None, tile_size=256, model_name=None).enhance(img) -> img x4

Differences a maintainer should know (all deliberate):
  * there is no CPU path: `device="cpu"` (or a box without a gfx950 GPU) raises RuntimeError
    instead of silently running for minutes on the host (reference :174-177);
  * weights are never fetched from the network unless S2SR_ALLOW_DOWNLOAD=1; they are looked
    up as `<model dir>/<model_name>.pth` exactly like the reference (:48-70), and
    `state_dict=` may be passed directly (tests, synthetic benchmarks);
  * native engines are cached per (weights, device), so the reference's construct-per-job
    pattern (wow_sr.py:93-97) costs nothing after the first job.
"""
from __future__ import annotations

import hashlib
import os
import threading
import urllib.request
from pathlib import Path
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from s2sr import native
from s2sr.weights import MODEL_TABLE, compact_specs, conv_specs, dni, first_conv_cin, flatten_state_dict, select_params

# Model table -- keys and fields as in the reference (:28-45)
MODELS = {
    "realesrgan_x4": {
        "url": "https://github.com/xinntao/Real-ESRGAN/releases/download/v0.1.0/RealESRGAN_x4plus.pth",
        "description": "General photos (best quality)",
        **MODEL_TABLE["realesrgan_x4"],
    },
    "realesrgan_anime": {
        "url": "https://github.com/xinntao/Real-ESRGAN/releases/download/v0.2.2.4/RealESRGAN_x4plus_anime_6B.pth",
        "description": "Sharp edges (best for text/plates)",
        **MODEL_TABLE["realesrgan_anime"],
    },
}

# Models beyond the reference's table, resolved by name after MODELS (download_weights, RealESRGAN(model_name=...)).  MODELS stays
# the reference's, so RealESRGAN(scale=2) still looks up "realesrgan_x2" and fails as the reference does; a deployment serves
# x2plus by naming it.
EXTRA_MODELS = {
    "realesrgan_x2plus": {
        "url": "https://github.com/xinntao/Real-ESRGAN/releases/download/v0.2.1/RealESRGAN_x2plus.pth",
        "description": "Quick upscaling (less hallucination, 2x upscale)",
        **MODEL_TABLE["realesrgan_x2plus"],
    },
    # SRVGGNetCompact ("arch": "compact"): Real-ESRGAN's small x4 models, 2.42 MFLOP per input pixel against RRDBNet-23's 35.8.
    # realesr_general_x4v3 takes RealESRGAN(denoise_strength=s): dni(x4v3, wdn_x4v3, s), upstream's interpolation.
    "realesr_general_x4v3": {
        "url": "https://github.com/xinntao/Real-ESRGAN/releases/download/v0.2.5.0/realesr-general-x4v3.pth",
        "description": "General scenes, small and fast (SRVGGNetCompact, 1.2 M parameters)",
        **MODEL_TABLE["realesr_general_x4v3"],
    },
    "realesr_general_wdn_x4v3": {
        "url": "https://github.com/xinntao/Real-ESRGAN/releases/download/v0.2.5.0/realesr-general-wdn-x4v3.pth",
        "description": "General scenes, small and fast, with denoising (the other end of denoise_strength)",
        **MODEL_TABLE["realesr_general_wdn_x4v3"],
    },
    "realesr_animevideov3": {
        "url": "https://github.com/xinntao/Real-ESRGAN/releases/download/v0.2.5.0/realesr-animevideov3.pth",
        "description": "Anime video, smallest (SRVGGNetCompact, 16 convs)",
        **MODEL_TABLE["realesr_animevideov3"],
    },
}
DNI_MODEL, DNI_WDN_MODEL = "realesr_general_x4v3", "realesr_general_wdn_x4v3"


def model_config(model_name: str) -> Optional[dict]:
    """The table entry of `model_name`: MODELS first, then EXTRA_MODELS; None when neither has it."""
    return MODELS.get(model_name) or EXTRA_MODELS.get(model_name)


def get_model_dir() -> Path:
    """`server/models` next to the app package, or $S2SR_MODEL_DIR (reference :48-52)."""
    d = Path(os.environ.get("S2SR_MODEL_DIR", Path(__file__).resolve().parent.parent / "models"))
    d.mkdir(parents=True, exist_ok=True)
    return d


def download_weights(model_name: str) -> Path:
    """Path of `<model_name>.pth`; ValueError for unknown names (reference :55-70).  Names resolve in MODELS, then EXTRA_MODELS."""
    config = model_config(model_name)
    if config is None:
        raise ValueError(f"Unknown model: {model_name}")
    path = get_model_dir() / f"{model_name}.pth"
    if not path.exists():
        if os.environ.get("S2SR_ALLOW_DOWNLOAD") == "1":
            print(f"Downloading {model_name} weights...")
            urllib.request.urlretrieve(config["url"], path)
        else:
            raise FileNotFoundError(
                f"{path} not found and network download is disabled (set S2SR_ALLOW_DOWNLOAD=1 to fetch "
                f"{config['url']}, or place the file there)")
    return path


# ------------------------------------------------------------------------------------------
# Parameter containers with the reference's state-dict layout.  They hold weights only;
# the arithmetic of ResidualDenseBlock / RRDB / RRDBNet.forward lives in csrc/.
# ------------------------------------------------------------------------------------------
def _attach(root: nn.Module, dotted: str, leaf: nn.Module) -> None:
    parts = dotted.split(".")
    node = root
    for name in parts[:-1]:
        if not hasattr(node, name):
            node.add_module(name, nn.Module())
        node = getattr(node, name)
    node.add_module(parts[-1], leaf)


class RRDBNet(nn.Module):
    """Shape-compatible with the reference RRDBNet (:110-158): `load_state_dict(strict=True)`
    accepts RealESRGAN_x4plus / anime_6B checkpoints.  `forward` runs on the GPU engine.

    num_in_ch=12 (with scale=4, the reference class's own spelling of it) holds RealESRGAN_x2plus: that checkpoint is
    RRDBNet(num_in_ch=12, scale=4) applied to pixel_unshuffle(x, 2).  Its `forward` takes the [N,3,H,W] image (the unshuffle
    runs on the device) and returns [N,3,2H,2W]; `scale` is then 2.  The reference's one-upsample scale=2 branch stays refused."""

    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=64, num_block=23, num_grow_ch=32, scale=4):
        super().__init__()
        if num_in_ch not in (3, 12) or (num_out_ch, num_feat, num_grow_ch, scale) != (3, 64, 32, 4):
            raise ValueError("the native path is built for num_in_ch=3 (or 12: RealESRGAN_x2plus), num_out_ch=3, num_feat=64, "
                             "num_grow_ch=32, scale=4 (the shapes in MODELS and EXTRA_MODELS)")
        self.scale = 2 if num_in_ch == 12 else 4
        self.arch = "rrdb"
        self.num_block = num_block
        for name, cin, cout, _ in conv_specs(num_block, num_in_ch=num_in_ch):
            _attach(self, name, nn.Conv2d(cin, cout, 3, 1, 1))
        self._engine: Optional[native.Engine] = None
        self._engine_key = None

    # -- engine management ------------------------------------------------------------------
    def _fingerprint(self) -> str:
        h = hashlib.sha1()
        for k, v in self.state_dict().items():
            h.update(k.encode())
            t = v.detach().cpu().contiguous()
            h.update(t.numpy().tobytes()[:4096])
            h.update(str(float(t.double().sum())).encode())
        return h.hexdigest()

    def _version(self):
        """Cheap change detector: torch bumps a tensor's _version on every in-place write."""
        return tuple((id(p), p._version) for p in self.parameters())

    def engine(self, device_index: int = 0) -> native.Engine:
        ver = self._version()
        prec = _precision_override() or os.environ.get("S2SR_PRECISION", "hp")
        if self._engine is not None and self._engine_key is not None and self._engine_key[1:] == (device_index, ver, prec):
            return self._engine
        fp = self._fingerprint()
        self._engine = _engine_for(self.state_dict(), self.num_block, device_index, fp, self.scale, self.arch)
        self._engine_key = (fp, device_index, ver, prec)
        return self._engine

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[N,3,H,W] float in [0,1] -> [N,3,sH,sW] float32 (unclamped, s = self.scale), computed on the GPU."""
        dev = x.device
        idx = dev.index if dev.type == "cuda" and dev.index is not None else 0
        y = self.engine(idx).forward_f32(x.detach().float().cpu().numpy())
        return torch.from_numpy(y).to(dev)


class SRVGGNetCompact(nn.Module):
    """Shape-compatible with Real-ESRGAN's SRVGGNetCompact(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv, upscale=4,
    act_type="prelu"): a flat `body` ModuleList of conv / PReLU(64) alternating and the last conv, so
    `load_state_dict(strict=True)` accepts realesr-general-x4v3 / -wdn-x4v3 / realesr-animevideov3 checkpoints.  It holds
    weights only; `forward` runs on the GPU engine (pixel-shuffle and the nearest-x4 base add are in the last conv's stores)."""

    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=32, upscale=4, act_type="prelu"):
        super().__init__()
        if (num_in_ch, num_out_ch, num_feat, upscale, act_type) != (3, 3, 64, 4, "prelu") or num_conv not in (16, 32):
            raise ValueError("the native path is built for SRVGGNetCompact(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv in "
                             "{16, 32}, upscale=4, act_type='prelu')")
        self.scale = 4
        self.arch = "compact"
        self.num_block = num_conv          # what native.Engine carries in num_block
        self.body = nn.ModuleList()
        for key, shape in compact_specs(num_conv):
            if key.endswith(".bias"):
                continue
            self.body.append(nn.Conv2d(shape[1], shape[0], 3, 1, 1) if len(shape) == 4 else nn.PReLU(num_parameters=shape[0]))
        self._engine: Optional[native.Engine] = None
        self._engine_key = None

    _fingerprint = RRDBNet._fingerprint
    _version = RRDBNet._version
    engine = RRDBNet.engine
    forward = RRDBNet.forward


_ENGINES: Dict[Tuple[str, int], native.Engine] = {}
_ENGINES_LOCK = threading.Lock()
_LOADED_MODELS: Dict[tuple, "RRDBNet"] = {}      # checkpoint file identity -> loaded parameter shell
_MODELS_LOCK = threading.Lock()


def _engine_for(state_dict, num_block: int, device_index: int, fingerprint: str, scale: int = 4, arch: str = "rrdb") -> native.Engine:
    """One native handle per (weights, scale, GPU), shared by every RealESRGAN object of the process."""
    with _ENGINES_LOCK:
        key = (fingerprint, device_index, _precision_override() or os.environ.get("S2SR_PRECISION", "hp"), scale, arch)
        eng = _ENGINES.get(key)
        if eng is None:
            # S2SR_PRECISION=fast trades the <=1e-4 parity of the default for ~14 % more throughput; =fp8 runs the RDB
            # trunk on e4m3 operands (BASELINE configs[4], ~1.5x, max-abs ~5e-3: outside the 1e-3 tolerance)
            prec = {"fast": native.PREC_F16, "fp8": native.PREC_FP8}.get(_precision_override() or
                                                                          os.environ.get("S2SR_PRECISION", "hp"), native.PREC_F16_HP)
            if arch == "compact" and prec == native.PREC_FP8:
                prec = native.PREC_F16      # the compact arch has one arithmetic (fp16 operands, fp32 accumulate); no fp8 form of it
            eng = native.Engine(num_block=num_block, device=device_index, precision=prec,
                                group=int(os.environ.get("S2SR_GROUP", "0")), scale=scale, arch=arch)
            eng.load_blob(flatten_state_dict(state_dict, num_block, scale=scale, arch=arch))
            if arch == "rrdb" and prec == native.PREC_FP8 and not (os.environ.get("S2SR_FP8_XEXP") or os.environ.get("S2SR_FP8_GEXP")):
                # activation scales of the fp8 trunk from data: a few imagery-like tiles through THIS checkpoint
                from s2sr.synth import synthetic_tiles
                eng.calibrate_fp8(synthetic_tiles(4, 64, seed=0), headroom=2.0)
            _ENGINES[key] = eng
        return eng


_THREAD = threading.local()


class thread_precision:
    """`with thread_precision("fp8"):` -- engines built for jobs on this thread use that arithmetic
    (app.farm_sr selects the /api/sr path onto the fp8 trunk with S2SR_FARM_PRECISION=fp8)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = getattr(_THREAD, "precision", None)
        _THREAD.precision = self.name
        return self

    def __exit__(self, *exc):
        _THREAD.precision = self.prev
        return False


def _precision_override():
    return getattr(_THREAD, "precision", None)


class thread_device:
    """`with thread_device(i):` -- jobs started on this thread resolve `device=None` to GPU i.  The
    reference's callers never pass a device (wow_sr.py:93, farm_sr.py:162), so this is how the admission
    queue (app.sr_routes.GpuAdmission) puts a job on the GPU it was admitted to."""

    def __init__(self, index: int):
        self.index = int(index)

    def __enter__(self):
        self.prev = getattr(_THREAD, "device", None)
        _THREAD.device = self.index
        return self

    def __exit__(self, *exc):
        _THREAD.device = self.prev
        return False


def current_device_index() -> int:
    d = getattr(_THREAD, "device", None)
    return int(os.environ.get("LOCAL_RANK", "0")) if d is None else d


def _resolve_device(device) -> torch.device:
    if device is None:
        return torch.device("cuda", current_device_index())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"device {device!r}: this build runs the network on an MI355X only; "
                           "there is no CPU fallback")
    return dev if dev.index is not None else torch.device("cuda", 0)


class Product16(NamedTuple):
    """What RealESRGAN.product16 makes of one image; a part that was not asked for is None."""
    out16: np.ndarray                        # uint16 [4H, 4W, 3], always
    display: Optional[np.ndarray] = None     # display=: uint8 [4H, 4W, 3], the 8-bit rendering of out16
    info: Optional[dict] = None              # display=: the stretch with the limits it found
    carried: Optional[np.ndarray] = None     # extra=: uint16 [4H, 4W, k], the carried bands
    carried_record: Optional[dict] = None    # extra=: their ranges, eps and inexact blocks, the weights and r (RealESRGAN.last_extra)
    indices: Optional[list] = None           # indices=: one dict per index (native.Engine.index_nd_u16)
    inexact_blocks: Optional[list] = None    # consistency: the blocks per band a clip kept off (RealESRGAN.last_inexact_blocks)


class RealESRGAN:
    """Real-ESRGAN inference wrapper with the reference's interface (:161-280)."""

    def __init__(self, scale: int = 4, device: str = None, tile_size: int = 256, model_name: str = None,
                 state_dict=None, denoise_strength: Optional[float] = None, seam_blend: bool = False, consistency=None):
        """consistency (not in the reference): None, "exact" or "smooth" -- one back-projection step on the quantised
        image (s2sr_enhance_consistent_*), so that the mean of the scale x scale output samples over an input pixel is that pixel
        again; honoured by enhance, enhance16 and enhance_job, with or without valid / nodata.  last_inexact_blocks: the blocks per
        band of the last such call that a clip kept off (None before one).
        seam_blend (not in the reference): tiled images are stitched with the cross-faded paste (s2sr_enhance_blend_*) -- the
        same windows and forwards, the window overlaps blended over a ramp around every tile line in place of the hard crop.
        denoise_strength (realesr_general_x4v3 only, upstream's knob): s in [0, 1] loads realesr_general_x4v3.pth and
        realesr_general_wdn_x4v3.pth and runs dni(x4v3, wdn, s) = s * x4v3 + (1 - s) * wdn: 1 = no denoising, 0 = the wdn model."""
        self.tile_size = tile_size
        self.tile_pad = 10
        self.seam_blend = bool(seam_blend)
        from s2sr.consistency import mode_of
        self.consistency = consistency
        self._cmode = mode_of(consistency)           # refuses an unknown name here, before anything is created
        self.last_inexact_blocks = None
        self.last_extra = None                # enhance16(extra=...): the ranges, eps and inexact blocks of the carried bands
        self.device = _resolve_device(device)
        print(f"   Device: {self.device}")

        if model_name is None:
            model_name = f"realesrgan_x{scale}"
        config = model_config(model_name)
        if config is None:
            raise ValueError(f"Unknown model: {model_name}. Available: {list(MODELS.keys())}")
        self.scale = config["scale"]
        self.model_name = model_name
        compact = config.get("arch") == "compact"
        if denoise_strength is not None:
            if model_name != DNI_MODEL:
                raise ValueError(f"denoise_strength belongs to {DNI_MODEL} (interpolated with {DNI_WDN_MODEL}), not to {model_name}")
            if not (0.0 <= float(denoise_strength) <= 1.0):
                raise ValueError(f"denoise_strength {denoise_strength} outside [0, 1]")
            if state_dict is not None:
                raise ValueError("denoise_strength interpolates the two checkpoint files; it cannot be combined with state_dict=")
        self.denoise_strength = None if denoise_strength is None else float(denoise_strength)

        # The reference builds the net and reads the 64 MB checkpoint in every job
        # (wow_sr.py:93-97, :164-215).  Here a checkpoint file that has not changed on disk
        # (path, mtime, size) hands back the already loaded parameter shell and its engine.
        cache_key = None
        if state_dict is None:
            weights_path = Path(download_weights(model_name))
            st = weights_path.stat()
            cache_key = (str(weights_path.resolve()), st.st_mtime_ns, st.st_size, config.get("blocks", config.get("num_conv")), config["scale"])
            if self.denoise_strength is not None:
                wdn_path = Path(download_weights(DNI_WDN_MODEL))
                st2 = wdn_path.stat()
                cache_key += (str(wdn_path.resolve()), st2.st_mtime_ns, st2.st_size, self.denoise_strength)
            with _MODELS_LOCK:
                self.model = _LOADED_MODELS.get(cache_key)
        else:
            self.model = None
        if self.model is None:
            # RealESRGAN_x2plus: the reference class's RRDBNet(num_in_ch=12, scale=4) on the unshuffled image
            if compact:
                self.model = SRVGGNetCompact(num_in_ch=3, num_out_ch=3, num_feat=config["channels"], num_conv=config["num_conv"],
                                             upscale=config["scale"], act_type="prelu")
            else:
                self.model = RRDBNet(num_in_ch=first_conv_cin(self.scale), num_out_ch=3, num_feat=config["channels"],
                                     num_block=config["blocks"], num_grow_ch=32, scale=4)
            if state_dict is None:
                state_dict = select_params(torch.load(weights_path, map_location="cpu"))
                if self.denoise_strength is not None:
                    state_dict = dni(state_dict, select_params(torch.load(wdn_path, map_location="cpu")), self.denoise_strength)
            state_dict = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in state_dict.items()}
            self.model.load_state_dict(state_dict, strict=True)
            self.model.eval()
            if cache_key is not None:
                with _MODELS_LOCK:
                    if len(_LOADED_MODELS) >= 8:
                        _LOADED_MODELS.clear()
                    _LOADED_MODELS[cache_key] = self.model
        self._engine = self.model.engine(self.device.index or 0)
        print(f"   Loaded {model_name} (x{self.scale})")

    @staticmethod
    def _mask_of(img: np.ndarray, valid, nodata, fill_radius):
        """The mask of a nodata call -> (valid uint8 [H, W] or None, the value invalid output pixels get).  valid: the mask itself
        (nonzero = valid); nodata: the value -- without `valid`, a pixel is invalid iff all three bands equal it.  Neither: None."""
        from s2sr.nodata import check_args, mask_from_value
        if valid is None and nodata is None:
            return None, 0
        check_args(nodata, fill_radius)
        if nodata == "tag":
            raise ValueError("nodata=\"tag\" belongs to the file-level jobs (app.wow_sr): an array has no tags")
        if valid is None:
            valid = mask_from_value(img, nodata)
        valid = np.asarray(valid)
        if valid.shape != img.shape[:2]:
            raise ValueError(f"valid: expected shape {img.shape[:2]}, got {valid.shape}")
        return valid, 0 if nodata is None else int(nodata)

    def enhance(self, img: np.ndarray, valid=None, nodata=None, fill_radius: int = 32) -> np.ndarray:
        """HxWx3 uint8 (channel order as given) -> 4Hx4Wx3 uint8 (self.scale x: 2Hx2Wx3 for realesrgan_x2plus, whose odd
        sizes are reflect-padded by one row / column and cropped back, RealESRGANer's mod-2 rule).

        valid / nodata (not in the reference): pixels that were never measured -- `valid` uint8 [H, W], or all
        three bands equal to `nodata` -- are filled from their nearest valid neighbour within fill_radius in front of the net
        and come out as `nodata` (0 without one) again; see native.Engine.enhance_masked_u8.

        Whole-image forward when h*w <= tile_size^2*4, otherwise the reference's window plan
        (tile_size + 2*tile_pad windows, halo crop, later windows overwrite) -- both inside
        s2sr_enhance_u8; quantisation is the reference's truncation (:232)."""
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"expected HxWx3 image, got shape {img.shape}")
        if img.dtype != np.uint8:
            # the reference divides whatever it gets by 255 (:220); only u8 is on the native path
            raise TypeError(f"expected uint8 image, got {img.dtype}")
        valid, out_nodata = self._mask_of(img, valid, nodata, fill_radius)
        with self._engine.chain_lock:        # (not between another job's enhance16 and its display rendering)
            return self._door(img, valid, fill_radius, out_nodata)

    def _door(self, img: np.ndarray, valid, fill_radius, out_nodata, **fields) -> np.ndarray:
        """One whole-image call with this object's options (seam blend, consistency mode) and the call's (its mask; fields: what
        else the record takes) -> the quantised image.  The caller holds the chain lock."""
        r = self._engine.enhance(img, tile=self.tile_size, pad=self.tile_pad, blend=self.seam_blend, consistency=self._cmode or 0,
                                 valid=valid, radius=fill_radius, out_nodata=out_nodata, **fields)
        if self._cmode:
            self.last_inexact_blocks = [int(v) for v in r.inexact]
        return r.q

    def product16(self, img: np.ndarray, value_range=None, display=None, valid=None, nodata=None, fill_radius: int = 32, extra=None,
                  extra_range=None, extra_weights=None, indices=None) -> "Product16":
        """HxWx3 uint16 (channel order as given) -> Product16, whose out16 is 4Hx4Wx3 uint16 in the source's units: the 16-bit door
        of the native library (upstream RealESRGANer's max_range = 65535 branch; the reference has none).  value_range (lo, hi),
        None = (0, 65535): the net sees (clip(v, lo, hi) - lo) / (hi - lo), the output is lo + rint(clip(y, 0, 1) * (hi - lo)).
        Same whole / tiled switch and window plan as `enhance`.  The x4 RRDB models only (realesrgan_x4, realesrgan_anime).
        display (a s2sr.display.Stretch or a dict of its fields): .display and .info, the 8-bit display rendering of the output
        (percentile stretch, s2sr/display.py) made from the output's device copy, without a second upload; per-band limits are in
        the channel order of `img`.
        valid / nodata / fill_radius: as `enhance`; a display stretch that names no nodata of its own leaves the job's out of its
        statistics.
        extra (HxWxk uint16): bands the net never saw, carried to the output grid against the output's device copy
        (native.Engine.carry_band_u16: guided upsampling, then block means that reproduce the band), behind the door and in front of
        the display rendering, under the call's mask: .carried (4Hx4Wxk) and .carried_record (the ranges, eps and inexact blocks per
        band; also kept as last_extra).  extra_range: one (lo, hi) or one per band; None: each band's own min and max over the
        valid pixels.  extra_weights: the three guide weights in the channel order of `img` (None: 1, 1, 1).
        indices: normalised-difference indices on the output grid, a list of {"a", "b", "offset", "L", "K", "lut",
        "zones", "zone_scale", "Z"} with a and b either ("img", channel of `img`) -- read from the output's device copy -- or
        ("extra", i) -- the i-th carried band; lut (uint8 [65536][4]) and zones (uint16 labels, with zone_scale and Z) may be None.
        Under the call's mask.  .indices: per index {"index" int16 [4H, 4W], "hist", "undefined"} and, with a lut / zones, "rgba" /
        "zonal" (native.Engine.index_nd_u16).
        .inexact_blocks: with consistency, the blocks per band a clip kept off (also kept as last_inexact_blocks)."""
        if self.scale != 4 or getattr(self.model, "arch", "rrdb") != "rrdb":
            raise ValueError(f"enhance16 is built for the x4 RRDB models, not {self.model_name}")
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"expected HxWx3 image, got shape {img.shape}")
        if img.dtype != np.uint16:
            raise TypeError(f"expected uint16 image, got {img.dtype}")
        lo, hi = (0, 65535) if value_range is None else (int(value_range[0]), int(value_range[1]))
        if not (0 <= lo < hi <= 65535):
            raise ValueError(f"value_range {value_range}: need 0 <= lo < hi <= 65535")
        valid, out_nodata = self._mask_of(img, valid, nodata, fill_radius)
        plan = None if extra is None else self._extra_plan(img, extra, extra_range, extra_weights, valid, out_nodata)
        iplan = None if indices is None else self._index_plan(indices, 0 if extra is None else np.asarray(extra).shape[2])
        stretch = None
        if display is not None:
            from s2sr.display import Stretch, render_u16
            stretch = Stretch.of(display)
            if nodata is not None and stretch.nodata is None:
                import dataclasses
                stretch = dataclasses.replace(stretch, nodata=out_nodata)
        disp = info = carried = record = found = None
        with self._engine.chain_lock:        # the engine is shared by every job of the process: nothing between the door and its readers
            out16 = self._door(img, valid, fill_radius, out_nodata, lo=lo, hi=hi)
            if plan is not None:             # (it leaves the device copy as the door left it)
                carried = self._carry_extra(plan)
                record = self.last_extra
            if stretch is not None:
                disp, info = render_u16(None, stretch, self._engine, shape=out16.shape[:2])
            if iplan is not None:            # (behind the rendering: see _run_indices)
                found = self._run_indices(iplan, out16, carried, valid)
            inexact = self.last_inexact_blocks if self._cmode else None
        return Product16(out16, disp, info, carried, record, found, inexact)

    def enhance16(self, img: np.ndarray, value_range=None, display=None, valid=None, nodata=None, fill_radius: int = 32, extra=None,
                  extra_range=None, extra_weights=None, indices=None):
        """`product16` (same arguments, see there) flattened into a bare array or a tuple of the parts that were asked for:

        | display | extra | indices | returns                                   |
        |---------|-------|---------|-------------------------------------------|
        | -       | -     | -       | out16 (a bare array)                      |
        | -       | yes   | -       | (out16, carried)                          |
        | -       | -     | yes     | (out16, indices)                          |
        | -       | yes   | yes     | (out16, carried, indices)                 |
        | yes     | -     | -       | (out16, display, info)                    |
        | yes     | yes   | -       | (out16, display, info, carried)           |
        | yes     | -     | yes     | (out16, display, info, indices)           |
        | yes     | yes   | yes     | (out16, display, info, carried, indices)  |

        carried_record and inexact_blocks are not in the tuple: read last_extra and last_inexact_blocks, or call product16."""
        p = self.product16(img, value_range, display, valid, nodata, fill_radius, extra, extra_range, extra_weights, indices)
        res = (p.out16,) + (() if display is None else (p.display, p.info)) + (() if extra is None else (p.carried,)) + \
              (() if indices is None else (p.indices,))
        return res[0] if len(res) == 1 else res

    @staticmethod
    def _index_plan(indices, k: int) -> list:
        """The index records of a call, checked before the door runs."""
        from s2sr import index as X
        plan = []
        for d in indices:
            for side in ("a", "b"):
                kind, c = d[side]
                if kind not in ("img", "extra") or not 0 <= int(c) < (3 if kind == "img" else k):
                    raise ValueError(f"indices: {side} = {d[side]!r} names neither a channel of the image nor one of the {k} carried band(s)")
            if d["a"] == d["b"]:
                raise ValueError(f"indices: a and b are both {d['a']!r}")
            X._int(d.get("offset", 0), 0, 65535, "offset"), X._int(d.get("L", 0), 0, 65535, "L"), X._int(d.get("K", 10000), 1, X.K_MAX, "K")
            plan.append(dict(d))
        return plan

    def _run_indices(self, plan, out16, carried, valid):
        """Inside the chain lock, behind the door, the carried bands and the display rendering.  An image channel is read from the
        output's device copy, which the engine takes as plane a only: an index whose b is an image channel runs with the planes
        exchanged -- that negates every defined value exactly -- through the mirrored LUT, and its raster,
        histogram and zonal sums are mirrored back here.  Indices of two carried bands upload both planes over the device copy,
        so they run last."""
        found = [None] * len(plan)
        order = sorted(range(len(plan)), key=lambda i: plan[i]["a"][0] == "extra" and plan[i]["b"][0] == "extra")
        for i in order:
            d = plan[i]
            (ka, ca), (kb, cb) = d["a"], d["b"]
            flip = kb == "img" and ka == "extra"
            if flip:
                (ka, ca), (kb, cb) = (kb, cb), (ka, ca)
            lut = d.get("lut")
            if flip and lut is not None:
                lut = np.concatenate([lut[:1], lut[:0:-1]])            # entry (-v) + 32768 = 65536 - (v + 32768)
            zones = d.get("zones")
            want = ("index", "hist") + (("rgba",) if lut is not None else ()) + (("zonal",) if zones is not None else ())
            a = None if ka == "img" else np.ascontiguousarray(carried[..., ca])
            b = np.ascontiguousarray(out16[..., cb]) if kb == "img" else np.ascontiguousarray(carried[..., cb])
            r = self._engine.index_nd_u16(a, b, ca=ca if ka == "img" else 0, cb=0, offset=d.get("offset", 0), L=d.get("L", 0), K=d.get("K", 10000),
                                          valid=valid, valid_scale=4, zones=zones, zone_scale=d.get("zone_scale", 1), Z=d.get("Z", 0), lut=lut,
                                          want=want)
            r = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in r.items()}       # (out of the pinned pool, which the next call reuses)
            if flip:
                r["index"] = np.negative(r["index"])                    # int16: -(-32768) is -32768, nodata stays
                r["hist"] = np.ascontiguousarray(r["hist"][::-1])
                if "zonal" in r:
                    r["zonal"][:, 1] *= -1
            found[i] = r
        return found

    @staticmethod
    def _extra_plan(img, extra, extra_range, extra_weights, valid, fill):
        """The arguments of every band of `extra`, checked before the door runs: [(band [H, W], s2sr.bands.check_args's dict)], valid."""
        from s2sr import bands as B
        extra = np.asarray(extra)
        if extra.ndim != 3 or extra.shape[:2] != img.shape[:2] or extra.shape[2] < 1:
            raise ValueError(f"extra: expected {img.shape[:2]} x k bands, got shape {extra.shape}")
        if extra.dtype != np.uint16:
            raise TypeError(f"extra: expected uint16 bands, got {extra.dtype}")
        k = extra.shape[2]
        if extra_range is None:
            ranges = [B.band_range(extra[..., i], valid) for i in range(k)]
        else:
            r = np.asarray(extra_range)
            if r.shape not in ((2,), (k, 2)):
                raise ValueError(f"extra_range: one (lo, hi) or one per band ({k}), got {extra_range!r}")
            ranges = [(int(a), int(b)) for a, b in (np.broadcast_to(r, (k, 2)))]
        w = B.WEIGHTS if extra_weights is None else extra_weights
        return [(np.ascontiguousarray(extra[..., i]), B.check_args(4, lo, hi, w, fill=int(fill))) for i, (lo, hi) in enumerate(ranges)], valid

    def _carry_extra(self, plan):
        """Inside the chain lock, behind the door: every band against the device copy -> uint16 [4H, 4W, k]."""
        bands, valid = plan
        out, rec = [], {"ranges": [], "eps": [], "inexact": []}
        for band, a in bands:
            g, bad = self._engine.carry_band_u16(band, 4, lo=a["lo"], hi=a["hi"], weights=a["weights"], r=a["r"], eps=a["eps"], valid=valid,
                                                 fill=a["fill"])
            out.append(g)
            rec["ranges"].append((a["lo"], a["hi"])); rec["eps"].append(a["eps"]); rec["inexact"].append(bad)
        rec.update(weights=bands[0][1]["weights"], r=bands[0][1]["r"])
        self.last_extra = rec
        return np.stack(out, axis=-1)

    def enhance_job(self, rgb: np.ndarray, post=None, valid=None, nodata=None, fill_radius: int = 32) -> np.ndarray:
        """What a job does around `enhance` (wow_sr.py:85-110, farm_sr.py:156-178) in one native call: RGB in, RGB2BGR, the net,
        BGR2RGB, the crop-visibility post-process `post` (native.pp_wow() / pp_farm(); None: none), RGB out.  The same bytes as
        `enhance(rgb[:, :, ::-1])[:, :, ::-1]` followed by the post-process -- one upload and one download instead of three
        round trips and two host-side channel flips of the 16x image (tests/test_gpu_app.py).
        valid / nodata / fill_radius: as `enhance`; the post-process runs on the filled image, the mask goes on last."""
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"expected HxWx3 image, got shape {rgb.shape}")
        if rgb.dtype != np.uint8:
            raise TypeError(f"expected uint8 image, got {rgb.dtype}")
        valid, out_nodata = self._mask_of(rgb, valid, nodata, fill_radius)
        with self._engine.chain_lock:            # (a consistency pass sits in front of the post-process: the product is consistent before it)
            return self._door(rgb, valid, fill_radius, out_nodata, prm=post, swap_rb=True)

    def _tile_process(self, img: torch.Tensor) -> torch.Tensor:
        """[1,3,H,W] float in [0,1] -> [1,3,sH,sW] float32 (s = self.scale) through the tiled path (:236-280)."""
        u8 = (img[0].permute(1, 2, 0).cpu().numpy() * 255.0).round().clip(0, 255).astype(np.uint8)
        out = self._engine.tile_process_f32(u8, tile=self.tile_size, pad=self.tile_pad)
        return torch.from_numpy(out).permute(2, 0, 1).unsqueeze(0)


def apply_cnn_sr(input_path: Path, output_path: Path, scale: int = 4) -> Tuple[Path, dict]:
    """File-level glue of the reference (:283-382): read raster -> enhance -> write raster."""
    from s2sr import rasterio_lite as rio

    print(f"\nCNN Super-Resolution (Real-ESRGAN x{scale})")
    input_path = Path(input_path)
    img, georef = rio.read_rgb_u8(input_path, minmax_eps=1e-6)
    model = RealESRGAN(scale=scale, tile_size=256)
    out_bgr = model.enhance(np.ascontiguousarray(img[:, :, ::-1]))
    out_rgb = np.ascontiguousarray(out_bgr[:, :, ::-1])
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    if georef is not None:
        final_path = output_path.with_suffix(".tif")
        rio.write_geotiff_rgb(final_path, out_rgb, georef.scaled(scale))
    else:
        final_path = output_path.with_suffix(".png")
        rio.write_png(final_path, out_rgb)
    metadata = {
        "model": f"RealESRGAN_x{scale}",
        "scale": scale,
        "input_size": [img.shape[1], img.shape[0]],
        "output_size": [out_rgb.shape[1], out_rgb.shape[0]],
        "device": str(model.device),
        "original_resolution_m": 10.0,
        "effective_resolution_m": 10.0 / scale,
    }
    return final_path, metadata
