"""Frame-quality metrics of the paper's evaluation protocol; pretrained networks (VGG19, LPIPS, Inception) take their weights from the caller.
Inputs are (bs, observations_count, channels, height, width) tensors in the same value range; results are (bs, observations_count).

    mse / psnr                  evaluation/metrics/mse.py:13-24, psnr.py:11-31 -- plain torch expressions
    ssim                        evaluation/metrics/ssim.py:13-35 (piq.ssim)                            \
    motion_masked_mse           evaluation/metrics/motion_masked_mse.py:16-28 + motion_mask.py:14-37    > the fused HIP pass of csrc/frame_metrics.hip
    vgg_cosine_similarity       evaluation/metrics/vgg_cosine_similarity.py:22-57 (VGG19 relu1_1..5_1)  /  (+ the VGG19 kernels of csrc/perceptual.hip)
    breakout_platform_positions evaluation/metrics/breakout_platform_position.py                       -- the row scan of csrc/detection.hip
    lpips                       evaluation/metrics/lpips.py:14,33 (lpips.LPIPS(net='vgg'))              -- VGG16 to relu5_3 on the VGG kernels of csrc/perceptual.hip
                                                                                                          + the normalise / weight / average head of csrc/lpips.hip

The HIP-backed metrics run on a metrics context of libcaddy_hip.so (caddy_metrics_ctx_create), cached per frame geometry; there is no torch fallback.
`set_library` points them at another build of the same kernels (the tests' host simulator).
    fid                         evaluation/metrics/fid.py:140-159 (pytorch_fid InceptionV3([3]) features)  -- the Inception-v3 trunk on the implicit-GEMM convolution,
                                                                                                          pooling and resize kernels of csrc/fid.hip; mean, covariance and
                                                                                                          the Frechet distance in fp64 on the host
LPIPS needs its weights from the caller (a torchvision vgg16 state dict plus the package's five `lin` tensors, see lpips_state), FID the pt_inception-2015-12-05 state dict
(fid_inception_state): nothing is downloaded.
    fvd                         evaluation/metrics/fvd.py:67-126,188-226 (Kinetics-400 I3D logits per video)  -- the I3D trunk on the 3-D implicit-GEMM convolution, SAME max
                                                                                                          pools and legacy bilinear input stage of csrc/fvd.hip; the same host
                                                                                                          fp64 statistics and Frechet distance as FID
FVD needs the variables of the I3D module from the caller (fvd_i3d_state; INTEGRATION.md has the export recipe): nothing is downloaded.
    inception_score             evaluation/metrics/inception_score.py:17-65 (torchvision inception_v3 softmax)  -- the same Inception-v3 graph in its torchvision flavour (no input
                                                                                                          normalisation, padding-including average pools), fc as a 1 x 1
                                                                                                          implicit-GEMM convolution and the wave-per-frame softmax of csrc/fid.hip;
                                                                                                          the split KL score in fp64 on the host
The Inception Score needs a torchvision inception_v3 state dict from the caller (is_inception_state): nothing is downloaded.
(The Tennis detector and the plots stay out of scope.)"""
import ctypes as C
import re
from typing import Dict, Optional

import numpy as np
import torch


def mse(reference_observations: torch.Tensor, generated_observations: torch.Tensor) -> torch.Tensor:
    return torch.mean((reference_observations - generated_observations).pow(2), dim=[2, 3, 4])


def psnr(reference_observations: torch.Tensor, generated_observations: torch.Tensor, value_range: float = 1.0) -> torch.Tensor:
    """-10 log10(MSE of the range-normalised frames + 1e-8): the reference's stabilising constant caps the score at 80 dB"""
    err = torch.mean(((reference_observations - generated_observations) / value_range) ** 2, dim=[2, 3, 4])
    return -10.0 * torch.log10(err + 1e-8)


# ---- HIP-backed metrics (caddy_frame_metrics) ----
SLOTS = ("mse", "motion_masked_mse", "psnr", "ssim", "vgg_sim", "ref_min", "ref_max", "gen_min", "gen_max")      # CADDY_FM_* of include/caddy_hip.h
VGG_FRAMES_256 = 30      # frames per VGG19 chunk at 256 x 256 (scaled by the frame area): ~4 GB of feature maps
_default_lib = None
_contexts: Dict = {}      # every cached context: (kind, library, device, geometry, weights) -> FrameMetrics | LPIPS | InceptionFeatures | I3DEmbeddings | InceptionProbabilities


def set_library(lib) -> None:
    """library the HIP-backed metrics use when none is passed (None: libcaddy_hip.so); drops the cached contexts"""
    global _default_lib
    _default_lib = lib
    _contexts.clear()


def _bind(lib):
    from .engine import _bind as bind_engine
    lib = bind_engine(lib)
    if not getattr(lib, "_caddy_metrics_bound", False):
        lib.caddy_metrics_workspace_bytes.restype = C.c_size_t
        lib.caddy_metrics_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        lib.caddy_metrics_ctx_create.restype = C.c_void_p
        lib.caddy_metrics_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        lib.caddy_frame_metrics.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
        lib.caddy_platform_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p]
        lib.caddy_lpips_workspace_bytes.restype = C.c_size_t
        lib.caddy_lpips_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.caddy_lpips_ctx_create.restype = C.c_void_p
        lib.caddy_lpips_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        lib.caddy_lpips_param_floats.restype = C.c_long
        lib.caddy_lpips_param_info_get.argtypes = [C.c_int, C.c_void_p]
        lib.caddy_load_lpips.argtypes = [C.c_void_p, C.c_void_p]
        lib.caddy_frame_lpips.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
        lib.caddy_debug_lpips_tap_formats.argtypes = [C.c_void_p]
        lib.caddy_fid_workspace_bytes.restype = C.c_size_t
        lib.caddy_fid_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        lib.caddy_fid_ctx_create.restype = C.c_void_p
        lib.caddy_fid_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        lib.caddy_fid_param_floats.restype = C.c_long
        lib.caddy_fid_param_info_get.argtypes = [C.c_int, C.c_void_p]
        lib.caddy_load_fid_inception.argtypes = [C.c_void_p, C.c_void_p]
        lib.caddy_set_fid_precision.argtypes = [C.c_void_p, C.c_int]
        lib.caddy_fid_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.caddy_debug_fid_block.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.caddy_debug_fid_fallback_layers.argtypes = [C.c_void_p]
        lib.caddy_debug_fid_stage_ms.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.caddy_fid_macs_per_frame.restype = C.c_double
        lib.caddy_fid_macs_per_frame.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.caddy_is_workspace_bytes.restype = C.c_size_t
        lib.caddy_is_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        lib.caddy_is_ctx_create.restype = C.c_void_p
        lib.caddy_is_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        lib.caddy_is_param_floats.restype = C.c_long
        lib.caddy_is_param_info_get.argtypes = [C.c_int, C.c_void_p]
        lib.caddy_load_is_inception.argtypes = [C.c_void_p, C.c_void_p]
        lib.caddy_set_is_precision.argtypes = [C.c_void_p, C.c_int]
        lib.caddy_is_probabilities.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.caddy_debug_is_logits.argtypes = [C.c_void_p, C.c_void_p]
        lib.caddy_debug_is_fallback_layers.argtypes = [C.c_void_p]
        lib.caddy_debug_is_stage_ms.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.caddy_is_macs_per_frame.restype = C.c_double
        lib.caddy_is_macs_per_frame.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.caddy_fvd_workspace_bytes.restype = C.c_size_t
        lib.caddy_fvd_workspace_bytes.argtypes = [C.c_int] * 5
        lib.caddy_fvd_ctx_create.restype = C.c_void_p
        lib.caddy_fvd_ctx_create.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_size_t]
        lib.caddy_fvd_param_floats.restype = C.c_long
        lib.caddy_fvd_param_info_get.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        lib.caddy_load_fvd_i3d.argtypes = [C.c_void_p, C.c_void_p]
        lib.caddy_set_fvd_precision.argtypes = [C.c_void_p, C.c_int]
        lib.caddy_fvd_embeddings.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.caddy_debug_fvd_block.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.caddy_debug_fvd_fallback_layers.argtypes = [C.c_void_p]
        lib.caddy_debug_fvd_stage_ms.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.caddy_fvd_macs_per_video.restype = C.c_double
        lib.caddy_fvd_macs_per_video.argtypes = [C.c_int] * 4
        lib._caddy_metrics_bound = True
    return lib


def _param_table(count, info_get):
    """[(name, offset, shape)] of a caddy_*_param_count / caddy_*_param_info_get pair"""
    from .engine import ParamInfo
    info, table = ParamInfo(), []
    for i in range(count()):
        info_get(i, C.byref(info))
        table.append((info.name.decode(), int(info.offset), tuple(info.shape[:info.ndim])))
    return table


def _cached(key, weights, make, stale=lambda ctx: False):
    """the context cached under `key`, made (again, if `stale`) by `make`; `weights` is kept alive because the key holds its id"""
    ctx = _contexts.get(key)
    if ctx is None or stale(ctx):
        _contexts.pop(key, None)
        ctx = make()
        ctx._keep = weights
        _contexts[key] = ctx
    return ctx


class _EvalContext:
    """What the evaluation contexts share: library and device, a context created in a workspace of its own, error handling and the upload of a flat parameter buffer."""

    def __init__(self, height: int, width: int, max_frames: int, lib, device):
        from . import _lib
        self.lib = _bind(lib if lib is not None else (_default_lib if _default_lib is not None else _lib.load()))
        kind = getattr(self.lib, "_caddy_device_type", "cuda")
        self.device = torch.device(device) if device is not None else torch.device(kind)
        self.H, self.W, self.max_frames = int(height), int(width), int(max_frames)
        self._err = lambda: self.lib.caddy_last_error().decode()

    def _create(self, workspace_bytes, ctx_create, *extra):
        """workspace_bytes / ctx_create: the kind's two C functions, both taking (max_frames, height, width, *extra)"""
        from .engine import CaddyError
        n = workspace_bytes(self.max_frames, self.H, self.W, *extra)
        if n == 0:
            raise CaddyError(self._err())
        raw = torch.empty(n + 256, dtype=torch.uint8, device=self.device)
        self._ws = raw
        self.ws_bytes = n
        self.ctx = ctx_create(self.max_frames, self.H, self.W, *extra, raw.data_ptr() + (-raw.data_ptr()) % 256, n)
        if not self.ctx:
            raise CaddyError(self._err())

    def _load(self, load, floats, table, state, what, staging=None):
        """fills a flat fp32 buffer of `floats` floats with the tensors of `state` along the (name, offset, shape) `table` -- on `staging`, by default the context's
        device -- and hands it to the C function `load`"""
        from .engine import CaddyError
        flat = torch.zeros(floats, dtype=torch.float32, device=self.device if staging is None else staging)
        for name, off, shape in table:
            t = state[name].detach().to(flat.device, torch.float32)
            if tuple(t.shape) != shape:
                raise CaddyError(f"{what} {name}: shape {tuple(t.shape)}, expected {shape}")
            flat[off:off + t.numel()] = t.reshape(-1)
        flat = flat.to(self.device)
        self._stream()
        self._check(load(self.ctx, flat.data_ptr()))
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()

    def _check(self, rc):
        if rc != 0:
            from .engine import CaddyError
            raise CaddyError(self._err() or f"caddy error {rc}")

    def _stream(self):
        self.lib.caddy_set_stream(self.ctx, torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else 0)

    def __del__(self):
        if getattr(self, "ctx", None):
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()
            self.lib.caddy_ctx_destroy(self.ctx)
            self.ctx = None


class _VggContext(_EvalContext):
    """the two kinds that run a VGG trunk"""

    def set_vgg_precision(self, forward: int):
        """arithmetic of the VGG convolutions: 0 (exact fp32) | 16 (split f16, default) | 18 (plain f16)"""
        self._check(self.lib.caddy_set_vgg_precision(self.ctx, int(forward), 17))


class FrameMetrics(_VggContext):
    """A metrics context for frames of height x width: the fused per-frame pass and, with `vgg_state_dict` (torchvision vgg19 naming, as
    Engine.load_vgg takes it), the VGG19 cosine similarity.  Calls with more than `max_frames` frames run in chunks of `max_frames`."""

    def __init__(self, height: int, width: int, max_frames: int, vgg_state_dict=None, lib=None, device=None):
        super().__init__(height, width, max_frames, lib, device)
        self.vgg = vgg_state_dict is not None
        self._create(self.lib.caddy_metrics_workspace_bytes, self.lib.caddy_metrics_ctx_create, int(self.vgg))
        if self.vgg:
            from .engine import CaddyError
            table, state = _param_table(self.lib.caddy_vgg_param_count, self.lib.caddy_vgg_param_info_get), {}
            for name, _, _ in table:      # torchvision's vgg19() names, or those of its .features
                key = name if name in vgg_state_dict else name[len("features."):]
                if key not in vgg_state_dict:
                    raise CaddyError(f"VGG19 state dict lacks {name}")
                state[name] = vgg_state_dict[key]
            self._load(self.lib.caddy_load_vgg, self.lib.caddy_vgg_param_floats(), table, state, "VGG19")

    def __call__(self, reference_observations: torch.Tensor, generated_observations: torch.Tensor, value_range: float = 1.0,
                 want_vgg: bool = False) -> Dict[str, torch.Tensor]:
        """-> {slot: (bs, observations_count) float64 CPU tensor} for the slots of SLOTS (vgg_sim: NaN unless want_vgg)"""
        r, g = reference_observations, generated_observations
        if r.dim() != 5 or r.shape != g.shape or r.shape[2] != 3 or tuple(r.shape[3:]) != (self.H, self.W):
            raise ValueError(f"expected two (bs, observations_count, 3, {self.H}, {self.W}) tensors, got {tuple(r.shape)} and {tuple(g.shape)}")
        if want_vgg and not self.vgg:
            raise ValueError("this metrics context was created without VGG19 weights")
        B, T = int(r.shape[0]), int(r.shape[1])
        r = r.detach().to(self.device, torch.float32).contiguous()
        g = g.detach().to(self.device, torch.float32).contiguous()
        out = torch.empty(len(SLOTS), B, T, dtype=torch.float64)
        self._stream()
        self._check(self.lib.caddy_frame_metrics(self.ctx, r.data_ptr(), g.data_ptr(), B, T, float(value_range), int(want_vgg), out.data_ptr()))
        return {k: out[i] for i, k in enumerate(SLOTS)}

    def platform_positions(self, observations: torch.Tensor, row: int, lo: float, hi: float, min_run: int) -> np.ndarray:
        """-> (bs, observations_count) int64: the start of the first run of >= min_run columns of row `row` whose channel-0 value lies in [lo, hi]
        (the last column never counts), -1 where there is none (caddy_platform_positions)"""
        o = observations
        if o.dim() != 5 or o.shape[2] != 3 or tuple(o.shape[3:]) != (self.H, self.W):
            raise ValueError(f"expected a (bs, observations_count, 3, {self.H}, {self.W}) tensor, got {tuple(o.shape)}")
        B, T = int(o.shape[0]), int(o.shape[1])
        o = o.detach().to(self.device, torch.float32).contiguous()
        out = np.empty((B, T), dtype=np.int32)
        self._stream()
        self._check(self.lib.caddy_platform_positions(self.ctx, o.data_ptr(), B, T, int(row), float(lo), float(hi), int(min_run),
                                                      out.ctypes.data_as(C.c_void_p)))
        return out.astype(np.int64)


def check_range(values: Dict[str, torch.Tensor], which: str = "ref") -> None:
    """DatasetEvaluator.check_range (evaluation/dataset_evaluator.py:73-83) from the per-frame minima / maxima of the fused pass"""
    mx, mn = float(values[which + "_max"].max()), float(values[which + "_min"].min())
    if mx > 1.0 or mn < 0.0:
        raise Exception(f"Input tensor outside allowed range [0.0, 1.0]: [{mn}, {mx}]")


def _cached_context(observations: torch.Tensor, vgg_state_dict, lib) -> FrameMetrics:
    """the metrics context of this library, device, frame geometry and VGG19 weights, (re)created when it holds too few frames"""
    B, T, _, H, W = observations.shape
    n = int(B) * int(T)
    lib = lib if lib is not None else _default_lib
    vkey = None if vgg_state_dict is None else id(vgg_state_dict)
    key = ("metrics", id(lib), str(observations.device), int(H), int(W), vkey)
    want = n if vgg_state_dict is None else min(n, max(1, VGG_FRAMES_256 * 256 * 256 // (int(H) * int(W))))
    return _cached(key, vgg_state_dict, lambda: FrameMetrics(H, W, min(want, 1024), vgg_state_dict, lib),
                   lambda fm: vgg_state_dict is None and fm.max_frames < min(n, 1024))


def frame_metrics(reference_observations: torch.Tensor, generated_observations: torch.Tensor, value_range: float = 1.0, vgg_state_dict=None,
                  lib=None) -> Dict[str, torch.Tensor]:
    """every slot of SLOTS in one pass (vgg_sim only with `vgg_state_dict`); the metrics context is cached per frame geometry"""
    fm = _cached_context(reference_observations, vgg_state_dict, lib)
    return fm(reference_observations, generated_observations, value_range, want_vgg=vgg_state_dict is not None)


def breakout_platform_parameters(height: int):
    """(row, lo, hi, min_run) of BreakoutPlatformPosition (evaluation/metrics/breakout_platform_position.py): the platform row int(188 / 208 * height),
    the fp32 channel-0 bounds of its colour mask (torch's float32 arithmetic, as the reference computes them) and the run length of detect_platform"""
    lo = float(torch.tensor([100], dtype=torch.float) / 255 - 0.15)
    hi = float(torch.tensor([200], dtype=torch.float) / 255 + 0.15)
    return int(188 / 208 * int(height)), lo, hi, 12


def breakout_platform_positions(observations: torch.Tensor, lib=None) -> np.ndarray:
    """(bs, observations_count, 3, H, W) frames in [0, 1] -> (bs, observations_count) int64 left edge of the Breakout platform, -1 where it is not
    found (BreakoutPlatformPosition.forward); runs on the metrics context frame_metrics caches for this geometry"""
    if observations.dim() != 5:
        raise ValueError(f"expected a (bs, observations_count, 3, H, W) tensor, got {tuple(observations.shape)}")
    row, lo, hi, min_run = breakout_platform_parameters(observations.shape[3])
    return _cached_context(observations, None, lib).platform_positions(observations, row, lo, hi, min_run)


def device(lib=None) -> torch.device:
    """the torch device the pointers of `lib` (default: the library of the HIP-backed metrics) live on"""
    from . import _lib
    lib = lib if lib is not None else (_default_lib if _default_lib is not None else _lib.load())
    return torch.device(getattr(lib, "_caddy_device_type", "cuda"))


def ssim(reference_observations: torch.Tensor, generated_observations: torch.Tensor, value_range: float = 1.0, lib=None) -> torch.Tensor:
    """piq.ssim(generated / range, reference / range, reduction="none") per observation (evaluation/metrics/ssim.py:13-35)"""
    return frame_metrics(reference_observations, generated_observations, value_range, lib=lib)["ssim"]


def motion_masked_mse(reference_observations: torch.Tensor, generated_observations: torch.Tensor, lib=None) -> torch.Tensor:
    """MSE weighted by the frame-difference motion mask of the reference sequence (evaluation/metrics/motion_masked_mse.py:16-28)"""
    return frame_metrics(reference_observations, generated_observations, lib=lib)["motion_masked_mse"]


def vgg_cosine_similarity(reference_observations: torch.Tensor, generated_observations: torch.Tensor, vgg_state_dict, value_range: float = 1.0,
                          lib=None) -> torch.Tensor:
    """mean over relu1_1 .. relu5_1 of the cosine similarity of the VGG19 features (evaluation/metrics/vgg_cosine_similarity.py:22-57)"""
    if vgg_state_dict is None:
        raise ValueError("vgg_cosine_similarity needs VGG19 weights")
    return frame_metrics(reference_observations, generated_observations, value_range, vgg_state_dict, lib=lib)["vgg_sim"]


# ---- LPIPS (caddy_frame_lpips) ----
LPIPS_FRAMES_256 = 30      # frames per VGG16 chunk at 256 x 256 (scaled by the frame area), as VGG_FRAMES_256
LPIPS_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # torchvision vgg16().features indices of the trunk's convolutions
LPIPS_LEVELS = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)      # the package's scaling layer; compiled into csrc/lpips.hip


def lpips_state(weights: Dict[str, torch.Tensor], linear: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """The tensors of lpips.LPIPS(net='vgg') under the names of caddy_lpips_param_info_get (features.{idx}.weight / .bias, lin{l}.model.1.weight) from
      (a) one dict with torchvision's vgg16 names (vgg16().state_dict() or .features.state_dict(): `features.{idx}.*` or `{idx}.*`) plus `lin{l}.model.1.weight`,
      (b) the package's own state dict (`net.slice{k}.{idx}.*`, `lin{l}.model.1.weight` / `lins.{l}.model.1.weight`, optionally `scaling_layer.shift` / `.scale`,
          which must equal the constants the kernel applies),
      (c) the trunk in `weights` and the `lin` tensors in `linear` (the package ships only the latter and takes the trunk from torchvision).
    A missing tensor raises CaddyError naming it."""
    from .engine import CaddyError
    src = dict(weights)
    if linear is not None:
        src.update(linear)
    for key, want in (("scaling_layer.shift", LPIPS_SHIFT), ("scaling_layer.scale", LPIPS_SCALE)):
        if key in src and not torch.allclose(src[key].detach().float().reshape(-1), torch.tensor(want), rtol=0, atol=1e-6):
            raise CaddyError(f"LPIPS {key} is {src[key].reshape(-1).tolist()}, but the kernel applies {list(want)}")
    sliced = {}
    for k in src:
        m = re.fullmatch(r"net\.slice\d+\.(\d+\.(?:weight|bias))", k)
        if m:
            sliced[m.group(1)] = k
    out = {}
    for idx in LPIPS_CONVS:
        for leaf in ("weight", "bias"):
            name = f"features.{idx}.{leaf}"
            key = next((k for k in (name, f"{idx}.{leaf}", sliced.get(f"{idx}.{leaf}")) if k is not None and k in src), None)
            if key is None:
                raise CaddyError(f"LPIPS weights lack {name}")
            out[name] = src[key]
    for l in range(5):
        name = f"lin{l}.model.1.weight"
        key = next((k for k in (name, f"lins.{l}.model.1.weight") if k in src), None)
        if key is None:
            raise CaddyError(f"LPIPS weights lack {name}")
        out[name] = src[key]
    return out


def find_lpips_weights(cfg) -> Optional[Dict[str, torch.Tensor]]:
    """config["evaluation"] -> lpips_state(...) of `lpips_weights` (one path or dict), or of `lpips_vgg16_weights` + `lpips_linear_weights`; None when neither is configured"""
    def load(src):
        if isinstance(src, str):
            sd = torch.load(src, map_location="cpu", weights_only=True)
            return sd.get("state_dict", sd) if isinstance(sd, dict) else sd
        return src
    one, trunk, lin = cfg.get("lpips_weights", None), cfg.get("lpips_vgg16_weights", None), cfg.get("lpips_linear_weights", None)
    if one is not None:
        return lpips_state(load(one))
    if trunk is not None or lin is not None:
        from .engine import CaddyError
        if trunk is None or lin is None:
            raise CaddyError("evaluation.lpips_vgg16_weights and evaluation.lpips_linear_weights must be given together")
        return lpips_state(load(trunk), load(lin))
    return None


class LPIPS(_VggContext):
    """An LPIPS context for frames of height x width (multiples of 16) with the weights of lpips_state().  Calls with more than `max_frames` frames run in chunks."""

    def __init__(self, height: int, width: int, max_frames: int, lpips_weights, lib=None, device=None):
        super().__init__(height, width, max_frames, lib, device)
        state = lpips_state(lpips_weights)
        self._create(self.lib.caddy_lpips_workspace_bytes, self.lib.caddy_lpips_ctx_create)
        self._load(self.lib.caddy_load_lpips, self.lib.caddy_lpips_param_floats(), _param_table(self.lib.caddy_lpips_param_count, self.lib.caddy_lpips_param_info_get),
                   state, "LPIPS")
        self.levels = None

    def tap_formats(self) -> int:
        """bit l set: the level-l feature maps travelled as S16 tensors in some chunk of the last call (caddy_debug_lpips_tap_formats)"""
        return int(self.lib.caddy_debug_lpips_tap_formats(self.ctx))

    def __call__(self, reference_observations: torch.Tensor, generated_observations: torch.Tensor, value_range: float = 1.0, return_levels: bool = False):
        """-> (bs, observations_count) float64 CPU tensor; with return_levels also the (5, bs, observations_count) terms of LPIPS_LEVELS (kept in self.levels either way)"""
        r, g = reference_observations, generated_observations
        if r.dim() != 5 or r.shape != g.shape or r.shape[2] != 3 or tuple(r.shape[3:]) != (self.H, self.W):
            raise ValueError(f"expected two (bs, observations_count, 3, {self.H}, {self.W}) tensors, got {tuple(r.shape)} and {tuple(g.shape)}")
        B, T = int(r.shape[0]), int(r.shape[1])
        r = r.detach().to(self.device, torch.float32).contiguous()
        g = g.detach().to(self.device, torch.float32).contiguous()
        out = torch.empty(6, B, T, dtype=torch.float64)
        self._stream()
        self._check(self.lib.caddy_frame_lpips(self.ctx, r.data_ptr(), g.data_ptr(), B, T, float(value_range), out.data_ptr()))
        self.levels = out[1:]
        return (out[0], out[1:]) if return_levels else out[0]


def _cached_lpips(observations: torch.Tensor, lpips_weights, lib) -> LPIPS:
    """the LPIPS context of this library, device, frame geometry and weights (cached like _cached_context)"""
    B, T, _, H, W = observations.shape
    lib = lib if lib is not None else _default_lib
    key = ("lpips", id(lib), str(observations.device), int(H), int(W), id(lpips_weights))
    want = min(int(B) * int(T), max(1, LPIPS_FRAMES_256 * 256 * 256 // (int(H) * int(W))))
    return _cached(key, lpips_weights, lambda: LPIPS(H, W, min(want, 1024), lpips_weights, lib))


def lpips(reference_observations: torch.Tensor, generated_observations: torch.Tensor, lpips_weights, value_range: float = 1.0, lib=None,
          return_levels: bool = False):
    """lpips.LPIPS(net='vgg')(reference, generated, normalize=True) per observation (evaluation/metrics/lpips.py:14,33) -> (bs, observations_count) float64"""
    if lpips_weights is None:
        raise ValueError("lpips needs LPIPS weights (see lpips_state)")
    return _cached_lpips(reference_observations, lpips_weights, lib)(reference_observations, generated_observations, value_range, return_levels)


# ---- FID (caddy_fid_features + host fp64 statistics) ----
FID_FRAMES_256 = 64       # frames per Inception chunk at 256 x 256 with the 299 x 299 resize: ~0.9 GB of activations
FID_DIM = 2048
FID_BLOCK_CHANNELS = (64, 192, 768, 2048)      # InceptionV3.BLOCK_INDEX_BY_DIM (pytorch_fid/inception.py:24-29)
_fid_names = None


def fid_param_table(lib=None):
    """[(name, offset, shape)] of caddy_fid_param_info_get: the trunk's tensors under the pt_inception-2015-12-05 names, in graph order"""
    global _fid_names
    from . import _lib
    if _fid_names is None or lib is not None:
        L = _bind(lib if lib is not None else (_default_lib if _default_lib is not None else _lib.load()))
        table = _param_table(L.caddy_fid_param_count, L.caddy_fid_param_info_get)
        if lib is not None:
            return table
        _fid_names = table
    return _fid_names


def fid_inception_state(state_dict: Dict[str, torch.Tensor], lib=None) -> Dict[str, torch.Tensor]:
    """The trunk's tensors of the pt_inception-2015-12-05 state dict (pytorch_fid/inception.py:13,200-201) under the names of caddy_fid_param_info_get.  Accepts the
    keys as they are, under a `module.` / `model.` prefix, or wrapped in {"state_dict": ...}; `fc.*`, `AuxLogits.*` and `num_batches_tracked` are ignored.
    A missing tensor raises CaddyError naming it."""
    from .engine import CaddyError
    src = state_dict.get("state_dict", state_dict) if isinstance(state_dict, dict) else state_dict
    out = {}
    for name, _, _ in fid_param_table(lib):
        key = next((k for k in (name, "module." + name, "model." + name) if k in src), None)
        if key is None:
            raise CaddyError(f"FID Inception weights lack {name}")
        out[name] = src[key]
    return out


def find_fid_weights(cfg) -> Optional[Dict[str, torch.Tensor]]:
    """config["evaluation"] -> fid_inception_state(...) of `fid_inception_weights` (a path or a dict); None when it is not configured.  Nothing is downloaded."""
    src = cfg.get("fid_inception_weights", None)
    if src is None:
        return None
    if isinstance(src, str):
        src = torch.load(src, map_location="cpu", weights_only=True)
    return fid_inception_state(src)


class InceptionFeatures(_EvalContext):
    """The FID feature network for frames of height x width: pytorch_fid's InceptionV3([3], resize_input=resize) on csrc/fid.hip.  Calling it on (bs, T, 3, H, W) or
    (n, 3, H, W) frames in [0, 1] returns an (n, 2048) float64 CPU tensor; more than `max_frames` frames run in chunks."""

    def __init__(self, height: int, width: int, max_frames: int, weights, resize: bool = True, lib=None, device=None):
        super().__init__(height, width, max_frames, lib, device)
        self.resize = bool(resize)
        table = fid_param_table(self.lib)
        state = fid_inception_state(weights, self.lib)
        self._create(self.lib.caddy_fid_workspace_bytes, self.lib.caddy_fid_ctx_create, int(self.resize))
        # (22 M floats in ~470 tensors: assembled on the host and moved once)
        self._load(self.lib.caddy_load_fid_inception, self.lib.caddy_fid_param_floats(), table, state, "FID Inception", staging="cpu")

    def set_precision(self, forward: int):
        """arithmetic of the convolutions: 16 (split f16, default) | 0 (exact fp32)"""
        self._check(self.lib.caddy_set_fid_precision(self.ctx, int(forward)))

    def fallback_layers(self) -> int:
        return int(self.lib.caddy_debug_fid_fallback_layers(self.ctx))

    def __call__(self, observations: torch.Tensor) -> torch.Tensor:
        o = observations
        if o.dim() == 5:
            o = o.reshape((-1,) + tuple(o.shape[2:]))      # TensorFolder.flatten (evaluation/metrics/fid.py:123): every frame of every sequence is a sample
        if o.dim() != 4 or o.shape[1] != 3 or tuple(o.shape[2:]) != (self.H, self.W):
            raise ValueError(f"expected (bs, observations_count, 3, {self.H}, {self.W}) or (n, 3, {self.H}, {self.W}) frames, got {tuple(observations.shape)}")
        n = int(o.shape[0])
        o = o.detach().to(self.device, torch.float32).contiguous()
        out = torch.empty(n, FID_DIM, dtype=torch.float64)
        self._stream()
        self._check(self.lib.caddy_fid_features(self.ctx, o.data_ptr(), n, out.data_ptr()))
        self.last_frames = (n - 1) % self.max_frames + 1
        return out

    def block(self, index: int) -> torch.Tensor:
        """output of block `index` (0..3) for the frames of the last chunk of the last call, (frames, C, h, w) float32 on the CPU (caddy_debug_fid_block)"""
        hs = _fid_block_sizes(self.H, self.W, self.resize)
        h, w = hs[index]
        buf = torch.empty(self.last_frames, FID_BLOCK_CHANNELS[index], h, w, dtype=torch.float32, device=self.device)
        self._check(self.lib.caddy_debug_fid_block(self.ctx, int(index), buf.data_ptr()))
        return buf.cpu()

    def stage_times(self, on: bool = True, read: bool = False):
        """per-stage milliseconds of the last timed chunk (input stage, stem, 35 x 35, 17 x 17, 8 x 8) when `read`; `on` switches the event recording"""
        ms = (C.c_float * 5)()
        self._check(self.lib.caddy_debug_fid_stage_ms(self.ctx, int(on), ms if read else None))
        return list(ms) if read else None


def _fid_block_sizes(H: int, W: int, resize: bool):
    """spatial sizes of the four block outputs (the trunk's unpadded 3 x 3 convolutions and stride-2 poolings)"""
    def chain(s):
        s = 299 if resize else s
        a = (s - 3) // 2 + 1 - 2
        p1 = (a - 3) // 2 + 1
        p2 = (p1 - 2 - 3) // 2 + 1
        return p1, p2, (p2 - 3) // 2 + 1
    (h0, h1, h2), (w0, w1, w2) = chain(int(H)), chain(int(W))
    return [(h0, w0), (h1, w1), (h2, w2), (1, 1)]


def _cached_fid(observations: torch.Tensor, weights, lib, resize: bool = True) -> InceptionFeatures:
    """the FID context of this library, device, frame geometry and weights (cached like _cached_lpips)"""
    H, W = int(observations.shape[-2]), int(observations.shape[-1])
    n = int(np.prod(observations.shape[:-3]))
    lib = lib if lib is not None else _default_lib
    key = ("fid", id(lib), str(observations.device), H, W, bool(resize), id(weights))
    area = 299 * 299 if resize else H * W
    want = min(n, max(1, FID_FRAMES_256 * 299 * 299 // area))
    return _cached(key, weights, lambda: InceptionFeatures(H, W, min(want, 1024), weights, resize, lib))


def inception_features(observations: torch.Tensor, weights, lib=None, resize: bool = True) -> torch.Tensor:
    """(bs, T, 3, H, W) or (n, 3, H, W) frames in [0, 1] -> (n, 2048) float64 pool_3 features (evaluation/metrics/fid.py:98-137)"""
    if weights is None:
        raise ValueError("FID needs Inception weights (see fid_inception_state)")
    return _cached_fid(observations, weights, lib, resize)(observations)


def activation_statistics(features):
    """(mu, sigma) of evaluation/metrics/fid.py:93-96: the mean and np.cov(features, rowvar=False), fp64 on the host"""
    act = np.asarray(features, dtype=np.float64)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + Tr(S1 + S2 - 2 sqrt(S1 S2)) (evaluation/metrics/fid.py:24-75).  Tr sqrt(S1 S2) is the sum of the square roots of the eigenvalues of the symmetric
    positive semi-definite S1^(1/2) S2 S1^(1/2) (similar to S1 S2), from two symmetric eigen-decompositions in fp64 with eigenvalues below the rank tolerance set to 0: the quantity the
    reference's scipy.linalg.sqrtm computes, without its complex or singular branches."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape or s1.shape != s2.shape:
        raise ValueError("Training and test statistics have different dimensions")
    def significant(values):
        # eigh returns the zero eigenvalues of a rank-deficient matrix (N samples < d dimensions: rank <= N - 1) as noise of size eps |A|, and the square root turns 1e-17 into
        # 3e-9 -- times ~2000 null directions that is 1e-5 of spurious trace.  Eigenvalues below d eps max|lambda| (the tolerance of numpy.linalg.matrix_rank) are zeros.
        top = float(values.max()) if values.size else 0.0
        return np.where(values > values.size * np.finfo(np.float64).eps * max(top, 0.0), values, 0.0)
    w, v = np.linalg.eigh((s1 + s1.T) / 2)
    root = (v * np.sqrt(significant(w))) @ v.T
    m = root @ ((s2 + s2.T) / 2) @ root
    ev = np.linalg.eigvalsh((m + m.T) / 2)
    tr_covmean = float(np.sqrt(significant(ev)).sum())
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * tr_covmean)


def fid_from_features(reference_features, generated_features) -> float:
    m1, s1 = activation_statistics(reference_features)
    m2, s2 = activation_statistics(generated_features)
    return frechet_distance(m1, s1, m2, s2)


def fid(reference_observations: torch.Tensor, generated_observations: torch.Tensor, weights, lib=None, resize: bool = True) -> float:
    """FID between two sets of frames in [0, 1] (evaluation/metrics/fid.py:140-159); every frame of every sequence is a sample"""
    return fid_from_features(inception_features(reference_observations, weights, lib, resize).numpy(),
                             inception_features(generated_observations, weights, lib, resize).numpy())


# ---- Inception Score (caddy_is_probabilities + the host fp64 score) ----
IS_CLASSES = 1000


def is_param_table(lib=None):
    """[(name, offset, shape)] of caddy_is_param_info_get: the trunk's tensors under torchvision's names in graph order, then fc.weight and fc.bias"""
    from . import _lib
    L = _bind(lib if lib is not None else (_default_lib if _default_lib is not None else _lib.load()))
    return _param_table(L.caddy_is_param_count, L.caddy_is_param_info_get)


def is_inception_state(state_dict: Dict[str, torch.Tensor], lib=None) -> Dict[str, torch.Tensor]:
    """The tensors of torchvision's inception_v3 (evaluation/metrics/inception_score.py:20) under the names of caddy_is_param_info_get: the trunk and `fc.*`.  Key handling as
    fid_inception_state (a `module.` / `model.` prefix, a {"state_dict": ...} wrapper); `AuxLogits.*` and `num_batches_tracked` are ignored.  A missing tensor raises
    CaddyError naming it."""
    from .engine import CaddyError
    src = state_dict.get("state_dict", state_dict) if isinstance(state_dict, dict) else state_dict
    out = {}
    for name, _, _ in is_param_table(lib):
        key = next((k for k in (name, "module." + name, "model." + name) if k in src), None)
        if key is None:
            raise CaddyError(f"Inception Score weights lack {name}")
        out[name] = src[key]
    return out


def find_is_weights(cfg) -> Optional[Dict[str, torch.Tensor]]:
    """config["evaluation"] -> is_inception_state(...) of `is_inception_weights` (a path or a dict); None when it is not configured.  Nothing is downloaded."""
    src = cfg.get("is_inception_weights", None)
    if src is None:
        return None
    if isinstance(src, str):
        src = torch.load(src, map_location="cpu", weights_only=True)
    return is_inception_state(src)


class InceptionProbabilities(_EvalContext):
    """The Inception Score's classifier for frames of height x width: torchvision's inception_v3(transform_input=False).eval() behind the 299 x 299 bilinear resize and the softmax
    (evaluation/metrics/inception_score.py:20-22,41-43) on csrc/fid.hip.  Calling it on (bs, T, 3, H, W) or (n, 3, H, W) frames in [0, 1] returns an (n, 1000) float32 CPU tensor;
    more than `max_frames` frames run in chunks.  resize=False runs the network at the frames' own size (at least 75 x 75)."""

    def __init__(self, height: int, width: int, max_frames: int, weights, resize: bool = True, lib=None, device=None):
        super().__init__(height, width, max_frames, lib, device)
        self.resize = bool(resize)
        table = is_param_table(self.lib)
        state = is_inception_state(weights, self.lib)
        self._create(self.lib.caddy_is_workspace_bytes, self.lib.caddy_is_ctx_create, int(self.resize))
        self._load(self.lib.caddy_load_is_inception, self.lib.caddy_is_param_floats(), table, state, "Inception Score", staging="cpu")

    def set_precision(self, forward: int):
        """arithmetic of the convolutions and of fc: 16 (split f16, default) | 0 (exact fp32)"""
        self._check(self.lib.caddy_set_is_precision(self.ctx, int(forward)))

    def fallback_layers(self) -> int:
        return int(self.lib.caddy_debug_is_fallback_layers(self.ctx))

    def __call__(self, observations: torch.Tensor) -> torch.Tensor:
        o = observations
        if o.dim() == 5:
            o = o.reshape((-1,) + tuple(o.shape[2:]))      # every frame of every sequence is a row of all_preds (inception_score.py:39-46)
        if o.dim() != 4 or o.shape[1] != 3 or tuple(o.shape[2:]) != (self.H, self.W):
            raise ValueError(f"expected (bs, observations_count, 3, {self.H}, {self.W}) or (n, 3, {self.H}, {self.W}) frames, got {tuple(observations.shape)}")
        n = int(o.shape[0])
        o = o.detach().to(self.device, torch.float32).contiguous()
        out = torch.empty(n, IS_CLASSES, dtype=torch.float32)
        self._stream()
        self._check(self.lib.caddy_is_probabilities(self.ctx, o.data_ptr(), n, out.data_ptr()))
        self.last_frames = (n - 1) % self.max_frames + 1
        return out

    def logits(self) -> torch.Tensor:
        """the (frames, 1000) float32 logits of the last chunk of the last call, on the CPU (caddy_debug_is_logits)"""
        buf = torch.empty(self.last_frames, IS_CLASSES, dtype=torch.float32, device=self.device)
        self._check(self.lib.caddy_debug_is_logits(self.ctx, buf.data_ptr()))
        return buf.cpu()

    def stage_times(self, on: bool = True, read: bool = False):
        """per-stage milliseconds of the last timed chunk (input stage, stem, 35 x 35, 17 x 17, 8 x 8, fc + softmax) when `read`; `on` switches the event recording"""
        ms = (C.c_float * 6)()
        self._check(self.lib.caddy_debug_is_stage_ms(self.ctx, int(on), ms if read else None))
        return list(ms) if read else None


def _cached_is(observations: torch.Tensor, weights, lib, resize: bool = True) -> InceptionProbabilities:
    """the Inception Score context of this library, device, frame geometry and weights (cached like _cached_fid)"""
    H, W = int(observations.shape[-2]), int(observations.shape[-1])
    n = int(np.prod(observations.shape[:-3]))
    lib = lib if lib is not None else _default_lib
    key = ("is", id(lib), str(observations.device), H, W, bool(resize), id(weights))
    area = 299 * 299 if resize else H * W
    want = min(n, max(1, FID_FRAMES_256 * 299 * 299 // area))
    return _cached(key, weights, lambda: InceptionProbabilities(H, W, min(want, 1024), weights, resize, lib))


def inception_probabilities(observations: torch.Tensor, weights, lib=None, resize: bool = True) -> torch.Tensor:
    """(bs, T, 3, H, W) or (n, 3, H, W) frames in [0, 1] -> (n, 1000) float32 class probabilities (evaluation/metrics/inception_score.py:39-46)"""
    if weights is None:
        raise ValueError("the Inception Score needs Inception weights (see is_inception_state)")
    return _cached_is(observations, weights, lib, resize)(observations)


def inception_score_from_probabilities(probs, splits: int = 1) -> Dict[str, float]:
    """{"is/mean", "is/std"} of evaluation/metrics/inception_score.py:48-65 in host fp64: for each of `splits` parts of N // splits rows (the tail is dropped)
    exp(mean_i KL(p_i || mean_j p_j)), with scipy.stats.entropy's renormalisation of both arguments; the mean and the population standard deviation over the parts."""
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim != 2:
        raise ValueError(f"expected (n, classes) probabilities, got {p.shape}")
    n, splits = p.shape[0], int(splits)
    if splits < 1 or splits > n:
        raise ValueError(f"inception score: {splits} splits of {n} rows (a part would be empty)")
    size, scores = n // splits, []
    for k in range(splits):
        part = p[k * size:(k + 1) * size]
        py = part.mean(axis=0)
        pk, qk = part / part.sum(axis=1, keepdims=True), py / py.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = np.where(pk > 0, pk * np.log(pk / qk), 0.0)      # rel_entr: 0 where p = 0 (q = 0 with p > 0 cannot occur: q is the mean of the p)
        scores.append(np.exp(terms.sum(axis=1).mean()))
    return {"is/mean": float(np.mean(scores)), "is/std": float(np.std(scores))}


def inception_score(observations: torch.Tensor, weights, splits: int = 1, resize: bool = True, lib=None) -> Dict[str, float]:
    """Inception Score of frames in [0, 1] (evaluation/metrics/inception_score.py:24-65); every frame of every sequence is a sample"""
    return inception_score_from_probabilities(inception_probabilities(observations, weights, lib, resize).numpy(), splits)


# ---- FVD (caddy_fvd_embeddings + the host fp64 statistics of FID) ----
FVD_DIM = 400
FVD_SIZE = 224
FVD_BATCH = 16                # IncrementalFVD feeds I3D 16 sequences at a time and drops the incomplete tail (evaluation/metrics/fvd.py:270-280,322-324)
FVD_VIDEOS_30x224 = 8         # videos per I3D chunk at 30 frames of 224 x 224 (scaled by the video volume): ~1.7 GB of activations
FVD_BLOCK_CHANNELS = (192, 480, 832, 1024)      # Conv3d_2c_3x3, Mixed_3c, Mixed_4f, Mixed_5c
FVD_PREFIX = "RGB/inception_i3d/"
FVD_ALIAS = {"Mixed_5b/Branch_2/Conv3d_0b_3x3/": "Mixed_5b/Branch_2/Conv3d_0a_3x3/"}      # the published checkpoint's name of that unit


def fvd_param_table(lib=None):
    """[(name, offset, shape, optional)] of caddy_fvd_param_info_get: the I3D variables under their TF names (prefix and `:0` stripped) in graph order, convolution filters
    DHWIO; the trailing optional entries are the batch-norm gammas"""
    from . import _lib
    from .engine import ParamInfo
    L = _bind(lib if lib is not None else (_default_lib if _default_lib is not None else _lib.load()))
    info, five, table = ParamInfo(), (C.c_int * 5)(), []
    for i in range(L.caddy_fvd_param_count()):
        L.caddy_fvd_param_info_get(i, C.byref(info), five)
        shape = tuple(five) if five[0] else tuple(info.shape[:info.ndim])
        table.append((info.name.decode(), int(info.offset), shape, info.kind == 4))
    return table


def _load_state_file(path):
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    return torch.load(path, map_location="cpu", weights_only=True)


def fvd_i3d_state(state, lib=None) -> Dict[str, torch.Tensor]:
    """The I3D variables of the FVD module (evaluation/metrics/fvd.py:67-71) under the names of caddy_fvd_param_info_get, from a dict, an .npz or a torch.save'd dict.  Keys may
    carry the `RGB/inception_i3d/` prefix (under any module scope), a `:0` suffix, a `module.` prefix or a {"state_dict": ...} wrapper; Mixed_5b/Branch_2's second convolution is accepted under either of
    its two names; batch-norm statistics may have any shape that squeezes to (C,); gamma is optional (1 without it, as the module has no scale); other tensors are ignored.
    A missing tensor raises CaddyError naming it, a wrong shape one naming the tensor."""
    from .engine import CaddyError
    src = _load_state_file(state) if isinstance(state, (str, bytes)) or hasattr(state, "__fspath__") else state
    src = src.get("state_dict", src) if isinstance(src, dict) else src
    clean = {}
    for k, v in src.items():
        k = k[:-2] if k.endswith(":0") else k
        k = k[len("module."):] if k.startswith("module.") else k
        k = k[k.index(FVD_PREFIX) + len(FVD_PREFIX):] if FVD_PREFIX in k else k      # (whatever scope the module was instantiated under)
        clean[k] = v
    out = {}
    for name, _, shape, optional in fvd_param_table(lib):
        keys = [name] + [name.replace(a, b) for a, b in FVD_ALIAS.items() if name.startswith(a)]
        key = next((k for k in keys if k in clean), None)
        if key is None:
            if optional:
                continue
            raise CaddyError(f"FVD I3D weights lack {name}")
        t = torch.as_tensor(clean[key])
        if len(shape) == 1 and t.numel() == shape[0]:
            t = t.reshape(shape)
        if tuple(t.shape) != shape:
            raise CaddyError(f"FVD I3D {name}: shape {tuple(t.shape)}, expected {shape}")
        out[name] = t
    return out


def find_fvd_weights(cfg) -> Optional[Dict[str, torch.Tensor]]:
    """config["evaluation"] -> fvd_i3d_state(...) of `fvd_i3d_weights` (a path or a dict); None when it is not configured.  Nothing is downloaded."""
    src = cfg.get("fvd_i3d_weights", None)
    return None if src is None else fvd_i3d_state(src)


class I3DEmbeddings(_EvalContext):
    """The FVD feature network for videos of `frames` frames of height x width: the Kinetics-400 I3D of evaluation/metrics/fvd.py:67-126 on csrc/fvd.hip.  Calling it on
    (bs, frames, 3, H, W) videos in [0, 1] returns a (bs, 400) float64 CPU tensor; more than `max_videos` videos run in chunks."""

    def __init__(self, frames: int, height: int, width: int, max_videos: int, weights, resize: bool = True, lib=None, device=None):
        super().__init__(height, width, max_videos, lib, device)
        self.T, self.resize, self.max_videos = int(frames), bool(resize), int(max_videos)
        state = fvd_i3d_state(weights, self.lib)
        table = fvd_param_table(self.lib)
        for name, _, shape, optional in table:
            if optional and name not in state:
                state[name] = torch.ones(shape)
        flat_table = [(name, off, shape) for name, off, shape, _ in table]
        self._create(lambda m, h, w, r: self.lib.caddy_fvd_workspace_bytes(m, self.T, h, w, r),
                     lambda m, h, w, r, ws, n: self.lib.caddy_fvd_ctx_create(m, self.T, h, w, r, ws, n), int(self.resize))
        self._load(self.lib.caddy_load_fvd_i3d, self.lib.caddy_fvd_param_floats(), flat_table, state, "FVD I3D", staging="cpu")

    def set_precision(self, forward: int):
        """arithmetic of the convolutions: 16 (split f16, default) | 0 (exact fp32)"""
        self._check(self.lib.caddy_set_fvd_precision(self.ctx, int(forward)))

    def fallback_layers(self) -> int:
        return int(self.lib.caddy_debug_fvd_fallback_layers(self.ctx))

    def __call__(self, observations: torch.Tensor) -> torch.Tensor:
        o = observations
        if o.dim() != 5 or o.shape[2] != 3 or int(o.shape[1]) != self.T or tuple(o.shape[3:]) != (self.H, self.W):
            raise ValueError(f"expected (bs, {self.T}, 3, {self.H}, {self.W}) videos, got {tuple(o.shape)}")
        n = int(o.shape[0])
        o = o.detach().to(self.device, torch.float32).contiguous()
        out = torch.empty(n, FVD_DIM, dtype=torch.float64)
        self._stream()
        self._check(self.lib.caddy_fvd_embeddings(self.ctx, o.data_ptr(), n, out.data_ptr()))
        self.last_videos = (n - 1) % self.max_videos + 1
        return out

    def block(self, index: int) -> torch.Tensor:
        """output of Conv3d_2c_3x3 / Mixed_3c / Mixed_4f / Mixed_5c (index 0..3) for the videos of the last chunk of the last call, (videos, C, t, h, w) float32 on the CPU"""
        t, h, w = _fvd_block_sizes(self.T, self.H, self.W, self.resize)[index]
        buf = torch.empty(self.last_videos, FVD_BLOCK_CHANNELS[index], t, h, w, dtype=torch.float32, device=self.device)
        self._check(self.lib.caddy_debug_fvd_block(self.ctx, int(index), buf.data_ptr()))
        return buf.cpu()

    def stage_times(self, on: bool = True, read: bool = False):
        """per-stage milliseconds of the last timed chunk (input stage, stem, Mixed_3, Mixed_4, Mixed_5 + head) when `read`; `on` switches the event recording"""
        ms = (C.c_float * 5)()
        self._check(self.lib.caddy_debug_fvd_stage_ms(self.ctx, int(on), ms if read else None))
        return list(ms) if read else None


def _fvd_block_sizes(T: int, H: int, W: int, resize: bool):
    """(t, h, w) of the four tapped outputs: SAME padding, so every stride-2 layer maps s to ceil(s / 2)"""
    def halve(s, times):
        for _ in range(times):
            s = (s + 1) // 2
        return s
    h, w = (FVD_SIZE, FVD_SIZE) if resize else (int(H), int(W))
    return [(halve(T, 1), halve(h, 2), halve(w, 2)), (halve(T, 1), halve(h, 3), halve(w, 3)), (halve(T, 2), halve(h, 4), halve(w, 4)), (halve(T, 3), halve(h, 5), halve(w, 5))]


def _cached_fvd(observations: torch.Tensor, weights, lib, resize: bool = True) -> I3DEmbeddings:
    """the FVD context of this library, device, video geometry and weights (cached like _cached_fid)"""
    n, T, _, H, W = (int(v) for v in observations.shape)
    lib = lib if lib is not None else _default_lib
    key = ("fvd", id(lib), str(observations.device), T, H, W, bool(resize), id(weights))
    volume = T * (FVD_SIZE * FVD_SIZE if resize else H * W)
    want = min(n, max(1, FVD_VIDEOS_30x224 * 30 * FVD_SIZE * FVD_SIZE // volume))
    return _cached(key, weights, lambda: I3DEmbeddings(T, H, W, min(want, 1024), weights, resize, lib))


def i3d_embeddings(observations: torch.Tensor, weights, lib=None, resize: bool = True) -> torch.Tensor:
    """(bs, T, 3, H, W) videos in [0, 1] -> (bs, 400) float64 I3D logits (evaluation/metrics/fvd.py:188-226)"""
    if weights is None:
        raise ValueError("FVD needs I3D weights (see fvd_i3d_state)")
    return _cached_fvd(observations, weights, lib, resize)(observations)


def fvd_from_embeddings(reference_embeddings, generated_embeddings) -> float:
    """Frechet distance of two sets of I3D logits (evaluation/metrics/fvd.py:129-152 calls tfgan's frechet_classifier_distance_from_activations): activation_statistics +
    frechet_distance.  tfgan's function is the same quantity -- fp64, unbiased covariance, Tr sqrt(S1 S2); the equality is mathematical, it is not tested against tfgan."""
    return fid_from_features(reference_embeddings, generated_embeddings)


def fvd_batched_count(n: int) -> int:
    """sequences of a dataset of n that enter the statistics: IncrementalFVD's complete batches of 16 (evaluation/metrics/fvd.py:270-280,322-324); fewer than 16 raise, as there"""
    if n < FVD_BATCH:
        raise Exception(f"FVD needs at least {FVD_BATCH} sequences per dataset (it feeds I3D {FVD_BATCH} at a time and drops the incomplete tail), got {n}")
    return FVD_BATCH * (n // FVD_BATCH)


def fvd(reference_videos: torch.Tensor, generated_videos: torch.Tensor, weights, lib=None, resize: bool = True) -> float:
    """FVD between two sets of (n, T, 3, H, W) videos in [0, 1] (evaluation/metrics/fvd.py:229-330): the first 16 floor(n / 16) videos of each set, in order"""
    r, g = reference_videos[:fvd_batched_count(len(reference_videos))], generated_videos[:fvd_batched_count(len(generated_videos))]
    return fvd_from_embeddings(i3d_embeddings(r, weights, lib, resize).numpy(), i3d_embeddings(g, weights, lib, resize).numpy())


def rollout_quality(model, batch_tuple, ground_truth_observations_init: int = 1, gumbel_temperature: float = 1.0) -> dict:
    """MSE / PSNR of an eval-mode roll-out against its ground truth, frames mapped from [-1, 1] to [0, 1] like the evaluation dataset builder
    does (evaluation_dataset_builder.py:140-153): the end-to-end quality number of the paper's protocol on the HIP path."""
    was_training = model.training
    model.eval()
    with torch.no_grad():
        rec = model(batch_tuple, ground_truth_observations_init=ground_truth_observations_init, gumbel_temperature=gumbel_temperature)[0]
    model.train(was_training)
    gt = batch_tuple[0][:, 1:, 0:3].to(rec.device, rec.dtype)
    a, b = (gt + 1) / 2, (rec + 1) / 2
    m, p = mse(a, b), psnr(a, b)
    return {"mse": m.mean().item(), "psnr": p.mean().item(), "mse_per_position": m.mean(0).tolist(), "psnr_per_position": p.mean(0).tolist()}
