"""Device-side frame pipeline (csrc/frames.hip): the distinct decoded uint8 frames of a batch in, the model's observation tensor out.

    crop / resize / normalise   dataset/transforms.py:13-30,90-107   PIL's 8-bit crop + bilinear resize, bit for bit, then the byte -> fp32 table of the mode
    stacking / collate          dataset/batching.py:97-112           slot i of the (bs, T, 3 S, H, W) tensor is (b, t, s) in row-major order, newest frame first

The host decodes every frame once and ships it as uint8 (`video_dataset.raw_frame_spec`, `batching.RawBatch`); `FramePipeline` runs the one kernel that does the
rest.  `FrameWriter` is the output side (evaluation/evaluation_dataset_builder.py:60-81,140-153, play.py:140): fp32 planar frames in, the uint8 interleaved frames the host
would have written out, and / or their evaluation_transform, without leaving the device.  The byte -> fp32 tables are computed here with the very expressions of the host transforms (`batching.normalize_frame`, `video_dataset.evaluation_transform`), so
both paths give the same bits by construction.  There is no torch fallback: the kernel of the library in use (libcaddy_hip.so, or the tests' host simulator) is the
only implementation.
"""
import ctypes as C
from typing import Optional, Sequence

import torch

from . import metrics as M

MODE_TRAINING = 0       # ((x / 255) - 0.5) / 0.5: final_transform / normalize_frame
MODE_EVALUATION = 1     # x / 255: evaluation_transform


def _bind(lib):
    lib = M._bind(lib)
    if not getattr(lib, "_caddy_frames_bound", False):
        lib.caddy_frames_workspace_bytes.restype = C.c_size_t
        lib.caddy_frames_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        lib.caddy_frames_ctx_create.restype = C.c_void_p
        lib.caddy_frames_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.caddy_frames_tables_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.caddy_debug_frames_plan.argtypes = [C.c_void_p, C.c_void_p]
        lib.caddy_frames_to_observations.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        lib.caddy_frames_write.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p]
        lib.caddy_frames_write_stats_get.argtypes = [C.c_void_p, C.c_void_p]
        lib._caddy_frames_bound = True
    return lib


def value_tables() -> torch.Tensor:
    """(2, 256) fp32: what the host transforms make of every byte -- row 0 as normalize_frame, row 1 as evaluation_transform"""
    from .batching import normalize_frame
    x = torch.arange(256, dtype=torch.uint8)
    training = normalize_frame(x.reshape(256, 1, 1).expand(256, 1, 3))[0].reshape(256)
    evaluation = x.float().div(255) / 1.0
    return torch.stack([training, evaluation]).contiguous()


def validate_slots(slot_src: torch.Tensor, n_frames: int) -> None:
    """every slot must name one of the batch's frames; checked on the host before anything is staged"""
    if slot_src.numel() == 0:
        raise ValueError("no slots")
    lo, hi = int(slot_src.min()), int(slot_src.max())
    if lo < 0 or hi >= n_frames:
        raise ValueError(f"slot_src names frames {lo}..{hi}, the batch holds {n_frames}")


class FramePipeline(M._EvalContext):
    """A FRAMES context for source frames of src_h x src_w, `crop` ([left, upper, right, lower] or None) and output frames of `target_size_wh` = (width, height).
    `pipeline(frames_u8, slot_src)` -> (n_slots, 3, H, W) fp32 on the device; at most `max_frames` frames per call."""

    def __init__(self, src_h: int, src_w: int, crop: Optional[Sequence[int]], target_size_wh: Sequence[int], max_frames: int, mode: int, lib=None, device=None):
        W, H = (int(v) for v in target_size_wh)
        super().__init__(H, W, max_frames, lib, device)
        self.lib = _bind(self.lib)
        if mode not in (MODE_TRAINING, MODE_EVALUATION):
            raise ValueError(f"mode must be {MODE_TRAINING} ([-1, 1]) or {MODE_EVALUATION} ([0, 1]), got {mode}")
        self.src_h, self.src_w, self.mode = int(src_h), int(src_w), int(mode)
        self.crop = None if crop is None else tuple(int(v) for v in crop)
        if self.crop is not None and len(self.crop) != 4:
            raise ValueError(f"crop must be [left, upper, right, lower], got {crop}")
        box = (C.c_int * 4)(*self.crop) if self.crop is not None else None
        lut = value_tables()
        self._create(lambda n, h, w: self.lib.caddy_frames_workspace_bytes(n, self.src_h, self.src_w, box, h, w),
                     lambda n, h, w, ws, nbytes: self.lib.caddy_frames_ctx_create(n, self.src_h, self.src_w, box, h, w, lut.data_ptr(), ws, nbytes))

    def tables(self, axis: int):
        """(runs, ksize, bounds (out, 2), kk (out, ksize)) of the horizontal (0) / vertical (1) pass: the host copies of what the kernel reads"""
        import numpy as np
        ks = C.c_int(0)
        rc = self.lib.caddy_frames_tables_get(self.ctx, int(axis), C.byref(ks), None, None)
        if rc < 0:
            self._check(rc)
        n = self.W if axis == 0 else self.H
        bounds, kk = np.zeros((n, 2), np.int32), np.zeros((n, ks.value), np.int32)
        self.lib.caddy_frames_tables_get(self.ctx, int(axis), None, bounds.ctypes.data_as(C.c_void_p), kk.ctypes.data_as(C.c_void_p))
        return bool(rc), ks.value, bounds, kk

    def plan(self):
        """{rows_per_block, max_source_rows, rows_per_round, lds_bytes, lds_variant} the kernel runs with"""
        v = (C.c_int * 5)()
        self._check(self.lib.caddy_debug_frames_plan(self.ctx, v))
        return dict(zip(("rows_per_block", "max_source_rows", "rows_per_round", "lds_bytes", "lds_variant"), (int(x) for x in v)))

    def __call__(self, frames_u8: torch.Tensor, slot_src: torch.Tensor) -> torch.Tensor:
        f = frames_u8
        if f.dim() != 4 or f.dtype != torch.uint8 or tuple(f.shape[1:]) != (self.src_h, self.src_w, 3):
            raise ValueError(f"expected (n_frames, {self.src_h}, {self.src_w}, 3) uint8 frames, got {tuple(f.shape)} {f.dtype}")
        if slot_src.device.type == "cpu":
            validate_slots(slot_src, int(f.shape[0]))
        f = f.to(self.device).contiguous()
        s = slot_src.to(self.device, torch.int32).reshape(-1).contiguous()
        out = torch.empty(s.numel(), 3, self.H, self.W, dtype=torch.float32, device=self.device)
        self._stream()
        self._check(self.lib.caddy_frames_to_observations(self.ctx, f.data_ptr(), int(f.shape[0]), s.data_ptr(), int(s.numel()), self.mode, out.data_ptr()))
        return out


def cached_pipeline(src_h: int, src_w: int, crop, target_size_wh, mode: int, n_frames: int, lib=None, device=None) -> FramePipeline:
    """the pipeline of this library, device, geometry and mode, (re)created when it holds too few frames"""
    lib = lib if lib is not None else M._default_lib
    dev = str(device) if device is not None else str(M.device(lib))
    crop_key = None if crop is None else tuple(int(v) for v in crop)
    key = ("frames", id(lib), dev, int(src_h), int(src_w), crop_key, tuple(int(v) for v in target_size_wh), int(mode))
    room = max(64, 1 << (max(int(n_frames), 1) - 1).bit_length())
    return M._cached(key, None, lambda: FramePipeline(src_h, src_w, crop, target_size_wh, room, mode, lib, device), lambda fp: fp.max_frames < n_frames)


MAP_NONE = 0            # the values are in [0, 1] already
MAP_ALWAYS = 1          # (x + 1) / 2: play.py:140
MAP_IF_NEGATIVE = 2     # (x + 1) / 2 when the minimum over everything is negative: evaluation_dataset_builder.py:140-153


def _planar_frames(t: torch.Tensor, H: int, W: int) -> bool:
    """do the (3, H, W) blocks at t[b, 0, :3] (5 dims) / t[b, :3] (4 dims) lie planar and dense in memory?"""
    return t.stride(-1) == 1 and t.stride(-2) == W and t.stride(-3) == H * W and (t.shape[0] == 1 or t.stride(0) >= 3 * H * W)


class FrameWriter(M._EvalContext):
    """The frame writer on an identity-geometry FRAMES context for frames of height x width, at most `max_frames` per call.
    `writer(rec, first=None, map=1, want_u8=True, want_f32=False)`: rec (B, Trec, 3, H, W) fp32; `first` -- (B, 3, H, W), (B, 1, 3, H, W) or a whole (B, T, 3 S, H, W)
    observation tensor, whose channels 0..2 at t = 0 are read in place -- becomes sequence position 0.  -> (B, T, H, W, 3) uint8 and / or (B, T, 3, H, W) fp32 in [0, 1]
    (one tensor, or the pair when both are wanted), on the device.  `stats()` -> {"mapped", "saturated", "nan"} of the last call."""

    def __init__(self, height: int, width: int, max_frames: int, lib=None, device=None):
        super().__init__(height, width, max_frames, lib, device)
        self.lib = _bind(self.lib)
        lut = value_tables()
        self._create(lambda n, h, w: self.lib.caddy_frames_workspace_bytes(n, h, w, None, h, w),
                     lambda n, h, w, ws, nbytes: self.lib.caddy_frames_ctx_create(n, h, w, None, h, w, lut.data_ptr(), ws, nbytes))

    def __call__(self, rec: torch.Tensor, first: Optional[torch.Tensor] = None, map: int = MAP_ALWAYS, want_u8: bool = True, want_f32: bool = False):
        if rec.dim() != 5 or rec.dtype != torch.float32 or tuple(rec.shape[2:]) != (3, self.H, self.W):
            raise ValueError(f"expected (B, T, 3, {self.H}, {self.W}) fp32 frames, got {tuple(rec.shape)} {rec.dtype}")
        if not (want_u8 or want_f32):
            raise ValueError("neither the uint8 nor the fp32 frames are wanted")
        rec = rec.to(self.device).contiguous()
        B, Trec = int(rec.shape[0]), int(rec.shape[1])
        first_ptr, first_stride = None, 0
        if first is not None:
            if first.dtype != torch.float32 or first.dim() not in (4, 5) or int(first.shape[0]) != B or tuple(first.shape[-2:]) != (self.H, self.W) or int(first.shape[-3]) < 3:
                raise ValueError(f"expected {B} first frames of (3, {self.H}, {self.W}) fp32, got {tuple(first.shape)} {first.dtype}")
            first = first.to(self.device)
            if not _planar_frames(first, self.H, self.W):
                first = (first[:, 0, :3] if first.dim() == 5 else first[:, :3]).contiguous()
            first_ptr, first_stride = first.data_ptr(), int(first.stride(0))
        T = Trec + (first is not None)
        u8 = torch.empty(B, T, self.H, self.W, 3, dtype=torch.uint8, device=self.device) if want_u8 else None
        f32 = torch.empty(B, T, 3, self.H, self.W, dtype=torch.float32, device=self.device) if want_f32 else None
        self._stream()
        self._check(self.lib.caddy_frames_write(self.ctx, rec.data_ptr(), B, Trec, first_ptr, first_stride, int(map), u8.data_ptr() if want_u8 else None,
                                                f32.data_ptr() if want_f32 else None))
        return (u8, f32) if want_u8 and want_f32 else (u8 if want_u8 else f32)

    def stats(self):
        """{"mapped": bool, "saturated": int, "nan": int} of the last call, counted on the device; waits for the stream"""
        v = (C.c_uint * 3)()
        self._stream()
        self._check(self.lib.caddy_frames_write_stats_get(self.ctx, v))
        return {"mapped": bool(v[0]), "saturated": int(v[1]), "nan": int(v[2])}


def cached_writer(height: int, width: int, n_frames: int, lib=None, device=None) -> FrameWriter:
    """the writer of this library, device and geometry, (re)created when it holds too few frames"""
    lib = lib if lib is not None else M._default_lib
    dev = str(device) if device is not None else str(M.device(lib))
    key = ("frame_writer", id(lib), dev, int(height), int(width))
    room = max(64, 1 << (max(int(n_frames), 1) - 1).bit_length())
    return M._cached(key, None, lambda: FrameWriter(height, width, room, lib, device), lambda fw: fw.max_frames < n_frames)

