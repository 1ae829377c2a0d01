"""Evaluation example sheets (csrc/sheets.hip): the contact sheets the reference's evaluator saves before it computes its losses, composed on the device.

    ground truth / reconstruction sheet   evaluation/evaluator.py:392-436 (save_examples)               one per output resolution of the forward pass
    motion-weighted sheet                 evaluation/evaluator.py:314-376, 270-301, training/losses.py:604-649   the motion-weight mask, coloured with viridis and blended over the frames
    strip                                 interpolate.py:102-158                                        one row per sequence

`ExampleSheets` reads the fp32 tensors where the forward pass left them and returns the finished uint8 image: two launches per sheet, only the image bytes cross to the host.
The arithmetic is restated in include/caddy_hip.h (caddy_sheet_examples) and DESIGN.md section 9k; the tests compare against the torch / numpy / torchvision-layout expressions
byte for byte.  There is no torch fallback: the kernels of the library in use (libcaddy_hip.so, or the tests' host simulator) are the only implementation.
"""
import ctypes as C
import logging
from typing import Optional

import numpy as np
import torch

from . import metrics as M

_log = logging.getLogger(__name__)

MAX_SEQUENCES = 30      # max_batches of evaluator.py:132,137
MAP_NONE = 0            # the values are in [0, 1] already
MAP_ALWAYS = 1          # (x + 1) / 2


def _bind(lib):
    lib = M._bind(lib)
    if not getattr(lib, "_caddy_sheets_bound", False):
        lib.caddy_sheets_workspace_bytes.restype = C.c_size_t
        lib.caddy_sheets_workspace_bytes.argtypes = [C.c_int, C.c_int]
        lib.caddy_sheets_ctx_create.restype = C.c_void_p
        lib.caddy_sheets_ctx_create.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        lib.caddy_sheet_examples.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                             C.c_void_p, C.c_void_p]
        lib.caddy_sheet_strip.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.caddy_sheet_stats_get.argtypes = [C.c_void_p, C.c_void_p]
        lib._caddy_sheets_bound = True
    return lib


def viridis_table() -> Optional[np.ndarray]:
    """(256, 3) float64: the `colors` table of matplotlib's viridis, which `colormap(w)` indexes with min((int)(w * 256), 255); None when matplotlib is not importable"""
    try:
        import matplotlib
        cmap = matplotlib.colormaps["viridis"] if hasattr(matplotlib, "colormaps") else __import__("matplotlib.cm").cm.get_cmap("viridis")
    except ImportError:
        return None
    table = np.ascontiguousarray(np.asarray(cmap.colors, dtype=np.float64))
    assert table.shape == (256, 3)
    return table


def sheet_shape(rows: int, T: int, h: int, w: int):
    """make_grid(list, nrow=T, padding=2): (rows (h + 2) + 2, T (w + 2) + 2, 3)"""
    return rows * (h + 2) + 2, T * (w + 2) + 2, 3


class ExampleSheets(M._EvalContext):
    """A SHEETS context for sheets of at most `max_rows` rows of `max_cols` cells.  `colour_table`: (256, 3) float64, by default matplotlib's viridis (None without matplotlib:
    the motion-weighted sheet is then not available).
    `examples(obs, rec, weighted=False, bias=0.0)` -> (2 min(B, 30) (h + 2) + 2, T (w + 2) + 2, 3) uint8 numpy; `strip(frames, map)` -> (n (h + 2) + 2, T (w + 2) + 2, 3);
    `stats()` -> {"mapped_gt", "mapped_rec", "saturated", "nan", "mask_invalid"} of the last sheet.  With `device_png=True` both return the sheet as a complete PNG file
    (bytes) encoded on the device (png_writer.PngEncoder): only the compressed bytes are copied."""

    def __init__(self, max_rows: int = 2 * MAX_SEQUENCES, max_cols: int = 64, lib=None, device=None, colour_table=None):
        super().__init__(0, 0, max_rows, lib, device)
        self.lib = _bind(self.lib)
        self.max_rows, self.max_cols = int(max_rows), int(max_cols)
        self._create(lambda n, h, w: self.lib.caddy_sheets_workspace_bytes(self.max_rows, self.max_cols),
                     lambda n, h, w, ws, nbytes: self.lib.caddy_sheets_ctx_create(self.max_rows, self.max_cols, ws, nbytes))
        table = viridis_table() if colour_table is None else np.ascontiguousarray(np.asarray(colour_table, dtype=np.float64))
        if table is not None and table.shape != (256, 3):
            raise ValueError(f"the colour table must be (256, 3), got {table.shape}")
        self.lut = None if table is None else torch.from_numpy(table).to(self.device)

    def _image(self, rows, T, h, w):
        return torch.empty(*sheet_shape(rows, T, h, w), dtype=torch.uint8, device=self.device)

    def _result(self, out: torch.Tensor, device_png: bool):
        if not device_png:
            return out.cpu().numpy()
        from .png_writer import FILTER_ADAPTIVE, cached_png_encoder
        return cached_png_encoder(int(out.shape[0]), int(out.shape[1]), 1, FILTER_ADAPTIVE, self.lib, self.device)(out[None])[0]

    def examples(self, obs: torch.Tensor, rec: torch.Tensor, weighted: bool = False, bias: float = 0.0, device_png: bool = False):
        if obs.dim() != 5 or obs.dtype != torch.float32 or rec.dim() != 5 or rec.dtype != torch.float32 or rec.shape[2] != 3 or rec.shape[0] != obs.shape[0]:
            raise ValueError(f"expected (B, T, 3 S, H, W) observations and (B, Trec, 3, h, w) frames, both fp32, got {tuple(obs.shape)} {obs.dtype} and {tuple(rec.shape)} {rec.dtype}")
        if weighted and self.lut is None:
            raise ValueError("the motion-weighted sheet needs matplotlib's viridis table (matplotlib is not importable and no colour_table was given)")
        obs, rec = obs.detach().to(self.device).contiguous(), rec.detach().to(self.device).contiguous()
        B, T, Cn, H, W = (int(v) for v in obs.shape)
        Trec, h, w = int(rec.shape[1]), int(rec.shape[3]), int(rec.shape[4])
        out = self._image(2 * min(B, MAX_SEQUENCES), T, h, w)
        self._stream()
        self._check(self.lib.caddy_sheet_examples(self.ctx, obs.data_ptr(), B, T, Cn, H, W, rec.data_ptr(), Trec, h, w, int(bool(weighted)), float(bias),
                                                  self.lut.data_ptr() if self.lut is not None else None, out.data_ptr()))
        return self._result(out, device_png)

    def strip(self, frames: torch.Tensor, map: int = MAP_ALWAYS, device_png: bool = False):
        if frames.dim() != 5 or frames.dtype != torch.float32 or frames.shape[2] != 3:
            raise ValueError(f"expected (n, T, 3, h, w) fp32 frames, got {tuple(frames.shape)} {frames.dtype}")
        frames = frames.detach().to(self.device).contiguous()
        n, T, _, h, w = (int(v) for v in frames.shape)
        out = self._image(n, T, h, w)
        self._stream()
        self._check(self.lib.caddy_sheet_strip(self.ctx, frames.data_ptr(), n, T, h, w, int(map), out.data_ptr()))
        return self._result(out, device_png)

    def stats(self):
        """counted on the device for the last sheet; waits for the stream"""
        v = (C.c_uint * 5)()
        self._stream()
        self._check(self.lib.caddy_sheet_stats_get(self.ctx, v))
        return {"mapped_gt": bool(v[0]), "mapped_rec": bool(v[1]), "saturated": int(v[2]), "nan": int(v[3]), "mask_invalid": bool(v[4])}


def cached_sheets(rows: int, cols: int, lib=None, device=None) -> ExampleSheets:
    """the sheet composer of this library and device, (re)created when it holds too few rows or columns"""
    lib = lib if lib is not None else M._default_lib
    dev = str(device) if device is not None else str(M.device(lib))
    key = ("example_sheets", id(lib), dev)
    room_r = max(2 * MAX_SEQUENCES, int(rows))
    room_c = max(64, 1 << (max(int(cols), 1) - 1).bit_length())
    return M._cached(key, None, lambda: ExampleSheets(room_r, room_c, lib, device), lambda es: es.max_rows < rows or es.max_cols < cols)


def evaluation_sheets(observations: torch.Tensor, multiresolution_reconstructions, bias: float, lib=None, log=None, device_png: bool = False):
    """the sheets of evaluator.py:128-138 for one forward pass -> {log key: uint8 image, or with device_png its PNG file encoded on the device}: "observations_r{i}" for every resolution and "motion_weighted_observations_" on the
    full-resolution reconstruction (multiresolution_reconstructions[0]).  The weighted sheet is left out, with a logged line, without matplotlib or when the mask holds a NaN
    or a negative value (the reference's assert)."""
    say = log if log is not None else _log.warning
    first = multiresolution_reconstructions[0]
    sheets = cached_sheets(2 * min(int(observations.shape[0]), MAX_SEQUENCES), int(observations.shape[1]), lib, first.device)
    out = {}
    for i, rec in enumerate(multiresolution_reconstructions):
        out[f"observations_r{i}"] = sheets.examples(observations, rec, device_png=device_png)
    if sheets.lut is None:
        say("motion-weighted example sheet not written: matplotlib is not available")
        return out
    image = sheets.examples(observations, first, weighted=True, bias=bias, device_png=device_png)
    if sheets.stats()["mask_invalid"]:
        say("motion-weighted example sheet not written: the motion weight mask holds a NaN or a negative value")
        return out
    out["motion_weighted_observations_"] = image
    return out
