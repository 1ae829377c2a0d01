"""Device-side PNG writer (csrc/png.hip): the lossless files every driver saves -- the dataset folders' NNNNN.png, the frames of `play` and `interpolate`, the evaluator's
example sheets -- filtered, deflated and framed on the device, so that only the compressed bytes cross to the host (in place of PIL's Image.save(f, format="PNG") on one host
thread over raw uint8 frames).

    PngEncoder          uint8 (n, H, W, 3) images on the device (what FrameWriter and the sheets produce), or fp32 (n, 3, H, W) through FrameWriter first -> list[bytes], one
                        complete PNG file per image: 8-bit RGB, no interlace, one IDAT.  Not Pillow's bytes: the contract is the PNG and deflate specifications -- any decoder
                        returns exactly the input and both checksums hold (include/caddy_hip.h states the filter rule and the block coding)
    cached_png_encoder  the encoder of a library, device, geometry and filter mode
    save_png            one image to a path

Not built: a general LZ77 match finder (the matches are distance-1 runs, as zlib's Z_RLE strategy finds them), palette / grey / 16-bit / alpha images, interlacing (the
decoder is png_reader.py).  There is no host fallback: the kernels of the library in use (libcaddy_hip.so, or the tests' host simulator) are the only encoder.
"""
import ctypes as C
from typing import List, Sequence

import torch

from . import metrics as M
from .frame_pipeline import MAP_ALWAYS, cached_writer

FILTER_NONE, FILTER_SUB, FILTER_UP, FILTER_AVERAGE, FILTER_PAETH, FILTER_ADAPTIVE = range(6)
BLOCK = 16384            # filtered-stream bytes per deflate block (CADDY_PNG_BLOCK)
CALL_LIMIT = (1 << 31) - 1


def _bind(lib):
    lib = M._bind(lib)
    if not getattr(lib, "_caddy_png_bound", False):
        lib.caddy_png_workspace_bytes.restype = C.c_size_t
        lib.caddy_png_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.caddy_png_ctx_create.restype = C.c_void_p
        lib.caddy_png_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        lib.caddy_png_stream_bound.restype = C.c_size_t
        lib.caddy_png_stream_bound.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.caddy_png_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        lib._caddy_png_bound = True
    return lib


class PngEncoder(M._EvalContext):
    """A PNG context for images of height x width; a call with more than `max_frames` images is encoded in chunks.  `filter_mode`: FILTER_ADAPTIVE (per row, the type with
    the smallest sum of |int8|) or one fixed type 0..4.  `encoder(frames, map=MAP_ALWAYS)` -> list[bytes]: frames (n, H, W, 3) uint8 on the device, or (n, 3, H, W) fp32,
    which the frame writer quantises first under `map` (frame_pipeline.MAP_*).  `last_offsets`: where each file of the last call started in the stream, and its total length.
    `last_copied`: the bytes that call copied to the host (the offsets and the compressed stream)."""

    def __init__(self, height: int, width: int, max_frames: int, filter_mode: int = FILTER_ADAPTIVE, lib=None, device=None):
        super().__init__(height, width, max_frames, lib, device)
        self.lib = _bind(self.lib)
        self.filter_mode = int(filter_mode)
        self._create(lambda n, h, w: self.lib.caddy_png_workspace_bytes(n, h, w),
                     lambda n, h, w, ws, nbytes: self.lib.caddy_png_ctx_create(n, h, w, self.filter_mode, ws, nbytes))
        self._out = None
        self.last_offsets, self.last_copied = [0], 0

    def stream_bound(self, n: int) -> int:
        """the output capacity no input of n images can exceed"""
        return int(self.lib.caddy_png_stream_bound(int(n), self.H, self.W))

    def _frames_u8(self, frames: torch.Tensor, map: int) -> torch.Tensor:
        if frames.dim() == 4 and frames.dtype == torch.uint8 and tuple(frames.shape[1:]) == (self.H, self.W, 3):
            return frames.to(self.device).contiguous()
        if frames.dim() == 4 and frames.dtype == torch.float32 and tuple(frames.shape[1:]) == (3, self.H, self.W):
            writer = cached_writer(self.H, self.W, int(frames.shape[0]), self.lib, self.device)
            return writer(frames.detach().to(self.device)[None], map=map)[0]
        raise ValueError(f"expected (n, {self.H}, {self.W}, 3) uint8 or (n, 3, {self.H}, {self.W}) fp32 frames, got {tuple(frames.shape)} {frames.dtype}")

    def __call__(self, frames: torch.Tensor, map: int = MAP_ALWAYS) -> List[bytes]:
        u8 = self._frames_u8(frames, map)
        n = int(u8.shape[0])
        if n < 1:
            raise ValueError("no frames")
        step = max(1, min(n, CALL_LIMIT // self.stream_bound(1)))      # (the offsets of one call are 32-bit words)
        files, offsets, copied = [], [0], 0
        for n0 in range(0, n, step):
            part = u8[n0:n0 + step]
            k = int(part.shape[0])
            bound = self.stream_bound(k)
            if self._out is None or self._out.numel() < bound:
                self._out = torch.empty(bound, dtype=torch.uint8, device=self.device)
            off = torch.empty(k + 1, dtype=torch.int32, device=self.device)
            self._stream()
            self._check(self.lib.caddy_png_encode(self.ctx, part.data_ptr(), k, self._out.data_ptr(), bound, off.data_ptr()))
            o = [int(v) & 0xFFFFFFFF for v in off.cpu().tolist()]
            stream = self._out[:o[k]].cpu().numpy().tobytes()      # only the compressed bytes are copied
            copied += 4 * (k + 1) + o[k]
            files += [stream[o[i]:o[i + 1]] for i in range(k)]
            offsets += [offsets[n0] + v for v in o[1:]]
        self.last_offsets, self.last_copied = offsets, copied
        return files


def cached_png_encoder(H: int, W: int, n_frames: int, filter_mode: int = FILTER_ADAPTIVE, lib=None, device=None) -> PngEncoder:
    """the encoder of this library, device, geometry and filter mode; it holds at most 64 images per chunk (a longer call runs in chunks), so it is never re-created for a
    longer sequence"""
    lib = lib if lib is not None else M._default_lib
    dev = str(device) if device is not None else str(M.device(lib))
    key = ("png_writer", id(lib), dev, int(H), int(W), int(filter_mode))
    room = min(64, 1 << (max(int(n_frames), 1) - 1).bit_length())
    return M._cached(key, None, lambda: PngEncoder(H, W, room, filter_mode, lib, device), lambda e: e.max_frames < room)


def _library_of(model_or_lib):
    if model_or_lib is None or isinstance(model_or_lib, C.CDLL):
        return model_or_lib
    return getattr(getattr(model_or_lib, "module", model_or_lib), "_lib", None)


def encode_pngs(model_or_lib, frames: torch.Tensor, map: int = MAP_ALWAYS) -> List[bytes]:
    """frames (n, H, W, 3) uint8 or (n, 3, H, W) fp32 (quantised under `map`), encoded on the device of `frames` (host frames are staged on the library's device) by the
    library of `model_or_lib` (a model, a loaded library, or None for the default one) -> one PNG file per frame"""
    if frames.dim() != 4:
        raise ValueError(f"expected (n, H, W, 3) uint8 or (n, 3, H, W) fp32 frames, got {tuple(frames.shape)}")
    H, W = (int(frames.shape[1]), int(frames.shape[2])) if frames.dtype == torch.uint8 else (int(frames.shape[2]), int(frames.shape[3]))
    lib = _library_of(model_or_lib)
    device = frames.device if frames.device.type == M.device(lib).type else None
    return cached_png_encoder(H, W, int(frames.shape[0]), FILTER_ADAPTIVE, lib, device)(frames, map=map)


def write_files(files: Sequence[bytes], paths: Sequence[str]) -> int:
    """ready files to their paths -> the bytes written"""
    if len(files) != len(paths):
        raise ValueError(f"{len(files)} files for {len(paths)} paths")
    for data, path in zip(files, paths):
        with open(path, "wb") as f:
            f.write(data)
    return sum(len(d) for d in files)


def save_png(model_or_lib, image: torch.Tensor, path: str, map: int = MAP_ALWAYS) -> int:
    """one image, (H, W, 3) uint8 or (3, H, W) fp32, to `path` -> the bytes written"""
    return write_files(encode_pngs(model_or_lib, image[None], map), [path])
