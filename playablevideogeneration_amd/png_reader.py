"""Device-side PNG reader (csrc/png_read.hip): the files of a frame folder -- NNNNN.png, what the reference's dataset reads with PIL's Image.open per frame in a DataLoader
worker -- parsed, inflated and unfiltered on the device, so that the compressed bytes cross to the device instead of raw uint8 frames and the frames appear where the frame
pipeline (frame_pipeline.FramePipeline) reads them.

    PngDecoder          list[bytes] of complete PNG files (8-bit RGB, no interlace, any number of IDATs) -> (uint8 (n, H, W, 3) frames on the device, [status]): bit for bit
                        what Pillow decodes; a zlib stream is accepted exactly where zlib's inflate accepts it (include/caddy_hip.h states the rules).  A file that is refused
                        costs its own status (STATUS_NAMES) and a zero frame; the others decode.  decode_stream takes the files as device tensors, e.g. a PngEncoder's output
    cached_png_decoder  the decoder of a library, device and geometry
    decode_pngs         the frames, or ValueError naming the first file that failed
    probe               (width, height, bit depth, colour type, interlace) from the first 29 bytes on the host: what a caller needs to pick the context, no decoding

Not built: palette / grey / 16-bit / alpha images, interlacing, a parallel split of one stream (inflate is one lane per image).  There is no host fallback: the
kernels of the library in use (libcaddy_hip.so, or the tests' host simulator) are the only decoder.
"""
import ctypes as C
import struct
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import metrics as M

STATUS_NAMES = ("OK", "NOT_PNG", "TRUNCATED", "BAD_CRC", "UNSUPPORTED", "GEOMETRY", "BAD_DEFLATE", "BAD_ADLER", "BAD_LENGTH", "BAD_FILTER", "TOO_LARGE")
(OK, NOT_PNG, TRUNCATED, BAD_CRC, UNSUPPORTED, GEOMETRY, BAD_DEFLATE, BAD_ADLER, BAD_LENGTH, BAD_FILTER, TOO_LARGE) = range(11)
CALL_LIMIT = (1 << 32) - 1       # the offsets of one call are 32-bit words
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _bind(lib):
    lib = M._bind(lib)
    if not getattr(lib, "_caddy_png_read_bound", False):
        lib.caddy_png_read_workspace_bytes.restype = C.c_size_t
        lib.caddy_png_read_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.caddy_png_read_ctx_create.restype = C.c_void_p
        lib.caddy_png_read_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        lib.caddy_png_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib._caddy_png_read_bound = True
    return lib


def probe(data) -> Tuple[int, int, int, int, int]:
    """(width, height, bit depth, colour type, interlace) of a PNG file's IHDR; ValueError where the first 29 bytes are not a signature and an IHDR"""
    head = bytes(data[:29])
    if len(head) < 29 or head[:8] != SIGNATURE or head[8:16] != b"\x00\x00\x00\x0dIHDR":
        raise ValueError("not a PNG file (no signature and IHDR in the first 29 bytes)")
    width, height, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", head[16:29])
    return width, height, depth, colour, interlace


def pack_files(files: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """files (bytes or uint8 arrays) -> (the blob uint8, the n + 1 offsets int64)"""
    parts = [np.frombuffer(f, np.uint8) if isinstance(f, (bytes, bytearray, memoryview)) else np.asarray(f, np.uint8).reshape(-1) for f in files]
    offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([p.size for p in parts], out=offsets[1:])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), offsets


class PngDecoder(M._EvalContext):
    """A PNG-read context for images of height x width; a call with more than `max_frames` images is decoded in chunks.  `decoder(files)` -> (frames (n, H, W, 3) uint8 on the
    device, [status per file]).  `last_copied`: the bytes that call sent to the device (the files and their offsets)."""

    def __init__(self, height: int, width: int, max_frames: int, lib=None, device=None):
        super().__init__(height, width, max_frames, lib, device)
        self.lib = _bind(self.lib)
        self._create(lambda n, h, w: self.lib.caddy_png_read_workspace_bytes(n, h, w),
                     lambda n, h, w, ws, nbytes: self.lib.caddy_png_read_ctx_create(n, h, w, ws, nbytes))
        self.last_copied = 0

    def decode_stream(self, stream: torch.Tensor, offsets: torch.Tensor, out: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """stream: uint8 on the device, the files back to back; offsets: int32 (n + 1) on the device (as caddy_png_encode leaves them) -> (frames (n, H, W, 3) uint8, status
        int32 (n)), both on the device: nothing is copied and nothing waited for"""
        if stream.dtype != torch.uint8 or offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2:
            raise ValueError(f"expected a uint8 stream and n + 1 int32 offsets, got {stream.dtype} and {offsets.dtype} {tuple(offsets.shape)}")
        if stream.device.type != self.device.type or offsets.device.type != self.device.type:
            raise ValueError(f"the stream and the offsets must lie on {self.device}")
        n = int(offsets.numel()) - 1
        stream, offsets = stream.contiguous().reshape(-1), offsets.contiguous()
        if stream.numel() == 0:
            stream = torch.zeros(1, dtype=torch.uint8, device=self.device)      # (a pointer to hand over; offsets[n] says that nothing of it is read)
        frames = out if out is not None else torch.empty((n, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        if tuple(frames.shape) != (n, self.H, self.W, 3) or frames.dtype != torch.uint8 or not frames.is_contiguous():
            raise ValueError(f"expected a contiguous uint8 ({n}, {self.H}, {self.W}, 3) output")
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        self._stream()
        self._check(self.lib.caddy_png_decode(self.ctx, stream.data_ptr(), offsets.data_ptr(), n, frames.data_ptr(), status.data_ptr()))
        return frames, status

    def __call__(self, files: Sequence) -> Tuple[torch.Tensor, List[int]]:
        if len(files) < 1:
            raise ValueError("no files")
        frames = torch.empty((len(files), self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        status, copied, n0 = [], 0, 0
        while n0 < len(files):      # (the offsets of one call are 32-bit words)
            n1, total = n0, 0
            while n1 < len(files) and (n1 == n0 or total + len(files[n1]) <= CALL_LIMIT):
                total += len(files[n1])
                n1 += 1
            if total > CALL_LIMIT:
                raise ValueError(f"file {n0} has {total} bytes: more than the 32-bit offsets hold")
            blob, offsets = pack_files(files[n0:n1])
            _, st = self.decode_stream(torch.from_numpy(blob).to(self.device), torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(self.device), frames[n0:n1])
            status += [int(v) for v in st.cpu().tolist()]
            copied += blob.size + 4 * offsets.size
            n0 = n1
        self.last_copied = copied
        return frames, status


def cached_png_decoder(H: int, W: int, n_frames: int, lib=None, device=None) -> PngDecoder:
    """the decoder of this library, device and geometry; it holds at most 256 images per chunk (one wave each; a longer call runs in chunks), so it is never re-created for
    a longer batch"""
    lib = lib if lib is not None else M._default_lib
    dev = str(device) if device is not None else str(M.device(lib))
    key = ("png_reader", id(lib), dev, int(H), int(W))
    room = min(256, 1 << (max(int(n_frames), 1) - 1).bit_length())
    return M._cached(key, None, lambda: PngDecoder(H, W, room, lib, device), lambda d: d.max_frames < room)


def _library_of(model_or_lib):
    if model_or_lib is None or isinstance(model_or_lib, C.CDLL):
        return model_or_lib
    return getattr(getattr(model_or_lib, "module", model_or_lib), "_lib", None)


def status_error(status: Sequence[int], names: Sequence[str] = None):
    """None, or the ValueError naming the first file that failed (its index, or its name in `names`) and its status"""
    for i, v in enumerate(status):
        if v != OK:
            what = STATUS_NAMES[v] if 0 <= v < len(STATUS_NAMES) else f"status {v}"
            return ValueError(f"PNG file {names[i] if names is not None else i}: {what}")
    return None


def decode_pngs(model_or_lib, files: Sequence, device=None) -> torch.Tensor:
    """complete PNG files of one size -> uint8 (n, H, W, 3) on the device, decoded by the library of `model_or_lib` (a model, a loaded library, or None for the default one);
    ValueError names the index and the status of the first file that failed"""
    if len(files) < 1:
        raise ValueError("no files")
    width, height = probe(files[0])[:2]
    frames, status = cached_png_decoder(height, width, len(files), _library_of(model_or_lib), device)(files)
    error = status_error(status)
    if error is not None:
        raise error
    return frames
