"""Device-side JPEG reader (csrc/jpeg_read.hip): the files of a frame folder whose frames are .jpg -- the reference's dataset discovers the extension and reads anything with
PIL's Image.open per frame in a DataLoader worker -- and the frames of the MJPEG files the video writer leaves (video_writer.py), parsed, Huffman-decoded, inverse-transformed,
upsampled and colour-converted on the device, so that the compressed bytes cross to the device instead of raw uint8 frames and the frames appear where the frame pipeline
(frame_pipeline.FramePipeline) reads them.

    JpegDecoder          list[bytes] of complete baseline JPEG files (8-bit, three components, 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, restart markers or none) -> (uint8
                         (n, H, W, 3) frames on the device, [status]): bit for bit what Pillow decodes for every file an encoder wrote (include/caddy_hip.h states the arithmetic,
                         which is the arbiter for everything else).  A file that is refused costs its own status (STATUS_NAMES) and a zero frame; the others decode.
                         decode_stream takes the files as device tensors, e.g. a JpegEncoder's output
    cached_jpeg_decoder  the decoder of a library, device and geometry
    decode_jpegs         the frames, or ValueError naming the first file that failed
    probe                (width, height, precision, components, ((h, v), ..), SOF marker) from the markers on the host: what a caller needs to pick the context, no decoding
    unsupported          None, or why the decoder would refuse a file with that probe
    read_video           an MJPEG .avi (video_writer.write_avi) -> (info, the frames uint8 (n, H, W, 3) on the device)

Not built: progressive, arithmetic-coded, 12-bit, greyscale and CMYK / RGB-coded files, 4:4:0 / 4:1:1 sampling, multi-scan files, EXIF orientation, a parallel split of one
stream (a file without restart markers is decoded by one lane).  There is no host fallback: the kernels of the library in use (libcaddy_hip.so, or the tests' host simulator)
are the only decoder.
"""
import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import metrics as M
from .png_reader import CALL_LIMIT, _library_of, pack_files

STATUS_NAMES = ("OK", "NOT_JPEG", "TRUNCATED", "UNSUPPORTED", "GEOMETRY", "BAD_TABLE", "BAD_CODE", "BAD_COEFFICIENT", "BAD_RESTART", "BAD_SCAN")
(OK, NOT_JPEG, TRUNCATED, UNSUPPORTED, GEOMETRY, BAD_TABLE, BAD_CODE, BAD_COEFFICIENT, BAD_RESTART, BAD_SCAN) = range(10)
SAMPLINGS = (((1, 1), (1, 1), (1, 1)), ((2, 1), (1, 1), (1, 1)), ((2, 2), (1, 1), (1, 1)))      # 4:4:4, 4:2:2, 4:2:0
MAX_SIDE = 4096


def _bind(lib):
    lib = M._bind(lib)
    if not getattr(lib, "_caddy_jpeg_read_bound", False):
        lib.caddy_jpeg_read_workspace_bytes.restype = C.c_size_t
        lib.caddy_jpeg_read_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.caddy_jpeg_read_ctx_create.restype = C.c_void_p
        lib.caddy_jpeg_read_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        lib.caddy_jpeg_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib._caddy_jpeg_read_bound = True
    return lib


def probe(data) -> Tuple[int, int, int, int, Tuple[Tuple[int, int], ...], int]:
    """(width, height, precision, components, ((h, v) per component), SOF marker) of a JPEG file's first frame header: a walk over the markers, no decoding; ValueError where
    the file does not start with SOI or holds no frame header before its scan"""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file (no SOI)")
    pos = 2
    while pos + 4 <= len(data):
        if data[pos] != 0xFF:
            break
        while pos < len(data) and data[pos] == 0xFF:
            pos += 1
        if pos + 2 >= len(data):
            break
        marker, length = data[pos], (data[pos + 1] << 8) | data[pos + 2]
        if 0xC0 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC):
            seg = data[pos + 3:pos + 1 + length]
            if len(seg) < 6 or len(seg) < 6 + 3 * seg[5]:
                break
            comps = tuple((seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15) for c in range(seg[5]))
            return (seg[3] << 8) | seg[4], (seg[1] << 8) | seg[2], seg[0], seg[5], comps, marker
        if marker in (0xDA, 0xD9) or length < 2:
            break
        pos += 1 + length
    raise ValueError("not a JPEG file the reader can size (no frame header before the scan)")


def unsupported(info) -> Optional[str]:
    """None, or why caddy_jpeg_decode answers UNSUPPORTED for a file whose probe is `info`"""
    width, height, precision, components, sampling, sof = info
    if sof != 0xC0:
        return f"SOF{sof - 0xC0} (baseline sequential DCT, SOF0, only)"
    if precision != 8:
        return f"precision {precision} (8 only)"
    if components != 3:
        return f"{components} component{'s' if components != 1 else ''} (3 only)"
    if sampling not in SAMPLINGS:
        return f"sampling {sampling} (4:4:4, 4:2:2 and 4:2:0 only)"
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        return f"{width} x {height} (sides of 1..{MAX_SIDE} only)"
    return None


class JpegDecoder(M._EvalContext):
    """A JPEG-read context for images of height x width; a call with more than `max_frames` images is decoded in chunks.  `decoder(files)` -> (frames (n, H, W, 3) uint8 on the
    device, [status per file]).  `last_copied`: the bytes that call sent to the device (the files and their offsets)."""

    def __init__(self, height: int, width: int, max_frames: int, lib=None, device=None):
        super().__init__(height, width, max_frames, lib, device)
        self.lib = _bind(self.lib)
        self._create(lambda n, h, w: self.lib.caddy_jpeg_read_workspace_bytes(n, h, w),
                     lambda n, h, w, ws, nbytes: self.lib.caddy_jpeg_read_ctx_create(n, h, w, ws, nbytes))
        self.last_copied = 0

    def decode_stream(self, stream: torch.Tensor, offsets: torch.Tensor, out: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """stream: uint8 on the device, the files back to back; offsets: int32 (n + 1) on the device (as caddy_video_encode leaves them) -> (frames (n, H, W, 3) uint8, status
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
        self._check(self.lib.caddy_jpeg_decode(self.ctx, stream.data_ptr(), offsets.data_ptr(), n, frames.data_ptr(), status.data_ptr()))
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


def cached_jpeg_decoder(H: int, W: int, n_frames: int, lib=None, device=None) -> JpegDecoder:
    """the decoder of this library, device and geometry; it holds at most 256 images per chunk (one wave each in the entropy stage; a longer call runs in chunks), so it is
    never re-created for a longer batch"""
    lib = lib if lib is not None else M._default_lib
    dev = str(device) if device is not None else str(M.device(lib))
    key = ("jpeg_reader", id(lib), dev, int(H), int(W))
    room = min(256, 1 << (max(int(n_frames), 1) - 1).bit_length())
    return M._cached(key, None, lambda: JpegDecoder(H, W, room, lib, device), lambda d: d.max_frames < room)


def status_error(status: Sequence[int], names: Sequence[str] = None):
    """None, or the ValueError naming the first file that failed (its index, or its name in `names`) and its status"""
    for i, v in enumerate(status):
        if v != OK:
            what = STATUS_NAMES[v] if 0 <= v < len(STATUS_NAMES) else f"status {v}"
            return ValueError(f"JPEG file {names[i] if names is not None else i}: {what}")
    return None


def decode_jpegs(model_or_lib, files: Sequence, device=None) -> torch.Tensor:
    """complete JPEG files of one size -> uint8 (n, H, W, 3) on the device, decoded by the library of `model_or_lib` (a model, a loaded library, or None for the default one);
    ValueError names the index and the status of the first file that failed"""
    if len(files) < 1:
        raise ValueError("no files")
    width, height = probe(files[0])[:2]
    frames, status = cached_jpeg_decoder(height, width, len(files), _library_of(model_or_lib), device)(files)
    error = status_error(status)
    if error is not None:
        raise error
    return frames


def read_video(model_or_lib, path: str, device=None):
    """an MJPEG .avi as video_writer.write_avi leaves it -> (info of video_writer.read_avi, the frames uint8 (n, H, W, 3) on the device); ValueError names the first frame
    the decoder refuses"""
    from .video_writer import read_avi
    info, jpegs = read_avi(path)
    if not jpegs:
        raise ValueError(f"{path}: no frames")
    return info, decode_jpegs(model_or_lib, jpegs, device)
