"""Device-side MJPEG video writer (csrc/video.hip): what the reference's drivers end every sequence with (utils/save_video_ffmpeg.py:172-198, play.py:192,
interpolate.py:147, framerate = 5), without ffmpeg: the frames are encoded as baseline JPEG on the device and only the encoded bytes cross to the host, where they are put
into an AVI container with `struct`.

    JpegEncoder      uint8 (n, H, W, 3) frames on the device (what FrameWriter produces), or fp32 (n, 3, H, W) through FrameWriter first -> list[bytes], one complete JPEG
                     file per frame: byte for byte what Pillow's Image.save(f, format="JPEG", quality=q, subsampling=0, optimize=False) writes (libjpeg's integer path:
                     jccolor.c, jfdctint.c, jchuff.c with the Annex K tables; 4:4:4, one interleaved scan, no restart markers)
    write_avi        RIFF 'AVI ' with one 'vids' / 'MJPG' stream, an idx1 index, no OpenDML (a file that would pass 2 GiB raises); read_avi reads it back
    save_video       the two together

Not built: the action number and timecode overlays of save_action_video / timecode_video (a TrueType rasteriser), mp4 / H.264, chroma subsampling and optimised Huffman
tables.  There is no torch fallback: the kernels of the library in use (libcaddy_hip.so, or the tests' host simulator) are the only encoder.
"""
import ctypes as C
import os
import struct
from fractions import Fraction
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import metrics as M
from .frame_pipeline import MAP_ALWAYS, cached_writer

DEFAULT_FPS = 5          # `framerate` of play.py:192 / interpolate.py:147
DEFAULT_QUALITY = 90
AVI_LIMIT = (1 << 31) - 1


def _bind(lib):
    lib = M._bind(lib)
    if not getattr(lib, "_caddy_video_bound", False):
        lib.caddy_video_workspace_bytes.restype = C.c_size_t
        lib.caddy_video_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.caddy_video_ctx_create.restype = C.c_void_p
        lib.caddy_video_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        lib.caddy_video_stream_bound.restype = C.c_size_t
        lib.caddy_video_stream_bound.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.caddy_video_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.caddy_video_tables_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib._caddy_video_bound = True
    return lib


class JpegEncoder(M._EvalContext):
    """A VIDEO context for frames of height x width at `quality` (1..100); a call with more than `max_frames` frames is encoded in chunks.
    `encoder(frames, map=MAP_ALWAYS)` -> list[bytes]: frames (n, H, W, 3) uint8 on the device, or (n, 3, H, W) fp32, which the frame writer quantises first under `map`
    (frame_pipeline.MAP_*).  `last_offsets`: where each file of the last call started in the stream, and its total length.  `last_copied`: the bytes that call copied to the
    host (the offsets and the encoded stream)."""

    def __init__(self, height: int, width: int, max_frames: int, quality: int = DEFAULT_QUALITY, lib=None, device=None):
        super().__init__(height, width, max_frames, lib, device)
        self.lib = _bind(self.lib)
        self.quality = int(quality)
        self._create(lambda n, h, w: self.lib.caddy_video_workspace_bytes(n, h, w),
                     lambda n, h, w, ws, nbytes: self.lib.caddy_video_ctx_create(n, h, w, self.quality, ws, nbytes))
        self._out = None
        self.last_offsets, self.last_copied = [0], 0

    def stream_bound(self, n: int) -> int:
        """the output capacity no input of n frames can exceed"""
        return int(self.lib.caddy_video_stream_bound(int(n), self.H, self.W))

    def tables(self) -> Tuple[np.ndarray, bytes]:
        """((2, 64) uint8 quantisation tables in natural order, luminance first; the constant header SOI .. SOS) as the context built them"""
        q, n = np.zeros((2, 64), np.uint8), C.c_int(0)
        self._check(self.lib.caddy_video_tables_get(self.ctx, None, None, C.byref(n)))
        hdr = np.zeros(n.value, np.uint8)
        self._check(self.lib.caddy_video_tables_get(self.ctx, q.ctypes.data_as(C.c_void_p), hdr.ctypes.data_as(C.c_void_p), C.byref(n)))
        return q, hdr.tobytes()

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
        step = max(1, min(n, AVI_LIMIT // self.stream_bound(1)))      # (the offsets of one call are 32-bit words)
        files, offsets, copied = [], [0], 0
        for n0 in range(0, n, step):
            part = u8[n0:n0 + step]
            k = int(part.shape[0])
            bound = self.stream_bound(k)
            if self._out is None or self._out.numel() < bound:
                self._out = torch.empty(bound, dtype=torch.uint8, device=self.device)
            off = torch.empty(k + 1, dtype=torch.int32, device=self.device)
            self._stream()
            self._check(self.lib.caddy_video_encode(self.ctx, part.data_ptr(), k, self._out.data_ptr(), bound, off.data_ptr()))
            o = [int(v) & 0xFFFFFFFF for v in off.cpu().tolist()]
            stream = self._out[:o[k]].cpu().numpy().tobytes()      # only the encoded bytes are copied
            copied += 4 * (k + 1) + o[k]
            files += [stream[o[i]:o[i + 1]] for i in range(k)]
            offsets += [offsets[n0] + v for v in o[1:]]
        self.last_offsets, self.last_copied = offsets, copied
        return files


def cached_encoder(H: int, W: int, n_frames: int, quality: int = DEFAULT_QUALITY, lib=None, device=None) -> JpegEncoder:
    """the encoder of this library, device, geometry and quality; it holds at most 64 frames per chunk (a longer call runs in chunks), so it is never re-created for a
    longer video"""
    lib = lib if lib is not None else M._default_lib
    dev = str(device) if device is not None else str(M.device(lib))
    key = ("video_writer", id(lib), dev, int(H), int(W), int(quality))
    room = min(64, 1 << (max(int(n_frames), 1) - 1).bit_length())
    return M._cached(key, None, lambda: JpegEncoder(H, W, room, quality, lib, device), lambda e: e.max_frames < room)


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _rate(fps) -> Fraction:
    r = Fraction(fps).limit_denominator(1001)
    if r <= 0:
        raise ValueError(f"fps must be positive, got {fps}")
    return r


def write_avi(path: str, jpegs: Sequence[bytes], width: int, height: int, fps=DEFAULT_FPS) -> int:
    """Motion-JPEG in an AVI container: RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh (vids, MJPG, scale / rate = 1 / fps), strf (BITMAPINFOHEADER, 24 bit, MJPG) } },
    LIST movi { one '00dc' chunk per frame, padded to even length }, idx1 }.  -> the bytes written.  No OpenDML: a file that would pass 2 GiB raises."""
    if not jpegs:
        raise ValueError("no frames")
    rate = _rate(fps)
    n, largest = len(jpegs), max(len(j) for j in jpegs)
    movi_size = 4 + sum(8 + len(j) + (len(j) & 1) for j in jpegs)
    total = 12 + (12 + (8 + 56) + (12 + (8 + 56) + (8 + 40))) + (8 + movi_size) + (8 + 16 * n)
    if total > AVI_LIMIT:
        raise ValueError(f"the AVI file would be {total} bytes: above 2 GiB (no OpenDML index is written); split the video")
    usec = int(round(1e6 * rate.denominator / rate.numerator))
    avih = struct.pack("<14I", usec, int(largest * rate) + 1, 0, 0x10, n, 0, 1, largest, width, height, 0, 0, 0, 0)                                  # 0x10: AVIF_HASINDEX
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, rate.denominator, rate.numerator, 0, n, largest, 0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = b"LIST" + struct.pack("<I", 4 + (8 + 56) + (12 + (8 + 56) + (8 + 40))) + b"hdrl" + _chunk(b"avih", avih) + \
        b"LIST" + struct.pack("<I", 4 + (8 + 56) + (8 + 40)) + b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
    index, at = [], 4      # offsets count from the 'movi' fourcc
    for j in jpegs:
        index.append(struct.pack("<4sIII", b"00dc", 0x10, at, len(j)))                                                                              # 0x10: AVIIF_KEYFRAME
        at += 8 + len(j) + (len(j) & 1)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_size) + b"movi")
        for j in jpegs:
            f.write(_chunk(b"00dc", j))
        f.write(_chunk(b"idx1", b"".join(index)))
    return total


def read_avi(path: str) -> Tuple[Dict, List[bytes]]:
    """-> ({"width", "height", "fps", "frames" (dwTotalFrames), "microsec_per_frame", "scale", "rate", "handler", "compression", "bit_count", "riff_size", "file_size",
    "movi_offset" (of the 'movi' fourcc), "movi_size", "chunk_offsets" (of every '00dc' header), "index": [(ckid, flags, offset, size)]}, the frames' bytes)"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path} is not a RIFF AVI file")
    head: Dict = {"riff_size": struct.unpack_from("<I", data, 4)[0], "file_size": len(data), "chunk_offsets": [], "index": []}
    frames: List[bytes] = []

    def walk(lo, hi):
        at = lo
        while at + 8 <= hi:
            fourcc, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
            body = at + 8
            if body + size > hi:
                raise ValueError(f"{path}: chunk {fourcc!r} at {at} runs past its list")
            if fourcc == b"LIST":
                kind = data[body:body + 4]
                if kind == b"movi":
                    head["movi_offset"], head["movi_size"] = body, size
                walk(body + 4, body + size)
            elif fourcc == b"avih":
                v = struct.unpack_from("<14I", data, body)
                head.update(microsec_per_frame=v[0], flags=v[3], frames=v[4], streams=v[6], width=v[8], height=v[9])
            elif fourcc == b"strh":
                head["type"], head["handler"] = data[body:body + 4], data[body + 4:body + 8]
                v = struct.unpack_from("<IHHIIIIIIII", data, body + 8)
                head.update(scale=v[4], rate=v[5], length=v[7])
                head["fps"] = v[5] / v[4]
            elif fourcc == b"strf":
                v = struct.unpack_from("<IiiHH4sI", data, body)
                head.update(bit_count=v[4], compression=v[5], bitmap_width=v[1], bitmap_height=v[2])
            elif fourcc == b"00dc":
                head["chunk_offsets"].append(at)
                frames.append(data[body:body + size])
            elif fourcc == b"idx1":
                head["index"] = [struct.unpack_from("<4sIII", data, body + 16 * i) for i in range(size // 16)]
            at = body + size + (size & 1)
    walk(12, len(data))
    return head, frames


def _library_of(model_or_lib):
    if model_or_lib is None or isinstance(model_or_lib, C.CDLL):
        return model_or_lib
    return getattr(getattr(model_or_lib, "module", model_or_lib), "_lib", None)


def save_video(model_or_lib, frames: torch.Tensor, path: str, fps=DEFAULT_FPS, quality: int = DEFAULT_QUALITY, map: int = MAP_ALWAYS) -> int:
    """utils/save_video_ffmpeg.py:172-198 as Motion-JPEG: frames (n, H, W, 3) uint8 or (n, 3, H, W) fp32 (quantised under `map`), encoded on the device of `frames` by the
    library of `model_or_lib` (a model, a loaded library, or None for the default one) -> the bytes written to `path`"""
    if frames.dim() != 4:
        raise ValueError(f"expected (n, H, W, 3) uint8 or (n, 3, H, W) fp32 frames, got {tuple(frames.shape)}")
    H, W = (int(frames.shape[1]), int(frames.shape[2])) if frames.dtype == torch.uint8 else (int(frames.shape[2]), int(frames.shape[3]))
    lib = _library_of(model_or_lib)
    device = frames.device if frames.device.type == M.device(lib).type else None      # (host frames are staged on the library's device)
    enc = cached_encoder(H, W, int(frames.shape[0]), quality, lib, device)
    return write_avi(path, enc(frames, map=map), W, H, fps)


MAX_SAVED_VIDEOS = 30      # default of evaluation_dataset.max_saved_videos


class ComparisonVideos:
    """`evaluation_dataset.save_videos`: <directory>/<sequence index>.avi for the first `evaluation_dataset.max_saved_videos` (default 30) sequences of an evaluation, the
    reference frames on the left and the generated ones on the right, at the reference's 5 frames per second and quality 90.  `add(reference_u8, generated_u8)` takes the (bs, T, H, W, 3) uint8 tensors of one batch where they
    are -- they are joined and encoded on the device, all sequences of the batch in one call."""

    def __init__(self, config, directory: str, lib=None):
        ed = config.get("evaluation_dataset", {})
        self.enabled = bool(ed.get("save_videos", False))
        self.limit = int(ed.get("max_saved_videos", MAX_SAVED_VIDEOS))
        self.directory, self.lib, self.saved = directory, lib, 0

    def wanted(self) -> bool:
        return self.enabled and self.saved < self.limit

    def add(self, reference_u8: torch.Tensor, generated_u8: torch.Tensor):
        if not self.wanted():
            return
        if reference_u8.shape != generated_u8.shape or reference_u8.dim() != 5:
            raise ValueError(f"expected two (bs, T, H, W, 3) uint8 tensors, got {tuple(reference_u8.shape)} and {tuple(generated_u8.shape)}")
        k = min(int(reference_u8.shape[0]), self.limit - self.saved)
        pair = torch.cat([reference_u8[:k], generated_u8[:k].to(reference_u8.device)], dim=3)      # (k, T, H, 2 W, 3)
        _, T, H, W2, _ = (int(v) for v in pair.shape)
        files = cached_encoder(H, W2, k * T, DEFAULT_QUALITY, self.lib, pair.device)(pair.reshape(k * T, H, W2, 3))
        os.makedirs(self.directory, exist_ok=True)
        for b in range(k):
            write_avi(os.path.join(self.directory, f"{self.saved}.avi"), files[b * T:(b + 1) * T], W2, H, DEFAULT_FPS)
            self.saved += 1
