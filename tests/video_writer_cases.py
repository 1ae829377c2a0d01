"""Shared by the video-writer tests (csrc/video.hip: caddy_video_encode; video_writer.JpegEncoder): the fixtures and the expected files.  The expected file is an integer
restatement in numpy / plain Python of libjpeg's baseline path (jccolor.c, jfdctint.c, jcdctmgr.c, jchuff.c) as include/caddy_hip.h states it, plus a builder of the constant
header -- never the kernel; every comparison is byte for byte.  The CPU tests hold the restatement against Pillow's whole file, so on a machine whose Pillow carries another
libjpeg the GPU tests still have their oracle.  The check functions take the torch device the library's pointers live on ("cpu" for the host simulator, "cuda" for
libcaddy_hip.so)."""
import functools
import io

import numpy as np
import torch

from playablevideogeneration_amd import video_writer as VW

# Annex K.1 / K.2 of the JPEG standard, in natural (row-major) order
BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# Annex K.3: (class << 4 | id, the 16 code counts, the symbols in code order)
HUFFMAN = [
    (0x00, [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0x10, [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
     [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1,
      0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39,
      0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
      0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
      0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
      0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
    (0x01, [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (0x11, [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
     [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09,
      0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38,
      0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
      0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
      0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
      0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
]


def quant_tables(quality: int):
    """the two tables in natural order: libjpeg's jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [[min(max((b * scale + 50) // 100, 1), 255) for b in base] for base in (BASE_LUMA, BASE_CHROMA)]


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(H: int, W: int, quality: int) -> bytes:
    """SOI .. SOS as libjpeg writes them for a 4:4:4 baseline file: APP0 JFIF 1.01 (no density), two DQT, SOF0, four DHT, SOS"""
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, table in enumerate(quant_tables(quality)):
        out += _segment(0xDB, bytes([i]) + bytes(table[z] for z in ZIGZAG))
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, counts, symbols in HUFFMAN:
        out += _segment(0xC4, bytes([tc_th]) + bytes(counts) + bytes(symbols))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


@functools.lru_cache(None)
def _codes():
    """[dc luma, ac luma, dc chroma, ac chroma] -> {symbol: (code, length)} (jchuff.c: jpeg_make_c_derived_tbl)"""
    tables = []
    for _, counts, symbols in HUFFMAN:
        table, code, k = {}, 0, 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                table[symbols[k]] = (code, length)
                code += 1
                k += 1
            code <<= 1
        tables.append(table)
    return tables


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first: bool):
    """one pass of jfdctint.c over the last axis of d (int64)"""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = np.empty_like(d)
    out[..., 0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[..., 4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = _descale(z1 + t13 * 6270, n)
    out[..., 6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def quantised_blocks(frame: np.ndarray, quality: int) -> np.ndarray:
    """(H, W, 3) uint8 -> (MCU rows, MCU columns, 3, 64) quantised coefficients in zigzag order"""
    H, W, _ = frame.shape
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    rgb = np.pad(frame, ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    fix = lambda x: int(x * 65536 + 0.5)
    ycc = np.stack([(fix(.299) * r + fix(.587) * g + fix(.114) * b + 32768) >> 16,
                    (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + (128 << 16) + 32767) >> 16,
                    (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + (128 << 16) + 32767) >> 16]) - 128
    blocks = ycc.reshape(3, Hp // 8, 8, Wp // 8, 8).transpose(1, 3, 0, 2, 4)                 # (my, mx, c, row, column)
    coef = _fdct_pass(_fdct_pass(blocks, True).swapaxes(-1, -2), False).swapaxes(-1, -2)      # rows, then columns
    tables = np.array(quant_tables(quality), dtype=np.int64)[[0, 1, 1]].reshape(1, 1, 3, 64) << 3
    flat = coef.reshape(Hp // 8, Wp // 8, 3, 64)
    q = np.sign(flat) * ((np.abs(flat) + (tables >> 1)) // tables)
    return q[..., ZIGZAG]


EVENT_NAMES = ("zero_run_escape", "dc_category_11", "ac_category_10", "negative_dc_difference", "zero_dc_difference", "block_ends_at_63", "eob_only_block", "stuffed_byte",
               "ends_on_a_byte_boundary", "ends_padded", "scan_longer_than_the_frame")


def entropy_scan(q: np.ndarray, events=None) -> bytes:
    """jchuff.c over the interleaved MCUs of one frame -> the stuffed scan bytes (no markers)"""
    dc_l, ac_l, dc_c, ac_c = _codes()
    ev = events if events is not None else {}
    acc, nacc, out = 0, 0, bytearray()

    def put(code, length):
        nonlocal acc, nacc
        acc = (acc << length) | code
        nacc += length
        while nacc >= 8:
            nacc -= 8
            out.append((acc >> nacc) & 0xFF)
        acc &= (1 << nacc) - 1
    pred = [0, 0, 0]
    for block in q.reshape(-1, 3, 64).tolist():
        for c in range(3):
            dc_t, ac_t = (dc_l, ac_l) if c == 0 else (dc_c, ac_c)
            z = block[c]
            diff, pred[c] = z[0] - pred[c], z[0]
            n = abs(diff).bit_length()
            put(*dc_t[n])
            put((diff - 1 if diff < 0 else diff) & ((1 << n) - 1), n)
            ev["dc_category_11"] = ev.get("dc_category_11", 0) + (n == 11)
            ev["negative_dc_difference"] = ev.get("negative_dc_difference", 0) + (diff < 0)
            ev["zero_dc_difference"] = ev.get("zero_dc_difference", 0) + (diff == 0)
            run = 0
            for v in z[1:]:
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    put(*ac_t[0xF0])
                    run -= 16
                    ev["zero_run_escape"] = ev.get("zero_run_escape", 0) + 1
                n = abs(v).bit_length()
                put(*ac_t[(run << 4) + n])
                put((v - 1 if v < 0 else v) & ((1 << n) - 1), n)
                ev["ac_category_10"] = ev.get("ac_category_10", 0) + (n == 10)
                run = 0
            if run:
                put(*ac_t[0x00])
                ev["eob_only_block"] = ev.get("eob_only_block", 0) + (run == 63)
            else:
                ev["block_ends_at_63"] = ev.get("block_ends_at_63", 0) + 1
    ev["ends_on_a_byte_boundary" if nacc == 0 else "ends_padded"] = ev.get("ends_on_a_byte_boundary" if nacc == 0 else "ends_padded", 0) + 1
    if nacc:
        put((1 << (8 - nacc)) - 1, 8 - nacc)
    ev["stuffed_byte"] = ev.get("stuffed_byte", 0) + out.count(0xFF)
    return bytes(out).replace(b"\xff", b"\xff\x00")


def oracle(frame: np.ndarray, quality: int, events=None) -> bytes:
    """the whole file of one (H, W, 3) uint8 frame"""
    H, W, _ = frame.shape
    scan = entropy_scan(quantised_blocks(frame, quality), events)
    if events is not None:
        events["scan_longer_than_the_frame"] = events.get("scan_longer_than_the_frame", 0) + (len(scan) > 3 * H * W)
    return header(H, W, quality) + scan + b"\xff\xd9"


def pillow(frame: np.ndarray, quality: int) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=0, optimize=False)
    return buf.getvalue()


def pillow_is_turbo() -> bool:
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


def _noise(H, W):
    return np.random.default_rng(1234).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _flat(H, W):
    return np.broadcast_to(np.array([200, 30, 90], np.uint8), (H, W, 3)).copy()


def _blocks(H, W):
    y, x = np.mgrid[:H, :W]
    return np.repeat((((y // 8 + x // 8) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)


def _pixel_checker(H, W):
    y, x = np.mgrid[:H, :W]
    return np.repeat((((x + y) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)


def _wide(H, W):
    y, x = np.mgrid[:H, :W]
    ramps = np.stack([x * 255 // (W - 1), y * 255 // (H - 1), (x + y) * 255 // (W + H - 2)], axis=2)
    return np.clip(ramps + np.random.default_rng(1234).integers(-9, 10, (H, W, 3)), 0, 255).astype(np.uint8)


# name -> (maker, H, W, quality)
FIXTURES = {"one_mcu": (_noise, 8, 8, 100), "ragged": (_noise, 20, 28, 75), "overhang": (_noise, 33, 17, 90), "flat": (_flat, 16, 24, 75), "blocks": (_blocks, 32, 32, 100),
            "pixel_checker": (_pixel_checker, 16, 16, 100), "noise_q100": (_noise, 64, 64, 100), "wide": (_wide, 72, 136, 90), "low_q": (_noise, 24, 40, 1)}
FIXTURE_IDS = list(FIXTURES)


@functools.lru_cache(None)
def fixture(name):
    """-> (frame (H, W, 3) uint8, quality, the oracle's file, the events its scan contains); computed once, never changed"""
    make, H, W, q = FIXTURES[name]
    frame = make(H, W)
    frame.setflags(write=False)
    events = {}
    return frame, q, oracle(frame, q, events), events


def assert_the_fixtures_cover_every_branch():
    total = {k: sum(fixture(n)[3].get(k, 0) for n in FIXTURES) for k in EVENT_NAMES}
    missing = [k for k, v in total.items() if v < 1]
    assert not missing, (missing, total)
    return total


def encode(device, frames, quality, max_frames=None, **kw):
    """frames (n, H, W, 3) uint8 numpy -> list[bytes] through a fresh context"""
    n, H, W, _ = frames.shape
    enc = VW.JpegEncoder(H, W, max_frames if max_frames is not None else n, quality, device=device)
    return enc(torch.from_numpy(np.array(frames)).to(device), **kw), enc      # (np.array: a writable copy, the fixtures stay as they are)


def check_fixture(device, name):
    frame, q, want, _ = fixture(name)
    got, enc = encode(device, frame[None], q)
    assert len(got) == 1 and got[0] == want, (name, len(got[0]), len(want))
    if device == "cpu" and pillow_is_turbo():      # the device result against the installed encoder itself
        assert got[0] == pillow(frame, q), name


def check_tables(device, quality):
    """the context's quantisation tables (natural order) and header against the restatement (the CPU tests hold the restatement against Pillow)"""
    enc = VW.JpegEncoder(24, 40, 1, quality, device=device)
    tables, hdr = enc.tables()
    assert tables.tolist() == quant_tables(quality) and hdr == header(24, 40, quality)
    return tables, hdr


def _several():
    """five 64 x 64 frames at q = 100: the four 32 x 32 tiles of noise_q100 tiled back to 64 x 64, a flat frame, and `blocks` at that size"""
    noise = fixture("noise_q100")[0]
    tiles = [np.tile(noise[y:y + 32, x:x + 32], (2, 2, 1)) for y in (0, 32) for x in (0, 32)]
    return np.stack(tiles[:3] + [_flat(64, 64), _blocks(64, 64)]), 100


@functools.lru_cache(None)
def _several_expected():
    frames, q = _several()
    return [oracle(f, q) for f in frames]


def check_several_frames(device):
    """each file of a multi-frame call equals its single-frame encoding: the DC prediction restarts per frame, and the offsets are exact"""
    frames, q = _several()
    want = _several_expected()
    got, enc = encode(device, frames, q)
    assert got == want
    assert enc.last_offsets == np.cumsum([0] + [len(w) for w in want]).tolist()


def check_chunking(device):
    """n > max_frames: chunks of 2, 2 and 1 frames"""
    frames, q = _several()
    got, enc = encode(device, frames, q, max_frames=2)
    assert got == _several_expected()


def check_context_reuse(device):
    """a second call is bit-identical; a smaller, flatter batch after a larger, noisier one is exact (no stale bits in the OR-ed buffer)"""
    frames, q = _several()
    want = _several_expected()
    dev = torch.from_numpy(frames).to(device)
    enc = VW.JpegEncoder(64, 64, 5, q, device=device)
    assert enc(dev) == want and enc(dev) == want
    quiet = np.stack([_flat(64, 64), _blocks(64, 64)])
    assert enc(torch.from_numpy(quiet).to(device)) == [want[3], want[4]]
    assert enc(dev) == want


def check_capacity(device):
    """a capacity below the bound is refused (-2) and nothing is written; with exactly the bound nothing is written past the total"""
    import ctypes as C
    frames, q = _several()
    want = b"".join(_several_expected())
    n = len(frames)
    enc = VW.JpegEncoder(64, 64, n, q, device=device)
    bound = enc.stream_bound(n)
    hdr = len(header(64, 64, q))
    blocks = 3 * 64
    assert bound == n * (hdr + 2 * ((blocks * (63 * 26 + 22) + 7) // 8) + 2)      # AC 16 + 10 bits, DC 11 + 11 bits, every byte stuffed, header and EOI
    dev = torch.from_numpy(frames).to(device)
    out = torch.full((bound + 64,), 0x5A, dtype=torch.uint8, device=device)
    offsets = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int64, device=device).to(torch.int32)
    enc._stream()
    rc = enc.lib.caddy_video_encode(enc.ctx, dev.data_ptr(), n, out.data_ptr(), C.c_size_t(bound - 1), offsets.data_ptr())
    assert rc == -2 and "caddy_video_stream_bound" in enc.lib.caddy_last_error().decode()
    assert bool((out == 0x5A).all())
    rc = enc.lib.caddy_video_encode(enc.ctx, dev.data_ptr(), n, out.data_ptr(), C.c_size_t(bound), offsets.data_ptr())
    assert rc == 0
    host = out.cpu().numpy()
    assert int(offsets[n]) == len(want) and host[:len(want)].tobytes() == want and (host[len(want):] == 0x5A).all()


def check_fp32_input(device):
    """(n, 3, H, W) fp32 goes through the frame writer with the given map first: the bytes of frame_to_uint8, then the oracle"""
    from playablevideogeneration_amd import drivers as D
    from playablevideogeneration_amd.frame_pipeline import MAP_ALWAYS
    x = torch.rand(2, 3, 20, 28, generator=torch.Generator().manual_seed(5)) * 1.9 - 0.95
    enc = VW.JpegEncoder(20, 28, 2, 75, device=device)
    got = enc(x.to(device), map=MAP_ALWAYS)
    assert got == [oracle(D.frame_to_uint8(f), 75) for f in x]


def check_largest_scan(device):
    """256 x 256 noise at q = 100: 1024 MCUs, the longest scan a frame of the benchmark's size can have"""
    frame = _noise(256, 256)
    got, _ = encode(device, frame[None], 100)
    assert got[0] == oracle(frame, 100)
