"""Shared by the PNG-writer tests (csrc/png.hip: caddy_png_encode; png_writer.PngEncoder): the fixtures, a numpy restatement of the filter rule as include/caddy_hip.h states
it, a PNG chunk parser and a small deflate walker -- a minimal inflate that also reports, per block, its type, the longest code of every tree, the match lengths seen and whether
the distance tree carried codes no token used.  The files are not compared with Pillow's bytes: the contract is that independent decoders (Pillow's PNG reader, zlib.decompress)
return exactly the input, that the filtered stream is the restated one, and that the files are not meaningfully larger than Pillow's."""
import ctypes as C
import functools
import io
import struct
import zlib

import numpy as np
import torch
from PIL import Image

from playablevideogeneration_amd import png_writer as PW

BLOCK = PW.BLOCK
STORED = 5          # a stored block's bytes besides its data: one byte of header and padding, LEN, NLEN
FRAME = 63          # signature 8 + IHDR 25 + IDAT length, type, CRC 12 + zlib header 2 + Adler-32 4 + IEND 12


# ---- the filter rule -----------------------------------------------------------------------------------------------------------------------------------------------
def _candidates(cur, up):
    """the five filtered rows (uint8) of raw row `cur` (3 W bytes) under raw row `up`; bpp = 3"""
    x = cur.astype(np.int32)
    b = up.astype(np.int32)
    a = np.concatenate([np.zeros(3, np.int32), x[:-3]])
    c = np.concatenate([np.zeros(3, np.int32), b[:-3]])
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return [((x - pred) & 255).astype(np.uint8) for pred in (0 * x, a, b, (a + b) >> 1, paeth)]


def filter_sums(cur, up):
    return [int(np.abs(r.view(np.int8).astype(np.int32)).sum()) for r in _candidates(cur, up)]


def filtered_stream(image, mode=PW.FILTER_ADAPTIVE):
    """image (H, W, 3) uint8 -> (the filtered stream, the type chosen for every row): per row the type with the smallest sum of |int8|, ties to the lower type"""
    H, W, _ = image.shape
    rows = image.reshape(H, 3 * W)
    out, types = [], []
    for y in range(H):
        up = rows[y - 1] if y > 0 else np.zeros(3 * W, np.uint8)
        cand = _candidates(rows[y], up)
        if mode == PW.FILTER_ADAPTIVE:
            sums = [int(np.abs(r.view(np.int8).astype(np.int32)).sum()) for r in cand]
            t = int(np.argmin(sums))      # (the first of equal minima)
        else:
            t = mode
        types.append(t)
        out.append(bytes([t]) + cand[t].tobytes())
    return b"".join(out), types


# ---- the container -------------------------------------------------------------------------------------------------------------------------------------------------
def parse_png(data):
    """-> [(type, payload)]; the signature, every chunk length and every CRC are checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack_from(">I4s", data, at)
        payload = data[at + 8:at + 8 + n]
        assert len(payload) == n, (kind, n)
        crc, = struct.unpack_from(">I", data, at + 8 + n)
        assert crc == zlib.crc32(kind + payload), kind
        chunks.append((kind, payload))
        at += 12 + n
    assert at == len(data)
    return chunks


# ---- the deflate walker --------------------------------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data, at=0):
        self.d, self.pos = data, 8 * at

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7


def _decoder(lengths):
    """canonical Huffman decoder of RFC 1951 3.2.2: {(length, code): symbol}; an over-subscribed set of lengths is refused"""
    count = [0] * 16
    for v in lengths:
        count[v] += 1
    count[0] = 0
    assert sum(c << (15 - i) for i, c in enumerate(count) if i) <= 1 << 15, "over-subscribed code"
    code, nxt = 0, [0] * 16
    for i in range(1, 16):
        code = (code + count[i - 1]) << 1
        nxt[i] = code
    table = {}
    for s, v in enumerate(lengths):
        if v:
            table[v, nxt[v]] = s
            nxt[v] += 1
    return table


def _symbol(bits, table):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (n, code) in table:
            return table[n, code]
    raise AssertionError("no such code")


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def walk_deflate(data):
    """a raw deflate stream -> (the bytes, [per block: {"type" 0 / 1 / 2, "bytes" produced, "at" / "end" bit positions, "literals", "matches" [lengths], "distances" {set},
    and for a dynamic block "max_ll" / "max_d" / "max_cl" longest code lengths, "ll_freq" / "cl_freq" how often every symbol was used, "ll_codes" / "d_codes" / "cl_codes" numbers of codes of non-zero length, "d_used" distance
    symbols a token used}])"""
    bits, out, blocks = _Bits(data), bytearray(), []
    while True:
        info = {"at": bits.pos, "literals": 0, "matches": [], "distances": set()}
        final, kind = bits.take(1), bits.take(2)
        info["type"] = kind
        start = len(out)
        assert kind in (0, 1, 2)
        if kind == 0:
            bits.align()
            n, inv = bits.take(16), bits.take(16)
            assert n ^ inv == 0xFFFF
            out += data[bits.pos >> 3:(bits.pos >> 3) + n]
            assert len(out) - start == n
            bits.pos += 8 * n
        else:
            if kind == 1:
                ll, dd = _decoder(_FIXED_LL), _decoder([5] * 30)
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_ORDER[i]] = bits.take(3)
                cld = _decoder(cl)
                lens, cl_freq = [], [0] * 19
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, cld)
                    cl_freq[s] += 1
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.take(3))
                    else:
                        lens += [0] * (11 + bits.take(7))
                assert len(lens) == hlit + hdist
                ll_l, d_l = lens[:hlit], lens[hlit:]
                assert ll_l[256] > 0
                info.update(max_ll=max(ll_l), max_d=max(d_l), max_cl=max(cl), ll_codes=sum(v > 0 for v in ll_l), d_codes=sum(v > 0 for v in d_l),
                            cl_codes=sum(v > 0 for v in cl), d_used=set(), cl_freq=cl_freq, ll_freq=[0] * 286)
                ll, dd = _decoder(ll_l), _decoder(d_l)
            while True:
                s = _symbol(bits, ll)
                if kind == 2:
                    info["ll_freq"][s] += 1
                if s < 256:
                    out.append(s)
                    info["literals"] += 1
                elif s == 256:
                    break
                else:
                    assert s <= 285
                    n = _LEN_BASE[s - 257] + bits.take(_LEN_EXTRA[s - 257])
                    ds = _symbol(bits, dd)
                    dist = _DIST_BASE[ds] + bits.take(_DIST_EXTRA[ds])
                    assert dist <= len(out)
                    for _ in range(n):
                        out.append(out[-dist])
                    info["matches"].append(n)
                    info["distances"].add(dist)
                    if kind == 2:
                        info["d_used"].add(ds)
        info["bytes"], info["end"] = len(out) - start, bits.pos
        blocks.append(info)
        if final:
            break
    bits.align()
    assert bits.pos == 8 * len(data), "bytes behind the final block"
    return bytes(out), blocks


def expected_tokens(block):
    """the (literals, [match lengths]) the stated parse gives for one block of stream bytes: a run of R equal bytes is a literal, then matches of min(258, left) while at least 3
    are left, then literals"""
    lits, matches, i, n = 0, [], 0, len(block)
    while i < n:
        j = i
        while j + 1 < n and block[j + 1] == block[i]:
            j += 1
        left = j - i
        lits += 1
        while left >= 3:
            m = min(258, left)
            matches.append(m)
            left -= m
        lits += left
        i = j + 1
    return lits, matches


def check_file(data, image, mode=PW.FILTER_ADAPTIVE):
    """everything the exactness contract asks of one file -> the walker's blocks.  Empty stored blocks (the byte-boundary markers) are dropped from the list after the check
    that each directly follows a compressed block."""
    H, W, _ = image.shape
    with Image.open(io.BytesIO(data)) as im:
        im.verify()
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == "RGB" and im.size == (W, H) and np.array_equal(np.asarray(im), image)
    chunks = parse_png(data)
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0) and chunks[2][1] == b""
    idat = chunks[1][1]
    want, _ = filtered_stream(image, mode)
    assert zlib.decompress(idat) == want
    assert (idat[0] * 256 + idat[1]) % 31 == 0 and idat[0] == 0x78
    assert struct.unpack(">I", idat[-4:])[0] == zlib.adler32(want)
    got, blocks = walk_deflate(idat[2:-4])
    assert got == want
    real, at = [], 0
    for i, b in enumerate(blocks):
        if b["type"] == 0 and b["bytes"] == 0:
            assert i > 0 and blocks[i - 1]["type"] != 0 and blocks[i - 1]["end"] % 8 != 0 and b["end"] % 8 == 0      # only where it is needed
            continue
        assert b["at"] % 8 == 0, "every block starts on a byte boundary"
        assert b["bytes"] == min(BLOCK, len(want) - at)
        lits, matches = expected_tokens(want[at:at + b["bytes"]])
        if b["type"] != 0:
            assert (b["literals"], b["matches"]) == (lits, matches) and b["distances"] <= {1}
        if b["type"] == 2:
            assert b["max_ll"] <= 15 and b["max_d"] <= 15 and b["max_cl"] <= 7 and b["ll_codes"] >= 2 and b["d_codes"] >= 2 and b["cl_codes"] >= 2
        b["single_run"] = lits == 1
        at += b["bytes"]
        real.append(b)
    assert at == len(want) and len(real) == -(-len(want) // BLOCK)
    return real


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def _noise(H, W, seed=1):
    return _rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _smooth(H, W, sigma=0.0, seed=2):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([96 + 80 * np.sin(x / 17.0) * np.cos(y / 23.0), 120 + 70 * np.cos((x + y) / 29.0), 90 + 0.9 * x + 0.4 * y], axis=-1)
    if sigma:
        base = base + _rng(seed).normal(0, sigma, base.shape)
    return np.clip(np.rint(base), 0, 255).astype(np.uint8)


def _breakout(H, W):
    """a Breakout-like flat frame: black, a grey border, six rows of coloured bricks, a paddle and a ball"""
    f = np.zeros((H, W, 3), np.uint8)
    f[: H // 10] = 142
    f[:, : W // 20] = 142
    f[:, -(W // 20):] = 142
    colours = [(200, 72, 72), (198, 108, 58), (180, 122, 48), (162, 162, 42), (72, 160, 72), (66, 72, 200)]
    for i, c in enumerate(colours):
        f[H // 4 + 4 * i: H // 4 + 4 * i + 4, W // 20: W - W // 20] = c
    f[H // 4 + 8: H // 4 + 12, W // 2: W // 2 + 24] = 0      # bricks knocked out
    f[H - 12: H - 9, W // 3: W // 3 + 16] = (200, 72, 72)
    f[H // 2: H // 2 + 3, W // 2 + 5: W // 2 + 7] = (200, 72, 72)
    return f


def _stream_image(stream, width_bytes, pad_values=None):
    """an image whose fixed-filter-0 stream holds `stream` in the rows' data bytes (rows of width_bytes = 3 W bytes; the last row is filled with a byte pattern without runs,
    or with `pad_values` in turn)"""
    assert width_bytes % 3 == 0
    data = bytearray(stream)
    pad = (-len(data)) % width_bytes
    data += bytes(((37 + 11 * i) % 251 + 1) if pad_values is None else pad_values[i % len(pad_values)] for i in range(pad))
    return np.frombuffer(bytes(data), np.uint8).reshape(-1, width_bytes // 3, 3).copy()


def _runs():
    """runs of length exactly 2, 3, 4, 258, 259, 260, 261 and 517 of distinct values, separated by bytes without runs.  Rows of 1 + 3000 bytes: the row's type byte 0 would
    cut or lengthen a run of zeros, so the runs use values 1.. and every run lies inside a row."""
    width = 3000
    rows, cur = [], bytearray()
    for k, n in enumerate((2, 3, 4, 258, 259, 260, 261, 517)):
        piece = bytes([200 + k]) * n + bytes([10 + k, 60 + k, 110 + k])
        if len(cur) + len(piece) > width:
            cur += bytes((91 + 7 * i) % 199 + 1 for i in range(width - len(cur)))
            rows.append(bytes(cur))
            cur = bytearray()
        cur += piece
    return _stream_image(b"".join(rows) + bytes(cur), width)


RUN_LENGTHS = (2, 3, 4, 258, 259, 260, 261, 517)


def _arranged(counts):
    """{value: count} -> the values in an order in which no byte repeats its predecessor (most frequent first on the even places, then the odd ones; the largest count is
    at most half), so that no match disturbs the frequencies"""
    values = [v for v, n in sorted(counts.items(), key=lambda kv: -kv[1]) for _ in range(n)]
    assert 2 * max(counts.values()) <= len(values) + 1
    out = [0] * len(values)
    half = (len(values) + 1) // 2
    out[0::2], out[1::2] = values[:half], values[half:]
    assert all(x != y for x, y in zip(out, out[1:]))
    return bytes(out)


def unlimited_depth(freqs):
    """the longest code of an unrestricted Huffman code for the non-zero frequencies"""
    import heapq
    heap = [(f, i, 0) for i, f in enumerate(f for f in freqs if f)]      # (weight, tie-breaker, depth of the subtree)
    heapq.heapify(heap)
    n = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        n += 1
        heapq.heappush(heap, (a[0] + b[0], n, max(a[2], b[2]) + 1))
    return heap[0][2]


def _fibonacci():
    """literal frequencies 1 (the row's type byte), 1 (end of block), 2, 3, 5, .. 2584: a Huffman code without a limit is 17 bits deep, so the limit of 15 is met.  One row
    of 6762 bytes in which no byte repeats its predecessor: one block without a match."""
    fib = [2, 3]
    while fib[-1] < 2584:
        fib.append(fib[-1] + fib[-2])
    return _stream_image(_arranged({k + 1: f for k, f in enumerate(fib)}), sum(fib))


def _wide_lengths():
    """literal frequencies 2^(12 - k) for n_k symbols of code length k, the n_k found by a search such that the Kraft sum is exactly 1 (the Huffman code then has these very
    lengths) and that the code-length alphabet -- which sees length k about n_k times, next to the two distance lengths and the zero runs -- has a profile whose unrestricted
    Huffman code is 8 deep: its own code needs the limit of 7.  Two of the 12-bit symbols are the row's type byte and the end of block.  The symbol values are ordered so that
    equal lengths do not touch (no repeat code takes the place of a length).  One row, no match."""
    counts = {2: 3, 4: 1, 5: 1, 7: 3, 8: 2, 9: 31, 10: 56, 11: 10, 12: 18}
    lengths = sorted((k for k, n in counts.items() for _ in range(n)), key=lambda k: -counts[k])
    order = [0] * len(lengths)      # the most common length on the even places, the rest on the odd ones
    order[0::2], order[1::2] = lengths[:(len(lengths) + 1) // 2], lengths[(len(lengths) + 1) // 2:]
    data = _arranged({sym + 1: 1 << (12 - k) for sym, k in enumerate(order)})
    top = order.index(2) + 1
    return _stream_image(data, len(data) + (-len(data)) % 3, (top,))


def _no_match():
    """3000 bytes of seven values, each distinct from its predecessor: compressible, and without a match"""
    return _stream_image(bytes((i * 3) % 7 + 1 for i in range(3000)), 3000)


def _single_run(H=75, W=75):
    return np.zeros((H, W, 3), np.uint8)


def _filters():
    """nine rows: noise; a row on which None wins; Sub; noise; Up; Average; Paeth; noise; a copy of the row above, where Up and Paeth tie exactly at 0 (the lower type is
    taken).  check_filter_choices holds the strict wins and the tie against the restated sums."""
    r, W = _rng(21), 24
    n = 3 * W
    rows = np.zeros((9, n), np.int64)
    rows[0] = r.integers(0, 256, n)
    rows[1] = r.integers(-3, 4, n) & 255                                        # None: small signed bytes under a noisy row
    rows[2] = (np.cumsum(r.integers(20, 40, (W, 3)), axis=0).reshape(-1) + 7) & 255      # Sub: a ramp per channel
    rows[3] = r.integers(0, 256, n)
    rows[4] = (rows[3] + r.integers(-1, 2, n)) & 255                            # Up: the row above and a little; every fifth pixel jumps, which misleads Paeth at the next
    rows[4].reshape(W, 3)[::5] = r.integers(0, 256, (len(range(0, W, 5)), 3))
    for i in range(n):                                                          # Average: the mean of left and up, plus 1
        rows[5, i] = ((((rows[5, i - 3] if i >= 3 else 0) + rows[4, i]) >> 1) + 1) & 255
    for i in range(n):                                                          # Paeth: the predictor and a little; every fifth pixel jumps, so the row is no copy of the one above
        a, b, c = (rows[6, i - 3] if i >= 3 else 0), rows[5, i], (rows[5, i - 3] if i >= 3 else 0)
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        rows[6, i] = r.integers(0, 256) if (i // 3) % 5 == 0 else ((a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)) + r.integers(-1, 2)) & 255
    rows[7] = r.integers(0, 256, n)
    rows[8] = rows[7]
    return rows.astype(np.uint8).reshape(9, W, 3)


FILTER_WINS = {1: 0, 2: 1, 4: 2, 5: 3, 6: 4}      # row -> the type that wins it strictly


def _paeth_tie():
    """a constant image: left, upper and upper-left neighbour are equal, so p - a = p - b = p - c -- the three predictors tie and `a` is taken"""
    return np.full((6, 9, 3), 77, np.uint8)


FIXTURES = {
    "one": (lambda: _noise(1, 1, 3), PW.FILTER_ADAPTIVE),
    "row": (lambda: _noise(1, 7, 4), PW.FILTER_ADAPTIVE),
    "column": (lambda: _noise(7, 1, 5), PW.FILTER_ADAPTIVE),
    "odd_stride": (lambda: _smooth(33, 17, 3.0), PW.FILTER_ADAPTIVE),
    "noise": (lambda: _noise(64, 64), PW.FILTER_ADAPTIVE),
    "breakout": (lambda: _breakout(160, 160), PW.FILTER_ADAPTIVE),
    "zeros": (lambda: _single_run(), PW.FILTER_ADAPTIVE),
    "smooth": (lambda: _smooth(96, 96), PW.FILTER_ADAPTIVE),
    "smooth_noise": (lambda: _smooth(96, 96, 2.0), PW.FILTER_ADAPTIVE),
    "runs": (_runs, PW.FILTER_NONE),
    "fibonacci": (_fibonacci, PW.FILTER_NONE),
    "wide_lengths": (_wide_lengths, PW.FILTER_NONE),
    "no_match": (_no_match, PW.FILTER_NONE),
    "filters": (_filters, PW.FILTER_ADAPTIVE),
    "paeth_tie": (_paeth_tie, PW.FILTER_PAETH),
    "sub_fixed": (lambda: _smooth(20, 28, 2.0, 9), PW.FILTER_SUB),
    "up_fixed": (lambda: _smooth(20, 28, 2.0, 9), PW.FILTER_UP),
    "average_fixed": (lambda: _smooth(20, 28, 2.0, 9), PW.FILTER_AVERAGE),
}
FIXTURE_IDS = list(FIXTURES)
SIZE_FIXTURES = ("breakout", "smooth", "smooth_noise")
# file size over Pillow's default save(format="PNG"), measured on the simulator (the sizes are deterministic; profiles/png_writer.md); the tests allow this + 0.02
# (smooth, without noise, passes 1.10: Pillow's zlib finds repeated residual patterns at longer distances there, which distance-1 runs cannot -- a finding, not a bound to widen)
MEASURED_BYTES = {"breakout": 653, "smooth": 8219, "smooth_noise": 12998}      # the writer's files
MEASURED_RATIO = {"breakout": 653 / 636, "smooth": 8219 / 6033, "smooth_noise": 12998 / 13061}


@functools.lru_cache(None)
def fixture(name):
    """-> (image (H, W, 3) uint8, filter mode); computed once, never changed"""
    make, mode = FIXTURES[name]
    image = make()
    image.setflags(write=False)
    return image, mode


def pillow_size(image):
    f = io.BytesIO()
    Image.fromarray(image).save(f, format="PNG")
    return len(f.getvalue())


def encode(device, images, mode=PW.FILTER_ADAPTIVE, max_frames=None, **kw):
    """images (n, H, W, 3) uint8 numpy -> (list[bytes], the encoder) through a fresh context"""
    n, H, W, _ = images.shape
    enc = PW.PngEncoder(H, W, max_frames if max_frames is not None else n, mode, device=device)
    return enc(torch.from_numpy(np.array(images)).to(device), **kw), enc


_files = {}


def encoded(device, name):
    """the fixture's file and its walked blocks on `device`, encoded and checked once"""
    if (device, name) not in _files:
        image, mode = fixture(name)
        got, _ = encode(device, image[None], mode)
        assert len(got) == 1
        _files[device, name] = (got[0], check_file(got[0], image, mode))
    return _files[device, name]


def check_fixture(device, name):
    data, blocks = encoded(device, name)
    image, mode = fixture(name)
    assert len(data) <= FRAME + len(filtered_stream(image, mode)[0]) + STORED * len(blocks)
    return data, blocks


def check_special_streams(device):
    """what the fixed-filter streams were built to contain"""
    _, blocks = encoded(device, "runs")
    image, _ = fixture("runs")
    stream, _ = filtered_stream(image, PW.FILTER_NONE)
    matches = [m for b in blocks for m in b["matches"]]
    assert all(b["type"] != 0 for b in blocks)
    # 2 and 3 give no match; 4 -> 3; 258 -> 257; 259 -> 258; 260 -> 258 and a literal; 261 -> 258 and two literals; 517 -> 258, 258
    assert sorted(matches) == sorted([3, 257, 258, 258, 258, 258, 258]), matches
    for k, n in enumerate(RUN_LENGTHS):
        v = bytes([200 + k])
        assert stream.count(v * n) == 1 and stream.count(v * (n + 1)) == 0
    _, blocks = encoded(device, "fibonacci")
    assert [b["type"] for b in blocks] == [2] and blocks[0]["max_ll"] == 15 and not blocks[0]["matches"] and unlimited_depth(blocks[0]["ll_freq"]) > 15
    _, blocks = encoded(device, "wide_lengths")
    assert [b["type"] for b in blocks] == [2] and blocks[0]["max_cl"] == 7 and unlimited_depth(blocks[0]["cl_freq"]) > 7
    _, blocks = encoded(device, "no_match")
    assert len(blocks) == 1 and blocks[0]["type"] != 0 and not blocks[0]["matches"]
    _, blocks = encoded(device, "zeros")
    assert len(blocks) == 2 and all(b["single_run"] and b["literals"] == 1 and b["type"] != 0 for b in blocks)      # one run crosses the block boundary and restarts
    _, blocks = encoded(device, "noise")
    assert all(b["type"] == 0 for b in blocks)
    _, blocks = encoded(device, "smooth_noise")
    assert len(blocks) >= 2 and all(b["type"] == 2 for b in blocks)


def check_filter_choices():
    """the fixture rows on which each filter wins strictly, the exact tie and the Paeth tie, from the restated rule itself"""
    image, _ = fixture("filters")
    _, types = filtered_stream(image)
    rows = image.reshape(image.shape[0], -1)
    for y, t in FILTER_WINS.items():
        sums = filter_sums(rows[y], rows[y - 1])
        assert types[y] == t and sums.count(min(sums)) == 1, (y, sums)
    sums = filter_sums(rows[8], rows[7])
    assert sums[2] == sums[4] == min(sums) == 0 and types[8] == 2      # an exact tie: the lower type
    image, _ = fixture("paeth_tie")
    rows = image.reshape(image.shape[0], -1)
    assert int(rows[3, 0]) == int(rows[2, 3]) == int(rows[2, 0])


def assert_the_fixtures_cover_every_branch(device):
    """from the walker's counts over the whole set: stored, fixed and dynamic blocks; the limits 15 and 7 reached; a dynamic block without a match, whose distance tree still
    carries two codes (zlib's forced pair), and one with a match, where the second code is the forced one; a block that is a single run; a marker block and a block that needed
    none"""
    total = {"stored": 0, "fixed": 0, "dynamic": 0, "max_ll_15": 0, "max_cl_7": 0, "distance_tree_unused": 0, "distance_tree_one_used": 0, "single_run": 0, "several_blocks": 0}
    for name in FIXTURES:
        _, blocks = encoded(device, name)
        total["several_blocks"] += len(blocks) > 1
        for b in blocks:
            total[("stored", "fixed", "dynamic")[b["type"]]] += 1
            total["single_run"] += b["single_run"]
            if b["type"] == 2:
                total["max_ll_15"] += b["max_ll"] == 15
                total["max_cl_7"] += b["max_cl"] == 7
                total["distance_tree_unused"] += not b["d_used"] and b["d_codes"] == 2
                total["distance_tree_one_used"] += len(b["d_used"]) == 1 and b["d_codes"] == 2
    missing = [k for k, v in total.items() if v < 1]
    assert not missing, (missing, total)
    return total


def _several():
    """five 40 x 56 images of different kinds"""
    return np.stack([_noise(40, 56, 31), _smooth(40, 56), _breakout(40, 56), _smooth(40, 56, 4.0, 5), np.zeros((40, 56, 3), np.uint8)])


@functools.lru_cache(None)
def _several_expected(device):
    files = [encode(device, f[None])[0][0] for f in _several()]
    for data, f in zip(files, _several()):
        check_file(data, f)
    return files


def check_several_frames(device):
    """each file of a multi-image call equals its single-image encoding, and the offsets are exact"""
    want = _several_expected(device)
    got, enc = encode(device, _several())
    assert got == want
    assert enc.last_offsets == np.cumsum([0] + [len(w) for w in want]).tolist()
    assert enc.last_copied == 4 * 6 + sum(len(w) for w in want)


def check_chunking(device):
    """n > max_frames: chunks of 2, 2 and 1 images"""
    got, _ = encode(device, _several(), max_frames=2)
    assert got == _several_expected(device)


def check_context_reuse(device):
    """a second call is bit-identical; a smaller, flatter batch after a larger, noisier one is exact"""
    frames, want = _several(), _several_expected(device)
    dev = torch.from_numpy(frames).to(device)
    enc = PW.PngEncoder(40, 56, 5, device=device)
    assert enc(dev) == want and enc(dev) == want
    assert enc(torch.from_numpy(frames[[4, 2]]).to(device)) == [want[4], want[2]]
    assert enc(dev) == want


def check_capacity(device):
    """a capacity below the bound is refused (-2) and nothing is written; with exactly the bound nothing is written past the total"""
    frames = _several()
    want = b"".join(_several_expected(device))
    n = len(frames)
    enc = PW.PngEncoder(40, 56, n, device=device)
    bound = enc.stream_bound(n)
    S = 40 * (1 + 3 * 56)
    assert bound == n * (FRAME + S + STORED * -(-S // BLOCK))
    dev = torch.from_numpy(frames).to(device)
    out = torch.full((bound + 64,), 0x5A, dtype=torch.uint8, device=device)
    offsets = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int64, device=device).to(torch.int32)
    enc._stream()
    rc = enc.lib.caddy_png_encode(enc.ctx, dev.data_ptr(), n, out.data_ptr(), C.c_size_t(bound - 1), offsets.data_ptr())
    assert rc == -2 and "caddy_png_stream_bound" in enc.lib.caddy_last_error().decode()
    assert bool((out == 0x5A).all()) and bool((offsets == 0x5A5A5A5A).all())
    rc = enc.lib.caddy_png_encode(enc.ctx, dev.data_ptr(), n, out.data_ptr(), C.c_size_t(bound), offsets.data_ptr())
    assert rc == 0
    host = out.cpu().numpy()
    assert int(offsets[n]) == len(want) and host[:len(want)].tobytes() == want and (host[len(want):] == 0x5A).all()


def check_fp32_input(device):
    """(n, 3, H, W) fp32 goes through the frame writer with the given map first: the bytes of frame_to_uint8, then the file"""
    from playablevideogeneration_amd import drivers as D
    from playablevideogeneration_amd.frame_pipeline import MAP_ALWAYS
    x = torch.rand(2, 3, 20, 28, generator=torch.Generator().manual_seed(5)) * 1.9 - 0.95
    enc = PW.PngEncoder(20, 28, 2, device=device)
    got = enc(x.to(device), map=MAP_ALWAYS)
    for data, f in zip(got, x):
        check_file(data, D.frame_to_uint8(f))


def check_unaligned_bases(device):
    """9 x 9 images are 243 bytes: the second and third image start at odd addresses; and a view one byte into a buffer"""
    frames = _rng(41).integers(0, 256, (3, 9, 9, 3), dtype=np.uint8)
    got, enc = encode(device, frames)
    for data, f in zip(got, frames):
        check_file(data, f)
    flat = torch.zeros(3 * 243 + 1, dtype=torch.uint8, device=device)
    flat[1:] = torch.from_numpy(frames.reshape(-1)).to(device)
    view = flat[1:].view(3, 9, 9, 3)
    assert view.data_ptr() % 2 == 1 or view.data_ptr() % 4 != 0
    assert enc(view) == got


def check_noise_meets_the_bound(device):
    """the noise fixture is stored: its file is within the bound and the bound is not slack by more than the per-block overhead -- here it is met exactly: every block goes out
    stored, 5 bytes each"""
    data, blocks = encoded(device, "noise")
    image, _ = fixture("noise")
    enc = PW.PngEncoder(64, 64, 1, device=device)
    bound = enc.stream_bound(1)
    assert len(data) <= bound and bound - len(data) <= STORED * len(blocks)
    assert len(data) == bound


def check_many_blocks(device):
    """3510 x 400, the upper half zeros and the lower half noise: 258 blocks, more than one pass of the per-image scan (256 blocks a pass) and of the write launch (32
    workgroups an image); dynamic blocks of single runs, then stored ones"""
    H, W = 3510, 400
    image = np.zeros((H, W, 3), np.uint8)
    image[H // 2:] = _noise(H - H // 2, W, 77)
    got, enc = encode(device, image[None])
    blocks = check_file(got[0], image)
    assert len(blocks) == 258 and {b["type"] for b in blocks} == {0, 2} and len(got[0]) <= enc.stream_bound(1)


def check_sizes(device):
    """the files against Pillow's default save of the same array: at most Pillow's size x (the measured ratio + 0.02)"""
    figures = {}
    for name in SIZE_FIXTURES:
        data, _ = encoded(device, name)
        ours, theirs = len(data), pillow_size(np.array(fixture(name)[0]))
        figures[name] = (ours, theirs, ours / theirs)
        print(f"png size {name}: {ours} bytes, Pillow {theirs}, ratio {ours / theirs:.4f}")
    for name, (ours, theirs, _) in figures.items():
        assert ours <= theirs * (MEASURED_RATIO[name] + 0.02), (name, ours, theirs)
    return figures
