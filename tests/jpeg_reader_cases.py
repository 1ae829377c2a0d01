"""Shared by the JPEG-reader tests (csrc/jpeg_read.hip: caddy_jpeg_decode; jpeg_reader.JpegDecoder): the cases, on "cpu" (the host simulator) and on "cuda".  The arbiter is
`ref_decode`, a plain-Python / numpy restatement of the rules and the integer arithmetic include/caddy_hip.h states (markers, Huffman decoding per restart interval,
dequantisation, jidctint.c, fancy upsampling at the chroma plane's true size, jdcolor.c) -- never the kernel.  The CPU tests hold it to Pillow byte for byte on every
encoder-written file of the cases, so on a machine whose Pillow carries another libjpeg the GPU tests still have their oracle.  Besides Pillow's files the cases need legal (and
illegal) streams no encoder emits, so this file holds a small token-level JPEG writer: explicit segments, explicit Huffman tables, blocks from explicit quantised values or raw
bits.  Every decode goes through guarded buffers: the bytes around frames_u8 and status must come back untouched.
(One Pillow file is 72 x 64, above the 64 x 64 of everything else: with 4:4:4 blocks, 65 restart intervals -- what makes the lane batch wrap -- need more than 64 MCUs.)"""
import functools
import io

import numpy as np
import torch
from PIL import Image

from playablevideogeneration_amd import jpeg_reader as JR
from playablevideogeneration_amd import png_reader as PR
from tests import video_writer_cases as VC

GUARD = 64                      # bytes around frames_u8, words around status
FILL, FILL_WORD = 0x5A, 0x5A5A5A5A
ZZ = VC.ZIGZAG
M32 = 0xFFFFFFFF


# ---- the reference decoder -----------------------------------------------------------------------------------------------------------------------------------------
class Refused(Exception):
    def __init__(self, status):
        super().__init__(JR.STATUS_NAMES[status])
        self.status = status


def _be16(d, p):
    return (d[p] << 8) | d[p + 1]


def _huffman(counts, symbols):
    """{(length, code): symbol}"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return out


def ref_parse(d, H, W):
    """the markers up to SOS -> dict(mode (hs, vs), q [3 tables in zigzag order], dc / ac [3 code dicts], ri, scan)"""
    if d[:2] != b"\xff\xd8"[:len(d[:2])]:
        raise Refused(JR.NOT_JPEG)
    if len(d) < 2:
        raise Refused(JR.TRUNCATED)
    pos, qt, ht, sof, jfif, adobe, ri = 2, {}, {}, None, False, None, 0
    while True:
        if pos >= len(d):
            raise Refused(JR.TRUNCATED)
        if d[pos] != 0xFF:
            raise Refused(JR.BAD_TABLE)
        while pos < len(d) and d[pos] == 0xFF:
            pos += 1
        if pos >= len(d):
            raise Refused(JR.TRUNCATED)
        m = d[pos]
        pos += 1
        if m == 0xD9:
            raise Refused(JR.TRUNCATED)
        if m in (0x00, 0x01) or 0xD0 <= m <= 0xD8:
            raise Refused(JR.BAD_TABLE)
        if len(d) - pos < 2:
            raise Refused(JR.TRUNCATED)
        length = _be16(d, pos)
        if length < 2:
            raise Refused(JR.BAD_TABLE)
        if length > len(d) - pos:
            raise Refused(JR.TRUNCATED)
        seg = d[pos + 2:pos + length]
        pos += length
        n = len(seg)
        if m == 0xC0:
            if sof is not None or n < 6 or n != 6 + 3 * seg[5]:
                raise Refused(JR.BAD_TABLE)
            if seg[0] != 8 or seg[5] != 3 or _be16(seg, 1) == 0:
                raise Refused(JR.UNSUPPORTED)
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c], seg[8 + 3 * c]) for c in range(3)]
            if any(c[2] > 3 for c in comps):
                raise Refused(JR.BAD_TABLE)
            if comps[1][1] != 0x11 or comps[2][1] != 0x11 or comps[0][1] not in (0x11, 0x21, 0x22):
                raise Refused(JR.UNSUPPORTED)
            if _be16(seg, 1) != H or _be16(seg, 3) != W:
                raise Refused(JR.GEOMETRY)
            sof = comps
        elif (0xC1 <= m <= 0xCF and m != 0xC4) or m in (0xDC, 0xDE, 0xDF):
            raise Refused(JR.UNSUPPORTED)
        elif m == 0xDB:
            o = 0
            while o < n:
                pq, tid = seg[o] >> 4, seg[o] & 15
                if pq == 1:
                    raise Refused(JR.UNSUPPORTED)
                if pq > 1 or tid > 3 or n - o < 65:
                    raise Refused(JR.BAD_TABLE)
                qt[tid] = list(seg[o + 1:o + 65])
                o += 65
        elif m == 0xC4:
            o = 0
            while o < n:
                tc, tid = seg[o] >> 4, seg[o] & 15
                if tc > 1 or tid > 3 or n - o < 17:
                    raise Refused(JR.BAD_TABLE)
                counts, left = list(seg[o + 1:o + 17]), 1
                for c in counts:
                    left = 2 * left - c
                    if left < 0:
                        raise Refused(JR.BAD_TABLE)
                total = sum(counts)
                if total > 256 or n - o - 17 < total:
                    raise Refused(JR.BAD_TABLE)
                ht[(tc, tid)] = _huffman(counts, list(seg[o + 17:o + 17 + total]))
                o += 17 + total
        elif m == 0xDD:
            if n != 2:
                raise Refused(JR.BAD_TABLE)
            ri = _be16(seg, 0)
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\0"
        elif m == 0xEE:
            if n >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            if sof is None or n < 1 or n != 4 + 2 * seg[0]:
                raise Refused(JR.BAD_TABLE)
            if seg[0] != 3:
                raise Refused(JR.UNSUPPORTED)
            tabs = []
            for c in range(3):
                if seg[1 + 2 * c] != sof[c][0]:
                    raise Refused(JR.UNSUPPORTED)
                tabs.append((seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15))
                if tabs[-1][0] > 3 or tabs[-1][1] > 3:
                    raise Refused(JR.BAD_TABLE)
            if (seg[7], seg[8], seg[9]) != (0, 63, 0):
                raise Refused(JR.UNSUPPORTED)
            if not jfif and ((adobe != 1) if adobe is not None else bytes(c[0] for c in sof) == b"RGB"):
                raise Refused(JR.UNSUPPORTED)
            for c in range(3):
                if sof[c][2] not in qt or (0, tabs[c][0]) not in ht or (1, tabs[c][1]) not in ht:
                    raise Refused(JR.BAD_TABLE)
            return dict(mode=(sof[0][1] >> 4, sof[0][1] & 15), q=[qt[sof[c][2]] for c in range(3)], dc=[ht[(0, tabs[c][0])] for c in range(3)],
                        ac=[ht[(1, tabs[c][1])] for c in range(3)], ri=ri, scan=pos)


class _Bits:
    """MSB first over an interval's bytes, 0xFF (0xFF)* 0x00 read as one 0xFF; zeros past the end"""

    def __init__(self, raw):
        out, i = bytearray(), 0
        while i < len(raw):
            b = raw[i]
            i += 1
            if b == 0xFF:
                q = i
                while q < len(raw) and raw[q] == 0xFF:
                    q += 1
                if q < len(raw) and raw[q] == 0:
                    i = q + 1
                else:
                    break
            out.append(b)
        self.total, self.at = 8 * len(out), 0
        self.value = int.from_bytes(bytes(out) + bytes(4), "big")
        self.width = self.total + 32

    def peek(self, n):
        return (self.value >> (self.width - self.at - n)) & ((1 << n) - 1)

    def symbol(self, table):
        """-> the symbol; Refused(BAD_CODE) where no code matches 16 real bits; None where bits past the end were used"""
        for length in range(1, 17):
            s = table.get((length, self.peek(length)))
            if s is not None:
                self.at += length
                return None if self.at > self.total else s
        if self.total - self.at < 16:
            return None
        raise Refused(JR.BAD_CODE)

    def take(self, n):
        v = self.peek(n) if n else 0
        self.at += n
        return None if self.at > self.total else v


class _Over(Exception):
    pass


def _need(v):
    if v is None:
        raise _Over()
    return v


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _ref_block(b, dc, ac, pred):
    """-> (64 quantised values in natural order, the new predictor)"""
    out = [0] * 64
    s = _need(b.symbol(dc))
    if s > 11:
        raise Refused(JR.BAD_COEFFICIENT)
    pred += _extend(_need(b.take(s)), s)
    if not -2048 <= pred <= 2047:
        raise Refused(JR.BAD_COEFFICIENT)
    out[0] = pred
    k = 1
    while k < 64:
        rs = _need(b.symbol(ac))
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            if k + 15 > 63:
                raise Refused(JR.BAD_COEFFICIENT)
            k += 16
            continue
        if s > 10:
            raise Refused(JR.BAD_COEFFICIENT)
        k += r
        if k > 63:
            raise Refused(JR.BAD_COEFFICIENT)
        out[ZZ[k]] = _extend(_need(b.take(s)), s)
        k += 1
    return out, pred


def _idct_pass(v, shift):
    """jidctint.c over the last axis of uint32 (.., 8); wraps on 32 bits"""
    u = np.uint32
    i0, i1, i2, i3, i4, i5, i6, i7 = [v[..., k] for k in range(8)]
    z1 = (i2 + i6) * u(4433)
    t2, t3 = z1 - i6 * u(15137), z1 + i2 * u(6270)
    t0, t1 = (i0 + i4) << u(13), (i0 - i4) << u(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * u(9633)
    t0, t1, t2, t3 = t0 * u(2446), t1 * u(16819), t2 * u(25172), t3 * u(12299)
    z1, z2, z3, z4 = z1 * u(M32 + 1 - 7373), z2 * u(M32 + 1 - 20995), z3 * u(M32 + 1 - 16069) + z5, z4 * u(M32 + 1 - 3196) + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    rnd = u(1 << (shift - 1))
    outs = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([((o + rnd).view(np.int32) >> shift).view(np.uint32) for o in outs], axis=-1)


def ref_idct(blocks, q_natural):
    """(n, 64) quantised values in natural order, the table in natural order -> (n, 8, 8) uint8 samples"""
    with np.errstate(over="ignore"):
        c = (np.asarray(blocks, np.int64).astype(np.uint32) * np.asarray(q_natural, np.uint32)[None]).reshape(-1, 8, 8)
        ws = _idct_pass(np.ascontiguousarray(c.transpose(0, 2, 1)), 11).transpose(0, 2, 1)      # columns first
        out = _idct_pass(np.ascontiguousarray(ws), 18).view(np.int32)
    return np.clip(out.astype(np.int64) + 128, 0, 255).astype(np.uint8)


def _upsample(plane, hs, vs, H, W):
    """a chroma plane of the true size -> (H, W) int, fancy upsampling with the neighbours replicated at the plane's own edge"""
    s = plane.astype(np.int64)
    ch, cw = s.shape
    if hs == 1:
        return s[:H, :W]
    if vs == 2:
        y = np.arange(H)
        r = y >> 1
        r2 = np.where(y & 1, np.minimum(r + 1, ch - 1), np.maximum(r - 1, 0))
        v, even, odd, sh = 3 * s[r] + s[r2], 8, 7, 4
    else:
        v, even, odd, sh = s, 1, 2, 2
    left, right = np.concatenate([v[:, :1], v[:, :-1]], 1), np.concatenate([v[:, 1:], v[:, -1:]], 1)
    out = np.empty((v.shape[0], 2 * cw), np.int64)
    out[:, 0::2] = (3 * v + left + even) >> sh
    out[:, 1::2] = (3 * v + right + odd) >> sh
    return out[:H, :W]


def _ref_decode(d, H, W):
    P = ref_parse(d, H, W)
    hs, vs = P["mode"]
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    mcus, ri = mcux * mcuy, P["ri"]
    ni = -(-mcus // ri) if ri else 1
    markers = [(q, d[q]) for q in range(P["scan"] + 1, len(d)) if d[q] not in (0, 0xFF) and d[q - 1] == 0xFF]
    term = next((k for k, (_, v) in enumerate(markers) if not 0xD0 <= v <= 0xD7), None)
    if term is None:
        raise Refused(JR.TRUNCATED)
    if term != ni - 1 or any(markers[k][1] != 0xD0 + (k & 7) for k in range(term)):
        raise Refused(JR.BAD_RESTART)
    if markers[term][1] != 0xD9:
        raise Refused(JR.UNSUPPORTED if markers[term][1] == 0xDC else JR.BAD_SCAN)
    dims = [(mcux * hs, mcuy * vs), (mcux, mcuy), (mcux, mcuy)]
    coef = [np.zeros((bh, bw, 64), np.int64) for bw, bh in dims]
    for i in range(ni):
        last = i == ni - 1
        start = P["scan"] if i == 0 else markers[i - 1][0] + 1
        end = markers[i][0] - 1
        while end > start and d[end - 1] == 0xFF:
            end -= 1
        b = _Bits(d[start:end])
        pred = [0, 0, 0]
        try:
            for m in range(i * ri, min(i * ri + ri, mcus) if ri else mcus):
                my, mx = divmod(m, mcux)
                for c in range(3):
                    for v in range(vs if c == 0 else 1):
                        for h in range(hs if c == 0 else 1):
                            blk, pred[c] = _ref_block(b, P["dc"][c], P["ac"][c], pred[c])
                            coef[c][my * (vs if c == 0 else 1) + v, mx * (hs if c == 0 else 1) + h] = blk
        except _Over:
            raise Refused(JR.TRUNCATED if last else JR.BAD_RESTART)
        if b.total - b.at >= 8:
            raise Refused(JR.BAD_SCAN if last else JR.BAD_RESTART)
    planes = []
    for c in range(3):
        bw, bh = dims[c]
        q_nat = [0] * 64
        for k in range(64):
            q_nat[ZZ[k]] = P["q"][c][k]
        px = ref_idct(coef[c].reshape(-1, 64), q_nat).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)
        planes.append(px)
    Y = planes[0][:H, :W].astype(np.int64)
    cw, ch = -(-W // hs), -(-H // vs)
    cb, cr = [_upsample(p[:ch, :cw], hs, vs, H, W) - 128 for p in planes[1:]]
    rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)], axis=2)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def ref_decode(data, H, W):
    """-> (status, the (H, W, 3) uint8 frame or None)"""
    try:
        return JR.OK, _ref_decode(bytes(data), H, W)
    except Refused as e:
        return e.status, None


# ---- Pillow's files --------------------------------------------------------------------------------------------------------------------------------------------------
def pillow_file(image, **kw):
    f = io.BytesIO()
    Image.fromarray(np.asarray(image)).save(f, format="JPEG", **kw)
    return f.getvalue()


def pillow_pixels(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB")).copy()


@functools.lru_cache(None)
def image(H, W, kind="noise", seed=7):
    if kind == "noise":
        out = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == "smooth":
        y, x = np.mgrid[:H, :W]
        out = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(W + H - 2, 1)], axis=2)
        out = np.clip(out + np.random.default_rng(seed).integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
    else:
        out = np.broadcast_to(np.array([200, 30, 90], np.uint8), (H, W, 3)).copy()
    out.setflags(write=False)
    return out


SIZES = ((1, 1), (7, 9), (8, 8), (16, 16), (13, 21), (17, 33), (40, 24), (64, 64))      # (H, W)
KINDS = ("noise", "smooth", "constant")
QUALITIES = (1, 30, 90, 100)


def _mcu_row(W, subsampling):
    return -(-W // (8 if subsampling == 0 else 16))


@functools.lru_cache(None)
def pillow_cases():
    """[(name, H, W, file)]: every size x sampling x content; quality, optimize and the restart interval (none, 1, 3, one MCU row) go round so that each meets each size and
    each sampling; then the files with more than 8 and more than 64 intervals"""
    out, k = [], 0
    for H, W in SIZES:
        for sub in (0, 1, 2):
            for kind in KINDS:
                q, opt = QUALITIES[k % 4], bool((k // 4 + k // 9) % 2)
                rs = (0, 1, 3, _mcu_row(W, sub))[(k // 2 + k // 3) % 4]
                kw = dict(quality=q, subsampling=sub, optimize=opt)
                if rs:
                    kw["restart_marker_blocks"] = rs
                out.append((f"{H}x{W}_{kind}_s{sub}_q{q}_o{int(opt)}_r{rs}", H, W, pillow_file(image(H, W, kind), **kw)))
                k += 1
    out.append(("rst_index_wraps", 40, 24, pillow_file(image(40, 24), quality=90, subsampling=0, restart_marker_blocks=1)))            # 15 intervals
    out.append(("lane_batch_wraps", 72, 64, pillow_file(image(72, 64), quality=30, subsampling=0, restart_marker_blocks=1)))          # 72 intervals
    out.append(("one_mcu_row_420", 64, 64, pillow_file(image(64, 64, "smooth"), quality=90, subsampling=2, restart_marker_blocks=4)))
    return out


def count_rst(data):
    return sum(1 for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7)


def check_reference_equals_pillow():
    """the yardstick: the restated decoder against Pillow on every encoder-written file, byte for byte; and the files are what the cases say"""
    seen_q, seen_opt, seen_rs = set(), set(), set()
    for name, H, W, data in pillow_cases():
        st, frame = ref_decode(data, H, W)
        assert st == JR.OK, (name, JR.STATUS_NAMES[st])
        assert np.array_equal(frame, pillow_pixels(data)), name
        parts = name.split("_")
        if parts[-1].startswith("r") and parts[-1][1:].isdigit():
            seen_q.add(parts[-3]); seen_opt.add(parts[-2]); seen_rs.add(parts[-1])
            rs, ri = int(parts[-1][1:]), ref_parse(data, H, W)["ri"]
            assert ri == rs and (count_rst(data) > 0) == (rs > 0 and n_mcus(H, W, {"s0": 0x11, "s1": 0x21, "s2": 0x22}[parts[-4]])[0] > rs), name
    assert len(seen_q) == 4 and len(seen_opt) == 2 and len(seen_rs) >= 4
    by = {n: d for n, _, _, d in pillow_cases()}
    assert count_rst(by["rst_index_wraps"]) == 14 and count_rst(by["lane_batch_wraps"]) == 71


def VC_files():
    """the video writer's expected files (the oracle of tests/video_writer_cases.py): encoder-written, so held to Pillow too"""
    return {name: VC.fixture(name)[2] for name in VC.FIXTURE_IDS}


def check_reference_equals_pillow_on_the_writers_files():
    for name, data in VC_files().items():
        H, W = VC.fixture(name)[0].shape[:2]
        st, frame = ref_decode(data, H, W)
        assert st == JR.OK and np.array_equal(frame, pillow_pixels(data)), name


# ---- the token-level writer --------------------------------------------------------------------------------------------------------------------------------------------
def seg(marker, payload=b""):
    return (marker, bytes(payload))


def serialise(parts, fill=0):
    """[(marker, payload) | bytes] -> the file; a marker below 0 is SOI / EOI (no length); `fill`: 0xFF bytes in front of every marker"""
    out = b""
    for p in parts:
        if isinstance(p, (bytes, bytearray)):
            out += bytes(p)
            continue
        m, payload = p
        out += b"\xff" * ((0 if m == 0xD8 else fill) + 1) + bytes([m]) + (b"" if m in (0xD8, 0xD9) else (len(payload) + 2).to_bytes(2, "big") + payload)
    return out


def codes_of(counts, symbols):
    return {s: (code, length) for (length, code), s in _huffman(counts, symbols).items()}


STD = {(h[0] >> 4, h[0] & 15): (h[1], h[2]) for h in VC.HUFFMAN}      # (class, id) -> (counts, symbols); id 0 luminance, 1 chrominance
# a DC table with one code of every length 1..16: the categories 11 and 0 carry the longest codes
DC16 = ([1] * 16, [2, 3, 4, 5, 6, 1, 7, 8, 9, 10, 12, 13, 14, 15, 0, 11])


class Scan:
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]

    def bytes(self):
        b = self.bits + [1] * (-len(self.bits) % 8)
        raw = bytes(int("".join(map(str, b[i:i + 8])), 2) for i in range(0, len(b), 8))
        return raw.replace(b"\xff", b"\xff\x00")


def _category(v):
    return abs(v).bit_length()


def put_block(w, zz, pred, dc, ac):
    """one block of 64 quantised values in zigzag order (jchuff.c): -> the new predictor; ("raw", [(value, bits), ..]) writes bits as they are"""
    if isinstance(zz, tuple) and zz[0] == "raw":
        for v, n in zz[1]:
            w.put(v, n)
        return pred
    diff = zz[0] - pred
    s = _category(diff)
    w.put(*dc[s])
    w.put(diff if diff >= 0 else diff - 1 + (1 << s), s)
    run = 0
    for k in range(1, 64):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac[0xF0])
            run -= 16
        s = _category(zz[k])
        w.put(*ac[(run << 4) | s])
        w.put(zz[k] if zz[k] >= 0 else zz[k] - 1 + (1 << s), s)
        run = 0
    if run:
        w.put(*ac[0x00])
    return zz[0]


def intervals(mcus, ri, dc, ac):
    """mcus: per MCU its blocks in order (the luma blocks, Cb, Cr), each 64 zigzag values or ("raw", ..); dc / ac: per component {symbol: (code, length)} -> the stuffed
    bytes of every restart interval"""
    out = []
    step = ri if ri else len(mcus)
    for m0 in range(0, len(mcus), step):
        w, pred = Scan(), [0, 0, 0]
        for blocks in mcus[m0:m0 + step]:
            for j, zz in enumerate(blocks):
                c = 0 if j < len(blocks) - 2 else j - (len(blocks) - 2) + 1
                pred[c] = put_block(w, zz, pred[c], dc[c], ac[c])
        out.append(w.bytes())
    return out


def join(ivs, fill=0, first=0):
    """the intervals with RSTm between them"""
    out = b""
    for k, iv in enumerate(ivs):
        out += iv
        if k < len(ivs) - 1:
            out += b"\xff" * (fill + 1) + bytes([0xD0 + ((first + k) & 7)])
    return out


def dqt(tables, ids):
    return seg(0xDB, b"".join(bytes([i]) + bytes(t[z] for z in ZZ) for t, i in zip(tables, ids)))


def dht(entries):
    """entries: [(class, id, (counts, symbols))]"""
    return seg(0xC4, b"".join(bytes([(tc << 4) | i]) + bytes(t[0]) + bytes(t[1]) for tc, i, t in entries))


def sof(H, W, sampling=0x11, ids=(1, 2, 3), tq=(0, 1, 1), marker=0xC0, precision=8, chroma=0x11):
    return seg(marker, bytes([precision]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, ids[0], sampling, tq[0], ids[1], chroma, tq[1], ids[2], chroma, tq[2]]))


def sos(ids=(1, 2, 3), tabs=(0x00, 0x11, 0x11), tail=(0, 63, 0)):
    return seg(0xDA, bytes([len(ids)]) + b"".join(bytes([i, t]) for i, t in zip(ids, tabs)) + bytes(tail))


JFIF = seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))


def adobe(transform):
    return seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform]))


def dri(n):
    return seg(0xDD, n.to_bytes(2, "big"))


def std_dht():
    return [dht([(tc, i, STD[(tc, i)])]) for i in (0, 1) for tc in (0, 1)]


def std_codes():
    dc = [codes_of(*STD[(0, 0)]), codes_of(*STD[(0, 1)]), codes_of(*STD[(0, 1)])]
    ac = [codes_of(*STD[(1, 0)]), codes_of(*STD[(1, 1)]), codes_of(*STD[(1, 1)])]
    return dc, ac


def n_mcus(H, W, sampling):
    hs, vs = sampling >> 4, sampling & 15
    return -(-W // (8 * hs)) * -(-H // (8 * vs)), hs * vs + 2


def random_mcus(H, W, sampling, seed, amp=60, density=0.25, dc=300):
    """sparse random blocks whose DC differences stay small enough for the standard tables"""
    rng = np.random.default_rng(seed)
    n, per = n_mcus(H, W, sampling)
    out = []
    for _ in range(n):
        blocks = []
        for _ in range(per):
            zz = (rng.integers(-amp, amp + 1, 64) * (rng.random(64) < density)).astype(int).tolist()
            zz[0] = int(rng.integers(-dc, dc + 1))
            blocks.append(zz)
        out.append(blocks)
    return out


FLAT_Q = [[3] * 64, [5] * 64]


def plain_file(H, W, sampling, mcus, ri=0, q=FLAT_Q, head=(JFIF,), fill=0, scan_fill=0):
    """a file with the standard Huffman tables from explicit blocks"""
    dc, ac = std_codes()
    parts = [seg(0xD8)] + list(head) + [dqt(q, (0, 1)), sof(H, W, sampling)] + std_dht() + ([dri(ri)] if ri is not None else []) + [sos()]
    return serialise(parts, fill) + join(intervals(mcus, ri, dc, ac), scan_fill) + b"\xff" * scan_fill + b"\xff\xd9"


@functools.lru_cache(None)
def handwritten():
    """{name: (H, W, file)}; the expected frame is the reference decoder's"""
    out = {}
    dcs, acs = std_codes()
    # a 16-bit code (the DC category 11 of DC16), DC at +2047 and -2047 against a table of 255s (the products wrap in the IDCT), also the first byte of the scan stuffed
    H, W = 8, 16
    zero = [0] * 64
    mcus = [[[2047] + [0] * 63, [40] + zero[1:], [-40] + zero[1:]], [[-2047] + [0] * 63, zero, zero]]
    dc16 = codes_of(*DC16)
    parts = [seg(0xD8), JFIF, dqt([[255] * 64, [7] * 64], (0, 1)), sof(H, W), dht([(0, 0, DC16)]), dht([(1, 0, STD[(1, 0)])]), dht([(0, 1, STD[(0, 1)])]), dht([(1, 1, STD[(1, 1)])]), dri(1), sos()]
    scan = join(intervals(mcus, 1, [dc16, dcs[1], dcs[2]], acs), 0)      # (an interval each: both predictors start at 0)
    assert dc16[11][1] == 16 and scan[:2] == b"\xff\x00"
    out["code16_dc_2047_wrapping_products"] = (H, W, serialise(parts) + scan + b"\xff\xd9")
    # ZRL chains; a block that ends at index 63 without EOB; 4:2:0 with a partial MCU
    H, W = 17, 33
    mcus = random_mcus(H, W, 0x22, 3)
    mcus[0][0] = [5] + [0] * 39 + [-3] + [0] * 22 + [9]           # index 40 behind two ZRL, index 63 behind one more
    mcus[1][4] = [0] * 63 + [1]                                   # three ZRL and a run of 14 to index 63
    mcus[2][1] = [1] + [0] * 63                                   # EOB at once
    out["zrl_chains_and_index_63_420"] = (H, W, plain_file(H, W, 0x22, mcus))
    # luma on table id 1 and chroma on id 0, the quantisation tables likewise; no DRI at all; ids 'Y','U','V' without JFIF
    H, W = 13, 21
    mcus = random_mcus(H, W, 0x21, 4)
    ids = (ord("Y"), ord("U"), ord("V"))
    parts = [seg(0xD8), dqt(FLAT_Q, (1, 0)), sof(H, W, 0x21, ids=ids, tq=(1, 0, 0)),
             dht([(0, 1, STD[(0, 0)]), (1, 1, STD[(1, 0)]), (0, 0, STD[(0, 1)]), (1, 0, STD[(1, 1)])]), sos(ids, (0x11, 0x00, 0x00))]
    out["swapped_table_ids_merged_dht_422"] = (H, W, serialise(parts) + join(intervals(mcus, 0, dcs, acs)) + b"\xff\xd9")
    # tables split over several segments and redefined (first a wrong set, then the right one; table ids 2 and 3 in use); COM / APP1 between; fill bytes everywhere; DRI 0
    H, W = 16, 16
    mcus = random_mcus(H, W, 0x11, 5)
    parts = [seg(0xD8), JFIF, seg(0xFE, b"a comment"), dqt([[9] * 64], (2,)), dqt([[1] * 64], (3,)), seg(0xE1, b"Exif\0\0" + bytes(10)), dht([(0, 2, STD[(0, 1)]), (1, 2, STD[(1, 1)])]),
             sof(H, W, tq=(2, 3, 3)), dht([(0, 3, STD[(0, 0)])]), dht([(1, 3, STD[(1, 0)])]), dqt(FLAT_Q, (2, 3)), dht([(0, 2, STD[(0, 0)])]), seg(0xFE, b""),
             dht([(1, 2, STD[(1, 0)]), (0, 3, STD[(0, 1)])]), dht([(1, 3, STD[(1, 1)])]), dri(0), sos(tabs=(0x22, 0x33, 0x33))]
    out["tables_split_redefined_com_app1_fill_dri0"] = (H, W, serialise(parts, fill=2) + join(intervals(mcus, 0, dcs, acs)) + b"\xff\xff\xff\xd9")
    # an Adobe transform-1 file without JFIF; restart intervals of 2 MCUs with fill bytes in front of every RSTm; more than 8 intervals; bytes behind EOI
    H, W = 24, 40
    mcus = random_mcus(H, W, 0x11, 6)
    out["adobe_transform1_restarts_fill_trailing"] = (H, W, plain_file(H, W, 0x11, mcus, ri=1, head=(adobe(1),), scan_fill=1) + b"\xff\xd0 trailing \xff\xda bytes")
    # stuffed bytes at the first and the last byte of an interval: a DC category 11 opens every interval with 0xFF; the last value is searched so that the padding closes it
    H, W = 8, 24
    found = None
    for last, shift in ((a, b) for a in (1, 3, 7, 15, 31, 63, 127, 255, 511, 1023) for b in range(0, 64)):      # (the value's bits are 1s; `shift` moves where they end)
        mcus = [[[1500, shift] + [0] * 61 + [last], zero, [0] * 63 + [last]], [[1400] + [0] * 62 + [last], zero, [0, shift] + [0] * 61 + [last]], [[1300] + [3] + zero[2:], zero, zero]]
        ivs = intervals(mcus, 1, dcs, acs)
        if all(iv[:2] == b"\xff\x00" for iv in ivs) and ivs[0][-2:] == b"\xff\x00" and ivs[1][-2:] == b"\xff\x00":
            found = mcus
            break
    assert found is not None
    out["stuffing_at_both_ends_of_an_interval"] = (H, W, plain_file(H, W, 0x11, found, ri=1))
    return out


# ---- decoding through guarded buffers --------------------------------------------------------------------------------------------------------------------------------
_decoders = {}


def decoder(device, H, W, max_frames):
    key = (device, H, W, max_frames)
    if key not in _decoders:
        _decoders[key] = JR.JpegDecoder(H, W, max_frames, device=device)
    return _decoders[key]


def decode(device, files, H, W, max_frames=None, lead=0):
    """files -> (frames (n, H, W, 3) numpy, [status]); frames_u8 and status sit between guards, which must come back untouched.  `lead`: bytes in front of the first file in
    the blob (unaligned file starts)"""
    n = len(files)
    dec = decoder(device, H, W, max_frames if max_frames is not None else n)
    blob, offsets = PR.pack_files([bytes(lead)] + list(files))
    size = n * H * W * 3
    stream = torch.from_numpy(blob).to(device)
    off = torch.from_numpy(offsets[1:].astype(np.int32)).to(device)
    frames = torch.full((GUARD + size + GUARD,), FILL, dtype=torch.uint8, device=device)
    status = torch.full((GUARD + n + GUARD,), FILL_WORD, dtype=torch.int32, device=device)
    dec._stream()
    rc = dec.lib.caddy_jpeg_decode(dec.ctx, stream.data_ptr(), off.data_ptr(), n, frames.data_ptr() + GUARD, status.data_ptr() + 4 * GUARD)
    assert rc == 0, dec.lib.caddy_last_error().decode()
    f, s = frames.cpu().numpy(), status.cpu().numpy()
    assert (f[:GUARD] == FILL).all() and (f[GUARD + size:] == FILL).all(), "bytes around frames_u8 were written"
    assert (s[:GUARD] == FILL_WORD).all() and (s[GUARD + n:] == FILL_WORD).all(), "words around status were written"
    return f[GUARD:GUARD + size].reshape(n, H, W, 3), [int(v) for v in s[GUARD:GUARD + n]]


def names_of(status):
    return [JR.STATUS_NAMES[s] if 0 <= s < len(JR.STATUS_NAMES) else s for s in status]


def check_decodes(device, files, images, **kw):
    images = np.stack(images)
    got, status = decode(device, files, images.shape[1], images.shape[2], **kw)
    assert status == [JR.OK] * len(files), names_of(status)
    assert np.array_equal(got, images)


@functools.lru_cache(None)
def _pillow_expected():
    """Pillow's decode of every Pillow case, computed once (the CPU tests hold the reference decoder to it; the reference's frames are what the device is compared with, so
    that the GPU machine's libjpeg does not matter)"""
    return {name: ref_decode(data, H, W)[1] for name, H, W, data in pillow_cases()}


def check_pillow_files(device):
    """every Pillow case, the files of one size in one call"""
    want = _pillow_expected()
    groups = {}
    for name, H, W, data in pillow_cases():
        groups.setdefault((H, W), []).append((name, data))
    for (H, W), members in groups.items():
        got, status = decode(device, [d for _, d in members], H, W)
        assert status == [JR.OK] * len(members), (H, W, names_of(status))
        for i, (name, data) in enumerate(members):
            assert np.array_equal(got[i], want[name]), name
            if device == "cpu":
                assert np.array_equal(got[i], pillow_pixels(data)), name      # the device result against the installed decoder itself


def check_handwritten_by_reference():
    """the yardstick: the reference reads the token writer's files; where Pillow reads them too and no product wraps, it agrees"""
    for name, (H, W, data) in handwritten().items():
        st, frame = ref_decode(data, H, W)
        assert st == JR.OK, (name, JR.STATUS_NAMES[st])
        if "wrapping" not in name:
            assert np.array_equal(frame, pillow_pixels(data)), name


def check_handwritten(device):
    for name, (H, W, data) in handwritten().items():
        check_decodes(device, [data], [ref_decode(data, H, W)[1]])


# ---- with the writer -------------------------------------------------------------------------------------------------------------------------------------------------
def encode_on_device(device, frames, quality):
    """(n, H, W, 3) uint8 on the device -> (stream, offsets) as caddy_video_encode leaves them on the device"""
    from playablevideogeneration_amd import video_writer as VW
    n, H, W, _ = frames.shape
    enc = VW.JpegEncoder(H, W, n, quality, device=device)
    bound = enc.stream_bound(n)
    out = torch.zeros(bound, dtype=torch.uint8, device=device)
    off = torch.zeros(n + 1, dtype=torch.int32, device=device)
    enc._stream()
    enc._check(enc.lib.caddy_video_encode(enc.ctx, frames.data_ptr(), n, out.data_ptr(), bound, off.data_ptr()))
    return out, off


def check_round_trip(device, tmp_path=None):
    """JpegEncoder output into decode_stream with no host copy: every writer fixture; several frames in a call, also in chunks; read_video on a written .avi"""
    from playablevideogeneration_amd import video_writer as VW
    for name in VC.FIXTURE_IDS:
        frame, q, want_file, _ = VC.fixture(name)
        H, W = frame.shape[:2]
        frames = torch.from_numpy(np.array(frame)[None]).to(device)
        stream, off = encode_on_device(device, frames, q)
        got, status = decoder(device, H, W, 1).decode_stream(stream, off)
        want = ref_decode(want_file, H, W)[1]
        assert status.tolist() == [JR.OK] and np.array_equal(got[0].cpu().numpy(), want), name
    several = np.stack([np.asarray(image(24, 40, k, s)) for k, s in (("noise", 1), ("smooth", 2), ("constant", 3), ("noise", 4), ("smooth", 5))])
    stream, off = encode_on_device(device, torch.from_numpy(several).to(device), 90)
    files = stream.cpu().numpy().tobytes()
    o = off.cpu().tolist()
    want = np.stack([ref_decode(files[o[i]:o[i + 1]], 24, 40)[1] for i in range(5)])
    for room in (5, 2):
        got, status = decoder(device, 24, 40, room).decode_stream(stream, off)
        assert status.tolist() == [JR.OK] * 5 and np.array_equal(got.cpu().numpy(), want)
    if tmp_path is not None:
        path = str(tmp_path / "video.avi")
        VW.save_video(None, torch.from_numpy(several).to(device), path, fps=5, quality=90)
        info, got = JR.read_video(None, path, device=device)
        assert tuple(got.shape) == (5, 24, 40, 3) and np.array_equal(got.cpu().numpy(), want)


def check_chunking_and_reuse(device):
    """more images than the context holds; file starts at odd addresses; the second call on the same context is identical; the python front end"""
    H, W = 17, 33
    files = [pillow_file(image(H, W, k, s), quality=q, subsampling=sub, **kw) for k, s, q, sub, kw in
             (("noise", 1, 90, 0, {}), ("smooth", 2, 30, 2, {"restart_marker_blocks": 1}), ("noise", 3, 100, 1, {"optimize": True}), ("constant", 4, 75, 2, {}),
              ("smooth", 5, 90, 1, {"restart_marker_blocks": 2}))]
    images = [ref_decode(f, H, W)[1] for f in files]
    assert any(len(f) % 2 for f in files)
    for lead in (0, 1, 3):
        check_decodes(device, files, images, max_frames=2, lead=lead)
    check_decodes(device, files, images, max_frames=2)
    check_decodes(device, files[::-1], images[::-1], max_frames=5)
    dec = JR.JpegDecoder(H, W, 2, device=device)
    frames, status = dec(files)
    assert status == [0] * 5 and np.array_equal(frames.cpu().numpy(), np.stack(images)) and dec.last_copied == sum(len(f) for f in files) + 4 * 6
    assert torch.equal(JR.decode_jpegs(None, files, device=device), frames)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
REF_H, REF_W = 12, 20


def _replace_once(data, old, new):
    assert data.count(old) == 1, (old, data.count(old))
    return data.replace(old, new)


@functools.lru_cache(None)
def refusals():
    """[(name, file, expected status)]; geometry REF_H x REF_W"""
    H, W = REF_H, REF_W
    img = image(H, W, "smooth", 3)
    dcs, acs = std_codes()
    mcus = random_mcus(H, W, 0x11, 8)
    n = len(mcus)
    zero = [0] * 64
    head = [seg(0xD8), JFIF, dqt(FLAT_Q, (0, 1)), sof(H, W)] + std_dht()

    def build(parts, scan=None, tail=b"\xff\xd9"):
        return serialise(parts) + (join(intervals(mcus, 0, dcs, acs)) if scan is None else scan) + tail

    good = build(head + [sos()])
    assert ref_decode(good, H, W)[0] == JR.OK
    sos_at = good.index(b"\xff\xda")
    out = [("not_jpeg_png_signature", PR.SIGNATURE + bytes(40), JR.NOT_JPEG), ("not_jpeg_no_soi", good[2:], JR.NOT_JPEG)]
    for name, cut in (("empty", 0), ("cut_in_soi", 1), ("cut_in_dqt", 40), ("cut_in_a_length", good.index(b"\xff\xc4") + 3), ("cut_behind_sos", sos_at + 14),
                      ("cut_in_scan", sos_at + 14 + (len(good) - sos_at - 14) // 2), ("cut_before_eoi", len(good) - 2), ("cut_in_eoi", len(good) - 1)):
        out.append((name, good[:cut], JR.TRUNCATED))
    out.append(("eoi_before_sos", serialise(head) + b"\xff\xd9", JR.TRUNCATED))
    out.append(("scan_needs_more_bits", good[:-10] + b"\xff\xd9", JR.TRUNCATED))
    # UNSUPPORTED, one per cause
    out.append(("progressive", pillow_file(img, progressive=True), JR.UNSUPPORTED))
    out.append(("sof1_extended", build([sof(H, W, marker=0xC1) if p[0] == 0xC0 else p for p in head] + [sos()]), JR.UNSUPPORTED))
    out.append(("sof9_arithmetic", build([sof(H, W, marker=0xC9) if p[0] == 0xC0 else p for p in head] + [sos()]), JR.UNSUPPORTED))
    out.append(("precision_12", build([sof(H, W, precision=12) if p[0] == 0xC0 else p for p in head] + [sos()]), JR.UNSUPPORTED))
    out.append(("greyscale", pillow_file(np.asarray(img)[:, :, 0].copy()), JR.UNSUPPORTED))
    out.append(("cmyk_four_components", _cmyk(H, W), JR.UNSUPPORTED))
    out.append(("sampling_411", build([sof(H, W, 0x41) if p[0] == 0xC0 else p for p in head] + [sos()]), JR.UNSUPPORTED))
    out.append(("sampling_440", build([sof(H, W, 0x12) if p[0] == 0xC0 else p for p in head] + [sos()]), JR.UNSUPPORTED))
    out.append(("chroma_2x1", build([sof(H, W, 0x21, chroma=0x21) if p[0] == 0xC0 else p for p in head] + [sos()]), JR.UNSUPPORTED))
    out.append(("non_interleaved_scan", build(head + [sos(ids=(1,), tabs=(0x00,))]), JR.UNSUPPORTED))
    out.append(("scan_in_another_order", build(head + [sos(ids=(2, 1, 3))]), JR.UNSUPPORTED))
    out.append(("dqt_16_bit", build([seg(0xD8), JFIF, seg(0xDB, bytes([0x10]) + bytes(128)), dqt(FLAT_Q, (0, 1)), sof(H, W)] + std_dht() + [sos()]), JR.UNSUPPORTED))
    out.append(("dnl_height_0", build([sof(0, W) if p[0] == 0xC0 else p for p in head] + [sos()], tail=b"\xff\xdc\x00\x04" + H.to_bytes(2, "big") + b"\xff\xd9"), JR.UNSUPPORTED))
    out.append(("dnl_behind_the_scan", build(head + [sos()], tail=b"\xff\xdc\x00\x04" + H.to_bytes(2, "big") + b"\xff\xd9"), JR.UNSUPPORTED))
    out.append(("adobe_transform_0", build([seg(0xD8), adobe(0)] + head[2:] + [sos()]), JR.UNSUPPORTED))
    out.append(("adobe_transform_2", build([seg(0xD8), adobe(2)] + head[2:] + [sos()]), JR.UNSUPPORTED))
    rgb = (ord("R"), ord("G"), ord("B"))
    out.append(("ids_rgb_without_jfif", build([seg(0xD8), head[2], sof(H, W, ids=rgb)] + std_dht() + [sos(ids=rgb)]), JR.UNSUPPORTED))
    out.append(("spectral_end_62", build(head + [sos(tail=(0, 62, 0))]), JR.UNSUPPORTED))
    out.append(("successive_approximation", build(head + [sos(tail=(0, 63, 1))]), JR.UNSUPPORTED))
    # GEOMETRY
    out.append(("geometry", pillow_file(image(H, W + 1)), JR.GEOMETRY))
    out.append(("geometry_swapped", pillow_file(image(W, H)), JR.GEOMETRY))
    # BAD_TABLE
    out.append(("dqt_length_short", build([seg(0xD8), JFIF, seg(0xDB, bytes(64)), dqt(FLAT_Q, (0, 1)), sof(H, W)] + std_dht() + [sos()]), JR.BAD_TABLE))
    out.append(("dqt_id_4", build([seg(0xD8), JFIF, dqt(FLAT_Q, (0, 4)), sof(H, W)] + std_dht() + [sos()]), JR.BAD_TABLE))
    out.append(("dht_id_4", build(head + [dht([(0, 4, STD[(0, 0)])]), sos()]), JR.BAD_TABLE))
    out.append(("dht_class_2", build(head + [dht([(2, 0, STD[(0, 0)])]), sos()]), JR.BAD_TABLE))
    out.append(("dht_length_short", build(head + [seg(0xC4, bytes([0x00]) + bytes(STD[(0, 0)][0]) + bytes(STD[(0, 0)][1][:-1])), sos()]), JR.BAD_TABLE))
    out.append(("dht_over_subscribed", build(head + [dht([(0, 0, ([3] + [0] * 15, [0, 1, 2]))]), sos()]), JR.BAD_TABLE))
    out.append(("dht_257_symbols", build(head + [dht([(1, 0, ([0] * 14 + [2, 255], list(range(256)) + [0]))]), sos()]), JR.BAD_TABLE))
    out.append(("huffman_table_never_defined", build(head[:4] + std_dht()[:3] + [sos()]), JR.BAD_TABLE))
    out.append(("quantisation_table_never_defined", build([seg(0xD8), JFIF, dqt(FLAT_Q[:1], (0,)), sof(H, W)] + std_dht() + [sos()]), JR.BAD_TABLE))
    out.append(("component_table_id_4", build([sof(H, W, tq=(0, 1, 4)) if p[0] == 0xC0 else p for p in head] + [sos()]), JR.BAD_TABLE))
    out.append(("sos_without_sof", build([p for p in head if p[0] != 0xC0] + [sos()]), JR.BAD_TABLE))
    out.append(("second_sof", build(head + [sof(H, W), sos()]), JR.BAD_TABLE))
    out.append(("sos_length", build(head + [seg(0xDA, sos()[1] + b"\0")]), JR.BAD_TABLE))
    out.append(("dri_length", build(head + [seg(0xDD, bytes(3)), sos()]), JR.BAD_TABLE))
    out.append(("garbage_between_segments", build(head + [b"\x00\x01", sos()]), JR.BAD_TABLE))
    out.append(("rst_before_sos", build(head + [b"\xff\xd0", sos()]), JR.BAD_TABLE))
    # BAD_CODE: sixteen 1-bits are no code of the standard DC table
    out.append(("no_such_code", build(head + [sos()], scan=b"\xff\x00" * 6), JR.BAD_CODE))
    bad_ac = [list(m) for m in mcus]
    bad_ac[1] = [("raw", [(2, 3), (1, 1), (0xFFFF, 16), (0xFFFF, 16)]), zero, zero]      # DC category 1, then sixteen 1-bits where an AC code must stand
    out.append(("no_such_ac_code", build(head + [sos()], scan=join(intervals(bad_ac, 0, dcs, acs))), JR.BAD_CODE))
    # BAD_COEFFICIENT
    dc12, ac11 = codes_of(*DC16), dict(acs[0])
    parts12 = head[:4] + [dht([(0, 0, DC16)])] + std_dht()[1:] + [sos()]
    m12 = [[("raw", [(dc12[12][0], dc12[12][1]), (0xFFF, 12)]), zero, zero]] + mcus[1:]
    out.append(("dc_category_12", serialise(parts12) + join(intervals(m12, 0, [dc12, dcs[1], dcs[2]], acs)) + b"\xff\xd9", JR.BAD_COEFFICIENT))
    counts, symbols = STD[(1, 0)]
    symbols11 = [0x0B if s == 0xFA else s for s in symbols]
    ac11 = codes_of(counts, symbols11)
    parts11 = head[:4] + [std_dht()[0], dht([(1, 0, (counts, symbols11))])] + std_dht()[2:] + [sos()]
    m11 = [[("raw", [(dcs[0][0][0], dcs[0][0][1]), (ac11[0x0B][0], ac11[0x0B][1]), (0x7FF, 11)]), zero, zero]] + mcus[1:]
    out.append(("ac_size_11", serialise(parts11) + join(intervals(m11, 0, dcs, [ac11, acs[1], acs[2]])) + b"\xff\xd9", JR.BAD_COEFFICIENT))
    a0 = acs[0]
    run = [("raw", [(dcs[0][0][0], dcs[0][0][1])] + [(a0[0xF0][0], a0[0xF0][1])] * 3 + [(a0[0xF1][0], a0[0xF1][1]), (1, 1)]), zero, zero]      # k = 49, run 15: index 64
    out.append(("run_passes_63", build(head + [sos()], scan=join(intervals([run] + mcus[1:], 0, dcs, acs))), JR.BAD_COEFFICIENT))
    zrl = [("raw", [(dcs[0][0][0], dcs[0][0][1])] + [(a0[0xF0][0], a0[0xF0][1])] * 4), zero, zero]      # the fourth ZRL covers 49 .. 64
    out.append(("zrl_passes_63", build(head + [sos()], scan=join(intervals([zrl] + mcus[1:], 0, dcs, acs))), JR.BAD_COEFFICIENT))
    big = [[[2000] + zero[1:], zero, zero], [("raw", [(dcs[0][11][0], dcs[0][11][1]), (2000, 11), (a0[0][0], a0[0][1])]), zero, zero]] + [[[2000] + zero[1:], zero, zero]] * (n - 2)      # + 2000 on 2000
    out.append(("dc_value_4000", build(head + [sos()], scan=join(intervals(big, 0, dcs, acs))), JR.BAD_COEFFICIENT))
    # BAD_RESTART (Ri = 2: ceil(n / 2) intervals)
    ivs = intervals(mcus, 2, dcs, acs)
    assert len(ivs) >= 3
    rhead = head + [dri(2), sos()]
    ok = serialise(rhead) + join(ivs) + b"\xff\xd9"
    assert ref_decode(ok, H, W)[0] == JR.OK
    out.append(("rst_missing", serialise(rhead) + ivs[0] + join(ivs[1:], first=1) + b"\xff\xd9", JR.BAD_RESTART))
    out.append(("rst_extra", serialise(rhead) + join(ivs) + b"\xff" + bytes([0xD0 + ((len(ivs) - 1) & 7)]) + b"\xff\xd9", JR.BAD_RESTART))
    out.append(("rst_out_of_order", serialise(rhead) + join(ivs, first=1) + b"\xff\xd9", JR.BAD_RESTART))
    out.append(("rst_none_where_dri_says_some", serialise(rhead) + join(intervals(mcus, 0, dcs, acs)) + b"\xff\xd9", JR.BAD_RESTART))
    out.append(("rst_without_dri", serialise(head + [sos()]) + join(ivs) + b"\xff\xd9", JR.BAD_RESTART))
    out.append(("interval_ends_before_its_marker", serialise(rhead) + join([ivs[0][:-3]] + ivs[1:]) + b"\xff\xd9", JR.BAD_RESTART))
    out.append(("interval_ends_behind_its_marker", serialise(rhead) + join([ivs[0] + b"\x55"] + ivs[1:]) + b"\xff\xd9", JR.BAD_RESTART))
    # BAD_SCAN
    out.append(("bytes_left_over", build(head + [sos()], tail=b"\x12\x34\xff\xd9"), JR.BAD_SCAN))
    out.append(("com_behind_the_scan", build(head + [sos()], tail=b"\xff\xfe\x00\x02\xff\xd9"), JR.BAD_SCAN))
    out.append(("second_scan", build(head + [sos()], tail=serialise([sos()]) + b"\x00\xff\xd9"), JR.BAD_SCAN))
    out.append(("last_interval_left_over", serialise(rhead) + join(ivs) + b"\x55\xff\xd9", JR.BAD_SCAN))
    return out


def _cmyk(H, W):
    f = io.BytesIO()
    Image.fromarray(np.full((H, W, 4), 90, np.uint8), "CMYK").save(f, format="JPEG")
    return f.getvalue()


def check_refusals_by_the_reference():
    """the yardstick: the reference gives every refused file the status the cases name; every status and every listed cause is there; Pillow reads the encoder-written ones as
    something else than a baseline three-component file"""
    seen = set()
    for name, data, want in refusals():
        st, _ = ref_decode(data, REF_H, REF_W)
        assert st == want, (name, JR.STATUS_NAMES[st], JR.STATUS_NAMES[want])
        seen.add(want)
    assert seen == set(range(1, 10))
    by = {n: d for n, d, _ in refusals()}
    assert JR.probe(by["progressive"])[5] == 0xC2 and JR.probe(by["greyscale"])[3] == 1 and JR.probe(by["cmyk_four_components"])[3] == 4


def check_refusals(device):
    """each refused file in the middle of a batch of three whose neighbours decode exactly; the failed frame is zero; (the guards are checked by decode)"""
    H, W = REF_H, REF_W
    fa = pillow_file(image(H, W, "smooth", 1), quality=90, subsampling=2)
    fb = pillow_file(image(H, W, "noise", 2), quality=75, subsampling=0, restart_marker_blocks=1)
    a, b = ref_decode(fa, H, W)[1], ref_decode(fb, H, W)[1]
    wrong = []
    for name, data, want in refusals():
        frames, status = decode(device, [fa, data, fb], H, W, max_frames=3)
        if status != [JR.OK, want, JR.OK] or not np.array_equal(frames[0], a) or not np.array_equal(frames[2], b) or frames[1].any():
            wrong.append((name, names_of(status)))
    assert not wrong, wrong


def check_offsets_out_of_order(device):
    """offsets that are not monotonic or pass the total give that image an empty or shortened file, never a read outside the blob [0, offsets[n])"""
    H, W = REF_H, REF_W
    fa = pillow_file(image(H, W, "smooth", 1), quality=90, subsampling=2)
    a = ref_decode(fa, H, W)[1]
    n = len(fa)
    dec = decoder(device, H, W, 3)
    stream = torch.from_numpy(np.frombuffer(fa * 3, np.uint8).copy()).to(device)
    for offsets, want in (([0, n, 2 * n, 3 * n], [JR.OK] * 3),
                          ([0, 2 * n, n, 3 * n], [JR.OK, JR.TRUNCATED, JR.OK]),                   # two files as one (bytes behind EOI are ignored); [2n, n) is empty; two as one
                          ([n, 0, 5 * n, 3 * n], [JR.TRUNCATED, JR.OK, JR.TRUNCATED]),            # empty; clamped to the total; empty
                          ([7 * n, 7 * n, 7 * n, n], [JR.TRUNCATED] * 3),                         # everything clamped to the total
                          ([3, n, 2 * n + 1, 3 * n], [JR.NOT_JPEG, JR.OK, JR.NOT_JPEG])):         # starts inside a file
        got, status = dec.decode_stream(stream, torch.tensor(offsets, dtype=torch.int32, device=device))
        assert status.tolist() == want, (offsets, names_of(status.tolist()))
        for i, v in enumerate(want):
            assert np.array_equal(got[i].cpu().numpy(), a if v == JR.OK else np.zeros_like(a))


# ---- the mutation corpus -----------------------------------------------------------------------------------------------------------------------------------------------
CORPUS_H, CORPUS_W, CORPUS_SEED = 24, 24, 20261021


@functools.lru_cache(None)
def corpus():
    """[(file, the reference's status, the reference's frame or None)] from three valid files -- Pillow 4:2:0 with restart markers, Pillow 4:4:4 with optimised tables, a
    handwritten 4:2:2 one -- by seeded mutations: bytes anywhere, cuts, single bits of the scan, single bits of the table segments"""
    H, W = CORPUS_H, CORPUS_W
    bases = [pillow_file(image(H, W, "smooth", 1), quality=90, subsampling=2, restart_marker_blocks=1),
             pillow_file(image(H, W, "noise", 2), quality=30, subsampling=0, optimize=True),
             plain_file(H, W, 0x21, random_mcus(H, W, 0x21, 9), ri=1)]
    rng = np.random.default_rng(CORPUS_SEED)
    cases = []
    for z in bases:
        scan = z.index(b"\xff\xda") + 14
        for k in range(110):
            m = bytearray(z)
            family = k % 4
            if family == 0:                                        # one to three bytes anywhere
                for _ in range(int(rng.integers(1, 4))):
                    m[int(rng.integers(0, len(m)))] ^= int(rng.integers(1, 256))
            elif family == 1:                                      # a cut (every other one inside the scan)
                m = m[:int(rng.integers(scan if k % 8 == 1 else 0, len(m)))]
            elif family == 2:                                      # one bit of the scan
                m[int(rng.integers(scan, len(m) - 2))] ^= 1 << int(rng.integers(0, 8))
            else:                                                  # one bit in front of the scan
                m[int(rng.integers(2, scan))] ^= 1 << int(rng.integers(0, 8))
            m = bytes(m)
            st, frame = ref_decode(m, H, W)
            cases.append((m, st, frame))
    return cases


def check_corpus_conditions():
    """asserted on the CPU, by the reference alone: the corpus is large and varied enough, and shows both outcomes"""
    cases = corpus()
    originals = [c[2] for c in cases if c[1] == JR.OK]
    seen = {c[1] for c in cases}
    accepted = len(originals)
    assert len(cases) >= 300 and 20 <= accepted <= len(cases) - 100 and len(seen) >= 8, (len(cases), accepted, sorted(seen))
    return len(cases), accepted, sorted(seen)


def check_corpus(device):
    """every status in range and equal to the reference's; where it is OK the frame is the reference's, where not the frame is zero; the share of OK is neither 0 nor 1"""
    check_corpus_conditions()
    cases = corpus()
    H, W = CORPUS_H, CORPUS_W
    wrong, accepted = [], 0
    for at in range(0, len(cases), 64):
        part = cases[at:at + 64]
        frames, status = decode(device, [f for f, _, _ in part], H, W, max_frames=64)
        for i, (data, want, frame) in enumerate(part):
            if not 0 <= status[i] < len(JR.STATUS_NAMES):
                wrong.append((at + i, status[i]))
            elif status[i] != want:
                wrong.append((at + i, JR.STATUS_NAMES[status[i]], JR.STATUS_NAMES[want]))
            elif want == JR.OK and not np.array_equal(frames[i], frame):
                wrong.append((at + i, "pixels"))
            elif want != JR.OK and frames[i].any():
                wrong.append((at + i, "frame not zero"))
            accepted += status[i] == JR.OK
    assert not wrong, wrong
    assert 0 < accepted < len(cases)
