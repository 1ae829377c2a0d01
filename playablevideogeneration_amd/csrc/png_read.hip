// Device-side PNG reader: complete PNG files (8-bit RGB, no interlace, any number of IDATs) parsed, inflated and unfiltered on the device into the uint8 interleaved frames the
// frame pipeline (frames.hip: caddy_frames_observations) reads -- only the compressed bytes cross the bus.  Takes the place of the host's PIL Image.open per frame in a
// DataLoader worker (dataset/video.py:136-157).  The input is what caddy_png_encode (png.hip) leaves: the files back to back and n + 1 offsets.  The contract is the bytes:
// what Pillow decodes, a zlib stream accepted exactly where zlib's inflate accepts it (include/caddy_hip.h states the rules).
//
// One launch per chunk of at most max_frames images: k_png_read, grid (nf), one workgroup of ONE wave per image, the three stages one after the other in it:
//   (a) parse     every lane walks the chunk headers (the same few bytes: one broadcast load); the wave takes the CRC-32 of IHDR, every IDAT and IEND in 64 pieces (table per
//                 piece, the pieces shifted by x^(8 len) and met by XOR, as png.hip's) and gathers the IDAT payloads into the image's slice of the workspace
//   (b) inflate   lane 0 reads the bits (64-bit window, refilled by 32-bit words with the next word already under way) against tables in LDS: a 10-bit first-level table per
//                 alphabet, filled by the whole wave, and the canonical count / symbol walk for longer codes.  It queues up to 64 tokens; the wave then writes the literals, one
//                 a lane, and copies every match 64 bytes at a time (an overlapping match reads out[p - d + j mod d], which lies before the match).  A match whose source lies
//                 in the same batch waits for a barrier first; the others need none.  Stored blocks are a wave-wide copy.  Adler-32 in 64 pieces.
//   (c) unfilter  rows run staggered, 64 at a time: at step s lane t has pixel s - t of row band + t.  Left and upper-left are its own registers, the pixel above comes from
//                 lane t - 1 by one shuffle (lane 0: from the frame, the band before), so Average and Paeth, serial along a row, cost W + 63 steps for 64 rows.
// Why one launch and one wave: each stage is serial per image in its critical part (the chunk walk, the bit stream, the filter recurrence), a stage's verdict decides whether
// the next runs at all, and a one-wave workgroup's barrier is only the wave waiting for its own memory operations.  Keeping the stages in one kernel leaves the verdict and the
// lengths in LDS / registers and the launch count at one.  Not built: a parallel split of one stream.
//
// Safety (the bytes come from outside): every read of the blob is bounded by the end of that file (itself clamped to offsets[n]); past the gathered IDAT bytes the bit reader
// yields zeros and the image ends TRUNCATED; every write is bounded by the image's own slice (capacity / stream bytes) or its own frame.  Every loop states below what it consumes
// or produces and the bound known before it starts.
#include "eval_ctx.h"
#include "png_read.h"
#include <cstring>

namespace {

constexpr int RD_THREADS = 64;                 // one wave: __syncthreads() is the wave's own wait
constexpr int RD_TOKENS = 64;                  // tokens lane 0 queues before the wave writes them
constexpr int RD_FAST = 10;                    // bits of the first-level decoding tables
constexpr int RD_NLL = 288, RD_ND = 32;        // the fixed code has 288 / 32 codes (286, 287 and 30, 31 carry a code and are refused where one is met)
constexpr unsigned RD_POLY = 0xEDB88320u, RD_ADLER = 65521u;
enum { KIND_CODES = 0, KIND_LENS = 1, KIND_DISTS = 2 };
// sh[] words lane 0 leaves for the wave
enum { S_STATUS = 0, S_FINAL, S_TYPE, S_LEN, S_SRC, S_NTOK, S_EOB, S_OUT, S_NLL, S_ND, S_FLAG, S_COUNT };

struct ReadArgs {
    const unsigned char* files; const unsigned* offsets; long n_total, n0;
    int nf, H, W;
    long stream, capacity, zstride, sstride;
    const unsigned* crc_table;        // 256 + 32 words
    unsigned char* zbuf;              // nf x zstride: an image's IDAT payloads, gathered
    unsigned char* sbuf;              // nf x sstride: its inflated (filtered) stream
    unsigned char* frames;            // (n_total, H, W, 3)
    int* status;                      // n_total
};

struct Tables {      // LDS of one image
    unsigned short fast_ll[1 << RD_FAST], fast_d[1 << RD_FAST];      // symbol << 4 | length of the code whose reversed bits are the index's low bits; 0: longer than RD_FAST, or none
    unsigned short sym_ll[RD_NLL], sym_d[RD_ND];                     // symbols ordered by (length, symbol)
    unsigned short cnt_ll[16], cnt_d[16];                            // codes of every length
    unsigned short code[RD_NLL];                                     // canonical code of every symbol (table build)
    unsigned char lens[RD_NLL + RD_ND];
    unsigned tok_pos[RD_TOKENS], tok_what[RD_TOKENS];                // where a token's bytes go; literal: the byte; match: length | distance << 9 | (source in this batch) << 31
    unsigned long long red[2 * RD_THREADS];
    unsigned crc_t[256 + 32];
    unsigned sh[S_COUNT];
};

// ---- CRC-32 in pieces (png.hip: the same method) -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned rd_mulmod(unsigned a, unsigned b) {
    unsigned p = 0u;
    for (int i = 0; i < 32; i++) {      // (32 steps)
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ RD_POLY : b >> 1;
    }
    return p;
}
__device__ __forceinline__ unsigned rd_shift_bytes(unsigned v, unsigned long long nbytes, const unsigned* xp) {
    unsigned long long n = nbytes;
    for (int k = 3; n; k++, n >>= 1) if (n & 1ull) v = rd_mulmod(xp[k & 31], v);      // (n loses a bit every step: at most 64)
    return v;
}
// CRC-32 of p[0, n), in every lane; the caller has checked that p[0, n) lies inside the file
__device__ unsigned wave_crc(const unsigned char* p, unsigned n, const unsigned* crc_t) {
    const unsigned lane = threadIdx.x, piece = (n + RD_THREADS - 1u) / RD_THREADS;
    const unsigned q0 = lane * piece < n ? lane * piece : n, q1 = q0 + piece < n ? q0 + piece : n;
    unsigned crc = 0u;
    for (unsigned q = q0; q < q1; q++) crc = crc_t[(crc ^ p[q]) & 255u] ^ (crc >> 8);      // reads one byte of [q0, q1) a step, inside [0, n)
    if (q1 > q0) crc = rd_shift_bytes(crc, n - q1, crc_t + 256);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) crc ^= __shfl_xor(crc, s);
    return crc ^ rd_shift_bytes(0xFFFFFFFFu, n, crc_t + 256) ^ 0xFFFFFFFFu;
}
__device__ __forceinline__ unsigned be32(const unsigned char* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3]; }

// ---- (a) parse: -> status; zlen = the IDAT bytes gathered into z[0, capacity) -----------------------------------------------------------------------------------------------
__device__ int parse(const ReadArgs& a, const unsigned char* file, unsigned flen, unsigned char* z, Tables& L, unsigned& zlen) {
    const unsigned lane = threadIdx.x;
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    zlen = 0u;
    for (unsigned i = 0; i < 8u && i < flen; i++) if (file[i] != sig[i]) return CADDY_PNG_NOT_PNG;      // (at most 8 bytes, below flen)
    if (flen < 8u) return CADDY_PNG_TRUNCATED;
    unsigned pos = 8u;
    bool first = true;
    // every pass consumes one chunk of 12 + len bytes of [pos, flen): at most (flen - 8) / 12 passes
    for (;;) {
        const unsigned avail = flen - pos;      // (pos <= flen throughout)
        if (avail < 8u) return CADDY_PNG_TRUNCATED;
        const unsigned len = be32(file + pos), type = be32(file + pos + 4);
        if (first && (type != 0x49484452u || len != 13u)) return CADDY_PNG_NOT_PNG;      // 'IHDR'
        if (avail < 12u || len > avail - 12u) return CADDY_PNG_TRUNCATED;
        const unsigned char* data = file + pos + 8;      // data[0, len) and the CRC behind it lie inside the file
        const bool ihdr = first, idat = type == 0x49444154u, iend = type == 0x49454E44u;
        if (ihdr || idat || iend) {
            if (wave_crc(file + pos + 4, len + 4u, L.crc_t) != be32(data + len)) return CADDY_PNG_BAD_CRC;
        } else if (!((type >> 29) & 1u) && type != 0x504C5445u) return CADDY_PNG_UNSUPPORTED;      // a critical chunk other than PLTE (an ancillary one has bit 5 of its first letter set)
        if (ihdr) {
            if (data[8] != 8 || data[9] != 2 || data[10] != 0 || data[11] != 0 || data[12] != 0) return CADDY_PNG_UNSUPPORTED;
            if (be32(data) != (unsigned)a.W || be32(data + 4) != (unsigned)a.H) return CADDY_PNG_GEOMETRY;
        } else if (idat) {
            if ((unsigned long long)zlen + len > (unsigned long long)a.capacity) return CADDY_PNG_TOO_LARGE;
            for (unsigned j = lane; j < len; j += RD_THREADS) z[zlen + j] = data[j];      // produces bytes [zlen, zlen + len) <= capacity of the image's own slice
            zlen += len;
        } else if (iend) return CADDY_PNG_OK;
        first = false;
        pos += 12u + len;
    }
}

// ---- (b) inflate ----------------------------------------------------------------------------------------------------------------------------------------------------
// The bit reader of lane 0 over z[0, n): LSB first; zeros past n (used() > 8 n tells).  z is the image's own 16-byte aligned slice, read by words below ceil(n / 4).
struct Bits {
    const unsigned char* z; unsigned n, wi, nxt; unsigned long long acc; int cnt;
    __device__ __forceinline__ unsigned word(unsigned i) const {
        if (4ull * i >= n) return 0u;
        const unsigned v = ((const unsigned*)z)[i], left = n - 4u * i;
        return left >= 4u ? v : v & ((1u << (8u * left)) - 1u);
    }
    __device__ __forceinline__ void seek(unsigned byte) {
        wi = byte >> 2;
        const unsigned s = 8u * (byte & 3u);
        acc = (unsigned long long)(word(wi) >> s); cnt = 32 - (int)s;
        wi++; nxt = word(wi);
    }
    __device__ __forceinline__ void fill() { if (cnt <= 32) { acc |= (unsigned long long)nxt << cnt; cnt += 32; wi++; nxt = word(wi); } }      // -> at least 33 bits
    __device__ __forceinline__ unsigned peek(int k) const { return (unsigned)acc & ((1u << k) - 1u); }      // k <= 16
    __device__ __forceinline__ void drop(int k) { acc >>= k; cnt -= k; }
    __device__ __forceinline__ unsigned take(int k) { const unsigned v = peek(k); drop(k); return v; }
    __device__ __forceinline__ unsigned long long used() const { return 32ull * wi - (unsigned long long)cnt; }
    __device__ __forceinline__ bool over() const { return used() > 8ull * n; }
};

// one symbol (lane 0; at least 15 bits in the window): -1 where no code matches
__device__ __forceinline__ int decode(Bits& b, const unsigned short* fast, const unsigned short* cnt, const unsigned short* sym) {
    const unsigned v = b.peek(15), e = fast[v & ((1u << RD_FAST) - 1u)];
    if (e) { b.drop((int)(e & 15u)); return (int)(e >> 4); }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; len++) {      // (15 steps)
        code |= (int)((v >> (len - 1)) & 1u);
        const int c = cnt[len];
        if (code - c < first) { b.drop(len); return sym[index + (code - first)]; }
        index += c; first += c; first <<= 1; code <<= 1;
    }
    return -1;
}

// The decoding tables of lens[0, n), n <= RD_NLL (every lane calls it).  zlib's inflate_table rules: an over-subscribed set is refused; an incomplete one too, unless it is
// one single code of length 1 in a literal / length or distance set; no code at all is an empty table (every code met is then refused), which a code-length set may not be.
__device__ bool build_table(Tables& L, const unsigned char* lens, int n, int kind, unsigned short* fast, unsigned short* cnt, unsigned short* sym) {
    const int lane = threadIdx.x;
    for (int i = lane; i < (1 << RD_FAST); i += RD_THREADS) fast[i] = 0;
    if (lane == 0) {
        int count[16], offs[16];
        for (int i = 0; i < 16; i++) count[i] = 0;
        for (int i = 0; i < n; i++) count[lens[i]]++;      // (lens are 0..15)
        count[0] = 0;
        int maxl = 15;
        while (maxl > 0 && count[maxl] == 0) maxl--;      // (at most 15 steps)
        bool bad = maxl == 0 && kind == KIND_CODES;
        int left = 1;
        for (int len = 1; len <= 15 && maxl > 0; len++) { left <<= 1; left -= count[len]; if (left < 0) { bad = true; break; } }
        if (maxl > 0 && left > 0 && (kind == KIND_CODES || maxl != 1)) bad = true;
        unsigned next = 0u;
        int at = 0;
        unsigned nx[16];
        for (int len = 1; len <= 15; len++) { next = (next + (unsigned)count[len - 1]) << 1; nx[len] = next; offs[len] = at; at += count[len]; cnt[len] = (unsigned short)count[len]; }
        cnt[0] = 0;
        if (!bad) for (int i = 0; i < n; i++) { const int l = lens[i]; if (l) { sym[offs[l]++] = (unsigned short)i; L.code[i] = (unsigned short)nx[l]++; } }
        L.sh[S_FLAG] = bad ? 1u : 0u;
    }
    __syncthreads();
    const bool ok = L.sh[S_FLAG] == 0u;
    if (ok) for (int i = lane; i < n; i += RD_THREADS) {
        const int l = lens[i];
        if (l < 1 || l > RD_FAST) continue;
        const unsigned rev = __builtin_bitreverse32((unsigned)L.code[i]) >> (32 - l);
        for (unsigned k = rev; k < (1u << RD_FAST); k += 1u << l) fast[k] = (unsigned short)((i << 4) | l);      // (a complete-or-less code: the entries of two symbols are disjoint)
    }
    __syncthreads();
    return ok;
}

// z[0, zlen) -> out[0, stream); every lane gets the verdict
__device__ int inflate(const unsigned char* z, unsigned zlen, unsigned char* out, unsigned stream, Tables& L) {
    const unsigned lane = threadIdx.x;
    Bits b{};
    if (zlen < 2u) return CADDY_PNG_TRUNCATED;
    {
        const unsigned cmf = z[0], flg = z[1];
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return CADDY_PNG_BAD_DEFLATE;
    }
    b.z = z; b.n = zlen;
    if (lane == 0) { b.seek(2u); L.sh[S_OUT] = 0u; L.sh[S_STATUS] = CADDY_PNG_OK; }
    __syncthreads();
    // every block consumes at least its 3 header bits of the 8 zlen the stream has (a pass that reads past them ends the image)
    for (;;) {
        if (lane == 0) {
            int st = CADDY_PNG_OK;
            b.fill();
            const unsigned final_block = b.take(1), type = b.take(2);
            L.sh[S_FINAL] = final_block; L.sh[S_TYPE] = type;
            if (b.over()) st = CADDY_PNG_TRUNCATED;
            else if (type == 3u) st = CADDY_PNG_BAD_DEFLATE;
            else if (type == 0u) {
                b.drop(b.cnt & 7);
                b.fill();
                const unsigned len = b.take(16), nlen = b.take(16);
                const unsigned long long at = b.used() >> 3;
                if (b.over()) st = CADDY_PNG_TRUNCATED;
                else if ((len ^ nlen) != 0xFFFFu) st = CADDY_PNG_BAD_DEFLATE;
                else if (at + len > zlen) st = CADDY_PNG_TRUNCATED;
                else if ((unsigned long long)L.sh[S_OUT] + len > stream) st = CADDY_PNG_BAD_LENGTH;
                L.sh[S_LEN] = len; L.sh[S_SRC] = (unsigned)at;      // (at <= zlen where st is OK)
            } else if (type == 2u) {
                const unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                const unsigned hlit = b.take(5) + 257u, hdist = b.take(5) + 1u, hclen = b.take(4) + 4u;
                if (hlit > 286u || hdist > 30u) st = CADDY_PNG_BAD_DEFLATE;
                for (int i = 0; i < 19; i++) L.lens[i] = 0;
                for (unsigned i = 0; i < hclen; i++) { b.fill(); L.lens[order[i]] = (unsigned char)b.take(3); }      // (hclen <= 19 steps of 3 bits)
                if (b.over()) st = CADDY_PNG_TRUNCATED;
                L.sh[S_NLL] = hlit; L.sh[S_ND] = hdist;
            }
            L.sh[S_STATUS] = (unsigned)st;
        }
        __syncthreads();
        if (L.sh[S_STATUS] != CADDY_PNG_OK) break;
        const unsigned type = L.sh[S_TYPE], final_block = L.sh[S_FINAL];      // (registers: lane 0 rewrites the words in the next pass, behind at least one barrier)
        if (type == 0u) {
            const unsigned len = L.sh[S_LEN], src = L.sh[S_SRC], to = L.sh[S_OUT];
            for (unsigned j = lane; j < len; j += RD_THREADS) out[to + j] = z[src + j];      // produces [to, to + len) <= stream from z[src, src + len) <= zlen: both checked by lane 0
            __syncthreads();
            if (lane == 0) { L.sh[S_OUT] = to + len; b.seek(src + len); }
        } else {
            int n_ll = RD_NLL, n_d = RD_ND;
            if (type == 1u) {
                for (int i = lane; i < RD_NLL + RD_ND; i += RD_THREADS) L.lens[i] = (unsigned char)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
                __syncthreads();
            } else {
                n_ll = (int)L.sh[S_NLL]; n_d = (int)L.sh[S_ND];
                const bool ok = build_table(L, L.lens, 19, KIND_CODES, L.fast_d, L.cnt_d, L.sym_d);
                if (lane == 0) {
                    int st = ok ? CADDY_PNG_OK : CADDY_PNG_BAD_DEFLATE;
                    const int total = n_ll + n_d;
                    int have = 0;
                    // every pass consumes at least one bit and produces at least one of the total <= 316 lengths
                    while (st == CADDY_PNG_OK && have < total) {
                        b.fill();
                        const int s = decode(b, L.fast_d, L.cnt_d, L.sym_d);
                        int rep = 1, val = s;
                        if (s == 16) { rep = 3 + (int)b.take(2); val = have > 0 ? L.lens[have - 1] : -1; }
                        else if (s == 17) { rep = 3 + (int)b.take(3); val = 0; }
                        else if (s == 18) { rep = 11 + (int)b.take(7); val = 0; }
                        if (b.over()) st = CADDY_PNG_TRUNCATED;
                        else if (s < 0 || val < 0 || have + rep > total) st = CADDY_PNG_BAD_DEFLATE;
                        else for (int i = 0; i < rep; i++) L.lens[have++] = (unsigned char)val;      // (have + rep <= total <= 316 = the array)
                    }
                    if (st == CADDY_PNG_OK && L.lens[256] == 0) st = CADDY_PNG_BAD_DEFLATE;      // no end-of-block code
                    L.sh[S_STATUS] = (unsigned)st;
                }
                __syncthreads();
                if (L.sh[S_STATUS] != CADDY_PNG_OK) break;
            }
            const bool ok_ll = build_table(L, L.lens, n_ll, KIND_LENS, L.fast_ll, L.cnt_ll, L.sym_ll);
            const bool ok_d = build_table(L, L.lens + n_ll, n_d, KIND_DISTS, L.fast_d, L.cnt_d, L.sym_d);
            if (!ok_ll || !ok_d) { if (lane == 0) L.sh[S_STATUS] = CADDY_PNG_BAD_DEFLATE; __syncthreads(); break; }
            // every batch consumes at least one bit (a code has at least one) of the 8 zlen and produces at most stream - S_OUT bytes; reading past the end or writing
            // past stream ends the image
            for (;;) {
                if (lane == 0) {
                    int st = CADDY_PNG_OK;
                    unsigned nt = 0u, eob = 0u, at = L.sh[S_OUT];
                    const unsigned start = at;
                    while (nt < (unsigned)RD_TOKENS) {      // every token consumes at least one bit; at most RD_TOKENS tokens
                        b.fill();
                        const int s = decode(b, L.fast_ll, L.cnt_ll, L.sym_ll);
                        if (s >= 0 && s < 256) {
                            if (b.over()) { st = CADDY_PNG_TRUNCATED; break; }
                            if (at >= stream) { st = CADDY_PNG_BAD_LENGTH; break; }
                            L.tok_pos[nt] = at; L.tok_what[nt] = (unsigned)s; nt++; at++;
                            continue;
                        }
                        if (s == 256) { if (b.over()) st = CADDY_PNG_TRUNCATED; else eob = 1u; break; }
                        unsigned len = 0u, dist = 0u;
                        int ds = -1;
                        if (s > 256 && s < 286) {
                            const int eb = (s < 265 || s == 285) ? 0 : (s - 261) >> 2;
                            len = s < 265 ? (unsigned)(s - 254) : s == 285 ? 258u : 3u + ((4u + (unsigned)((s - 265) & 3)) << eb) + b.take(eb);
                            b.fill();
                            ds = decode(b, L.fast_d, L.cnt_d, L.sym_d);
                            if (ds >= 0 && ds < 30) {
                                const int de = ds < 4 ? 0 : (ds >> 1) - 1;
                                dist = ds < 4 ? (unsigned)ds + 1u : 1u + ((2u + (unsigned)(ds & 1)) << de) + b.take(de);
                            }
                        }
                        if (b.over()) { st = CADDY_PNG_TRUNCATED; break; }
                        if (s < 0 || s >= 286 || ds < 0 || ds >= 30 || dist > at) { st = CADDY_PNG_BAD_DEFLATE; break; }      // no such code; 286 / 287; 30 / 31; before the first byte
                        if ((unsigned long long)at + len > stream) { st = CADDY_PNG_BAD_LENGTH; break; }
                        const unsigned reach = at - dist + (dist < len ? dist : len);      // the end of the bytes the match reads
                        L.tok_pos[nt] = at; L.tok_what[nt] = len | (dist << 9) | (reach > start ? 0x80000000u : 0u); nt++; at += len;
                    }
                    L.sh[S_NTOK] = nt; L.sh[S_EOB] = eob; L.sh[S_OUT] = at; L.sh[S_STATUS] = (unsigned)st;
                }
                __syncthreads();
                const unsigned nt = L.sh[S_NTOK];      // (<= RD_TOKENS; the positions and lengths were checked against stream by lane 0)
                const bool last = L.sh[S_STATUS] != CADDY_PNG_OK || L.sh[S_EOB];      // (a register: lane 0 rewrites the words behind the barrier below)
                if (lane < nt && !((L.tok_what[lane] >> 9) & 0xFFFFu)) out[L.tok_pos[lane]] = (unsigned char)L.tok_what[lane];
                for (unsigned k = 0; k < nt; k++) {      // produces the bytes of at most RD_TOKENS matches, each inside [0, stream)
                    const unsigned what = L.tok_what[k], dist = (what >> 9) & 0xFFFFu, len = what & 511u, p = L.tok_pos[k];
                    if (!dist) continue;
                    if (what >> 31) __syncthreads();      // its source was written in this batch
                    for (unsigned j = lane; j < len; j += RD_THREADS) out[p + j] = out[p - dist + (j % dist)];      // reads [p - dist, p), p >= dist
                }
                __syncthreads();
                if (last) break;
            }
            if (L.sh[S_STATUS] != CADDY_PNG_OK) break;      // (nobody writes the word before the next barrier)
        }
        __syncthreads();
        if (final_block) break;
    }
    __syncthreads();
    const unsigned verdict = L.sh[S_STATUS], produced = L.sh[S_OUT];
    __syncthreads();      // (every lane has read the words lane 0 writes next)
    if (verdict != CADDY_PNG_OK) return (int)verdict;
    if (produced != stream) return CADDY_PNG_BAD_LENGTH;
    // Adler-32 of out[0, stream) in 64 pieces: A = 1 + sum of the bytes, B = stream + sum of (stream - i) byte[i]; a piece is below 2^25 bytes, so its sums stay below 2^58
    const unsigned piece = (stream + RD_THREADS - 1u) / RD_THREADS;
    const unsigned q0 = lane * piece < stream ? lane * piece : stream, q1 = q0 + piece < stream ? q0 + piece : stream;
    unsigned long long s1 = 0ull, s2 = 0ull;
    for (unsigned q = q0; q < q1; q++) { const unsigned v = out[q]; s1 += v; s2 += (unsigned long long)(q1 - q) * v; }      // reads one byte of [q0, q1) a step, inside [0, stream)
    L.red[lane] = s1 % RD_ADLER;
    L.red[RD_THREADS + lane] = (s2 % RD_ADLER + (unsigned long long)(stream - q1) * (s1 % RD_ADLER)) % RD_ADLER;
    if (lane == 0) {
        int st = CADDY_PNG_OK;
        b.drop(b.cnt & 7);
        unsigned want = 0u;
        for (int i = 0; i < 4; i++) { b.fill(); want = (want << 8) | b.take(8); }
        if (b.over()) st = CADDY_PNG_TRUNCATED;
        L.sh[S_LEN] = want; L.sh[S_STATUS] = (unsigned)st;
    }
    __syncthreads();
    const unsigned tail = L.sh[S_STATUS];
    if (tail != CADDY_PNG_OK) return (int)tail;
    unsigned long long A = 1ull, B = stream % RD_ADLER;
    for (int i = 0; i < RD_THREADS; i++) { A += L.red[i]; B += L.red[RD_THREADS + i]; }
    const unsigned adler = ((unsigned)(B % RD_ADLER) << 16) | (unsigned)(A % RD_ADLER);
    return adler == L.sh[S_LEN] ? CADDY_PNG_OK : CADDY_PNG_BAD_ADLER;
}

// ---- (c) unfilter: s[0, H (1 + 3 W)) -> frame (H, W, 3) --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned load3(const unsigned char* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16); }
__device__ __forceinline__ int rd_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ int unfilter(const unsigned char* s, unsigned char* frame, int H, int W, Tables& L) {
    const int lane = threadIdx.x;
    const long rb = 3L * W, row = rb + 1;
    unsigned bad = 0u;
    for (long y = lane; y < H; y += RD_THREADS) bad |= s[y * row] > 4 ? 1u : 0u;      // reads one type byte a step: H / 64 steps inside the stream
    if (lane == 0) L.sh[S_FLAG] = 0u;
    __syncthreads();
    if (bad) atomicOr(&L.sh[S_FLAG], 1u);
    __syncthreads();
    if (L.sh[S_FLAG]) return CADDY_PNG_BAD_FILTER;
    // a band produces 64 rows (the last band what is left of H) in W + 63 steps
    for (long band = 0; band < H; band += RD_THREADS) {
        const long y = band + lane;
        const bool active = y < H;
        const unsigned char* src = s + (active ? y : 0) * row + 1;      // the row's 3 W filtered bytes
        unsigned char* dst = frame + (active ? y : 0) * rb;
        const unsigned char* above = (lane == 0 && band > 0) ? frame + (y - 1) * rb : nullptr;      // the band before left it there
        const int ft = active ? src[-1] : 0;
        unsigned a = 0u, c = 0u;
        unsigned raw_next = (active && lane == 0) ? load3(src) : 0u;      // pixel 0 of lane 0, one step ahead
        unsigned up_next = above ? load3(above) : 0u;
        for (int step = 0; step < W + RD_THREADS - 1; step++) {
            const int x = step - lane;
            unsigned b = __shfl(a, (lane - 1) & 63);      // what the lane above produced in the step before: its pixel x
            if (lane == 0) b = up_next;
            const bool mine = active && x >= 0 && x < W;
            const unsigned raw = raw_next;
            if (active && x + 1 >= 0 && x + 1 < W) {      // the loads of the next step, under way while this pixel is computed: inside the row / the row above
                raw_next = load3(src + 3L * (x + 1));
                if (above) up_next = load3(above + 3L * (x + 1));
            }
            if (!mine) continue;
            if (x == 0) { a = 0u; c = 0u; }
            unsigned px = 0u;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const int av = (a >> (8 * ch)) & 255, bv = (b >> (8 * ch)) & 255, cv = (c >> (8 * ch)) & 255;
                const int pred = ft == 0 ? 0 : ft == 1 ? av : ft == 2 ? bv : ft == 3 ? (av + bv) >> 1 : rd_paeth(av, bv, cv);
                px |= ((((raw >> (8 * ch)) & 255u) + (unsigned)pred) & 255u) << (8 * ch);
            }
            dst[3L * x] = (unsigned char)px; dst[3L * x + 1] = (unsigned char)(px >> 8); dst[3L * x + 2] = (unsigned char)(px >> 16);      // pixel x < W of row y < H
            a = px; c = b;
        }
        __syncthreads();
    }
    return CADDY_PNG_OK;
}

__global__ __launch_bounds__(RD_THREADS) void k_png_read(ReadArgs a) {
    __shared__ Tables L;
    const int lane = threadIdx.x, f = blockIdx.x;
    const long g = a.n0 + f;
    for (int i = lane; i < 256 + 32; i += RD_THREADS) L.crc_t[i] = a.crc_table[i];
    __syncthreads();
    // the file: [o0, o1) clamped to the blob [0, offsets[n]); offsets out of order give an empty or shortened file
    const unsigned total = a.offsets[a.n_total];
    const unsigned o0 = a.offsets[g] < total ? a.offsets[g] : total, o1 = a.offsets[g + 1] < total ? a.offsets[g + 1] : total;
    const unsigned flen = o1 > o0 ? o1 - o0 : 0u;
    unsigned char* z = a.zbuf + (long)f * a.zstride;
    unsigned char* s = a.sbuf + (long)f * a.sstride;
    unsigned char* frame = a.frames + g * ((long)a.H * a.W * 3);
    unsigned zlen = 0u;
    int st = parse(a, a.files + o0, flen, z, L, zlen);
    __syncthreads();      // (the gathered bytes are read by lane 0)
    if (st == CADDY_PNG_OK) st = inflate(z, zlen, s, (unsigned)a.stream, L);
    __syncthreads();
    if (st == CADDY_PNG_OK) st = unfilter(s, frame, a.H, a.W, L);
    if (st != CADDY_PNG_OK) for (long i = lane; i < (long)a.H * a.W * 3; i += RD_THREADS) frame[i] = 0;      // produces the image's own frame, zero
    if (lane == 0) a.status[g] = st;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
long rd_stream(int H, int W) { return (long)H * (1 + 3L * W); }
// zlib's deflateBound for parameters other than its defaults (Pillow sets memLevel 9, and measured on noise its files pass the tighter compressBound) and the 6 bytes of the
// zlib wrapper; above what png.hip writes at most, S + 5 ceil(S / 16384) + 6, for every S
long rd_capacity(int H, int W) {
    const long S = rd_stream(H, W);
    return S + ((S + 7) >> 3) + ((S + 63) >> 6) + 5 + 6;
}
bool rd_args_ok(int max_frames, int H, int W) {
    if (max_frames < 1 || H < 1 || W < 1) { set_error("caddy_png_read: max_frames, height and width must be positive"); return false; }
    if (max_frames > 65535) { set_error("caddy_png_read: at most 65535 images per chunk"); return false; }
    // (the limit of caddy_png_ctx_create: what the writer may produce for one image stays below 2^31)
    if ((unsigned long long)H * (1ull + 3ull * W) > 0x7FFFFFFFull || 63ull + (unsigned long long)rd_stream(H, W) + 5ull * ((rd_stream(H, W) + CADDY_PNG_BLOCK - 1) / CADDY_PNG_BLOCK) > 0x7FFFFFFFull) {
        set_error("caddy_png_read: the bound of one " + std::to_string(H) + " x " + std::to_string(W) + " image passes 2^31 - 1 bytes");
        return false;
    }
    return true;
}

void read_chunk(caddy_ctx* c, const unsigned char* files, const unsigned* offsets, long n_total, long n0, int nf, unsigned char* frames, int* status) {
    PngReadState* s = c->png_read;
    c->act.reset();
    ReadArgs a{};
    const size_t M = (size_t)s->max_frames;      // (sized for a full chunk whatever nf is, so the walk's count holds for every call)
    a.zbuf = (unsigned char*)c->act.alloc(M * s->zstride);
    a.sbuf = (unsigned char*)c->act.alloc(M * s->sstride);
    if (c->dry || c->act.overflow()) return;
    a.files = files; a.offsets = offsets; a.n_total = n_total; a.n0 = n0; a.nf = nf; a.H = s->H; a.W = s->W;
    a.stream = s->stream; a.capacity = s->capacity; a.zstride = s->zstride; a.sstride = s->sstride;
    a.crc_table = s->d_crc_table; a.frames = frames; a.status = status;
    hipLaunchKernelGGL(k_png_read, dim3((unsigned)nf), dim3(RD_THREADS), 0, c->stream, a);
    c->ck(hipGetLastError() == hipSuccess ? 0 : -1, "png decoder");
}

EvalKind read_kind(int max_frames, int H, int W) {
    return {CTX_PNG_READ, max_frames, H, W,
            [=](caddy_ctx* c) {
                PngReadState* s = new PngReadState();
                c->png_read = s;
                s->max_frames = max_frames; s->H = H; s->W = W;
                s->stream = rd_stream(H, W); s->capacity = rd_capacity(H, W);
                s->zstride = (s->capacity + 15) & ~15L; s->sstride = (s->stream + 15) & ~15L;
                s->d_crc_table = (unsigned*)c->persist.alloc(sizeof(unsigned) * (256 + 32));
            },
            [](caddy_ctx* c) { read_chunk(c, nullptr, nullptr, 0, 0, c->png_read->max_frames, nullptr, nullptr); },
            "caddy_png_read_workspace_bytes"};
}
unsigned rd_host_mulmod(unsigned a, unsigned b) {
    unsigned p = 0u;
    for (int i = 0; i < 32; i++) { if (a & (0x80000000u >> i)) p ^= b; b = (b & 1u) ? (b >> 1) ^ RD_POLY : b >> 1; }
    return p;
}

}  // namespace

void png_read_free(caddy_ctx* c) {
    if (!c || !c->png_read) return;
    delete c->png_read;
    c->png_read = nullptr;
}

extern "C" {
size_t caddy_png_read_workspace_bytes(int max_frames, int H, int W) {
    return rd_args_ok(max_frames, H, W) ? eval_workspace_bytes(read_kind(max_frames, H, W)) : 0;
}
caddy_ctx* caddy_png_read_ctx_create(int max_frames, int H, int W, void* workspace, size_t bytes) {
    if (!rd_args_ok(max_frames, H, W)) return nullptr;
    caddy_ctx* c = eval_ctx_create(read_kind(max_frames, H, W), workspace, bytes);
    if (!c) return nullptr;
    std::vector<unsigned> table(256 + 32);      // the table of png.hip: CRC-32 by byte, then x^(2^k) mod P
    for (unsigned i = 0; i < 256; i++) { unsigned v = i; for (int k = 0; k < 8; k++) v = (v & 1u) ? (v >> 1) ^ RD_POLY : v >> 1; table[i] = v; }
    unsigned p = 1u << 30;      // x^1
    table[256] = p;
    for (int k = 1; k < 32; k++) table[256 + k] = p = rd_host_mulmod(p, p);
    hipMemcpy(c->png_read->d_crc_table, table.data(), sizeof(unsigned) * table.size(), hipMemcpyHostToDevice);
    if (hipGetLastError() != hipSuccess) { set_error("caddy_png_read_ctx_create: uploading the table failed"); caddy_ctx_destroy(c); return nullptr; }
    return c;
}
int caddy_png_decode(caddy_ctx* c, const unsigned char* files, const unsigned* offsets, int n, unsigned char* frames_u8, int* status) {
    if (!ctx_needs(c, CTX_PNG_READ, "caddy_png_decode")) return -2;
    c->fail = false;
    if (!files || !offsets || !frames_u8 || !status) { set_error("null input"); return -2; }
    if (((uintptr_t)offsets & 3) || ((uintptr_t)status & 3)) { set_error("caddy_png_decode: offsets and status must be 4-byte aligned"); return -2; }
    if (n < 1) { set_error("caddy_png_decode: n must be positive"); return -2; }
    for_chunks(c, n, [&](long n0, int nf) {
        read_chunk(c, files, offsets, n, n0, nf, frames_u8, status);
        return !c->fail;
    });
    return finish(c, "caddy_png_read_workspace_bytes");
}
}
