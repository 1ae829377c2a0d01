// Device-side JPEG reader: complete baseline JPEG files (SOF0, 8 bits, three components, 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan) parsed, Huffman-decoded, inverse-transformed,
// upsampled and colour-converted on the device into the uint8 interleaved frames the frame pipeline (frames.hip: caddy_frames_observations) reads -- only the compressed bytes
// cross the bus.  Takes the place of the host's PIL Image.open per frame in a DataLoader worker for .jpg frame folders (dataset/video.py:120-157) and reads back what
// caddy_video_encode (video.hip) leaves: the files back to back and n + 1 offsets.  The contract is the bytes: what Pillow decodes for every file an encoder wrote, and the
// integer arithmetic of include/caddy_hip.h for everything else.  A sibling of png_read.hip, same shape.
//
// Three launches per chunk of at most max_frames images:
//   (a) k_jpeg_entropy   grid (nf), one workgroup of ONE wave per image.  Every lane walks the marker segments (the same few bytes: one broadcast load); the wave copies the
//                        quantisation tables and builds the Huffman look-up tables in LDS (a first-level table indexed by the next 9 bits, the canonical walk for longer
//                        codes); the wave finds the markers of the scan in 64 pieces (count, prefix, write), checks their number and order, and then ONE LANE DECODES ONE
//                        RESTART INTERVAL, 64 at a time: each lane has its own bit window over its own byte range, handles the stuffing in its refill, and writes the
//                        quantised coefficients as int16, in natural order, into the image's slice (zeroed by the wave before, so only non-zero values are written).  A file
//                        without restart markers is one interval on one lane.  The verdict goes to status[], the sampling and the tables in natural order to the image's meta.
//   (b) k_jpeg_idct      block-parallel: eight lanes a block, 32 blocks a workgroup.  Dequantise (value * table on 32-bit words: the product does not fit 16 bits, which is
//                        why (a) leaves quantised values), jidctint.c columns then rows through LDS, + 128, clamp, one 8-byte store per block row into uint8 component planes.
//   (c) k_jpeg_colour    pixel-parallel: four pixels of a row a lane.  Fancy upsampling at the chroma plane's TRUE size (indices clamped into it, which is the replication the
//                        formulas state), YCbCr -> RGB, three dword stores where the frame address allows, bytes otherwise.  A refused image gets its zero frame here.
// Not built: a parallel split of one stream (a file without restart markers keeps one lane busy).
//
// Safety (the bytes come from outside): every read of the blob is bounded by the end of that file (itself clamped to offsets[n]), every read of a lane by the end of its
// interval; past it the bit reader yields zeros and the first symbol that used one ends the image; every write is bounded by the image's own slice or frame.  Every loop
// states below what it consumes or produces and the bound known before it starts.
#include "eval_ctx.h"
#include "jpeg_read.h"
#include <cstring>

namespace {

constexpr int JR_THREADS = 64;                 // one wave: __syncthreads() is the wave's own wait
constexpr int JR_FAST = 9;                     // bits of the first-level decoding tables
constexpr int JR_META = 512;                   // bytes of an image's meta
constexpr int IDCT_BLOCKS = 32;                // blocks of a k_jpeg_idct workgroup, eight lanes each
constexpr unsigned NONE = 0xFFFFFFFFu;
enum { MODE_444 = 0, MODE_422 = 1, MODE_420 = 2 };

struct Meta { int mode; int pad; unsigned short q[3][64]; };      // what (b) and (c) need of an accepted image: the sampling; the tables in natural order

struct JpegArgs {
    const unsigned char* files; const unsigned* offsets; long n_total, n0;
    int nf, H, W, bw, bh;
    long cstride, pstride;
    short* coef;                      // nf x cstride: per component plane (bw bh 64 each) the blocks in raster order, 64 quantised values in natural order
    unsigned char* planes;            // nf x pstride: per component plane 8 bh rows; the row stride is 8 x the component's block columns
    unsigned* marks;                  // nf x (bw bh): where the marker code bytes of the scan stand
    unsigned char* meta;              // nf x JR_META
    unsigned char* frames;            // (n_total, H, W, 3)
    int* status;                      // n_total
};

struct JTables {     // LDS of one image; Huffman table t = 4 class + id
    unsigned short fast[8][1 << JR_FAST];        // symbol << 4 | length of the code the index starts with; 0: longer than JR_FAST, or none
    unsigned char sym[8][256];                   // symbols ordered by (length, symbol)
    unsigned maxcode[8][17];                     // one past the last code of every length
    unsigned short mincode[8][17], valptr[8][17];
    unsigned char cnt[8][17];
    unsigned char qt[4][64];                     // zigzag order, as the file has them
    unsigned char zz[64];
    unsigned red[JR_THREADS], red2[JR_THREADS];
    unsigned flag;
};

struct Frame {       // what the markers in front of the scan said (the same in every lane)
    int mode, mcux, mcuy, ri;
    int hs0, vs0;
    int td[3], ta[3];
    unsigned scan;                    // where the entropy bytes start
};

__device__ __forceinline__ unsigned be16(const unsigned char* p) { return ((unsigned)p[0] << 8) | p[1]; }

// ---- (a) the markers in front of the scan: -> status ---------------------------------------------------------------------------------------------------------------------------
__device__ int parse(const JpegArgs& a, const unsigned char* file, unsigned flen, JTables& L, Frame& F, Meta* meta) {
    const unsigned lane = threadIdx.x;
    for (unsigned i = 0; i < 2u && i < flen; i++) if (file[i] != (i ? 0xD8 : 0xFF)) return CADDY_JPEG_NOT_JPEG;      // (at most 2 bytes, below flen)
    if (flen < 2u) return CADDY_JPEG_TRUNCATED;
    unsigned pos = 2u, qdef = 0u, hdef = 0u;
    bool sof = false, jfif = false, adobe = false;
    int transform = 0, ids[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
    F.ri = 0;
    // every pass consumes one marker of at least 2 bytes, and with a segment at least 4, of [pos, flen): at most flen / 2 passes
    for (;;) {
        if (pos >= flen) return CADDY_JPEG_TRUNCATED;
        if (file[pos] != 0xFF) return CADDY_JPEG_BAD_TABLE;
        while (pos < flen && file[pos] == 0xFF) pos++;      // fill bytes: consumes one byte of [pos, flen) a step
        if (pos >= flen) return CADDY_JPEG_TRUNCATED;
        const unsigned m = file[pos++];
        if (m == 0xD9) return CADDY_JPEG_TRUNCATED;      // the file ends before a scan
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) return CADDY_JPEG_BAD_TABLE;
        if (flen - pos < 2u) return CADDY_JPEG_TRUNCATED;
        const unsigned len = be16(file + pos);
        if (len < 2u) return CADDY_JPEG_BAD_TABLE;
        if (len > flen - pos) return CADDY_JPEG_TRUNCATED;
        const unsigned char* seg = file + pos + 2;      // seg[0, n) lies inside the file
        const unsigned n = len - 2u;
        pos += len;
        if (m == 0xC0) {
            if (sof || n < 6u || n != 6u + 3u * seg[5]) return CADDY_JPEG_BAD_TABLE;
            if (seg[0] != 8 || seg[5] != 3 || be16(seg + 1) == 0u) return CADDY_JPEG_UNSUPPORTED;
            for (int c = 0; c < 3; c++) { ids[c] = seg[6 + 3 * c]; tq[c] = seg[8 + 3 * c]; if (tq[c] > 3) return CADDY_JPEG_BAD_TABLE; }
            const unsigned s0 = seg[7];
            if (seg[10] != 0x11 || seg[13] != 0x11 || (s0 != 0x11 && s0 != 0x21 && s0 != 0x22)) return CADDY_JPEG_UNSUPPORTED;
            if (be16(seg + 1) != (unsigned)a.H || be16(seg + 3) != (unsigned)a.W) return CADDY_JPEG_GEOMETRY;
            F.mode = s0 == 0x11 ? MODE_444 : s0 == 0x21 ? MODE_422 : MODE_420;
            F.hs0 = (int)(s0 >> 4); F.vs0 = (int)(s0 & 15u);
            F.mcux = (a.W + 8 * F.hs0 - 1) / (8 * F.hs0); F.mcuy = (a.H + 8 * F.vs0 - 1) / (8 * F.vs0);
            sof = true;
        } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4) || m == 0xDC || m == 0xDE || m == 0xDF) {
            return CADDY_JPEG_UNSUPPORTED;      // another process, arithmetic conditioning, DNL, hierarchical
        } else if (m == 0xDB) {
            // every pass consumes the 65 bytes of one table of seg[o, n)
            for (unsigned o = 0; o < n; o += 65u) {
                const unsigned pq = seg[o] >> 4, id = seg[o] & 15u;
                if (pq == 1u) return CADDY_JPEG_UNSUPPORTED;
                if (pq > 1u || id > 3u || n - o < 65u) return CADDY_JPEG_BAD_TABLE;
                __syncthreads();
                if (lane < 64u) L.qt[id][lane] = seg[o + 1u + lane];
                qdef |= 1u << id;
            }
        } else if (m == 0xC4) {
            // every pass consumes the 17 + total bytes of one table of seg[o, n)
            for (unsigned o = 0; o < n;) {
                const unsigned tc = seg[o] >> 4, id = seg[o] & 15u;
                if (tc > 1u || id > 3u || n - o < 17u) return CADDY_JPEG_BAD_TABLE;
                const unsigned t = 4u * tc + id;
                unsigned total = 0u;
                int left = 1;
                for (unsigned l = 1; l <= 16u; l++) {      // (16 steps)
                    const unsigned c = seg[o + l];
                    total += c; left = (left << 1) - (int)c;
                    if (left < 0) return CADDY_JPEG_BAD_TABLE;
                }
                if (total > 256u || n - o - 17u < total) return CADDY_JPEG_BAD_TABLE;
                __syncthreads();
                if (lane == 0) {
                    unsigned code = 0u, at = 0u;
                    for (unsigned l = 1; l <= 16u; l++) {
                        const unsigned c = seg[o + l];
                        L.cnt[t][l] = (unsigned char)c; L.mincode[t][l] = (unsigned short)code; L.valptr[t][l] = (unsigned short)at;
                        code += c; at += c;
                        L.maxcode[t][l] = code;
                        code <<= 1;
                    }
                }
                for (unsigned i = lane; i < total; i += JR_THREADS) L.sym[t][i] = seg[o + 17u + i];      // produces sym[0, total), total <= 256
                for (unsigned i = lane; i < (1u << JR_FAST); i += JR_THREADS) L.fast[t][i] = 0;
                __syncthreads();
                for (unsigned k = lane; k < total; k += JR_THREADS) {
                    unsigned l = 1u;
                    while (l < 16u && k >= (unsigned)L.valptr[t][l] + L.cnt[t][l]) l++;      // (at most 15 steps; k < total lies in some length's range)
                    if (l > (unsigned)JR_FAST) continue;
                    const unsigned code = L.mincode[t][l] + (k - L.valptr[t][l]), e = ((unsigned)L.sym[t][k] << 4) | l;
                    // (a code space that is not over-subscribed: code < 2^l, so the entries lie below 2^JR_FAST and those of two symbols are disjoint)
                    for (unsigned x = code << (JR_FAST - l); x < ((code + 1u) << (JR_FAST - l)); x++) L.fast[t][x] = (unsigned short)e;
                }
                hdef |= 1u << t;
                o += 17u + total;
            }
        } else if (m == 0xDD) {
            if (n != 2u) return CADDY_JPEG_BAD_TABLE;
            F.ri = (int)be16(seg);
        } else if (m == 0xE0) {
            if (n >= 5u && seg[0] == 'J' && seg[1] == 'F' && seg[2] == 'I' && seg[3] == 'F' && seg[4] == 0) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12u && seg[0] == 'A' && seg[1] == 'd' && seg[2] == 'o' && seg[3] == 'b' && seg[4] == 'e') { adobe = true; transform = seg[11]; }
        } else if (m == 0xDA) {
            if (!sof || n < 1u || n != 4u + 2u * seg[0]) return CADDY_JPEG_BAD_TABLE;
            if (seg[0] != 3) return CADDY_JPEG_UNSUPPORTED;
            for (int c = 0; c < 3; c++) {
                if (seg[1 + 2 * c] != ids[c]) return CADDY_JPEG_UNSUPPORTED;
                F.td[c] = seg[2 + 2 * c] >> 4; F.ta[c] = seg[2 + 2 * c] & 15;
                if (F.td[c] > 3 || F.ta[c] > 3) return CADDY_JPEG_BAD_TABLE;
            }
            if (seg[7] != 0 || seg[8] != 63 || seg[9] != 0) return CADDY_JPEG_UNSUPPORTED;
            if (!jfif && (adobe ? transform != 1 : (ids[0] == 'R' && ids[1] == 'G' && ids[2] == 'B'))) return CADDY_JPEG_UNSUPPORTED;
            for (int c = 0; c < 3; c++)
                if (!((qdef >> tq[c]) & 1u) || !((hdef >> F.td[c]) & 1u) || !((hdef >> (4 + F.ta[c])) & 1u)) return CADDY_JPEG_BAD_TABLE;
            __syncthreads();
            meta->mode = F.mode;      // (every lane the same word)
            for (unsigned i = lane; i < 192u; i += JR_THREADS) meta->q[i >> 6][L.zz[i & 63u]] = L.qt[tq[i >> 6]][i & 63u];
            F.scan = pos;
            return CADDY_JPEG_OK;
        }
        // APPn, COM and whatever else carries a length: skipped
    }
}

// ---- the bit reader of one lane over file[pos, end): MSB first; 0xFF (0xFF)* 0x00 is one 0xFF; zeros past the end, and `fake` counts them ---------------------------------
struct JBits {
    const unsigned char* p; unsigned pos, end, acc; int cnt, fake;
    // -> at least 25 bits; every pass consumes at least one byte of [pos, end) or appends eight zeros: at most 4 passes
    __device__ __forceinline__ void fill() {
        while (cnt <= 24) {
            unsigned byte = 0u;
            if (pos < end) {
                byte = p[pos++];
                if (byte == 0xFFu) {
                    unsigned q = pos;
                    while (q < end && p[q] == 0xFFu) q++;      // reads one byte of [pos, end) a step
                    if (q < end && p[q] == 0u) pos = q + 1u;
                    else { pos = end; byte = 0u; fake += 8; }      // (an interval never ends in 0xFF: its end lies in front of the marker's)
                }
            } else fake += 8;
            acc |= byte << (24 - cnt); cnt += 8;
        }
    }
    __device__ __forceinline__ unsigned peek16() const { return acc >> 16; }
    __device__ __forceinline__ void drop(int k) { acc <<= k; cnt -= k; }
    __device__ __forceinline__ unsigned take(int k) { const unsigned v = k ? acc >> (32 - k) : 0u; drop(k); return v; }      // k <= 16
    __device__ __forceinline__ bool over() const { return cnt < fake; }
    __device__ __forceinline__ bool leftover() const { return cnt - fake >= 8 || pos < end; }
};

// one symbol (at least 16 bits in the window): -1 where no code matches; consumes at least one bit otherwise
__device__ __forceinline__ int huff(JBits& b, const JTables& L, int t) {
    const unsigned v = b.peek16(), e = L.fast[t][v >> (16 - JR_FAST)];
    if (e) { b.drop((int)(e & 15u)); return (int)(e >> 4); }
    for (int l = JR_FAST + 1; l <= 16; l++) {      // (7 steps)
        const unsigned c = v >> (16 - l);
        if (c < L.maxcode[t][l] && c >= L.mincode[t][l]) { b.drop(l); return L.sym[t][L.valptr[t][l] + (c - L.mincode[t][l])]; }      // (the index is below the table's total)
    }
    return -1;
}
__device__ __forceinline__ int extend(unsigned v, int s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// one block: the quantised values into blk[0, 64) (zero before), natural order; -> status
__device__ __forceinline__ int block(JBits& b, const JTables& L, int td, int ta, int& pred, short* blk) {
    b.fill();
    int s = huff(b, L, td);
    if (s < 0) return b.cnt - b.fake < 16 ? -1 : CADDY_JPEG_BAD_CODE;      // (no code among 16 bits of which some lie past the end: the end decides)
    if (b.over()) return -1;
    if (s > 11) return CADDY_JPEG_BAD_COEFFICIENT;
    b.fill();
    pred += extend(b.take(s), s);
    if (b.over()) return -1;
    if (pred < -2048 || pred > 2047) return CADDY_JPEG_BAD_COEFFICIENT;
    blk[0] = (short)pred;
    // every pass consumes at least one bit and either ends the block or moves k up: at most 63 passes
    for (int k = 1; k < 64;) {
        b.fill();
        const int rs = huff(b, L, 4 + ta);
        if (rs < 0) return b.cnt - b.fake < 16 ? -1 : CADDY_JPEG_BAD_CODE;
        if (b.over()) return -1;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;
            if (k + 15 > 63) return CADDY_JPEG_BAD_COEFFICIENT;
            k += 16;
            continue;
        }
        if (s > 10) return CADDY_JPEG_BAD_COEFFICIENT;
        k += r;
        if (k > 63) return CADDY_JPEG_BAD_COEFFICIENT;
        b.fill();
        const int v = extend(b.take(s), s);
        if (b.over()) return -1;
        blk[L.zz[k]] = (short)v;      // zz[k] < 64: inside the block
        k++;
    }
    return CADDY_JPEG_OK;
}

__global__ __launch_bounds__(JR_THREADS) void k_jpeg_entropy(JpegArgs a) {
    __shared__ JTables L;
    const unsigned lane = threadIdx.x;
    const int f = blockIdx.x;
    const long g = a.n0 + f;
    const unsigned char zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    L.zz[lane] = zigzag[lane];
    if (lane == 0) L.flag = 0u;
    __syncthreads();
    // the file: [o0, o1) clamped to the blob [0, offsets[n]); offsets out of order give an empty or shortened file
    const unsigned total = a.offsets[a.n_total];
    const unsigned o0 = a.offsets[g] < total ? a.offsets[g] : total, o1 = a.offsets[g + 1] < total ? a.offsets[g + 1] : total;
    const unsigned flen = o1 > o0 ? o1 - o0 : 0u;
    const unsigned char* file = a.files + o0;
    short* coef = a.coef + (long)f * a.cstride;
    unsigned* marks = a.marks + (long)f * a.bw * a.bh;
    Meta* meta = (Meta*)(a.meta + (long)f * JR_META);
    Frame F{};
    int st = parse(a, file, flen, L, F, meta);
    __syncthreads();
    if (st != CADDY_JPEG_OK) { if (lane == 0) a.status[g] = st; return; }

    const long mcus = (long)F.mcux * F.mcuy;                                   // <= bw bh: the marks and the coefficient planes hold them
    const long ni = F.ri > 0 ? (mcus + F.ri - 1) / F.ri : 1;                   // intervals; the scan must hold ni markers: ni - 1 RSTm and the one behind it
    // the image's coefficients, zero: produces [0, cstride) of its own slice, 16 bytes a lane and step
    {
        int4* z = (int4*)coef;
        const int4 zero = {0, 0, 0, 0};
        for (long i = lane; i < a.cstride / 8; i += JR_THREADS) z[i] = zero;
    }
    // the markers of the scan, in 64 pieces of file[scan, flen): a marker is a byte other than 0x00 and 0xFF behind a 0xFF that lies in the scan.  Counted, then placed.
    const unsigned long long sbytes = flen - F.scan, piece = (sbytes + JR_THREADS - 1u) / JR_THREADS;
    const unsigned q0 = F.scan + (unsigned)(lane * piece < sbytes ? lane * piece : sbytes), q1 = F.scan + (unsigned)((lane + 1u) * piece < sbytes ? (lane + 1u) * piece : sbytes);
    unsigned mine = 0u, first_other = NONE;
    for (unsigned q = q0 > F.scan ? q0 : F.scan + 1u; q < q1; q++) {      // reads file[q - 1] and file[q], both in [scan, flen)
        const unsigned v = file[q];
        if (v != 0u && v != 0xFFu && file[q - 1] == 0xFFu) { if (first_other == NONE && (v < 0xD0u || v > 0xD7u)) first_other = mine; mine++; }
    }
    L.red[lane] = mine;
    __syncthreads();
    unsigned base = 0u;
    for (unsigned i = 0; i < lane; i++) base += L.red[i];      // (the markers in front of this lane's piece)
    L.red2[lane] = first_other == NONE ? NONE : base + first_other;
    __syncthreads();
    unsigned term = NONE;      // the index of the first marker that is no RSTm: the one behind the scan
    for (int i = 0; i < JR_THREADS; i++) term = L.red2[i] < term ? L.red2[i] : term;
    if (term == NONE) st = CADDY_JPEG_TRUNCATED;
    else if ((long)term != ni - 1) st = CADDY_JPEG_BAD_RESTART;
    if (st == CADDY_JPEG_OK) {
        unsigned at = base, wrong = 0u;
        for (unsigned q = q0 > F.scan ? q0 : F.scan + 1u; q < q1 && at <= term; q++) {      // the same walk; produces marks[at], at <= term < ni <= bw bh
            const unsigned v = file[q];
            if (v != 0u && v != 0xFFu && file[q - 1] == 0xFFu) { if (at < term && v != 0xD0u + (at & 7u)) wrong = 1u; marks[at++] = q; }
        }
        if (wrong) atomicOr(&L.flag, 1u);
    }
    __syncthreads();
    if (st == CADDY_JPEG_OK && L.flag) st = CADDY_JPEG_BAD_RESTART;
    if (st == CADDY_JPEG_OK) { const unsigned v = file[marks[term]]; if (v != 0xD9u) st = v == 0xDCu ? CADDY_JPEG_UNSUPPORTED : CADDY_JPEG_BAD_SCAN; }
    if (st != CADDY_JPEG_OK) { if (lane == 0) a.status[g] = st; return; }

    // one lane decodes one interval, 64 at a time; the first interval that fails decides
    const int cbw0 = F.mcux * F.hs0;
    const long plane = (long)a.bw * a.bh * 64;
    for (long i0 = 0; i0 < ni; i0 += JR_THREADS) {
        const long i = i0 + lane;
        int verdict = CADDY_JPEG_OK;
        if (i < ni) {
            const bool last = i == ni - 1;
            JBits b{};
            b.p = file;
            b.pos = i == 0 ? F.scan : marks[i - 1] + 1u;
            b.end = marks[i] - 1u;                                                    // the marker's 0xFF: at or behind pos
            while (b.end > b.pos && file[b.end - 1u] == 0xFFu) b.end--;               // fill bytes in front of it: one byte of [pos, end) a step
            long m = F.ri > 0 ? i * F.ri : 0;
            const long m1 = F.ri > 0 && m + F.ri < mcus ? m + F.ri : mcus;
            int pred[3] = {0, 0, 0};
            int mx = (int)(m % F.mcux), my = (int)(m / F.mcux);
            // every MCU consumes at least 2 bits a block; m1 - m MCUs, each inside the image's MCU grid
            for (; m < m1 && verdict == CADDY_JPEG_OK; m++) {
                for (int v = 0; v < F.vs0 && verdict == CADDY_JPEG_OK; v++)
                    for (int h = 0; h < F.hs0 && verdict == CADDY_JPEG_OK; h++)      // block (my vs + v, mx hs + h) of mcuy vs x cbw0 <= bh x bw: inside the luma plane
                        verdict = block(b, L, F.td[0], F.ta[0], pred[0], coef + ((long)(my * F.vs0 + v) * cbw0 + (mx * F.hs0 + h)) * 64);
                for (int c = 1; c < 3 && verdict == CADDY_JPEG_OK; c++)              // block (my, mx) of mcuy x mcux: inside the component's plane
                    verdict = block(b, L, F.td[c], F.ta[c], pred[c], coef + c * plane + ((long)my * F.mcux + mx) * 64);
                if (++mx == F.mcux) { mx = 0; my++; }
            }
            if (verdict < 0) verdict = last ? CADDY_JPEG_TRUNCATED : CADDY_JPEG_BAD_RESTART;      // a symbol used bits past the interval's end
            else if (verdict == CADDY_JPEG_OK && b.leftover()) verdict = last ? CADDY_JPEG_BAD_SCAN : CADDY_JPEG_BAD_RESTART;
        }
        L.red[lane] = (unsigned)verdict;
        __syncthreads();
        for (int k = JR_THREADS - 1; k >= 0; k--) if (L.red[k] != CADDY_JPEG_OK) st = (int)L.red[k];      // (the first one that failed)
        __syncthreads();
        if (st != CADDY_JPEG_OK) break;
    }
    if (lane == 0) a.status[g] = st;
}

// ---- (b) IDCT: the quantised blocks -> uint8 component planes -----------------------------------------------------------------------------------------------------------------
// one pass of jidctint.c over eight values; on unsigned words, so that the products wrap
__device__ __forceinline__ void idct8(const unsigned* in, int shift, int* out) {
    unsigned z2 = in[2], z3 = in[6];
    unsigned z1 = (z2 + z3) * 4433u;
    unsigned tmp2 = z1 - z3 * 15137u, tmp3 = z1 + z2 * 6270u;
    z2 = in[0]; z3 = in[4];
    unsigned tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
    const unsigned tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    unsigned z4 = tmp1 + tmp3;
    const unsigned z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 *= 0u - 7373u; z2 *= 0u - 20995u; z3 *= 0u - 16069u; z4 *= 0u - 3196u;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const unsigned round = 1u << (shift - 1);
    out[0] = (int)(tmp10 + tmp3 + round) >> shift; out[7] = (int)(tmp10 - tmp3 + round) >> shift;
    out[1] = (int)(tmp11 + tmp2 + round) >> shift; out[6] = (int)(tmp11 - tmp2 + round) >> shift;
    out[2] = (int)(tmp12 + tmp1 + round) >> shift; out[5] = (int)(tmp12 - tmp1 + round) >> shift;
    out[3] = (int)(tmp13 + tmp0 + round) >> shift; out[4] = (int)(tmp13 - tmp0 + round) >> shift;
}
__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v); }

// the block grid of component c of an image of the sampling `mode`: columns and rows of 8 x 8 blocks
__device__ __forceinline__ void comp_blocks(int mode, int c, int H, int W, int& cbw, int& cbh) {
    const int hs = mode == MODE_444 ? 1 : 2, vs = mode == MODE_420 ? 2 : 1;
    const int mcux = (W + 8 * hs - 1) / (8 * hs), mcuy = (H + 8 * vs - 1) / (8 * vs);
    cbw = c ? mcux : mcux * hs; cbh = c ? mcuy : mcuy * vs;
}

__global__ __launch_bounds__(8 * IDCT_BLOCKS) void k_jpeg_idct(JpegArgs a) {
    __shared__ int ws[IDCT_BLOCKS][64];
    const int f = blockIdx.y, j = threadIdx.x & 7, slot = threadIdx.x >> 3;
    if (a.status[a.n0 + f] != CADDY_JPEG_OK) return;      // (the whole workgroup: one image)
    const Meta* meta = (const Meta*)(a.meta + (long)f * JR_META);
    int cbw0, cbh0, cbw1, cbh1;
    comp_blocks(meta->mode, 0, a.H, a.W, cbw0, cbh0);
    comp_blocks(meta->mode, 1, a.H, a.W, cbw1, cbh1);
    const long n0 = (long)cbw0 * cbh0, n1 = (long)cbw1 * cbh1;
    long blk = (long)blockIdx.x * IDCT_BLOCKS + slot;
    const bool active = blk < n0 + 2 * n1;      // block blk of the image's n0 + 2 n1, each inside its component's bw x bh plane
    const int c = blk < n0 ? 0 : blk < n0 + n1 ? 1 : 2;
    if (c) blk -= n0 + (c - 1) * n1;
    const int cbw = c ? cbw1 : cbw0;
    const long plane = (long)a.bw * a.bh * 64;
    if (active) {
        const short* src = a.coef + (long)f * a.cstride + c * plane + blk * 64;
        unsigned in[8];
        int out[8];
#pragma unroll
        for (int r = 0; r < 8; r++) in[r] = (unsigned)(int)src[8 * r + j] * (unsigned)meta->q[c][8 * r + j];      // column j, dequantised
        idct8(in, 11, out);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[slot][8 * r + j] = out[r];
    }
    __syncthreads();
    if (active) {
        unsigned in[8];
        int out[8];
#pragma unroll
        for (int x = 0; x < 8; x++) in[x] = (unsigned)ws[slot][8 * j + x];      // row j
        idct8(in, 18, out);
        const int by = (int)(blk / cbw), bx = (int)(blk % cbw);
        int2 px;
        px.x = (int)(clamp255(out[0] + 128) | (clamp255(out[1] + 128) << 8) | (clamp255(out[2] + 128) << 16) | (clamp255(out[3] + 128) << 24));
        px.y = (int)(clamp255(out[4] + 128) | (clamp255(out[5] + 128) << 8) | (clamp255(out[6] + 128) << 16) | (clamp255(out[7] + 128) << 24));
        // row 8 by + j < 8 bh of the plane, columns [8 bx, 8 bx + 8) of its 8 cbw <= 8 bw: an aligned 8-byte store inside the image's plane
        *(int2*)(a.planes + (long)f * a.pstride + c * plane + ((long)(8 * by + j) * cbw + bx) * 8) = px;
    }
}

// ---- (c) upsample + colour: the planes -> (H, W, 3) ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_jpeg_colour(JpegArgs a) {
    const int f = blockIdx.y, H = a.H, W = a.W, w4 = (W + 3) >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)H * w4) return;
    const int y = (int)(t / w4), x0 = 4 * (int)(t % w4);
    unsigned char* dst = a.frames + ((a.n0 + f) * (long)H * W + (long)y * W + x0) * 3;      // pixels [x0, min(x0 + 4, W)) of row y < H
    unsigned rgb[3] = {0u, 0u, 0u};      // the 12 bytes
    if (a.status[a.n0 + f] == CADDY_JPEG_OK) {
        const Meta* meta = (const Meta*)(a.meta + (long)f * JR_META);
        const int mode = meta->mode;
        int cbw0, cbh0, cbw1, cbh1;
        comp_blocks(mode, 0, H, W, cbw0, cbh0);
        comp_blocks(mode, 1, H, W, cbw1, cbh1);
        const long plane = (long)a.bw * a.bh * 64;
        const unsigned char* py = a.planes + (long)f * a.pstride;
        const unsigned char* pc[2] = {py + plane, py + 2 * plane};
        // the plane rows are 8 cbw bytes from an aligned base: the four bytes at x0 (a multiple of 4 below 8 cbw) are one aligned word of the row
        const unsigned yy = *(const unsigned*)(py + (long)y * 8 * cbw0 + x0);
        int cv[2][4];
        if (mode == MODE_444) {
            for (int c = 0; c < 2; c++) {
                const unsigned v = *(const unsigned*)(pc[c] + (long)y * 8 * cbw1 + x0);
                for (int k = 0; k < 4; k++) cv[c][k] = (int)((v >> (8 * k)) & 255u);
            }
        } else {
            // the chroma plane's true size; every index is clamped into it
            const int cw = (W + 1) >> 1, ch = mode == MODE_420 ? (H + 1) >> 1 : H, i0 = x0 >> 1;
            const int r = mode == MODE_420 ? y >> 1 : y;
            int r2 = r;
            if (mode == MODE_420) r2 = (y & 1) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
            const int even = mode == MODE_420 ? 8 : 1, odd = mode == MODE_420 ? 7 : 2, sh = mode == MODE_420 ? 4 : 2;
            for (int c = 0; c < 2; c++) {
                int v[4];
                for (int k = 0; k < 4; k++) {
                    int i = i0 - 1 + k;
                    i = i < 0 ? 0 : i > cw - 1 ? cw - 1 : i;
                    const int s = pc[c][(long)r * 8 * cbw1 + i];
                    v[k] = mode == MODE_420 ? 3 * s + pc[c][(long)r2 * 8 * cbw1 + i] : s;
                }
                cv[c][0] = (3 * v[1] + v[0] + even) >> sh; cv[c][1] = (3 * v[1] + v[2] + odd) >> sh;
                cv[c][2] = (3 * v[2] + v[1] + even) >> sh; cv[c][3] = (3 * v[2] + v[3] + odd) >> sh;
            }
        }
        unsigned char out[12];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int Y = (int)((yy >> (8 * k)) & 255u), cb = cv[0][k] - 128, cr = cv[1][k] - 128;
            out[3 * k] = (unsigned char)clamp255(Y + ((91881 * cr + 32768) >> 16));
            out[3 * k + 1] = (unsigned char)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            out[3 * k + 2] = (unsigned char)clamp255(Y + ((116130 * cb + 32768) >> 16));
        }
#pragma unroll
        for (int w = 0; w < 3; w++) rgb[w] = out[4 * w] | ((unsigned)out[4 * w + 1] << 8) | ((unsigned)out[4 * w + 2] << 16) | ((unsigned)out[4 * w + 3] << 24);
    }
    if (x0 + 4 <= W && !((uintptr_t)dst & 3)) {
        unsigned* d = (unsigned*)dst;
        d[0] = rgb[0]; d[1] = rgb[1]; d[2] = rgb[2];
    } else {
        const int nb = 3 * (W - x0 < 4 ? W - x0 : 4);
        for (int k = 0; k < nb; k++) dst[k] = (unsigned char)(rgb[k >> 2] >> (8 * (k & 3)));      // the bytes of the pixels below W only
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
bool jr_args_ok(int max_frames, int H, int W) {
    if (max_frames < 1 || max_frames > 65535) { set_error("caddy_jpeg_read: max_frames must be 1..65535"); return false; }
    if (H < 1 || W < 1 || H > 4096 || W > 4096) { set_error("caddy_jpeg_read: height and width must be 1..4096"); return false; }
    return true;
}

void read_chunk(caddy_ctx* c, const unsigned char* files, const unsigned* offsets, long n_total, long n0, int nf, unsigned char* frames, int* status) {
    JpegReadState* s = c->jpeg_read;
    c->act.reset();
    JpegArgs a{};
    const size_t M = (size_t)s->max_frames;      // (sized for a full chunk whatever nf is, so the walk's count holds for every call)
    a.coef = (short*)c->act.alloc(M * s->cstride * sizeof(short));
    a.planes = (unsigned char*)c->act.alloc(M * s->pstride);
    a.marks = (unsigned*)c->act.alloc(M * (size_t)s->bw * s->bh * sizeof(unsigned));
    a.meta = (unsigned char*)c->act.alloc(M * JR_META);
    if (c->dry || c->act.overflow()) return;
    a.files = files; a.offsets = offsets; a.n_total = n_total; a.n0 = n0; a.nf = nf; a.H = s->H; a.W = s->W; a.bw = s->bw; a.bh = s->bh;
    a.cstride = s->cstride; a.pstride = s->pstride; a.frames = frames; a.status = status;
    hipLaunchKernelGGL(k_jpeg_entropy, dim3((unsigned)nf), dim3(JR_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)((3L * s->bw * s->bh + IDCT_BLOCKS - 1) / IDCT_BLOCKS), (unsigned)nf), dim3(8 * IDCT_BLOCKS), 0, c->stream, a);
    hipLaunchKernelGGL(k_jpeg_colour, dim3((unsigned)(((long)s->H * ((s->W + 3) / 4) + 255) / 256), (unsigned)nf), dim3(256), 0, c->stream, a);
    c->ck(hipGetLastError() == hipSuccess ? 0 : -1, "jpeg decoder");
}

EvalKind read_kind(int max_frames, int H, int W) {
    return {CTX_JPEG_READ, max_frames, H, W,
            [=](caddy_ctx* c) {
                JpegReadState* s = new JpegReadState();
                c->jpeg_read = s;
                s->max_frames = max_frames; s->H = H; s->W = W;
                s->bw = 2 * ((W + 15) / 16); s->bh = 2 * ((H + 15) / 16);
                s->cstride = 3L * s->bw * s->bh * 64; s->pstride = 3L * s->bw * s->bh * 64;
            },
            [](caddy_ctx* c) { read_chunk(c, nullptr, nullptr, 0, 0, c->jpeg_read->max_frames, nullptr, nullptr); },
            "caddy_jpeg_read_workspace_bytes"};
}

}  // namespace

void jpeg_read_free(caddy_ctx* c) {
    if (!c || !c->jpeg_read) return;
    delete c->jpeg_read;
    c->jpeg_read = nullptr;
}

extern "C" {
size_t caddy_jpeg_read_workspace_bytes(int max_frames, int H, int W) {
    return jr_args_ok(max_frames, H, W) ? eval_workspace_bytes(read_kind(max_frames, H, W)) : 0;
}
caddy_ctx* caddy_jpeg_read_ctx_create(int max_frames, int H, int W, void* workspace, size_t bytes) {
    if (!jr_args_ok(max_frames, H, W)) return nullptr;
    return eval_ctx_create(read_kind(max_frames, H, W), workspace, bytes);
}
int caddy_jpeg_decode(caddy_ctx* c, const unsigned char* files, const unsigned* offsets, int n, unsigned char* frames_u8, int* status) {
    if (!ctx_needs(c, CTX_JPEG_READ, "caddy_jpeg_decode")) return -2;
    c->fail = false;
    if (!files || !offsets || !frames_u8 || !status) { set_error("null input"); return -2; }
    if (((uintptr_t)offsets & 3) || ((uintptr_t)status & 3)) { set_error("caddy_jpeg_decode: offsets and status must be 4-byte aligned"); return -2; }
    if (n < 1) { set_error("caddy_jpeg_decode: n must be positive"); return -2; }
    for_chunks(c, n, [&](long n0, int nf) {
        read_chunk(c, files, offsets, n, n0, nf, frames_u8, status);
        return !c->fail;
    });
    return finish(c, "caddy_jpeg_read_workspace_bytes");
}
}
