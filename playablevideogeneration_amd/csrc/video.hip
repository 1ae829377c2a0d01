// Device-side MJPEG writer: baseline JPEG files encoded on the device from the uint8 interleaved frames the frame writer (frames.hip: caddy_frames_write) leaves there --
// only the encoded bytes are left to copy.  Takes the place of the reference's VideoSaver.save_video (utils/save_video_ffmpeg.py:172-198; play.py:192, interpolate.py:147),
// whose ffmpeg this project does not have; the container is written on the host (video_writer.py: write_avi).
//
// The file of one frame is, byte for byte, what libjpeg writes for quality q, 4:4:4 sampling, the Annex K Huffman tables and no restart markers (Pillow: Image.save(f,
// format = "JPEG", quality = q, subsampling = 0, optimize = False)).  Everything is integer arithmetic:
//   colour   jccolor.c, 16 fractional bits, FIX(x) = (int)(x * 65536 + 0.5):  Y = (FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16,
//            Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16) + 32767) >> 16,  Cr = (FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16
//   padding  the last column and row replicated up to the next multiple of 8; then - 128
//   DCT      jfdctint.c (CONST_BITS 13, PASS1_BITS 2): rows (<< 2, DESCALE(., 11)), then columns (DESCALE(., 2), DESCALE(., 15)); 8 times the DCT
//   quantise jcdctmgr.c: d = table[k] << 3, |c| -> (|c| + (d >> 1)) / d, the sign restored; stored in zigzag order
//   entropy  jchuff.c: DC difference against the previous MCU of the FRAME (0 at its first), run / size symbols, 0xF0 for every 16 zeros, EOB only when the block ends in zeros,
//            the scan padded with 1-bits to a byte, every 0xFF followed by 0x00
//
// Launches per chunk of at most max_frames frames, one thread per 8 x 8 block in (a) and (c), one workgroup per frame in (b) and (d):
//   (a) k_vid_dct    colour, padding, DCT, quantisation -> int16 coefficients; the block's AC bit count
//   (b) k_vid_scan   + the DC bits (they need the previous block's DC), exclusive scan of the bit counts of the frame; zeroes the words of the bit buffer the frame will use
//   (c) k_vid_emit   every block writes its codes, most significant bit first, at its bit offset: atomicOr on the first and the last word (shared with its neighbours), plain
//                    stores on the words it fills alone.  OR does not depend on the order, so a call is reproducible.
//   (d) k_vid_count  the 0xFF bytes of every chunk of 1024 scan bytes (the final padding applied), as a running sum per frame; the frame's file length
//   (e) k_vid_write  header + stuffed scan + EOI, compactly, frame after frame; the offsets
// Every buffer is sized from bounds no input can exceed: an AC symbol is at most 16 + 10 bits, a DC symbol 11 + 11, so a block is at most VID_BLOCK_BITS bits.
#include "eval_ctx.h"
#include "video.h"
#include <cstring>

namespace {

constexpr int VID_THREADS = 256, VID_WAVES = VID_THREADS / 64;
constexpr int VID_BLOCK_BITS = 63 * 26 + 22;
constexpr int VID_MAX_SIDE = 4096;        // 3 * 512 * 512 blocks of at most 1660 bits: every bit offset of a frame stays below 2^31
constexpr int VID_WRITE_BLOCKS = 32;      // workgroups per frame of the write launch (each walks the chunks c, c + 32, ...)
constexpr int VID_HEADER = 623;

// jpeg_natural_order: the row-major index of zigzag position k (a function, so that device code takes the value and never the address of a host table)
__host__ __device__ constexpr int zigzag(int k) {
    constexpr int t[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k];
}
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int FIX(double x) { return (int)(x * 65536 + 0.5); }

struct VidArgs {
    const unsigned char* frames;      // (nf, H, W, 3) of this chunk
    int nf, H, W, mcux, blocks;       // blocks per frame
    long wpf, cpf;
    const unsigned short* div;
    const unsigned* huff;
    const unsigned char* header;
    short* coef;                      // nf x blocks x 64, zigzag order
    unsigned* bits;                   // nf x blocks: (a) AC bits, (b) the block's first bit in the frame's scan
    unsigned* frame_bits;             // nf: bits of the scan
    unsigned* frame_len;              // nf: bytes of the file
    unsigned* words;                  // nf x wpf: the scan, big-endian words
    unsigned* chunk_ff;               // nf x cpf: 0xFF bytes in front of every chunk
    unsigned char* out; size_t capacity;
    unsigned* offsets; long n0;       // offsets of the whole call; this chunk's first frame
};

// one pass of jfdctint.c over d[0], d[S], .., d[7 S]
template <int S, bool FIRST> __device__ __forceinline__ void fdct_pass(int* d) {
    constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
    const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : (t10 + t11 + 2) >> 2;
    d[4 * S] = FIRST ? (t10 - t11) * 4 : (t10 - t11 + 2) >> 2;
    int z1 = (t12 + t13) * 4433;
    d[2 * S] = (z1 + t13 * 6270 + R) >> N;
    d[6 * S] = (z1 - t12 * 15137 + R) >> N;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    d[7 * S] = (a4 + z1 + z3 + R) >> N;
    d[5 * S] = (a5 + z2 + z4 + R) >> N;
    d[3 * S] = (a6 + z2 + z3 + R) >> N;
    d[S] = (a7 + z1 + z4 + R) >> N;
}

__device__ __forceinline__ int bit_length(unsigned a) { return a ? 32 - __builtin_clz(a) : 0; }

// (a) one thread per block: block i of a frame is component i % 3 of MCU i / 3
__global__ __launch_bounds__(VID_THREADS) void k_vid_dct(VidArgs a) {
    const long g = (long)blockIdx.x * VID_THREADS + threadIdx.x;
    if (g >= (long)a.nf * a.blocks) return;
    const int f = (int)(g / a.blocks), i = (int)(g - (long)f * a.blocks);
    const int mcu = i / 3, comp = i - 3 * mcu, my = mcu / a.mcux, mx = mcu - my * a.mcux;
    int kr, kg, kb, add;
    if (comp == 0) { kr = FIX(.299); kg = FIX(.587); kb = FIX(.114); add = 32768; }
    else if (comp == 1) { kr = -FIX(.16874); kg = -FIX(.33126); kb = FIX(.5); add = (128 << 16) + 32767; }
    else { kr = FIX(.5); kg = -FIX(.41869); kb = -FIX(.08131); add = (128 << 16) + 32767; }
    int d[64];
    const unsigned char* frame = a.frames + (long)f * a.H * a.W * 3;
    const bool inside = 8 * mx + 8 <= a.W;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = 8 * my + r < a.H ? 8 * my + r : a.H - 1;
        const unsigned char* row = frame + ((long)y * a.W + 8 * mx) * 3;
        if (inside && ((uintptr_t)row & 3) == 0) {      // 24 bytes as six words
            unsigned w[6];
#pragma unroll
            for (int j = 0; j < 6; j++) w[j] = ((const unsigned*)row)[j];
#pragma unroll
            for (int x = 0; x < 8; x++) {
                const int R = (w[(3 * x) >> 2] >> (8 * ((3 * x) & 3))) & 255, G = (w[(3 * x + 1) >> 2] >> (8 * ((3 * x + 1) & 3))) & 255, B = (w[(3 * x + 2) >> 2] >> (8 * ((3 * x + 2) & 3))) & 255;
                d[8 * r + x] = ((kr * R + kg * G + kb * B + add) >> 16) - 128;
            }
        } else {
#pragma unroll
            for (int x = 0; x < 8; x++) {
                const unsigned char* p = row + 3 * ((8 * mx + x < a.W ? 8 * mx + x : a.W - 1) - 8 * mx);
                d[8 * r + x] = ((kr * p[0] + kg * p[1] + kb * p[2] + add) >> 16) - 128;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 8; r++) fdct_pass<1, true>(d + 8 * r);
#pragma unroll
    for (int x = 0; x < 8; x++) fdct_pass<8, false>(d + x);
    const unsigned short* div = a.div + (comp ? 64 : 0);
    const unsigned* ac = a.huff + (comp ? 768 : 256);
    const unsigned zrl = ac[0xF0] >> 16, eob = ac[0] >> 16;
    unsigned packed[32], bits = 0;
    int run = 0;
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const int v = d[zigzag(k)];
        const unsigned dq = div[k], m = v < 0 ? (unsigned)-v : (unsigned)v;
        const unsigned q = (m + (dq >> 1)) / dq;
        const unsigned s = (unsigned)(v < 0 ? -(int)q : (int)q) & 0xFFFFu;
        if (k & 1) packed[k >> 1] |= s << 16; else packed[k >> 1] = s;
        if (k > 0) {
            if (q == 0) run++;
            else {
                const int nb = bit_length(q);
                bits += (unsigned)(run >> 4) * zrl + (ac[((run & 15) << 4) + nb] >> 16) + nb;
                run = 0;
            }
        }
    }
    if (run) bits += eob;
    u32x4* o = (u32x4*)(a.coef + g * 64);      // (128 bytes per block at a 256-byte aligned base)
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = u32x4{packed[4 * j], packed[4 * j + 1], packed[4 * j + 2], packed[4 * j + 3]};
    a.bits[g] = bits;
}

// the sum of v over the workgroup in every thread, and this thread's exclusive prefix (every thread of the workgroup calls it; lds holds VID_WAVES words)
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* lds, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const unsigned o = __shfl(inc, (lane - s) & 63); if (lane >= s) inc += o; }
    __syncthreads();      // (the words may still be read by the call before)
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned before = 0; total = 0;
#pragma unroll
    for (int k = 0; k < VID_WAVES; k++) { if (k < wave) before += lds[k]; total += lds[k]; }
    return before + inc - v;
}

// (b) one workgroup per frame
__global__ __launch_bounds__(VID_THREADS) void k_vid_scan(VidArgs a) {
    __shared__ unsigned lds[VID_WAVES];
    const int f = blockIdx.x;
    const short* coef = a.coef + (long)f * a.blocks * 64;
    unsigned* bits = a.bits + (long)f * a.blocks;
    unsigned carry = 0;
    for (int base = 0; base < a.blocks; base += VID_THREADS) {
        const int i = base + threadIdx.x;
        unsigned v = 0;
        if (i < a.blocks) {
            const int diff = coef[(long)i * 64] - (i >= 3 ? coef[(long)(i - 3) * 64] : 0);
            const int nb = bit_length((unsigned)(diff < 0 ? -diff : diff));
            v = bits[i] + (a.huff[(i % 3 ? 512 : 0) + nb] >> 16) + nb;
        }
        unsigned total;
        const unsigned at = carry + block_scan(v, lds, total);
        if (i < a.blocks) bits[i] = at;
        carry += total;
    }
    if (threadIdx.x == 0) a.frame_bits[f] = carry;
    unsigned* words = a.words + (long)f * a.wpf;
    const long used = ((long)carry + 31) / 32 + 1;      // (<= wpf: carry <= blocks * VID_BLOCK_BITS)
    for (long w = threadIdx.x; w < used && w < a.wpf; w += VID_THREADS) words[w] = 0u;
}

// (c) one thread per block
__global__ __launch_bounds__(VID_THREADS) void k_vid_emit(VidArgs a) {
    const long g = (long)blockIdx.x * VID_THREADS + threadIdx.x;
    if (g >= (long)a.nf * a.blocks) return;
    const int f = (int)(g / a.blocks), i = (int)(g - (long)f * a.blocks);
    const bool chroma = i % 3 != 0;
    const short* z = a.coef + g * 64;
    const unsigned* dc = a.huff + (chroma ? 512 : 0);
    const unsigned* ac = a.huff + (chroma ? 768 : 256);
    const unsigned pos = a.bits[g];
    unsigned* w = a.words + (long)f * a.wpf + (pos >> 5);
    unsigned* const end = a.words + (long)(f + 1) * a.wpf;
    unsigned long long acc = 0;
    int n = (int)(pos & 31);
    bool shared = n != 0;      // the first word is shared with the block in front unless this block starts it
    auto put = [&](unsigned code, int len) {      // len <= 27
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            const unsigned word = (unsigned)(acc >> n);
            if (w < end) { if (shared) atomicOr(w, word); else *w = word; }
            shared = false;
            w++;
            acc &= (1ull << n) - 1;
        }
    };
    const int diff = z[0] - (i >= 3 ? z[-192] : 0);
    {
        const int nb = bit_length((unsigned)(diff < 0 ? -diff : diff));
        const unsigned h = dc[nb];
        put(((h & 0xFFFFu) << nb) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1)), (int)(h >> 16) + nb);
    }
    const unsigned zrl = ac[0xF0], eob = ac[0];
    int run = 0;
    for (int k = 1; k < 64; k++) {
        const int v = z[k];
        if (v == 0) { run++; continue; }
        for (; run > 15; run -= 16) put(zrl & 0xFFFFu, (int)(zrl >> 16));
        const int nb = bit_length((unsigned)(v < 0 ? -v : v));
        const unsigned h = ac[(run << 4) + nb];
        put(((h & 0xFFFFu) << nb) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1)), (int)(h >> 16) + nb);
        run = 0;
    }
    if (run) put(eob & 0xFFFFu, (int)(eob >> 16));
    if (n > 0 && w < end) atomicOr(w, (unsigned)(acc << (32 - n)));
}

// word `idx` of a frame's scan with the 1-bits of the final padding in place; vb = how many of its bytes belong to the scan
__device__ __forceinline__ unsigned scan_word(const unsigned* words, long idx, unsigned total, int& vb) {
    const long nbytes = ((long)total + 7) >> 3;
    vb = nbytes - 4 * idx < 4 ? (int)(nbytes - 4 * idx) : 4;
    if (vb <= 0) { vb = 0; return 0u; }
    unsigned word = words[idx];
    if ((total & 7) && idx == (long)(total >> 5)) {
        const int s = (int)(total & 31), e = (s | 7) + 1;
        word |= (0xFFFFFFFFu >> s) & (e == 32 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> e));
    }
    return word;
}
__device__ __forceinline__ unsigned count_ff(unsigned word, int vb) {
    unsigned c = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) c += (b < vb && ((word >> (24 - 8 * b)) & 255u) == 255u) ? 1u : 0u;
    return c;
}

// (d) one workgroup per frame
__global__ __launch_bounds__(VID_THREADS) void k_vid_count(VidArgs a) {
    __shared__ unsigned lds[VID_WAVES];
    const int f = blockIdx.x;
    const unsigned total = a.frame_bits[f];
    const unsigned* words = a.words + (long)f * a.wpf;
    const long nbytes = ((long)total + 7) >> 3, nw = (nbytes + 3) >> 2, chunks = (nw + VID_THREADS - 1) / VID_THREADS;
    unsigned running = 0;
    for (long c = 0; c < chunks && c < a.cpf; c++) {
        int vb;
        const unsigned word = scan_word(words, c * VID_THREADS + threadIdx.x, total, vb);
        unsigned sum;
        block_scan(count_ff(word, vb), lds, sum);
        if (threadIdx.x == 0) a.chunk_ff[(long)f * a.cpf + c] = running;
        running += sum;
    }
    if (threadIdx.x == 0) a.frame_len[f] = (unsigned)(VID_HEADER + nbytes + running + 2);
}

// (e) grid (VID_WRITE_BLOCKS, nf)
__global__ __launch_bounds__(VID_THREADS) void k_vid_write(VidArgs a) {
    __shared__ unsigned lds[VID_WAVES];
    const int f = blockIdx.y;
    unsigned before = 0, sum;
    for (int gidx = threadIdx.x; gidx < f; gidx += VID_THREADS) before += a.frame_len[gidx];
    block_scan(before, lds, sum);
    const size_t base = (size_t)(a.n0 > 0 ? a.offsets[a.n0] : 0u) + sum;
    const unsigned total = a.frame_bits[f], len = a.frame_len[f];
    if (blockIdx.x == 0) {
        for (int j = threadIdx.x; j < VID_HEADER; j += VID_THREADS) if (base + j < a.capacity) a.out[base + j] = a.header[j];
        if (threadIdx.x < 2 && base + len - 2 + threadIdx.x < a.capacity) a.out[base + len - 2 + threadIdx.x] = threadIdx.x ? 0xD9 : 0xFF;
        if (threadIdx.x == 0) {
            if (f > 0 || a.n0 == 0) a.offsets[a.n0 + f] = (unsigned)base;      // (the first offset of a later chunk is the total the chunk before wrote)
            if (f == a.nf - 1) a.offsets[a.n0 + a.nf] = (unsigned)(base + len);
        }
    }
    const unsigned* words = a.words + (long)f * a.wpf;
    const long nbytes = ((long)total + 7) >> 3, nw = (nbytes + 3) >> 2, chunks = (nw + VID_THREADS - 1) / VID_THREADS;
    for (long c = blockIdx.x; c < chunks && c < a.cpf; c += gridDim.x) {
        const long idx = c * VID_THREADS + threadIdx.x;
        int vb;
        const unsigned word = scan_word(words, idx, total, vb);
        size_t pos = base + VID_HEADER + 4 * idx + a.chunk_ff[(long)f * a.cpf + c] + block_scan(count_ff(word, vb), lds, sum);
        for (int b = 0; b < vb; b++) {
            const unsigned char byte = (unsigned char)(word >> (24 - 8 * b));
            if (pos < a.capacity) a.out[pos] = byte;
            pos++;
            if (byte == 0xFF) { if (pos < a.capacity) a.out[pos] = 0; pos++; }
        }
    }
}

// ---- host: tables, header, the context kind ------------------------------------------------------------------------------------------------------------------------
const unsigned char BASE_LUMA[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const unsigned char BASE_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                       99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3: the 16 code counts, then the symbols in code order
const unsigned char DC_LUMA[] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char DC_CHROMA[] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char AC_LUMA[] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d,
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1,
    0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39,
    0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
    0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const unsigned char AC_CHROMA[] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77,
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09,
    0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38,
    0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
struct HuffSpec { int id; const unsigned char* t; int symbols; };      // id: class << 4 | table
const HuffSpec HUFF[4] = {{0x00, DC_LUMA, 12}, {0x10, AC_LUMA, 162}, {0x01, DC_CHROMA, 12}, {0x11, AC_CHROMA, 162}};
static_assert(sizeof(AC_LUMA) == 16 + 162 && sizeof(AC_CHROMA) == 16 + 162, "Annex K AC tables");

void segment(std::vector<unsigned char>& o, int marker, const std::vector<unsigned char>& payload) {
    o.push_back(0xFF); o.push_back((unsigned char)marker);
    o.push_back((unsigned char)((payload.size() + 2) >> 8)); o.push_back((unsigned char)((payload.size() + 2) & 255));
    o.insert(o.end(), payload.begin(), payload.end());
}
// the tables of a context: quantisation (jpeg_quality_scaling + jpeg_add_quant_table with force_baseline), the header, the derived Huffman tables (jpeg_make_c_derived_tbl)
void video_tables(VideoState* s, std::vector<unsigned short>& div, std::vector<unsigned>& huff) {
    const int q = s->quality, scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 64; k++) s->qt[64 * t + k] = (unsigned char)std::min(std::max(((t ? BASE_CHROMA : BASE_LUMA)[k] * scale + 50) / 100, 1), 255);
    div.resize(128);
    for (int t = 0; t < 2; t++) for (int k = 0; k < 64; k++) div[64 * t + k] = (unsigned short)(s->qt[64 * t + zigzag(k)] << 3);
    huff.assign(1024, 0u);
    for (int t = 0; t < 4; t++) {
        unsigned code = 0; int k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int j = 0; j < HUFF[t].t[len - 1]; j++, k++, code++) huff[256 * t + HUFF[t].t[16 + k]] = code | ((unsigned)len << 16);
            code <<= 1;
        }
    }
    std::vector<unsigned char>& h = s->header;
    h = {0xFF, 0xD8};
    segment(h, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; t++) {
        std::vector<unsigned char> p = {(unsigned char)t};
        for (int k = 0; k < 64; k++) p.push_back(s->qt[64 * t + zigzag(k)]);
        segment(h, 0xDB, p);
    }
    segment(h, 0xC0, {8, (unsigned char)(s->H >> 8), (unsigned char)(s->H & 255), (unsigned char)(s->W >> 8), (unsigned char)(s->W & 255), 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 4; t++) {
        std::vector<unsigned char> p = {(unsigned char)HUFF[t].id};
        p.insert(p.end(), HUFF[t].t, HUFF[t].t + 16 + HUFF[t].symbols);
        segment(h, 0xC4, p);
    }
    segment(h, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
}

long frame_blocks(int H, int W) { return 3L * ((H + 7) / 8) * ((W + 7) / 8); }
size_t frame_scan_bytes(int H, int W) { return (size_t)((frame_blocks(H, W) * VID_BLOCK_BITS + 7) / 8); }      // before stuffing

bool video_args_ok(int max_frames, int H, int W, int quality) {
    if (max_frames < 1 || H < 1 || W < 1) { set_error("caddy_video: max_frames, height and width must be positive"); return false; }
    if (H > VID_MAX_SIDE || W > VID_MAX_SIDE) { set_error("caddy_video: frames larger than 4096 x 4096"); return false; }
    if (quality < 1 || quality > 100) { set_error("caddy_video: quality must be in 1..100"); return false; }
    return true;
}

// one chunk of nf frames: the buffers of the activation arena, then the five launches (a dry context only counts the bytes)
void video_chunk(caddy_ctx* c, const unsigned char* frames, long n0, int nf, unsigned char* out, size_t capacity, unsigned* offsets) {
    VideoState* s = c->vid;
    c->act.reset();
    VidArgs a{};
    const size_t M = (size_t)s->max_frames;      // (sized for a full chunk whatever nf is, so the walk's count holds for every call)
    a.coef = (short*)c->act.alloc(sizeof(short) * 64 * M * s->blocks);
    a.bits = (unsigned*)c->act.alloc(sizeof(unsigned) * M * s->blocks);
    a.frame_bits = (unsigned*)c->act.alloc(sizeof(unsigned) * M);
    a.frame_len = (unsigned*)c->act.alloc(sizeof(unsigned) * M);
    a.words = (unsigned*)c->act.alloc(sizeof(unsigned) * M * s->wpf);
    a.chunk_ff = (unsigned*)c->act.alloc(sizeof(unsigned) * M * s->cpf);
    if (c->dry || c->act.overflow()) return;
    a.frames = frames; a.nf = nf; a.H = s->H; a.W = s->W; a.mcux = s->mcux; a.blocks = s->blocks; a.wpf = s->wpf; a.cpf = s->cpf;
    a.div = s->d_div; a.huff = s->d_huff; a.header = s->d_header;
    a.out = out; a.capacity = capacity; a.offsets = offsets; a.n0 = n0;
    const unsigned per_block = (unsigned)(((long)nf * s->blocks + VID_THREADS - 1) / VID_THREADS);
    hipLaunchKernelGGL(k_vid_dct, dim3(per_block), dim3(VID_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_vid_scan, dim3((unsigned)nf), dim3(VID_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_vid_emit, dim3(per_block), dim3(VID_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_vid_count, dim3((unsigned)nf), dim3(VID_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_vid_write, dim3((unsigned)std::min<long>(s->cpf, VID_WRITE_BLOCKS), (unsigned)nf), dim3(VID_THREADS), 0, c->stream, a);
    c->ck(hipGetLastError() == hipSuccess ? 0 : -1, "video encoder");
}

EvalKind video_kind(int max_frames, int H, int W, int quality) {
    return {CTX_VIDEO, max_frames, H, W,
            [=](caddy_ctx* c) {
                VideoState* s = new VideoState();
                c->vid = s;
                s->max_frames = max_frames; s->H = H; s->W = W; s->quality = quality;
                s->mcux = (W + 7) / 8; s->mcuy = (H + 7) / 8; s->blocks = (int)frame_blocks(H, W);
                s->wpf = ((long)s->blocks * VID_BLOCK_BITS + 31) / 32 + 1;
                s->cpf = (s->wpf + VID_THREADS - 1) / VID_THREADS;
                s->d_div = (unsigned short*)c->persist.alloc(sizeof(unsigned short) * 128);
                s->d_huff = (unsigned*)c->persist.alloc(sizeof(unsigned) * 1024);
                s->d_header = (unsigned char*)c->persist.alloc(VID_HEADER);
            },
            [](caddy_ctx* c) { video_chunk(c, nullptr, 0, c->vid->max_frames, nullptr, 0, nullptr); },
            "caddy_video_workspace_bytes"};
}

}  // namespace

void video_free(caddy_ctx* c) {
    if (!c || !c->vid) return;
    delete c->vid;
    c->vid = nullptr;
}

extern "C" {
size_t caddy_video_workspace_bytes(int max_frames, int H, int W) {
    return video_args_ok(max_frames, H, W, 50) ? eval_workspace_bytes(video_kind(max_frames, H, W, 50)) : 0;
}
caddy_ctx* caddy_video_ctx_create(int max_frames, int H, int W, int quality, void* workspace, size_t bytes) {
    if (!video_args_ok(max_frames, H, W, quality)) return nullptr;
    caddy_ctx* c = eval_ctx_create(video_kind(max_frames, H, W, quality), workspace, bytes);
    if (!c) return nullptr;
    VideoState* s = c->vid;
    std::vector<unsigned short> div; std::vector<unsigned> huff;
    video_tables(s, div, huff);
    if ((int)s->header.size() != VID_HEADER) { set_error("caddy_video_ctx_create: the header is not 623 bytes"); caddy_ctx_destroy(c); return nullptr; }
    hipMemcpy(s->d_div, div.data(), sizeof(unsigned short) * div.size(), hipMemcpyHostToDevice);
    hipMemcpy(s->d_huff, huff.data(), sizeof(unsigned) * huff.size(), hipMemcpyHostToDevice);
    hipMemcpy(s->d_header, s->header.data(), s->header.size(), hipMemcpyHostToDevice);
    if (hipGetLastError() != hipSuccess) { set_error("caddy_video_ctx_create: uploading the tables failed"); caddy_ctx_destroy(c); return nullptr; }
    return c;
}
size_t caddy_video_stream_bound(int n, int H, int W) {
    if (!video_args_ok(n, H, W, 50)) return 0;
    return (size_t)n * (VID_HEADER + 2 * frame_scan_bytes(H, W) + 2);
}
int caddy_video_encode(caddy_ctx* c, const unsigned char* frames_u8, int n, unsigned char* out_stream, size_t out_capacity, unsigned* offsets) {
    if (!ctx_needs(c, CTX_VIDEO, "caddy_video_encode")) return -2;
    c->fail = false;
    if (!frames_u8 || !out_stream || !offsets) { set_error("null input"); return -2; }
    if ((uintptr_t)offsets & 3) { set_error("caddy_video_encode: offsets must be 4-byte aligned"); return -2; }
    if (n < 1) { set_error("caddy_video_encode: n must be positive"); return -2; }
    const VideoState* s = c->vid;
    const size_t bound = (size_t)n * (VID_HEADER + 2 * frame_scan_bytes(s->H, s->W) + 2);
    if (bound > 0xFFFFFFFFull) { set_error("caddy_video_encode: the stream of " + std::to_string(n) + " frames may pass 2^32 bytes (the offsets are 32-bit words): encode fewer frames per call"); return -2; }
    if (out_capacity < bound) {
        set_error("caddy_video_encode: an output capacity of " + std::to_string(out_capacity) + " bytes, " + std::to_string(n) + " frames may need " + std::to_string(bound) + " (caddy_video_stream_bound)");
        return -2;
    }
    const size_t frame = (size_t)s->H * s->W * 3;
    for_chunks(c, n, [&](long n0, int nf) {
        video_chunk(c, frames_u8 + n0 * frame, n0, nf, out_stream, out_capacity, offsets);
        return !c->fail;
    });
    return finish(c, "caddy_video_workspace_bytes");
}
int caddy_video_tables_get(caddy_ctx* c, unsigned char* qtables128, unsigned char* header, int* header_bytes) {
    if (!ctx_needs(c, CTX_VIDEO, "caddy_video_tables_get")) return -2;
    const VideoState* s = c->vid;
    if (qtables128) memcpy(qtables128, s->qt, 128);
    if (header) memcpy(header, s->header.data(), s->header.size());
    if (header_bytes) *header_bytes = (int)s->header.size();
    return 0;
}
}
