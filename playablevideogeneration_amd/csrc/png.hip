// Device-side PNG writer: complete PNG files (8-bit RGB, no interlace, one IDAT) filtered, deflated and framed on the device from the uint8 interleaved frames the frame writer
// (frames.hip: caddy_frames_write) and the sheets (sheets.hip) leave there -- only the compressed bytes are left to copy.  Takes the place of the host's PIL Image.save(f,
// format = "PNG") behind every frame the drivers save (the dataset folders, play / interpolate, the evaluator's example sheets).  The files are not Pillow's bytes; the contract
// is the PNG and deflate specifications (include/caddy_hip.h states the arithmetic).
//
// Launches per chunk of at most max_frames images:
//   (a) k_png_filter   grid (H, nf): one workgroup per row.  The five candidate rows from the raw rows y and y - 1, the sums of |int8| met through LDS atomicAdd, the chosen row
//                      written with its type byte into the image's filtered stream
//   (b) k_png_deflate  grid (nb, nf): one workgroup per block of PNG_BLOCK stream bytes, held in LDS.  Runs of equal bytes by compare-with-predecessor and two scans (the start
//                      and the end of every run), the literal / length and distance histograms, length-limited code lengths, canonical codes, the code-length code of the
//                      dynamic header; the shortest of stored / fixed / dynamic is put together in LDS (LSB first, atomicOr on zeroed words: order independent) and staged;
//                      the block's byte length, the raw CRC-32 of the bytes as staged, and its two Adler sums
//   (c) k_png_finish   one workgroup per image: the exclusive scan of the block lengths, Adler-32 and CRC-32 combined over the blocks, the file length
//   (d) k_png_write    grid (min(nb, PNG_WRITE_BLOCKS), nf): signature, IHDR, IDAT (zlib header, the staged blocks compactly, Adler-32), its CRC, IEND; the offsets
// Every block but an image's last ends on a byte boundary (an empty stored block behind it where it does not already), so (c) is a plain prefix sum of bytes.  No block goes out
// longer than stored, which is what bounds the output on noise: an image is at most 63 + S + 5 nb bytes.
#include "eval_ctx.h"
#include "png.h"
#include <cstring>

namespace {

constexpr int PNG_THREADS = 256, PNG_WAVES = PNG_THREADS / 64;
constexpr int PNG_BLOCK = 16384;               // stream bytes per deflate block (<= 65535: a stored block holds it)
constexpr int PNG_PER = PNG_BLOCK / PNG_THREADS;      // consecutive stream bytes per thread
constexpr int PNG_STORED = 5;                  // a stored block's header: one byte of BFINAL / BTYPE and padding, LEN, NLEN
constexpr int PNG_OUT_WORDS = (PNG_BLOCK + PNG_STORED + 3) / 4 + 1;
constexpr int PNG_CSTRIDE = PNG_OUT_WORDS * 4;
constexpr int PNG_WRITE_BLOCKS = 32;
constexpr int PNG_HEAD = 41, PNG_FRAME = 63;   // bytes in front of the zlib stream; bytes of a file besides its deflate blocks
constexpr int PNG_ADAPTIVE = 5;
constexpr unsigned PNG_POLY = 0xEDB88320u, ADLER = 65521u;
constexpr int NLL = 286, ND = 30, NCL = 19, MAXN = 288;

struct PngArgs {
    const unsigned char* frames;      // (nf, H, W, 3) of this chunk
    int nf, H, W, mode;
    long stream, nb, fstride;
    const unsigned char* head;
    const unsigned* crc_table;        // 256 + 32 words
    unsigned char* filt;              // nf x fstride
    unsigned char* comp;              // nf x nb x PNG_CSTRIDE
    unsigned* blen;                   // nf x nb: bytes of the block as staged; (c) leaves the exclusive prefix in boff
    unsigned* boff;
    unsigned* bcrc;                   // raw CRC (register 0 at the start, no final complement) of the staged bytes
    unsigned* badl;                   // 2 x nf x nb: sum of the bytes mod 65521; sum of (len - i) byte[i] mod 65521
    unsigned* image;                  // 4 x nf: deflate bytes, Adler-32, CRC-32, file length
    unsigned char* out; size_t capacity;
    unsigned* offsets; long n0;
};

// ---- (a) filter ----------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ unsigned filtered(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (unsigned)(x - pred) & 255u;
}
__device__ __forceinline__ unsigned magnitude(unsigned v) { return v < 128u ? v : 256u - v; }

__global__ __launch_bounds__(PNG_THREADS) void k_png_filter(PngArgs a) {
    __shared__ unsigned sums[5];
    const int y = blockIdx.x, f = blockIdx.y, rb = 3 * a.W;
    const unsigned char* cur = a.frames + ((long)f * a.H + y) * rb;
    const unsigned char* up = y > 0 ? cur - rb : cur;      // (read only where y > 0)
    unsigned char* dst = a.filt + (long)f * a.fstride + (long)y * (rb + 1);
    int type = a.mode;
    if (a.mode == PNG_ADAPTIVE) {
        if (threadIdx.x < 5) sums[threadIdx.x] = 0u;
        __syncthreads();
        unsigned s[5] = {0u, 0u, 0u, 0u, 0u};
        for (int i = threadIdx.x; i < rb; i += PNG_THREADS) {
            const int x = cur[i], l = i >= 3 ? cur[i - 3] : 0, u = y > 0 ? up[i] : 0, ul = (i >= 3 && y > 0) ? up[i - 3] : 0;
#pragma unroll
            for (int t = 0; t < 5; t++) s[t] += magnitude(filtered(t, x, l, u, ul));
        }
#pragma unroll
        for (int t = 0; t < 5; t++) atomicAdd(&sums[t], s[t]);
        __syncthreads();
        type = 0;
        for (int t = 1; t < 5; t++) if (sums[t] < sums[type]) type = t;
    }
    if (threadIdx.x == 0) dst[0] = (unsigned char)type;
    for (int i = threadIdx.x; i < rb; i += PNG_THREADS) {
        const int x = cur[i], l = i >= 3 ? cur[i - 3] : 0, u = y > 0 ? up[i] : 0, ul = (i >= 3 && y > 0) ? up[i - 3] : 0;
        dst[1 + i] = (unsigned char)filtered(type, x, l, u, ul);
    }
}

// ---- (b) deflate ---------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned bit_reverse(unsigned code, int len) {
    unsigned r = 0;
    for (int i = 0; i < len; i++) { r = (r << 1) | (code & 1u); code >>= 1; }
    return r;
}
// the length symbol of a match of len 3..258: (symbol, extra bits, their value)
__device__ __forceinline__ void length_symbol(int len, int& sym, int& eb, unsigned& ev) {
    if (len == 258) { sym = 285; eb = 0; ev = 0u; return; }
    const int l = len - 3;
    if (l < 8) { sym = 257 + l; eb = 0; ev = 0u; return; }
    eb = (31 - __builtin_clz((unsigned)l)) - 2;
    sym = 257 + 4 * (eb + 1) + ((l >> eb) & 3);
    ev = (unsigned)l & ((1u << eb) - 1u);
}
__device__ __forceinline__ int length_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }
// the fixed code of RFC 1951 3.2.6 (bit-reversed for LSB-first output) and its length
__device__ __forceinline__ void fixed_code(int sym, unsigned& code, int& len) {
    unsigned c;
    if (sym < 144) { c = 0x30u + sym; len = 8; }
    else if (sym < 256) { c = 0x190u + (sym - 144); len = 9; }
    else if (sym < 280) { c = (unsigned)(sym - 256); len = 7; }
    else { c = 0xC0u + (sym - 280); len = 8; }
    code = bit_reverse(c, len);
}
__device__ __forceinline__ int fixed_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

// Code lengths of at most maxlen for the n <= MAXN symbols of freq (LDS); every thread of the workgroup calls it.  Symbols are ranked by (frequency, index) in parallel; thread 0
// then runs the in-place minimum-redundancy construction of Moffat and Katajainen on the sorted frequencies, folds the lengths above maxlen into maxlen and repairs the Kraft sum
// (the shortest codes go to the most frequent symbols).  Fewer than two symbols of non-zero frequency: symbol 0 (and 1) is given frequency 1 first, as zlib's build_tree does, so
// every tree has at least two codes.
__device__ void build_lengths(unsigned* freq, int n, int maxlen, unsigned char* lens, unsigned* key, unsigned* work, int* counts) {
    const int t = threadIdx.x;
    if (t == 0) {
        int used = 0;
        for (int i = 0; i < n; i++) used += freq[i] != 0u;
        for (int i = 0; used < 2 && i < n; i++) if (freq[i] == 0u) { freq[i] = 1u; used++; }
        counts[33] = used;
    }
    __syncthreads();
    for (int i = t; i < n; i += PNG_THREADS) {
        lens[i] = 0;
        const unsigned mine = freq[i];
        if (mine == 0u) continue;
        int rank = 0;
        for (int j = 0; j < n; j++) { const unsigned o = freq[j]; rank += (o != 0u && (o < mine || (o == mine && j < i))) ? 1 : 0; }
        key[rank] = (unsigned)i;
        work[rank] = mine;
    }
    __syncthreads();
    if (t == 0) {
        const int m = counts[33];
        unsigned* A = work;
        if (m == 2) { A[0] = 1u; A[1] = 1u; }
        else {
            A[0] += A[1];
            int root = 0, leaf = 2;
            for (int next = 1; next < m - 1; next++) {
                if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (unsigned)next; } else A[next] = A[leaf++];
                if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (unsigned)next; } else A[next] += A[leaf++];
            }
            A[m - 2] = 0u;
            for (int next = m - 3; next >= 0; next--) A[next] = A[A[next]] + 1u;
            int avbl = 1, used = 0, dpth = 0, root2 = m - 2, next = m - 1;
            while (avbl > 0) {
                while (root2 >= 0 && (int)A[root2] == dpth) { used++; root2--; }
                while (avbl > used) { A[next--] = (unsigned)dpth; avbl--; }
                avbl = 2 * used; dpth++; used = 0;
            }
        }
        for (int i = 0; i <= 32; i++) counts[i] = 0;
        for (int i = 0; i < m; i++) counts[A[i] > 32u ? 32 : (int)A[i]]++;
        for (int i = maxlen + 1; i <= 32; i++) { counts[maxlen] += counts[i]; counts[i] = 0; }
        unsigned total = 0;
        for (int i = maxlen; i > 0; i--) total += (unsigned)counts[i] << (maxlen - i);
        while (total > (1u << maxlen)) {
            counts[maxlen]--;
            for (int i = maxlen - 1; i > 0; i--) if (counts[i]) { counts[i]--; counts[i + 1] += 2; break; }
            total--;
        }
        int j = m;
        for (int i = 1; i <= maxlen; i++) for (int l = counts[i]; l > 0; l--) lens[key[--j]] = (unsigned char)i;
    }
    __syncthreads();
}
// canonical codes of lens (thread 0), bit-reversed for LSB-first output
__device__ void canonical_codes(const unsigned char* lens, int n, int maxlen, unsigned short* codes) {
    unsigned next[17], count[17];
    for (int i = 0; i <= maxlen; i++) count[i] = 0u;
    for (int i = 0; i < n; i++) count[lens[i]]++;
    count[0] = 0u;
    unsigned code = 0u;
    next[0] = 0u;
    for (int i = 1; i <= maxlen; i++) { code = (code + count[i - 1]) << 1; next[i] = code; }
    for (int i = 0; i < n; i++) codes[i] = lens[i] ? (unsigned short)bit_reverse(next[lens[i]]++, lens[i]) : (unsigned short)0;
}

struct BitWriter {      // LSB first into zeroed LDS words; OR does not depend on the order
    unsigned* words; unsigned long long acc; int n; unsigned w;
    __device__ __forceinline__ void start(unsigned* out, unsigned bit) { words = out; w = bit >> 5; n = (int)(bit & 31u); acc = 0ull; }
    __device__ __forceinline__ void put(unsigned v, int len) {      // len <= 16
        acc |= (unsigned long long)v << n;
        n += len;
        if (n >= 32) { if (w < (unsigned)PNG_OUT_WORDS) atomicOr(&words[w], (unsigned)acc); w++; acc >>= 32; n -= 32; }
    }
    __device__ __forceinline__ void flush() { if (n > 0 && w < (unsigned)PNG_OUT_WORDS) atomicOr(&words[w], (unsigned)acc); }
};

// the tokens of the stream bytes [p0, p1) of a block: run [s, e] of equal bytes is one literal, then matches of min(258, what is left) while at least 3 are left, then literals.
// S = the start of the run p0 lies in, E = the end of the run p1 - 1 lies in.  lit(byte) / match(len) are called in stream order.
template <class Lit, class Match> __device__ __forceinline__ void for_tokens(const unsigned char* in, int p0, int p1, int S, int E, Lit lit, Match match) {
    int p = p0, s = S;
    while (p < p1) {
        const unsigned char v = in[p];
        int e = p;
        while (e + 1 < p1 && in[e + 1] == v) e++;
        const int last = e;      // the last position of the run inside [p0, p1)
        if (e + 1 == p1) e = E;
        const int R = e - s + 1;
        for (int q = p; q <= last; q++) {
            const int k = q - s;
            if (k == 0) { lit(v); continue; }
            const int j = k - 1, c = j / 258, o = j - 258 * c, left = R - 1 - 258 * c, cl = left < 258 ? left : 258;
            if (cl < 3) lit(v);
            else if (o == 0) match(cl);
        }
        p = last + 1;
        s = p;
    }
}

// v * x^(8 n) mod P in the reflected representation (xp: x^(2^k) mod P for k = 0..31, cyclic)
__device__ __forceinline__ unsigned mulmod(unsigned a, unsigned b) {
    unsigned p = 0u;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ PNG_POLY : b >> 1;
    }
    return p;
}
__device__ __forceinline__ unsigned shift_bytes(unsigned v, unsigned long long nbytes, const unsigned* xp) {
    unsigned long long n = nbytes;
    for (int k = 3; n; k++, n >>= 1) if (n & 1ull) v = mulmod(xp[k & 31], v);
    return v;
}
// XOR / sum of v over the workgroup, in every thread (lds: PNG_WAVES words)
__device__ __forceinline__ unsigned block_xor(unsigned v, unsigned* lds) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v ^= __shfl_xor(v, s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned r = 0u;
#pragma unroll
    for (int k = 0; k < PNG_WAVES; k++) r ^= lds[k];
    return r;
}
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* lds, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const unsigned o = __shfl(inc, (lane - s) & 63); if (lane >= s) inc += o; }
    __syncthreads();
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned before = 0u; total = 0u;
#pragma unroll
    for (int k = 0; k < PNG_WAVES; k++) { if (k < wave) before += lds[k]; total += lds[k]; }
    return before + inc - v;
}

__global__ __launch_bounds__(PNG_THREADS) void k_png_deflate(PngArgs a) {
    __shared__ unsigned in_w[PNG_BLOCK / 4];
    __shared__ unsigned out_w[PNG_OUT_WORDS];
    __shared__ unsigned crc_t[256 + 32];
    __shared__ int scan_s[PNG_THREADS], scan_e[PNG_THREADS];
    __shared__ unsigned f_ll[MAXN], f_d[32], f_cl[32], key[MAXN], work[MAXN];
    __shared__ unsigned char l_ll[MAXN], l_d[32], l_cl[32];
    __shared__ unsigned short c_ll[MAXN], c_d[32], c_cl[32];
    __shared__ unsigned short cl_tok[MAXN + 32];      // code-length symbols of the dynamic header: symbol | extra value << 8
    __shared__ int counts[34];
    __shared__ unsigned sh[8];      // 0 dynamic token bits, 1 fixed bits, 2 dynamic header bits, 3 number of cl tokens, 4 hlit, 5 hclen, 6 matches, 7 hdist
    __shared__ unsigned red[PNG_WAVES];
    unsigned char* in = (unsigned char*)in_w;
    unsigned char* out = (unsigned char*)out_w;
    const int t = threadIdx.x, f = blockIdx.y;
    const long blk = blockIdx.x;
    const long at = blk * PNG_BLOCK;
    const int len = (int)(a.stream - at < PNG_BLOCK ? a.stream - at : PNG_BLOCK);
    const bool final_block = blk == a.nb - 1;
    const unsigned char* src = a.filt + (long)f * a.fstride + at;      // (fstride and PNG_BLOCK are multiples of 16 at a 256-byte aligned base: word loads)
    for (int i = t; i < PNG_BLOCK / 4; i += PNG_THREADS) in_w[i] = 4 * i < len ? ((const unsigned*)src)[i] : 0u;      // (the stream's buffer is padded to fstride)
    for (int i = t; i < PNG_OUT_WORDS; i += PNG_THREADS) out_w[i] = 0u;
    for (int i = t; i < 256 + 32; i += PNG_THREADS) crc_t[i] = a.crc_table[i];
    for (int i = t; i < MAXN; i += PNG_THREADS) f_ll[i] = 0u;
    if (t < 32) { f_d[t] = 0u; f_cl[t] = 0u; }
    if (t < 8) sh[t] = 0u;
    __syncthreads();

    // runs: the last start and the first end of a run inside this thread's bytes, then the start / end that reach it from its neighbours
    const int p0 = t * PNG_PER < len ? t * PNG_PER : len, p1 = (t + 1) * PNG_PER < len ? (t + 1) * PNG_PER : len;
    int last_start = -1, first_end = PNG_BLOCK;
    unsigned as = 0u, aw = 0u;      // Adler: sum of the bytes, sum of (p1 - i) byte[i]
    for (int p = p0; p < p1; p++) {
        const unsigned v = in[p];
        if (p == 0 || in[p - 1] != v) last_start = p;
        if (first_end == PNG_BLOCK && (p == len - 1 || in[p + 1] != v)) first_end = p;
        as += v; aw += (unsigned)(p1 - p) * v;
    }
    scan_s[t] = last_start; scan_e[t] = first_end;
    __syncthreads();
    for (int d = 1; d < PNG_THREADS; d <<= 1) {
        const int s = t >= d ? scan_s[t - d] : -1, e = t + d < PNG_THREADS ? scan_e[t + d] : PNG_BLOCK;
        __syncthreads();
        if (s > scan_s[t]) scan_s[t] = s;
        if (e < scan_e[t]) scan_e[t] = e;
        __syncthreads();
    }
    int S = p0, E = p1 - 1;
    if (p0 < p1) {
        if (!(p0 == 0 || in[p0 - 1] != in[p0])) S = scan_s[t - 1];
        if (!(p1 == len || in[p1] != in[p1 - 1])) E = scan_e[t + 1];
    }
    // Adler sums of the block: (len - i) byte[i] = (p1 - i) byte[i] + (len - p1) byte[i]; below 2^32 per thread, reduced before the workgroup's sum
    {
        unsigned tot;
        const unsigned w = (aw + (unsigned)(len - p1) * as) % ADLER;
        block_scan(as, red, tot);
        const unsigned s_all = tot % ADLER;
        block_scan(w, red, tot);
        if (t == 0) {
            a.badl[2 * ((long)f * a.nb + blk)] = s_all;
            a.badl[2 * ((long)f * a.nb + blk) + 1] = tot % ADLER;
        }
    }

    // histograms
    for_tokens(in, p0, p1, S, E, [&](unsigned char v) { atomicAdd(&f_ll[v], 1u); },
               [&](int ml) { int sym, eb; unsigned ev; length_symbol(ml, sym, eb, ev); atomicAdd(&f_ll[sym], 1u); atomicAdd(&f_d[0], 1u); });
    if (t == 0) f_ll[256] = 1u;
    __syncthreads();
    // the fixed cost is taken before build_lengths may force a frequency
    {
        unsigned fixed = 0u;
        for (int i = t; i < NLL; i += PNG_THREADS) fixed += f_ll[i] * (unsigned)(fixed_len(i) + length_extra_bits(i));
        if (t == 0) { fixed += f_d[0] * 5u + 3u; sh[6] = f_d[0]; }      // (the matches, before a distance frequency is forced)
        atomicAdd(&sh[1], fixed);
    }
    __syncthreads();
    build_lengths(f_ll, NLL, 15, l_ll, key, work, counts);
    build_lengths(f_d, ND, 15, l_d, key, work, counts);
    if (t == 0) {
        canonical_codes(l_ll, NLL, 15, c_ll);
        canonical_codes(l_d, ND, 15, c_d);
        // the code lengths of both alphabets as one sequence, run-length coded with 16 (repeat the previous 3..6), 17 (3..10 zeros), 18 (11..138 zeros)
        int hlit = NLL, hdist = ND;
        while (hlit > 257 && l_ll[hlit - 1] == 0) hlit--;
        while (hdist > 1 && l_d[hdist - 1] == 0) hdist--;
        const int total = hlit + hdist;
        int ntok = 0;
        auto at_len = [&](int i) -> int { return i < hlit ? l_ll[i] : l_d[i - hlit]; };
        for (int i = 0; i < total;) {
            const int v = at_len(i);
            int run = 1;
            while (i + run < total && at_len(i + run) == v) run++;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int r = run < 138 ? run : 138; cl_tok[ntok++] = (unsigned short)(18 | ((r - 11) << 8)); f_cl[18]++; run -= r; }
                if (run >= 3) { cl_tok[ntok++] = (unsigned short)(17 | ((run - 3) << 8)); f_cl[17]++; run = 0; }
            } else {
                cl_tok[ntok++] = (unsigned short)v; f_cl[v]++; run--;
                while (run >= 3) { const int r = run < 6 ? run : 6; cl_tok[ntok++] = (unsigned short)(16 | ((r - 3) << 8)); f_cl[16]++; run -= r; }
            }
            for (; run > 0; run--) { cl_tok[ntok++] = (unsigned short)v; f_cl[v]++; }
        }
        sh[3] = (unsigned)ntok; sh[4] = (unsigned)hlit; sh[7] = (unsigned)hdist;
    }
    __syncthreads();
    build_lengths(f_cl, NCL, 7, l_cl, key, work, counts);
    {
        unsigned dyn = 0u;
        for (int i = t; i < NLL; i += PNG_THREADS) dyn += f_ll[i] * (unsigned)(l_ll[i] + length_extra_bits(i));
        atomicAdd(&sh[0], dyn);
    }
    if (t == 0) {
        canonical_codes(l_cl, NCL, 7, c_cl);
        const int order[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = NCL;
        while (hclen > 4 && l_cl[order[hclen - 1]] == 0) hclen--;
        unsigned hb = 3u + 5u + 5u + 4u + 3u * (unsigned)hclen;
        const int ntok = (int)sh[3];
        for (int i = 0; i < ntok; i++) { const int s = cl_tok[i] & 255; hb += l_cl[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u); }
        sh[2] = hb; sh[5] = (unsigned)hclen;
    }
    __syncthreads();
    // the three candidates in bytes, with what ends a block that is not the last on a byte boundary
    const unsigned dyn_bits = sh[2] + sh[0] + sh[6] * l_d[0];
    const unsigned fix_bits = sh[1];
    auto closed = [&](unsigned bits) -> unsigned { return final_block ? (bits + 7u) >> 3 : ((bits & 7u) ? ((bits + 3u + 7u) >> 3) + 4u : bits >> 3); };
    const unsigned stored_bytes = (unsigned)len + PNG_STORED, fix_bytes = closed(fix_bits), dyn_bytes = closed(dyn_bits);
    int type = 0;
    unsigned out_len = stored_bytes;
    if (fix_bytes < out_len) { type = 1; out_len = fix_bytes; }
    if (dyn_bytes < out_len) { type = 2; out_len = dyn_bytes; }

    if (type == 0) {
        if (t == 0) { out[0] = final_block ? 1 : 0; out[1] = (unsigned char)(len & 255); out[2] = (unsigned char)(len >> 8); out[3] = (unsigned char)(~len & 255); out[4] = (unsigned char)((~len >> 8) & 255); }
        for (int i = t; i < len; i += PNG_THREADS) out[PNG_STORED + i] = in[i];
    } else {
        const unsigned head_bits = type == 2 ? sh[2] : 3u;
        const unsigned dlen = type == 2 ? l_d[0] : 5u, dcode = type == 2 ? c_d[0] : 0u;
        // the bits of this thread's tokens, their place, the tokens
        unsigned mine = 0u;
        for_tokens(in, p0, p1, S, E, [&](unsigned char v) { mine += type == 2 ? l_ll[v] : (unsigned)fixed_len(v); },
                   [&](int ml) { int sym, eb; unsigned ev; length_symbol(ml, sym, eb, ev); mine += (type == 2 ? l_ll[sym] : (unsigned)fixed_len(sym)) + eb + dlen; });
        unsigned total;
        const unsigned first = head_bits + block_scan(mine, red, total);
        BitWriter bw;
        if (t == 0) {
            bw.start(out_w, 0u);
            bw.put((final_block ? 1u : 0u) | ((unsigned)type << 1), 3);
            if (type == 2) {
                const int order[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                bw.put(sh[4] - 257u, 5); bw.put(sh[7] - 1u, 5); bw.put(sh[5] - 4u, 4);
                for (int i = 0; i < (int)sh[5]; i++) bw.put(l_cl[order[i]], 3);
                for (int i = 0; i < (int)sh[3]; i++) {
                    const int s = cl_tok[i] & 255;
                    bw.put(c_cl[s], l_cl[s]);
                    if (s >= 16) bw.put((unsigned)(cl_tok[i] >> 8), s == 16 ? 2 : s == 17 ? 3 : 7);
                }
            }
            bw.flush();
            // end of block
            unsigned code; int cl;
            if (type == 2) { code = c_ll[256]; cl = l_ll[256]; } else fixed_code(256, code, cl);
            bw.start(out_w, head_bits + total);
            bw.put(code, cl);
            bw.flush();
        }
        bw.start(out_w, first);
        for_tokens(in, p0, p1, S, E,
                   [&](unsigned char v) { unsigned code; int cl; if (type == 2) { code = c_ll[v]; cl = l_ll[v]; } else fixed_code(v, code, cl); bw.put(code, cl); },
                   [&](int ml) {
                       int sym, eb; unsigned ev, code; int cl;
                       length_symbol(ml, sym, eb, ev);
                       if (type == 2) { code = c_ll[sym]; cl = l_ll[sym]; } else fixed_code(sym, code, cl);
                       bw.put(code, cl);
                       if (eb) bw.put(ev, eb);
                       bw.put(dcode, (int)dlen);
                   });
        bw.flush();
        __syncthreads();
        if (t == 0 && !final_block) {
            const unsigned bits = type == 2 ? dyn_bits : fix_bits;
            if (bits & 7u) { out[out_len - 2] = 0xFF; out[out_len - 1] = 0xFF; }      // the empty stored block: 3 zero bits and the padding are there already, LEN = 0
        }
    }
    __syncthreads();
    // stage the bytes; their raw CRC: every thread takes a piece, shifts it by the bytes behind it, the pieces meet by XOR
    unsigned char* dst = a.comp + ((long)f * a.nb + blk) * PNG_CSTRIDE;
    for (unsigned i = t; i < (out_len + 3u) / 4u; i += PNG_THREADS) ((unsigned*)dst)[i] = out_w[i];
    const unsigned piece = (out_len + PNG_THREADS - 1u) / PNG_THREADS;
    const unsigned q0 = (unsigned)t * piece < out_len ? (unsigned)t * piece : out_len, q1 = q0 + piece < out_len ? q0 + piece : out_len;
    unsigned crc = 0u;
    for (unsigned q = q0; q < q1; q++) crc = crc_t[(crc ^ out[q]) & 255u] ^ (crc >> 8);
    if (q1 > q0) crc = shift_bytes(crc, out_len - q1, crc_t + 256);
    crc = block_xor(crc, red);
    if (t == 0) { a.blen[(long)f * a.nb + blk] = out_len; a.bcrc[(long)f * a.nb + blk] = crc; }
}

// ---- (c) per image: places of the blocks, Adler-32, CRC-32, the file length -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNG_THREADS) void k_png_finish(PngArgs a) {
    __shared__ unsigned red[PNG_WAVES];
    __shared__ unsigned xp[32];
    const int t = threadIdx.x, f = blockIdx.x;
    if (t < 32) xp[t] = a.crc_table[256 + t];
    const unsigned* blen = a.blen + (long)f * a.nb;
    const unsigned* badl = a.badl + 2 * (long)f * a.nb;
    unsigned* boff = a.boff + (long)f * a.nb;
    unsigned carry = 0u, A = 1u, B = 0u;      // Adler-32: A = 1 + sum of the bytes, B = sum of the running A
    for (long base = 0; base < a.nb; base += PNG_THREADS) {
        const long j = base + t;
        const bool in_range = j < a.nb;
        unsigned total;
        const unsigned off = carry + block_scan(in_range ? blen[j] : 0u, red, total);
        if (in_range) boff[j] = off;
        carry += total;
        const unsigned s = in_range ? badl[2 * j] : 0u, w = in_range ? badl[2 * j + 1] : 0u;
        const unsigned n = in_range ? (unsigned)(a.stream - j * PNG_BLOCK < PNG_BLOCK ? a.stream - j * PNG_BLOCK : PNG_BLOCK) : 0u;
        unsigned s_total;
        const unsigned a_before = (A + block_scan(s, red, s_total)) % ADLER;      // (256 terms below 65521 and A: below 2^32)
        unsigned b_total;
        block_scan((w + n * a_before % ADLER) % ADLER, red, b_total);               // (n <= 16384, a_before < 65521: the product is below 2^32)
        A = (A + s_total) % ADLER;
        B = (B + b_total) % ADLER;
    }
    const unsigned sum = carry, adler = (B << 16) | A;
    // CRC-32 over "IDAT", the zlib header, the blocks, the Adler value: raw pieces shifted by what follows them; then the standard start and end complement, which add
    // 0xFFFFFFFF x^(8 n) + 0xFFFFFFFF to the raw remainder of n bytes
    __syncthreads();
    unsigned crc = 0u;
    for (long j = t; j < a.nb; j += PNG_THREADS) crc ^= shift_bytes(a.bcrc[(long)f * a.nb + j], (unsigned long long)(sum - boff[j] - blen[j]) + 4ull, xp);
    if (t == 0) {
        unsigned h = 0u;
        for (int i = 0; i < 6; i++) { h ^= a.head[37 + i]; for (int k = 0; k < 8; k++) h = (h & 1u) ? (h >> 1) ^ PNG_POLY : h >> 1; }
        crc ^= shift_bytes(h, (unsigned long long)sum + 4ull, xp);
        unsigned tail = 0u;
        for (int i = 0; i < 4; i++) { tail ^= (adler >> (24 - 8 * i)) & 255u; for (int k = 0; k < 8; k++) tail = (tail & 1u) ? (tail >> 1) ^ PNG_POLY : tail >> 1; }
        crc ^= tail;
    }
    crc = block_xor(crc, red);
    if (t == 0) {
        const unsigned long long n = 10ull + sum;
        crc ^= shift_bytes(0xFFFFFFFFu, n, xp) ^ 0xFFFFFFFFu;
        unsigned* im = a.image + 4 * (long)f;
        im[0] = sum; im[1] = adler; im[2] = crc; im[3] = PNG_FRAME + sum;
    }
}

// ---- (d) grid (PNG_WRITE_BLOCKS, nf) ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNG_THREADS) void k_png_write(PngArgs a) {
    __shared__ unsigned red[PNG_WAVES];
    const int t = threadIdx.x, f = blockIdx.y;
    unsigned before = 0u, total;
    for (int g = t; g < f; g += PNG_THREADS) before += a.image[4 * (long)g + 3];
    block_scan(before, red, total);
    const size_t base = (size_t)(a.n0 > 0 ? a.offsets[a.n0] : 0u) + total;
    const unsigned* im = a.image + 4 * (long)f;
    const unsigned sum = im[0], adler = im[1], crc = im[2], flen = im[3];
    auto put = [&](size_t pos, unsigned v) { if (pos < a.capacity) a.out[pos] = (unsigned char)v; };
    if (blockIdx.x == 0) {
        if (t < PNG_HEAD + 2) {
            const unsigned idat = sum + 6u;      // the chunk's data: zlib header, blocks, Adler-32
            put(base + t, (t >= 33 && t < 37) ? (idat >> (8 * (36 - t))) & 255u : a.head[t]);
        }
        if (t >= 64 && t < 64 + 20) {
            const int i = t - 64;      // Adler-32, the IDAT CRC, IEND
            const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
            put(base + PNG_HEAD + 2 + sum + i, i < 4 ? (adler >> (24 - 8 * i)) & 255u : i < 8 ? (crc >> (24 - 8 * (i - 4))) & 255u : iend[i - 8]);
        }
        if (t == 0) {
            if (f > 0 || a.n0 == 0) a.offsets[a.n0 + f] = (unsigned)base;      // (the first offset of a later chunk is the total the chunk before wrote)
            if (f == a.nf - 1) a.offsets[a.n0 + a.nf] = (unsigned)(base + flen);
        }
    }
    for (long j = blockIdx.x; j < a.nb; j += gridDim.x) {
        const unsigned char* src = a.comp + ((long)f * a.nb + j) * PNG_CSTRIDE;
        const unsigned n = a.blen[(long)f * a.nb + j];
        const size_t to = base + PNG_HEAD + 2 + a.boff[(long)f * a.nb + j];
        for (unsigned i = t; i < n && i < (unsigned)PNG_CSTRIDE; i += PNG_THREADS) put(to + i, src[i]);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
unsigned host_crc(const unsigned char* p, size_t n) {
    unsigned c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ PNG_POLY : c >> 1; }
    return c ^ 0xFFFFFFFFu;
}
unsigned host_mulmod(unsigned a, unsigned b) {
    unsigned p = 0u;
    for (int i = 0; i < 32; i++) { if (a & (0x80000000u >> i)) p ^= b; b = (b & 1u) ? (b >> 1) ^ PNG_POLY : b >> 1; }
    return p;
}
long png_stream(int H, int W) { return (long)H * (1 + 3L * W); }
long png_blocks(int H, int W) { return (png_stream(H, W) + PNG_BLOCK - 1) / PNG_BLOCK; }
unsigned long long image_bound(int H, int W) { return (unsigned long long)PNG_FRAME + (unsigned long long)png_stream(H, W) + (unsigned long long)PNG_STORED * png_blocks(H, W); }

bool png_args_ok(int max_frames, int H, int W, int mode) {
    if (max_frames < 1 || H < 1 || W < 1) { set_error("caddy_png: max_frames, height and width must be positive"); return false; }
    if (mode < 0 || mode > PNG_ADAPTIVE) { set_error("caddy_png: filter_mode must be 0..4 or CADDY_PNG_FILTER_ADAPTIVE (5)"); return false; }
    if (max_frames > 65535) { set_error("caddy_png: at most 65535 images per chunk"); return false; }
    if ((unsigned long long)H * (1ull + 3ull * W) > 0x7FFFFFFFull || image_bound(H, W) > 0x7FFFFFFFull) {
        set_error("caddy_png: the bound of one " + std::to_string(H) + " x " + std::to_string(W) + " image passes 2^31 - 1 bytes");
        return false;
    }
    return true;
}

void png_chunk(caddy_ctx* c, const unsigned char* frames, long n0, int nf, unsigned char* out, size_t capacity, unsigned* offsets) {
    PngState* s = c->png;
    c->act.reset();
    PngArgs a{};
    const size_t M = (size_t)s->max_frames;      // (sized for a full chunk whatever nf is, so the walk's count holds for every call)
    a.filt = (unsigned char*)c->act.alloc(M * s->fstride);
    a.comp = (unsigned char*)c->act.alloc(M * s->nb * PNG_CSTRIDE);
    a.blen = (unsigned*)c->act.alloc(sizeof(unsigned) * M * s->nb);
    a.boff = (unsigned*)c->act.alloc(sizeof(unsigned) * M * s->nb);
    a.bcrc = (unsigned*)c->act.alloc(sizeof(unsigned) * M * s->nb);
    a.badl = (unsigned*)c->act.alloc(sizeof(unsigned) * 2 * M * s->nb);
    a.image = (unsigned*)c->act.alloc(sizeof(unsigned) * 4 * M);
    if (c->dry || c->act.overflow()) return;
    a.frames = frames; a.nf = nf; a.H = s->H; a.W = s->W; a.mode = s->filter_mode;
    a.stream = s->stream; a.nb = s->nb; a.fstride = s->fstride;
    a.head = s->d_head; a.crc_table = s->d_crc_table;
    a.out = out; a.capacity = capacity; a.offsets = offsets; a.n0 = n0;
    hipLaunchKernelGGL(k_png_filter, dim3((unsigned)s->H, (unsigned)nf), dim3(PNG_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_png_deflate, dim3((unsigned)s->nb, (unsigned)nf), dim3(PNG_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_png_finish, dim3((unsigned)nf), dim3(PNG_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_png_write, dim3((unsigned)std::min<long>(s->nb, PNG_WRITE_BLOCKS), (unsigned)nf), dim3(PNG_THREADS), 0, c->stream, a);
    c->ck(hipGetLastError() == hipSuccess ? 0 : -1, "png encoder");
}

EvalKind png_kind(int max_frames, int H, int W, int mode) {
    return {CTX_PNG, max_frames, H, W,
            [=](caddy_ctx* c) {
                PngState* s = new PngState();
                c->png = s;
                s->max_frames = max_frames; s->H = H; s->W = W; s->filter_mode = mode;
                s->stream = png_stream(H, W); s->nb = png_blocks(H, W);
                s->fstride = (s->stream + 15) & ~15L; s->cstride = PNG_CSTRIDE;
                s->d_head = (unsigned char*)c->persist.alloc(64);
                s->d_crc_table = (unsigned*)c->persist.alloc(sizeof(unsigned) * (256 + 32));
            },
            [](caddy_ctx* c) { png_chunk(c, nullptr, 0, c->png->max_frames, nullptr, 0, nullptr); },
            "caddy_png_workspace_bytes"};
}

}  // namespace

void png_free(caddy_ctx* c) {
    if (!c || !c->png) return;
    delete c->png;
    c->png = nullptr;
}

extern "C" {
size_t caddy_png_workspace_bytes(int max_frames, int H, int W) {
    return png_args_ok(max_frames, H, W, 0) ? eval_workspace_bytes(png_kind(max_frames, H, W, 0)) : 0;
}
caddy_ctx* caddy_png_ctx_create(int max_frames, int H, int W, int filter_mode, void* workspace, size_t bytes) {
    if (!png_args_ok(max_frames, H, W, filter_mode)) return nullptr;
    caddy_ctx* c = eval_ctx_create(png_kind(max_frames, H, W, filter_mode), workspace, bytes);
    if (!c) return nullptr;
    PngState* s = c->png;
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    unsigned char* h = s->head;
    memcpy(h, sig, 8);
    const unsigned char ihdr[21] = {0, 0, 0, 13, 'I', 'H', 'D', 'R', (unsigned char)(W >> 24), (unsigned char)(W >> 16), (unsigned char)(W >> 8), (unsigned char)W,
                                    (unsigned char)(H >> 24), (unsigned char)(H >> 16), (unsigned char)(H >> 8), (unsigned char)H, 8, 2, 0, 0, 0};
    memcpy(h + 8, ihdr, 21);
    const unsigned crc = host_crc(h + 12, 17);
    for (int i = 0; i < 4; i++) h[29 + i] = (unsigned char)(crc >> (24 - 8 * i));
    memcpy(h + 37, "IDAT", 4);      // (h[33..37), the chunk's length, is written per image)
    unsigned char head[64] = {};
    memcpy(head, h, PNG_HEAD);
    head[41] = 0x78; head[42] = 0x01;      // zlib: deflate, 32 KiB window, no preset dictionary, fastest
    std::vector<unsigned> table(256 + 32);
    for (unsigned i = 0; i < 256; i++) { unsigned v = i; for (int k = 0; k < 8; k++) v = (v & 1u) ? (v >> 1) ^ PNG_POLY : v >> 1; table[i] = v; }
    unsigned p = 1u << 30;      // x^1
    table[256] = p;
    for (int k = 1; k < 32; k++) table[256 + k] = p = host_mulmod(p, p);
    hipMemcpy(s->d_head, head, 64, hipMemcpyHostToDevice);
    hipMemcpy(s->d_crc_table, table.data(), sizeof(unsigned) * table.size(), hipMemcpyHostToDevice);
    if (hipGetLastError() != hipSuccess) { set_error("caddy_png_ctx_create: uploading the tables failed"); caddy_ctx_destroy(c); return nullptr; }
    return c;
}
size_t caddy_png_stream_bound(int n, int H, int W) {
    if (!png_args_ok(n < 1 ? n : 1, H, W, 0)) return 0;
    return (size_t)n * (size_t)image_bound(H, W);
}
int caddy_png_encode(caddy_ctx* c, const unsigned char* frames_u8, int n, unsigned char* out_stream, size_t out_capacity, unsigned* offsets) {
    if (!ctx_needs(c, CTX_PNG, "caddy_png_encode")) return -2;
    c->fail = false;
    if (!frames_u8 || !out_stream || !offsets) { set_error("null input"); return -2; }
    if ((uintptr_t)offsets & 3) { set_error("caddy_png_encode: offsets must be 4-byte aligned"); return -2; }
    if (n < 1) { set_error("caddy_png_encode: n must be positive"); return -2; }
    const PngState* s = c->png;
    const unsigned long long bound = (unsigned long long)n * image_bound(s->H, s->W);
    if (bound > 0xFFFFFFFFull) { set_error("caddy_png_encode: the stream of " + std::to_string(n) + " images may pass 2^32 bytes (the offsets are 32-bit words): encode fewer images per call"); return -2; }
    if (out_capacity < bound) {
        set_error("caddy_png_encode: an output capacity of " + std::to_string(out_capacity) + " bytes, " + std::to_string(n) + " images may need " + std::to_string(bound) + " (caddy_png_stream_bound)");
        return -2;
    }
    const size_t frame = (size_t)s->H * s->W * 3;
    for_chunks(c, n, [&](long n0, int nf) {
        png_chunk(c, frames_u8 + n0 * frame, n0, nf, out_stream, out_capacity, offsets);
        return !c->fail;
    });
    return finish(c, "caddy_png_workspace_bytes");
}
}
