// TEST ONLY: a stand-alone driver of the PNG-writer entry points (csrc/png.hip: caddy_png_encode, caddy_png_stream_bound) for a sanitizer build of that file against the host
// simulator (tests/test_png_writer_emu.py builds it with -fsanitize=address,undefined and runs it; nothing here is loaded into python).  Every buffer is exactly as large as
// the entry point's contract says -- the frames n H W 3 bytes, the stream caddy_png_stream_bound(n, H, W), the offsets n + 1 words, the workspace caddy_png_workspace_bytes --
// so a read past a frame or a write past the stream, the offsets or an intermediate buffer is reported.  The stream is also checked for its structure: the signature, the chunk
// lengths and CRCs, stored-block arithmetic where noise forces stored blocks, and the files of a several-image call against their single-image encodings.
#include "caddy_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fail(const char* what) { fprintf(stderr, "png writer sanitizer driver: %s (%s)\n", what, caddy_last_error()); return 1; }

static unsigned crc32_of(const unsigned char* p, size_t n) {
    unsigned c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1; }
    return c ^ 0xFFFFFFFFu;
}
static unsigned be32(const unsigned char* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3]; }

// signature, IHDR, one IDAT, IEND: lengths and CRCs
static int check_file(const std::vector<unsigned char>& f, int H, int W) {
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (f.size() < 63 || memcmp(f.data(), sig, 8) != 0) return 1;
    size_t at = 8;
    const char* want[3] = {"IHDR", "IDAT", "IEND"};
    for (int k = 0; k < 3; k++) {
        if (at + 12 > f.size()) return 1;
        const unsigned n = be32(&f[at]);
        if (at + 12 + n > f.size() || memcmp(&f[at + 4], want[k], 4) != 0) return 1;
        if (be32(&f[at + 8 + n]) != crc32_of(&f[at + 4], 4 + n)) return 1;
        if (k == 0 && (n != 13 || be32(&f[at + 8]) != (unsigned)W || be32(&f[at + 12]) != (unsigned)H)) return 1;
        if (k == 1 && (f[at + 8] != 0x78 || (f[at + 8] * 256 + f[at + 9]) % 31 != 0)) return 1;
        at += 12 + n;
    }
    return at == f.size() ? 0 : 1;
}

static int encode(int max_frames, int n, int H, int W, int mode, const std::vector<unsigned char>& frames, std::vector<std::vector<unsigned char>>& files) {
    const size_t bytes = caddy_png_workspace_bytes(max_frames, H, W);
    if (!bytes) return fail("workspace size");
    void* raw = nullptr;
    if (posix_memalign(&raw, 256, bytes)) return fail("allocation");
    caddy_ctx* c = caddy_png_ctx_create(max_frames, H, W, mode, raw, bytes);
    if (!c) return fail("context");
    const size_t bound = caddy_png_stream_bound(n, H, W);
    std::vector<unsigned char> out(bound, 0x5A);
    std::vector<unsigned> offsets((size_t)n + 1, 0x5A5A5A5Au);
    int bad = 0;
    if (caddy_png_encode(c, frames.data(), n, out.data(), bound - 1, offsets.data()) != -2) bad++;      // refused before anything is touched
    for (unsigned char v : out) if (v != 0x5A) { bad++; break; }
    for (int rep = 0; rep < 2; rep++) {      // the second call finds the buffers used
        if (caddy_png_encode(c, frames.data(), n, out.data(), bound, offsets.data()) != 0) return fail("caddy_png_encode");
        if (offsets[0] != 0 || offsets[n] > bound) bad++;
        for (size_t i = offsets[n]; i < bound; i++) if (out[i] != 0x5A) { bad++; break; }
        files.clear();
        for (int f = 0; f < n; f++) {
            if (offsets[f + 1] < offsets[f] + 63) { bad++; break; }
            std::vector<unsigned char> file(out.begin() + offsets[f], out.begin() + offsets[f + 1]);
            bad += check_file(file, H, W);
            files.push_back(file);
        }
    }
    caddy_ctx_destroy(c);
    free(raw);
    if (bad) fprintf(stderr, "png writer sanitizer driver: %d mismatches at n %d (chunks of %d) %d x %d mode %d\n", bad, n, max_frames, H, W, mode);
    return bad ? 1 : 0;
}

static std::vector<unsigned char> noise(size_t bytes, unsigned seed) {
    std::vector<unsigned char> v(bytes);
    for (unsigned char& b : v) { seed = seed * 1664525u + 1013904223u; b = (unsigned char)(seed >> 24); }
    return v;
}
static std::vector<unsigned char> ramp(int H, int W) {
    std::vector<unsigned char> v((size_t)H * W * 3);
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) for (int ch = 0; ch < 3; ch++) v[((size_t)y * W + x) * 3 + ch] = (unsigned char)(x / 3 + y / 2 + 40 * ch);
    return v;
}

static int run(int H, int W, int mode, const std::vector<unsigned char>& frame) {
    std::vector<std::vector<unsigned char>> files;
    return encode(1, 1, H, W, mode, frame, files);
}

// noise: every block stored, so the file is exactly the bound
static int run_noise(int H, int W) {
    std::vector<std::vector<unsigned char>> files;
    int rc = encode(1, 1, H, W, CADDY_PNG_FILTER_ADAPTIVE, noise((size_t)H * W * 3, 1234u + H * 131 + W), files);
    if (!rc && files[0].size() != caddy_png_stream_bound(1, H, W)) { fprintf(stderr, "png writer sanitizer driver: noise is not at the bound\n"); rc = 1; }
    return rc;
}

// three images (noise, flat, ramp) in one call, in one chunk and in chunks of two, against their single-image encodings
static int run_three(int H, int W) {
    const size_t frame = (size_t)H * W * 3;
    std::vector<unsigned char> frames = noise(3 * frame, 99u);
    memset(frames.data() + frame, 200, frame);
    const std::vector<unsigned char> r = ramp(H, W);
    memcpy(frames.data() + 2 * frame, r.data(), frame);
    std::vector<std::vector<unsigned char>> single, all, one;
    int rc = 0;
    for (int f = 0; f < 3; f++) {
        rc |= encode(1, 1, H, W, CADDY_PNG_FILTER_ADAPTIVE, std::vector<unsigned char>(frames.begin() + f * frame, frames.begin() + (f + 1) * frame), one);
        if (rc) return rc;
        single.push_back(one[0]);
    }
    for (int max_frames = 2; max_frames <= 3; max_frames++) {
        rc |= encode(max_frames, 3, H, W, CADDY_PNG_FILTER_ADAPTIVE, frames, all);
        if (rc) return rc;
        if (all != single) { fprintf(stderr, "png writer sanitizer driver: a three-image call in chunks of %d differs from the single-image encodings\n", max_frames); rc = 1; }
    }
    return rc;
}

int main() {
    int rc = 0;
    rc |= run(1, 1, CADDY_PNG_FILTER_ADAPTIVE, noise(3, 5u));                     // the smallest image: a 4-byte stream
    rc |= run(33, 17, CADDY_PNG_FILTER_ADAPTIVE, ramp(33, 17));                   // a row stride that is no multiple of 4
    rc |= run(75, 75, 0 /* None */, std::vector<unsigned char>(75 * 75 * 3, 0));      // one run across a block boundary; the second block is short
    rc |= run(128, 128, 4 /* Paeth */, ramp(128, 128));                  // exactly three full blocks and a fourth of 128 bytes
    rc |= run_noise(64, 64);
    rc |= run_noise(74, 74);                                                       // 16502 stream bytes: a last block of 118
    rc |= run_three(24, 40);
    if (!rc) puts("png writer sanitizer driver: ok");
    return rc;
}
