// TEST ONLY: a stand-alone driver of the PNG-reader entry points (csrc/png_read.hip: caddy_png_decode) for a sanitizer build of that file against the host simulator
// (tests/test_png_reader_emu.py builds it with -fsanitize=address,undefined and runs it; nothing here is loaded into python).  The decoder reads bytes nobody vouches for, so
// this is the evidence that no input makes the kernel read or write out of bounds: every buffer is exactly as large as the entry point's contract says -- the blob offsets[n]
// bytes, the offsets n + 1 words, the frames n H W 3 bytes, the status n words, the workspace caddy_png_read_workspace_bytes -- so a read past a file or a write past a frame,
// the status or the image's workspace slice is reported.  Fed: the files the cases refuse (argv[1]: a folder of good_*.png and bad_NN_*.png, NN the expected status), each
// between two good neighbours, and a few thousand seeded mutations of the good files generated here -- bytes anywhere in the file, cuts, and IDAT bytes with the chunk's CRC
// put right so that the mutation reaches the inflater.  Checked: the expected verdicts, that a refused frame is zero, that the neighbours decode to what they decode to alone,
// and that every call ends.
#include "caddy_hip.h"
#include <dirent.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef std::vector<unsigned char> Bytes;

static unsigned crc32_of(const unsigned char* p, size_t n) {
    unsigned c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1; }
    return c ^ 0xFFFFFFFFu;
}
static unsigned be32(const unsigned char* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3]; }
static unsigned rng_state = 12345u;
static unsigned rnd(unsigned below) { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) % below; }

static Bytes read_file(const std::string& path) {
    Bytes out;
    if (FILE* f = fopen(path.c_str(), "rb")) {
        unsigned char buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + n);
        fclose(f);
    }
    return out;
}

struct Decoder {
    int H, W, max_frames;
    void* raw = nullptr;
    caddy_ctx* ctx = nullptr;
    Decoder(int H_, int W_, int max_frames_) : H(H_), W(W_), max_frames(max_frames_) {
        const size_t bytes = caddy_png_read_workspace_bytes(max_frames, H, W);
        if (bytes && !posix_memalign(&raw, 256, bytes)) ctx = caddy_png_read_ctx_create(max_frames, H, W, raw, bytes);
    }
    ~Decoder() { if (ctx) caddy_ctx_destroy(ctx); free(raw); }
    // exactly sized buffers; -> false where the call itself failed
    bool run(const std::vector<Bytes>& files, std::vector<Bytes>& frames, std::vector<int>& status) {
        const int n = (int)files.size();
        size_t total = 0;
        for (const Bytes& f : files) total += f.size();
        Bytes blob(total ? total : 1);      // (an empty blob still needs a pointer; offsets[n] = 0 says that nothing of it is read)
        std::vector<unsigned> offsets((size_t)n + 1);
        size_t at = 0;
        for (int i = 0; i < n; i++) { offsets[i] = (unsigned)at; if (!files[i].empty()) memcpy(&blob[at], files[i].data(), files[i].size()); at += files[i].size(); }
        offsets[n] = (unsigned)at;
        const size_t frame = (size_t)H * W * 3;
        Bytes out(frame * n, 0x5A);
        status.assign(n, 0x5A5A5A5A);
        if (caddy_png_decode(ctx, blob.data(), offsets.data(), n, out.data(), status.data()) != 0) return false;
        frames.clear();
        for (int i = 0; i < n; i++) frames.emplace_back(out.begin() + i * frame, out.begin() + (i + 1) * frame);
        return true;
    }
};

static bool all_zero(const Bytes& v) { for (unsigned char b : v) if (b) return false; return true; }

static unsigned adler32_of(const unsigned char* p, size_t n) {
    unsigned a = 1u, b = 0u;
    for (size_t i = 0; i < n; i++) { a = (a + p[i]) % 65521u; b = (b + a) % 65521u; }
    return (b << 16) | a;
}
// a mutation of a good file; kind 0: bytes anywhere; 1: a cut; 2: bytes of the IDAT payload, the chunk's CRC put right, so that the inflater sees them; 3: the same, and where
// the payload is one stored block only its data bytes change and the Adler-32 is put right too, so that the unfilter sees them
static Bytes mutate(const Bytes& good, int kind) {
    Bytes m = good;
    if (kind == 0) {
        for (unsigned k = 1 + rnd(3); k > 0; k--) m[rnd((unsigned)m.size())] ^= (unsigned char)(1u + rnd(255));
        return m;
    }
    if (kind == 1) { m.resize(rnd((unsigned)m.size())); return m; }
    size_t at = 8;
    while (at + 12 <= m.size()) {      // (the good files are well formed)
        const unsigned len = be32(&m[at]);
        if (!memcmp(&m[at + 4], "IDAT", 4) && len > 6) {
            unsigned char* z = &m[at + 8];
            const bool stored = kind == 3 && len > 11 && z[2] == 1 && (unsigned)(z[3] | (z[4] << 8)) == len - 11;
            const unsigned first = stored ? 7u : 0u, span = stored ? len - 11 : len;
            for (unsigned k = 1 + rnd(2); k > 0; k--) {
                const unsigned where = first + rnd(span);
                if (rnd(2)) m[at + 8 + where] ^= (unsigned char)(1u << rnd(8)); else m[at + 8 + where] = (unsigned char)rnd(256);
            }
            if (stored) { const unsigned adler = adler32_of(z + 7, len - 11); for (int i = 0; i < 4; i++) z[len - 4 + i] = (unsigned char)(adler >> (24 - 8 * i)); }
            const unsigned crc = crc32_of(&m[at + 4], 4 + len);
            for (int i = 0; i < 4; i++) m[at + 8 + len + i] = (unsigned char)(crc >> (24 - 8 * i));
            break;
        }
        at += 12 + (size_t)len;
    }
    return m;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s folder H W\n", argv[0]); return 2; }
    const int H = atoi(argv[2]), W = atoi(argv[3]);
    std::vector<Bytes> good;
    std::vector<std::pair<int, Bytes>> bad;
    std::vector<std::string> names;
    if (DIR* d = opendir(argv[1])) {
        while (dirent* e = readdir(d)) names.push_back(e->d_name);
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    for (const std::string& name : names) {
        if (name.rfind("good_", 0) == 0) good.push_back(read_file(std::string(argv[1]) + "/" + name));
        if (name.rfind("bad_", 0) == 0) bad.push_back({atoi(name.c_str() + 4), read_file(std::string(argv[1]) + "/" + name)});
    }
    if (good.size() < 2 || bad.size() < 10) { fprintf(stderr, "png reader sanitizer driver: %zu good and %zu refused files\n", good.size(), bad.size()); return 2; }

    int wrong = 0;
    Decoder three(H, W, 3), many(H, W, 16);
    if (!three.ctx || !many.ctx) { fprintf(stderr, "png reader sanitizer driver: no context (%s)\n", caddy_last_error()); return 1; }
    std::vector<Bytes> frames, want;
    std::vector<int> status;
    // the good files alone: what the neighbours must decode to
    if (!many.run(good, want, status)) { fprintf(stderr, "png reader sanitizer driver: %s\n", caddy_last_error()); return 1; }
    for (size_t i = 0; i < good.size(); i++) if (status[i] != CADDY_PNG_OK) { fprintf(stderr, "good file %zu: status %d\n", i, status[i]); wrong++; }
    // every refused file between two good ones
    for (size_t k = 0; k < bad.size(); k++) {
        const size_t a = k % good.size(), b = (k + 1) % good.size();
        if (!three.run({good[a], bad[k].second, good[b]}, frames, status)) { fprintf(stderr, "png reader sanitizer driver: %s\n", caddy_last_error()); return 1; }
        if (status[0] != CADDY_PNG_OK || status[2] != CADDY_PNG_OK || status[1] != bad[k].first || frames[0] != want[a] || frames[2] != want[b] || !all_zero(frames[1])) {
            fprintf(stderr, "refused file %zu: status %d %d %d, expected 0 %d 0\n", k, status[0], status[1], status[2], bad[k].first);
            wrong++;
        }
    }
    // seeded mutations, 14 a call between two good files; the context holds 16, so every fourth call (of 20 files) also runs in two chunks
    int accepted = 0, verdicts[16] = {};
    const int calls = 260;
    for (int call = 0; call < calls; call++) {
        const size_t a = call % good.size(), b = (call + 1) % good.size();
        std::vector<Bytes> files{good[a]};
        const int inner = call % 4 == 3 ? 18 : 14;
        for (int k = 0; k < inner; k++) files.push_back(mutate(good[rnd((unsigned)good.size())], (call + k) % 4));
        files.push_back(good[b]);
        if (!many.run(files, frames, status)) { fprintf(stderr, "png reader sanitizer driver: %s\n", caddy_last_error()); return 1; }
        if (status.front() != CADDY_PNG_OK || status.back() != CADDY_PNG_OK || frames.front() != want[a] || frames.back() != want[b]) { fprintf(stderr, "call %d: a neighbour of the mutations changed\n", call); wrong++; }
        for (int k = 1; k <= inner; k++) {
            if (status[k] < 0 || status[k] > CADDY_PNG_TOO_LARGE) { fprintf(stderr, "call %d file %d: status %d\n", call, k, status[k]); wrong++; continue; }
            verdicts[status[k]]++;
            if (status[k] == CADDY_PNG_OK) accepted++;
            else if (!all_zero(frames[k])) { fprintf(stderr, "call %d file %d: refused (%d) and its frame is not zero\n", call, k, status[k]); wrong++; }
        }
    }
    printf("png reader sanitizer driver: %d mutations:", calls / 4 * (3 * 14 + 18));
    for (int v = 0; v <= CADDY_PNG_TOO_LARGE; v++) printf(" %d", verdicts[v]);
    printf("\n");
    // the mutations must have reached every stage: some accepted, some refused by the container, the inflater, the checksum and the filter
    if (accepted < 20 || verdicts[CADDY_PNG_BAD_CRC] < 20 || verdicts[CADDY_PNG_BAD_DEFLATE] < 20 || verdicts[CADDY_PNG_BAD_ADLER] < 20 || verdicts[CADDY_PNG_TRUNCATED] < 20) {
        fprintf(stderr, "png reader sanitizer driver: the mutations did not reach every stage\n");
        wrong++;
    }
    if (!wrong) puts("png reader sanitizer driver: ok");
    return wrong ? 1 : 0;
}
