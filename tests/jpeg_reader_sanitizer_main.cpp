// TEST ONLY: a stand-alone driver of the JPEG-reader entry points (csrc/jpeg_read.hip: caddy_jpeg_decode) for a sanitizer build of that file against the host simulator
// (tests/test_jpeg_reader_emu.py builds it with -fsanitize=address,undefined and runs it; nothing here is loaded into python).  The decoder reads bytes nobody vouches for, so
// this is the evidence that no input makes the kernels read or write out of bounds: every buffer is exactly as large as the entry point's contract says -- the blob offsets[n]
// bytes, the offsets n + 1 words, the frames n H W 3 bytes, the status n words, the workspace caddy_jpeg_read_workspace_bytes -- so a read past a file or a write past a frame,
// the status or the image's workspace slice is reported.  Fed: the files the cases refuse (argv[1]: a folder of good_*.jpg and bad_NN_*.jpg, NN the expected status), each
// between two good neighbours, and a few thousand seeded mutations of the good files generated here -- bytes anywhere in the file, cuts, bits of the scan and bits of the
// segments in front of it.  Checked: the expected verdicts, that a refused frame is zero, that the neighbours decode to what they decode to alone, and that every call ends.
#include "caddy_hip.h"
#include <dirent.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef std::vector<unsigned char> Bytes;

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
        const size_t bytes = caddy_jpeg_read_workspace_bytes(max_frames, H, W);
        if (bytes && !posix_memalign(&raw, 256, bytes)) ctx = caddy_jpeg_read_ctx_create(max_frames, H, W, raw, bytes);
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
        if (caddy_jpeg_decode(ctx, blob.data(), offsets.data(), n, out.data(), status.data()) != 0) return false;
        frames.clear();
        for (int i = 0; i < n; i++) frames.emplace_back(out.begin() + i * frame, out.begin() + (i + 1) * frame);
        return true;
    }
};

static bool all_zero(const Bytes& v) { for (unsigned char b : v) if (b) return false; return true; }

// where the entropy bytes of a (well-formed) file start: behind the SOS segment
static size_t scan_of(const Bytes& f) {
    for (size_t i = 2; i + 4 <= f.size();) {
        if (f[i] != 0xFF) return f.size();
        const unsigned len = ((unsigned)f[i + 2] << 8) | f[i + 3];
        if (f[i + 1] == 0xDA) return i + 2 + len;
        i += 2 + (size_t)len;
    }
    return f.size();
}
// a mutation of a good file; kind 0: bytes anywhere; 1: a cut; 2: one or two bits of the scan, so that the entropy decoder sees them; 3: one bit of the segments in front of it
static Bytes mutate(const Bytes& good, int kind) {
    Bytes m = good;
    const size_t scan = scan_of(good);
    if (kind == 0) {
        for (unsigned k = 1 + rnd(3); k > 0; k--) m[rnd((unsigned)m.size())] ^= (unsigned char)(1u + rnd(255));
    } else if (kind == 1) {
        m.resize(rnd((unsigned)m.size()));
    } else if (kind == 2 && scan + 2 < m.size()) {
        for (unsigned k = 1 + rnd(2); k > 0; k--) m[scan + rnd((unsigned)(m.size() - 2 - scan))] ^= (unsigned char)(1u << rnd(8));
    } else if (scan > 2) {
        m[2 + rnd((unsigned)(scan - 2))] ^= (unsigned char)(1u << rnd(8));
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
    if (good.size() < 2 || bad.size() < 10) { fprintf(stderr, "jpeg reader sanitizer driver: %zu good and %zu refused files\n", good.size(), bad.size()); return 2; }

    int wrong = 0;
    Decoder three(H, W, 3), many(H, W, 16);
    if (!three.ctx || !many.ctx) { fprintf(stderr, "jpeg reader sanitizer driver: no context (%s)\n", caddy_last_error()); return 1; }
    std::vector<Bytes> frames, want;
    std::vector<int> status;
    // the good files alone: what the neighbours must decode to
    if (!many.run(good, want, status)) { fprintf(stderr, "jpeg reader sanitizer driver: %s\n", caddy_last_error()); return 1; }
    for (size_t i = 0; i < good.size(); i++) if (status[i] != CADDY_JPEG_OK) { fprintf(stderr, "good file %zu: status %d\n", i, status[i]); wrong++; }
    // every refused file between two good ones
    for (size_t k = 0; k < bad.size(); k++) {
        const size_t a = k % good.size(), b = (k + 1) % good.size();
        if (!three.run({good[a], bad[k].second, good[b]}, frames, status)) { fprintf(stderr, "jpeg reader sanitizer driver: %s\n", caddy_last_error()); return 1; }
        if (status[0] != CADDY_JPEG_OK || status[2] != CADDY_JPEG_OK || status[1] != bad[k].first || frames[0] != want[a] || frames[2] != want[b] || !all_zero(frames[1])) {
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
        if (!many.run(files, frames, status)) { fprintf(stderr, "jpeg reader sanitizer driver: %s\n", caddy_last_error()); return 1; }
        if (status.front() != CADDY_JPEG_OK || status.back() != CADDY_JPEG_OK || frames.front() != want[a] || frames.back() != want[b]) { fprintf(stderr, "call %d: a neighbour of the mutations changed\n", call); wrong++; }
        for (int k = 1; k <= inner; k++) {
            if (status[k] < 0 || status[k] > CADDY_JPEG_BAD_SCAN) { fprintf(stderr, "call %d file %d: status %d\n", call, k, status[k]); wrong++; continue; }
            verdicts[status[k]]++;
            if (status[k] == CADDY_JPEG_OK) accepted++;
            else if (!all_zero(frames[k])) { fprintf(stderr, "call %d file %d: refused (%d) and its frame is not zero\n", call, k, status[k]); wrong++; }
        }
    }
    printf("jpeg reader sanitizer driver: %d mutations:", calls / 4 * (3 * 14 + 18));
    for (int v = 0; v <= CADDY_JPEG_BAD_SCAN; v++) printf(" %d", verdicts[v]);
    printf("\n");
    // the mutations must have reached every stage: some accepted (the IDCT and the colour stage ran on changed values), some refused by the marker walk, the tables, the
    // entropy decoder and the restart / end-of-scan checks
    if (accepted < 20 || verdicts[CADDY_JPEG_TRUNCATED] < 20 || verdicts[CADDY_JPEG_BAD_TABLE] < 20 || verdicts[CADDY_JPEG_BAD_RESTART] < 20 ||
        verdicts[CADDY_JPEG_BAD_CODE] + verdicts[CADDY_JPEG_BAD_COEFFICIENT] + verdicts[CADDY_JPEG_BAD_SCAN] < 20) {
        fprintf(stderr, "jpeg reader sanitizer driver: the mutations did not reach every stage\n");
        wrong++;
    }
    if (!wrong) puts("jpeg reader sanitizer driver: ok");
    return wrong ? 1 : 0;
}
