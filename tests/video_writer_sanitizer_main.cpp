// TEST ONLY: a stand-alone driver of the video-writer entry points (csrc/video.hip: caddy_video_encode, caddy_video_stream_bound, caddy_video_tables_get) for a sanitizer
// build of that file against the host simulator (tests/test_video_writer_emu.py builds it with -fsanitize=address,undefined and runs it; nothing here is loaded into python).
// Every buffer is exactly as large as the entry point's contract says -- the frames n H W 3 bytes, the stream caddy_video_stream_bound(n, H, W), the offsets n + 1 words,
// the workspace caddy_video_workspace_bytes -- so a read past a frame or a write past the stream, the offsets or an intermediate buffer is reported.  The stream is also
// checked for its structure: every file is header + scan + EOI, no marker inside a scan, the files of a several-frame call equal their single-frame encodings.
#include "caddy_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fail(const char* what) { fprintf(stderr, "video writer sanitizer driver: %s (%s)\n", what, caddy_last_error()); return 1; }

static int encode(int max_frames, int n, int H, int W, int quality, const std::vector<unsigned char>& frames, std::vector<std::vector<unsigned char>>& files) {
    const size_t bytes = caddy_video_workspace_bytes(max_frames, H, W);
    if (!bytes) return fail("workspace size");
    void* raw = nullptr;
    if (posix_memalign(&raw, 256, bytes)) return fail("allocation");
    caddy_ctx* c = caddy_video_ctx_create(max_frames, H, W, quality, raw, bytes);
    if (!c) return fail("context");
    unsigned char header[623];
    int header_bytes = 0;
    if (caddy_video_tables_get(c, nullptr, header, &header_bytes) != 0 || header_bytes != 623) return fail("tables");
    const size_t bound = caddy_video_stream_bound(n, H, W);
    std::vector<unsigned char> out(bound, 0x5A);
    std::vector<unsigned> offsets((size_t)n + 1, 0x5A5A5A5Au);
    int bad = 0;
    if (caddy_video_encode(c, frames.data(), n, out.data(), bound - 1, offsets.data()) != -2) bad++;      // refused before anything is touched
    for (unsigned char v : out) if (v != 0x5A) { bad++; break; }
    for (int rep = 0; rep < 2; rep++) {      // the second call finds the bit buffer used
        if (caddy_video_encode(c, frames.data(), n, out.data(), bound, offsets.data()) != 0) return fail("caddy_video_encode");
        if (offsets[0] != 0 || offsets[n] > bound) bad++;
        for (size_t i = offsets[n]; i < bound; i++) if (out[i] != 0x5A) { bad++; break; }
        files.clear();
        for (int f = 0; f < n; f++) {
            if (offsets[f + 1] < offsets[f] + 623 + 2) { bad++; break; }
            std::vector<unsigned char> file(out.begin() + offsets[f], out.begin() + offsets[f + 1]);
            if (memcmp(file.data(), header, 623) != 0) bad++;
            if (file[file.size() - 2] != 0xFF || file[file.size() - 1] != 0xD9) bad++;
            for (size_t i = 623; i + 2 < file.size(); i++) if (file[i] == 0xFF && file[i + 1] != 0x00) { bad++; break; }      // stuffed: no marker inside the scan
            files.push_back(file);
        }
    }
    caddy_ctx_destroy(c);
    free(raw);
    if (bad) fprintf(stderr, "video writer sanitizer driver: %d mismatches at n %d (chunks of %d) %d x %d q %d\n", bad, n, max_frames, H, W, quality);
    return bad ? 1 : 0;
}

static std::vector<unsigned char> noise(size_t bytes, unsigned seed) {
    std::vector<unsigned char> v(bytes);
    for (unsigned char& b : v) { seed = seed * 1664525u + 1013904223u; b = (unsigned char)(seed >> 24); }
    return v;
}

static int run(int H, int W, int quality) {
    std::vector<std::vector<unsigned char>> files;
    return encode(1, 1, H, W, quality, noise((size_t)H * W * 3, 1234u + H * 131 + W), files);
}

// three frames (noise, flat, noise) in one call, in one chunk and in chunks of two, against their single-frame encodings
static int run_three(int H, int W, int quality) {
    const size_t frame = (size_t)H * W * 3;
    std::vector<unsigned char> frames = noise(3 * frame, 99u);
    memset(frames.data() + frame, 200, frame);
    std::vector<std::vector<unsigned char>> single, all, one;
    int rc = 0;
    for (int f = 0; f < 3; f++) {
        rc |= encode(1, 1, H, W, quality, std::vector<unsigned char>(frames.begin() + f * frame, frames.begin() + (f + 1) * frame), one);
        if (rc) return rc;
        single.push_back(one[0]);
    }
    for (int max_frames = 2; max_frames <= 3; max_frames++) {
        rc |= encode(max_frames, 3, H, W, quality, frames, all);
        if (rc) return rc;
        if (all != single) { fprintf(stderr, "video writer sanitizer driver: a three-frame call in chunks of %d differs from the single-frame encodings\n", max_frames); rc = 1; }
    }
    return rc;
}

int main() {
    int rc = 0;
    rc |= run(20, 28, 75);        // ragged: a partial MCU row and column
    rc |= run(33, 17, 90);        // overhang: one row and one column past a multiple of 8; frame rows off the word boundary
    rc |= run(64, 64, 100);       // noise at q = 100: a scan longer than the frame
    rc |= run_three(24, 40, 90);
    if (!rc) puts("video writer sanitizer driver: ok");
    return rc;
}
