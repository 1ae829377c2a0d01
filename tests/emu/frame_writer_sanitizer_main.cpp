// TEST ONLY: a stand-alone driver of the frame writer's entry points (csrc/frames.hip: caddy_frames_write, caddy_frames_write_stats_get) for a sanitizer build of that
// file against the host simulator (tests/test_frame_writer_emu.py builds it with -fsanitize=address,undefined and runs it; nothing here is loaded into python).
// Every buffer is exactly as large as the entry point's contract says, so a read or write past a row, a plane, a frame or the stats block is reported.
#include "caddy_hip.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fail(const char* what) { fprintf(stderr, "frame writer sanitizer driver: %s (%s)\n", what, caddy_last_error()); return 1; }

static unsigned char host_byte(float x, bool mapped) {
    volatile float v = x;
    if (mapped) { v = x + 1.0f; v = v * 0.5f; }
    volatile float s = v * 255.0f;
    if (s != s || s < 0.0f) return 0;
    if (s >= 256.0f) return 255;
    return (unsigned char)(int)s;
}

static int run(int H, int W, int B, int Trec, bool with_first, int S) {
    const int T = Trec + (with_first ? 1 : 0), max_frames = B * T;
    std::vector<float> lut(512);
    for (int i = 0; i < 256; i++) { lut[i] = ((i / 255.0f) - 0.5f) / 0.5f; lut[256 + i] = i / 255.0f; }
    const size_t bytes = caddy_frames_workspace_bytes(max_frames, H, W, nullptr, H, W);
    if (!bytes) return fail("workspace size");
    void* raw = nullptr;
    if (posix_memalign(&raw, 256, bytes)) return fail("allocation");
    caddy_ctx* c = caddy_frames_ctx_create(max_frames, H, W, nullptr, H, W, lut.data(), raw, bytes);
    if (!c) return fail("context");
    const long fr = 3L * H * W, stride = (long)T * 3 * S * H * W;
    std::vector<float> rec((size_t)B * Trec * fr), obs(with_first ? (size_t)B * stride : 0);
    unsigned seed = 12345u + H * 131 + W;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) * (2.0f / 16777216.0f) - 1.0f; };
    for (float& v : rec) v = next();
    for (float& v : obs) v = next();
    rec[rec.size() / 2] = NAN; rec[1] = 3.0f; rec[rec.size() - 1] = -7.0f;
    std::vector<unsigned char> u8((size_t)B * T * H * W * 3);
    std::vector<float> f32((size_t)B * T * fr);
    int bad = 0;
    for (int map = 0; map <= 2; map++)
        for (int outs = 1; outs <= 3; outs++) {
            memset(u8.data(), 0xAB, u8.size());
            if (caddy_frames_write(c, rec.data(), B, Trec, with_first ? obs.data() : nullptr, stride, map, outs & 1 ? u8.data() : nullptr, outs & 2 ? f32.data() : nullptr) != 0)
                return fail("caddy_frames_write");
            unsigned st[3];
            if (caddy_frames_write_stats_get(c, st) != 0) return fail("stats");
            const bool mapped = map == 1;      // (map 2: the NaN in rec means no mapping)
            if ((st[0] != 0) != mapped || st[2] != 1) bad++;
            if (!(outs & 1)) continue;
            for (int b = 0; b < B; b++) for (int t = 0; t < T; t++) for (int ch = 0; ch < 3; ch++) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
                const float* src = (with_first && t == 0) ? obs.data() + b * stride : rec.data() + ((long)b * Trec + (t - (with_first ? 1 : 0))) * fr;
                const unsigned char want = host_byte(src[((long)ch * H + y) * W + x], mapped);
                if (u8[((((size_t)b * T + t) * H + y) * W + x) * 3 + ch] != want) bad++;
            }
        }
    // the refusals return before anything is touched
    if (caddy_frames_write(c, rec.data(), B, Trec, nullptr, 0, 3, u8.data(), nullptr) != -2) bad++;
    if (caddy_frames_write(c, rec.data(), B, Trec, nullptr, 0, 1, nullptr, nullptr) != -2) bad++;
    if (caddy_frames_write(c, rec.data(), B + 1, Trec + 1, nullptr, 0, 1, u8.data(), nullptr) != -2) bad++;
    caddy_ctx_destroy(c);
    free(raw);
    if (bad) fprintf(stderr, "frame writer sanitizer driver: %d mismatches at %d x %d\n", bad, H, W);
    return bad ? 1 : 0;
}

int main() {
    int rc = 0;
    rc |= run(5, 7, 2, 3, true, 2);        // scalar tails, frame bases at any byte
    rc |= run(16, 53, 2, 2, false, 1);
    rc |= run(8, 12, 1, 1, true, 1);
    rc |= run(3, 260, 2, 1, true, 1);      // rows longer than one wave's span
    if (!rc) puts("frame writer sanitizer driver: ok");
    return rc;
}
