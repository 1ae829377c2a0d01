// TEST ONLY: a stand-alone driver of the example-sheet entry points (csrc/sheets.hip: caddy_sheet_examples, caddy_sheet_strip, caddy_sheet_stats_get) for a sanitizer build
// of that file against the host simulator (tests/test_example_sheets_emu.py builds it with -fsanitize=address,undefined and runs it; nothing here is loaded into python).
// Every buffer is exactly as large as the entry point's contract says, so a read past a plane, a frame or the tensor, or a write past an image row or the image, is reported.
// The image is also checked: every padding byte is 255 and every byte was written (the buffer starts as 0x5A, a value no cell of these inputs produces next to its neighbours).
#include "caddy_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fail(const char* what) { fprintf(stderr, "example sheets sanitizer driver: %s (%s)\n", what, caddy_last_error()); return 1; }

static unsigned char host_byte(float x, bool mapped) {
    volatile float v = x;
    if (mapped) { v = x + 1.0f; v = v * 0.5f; }
    volatile float s = v * 255.0f;
    if (s != s || s < 0.0f) return 0;
    if (s >= 256.0f) return 255;
    return (unsigned char)(int)s;
}

static int run(int B, int T, int S, int H, int W, int f, int lead) {
    const int h = H / f, w = W / f, Trec = T - lead, rows = 2 * (B < 30 ? B : 30);
    const size_t bytes = caddy_sheets_workspace_bytes(rows, T);
    if (!bytes) return fail("workspace size");
    void* raw = nullptr;
    if (posix_memalign(&raw, 256, bytes)) return fail("allocation");
    caddy_ctx* c = caddy_sheets_ctx_create(rows, T, raw, bytes);
    if (!c) return fail("context");
    std::vector<float> obs((size_t)B * T * 3 * S * H * W), rec((size_t)B * Trec * 3 * h * w);
    unsigned seed = 777u + H * 131 + W + f;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) * (2.0f / 16777216.0f) - 1.0f; };
    for (float& v : obs) v = next();
    for (float& v : rec) v = next();
    std::vector<double> lut(768);
    for (int i = 0; i < 768; i++) lut[i] = (i % 256) / 255.0;
    const size_t ih = (size_t)rows * (h + 2) + 2, iw = (size_t)T * (w + 2) + 2;
    std::vector<unsigned char> img(ih * iw * 3);
    int bad = 0;
    for (int weighted = 0; weighted <= (f == 1 ? 1 : 0); weighted++) {
        memset(img.data(), 0x5A, img.size());
        if (caddy_sheet_examples(c, obs.data(), B, T, 3 * S, H, W, rec.data(), Trec, h, w, weighted, 0.25f, weighted ? lut.data() : nullptr, img.data()) != 0) return fail("caddy_sheet_examples");
        unsigned st[5];
        if (caddy_sheet_stats_get(c, st) != 0) return fail("stats");
        if (st[1] != 1 || st[3] != 0 || st[4] != 0) bad++;      // rec is mapped (values in [-1, 1)), no NaN, a valid mask
        for (size_t y = 0; y < ih; y++) for (size_t x = 0; x < iw; x++) {
            const size_t yy = y % (h + 2), xx = x % (w + 2);
            const bool cell = yy >= 2 && xx >= 2 && y < ih - 2 && x < iw - 2;
            const unsigned char* p = &img[(y * iw + x) * 3];
            if (!cell) { if (p[0] != 255 || p[1] != 255 || p[2] != 255) bad++; continue; }
            const int r = (int)(y / (h + 2)), t = (int)(x / (w + 2)), py = (int)yy - 2, px = (int)xx - 2, b = r / 2;
            if (weighted || f != 1 || !(r & 1) || (lead && t == 0)) continue;      // (the reconstruction cells of the plain full-resolution sheet are checked by value)
            for (int ch = 0; ch < 3; ch++)
                if (p[ch] != host_byte(rec[((((size_t)b * Trec + (t - lead)) * 3 + ch) * h + py) * w + px], true)) bad++;
        }
    }
    // the strip on the same context: `rec` as B sequences of Trec frames
    if (B <= rows && Trec <= T) {
        const size_t sh = (size_t)B * (h + 2) + 2, sw = (size_t)Trec * (w + 2) + 2;
        std::vector<unsigned char> strip(sh * sw * 3, 0x5A);
        if (caddy_sheet_strip(c, rec.data(), B, Trec, h, w, 1, strip.data()) != 0) return fail("caddy_sheet_strip");
        for (size_t y = 0; y < sh; y++) for (size_t x = 0; x < sw; x++) {
            const size_t yy = y % (h + 2), xx = x % (w + 2);
            const bool cell = yy >= 2 && xx >= 2 && y < sh - 2 && x < sw - 2;
            const unsigned char* p = &strip[(y * sw + x) * 3];
            if (!cell) { if (p[0] != 255 || p[1] != 255 || p[2] != 255) bad++; continue; }
            const int b = (int)(y / (h + 2)), t = (int)(x / (w + 2)), py = (int)yy - 2, px = (int)xx - 2;
            for (int ch = 0; ch < 3; ch++)
                if (p[ch] != host_byte(rec[((((size_t)b * Trec + t) * 3 + ch) * h + py) * w + px], true)) bad++;
        }
    }
    // the refusals return before anything is touched
    if (caddy_sheet_examples(c, obs.data(), B, T, 3 * S, H, W, rec.data(), Trec + 1 + lead, h, w, 0, 0.f, nullptr, img.data()) != -2) bad++;
    if (caddy_sheet_examples(c, obs.data(), B, T + 1, 3 * S, H, W, rec.data(), T, h, w, 0, 0.f, nullptr, img.data()) != -2) bad++;
    if (caddy_sheet_strip(c, rec.data(), rows + 1, Trec, h, w, 1, img.data()) != -2) bad++;
    caddy_ctx_destroy(c);
    free(raw);
    if (bad) fprintf(stderr, "example sheets sanitizer driver: %d mismatches at B %d T %d S %d %d x %d / %d lead %d\n", bad, B, T, S, H, W, f, lead);
    return bad ? 1 : 0;
}

int main() {
    int rc = 0;
    rc |= run(2, 3, 1, 16, 16, 1, 1);
    rc |= run(2, 3, 2, 16, 16, 2, 1);
    rc |= run(2, 3, 1, 16, 16, 4, 0);       // 4 x 4 cells
    rc |= run(1, 2, 1, 5, 7, 1, 1);         // scalar tails, bases at any byte
    rc |= run(1, 2, 2, 10, 14, 2, 0);       // 5 x 7 cells from 10 x 14: the scalar form of the factor-2 average
    rc |= run(1, 1, 1, 12, 20, 4, 0);       // 3 x 5 cells: the scalar form of the factor-4 average; one column
    rc |= run(31, 2, 1, 8, 8, 1, 1);        // 31 sequences: 60 rows are written, all 31 are read
    rc |= run(1, 2, 1, 3, 260, 1, 1);       // rows longer than one wave's span
    if (!rc) puts("example sheets sanitizer driver: ok");
    return rc;
}
