// TEST ONLY: a stand-alone driver of the per-kernel entry points of csrc/perceptual.hip and csrc/lpips.hip (caddy_k_vgg_*, caddy_k_lpips_*) for a sanitizer build of those files
// against the host simulator (tests/test_vgg_pointwise_emu.py builds it with -fsanitize=address,undefined and runs it; nothing here is loaded into python).
// Every buffer is a heap block of exactly the size the entry point's contract says, so a read or write past a map, a partial slab or an output row is reported: the partial-window
// stores of k_maxpool2_bwd_relu at odd sizes, the `in ? p : 0` addressing of the LPIPS head's tail group, the one-block and capped grids of the per-image sums, the second block
// of the two finalisers.
#include "caddy_hip.h"
#include "common.h"
#include "perceptual.h"
#include "lpips.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int bad = 0;
static void expect(bool ok, const char* what) { if (!ok) { fprintf(stderr, "vgg point-wise sanitizer driver: %s\n", what); bad++; } }

template <class T> struct Buf {      // exactly n elements, 64-byte aligned
    T* p; size_t n;
    explicit Buf(size_t n_) : p(nullptr), n(n_) { void* r = nullptr; if (posix_memalign(&r, 64, n_ * sizeof(T) ? n_ * sizeof(T) : 64)) abort(); p = (T*)r; }
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
};
static unsigned rng_state = 2463534242u;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) * (2.0f / 16777216.0f) - 1.0f; }
static void fill(Buf<float>& b) { for (size_t i = 0; i < b.n; i++) b.p[i] = rnd(); }
// an S16-f16 tensor of the same footprint: every 32 channels as 32 hi halves (0.5, 1, 1.5, ... in f16) and 32 lo halves (0)
static void fill_s16(Buf<float>& b) {
    uint16_t* h = (uint16_t*)b.p;
    for (size_t i = 0; i < 2 * b.n; i++) h[i] = (i & 63) < 32 ? (uint16_t)(0x3800 + 0x0100 * (i % 7)) : 0;
}
static void fill_map(Buf<float>& b, int s16) { if (s16) fill_s16(b); else fill(b); }

static void pool_bwd(int N, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2;
    for (int as = 0; as < 2; as++) for (int zs = 0; zs < 2; zs++) {
        Buf<float> a((size_t)N * H * W * C), gp((size_t)N * Ho * Wo * C), gz((size_t)N * H * W * C);
        fill_map(a, as); fill(gp);
        for (size_t i = 0; i < gz.n; i++) gz.p[i] = NAN;
        expect(caddy_k_vgg_maxpool2_bwd_relu(a.p, as, gp.p, gz.p, zs, N, H, W, C, nullptr) == 0, "maxpool2_bwd_relu status");
        if (as || zs) continue;
        for (int n = 0; n < N; n++) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) for (int c = 0; c < C; c++) {      // the routing rule on the host
            float want = 0.f;
            if (y < 2 * Ho && x < 2 * Wo) {
                const float* w0 = a.p + (((size_t)n * H + (y & ~1)) * W + (x & ~1)) * C + c;
                const float v[4] = {w0[0], w0[C], w0[(size_t)W * C], w0[(size_t)W * C + C]};
                int k = 0;
                for (int j = 1; j < 4; j++) if (v[j] > v[k]) k = j;
                if (k == (y & 1) * 2 + (x & 1) && v[k] > 0.f) want = gp.p[(((size_t)n * Ho + y / 2) * Wo + x / 2) * C + c];
            }
            if (gz.p[(((size_t)n * H + y) * W + x) * C + c] != want) { expect(false, "maxpool2_bwd_relu value"); return; }
        }
    }
    Buf<float> in((size_t)N * H * W * C), out((size_t)N * Ho * Wo * C);
    fill(in);
    expect(caddy_k_vgg_maxpool2(in.p, out.p, N, H, W, C, nullptr) == 0, "maxpool2 status");
}

static void feat_sums(int N, int H, int W, int C) {
    const size_t n = (size_t)N * H * W * C;
    for (int rs = 0; rs < 2; rs++) for (int gs = 0; gs < 2; gs++) {
        Buf<float> rec(n), gt(n), gz(n);
        Buf<double> acc(N), one(1);
        fill_map(rec, rs); fill_map(gt, gs);
        for (int i = 0; i < N; i++) acc.p[i] = 0.0;
        one.p[0] = 0.0;
        expect(caddy_k_vgg_feat_l1_img(rec.p, rs, gt.p, gs, N, H, W, C, acc.p, nullptr) == 0, "feat_l1_img status");
        for (int zs = 0; zs < 2; zs++) expect(caddy_k_vgg_feat_l1(rec.p, rs, gt.p, gs, N, H, W, C, 0.25f, gz.p, zs, one.p, nullptr) == 0, "feat_l1 status");
        expect(caddy_k_vgg_feat_l1(rec.p, rs, gt.p, gs, N, H, W, C, 0.25f, nullptr, 0, one.p, nullptr) == 0, "feat_l1 status (no seed)");
        double s = 0.0;
        for (int i = 0; i < N; i++) s += acc.p[i];
        expect(std::fabs(3.0 * s - one.p[0]) <= 1e-9 * (1.0 + s), "feat_l1 against feat_l1_img");
    }
}

static void feat_cos(int nf) {      // tiny maps, nf = 70: the second block of the finaliser
    const int H[5] = {3, 2, 1, 1, 1}, W[5] = {5, 2, 3, 1, 1}, Cc[5] = {64, 128, 256, 512, 512};
    for (int s = 0; s < 4; s++) {
        Buf<float>* x[5]; Buf<float>* y[5];
        VggCosArgs a{};
        long total = 0;
        for (int l = 0; l < 5; l++) {
            const size_t n = (size_t)nf * H[l] * W[l] * Cc[l];
            x[l] = new Buf<float>(n); y[l] = new Buf<float>(n);
            fill_map(*x[l], s & 1); fill_map(*y[l], s & 2);
            a.x[l] = x[l]->p; a.y[l] = y[l]->p; a.x_s16[l] = s & 1; a.y_s16[l] = (s & 2) >> 1; a.H[l] = H[l]; a.W[l] = W[l]; a.C[l] = Cc[l];
            total += 3L * nf * caddy_k_vgg_cos_blocks(H[l], W[l], Cc[l]);
        }
        Buf<double> part((size_t)total), out(nf);
        expect(caddy_k_vgg_feat_cos(&a, nf, part.p, total, out.p, nullptr) == 0, "feat_cos status");
        expect(caddy_k_vgg_feat_cos(&a, nf, part.p, total - 1, out.p, nullptr) == -1, "feat_cos refusal");
        for (int n = 0; n < nf; n++) expect(out.p[n] >= -1.0 - 1e-9 && out.p[n] <= 1.0 + 1e-9, "feat_cos range");
        for (int l = 0; l < 5; l++) { delete x[l]; delete y[l]; }
    }
}

static void stages_and_copies() {
    const int N = 2, H = 5, W = 7;
    Buf<float> src((size_t)N * 3 * H * W), out((size_t)N * H * W * 4);
    fill(src);
    expect(caddy_k_vgg_metric_stage(src.p, out.p, N, H, W, 1.0f, nullptr) == 0, "metric_stage status");
    expect(caddy_k_lpips_stage(src.p, out.p, N, H, W, 255.0f, nullptr) == 0, "lpips_stage status");
    for (int f = 1; f <= 4; f *= 2) for (int ld = 4; ld <= 12; ld += 8) {
        const int B = 2, Tobs = 4, Trec = 3, Ho = 3, Wo = 5;
        Buf<float> obs((size_t)B * Tobs * f * Ho * f * Wo * ld), o((size_t)B * Trec * Ho * Wo * 4);
        fill(obs);
        TV tv{obs.p, B * Tobs, f * Ho, f * Wo, 3, (long)f * Ho * f * Wo * ld, ld, 0};
        expect(caddy_k_vgg_gt_resize(&tv, o.p, Ho, Wo, B, Tobs, Trec, 1, f, nullptr) == 0, "gt_resize status");
        expect(caddy_k_vgg_gt_resize(&tv, o.p, Ho, Wo, B, Tobs, Trec, 2, f, nullptr) == -1, "gt_resize refusal");
    }
    const int B = 3, Tfull = 5, F4 = 7;
    Buf<float> full((size_t)B * Tfull * F4 * 4);
    fill(full);
    const int t0s[3] = {0, 2, 4}, lens[3] = {2, 3, 1};
    for (int k = 0; k < 3; k++) {
        Buf<float> chunk((size_t)B * lens[k] * F4 * 4);
        expect(caddy_k_vgg_time_chunk(full.p, chunk.p, B, Tfull, F4, t0s[k], lens[k], 0, nullptr) == 0, "time_chunk gather status");
        expect(caddy_k_vgg_time_chunk(full.p, chunk.p, B, Tfull, F4, t0s[k], lens[k], 1, nullptr) == 0, "time_chunk add status");
        expect(caddy_k_vgg_time_chunk(full.p, chunk.p, B, Tfull, F4, t0s[k] + 1, lens[k] + (k == 2 ? 0 : Tfull), 0, nullptr) == -1, "time_chunk refusal");
    }
    Buf<float> a(1000), b(1000);
    fill(a);
    expect(caddy_k_vgg_copy_f(a.p, b.p, 1000, nullptr) == 0 && memcmp(a.p, b.p, 4000) == 0, "copy_f");
}

static void lpips_head(int C, int npix, int blocks) {
    const int nf = 3;
    for (int s = 0; s < 4; s++) {
        Buf<float> f0((size_t)nf * npix * C), f1((size_t)nf * npix * C), w(C);
        Buf<double> part((size_t)nf * blocks), same((size_t)nf * blocks);
        fill_map(f0, s & 1); fill_map(f1, s & 2); fill(w);
        if (!(s & 1)) for (size_t i = 0; i < f0.n; i++) f0.p[i] = std::fabs(f0.p[i]);
        if (!(s & 2)) for (size_t i = 0; i < f1.n; i++) f1.p[i] = std::fabs(f1.p[i]);
        expect(caddy_k_lpips_head(f0.p, s & 1, f1.p, (s & 2) >> 1, w.p, nf, npix, C, blocks, part.p, nullptr) == 0, "lpips_head status");
        expect(caddy_k_lpips_head(f0.p, s & 1, f0.p, s & 1, w.p, nf, npix, C, blocks, same.p, nullptr) == 0, "lpips_head status");
        for (size_t i = 0; i < same.n; i++) expect(same.p[i] == 0.0 && part.p[i] == part.p[i], "lpips_head of identical maps");
    }
}

static void lpips_finalize(int nf) {
    const int blocks[5] = {1, 2, 5, 128, 3}, ldo = nf + 5;
    LpipsLevels lv{};
    long total = 0;
    for (int l = 0; l < 5; l++) { lv.off[l] = total; lv.blocks[l] = blocks[l]; lv.inv_px[l] = 1.0 / (l + 2); total += (long)nf * blocks[l]; }
    Buf<double> part((size_t)total), out((size_t)6 * ldo);
    for (long i = 0; i < total; i++) part.p[i] = rnd();
    for (size_t i = 0; i < out.n; i++) out.p[i] = 7.5;
    expect(caddy_k_lpips_finalize(part.p, &lv, total, nf, out.p, ldo, nullptr) == 0, "lpips_finalize status");
    expect(caddy_k_lpips_finalize(part.p, &lv, total - 1, nf, out.p, ldo, nullptr) == -1, "lpips_finalize refusal");
    for (int r = 0; r < 6; r++) for (int n = nf; n < ldo; n++) expect(out.p[(size_t)r * ldo + n] == 7.5, "lpips_finalize columns >= nf");
}

int main() {
    pool_bwd(1, 7, 9, 64);       // odd sizes: partial windows on the last row and column
    pool_bwd(2, 5, 5, 128);
    pool_bwd(2, 6, 8, 64);
    feat_sums(3, 3, 5, 64);      // n4 < 1024: one block per image
    feat_sums(2, 64, 65, 64);    // the 64-block cap
    feat_cos(70);
    feat_cos(3);
    stages_and_copies();
    lpips_head(64, 23, 2);       // a tail group and a stride trip
    lpips_head(512, 23, 2);
    lpips_head(128, 1, 1);
    lpips_head(256, 70, 5);
    lpips_finalize(70);
    lpips_finalize(3);
    if (!bad) puts("vgg point-wise sanitizer driver: ok");
    return bad ? 1 : 0;
}
