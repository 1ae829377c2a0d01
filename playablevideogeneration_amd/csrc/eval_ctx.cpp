// Evaluation contexts (eval_ctx.h): the shared scaffold, and the frame-metric, LPIPS and platform-position entry points built on it.  The FID and Inception Score kinds and their entry points live
// with their graph in fid.hip, the FVD kind in fvd.hip; what the driving of those trunks shares (TrunkState) is here.  Nothing here allocates device memory: a context lives in the caller's workspace.
#include "eval_ctx.h"
#include "frame_metrics.h"
#include "detection.h"
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <cstring>

static const size_t FLAG_BYTES = sizeof(unsigned) * 2 * CADDY_N_FLAGS;
static inline size_t round4k(size_t n) { return (n + 4095) & ~(size_t)4095; }

bool ctx_needs(caddy_ctx* c, int kinds, const char* who) {
    if (kinds == CTX_MODEL) {      // (the model entry points take their context unchecked, null included; they only turn the model-less kinds away)
        if (c->kind == CTX_MODEL) return true;
        set_error("a metrics context (caddy_metrics_ctx_create) holds no model");
        return false;
    }
    if (c && (c->kind & kinds)) return true;
    set_error(std::string(who) + " needs a context from " + (kinds & CTX_METRICS ? "caddy_metrics_ctx_create" : kinds & CTX_LPIPS ? "caddy_lpips_ctx_create" : kinds & CTX_FID ? "caddy_fid_ctx_create" : kinds & CTX_IS ? "caddy_is_ctx_create" : kinds & CTX_FRAMES ? "caddy_frames_ctx_create" : kinds & CTX_SHEETS ? "caddy_sheets_ctx_create" : kinds & CTX_VIDEO ? "caddy_video_ctx_create" : kinds & CTX_PNG ? "caddy_png_ctx_create" : kinds & CTX_PNG_READ ? "caddy_png_read_ctx_create" : kinds & CTX_JPEG_READ ? "caddy_jpeg_read_ctx_create" : "caddy_fvd_ctx_create"));
    return false;
}

caddy_ctx* eval_ctx_make(const EvalKind& k, void* ws, size_t act_cap) {
    caddy_ctx* c = new caddy_ctx();
    c->kind = k.kind; c->dry = ws == nullptr;
    c->cfg.batch = k.max_frames; c->cfg.seq_len = 1; c->cfg.height = k.H; c->cfg.width = k.W;
    c->persist.base = (char*)ws; c->persist.cap = (size_t)-1;
    c->sat_flag = (unsigned*)c->persist.alloc(FLAG_BYTES);
    k.fill(c);
    c->act.base = (char*)ws + round4k(c->persist.high); c->act.cap = act_cap; c->grad_delta = 0;      // (grad_delta 0: nothing is back-propagated)
    c->act.reset();
    return c;
}
void eval_sizes(const EvalKind& k, size_t* persist, size_t* act) {
    caddy_ctx* c = eval_ctx_make(k, nullptr, (size_t)1 << 50);
    k.walk(c);
    *persist = round4k(c->persist.high);
    *act = round4k(c->act.high) + 4096;
    caddy_ctx_destroy(c);      // (releases what the kind's fill allocated on the host)
}
size_t eval_workspace_bytes(const EvalKind& k) {
    size_t p, a; eval_sizes(k, &p, &a);
    return p + a + 4096;
}
caddy_ctx* eval_ctx_create(const EvalKind& k, void* workspace, size_t bytes) {
    if (!workspace) { set_error("null buffer"); return nullptr; }
    if ((uintptr_t)workspace & 255) { set_error("the workspace must be 256-byte aligned"); return nullptr; }
    size_t p, a; eval_sizes(k, &p, &a);
    if (bytes < p + a) { set_error(std::string("workspace too small (see ") + k.sizer + ")"); return nullptr; }
    caddy_ctx* c = eval_ctx_make(k, workspace, a);
    hipMemset(c->sat_flag, 0, FLAG_BYTES);
    return c;
}

bool range_guard_retry(caddy_ctx* c, int flag0, int count) {
    unsigned v[CADDY_N_FLAGS];
    assert(flag0 >= 0 && count >= 0 && flag0 + count <= CADDY_N_FLAGS);
    hipMemcpyAsync(v, c->sat_flag + flag0, sizeof(unsigned) * count, hipMemcpyDeviceToHost, c->stream);
    hipStreamSynchronize(c->stream);
    bool again = false;
    for (int i = 0; i < count; i++) if (v[i] && !c->layer_fallback[flag0 + i]) { c->layer_fallback[flag0 + i] = true; c->n_fallback++; again = true; }
    if (again) hipMemsetAsync(c->sat_flag, 0, FLAG_BYTES, c->stream);
    return again;
}

TrunkState::TrunkState() {
    if (const char* e = getenv("CADDY_PRECISION")) if (!strcmp(e, "exact") || !strcmp(e, "0")) precision = PREC_FP32;
}
TrunkState::~TrunkState() {
    for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
}
PackedConv TrunkState::alloc_layer(caddy_ctx* c, size_t weight_bytes, int cout) {
    PackedConv L;
    L.w32 = c->persist.alloc(weight_bytes); L.w16 = c->persist.alloc(weight_bytes);
    L.bias = (float*)c->persist.alloc((size_t)cout * 4);
    return L;
}
int trunk_set_precision(TrunkState& S, int forward, const char* who) {
    if (forward != PREC_FP32 && forward != PREC_F16X3) { set_error(std::string(who) + ": 0 (exact fp32) | 16 (split f16)"); return -2; }
    S.precision = forward;
    return 0;
}
int trunk_stage_ms(caddy_ctx* c, TrunkState& S, int on, float* ms, int stages, const char* who) {
    if (ms) {
        if (!S.timed_ran) { set_error(std::string(who) + ": no timed chunk has run"); return -2; }
        hipStreamSynchronize(c->stream);
        for (int k = 0; k < stages; k++) hipEventElapsedTime(ms + k, S.ev[k], S.ev[k + 1]);
    }
    if (on && !S.ev[0]) for (int k = 0; k <= stages; k++) hipEventCreate(&S.ev[k]);
    S.timed = on != 0;
    if (!on) S.timed_ran = false;
    return 0;
}

// The two VGG kinds read the VGG switches of the environment once, when a context is created (c null: creation failed)
static caddy_ctx* vgg_env(caddy_ctx* c) {
    if (!c) return c;
    if (const char* e = getenv("CADDY_VGG_S16")) c->vgg_s16 = atoi(e) != 0;
    if (const char* e = getenv("CADDY_PRECISION")) if (!strcmp(e, "exact") || !strcmp(e, "0")) c->vgg_precision = c->vgg_precision_bwd = PREC_FP32;
    return c;
}

// Frame-metrics kind (caddy_metrics_ctx_create): the fused frame-metric pass's slab and result rows for max_frames frames, and with vgg the packed VGG19 weights plus the
// activation arena of one chunk of the cosine similarity (vgg_metric_chunk's walk)
static bool metrics_args_ok(int max_frames, int H, int W, int vgg) {
    FmGeom g;
    if (max_frames < 1 || H < 1 || W < 1) { set_error("caddy_metrics: max_frames, height and width must be positive"); return false; }
    if (!fm_geometry(H, W, &g)) { set_error("caddy_metrics: frames smaller than the 11x11 SSIM window (after SSIM's down-sampling)"); return false; }
    if (vgg && (H % 16 || W % 16)) { set_error("caddy_metrics: the VGG19 cosine similarity needs height and width multiples of 16 (four 2x2 max-pools)"); return false; }
    return true;
}
static EvalKind metrics_kind(int max_frames, int H, int W, int vgg) {
    return {CTX_METRICS, max_frames, H, W,
            [=](caddy_ctx* c) {
                c->cfg.perceptual = vgg ? 1 : 0;
                if (vgg) vgg_build(c);
                FmGeom g;
                fm_geometry(H, W, &g);
                c->fm_slab = (double*)c->persist.alloc(sizeof(double) * FM_PART * (size_t)max_frames * g.tx * g.ty);
                c->fm_out = (double*)c->persist.alloc(sizeof(double) * FM_SLOTS * (size_t)max_frames);
            },
            [=](caddy_ctx* c) { if (vgg) vgg_metric_chunk(c, nullptr, nullptr, max_frames, 1.f, nullptr); },
            "caddy_metrics_workspace_bytes"};
}

// LPIPS kind (caddy_lpips_ctx_create; evaluation/metrics/lpips.py:14,33): the VGG state is the VGG16-to-relu5_3 trunk plus the five lin vectors; the activation arena of one
// chunk of vgg_lpips_chunk's walk and 6 x max_frames result doubles
#define LPIPS_ROWS 6
static bool lpips_args_ok(int max_frames, int H, int W) {
    if (max_frames < 1 || H < 1 || W < 1) { set_error("caddy_lpips: max_frames, height and width must be positive"); return false; }
    if (H % 16 || W % 16) { set_error("caddy_lpips: LPIPS (VGG16) needs height and width multiples of 16 (four 2x2 max-pools)"); return false; }
    return true;
}
static EvalKind lpips_kind(int max_frames, int H, int W) {
    return {CTX_LPIPS, max_frames, H, W,
            [=](caddy_ctx* c) {
                c->cfg.perceptual = 1;
                vgg_build(c, VGG_KIND_LPIPS);
                c->fm_out = (double*)c->persist.alloc(sizeof(double) * FM_SLOTS * (size_t)max_frames);      // (FM_SLOTS >= LPIPS_ROWS rows: caddy_platform_positions keeps working on it)
            },
            [=](caddy_ctx* c) { vgg_lpips_chunk(c, nullptr, nullptr, max_frames, 1.f, nullptr, max_frames); },
            "caddy_lpips_workspace_bytes"};
}

extern "C" {
size_t caddy_lpips_workspace_bytes(int max_frames, int height, int width) {
    return lpips_args_ok(max_frames, height, width) ? eval_workspace_bytes(lpips_kind(max_frames, height, width)) : 0;
}
caddy_ctx* caddy_lpips_ctx_create(int max_frames, int height, int width, void* workspace, size_t bytes) {
    return lpips_args_ok(max_frames, height, width) ? vgg_env(eval_ctx_create(lpips_kind(max_frames, height, width), workspace, bytes)) : nullptr;
}
int caddy_lpips_param_count(void) { return lpips_param_count(); }
int caddy_lpips_param_info_get(int index, caddy_param_info* out) { return lpips_param_info(index, out); }
long caddy_lpips_param_floats(void) { return lpips_param_floats(); }
int caddy_load_lpips(caddy_ctx* c, const float* lpips_flat) {
    if (!ctx_needs(c, CTX_LPIPS, "caddy_load_lpips")) return -2;
    c->fail = false;
    if (!lpips_flat) { set_error("null input"); return -2; }
    return vgg_load(c, lpips_flat);
}
int caddy_debug_lpips_tap_formats(caddy_ctx* c) { return (c && c->kind == CTX_LPIPS) ? (int)c->vgg.tap_s16 : -1; }
int caddy_frame_lpips(caddy_ctx* c, const float* ref, const float* gen, int B, int T, float value_range, double* out_host) {
    if (!ctx_needs(c, CTX_LPIPS, "caddy_frame_lpips")) return -2;
    c->fail = false;
    if (!ref || !gen || !out_host) { set_error("null input"); return -2; }
    if (B < 1 || T < 1 || !(value_range > 0.f)) { set_error("caddy_frame_lpips: B, T and value_range must be positive"); return -2; }
    if (!c->vgg.loaded) { set_error("caddy_frame_lpips: no LPIPS weights were loaded (caddy_load_lpips)"); return -2; }
    const int M = c->cfg.batch;
    const long N = (long)B * T, fr = 3L * c->cfg.height * c->cfg.width;
    hipStream_t st = c->stream;
    std::vector<double> tmp((size_t)LPIPS_ROWS * M);
    c->vgg.tap_s16 = 0;
    for_chunks(c, N, [&](long n0, int nf) {      // (the arena of the VGG16 trunk holds max_frames frames)
        // a layer of the split-f16 forward that left the f16 range moves to split bf16 and the chunk runs again
        for (int attempt = 0; attempt < 2; attempt++) {
            if (vgg_lpips_chunk(c, ref + n0 * fr, gen + n0 * fr, nf, value_range, c->fm_out, M) != 0) return false;
            if (!range_guard_retry(c, CADDY_VGG_FLAG0, VGG_NCONV)) break;
        }
        hipMemcpyAsync(tmp.data(), c->fm_out, sizeof(double) * LPIPS_ROWS * M, hipMemcpyDeviceToHost, st);
        hipStreamSynchronize(st);
        for (int s = 0; s < LPIPS_ROWS; s++)
            for (int j = 0; j < nf; j++) out_host[s * N + n0 + j] = tmp[(size_t)s * M + j];
        return true;
    });
    return finish(c);
}
size_t caddy_metrics_workspace_bytes(int max_frames, int height, int width, int vgg) {
    return metrics_args_ok(max_frames, height, width, vgg) ? eval_workspace_bytes(metrics_kind(max_frames, height, width, vgg)) : 0;
}
caddy_ctx* caddy_metrics_ctx_create(int max_frames, int height, int width, int vgg, void* workspace, size_t bytes) {
    return metrics_args_ok(max_frames, height, width, vgg) ? vgg_env(eval_ctx_create(metrics_kind(max_frames, height, width, vgg), workspace, bytes)) : nullptr;
}
int caddy_frame_metrics(caddy_ctx* c, const float* ref, const float* gen, int B, int T, float value_range, int want_vgg, double* out_host) {
    if (!ctx_needs(c, CTX_METRICS, "caddy_frame_metrics")) return -2;
    c->fail = false;
    if (!ref || !gen || !out_host) { set_error("null input"); return -2; }
    if (B < 1 || T < 1 || !(value_range > 0.f)) { set_error("caddy_frame_metrics: B, T and value_range must be positive"); return -2; }
    if (want_vgg && !(c->cfg.perceptual && c->vgg.loaded)) { set_error("caddy_frame_metrics: want_vgg needs a context created with vgg = 1 and loaded VGG19 weights (caddy_load_vgg)"); return -2; }
    FmGeom g;
    if (!fm_geometry(c->cfg.height, c->cfg.width, &g)) { set_error("caddy_metrics: frames smaller than the 11x11 SSIM window (after SSIM's down-sampling)"); return -2; }
    const int M = c->cfg.batch;
    const long N = (long)B * T, fr = 3L * c->cfg.height * c->cfg.width;
    hipStream_t st = c->stream;
    std::vector<double> tmp((size_t)FM_SLOTS * M);
    for_chunks(c, N, [&](long n0, int nf) {      // (the slab of the fused pass and the arena of the VGG19 branch hold max_frames frames)
        c->ck(fm_launch(ref, gen, (int)n0, nf, T, g, value_range, c->fm_slab, c->fm_out, M, st), "frame metrics");
        // a VGG19 layer of the split-f16 forward that left the f16 range moves to split bf16 (as caddy_f16_saturated does) and the chunk runs again
        for (int attempt = 0; want_vgg && attempt < 2; attempt++) {
            if (vgg_metric_chunk(c, ref + n0 * fr, gen + n0 * fr, nf, value_range, c->fm_out + (size_t)CADDY_FM_VGG_SIM * M) != 0) return false;
            if (!range_guard_retry(c, CADDY_VGG_FLAG0, VGG_NCONV)) break;
        }
        hipMemcpyAsync(tmp.data(), c->fm_out, sizeof(double) * FM_SLOTS * M, hipMemcpyDeviceToHost, st);
        hipStreamSynchronize(st);
        for (int s = 0; s < FM_SLOTS; s++)
            for (int j = 0; j < nf; j++) out_host[s * N + n0 + j] = (s == CADDY_FM_VGG_SIM && !want_vgg) ? NAN : tmp[(size_t)s * M + j];
        return true;
    });
    return finish(c);
}

int caddy_platform_positions(caddy_ctx* c, const float* obs, int B, int T, int row, float lo, float hi, int min_run, int* out_host) {
    if (!ctx_needs(c, CTX_METRICS | CTX_LPIPS, "caddy_platform_positions")) return -2;
    c->fail = false;
    if (!obs || !out_host) { set_error("null input"); return -2; }
    const int H = c->cfg.height, W = c->cfg.width;
    if (B < 1 || T < 1) { set_error("caddy_platform_positions: B and T must be positive"); return -2; }
    if (row < 0 || row >= H) { set_error("caddy_platform_positions: row outside the frame (0 <= row < height)"); return -2; }
    if (min_run < 1) { set_error("caddy_platform_positions: min_run must be positive"); return -2; }
    if (W > DET_MAX_W) { set_error("caddy_platform_positions: frames wider than 4096 columns"); return -2; }
    hipStream_t st = c->stream;
    int* dev = (int*)c->fm_out;      // (FM_SLOTS doubles = 72 bytes per frame: room for one int32 each)
    for_chunks(c, (long)B * T, [&](long n0, int nf) {
        c->ck(det_platform_launch(obs, (int)n0, nf, H, W, row, lo, hi, min_run, dev, st), "platform positions");
        hipMemcpyAsync(out_host + n0, dev, sizeof(int) * nf, hipMemcpyDeviceToHost, st);
        hipStreamSynchronize(st);
        return true;
    });
    return finish(c);
}
}
