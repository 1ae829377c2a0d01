// Model-less contexts of the dataset evaluation (frame metrics + VGG19 cosine, LPIPS, FID features): the scaffold every kind is built, sized, created and driven with.
// A kind says what differs -- what it keeps in the persistent arena and what one chunk of frames runs -- and eval_ctx.cpp does the rest once.
#pragma once
#include "net.h"
#include <algorithm>

struct EvalKind {
    int kind, max_frames, H, W;                  // CTX_*; the context's cfg.batch / height / width
    std::function<void(caddy_ctx*)> fill;        // allocates what the kind keeps in c->persist (behind the range-guard flag words): weights, result rows
    std::function<void(caddy_ctx*)> walk;        // one chunk of max_frames frames with null inputs: run on a dry context it sizes the activation arena
    const char* sizer;                           // name of its *_workspace_bytes entry point (error texts)
};
caddy_ctx* eval_ctx_make(const EvalKind& k, void* ws, size_t act_cap);      // ws null: a dry context (nothing is launched, the arenas only count)
void eval_sizes(const EvalKind& k, size_t* persist, size_t* act);           // the dry walk: both arenas rounded to 4 KiB
size_t eval_workspace_bytes(const EvalKind& k);
caddy_ctx* eval_ctx_create(const EvalKind& k, void* workspace, size_t bytes);

// f16 range guard of a split-f16 chunk: reads the flag words [flag0, flag0 + count) behind the stream; a layer that met |x| > 65504 moves onto its forward without a range
// limit for good (layer_fallback).  True when some layer moved -- the flags are cleared and the caller runs the chunk again.
bool range_guard_retry(caddy_ctx* c, int flag0, int count);

// body(n0, nf) for every chunk of at most cfg.batch = max_frames of N frames, until one returns false
template <class Body> void for_chunks(caddy_ctx* c, long N, Body body) {
    const int M = c->cfg.batch;
    for (long n0 = 0; n0 < N; n0 += M) if (!body(n0, (int)std::min<long>(M, N - n0))) return;
}

// ---- the convolution trunks (FID / IS in fid.hip, FVD in fvd.hip): what their states and entry points share ----
struct PackedConv { void* w32 = nullptr; void* w16 = nullptr; float* bias = nullptr; };      // both packed forms and the folded bias of one layer
struct TrunkState {
    bool loaded = false;
    int precision = PREC_F16X3;
    hipEvent_t ev[7] = {};                   // stage boundaries of a timed chunk (trunk_stage_ms)
    bool timed = false, timed_ran = false;
    TrunkState();                            // reads CADDY_PRECISION of the environment: "exact" | "0" selects exact fp32
    ~TrunkState();
    static PackedConv alloc_layer(caddy_ctx* c, size_t weight_bytes, int cout);      // in c->persist
};
int trunk_set_precision(TrunkState& S, int forward, const char* who);
// on: the next chunks record events at the stage boundaries; ms (nullable) receives the `stages` times of the LAST timed chunk
int trunk_stage_ms(caddy_ctx* c, TrunkState& S, int on, float* ms, int stages, const char* who);
// every chunk of n frames through walk(n0, nf); a layer of the split-f16 path that left the f16 range (flag words [0, nflags)) moves to exact fp32 and the chunk runs again.
// copy(n0, nf) fetches a chunk's result.
template <class Walk, class Copy> void trunk_run_chunks(caddy_ctx* c, const TrunkState& S, long n, int nflags, Walk walk, Copy copy) {
    for_chunks(c, n, [&](long n0, int nf) {      // (the activation arena holds max_frames frames)
        for (int attempt = 0; attempt < 2; attempt++) {
            walk(n0, nf);
            if (c->fail) return false;
            if (S.precision == PREC_FP32 || !range_guard_retry(c, 0, nflags)) break;
        }
        copy(n0, nf);
        hipStreamSynchronize(c->stream);
        return true;
    });
}

inline unsigned grid_for(long items) { long b = (items + 255) / 256; return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b)); }      // 256-thread workgroups of a grid-stride kernel
inline int launch_ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }
