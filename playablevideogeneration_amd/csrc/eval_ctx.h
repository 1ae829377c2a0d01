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
