// Device-side frame pipeline (frames.hip): uint8 frames -> the model's observation tensor, and the frame writer: fp32 planar frames -> uint8 interleaved frames.  What a FRAMES context keeps besides the scaffold of eval_ctx.h.
#pragma once
#include "net.h"

// One axis of PIL's 8-bit bilinear resize (Resample.c: precompute_coeffs + normalize_coeffs_8bpc): `out` outputs from `in` inputs, `ksize` taps each
struct FrAxis {
    int in = 0, out = 0, ksize = 0;
    std::vector<int> bounds;      // out x (first input index, tap count)
    std::vector<int> kk;          // out x ksize weights in 22 fractional bits
};

struct FramesState {
    int src_h = 0, src_w = 0, l = 0, u = 0, in_w = 0, in_h = 0, W = 0, H = 0;      // source frame, crop origin and size, output size
    bool hpass = false, vpass = false;
    FrAxis ax[2];                 // 0 horizontal, 1 vertical
    // the plan: R output rows per workgroup; block b reads source rows [blk[2b], blk[2b] + blk[2b + 1]) of the crop, at most ns_max; the horizontal pass stages `ch` rows per round
    int R = 0, nblk = 0, ns_max = 0, ch = 0, pitchA = 0, pitchB = 0, lds_used = 0, lds_variant = 0;
    std::vector<int> blk;
    float lut[512] = {};          // byte -> value, mode 0 then mode 1
    int *d_xb = nullptr, *d_xk = nullptr, *d_yb = nullptr, *d_yk = nullptr, *d_blk = nullptr;      // device copies (persistent arena)
    float* d_lut = nullptr;
    unsigned* d_wstats = nullptr; // frame writer (caddy_frames_write): FW_WORDS device words -- the two flags of the map-2 reduction, the counts and the decision of the last call
};
void frames_free(caddy_ctx* c);      // releases caddy_ctx::frs (caddy_ctx_destroy)
