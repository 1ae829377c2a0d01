// Evaluation example sheets: the contact sheets the reference's evaluator saves before it computes its losses, composed on the device from the fp32 tensors the forward pass
// left there -- only the finished uint8 image crosses the bus.
//
// Reference: evaluation/evaluator.py:115-147 ("Saving sample images"), save_examples :392-436 (ground truth / reconstruction rows at every output resolution),
// save_examples_with_weights :314-376 + upscale_and_color_weights :270-301 + blend_tensors :303-312 (the motion-weight mask blended over the frames),
// check_and_normalize_range :378-390, training/losses.py:604-649 (MotionLossWeightMaskCalculator.compute_weight_mask) and torchvision's make_grid(list, nrow = T, padding = 2,
// pad_value = 1).  The strip (caddy_sheet_strip) is the same grid with one row per sequence, for interpolate.py:102-158.
//
// Layout: R rows of T cells of h x w; the image is (R (h + 2) + 2, T (w + 2) + 2, 3) uint8 interleaved, cell (r, t) starts at pixel (r (h + 2) + 2, t (w + 2) + 2), every other
// pixel is 255.  Row 2 b is the ground truth of sequence b (channels 0..2 of the observation tensor, resized), row 2 b + 1 its reconstruction; with Trec = T - 1 column 0 of a
// reconstruction row is the mapped ground-truth frame 0.  Only the first min(B, 30) sequences are drawn; every decision below covers all B.
//
// Arithmetic, each operation rounded as written and nothing contracted:
//   resize   F.interpolate(mode = "bilinear", align_corners = False) on the CPU for the factors 1, 2, 4: a copy; ((0.25 a + 0.25 b) + 0.25 c) + 0.25 d over the source pixels
//            (2y, 2x), (2y, 2x + 1), (2y + 1, 2x), (2y + 1, 2x + 1); the same form over (4y + 1, 4x + 1), (4y + 1, 4x + 2), (4y + 2, 4x + 1), (4y + 2, 4x + 2)
//   range    (x + 1) / 2 for a tensor whose minimum is negative, decided per tensor (the resized ground truth; the reconstruction); a NaN means no mapping, -0.0 is not negative
//   byte     (int)(v * 255.0f), the frame writer's rules (frames.hip: fw_byte): s < 0 -> 0, s >= 256 -> 255, NaN -> 0, each counted
//   mask     t >= 1: m = ((d_0 + d_1) + d_2) + bias with d_c = |gt_t - gt_{t-1}| + |rec'_t - rec'_{t-1}| on the unmapped tensors, rec'_0 = gt_0 when Trec = T - 1; m = 1 at t = 0;
//            w = m / max |m| over the whole batch; col = lut[min((int)(w * 256.0f), 255)] (256 x 3 doubles: matplotlib's viridis table);
//            v = (double)(x * 0.4f) + col * 0.6 on the mapped frame x, byte = (int)(v * 255.0) with the same saturation rules; a NaN or a negative m is flagged
//
// Launches: a reduction (k_sheet_reduce: the four range flags and the mask's validity, folded per workgroup before one atomicOr each, and one partial maximum per workgroup, a
// plain store -- the kernel boundary publishes them) and the compose launch (k_sheet_compose), which folds the partial maxima (four L2-resident loads per lane; 16 bytes of
// LDS for a fold, the only LDS here) and writes every byte of the image once,
// padding included: a work item is (cell, row of the cell's (h + 4) x (w + 4) neighbourhood, group); group 0 is the 2 padding pixels left of the cell, groups 1..ceil(w / 4) take 4
// consecutive pixels (three 16-byte plane loads per source, 12 bytes packed into three dword stores when the destination is 4-byte aligned, bytes otherwise -- image rows are
// 3 (T (w + 2) + 2) bytes, so most cells start off a dword), the last group is the right edge of the last column; rows 0..1 are the padding above the cell, rows h + 2..h + 3 the
// bottom edge of the last row.  Consecutive lanes write consecutive bytes.  Memory-bound; no atomics on the image; the counts are integer atomics, so a call is deterministic.
#include "eval_ctx.h"
#include "sheets.h"

namespace {

enum { SH_NEG_GT = 0, SH_NAN_GT, SH_NEG_REC, SH_NAN_REC, SH_MASK_BAD, SH_SATURATED, SH_NANS, SH_MAPPED_GT, SH_MAPPED_REC, SH_WORDS = 16 };
constexpr int SH_THREADS = 256, SH_WAVES = SH_THREADS / 64, SH_RED_BLOCKS = 1024, SH_MAX_SEQUENCES = 30;
constexpr int SH_MAX_SIDE = 1 << 15;      // keeps every per-cell index below 2^31
constexpr unsigned SH_ONE_BITS = 0x3f800000u;

struct ShArgs {
    const float *obs, *rec;      // obs (B, T, C, H, W); rec (B, Trec, 3, h, w) -- the strip's frames are `rec` with Trec = T and no obs
    long obs_frame;              // C H W: floats from one (b, t) of obs to the next
    int B, T, Trec, H, W, h, w, f, ngx, rows, strip, map, weighted;
    float bias;
    const double* lut;
    unsigned *words, *slab; int nslab;
    uint8_t* out; long pitch;    // bytes per image row
    int dom_w, dom;              // work items per cell: (h + 4) rows of ngx + 2 groups
};

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte load at a 4-byte aligned address

__device__ __forceinline__ void load4(const float* s, int cnt, float v[4]) {
    if (cnt == 4) { const f32x4u t = *(const f32x4u*)s; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = j < cnt ? s[j] : 0.f;
    }
}
__device__ __forceinline__ float avg4(float a, float b, float c, float d) {
#pragma clang fp contract(off)
    return ((0.25f * a + 0.25f * b) + 0.25f * c) + 0.25f * d;
}
// `cnt` resized values of the H x W plane p: output row y, pixels 4 xg .. 4 xg + cnt - 1 (f = 1, 2, 4; H = f h, W = f w)
__device__ __forceinline__ void gt_group(const float* p, int W, int f, int y, int xg, int cnt, float v[4]) {
    if (f == 1) { load4(p + (long)y * W + 4 * xg, cnt, v); return; }
    const int o = f == 2 ? 0 : 1;      // the first of the two source rows / columns inside an f x f block
    const float* r0 = p + (long)(f * y + o) * W + (long)f * 4 * xg;
    const float* r1 = r0 + W;
    if (cnt == 4 && f == 2) {
        const f32x4u a0 = *(const f32x4u*)r0, a1 = *(const f32x4u*)(r0 + 4), b0 = *(const f32x4u*)r1, b1 = *(const f32x4u*)(r1 + 4);
        v[0] = avg4(a0.x, a0.y, b0.x, b0.y); v[1] = avg4(a0.z, a0.w, b0.z, b0.w);
        v[2] = avg4(a1.x, a1.y, b1.x, b1.y); v[3] = avg4(a1.z, a1.w, b1.z, b1.w);
    } else if (cnt == 4) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const f32x4u a = *(const f32x4u*)(r0 + 4 * j), b = *(const f32x4u*)(r1 + 4 * j);
            v[j] = avg4(a.y, a.z, b.y, b.z);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = j < cnt ? avg4(r0[f * j + o], r0[f * j + o + 1], r1[f * j + o], r1[f * j + o + 1]) : 0.f;
    }
}

// where frame t of row kind `rec` of sequence b lies: a ground-truth row, or column 0 of a reconstruction that is one frame short, reads obs (and resizes); else rec
struct ShSrc { const float* p; long plane; bool gt; };
__device__ __forceinline__ ShSrc sh_src(const ShArgs& a, int b, int t, bool rec) {
    const int lead = a.T - a.Trec;
    if (!rec || (lead && t == 0)) return {a.obs + ((long)b * a.T + t) * a.obs_frame, (long)a.H * a.W, true};
    return {a.rec + ((long)b * a.Trec + (t - lead)) * 3 * a.h * a.w, (long)a.h * a.w, false};
}
__device__ __forceinline__ void sh_load(const ShArgs& a, const ShSrc& s, int c, int y, int xg, int cnt, float v[4]) {
    if (s.gt) gt_group(s.p + c * s.plane, a.W, a.f, y, xg, cnt, v);
    else load4(s.p + c * s.plane + (long)y * a.w + 4 * xg, cnt, v);
}

// the unnormalised mask of sequence b at t >= 1 (full resolution); cur[c] receives frame t of the row kind `rec`, which the caller draws
__device__ __forceinline__ void mask_group(const ShArgs& a, int b, int t, int y, int xg, int cnt, bool rec, float m[4], float cur[3][4]) {
#pragma clang fp contract(off)
    const ShSrc g1 = sh_src(a, b, t, false), g0 = sh_src(a, b, t - 1, false), r1 = sh_src(a, b, t, true), r0 = sh_src(a, b, t - 1, true);
    float d[3][4];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float p[4], q[4], u[4], s[4];
        sh_load(a, g1, c, y, xg, cnt, p); sh_load(a, g0, c, y, xg, cnt, q);
        sh_load(a, r1, c, y, xg, cnt, u); sh_load(a, r0, c, y, xg, cnt, s);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            d[c][j] = fabsf(p[j] - q[j]) + fabsf(u[j] - s[j]);
            cur[c][j] = rec ? u[j] : p[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) m[j] = ((d[0][j] + d[1][j]) + d[2][j]) + a.bias;
}

// the maximum (IS_OR: the bitwise OR) over the workgroup, in every thread (every thread of the workgroup calls it)
template <bool IS_OR> __device__ __forceinline__ unsigned block_fold(unsigned v, unsigned* lds4) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { const unsigned o = __shfl_xor(v, s); v = IS_OR ? (v | o) : (o > v ? o : v); }
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned r = lds4[0];
#pragma unroll
    for (int k = 1; k < SH_WAVES; k++) r = IS_OR ? (r | lds4[k]) : (lds4[k] > r ? lds4[k] : r);
    return r;
}

// first launch: is any value of the resized ground truth / of the reconstruction negative, is any a NaN (-0.0 < 0 and NaN < 0 are false, as on the host); with `weighted`
// the mask's validity and this workgroup's maximum of the bit patterns of |m| (m >= 0 orders like its bits; a NaN lies above every number, as torch.max returns it)
__global__ __launch_bounds__(SH_THREADS) void k_sheet_reduce(ShArgs a) {
    __shared__ unsigned lds4[SH_WAVES], lds4b[SH_WAVES];
    const long tid = (long)blockIdx.x * SH_THREADS + threadIdx.x, nth = (long)gridDim.x * SH_THREADS;
    const long gpp = (long)a.h * a.ngx;      // groups per output plane
    bool neg_gt = false, nan_gt = false, neg_rec = false, nan_rec = false, bad = false;
    unsigned mx = SH_ONE_BITS;               // (t = 0: m = 1)
    for (long i = tid; i < (long)a.B * a.T * 3 * gpp; i += nth) {
        const long pl = i / gpp, bt = pl / 3;
        const int g = (int)(i - pl * gpp), c = (int)(pl - bt * 3), y = g / a.ngx, xg = g - y * a.ngx;
        const int cnt = a.w - 4 * xg < 4 ? a.w - 4 * xg : 4;
        float v[4];
        gt_group(a.obs + bt * a.obs_frame + (long)c * a.H * a.W, a.W, a.f, y, xg, cnt, v);
#pragma unroll
        for (int j = 0; j < 4; j++) if (j < cnt) { neg_gt |= v[j] < 0.f; nan_gt |= v[j] != v[j]; }
    }
    const long n_rec = (long)a.B * a.Trec * 3 * a.h * a.w;
    for (long i = tid; i < (n_rec + 3) >> 2; i += nth) {
        const long e = i * 4;
        const int cnt = n_rec - e < 4 ? (int)(n_rec - e) : 4;
        float v[4];
        load4(a.rec + e, cnt, v);
#pragma unroll
        for (int j = 0; j < 4; j++) if (j < cnt) { neg_rec |= v[j] < 0.f; nan_rec |= v[j] != v[j]; }
    }
    if (a.weighted) {
        for (long i = tid; i < (long)a.B * (a.T - 1) * gpp; i += nth) {
            const long bt = i / gpp, b = bt / (a.T - 1);
            const int g = (int)(i - bt * gpp), t = 1 + (int)(bt - b * (a.T - 1)), y = g / a.ngx, xg = g - y * a.ngx;
            const int cnt = a.w - 4 * xg < 4 ? a.w - 4 * xg : 4;
            float m[4], cur[3][4];
            mask_group(a, (int)b, t, y, xg, cnt, false, m, cur);
#pragma unroll
            for (int j = 0; j < 4; j++) if (j < cnt) {
                bad |= !(m[j] >= 0.f);
                const unsigned u = __float_as_uint(m[j]) & 0x7fffffffu;
                mx = u > mx ? u : mx;
            }
        }
    }
    // one atomic per workgroup and flag, not one per thread: on frames in [-1, 1] every thread has seen a negative value
    const unsigned flags = block_fold<true>((neg_gt ? 1u : 0u) | (nan_gt ? 2u : 0u) | (neg_rec ? 4u : 0u) | (nan_rec ? 8u : 0u) | (bad ? 16u : 0u), lds4b);
    if (threadIdx.x == 0) {
        if (flags & 1u) atomicOr(a.words + SH_NEG_GT, 1u);
        if (flags & 2u) atomicOr(a.words + SH_NAN_GT, 1u);
        if (flags & 4u) atomicOr(a.words + SH_NEG_REC, 1u);
        if (flags & 8u) atomicOr(a.words + SH_NAN_REC, 1u);
        if (flags & 16u) atomicOr(a.words + SH_MASK_BAD, 1u);
    }
    mx = block_fold<false>(mx, lds4);
    if (threadIdx.x == 0) a.slab[blockIdx.x] = mx;
}

// the frame writer's fw_byte (frames.hip), operation by operation: nothing here may be contracted or reassociated
__device__ __forceinline__ float sh_map(float x, bool mapped) {
#pragma clang fp contract(off)
    float v = x;
    if (mapped) { v = x + 1.0f; v = v * 0.5f; }
    return v;
}
__device__ __forceinline__ uint32_t sh_byte(float v, unsigned& saturated, unsigned& nans) {
#pragma clang fp contract(off)
    const float s = v * 255.0f;
    if (s != s) { nans++; return 0u; }
    if (s < 0.0f) { saturated++; return 0u; }
    if (s >= 256.0f) { saturated++; return 255u; }
    return (uint32_t)(int)s;
}
// the blended byte: first * (1 - 0.6) is an fp32 product, the colour and the sum are doubles (the reference blends a float32 tensor with a float64 one)
__device__ __forceinline__ uint32_t sh_blend_byte(float v, double col, unsigned& saturated, unsigned& nans) {
#pragma clang fp contract(off)
    const float first = v * 0.4f;
    const double second = col * 0.6;
    const double sum = (double)first + second;
    const double s = sum * 255.0;
    if (s != s) { nans++; return 0u; }
    if (s < 0.0) { saturated++; return 0u; }
    if (s >= 256.0) { saturated++; return 255u; }
    return (uint32_t)(int)s;
}

// one work item of one cell: row yy of the cell's neighbourhood (2 padding rows, h rows, the bottom edge), group gg (the left padding, ngx groups, the right edge)
__device__ __forceinline__ void compose_item(const ShArgs& a, int cell, int yy, int gg, bool map_gt, bool map_rec, float mmax, unsigned& saturated, unsigned& nans) {
#pragma clang fp contract(off)
    const int T = a.T, h = a.h, w = a.w;
    const int r = cell / T, t = cell - r * T;
    if (yy >= h + 2 && r != a.rows - 1) return;
    if (gg == a.ngx + 1 && t != T - 1) return;
    const bool edge = gg == 0 || gg == a.ngx + 1;
    const int xg = gg - 1, y = yy - 2;
    const int cnt = edge ? 2 : (w - 4 * xg < 4 ? w - 4 * xg : 4);
    const int x0 = gg == 0 ? t * (w + 2) : gg == a.ngx + 1 ? T * (w + 2) : t * (w + 2) + 2 + 4 * xg;
    uint8_t* o = a.out + ((long)r * (h + 2) + yy) * a.pitch + 3L * x0;
    const bool dwords = cnt == 4 && ((uintptr_t)o & 3) == 0;
    if (edge || yy < 2 || yy >= h + 2) {
        if (dwords) { uint32_t* o4 = (uint32_t*)o; o4[0] = 0xffffffffu; o4[1] = 0xffffffffu; o4[2] = 0xffffffffu; }
        else for (int j = 0; j < 3 * cnt; j++) o[j] = 255;
        return;
    }
    const int b = a.strip ? r : r >> 1;
    const bool rec = a.strip || (r & 1);
    const ShSrc src = sh_src(a, b, t, rec);
    const bool mapped = a.strip ? a.map == 1 : (src.gt ? map_gt : map_rec);
    float x[3][4];
    uint32_t q[3][4];
    if (a.weighted) {
        float m[4] = {1.0f, 1.0f, 1.0f, 1.0f};
        if (t > 0) mask_group(a, b, t, y, xg, cnt, rec, m, x);
        else {
#pragma unroll
            for (int c = 0; c < 3; c++) sh_load(a, src, c, y, xg, cnt, x[c]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float s = (m[j] / mmax) * 256.0f;
            const int k = !(s >= 0.0f) ? 0 : s >= 255.0f ? 255 : (int)s;      // (a NaN or a negative weight was flagged by the reduction: any in-range entry will do)
#pragma unroll
            for (int c = 0; c < 3; c++) q[c][j] = j < cnt ? sh_blend_byte(sh_map(x[c][j], mapped), a.lut[3 * k + c], saturated, nans) : 0u;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            sh_load(a, src, c, y, xg, cnt, x[c]);
#pragma unroll
            for (int j = 0; j < 4; j++) q[c][j] = j < cnt ? sh_byte(sh_map(x[c][j], mapped), saturated, nans) : 0u;
        }
    }
    if (dwords) {
        uint32_t d[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) d[(3 * j + c) >> 2] |= q[c][j] << (8 * ((3 * j + c) & 3));      // byte 3 j + c of the group is channel c of its pixel j
        uint32_t* o4 = (uint32_t*)o;
        o4[0] = d[0]; o4[1] = d[1]; o4[2] = d[2];
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (j < cnt) { o[3 * j] = (uint8_t)q[0][j]; o[3 * j + 1] = (uint8_t)q[1][j]; o[3 * j + 2] = (uint8_t)q[2][j]; }
    }
}

// grid: x = blocks of SH_THREADS work items inside a cell, y = cells (a cell loop past 65535)
__global__ __launch_bounds__(SH_THREADS) void k_sheet_compose(ShArgs a) {
    __shared__ unsigned lds4[SH_WAVES];
    float mmax = 1.0f;
    if (a.weighted) {      // (uniform: every thread reaches the barrier inside)
        unsigned mx = SH_ONE_BITS;
        for (int k = threadIdx.x; k < a.nslab; k += SH_THREADS) mx = a.slab[k] > mx ? a.slab[k] : mx;
        mmax = __uint_as_float(block_fold<false>(mx, lds4));
    }
    const bool map_gt = !a.strip && a.words[SH_NEG_GT] != 0u && a.words[SH_NAN_GT] == 0u;
    const bool map_rec = !a.strip && a.words[SH_NEG_REC] != 0u && a.words[SH_NAN_REC] == 0u;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        a.words[SH_MAPPED_GT] = a.strip ? (a.map == 1 ? 1u : 0u) : (map_gt ? 1u : 0u);
        a.words[SH_MAPPED_REC] = a.strip ? (a.map == 1 ? 1u : 0u) : (map_rec ? 1u : 0u);
    }
    const int i = blockIdx.x * SH_THREADS + threadIdx.x;
    if (i >= a.dom) return;
    const int yy = i / a.dom_w, gg = i - yy * a.dom_w;
    unsigned saturated = 0, nans = 0;
    for (int cell = blockIdx.y; cell < a.rows * a.T; cell += gridDim.y) compose_item(a, cell, yy, gg, map_gt, map_rec, mmax, saturated, nans);
    if (saturated) atomicAdd(a.words + SH_SATURATED, saturated);
    if (nans) atomicAdd(a.words + SH_NANS, nans);
}

bool sheets_args_ok(int max_rows, int max_cols) {
    if (max_rows < 1 || max_cols < 1) { set_error("caddy_sheets: max_rows and max_cols must be positive"); return false; }
    if (max_rows > SH_MAX_SIDE || max_cols > SH_MAX_SIDE) { set_error("caddy_sheets: more than 32768 rows or columns of cells"); return false; }
    return true;
}
EvalKind sheets_kind(int max_rows, int max_cols) {
    return {CTX_SHEETS, max_rows, 0, 0,
            [=](caddy_ctx* c) {
                SheetsState* s = new SheetsState();
                c->sh = s;
                s->max_rows = max_rows; s->max_cols = max_cols;
                s->d_words = (unsigned*)c->persist.alloc(sizeof(unsigned) * SH_WORDS);
                s->d_slab = (unsigned*)c->persist.alloc(sizeof(unsigned) * SH_RED_BLOCKS);
            },
            [](caddy_ctx*) {},
            "caddy_sheets_workspace_bytes"};
}

// what both entry points check of their geometry; the image must stay below 2^31 bytes
bool sheet_fits(caddy_ctx* c, const char* who, long rows, int T, int h, int w) {
    const SheetsState* s = c->sh;
    if (h > SH_MAX_SIDE || w > SH_MAX_SIDE) { set_error(std::string(who) + ": cell sides above 32768"); return false; }
    if (rows > s->max_rows || T > s->max_cols) {
        set_error(std::string(who) + ": a sheet of " + std::to_string(rows) + " x " + std::to_string(T) + " cells, the context was created for " + std::to_string(s->max_rows) + " x " + std::to_string(s->max_cols));
        return false;
    }
    const long bytes = (rows * (h + 2) + 2) * ((long)T * (w + 2) + 2) * 3;
    if (bytes > 0x7fffffffL) { set_error(std::string(who) + ": the image would exceed 2^31 bytes"); return false; }
    return true;
}
void sheet_launch(caddy_ctx* c, ShArgs& a, bool reduce) {
    const SheetsState* s = c->sh;
    a.ngx = (a.w + 3) >> 2; a.dom_w = a.ngx + 2; a.dom = (a.h + 4) * a.dom_w;      // (sides <= 32768: below 2^31)
    a.pitch = 3L * ((long)a.T * (a.w + 2) + 2);
    a.words = s->d_words; a.slab = s->d_slab;
    hipMemsetAsync(s->d_words, 0, sizeof(unsigned) * SH_WORDS, c->stream);
    if (reduce) {
        const long items = std::max((long)a.B * a.T * 3 * a.h * a.ngx, ((long)a.B * a.Trec * 3 * a.h * a.w + 3) >> 2);
        a.nslab = (int)std::min<long>((items + SH_THREADS - 1) / SH_THREADS, SH_RED_BLOCKS);
        hipLaunchKernelGGL(k_sheet_reduce, dim3((unsigned)a.nslab), dim3(SH_THREADS), 0, c->stream, a);
    }
    const dim3 grid((unsigned)((a.dom + SH_THREADS - 1) / SH_THREADS), (unsigned)std::min<long>((long)a.rows * a.T, 65535));
    hipLaunchKernelGGL(k_sheet_compose, grid, dim3(SH_THREADS), 0, c->stream, a);
    c->ck(hipGetLastError() == hipSuccess ? 0 : -1, "example sheet");
}

}  // namespace

void sheets_free(caddy_ctx* c) {
    if (!c || !c->sh) return;
    delete c->sh;
    c->sh = nullptr;
}

extern "C" {
size_t caddy_sheets_workspace_bytes(int max_rows, int max_cols) {
    return sheets_args_ok(max_rows, max_cols) ? eval_workspace_bytes(sheets_kind(max_rows, max_cols)) : 0;
}
caddy_ctx* caddy_sheets_ctx_create(int max_rows, int max_cols, void* workspace, size_t bytes) {
    return sheets_args_ok(max_rows, max_cols) ? eval_ctx_create(sheets_kind(max_rows, max_cols), workspace, bytes) : nullptr;
}
int caddy_sheet_examples(caddy_ctx* c, const float* obs, int B, int T, int channels, int H, int W, const float* rec, int Trec, int h, int w, int weighted, float bias,
                         const double* lut768, unsigned char* out_u8) {
    if (!ctx_needs(c, CTX_SHEETS, "caddy_sheet_examples")) return -2;
    c->fail = false;
    if (!obs || !rec || !out_u8) { set_error("null input"); return -2; }
    if (((uintptr_t)obs & 3) || ((uintptr_t)rec & 3) || ((uintptr_t)out_u8 & 3) || ((uintptr_t)lut768 & 7)) { set_error("caddy_sheet_examples: obs, rec and out_u8 must be 4-byte aligned, lut768 8-byte aligned"); return -2; }
    if (B < 1 || T < 1 || H < 1 || W < 1 || h < 1 || w < 1) { set_error("caddy_sheet_examples: B, T and the frame sizes must be positive"); return -2; }
    if (channels < 3) { set_error("caddy_sheet_examples: the observations need at least 3 channels"); return -2; }
    if (Trec < 1 || (Trec != T && Trec != T - 1)) { set_error("caddy_sheet_examples: a sequence length of " + std::to_string(T) + " with a reconstructed one of " + std::to_string(Trec) + " (must be T or T - 1)"); return -2; }
    int f = 0;
    for (int k = 1; k <= 4; k *= 2) if ((long)h * k == H && (long)w * k == W) f = k;
    if (!f) {
        set_error("caddy_sheet_examples: " + std::to_string(H) + " x " + std::to_string(W) + " observations against " + std::to_string(h) + " x " + std::to_string(w) +
                  " frames: only the ratios 1, 2 and 4 are reproduced bit for bit");
        return -2;
    }
    if (weighted && f != 1) { set_error("caddy_sheet_examples: the motion-weighted sheet is drawn at full resolution only"); return -2; }
    if (weighted && !lut768) { set_error("caddy_sheet_examples: the motion-weighted sheet needs the colour table (null lut768)"); return -2; }
    const int drawn = std::min(B, SH_MAX_SEQUENCES);
    if (!sheet_fits(c, "caddy_sheet_examples", 2L * drawn, T, h, w)) return -2;
    if (H > SH_MAX_SIDE || W > SH_MAX_SIDE) { set_error("caddy_sheet_examples: frame sides above 32768"); return -2; }
    ShArgs a{};
    a.obs = obs; a.rec = rec; a.obs_frame = (long)channels * H * W;
    a.B = B; a.T = T; a.Trec = Trec; a.H = H; a.W = W; a.h = h; a.w = w; a.f = f; a.rows = 2 * drawn; a.weighted = weighted ? 1 : 0;
    a.bias = bias; a.lut = lut768; a.out = out_u8;
    sheet_launch(c, a, true);
    return finish(c, "caddy_sheets_workspace_bytes");
}
int caddy_sheet_strip(caddy_ctx* c, const float* frames, int n, int T, int h, int w, int map, unsigned char* out_u8) {
    if (!ctx_needs(c, CTX_SHEETS, "caddy_sheet_strip")) return -2;
    c->fail = false;
    if (!frames || !out_u8) { set_error("null input"); return -2; }
    if (((uintptr_t)frames & 3) || ((uintptr_t)out_u8 & 3)) { set_error("caddy_sheet_strip: frames and out_u8 must be 4-byte aligned"); return -2; }
    if (n < 1 || T < 1 || h < 1 || w < 1) { set_error("caddy_sheet_strip: n, T and the frame sizes must be positive"); return -2; }
    if (map != 0 && map != 1) { set_error("caddy_sheet_strip: map must be 0 (values in [0, 1]) or 1 ((x + 1) / 2)"); return -2; }
    if (!sheet_fits(c, "caddy_sheet_strip", n, T, h, w)) return -2;
    ShArgs a{};
    a.rec = frames; a.B = n; a.T = T; a.Trec = T; a.H = h; a.W = w; a.h = h; a.w = w; a.f = 1; a.rows = n; a.strip = 1; a.map = map; a.out = out_u8;
    sheet_launch(c, a, false);
    return finish(c, "caddy_sheets_workspace_bytes");
}
int caddy_sheet_stats_get(caddy_ctx* c, unsigned* stats5) {
    if (!ctx_needs(c, CTX_SHEETS, "caddy_sheet_stats_get")) return -2;
    if (!stats5) { set_error("null input"); return -2; }
    unsigned v[SH_WORDS];
    hipMemcpyAsync(v, c->sh->d_words, sizeof(v), hipMemcpyDeviceToHost, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess) { set_error("caddy_sheet_stats_get: reading the counts failed"); return -1; }
    stats5[0] = v[SH_MAPPED_GT]; stats5[1] = v[SH_MAPPED_REC]; stats5[2] = v[SH_SATURATED]; stats5[3] = v[SH_NANS]; stats5[4] = v[SH_MASK_BAD];
    return 0;
}
}
