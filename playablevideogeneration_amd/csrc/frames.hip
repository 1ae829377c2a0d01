// Device-side frame pipeline: the distinct uint8 RGB frames of one batch in, the model's observation tensor out.
//
// Reference: dataset/transforms.py:13-30,90-107 (per frame on the host: PIL Image.crop -> Image.resize(size, BILINEAR) -> ToTensor -> Normalize) and dataset/batching.py:97-112
// (the collate function concatenates each observation's stack along channels, stacks observations along time and elements along the batch).  Here the host ships every
// decoded frame once, as uint8, plus an int32 list that says which frame fills which (b, t, s) slot of the (bs, T, 3 S, H, W) tensor; one kernel does the rest.
//
// Arithmetic: PIL's 8-bit resize (Resample.c), bit for bit.  Per axis scale = in / out, support = max(scale, 1), ksize = 2 ceil(support) + 1; output xx has its centre at
// (xx + 0.5) scale, reads inputs [xmin, xmin + n) with the triangle weights max(0, 1 - |(x + xmin - centre + 0.5) / support|) normalised to sum 1 in double and quantised as
// (int)(0.5 + w 2^22); a pass is out = clip8((2^21 + sum pixel kk) >> 22).  Horizontal pass first, uint8 in between, a pass skipped when its axis keeps its size; the crop comes
// first, so no tap leaves the crop box.  The tables are built on the host at context creation (axis_table, contraction off: PIL's result is the specification).  The byte ->
// fp32 map is a 256-entry table the caller computed with the host's own expression, so the result equals the host path's whatever the device's division does.
//
// Kernel: one 256-thread workgroup per (slot, block of R output rows), slot-major.  A frame that feeds several slots is resized once per slot: its re-reads hit L2 and the
// kernel is bound by its fp32 writes (12 bytes out per 3 bytes in at equal size), so no frame -> slots list is built.
//   1. stage:  the source rows the block needs (block table, host-built) are read as aligned dwords -- rows of 3-byte pixels at arbitrary crop offsets start at any byte: two
//              neighbouring dwords are funnel-shifted into one aligned LDS dword; no byte at or beyond n_frames src_h src_w 3 is read (ld_guard) --, `ch` rows per round;
//   2. horizontal pass: (row, group of 4 outputs) per thread, 12 result bytes written to LDS as three dwords;  rounds 1-2 repeat until the block's rows are done
//              (with no horizontal pass the rows are staged straight into the second buffer);
//   3. vertical pass + table + store: (output row, group of 4 outputs) per thread reads three LDS dwords per tap (lane stride 12 bytes: conflict-free), looks the 12 bytes up
//              in the LDS copy of the table and stores one 16-byte vector per channel plane; the last group of a row with W % 4 != 0 stores scalars.
// R is the largest of 16, 8, 4, 2, 1 whose rows fit 64 KiB of LDS; a plan within 16 KiB runs the 16 KiB variant of the kernel (more workgroups per CU).
//
// The same context also runs the output side, the frame writer (caddy_frames_write, further down): fp32 planar frames -> the uint8 interleaved frames the host would write.
#include "eval_ctx.h"
#include "frames.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int FR_THREADS = 256, FR_PREC = 22, FR_MAX_R = 16;
constexpr int FR_LDS_SMALL = 16 * 1024, FR_LDS_LARGE = 64 * 1024, FR_LUT_BYTES = 256 * 4;
constexpr int FR_MAX_SIDE = 1 << 15;      // keeps every index below 2^31

struct FrArgs {
    const uint32_t* frames; long total_bytes, frame_bytes; int n_frames;
    const int* slot_src; const float* lut; float* out;
    const int *xb, *xk, *yb, *yk, *blk; int ksx, ksy;
    int src_w, l, u, row_bytes, W, H, R, nblk, pitchA, pitchB, b_bytes, ch, hpass, vpass;
};

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte store at a 4-byte aligned address (rows of W % 4 != 0 floats)

// dword i of the frame buffer; the bytes at or beyond `total` are not read (zero)
__device__ __forceinline__ uint32_t ld_guard(const uint32_t* p, long i, long total) {
    if ((i + 1) * 4 <= total) return p[i];
    const uint8_t* b = (const uint8_t*)p;
    uint32_t v = 0;
    for (int j = 0; j < 4; j++) if (i * 4 + j < total) v |= (uint32_t)b[i * 4 + j] << (8 * j);
    return v;
}
// clip8(acc >> 22).  Written on the unsigned value: from `clamp(acc >> 22, 0, 255)` of two neighbouring bytes hipcc forms gfx950's v_ashr_pk_u8_i32, which writes the low half of
// its destination only, and then ORs the register as if the high half were zero -- the horizontal pass packed stale accumulator bits into the next two bytes (seen on the MI355X)
__device__ __forceinline__ uint32_t clip8(int acc) {
    const uint32_t v = (uint32_t)(acc < 0 ? 0 : acc) >> FR_PREC;
    return v > 255u ? 255u : v;
}

template <int LDS_BYTES>
__global__ __launch_bounds__(FR_THREADS) void k_frames(FrArgs a) {
    __shared__ uint32_t lds[LDS_BYTES / 4];
    float* lut = (float*)lds;
    uint32_t* B = lds + FR_LUT_BYTES / 4;
    uint32_t* A = B + a.b_bytes / 4;
    const int tid = threadIdx.x;
    const int slot = blockIdx.x / a.nblk, blk = blockIdx.x - slot * a.nblk;
    const int y0 = blk * a.R, rows = a.H - y0 < a.R ? a.H - y0 : a.R;
    const int W = a.W, H = a.H, ngx = (W + 3) >> 2;
    const int f = a.slot_src[slot];
    if (f < 0 || f >= a.n_frames) {      // (the whole workgroup: no barrier is skipped by some threads only)
        const float nan = __int_as_float(0x7fc00000);
        for (int c = 0; c < 3; c++) {
            float* o = a.out + (((long)slot * 3 + c) * H + y0) * W;
            for (int i = tid; i < rows * W; i += FR_THREADS) o[i] = nan;
        }
        return;
    }
    lut[tid] = a.lut[tid];
    const int ys0 = a.blk[2 * blk], ns = a.blk[2 * blk + 1];
    const long fbase = (long)f * a.frame_bytes;
    const int nd = (a.row_bytes + 3) >> 2;
    const int ch = a.hpass ? a.ch : ns;
    for (int c0 = 0; c0 < ns; c0 += ch) {
        const int nr = ns - c0 < ch ? ns - c0 : ch;
        uint32_t* dst = a.hpass ? A : B;
        const int pitch4 = (a.hpass ? a.pitchA : a.pitchB) >> 2;
        for (int i = tid; i < nr * nd; i += FR_THREADS) {
            const int r = i / nd, k = i - r * nd;
            const long g = fbase + ((long)(a.u + ys0 + c0 + r) * a.src_w + a.l) * 3;      // first byte of the row inside the crop
            const int m = (int)(g & 3);
            const long i0 = (g >> 2) + k;
            const uint32_t lo = ld_guard(a.frames, i0, a.total_bytes);
            const uint32_t hi = (m != 0 && (i0 + 1) * 4 < g + a.row_bytes) ? ld_guard(a.frames, i0 + 1, a.total_bytes) : 0u;
            dst[r * pitch4 + k] = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * m));
        }
        __syncthreads();
        if (a.hpass) {
            for (int i = tid; i < nr * ngx; i += FR_THREADS) {
                const int r = i / ngx, xg = i - r * ngx;
                const uint8_t* src = (const uint8_t*)(A + r * (a.pitchA >> 2));
                uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int x = 4 * xg + j;
                    if (x < W) {
                        const int xmin = a.xb[2 * x], cnt = a.xb[2 * x + 1];
                        const int* kx = a.xk + x * a.ksx;
                        const uint8_t* p = src + xmin * 3;
                        int a0 = 1 << (FR_PREC - 1), a1 = a0, a2 = a0;
                        for (int k = 0; k < cnt; k++) {
                            const int w = kx[k];
                            a0 += w * p[3 * k]; a1 += w * p[3 * k + 1]; a2 += w * p[3 * k + 2];
                        }
                        o[(3 * j) >> 2] |= clip8(a0) << (8 * ((3 * j) & 3));
                        o[(3 * j + 1) >> 2] |= clip8(a1) << (8 * ((3 * j + 1) & 3));
                        o[(3 * j + 2) >> 2] |= clip8(a2) << (8 * ((3 * j + 2) & 3));
                    }
                }
                uint32_t* q = B + (c0 + r) * (a.pitchB >> 2) + 3 * xg;
                q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < rows * ngx; i += FR_THREADS) {
        const int yl = i / ngx, xg = i - yl * ngx, y = y0 + yl;
        uint32_t v[12];
        if (a.vpass) {
            const int ymin = a.yb[2 * y], cnt = a.yb[2 * y + 1];
            const int* ky = a.yk + y * a.ksy;
            const uint32_t* p = B + (ymin - ys0) * (a.pitchB >> 2) + 3 * xg;
            int acc[12];
#pragma unroll
            for (int j = 0; j < 12; j++) acc[j] = 1 << (FR_PREC - 1);
            for (int k = 0; k < cnt; k++) {
                const int w = ky[k];
                const uint32_t d[3] = {p[0], p[1], p[2]};
                p += a.pitchB >> 2;
#pragma unroll
                for (int j = 0; j < 12; j++) acc[j] += w * (int)((d[j >> 2] >> (8 * (j & 3))) & 255u);
            }
#pragma unroll
            for (int j = 0; j < 12; j++) v[j] = clip8(acc[j]);
        } else {
            const uint32_t* p = B + (y - y0) * (a.pitchB >> 2) + 3 * xg;      // (no vertical pass: the block's rows are its source rows)
            const uint32_t d[3] = {p[0], p[1], p[2]};
#pragma unroll
            for (int j = 0; j < 12; j++) v[j] = (d[j >> 2] >> (8 * (j & 3))) & 255u;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {      // byte 3 j + c of the group is channel c of its pixel j
            float* o = a.out + (((long)slot * 3 + c) * H + y) * W + 4 * xg;
            const float f0 = lut[v[c]], f1 = lut[v[3 + c]], f2 = lut[v[6 + c]], f3 = lut[v[9 + c]];
            if (4 * xg + 4 <= W) {
                f32x4u t = {f0, f1, f2, f3};
                *(f32x4u*)o = t;
            } else {
                const int n = W - 4 * xg;
                o[0] = f0;
                if (n > 1) o[1] = f1;
                if (n > 2) o[2] = f2;
            }
        }
    }
}

// ---- Frame writer: fp32 planar frames -> uint8 interleaved frames (caddy_frames_write) ----
// Reference: evaluation/evaluation_dataset_builder.py:60-81,140-153 (torch.cat([first, rec]) -> (x + 1) / 2 when torch.min is negative -> numpy * 255 -> astype(uint8)) and
// play.py:140.  One lane takes 4 consecutive pixels of a row: three 16-byte loads (one per plane), 12 bytes packed into three dwords and stored contiguously (a wave writes 768
// contiguous bytes), or, for the fp32 output, the mode-1 table value of every byte as one 16-byte store per plane.  The last group of a row with W % 4 != 0 loads and stores
// scalars; a group whose 12 bytes do not start at a 4-byte boundary (odd W: row and frame bases at any byte) stores bytes.  Memory-bound, no LDS.
enum { FW_NEG = 0, FW_NAN = 1, FW_SATURATED = 2, FW_NANS = 3, FW_MAPPED = 4, FW_WORDS = 8 };
constexpr int FW_THREADS = 256, FW_SCAN_BLOCKS = 2048;

struct FwArgs {
    const float *rec, *first; long first_stride, rec_floats, first_floats, frame_floats;
    int N, Trec, T, H, W, ngx, groups_per_frame, map;
    const float* lut; unsigned* stats; uint8_t* out_u8; float* out_f32;
};

// map 2, first launch: is any value negative, is any a NaN?  (-0.0 < 0 and NaN < 0 are false, as on the host.)  The virtual array is rec followed by the B frames of `first`.
__global__ __launch_bounds__(FW_THREADS) void k_frame_writer_scan(FwArgs a) {
    const long n = a.rec_floats + a.first_floats, n4 = (n + 3) >> 2;
    bool neg = false, nan = false;
    for (long i = (long)blockIdx.x * FW_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * FW_THREADS) {
        const long e = i * 4;
        if (e + 4 <= a.rec_floats) {
            const f32x4u v = *(const f32x4u*)(a.rec + e);
            neg |= v.x < 0.f || v.y < 0.f || v.z < 0.f || v.w < 0.f;
            nan |= v.x != v.x || v.y != v.y || v.z != v.z || v.w != v.w;
        } else {
            for (long j = e; j < e + 4 && j < n; j++) {
                float x;
                if (j < a.rec_floats) x = a.rec[j];
                else { const long k = j - a.rec_floats, b = k / a.frame_floats; x = a.first[b * a.first_stride + (k - b * a.frame_floats)]; }
                neg |= x < 0.f;
                nan |= x != x;
            }
        }
    }
    if (neg) atomicOr(a.stats + FW_NEG, 1u);
    if (nan) atomicOr(a.stats + FW_NAN, 1u);
}

// the host's expression, operation by operation: nothing here may be contracted or reassociated (x * 127.5f + 127.5f differs at level boundaries)
__device__ __forceinline__ uint32_t fw_byte(float x, bool mapped, unsigned& saturated, unsigned& nans) {
#pragma clang fp contract(off)
    float v = x;
    if (mapped) { v = x + 1.0f; v = v * 0.5f; }
    const float s = v * 255.0f;
    if (s != s) { nans++; return 0u; }
    if (s < 0.0f) { saturated++; return 0u; }
    if (s >= 256.0f) { saturated++; return 255u; }
    return (uint32_t)(int)s;
}

// one group of frame n: row y, pixels [4 xg, 4 xg + cnt)
__device__ __forceinline__ void writer_group(const FwArgs& a, bool mapped, int n, int y, int xg, int cnt, int lead, long plane, unsigned& saturated, unsigned& nans) {
    const int H = a.H, W = a.W;
    const int b = n / a.T, t = n - b * a.T;
    const float* src = (lead && t == 0) ? a.first + (long)b * a.first_stride : a.rec + ((long)b * a.Trec + (t - lead)) * a.frame_floats;
    src += (long)y * W + 4 * xg;
    float x[3][4];
    if (cnt == 4) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const f32x4u v = *(const f32x4u*)(src + c * plane);
            x[c][0] = v.x; x[c][1] = v.y; x[c][2] = v.z; x[c][3] = v.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int j = 0; j < 4; j++) x[c][j] = j < cnt ? src[c * plane + j] : 0.f;
    }
    uint32_t q[3][4];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) q[c][j] = j < cnt ? fw_byte(x[c][j], mapped, saturated, nans) : 0u;
    if (a.out_u8) {
        uint8_t* o = a.out_u8 + (((long)n * H + y) * W + 4 * xg) * 3;
        if (cnt == 4 && ((uintptr_t)o & 3) == 0) {
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
    if (a.out_f32) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float* o = a.out_f32 + (((long)n * 3 + c) * H + y) * W + 4 * xg;
            if (cnt == 4) {
                f32x4u v = {a.lut[q[c][0]], a.lut[q[c][1]], a.lut[q[c][2]], a.lut[q[c][3]]};
                *(f32x4u*)o = v;
            } else {
                o[0] = a.lut[q[c][0]];
                if (cnt > 1) o[1] = a.lut[q[c][1]];
                if (cnt > 2) o[2] = a.lut[q[c][2]];
            }
        }
    }
}

// grid: x = blocks of FW_THREADS groups inside a frame, y = frames (a frame loop past 65535)
__global__ __launch_bounds__(FW_THREADS) void k_frame_writer(FwArgs a) {
    const bool mapped = a.map == 1 || (a.map == 2 && a.stats[FW_NEG] != 0u && a.stats[FW_NAN] == 0u);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.stats[FW_MAPPED] = mapped ? 1u : 0u;
    const int r = blockIdx.x * FW_THREADS + threadIdx.x;
    if (r >= a.groups_per_frame) return;
    const int H = a.H, W = a.W, y = r / a.ngx, xg = r - y * a.ngx, lead = a.first ? 1 : 0;
    const long plane = (long)H * W;
    const int cnt = W - 4 * xg < 4 ? W - 4 * xg : 4;
    unsigned saturated = 0, nans = 0;
    for (int n = blockIdx.y; n < a.N; n += gridDim.y) writer_group(a, mapped, n, y, xg, cnt, lead, plane, saturated, nans);
    if (saturated) atomicAdd(a.stats + FW_SATURATED, saturated);
    if (nans) atomicAdd(a.stats + FW_NANS, nans);
}

// PIL's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter, in double and without contraction: (int)(0.5 + w 2^22) must not become one fused operation
void axis_table(int in, int out, FrAxis* t) {
#pragma clang fp contract(off)
    t->in = in; t->out = out;
    const double scale = (double)in / out, filterscale = scale < 1.0 ? 1.0 : scale, support = 1.0 * filterscale, ss = 1.0 / filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    t->ksize = ksize;
    t->bounds.assign((size_t)out * 2, 0);
    t->kk.assign((size_t)out * ksize, 0);
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out; xx++) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        for (int x = 0; x < xmax; x++) {
            double v = (x + xmin - center + 0.5) * ss;
            if (v < 0.0) v = -v;
            w[x] = v < 1.0 ? 1.0 - v : 0.0;
            ww += w[x];
        }
        for (int x = 0; x < xmax; x++) if (ww != 0.0) w[x] /= ww;
        for (int x = 0; x < ksize; x++) {
            const double v = x < xmax ? w[x] : 0.0;
            t->kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << FR_PREC)) : (int)(0.5 + v * (1 << FR_PREC));
        }
        t->bounds[2 * xx] = xmin; t->bounds[2 * xx + 1] = xmax;
    }
}

// block table and LDS footprint for R output rows per workgroup; false when it does not fit `budget`
bool plan_rows(FramesState* s, int R, int budget) {
    const int nblk = (s->H + R - 1) / R;
    std::vector<int> blk((size_t)nblk * 2);
    int ns_max = 0;
    for (int b = 0; b < nblk; b++) {
        const int y0 = b * R, y1 = std::min(s->H, y0 + R);
        int lo = y0, hi = y1;
        if (s->vpass) {
            lo = s->in_h; hi = 0;
            for (int y = y0; y < y1; y++) { lo = std::min(lo, s->ax[1].bounds[2 * y]); hi = std::max(hi, s->ax[1].bounds[2 * y] + s->ax[1].bounds[2 * y + 1]); }
        }
        blk[2 * b] = lo; blk[2 * b + 1] = hi - lo;
        ns_max = std::max(ns_max, hi - lo);
    }
    const long b_bytes = (long)ns_max * s->pitchB;
    const long left = (long)budget - FR_LUT_BYTES - b_bytes - (s->hpass ? s->pitchA : 0);
    if (left < 0) return false;
    s->R = R; s->nblk = nblk; s->ns_max = ns_max; s->blk = blk;
    s->ch = s->hpass ? (int)std::min<long>(ns_max, 1 + left / s->pitchA) : ns_max;
    s->lds_used = (int)(FR_LUT_BYTES + b_bytes + (s->hpass ? (long)s->ch * s->pitchA : 0));
    s->lds_variant = s->lds_used <= FR_LDS_SMALL ? FR_LDS_SMALL : FR_LDS_LARGE;
    return true;
}

// geometry, tables and plan; null + caddy_last_error for a geometry the pipeline refuses
FramesState* frames_plan(int max_frames, int src_h, int src_w, const int* crop4, int out_h, int out_w) {
    if (max_frames < 1 || src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1) { set_error("caddy_frames: max_frames and the frame sizes must be positive"); return nullptr; }
    if (src_h > FR_MAX_SIDE || src_w > FR_MAX_SIDE || out_h > FR_MAX_SIDE || out_w > FR_MAX_SIDE) { set_error("caddy_frames: frame sides above 32768"); return nullptr; }
    const int l = crop4 ? crop4[0] : 0, u = crop4 ? crop4[1] : 0, r = crop4 ? crop4[2] : src_w, d = crop4 ? crop4[3] : src_h;
    if (l < 0 || u < 0 || r > src_w || d > src_h || l >= r || u >= d) {
        set_error("caddy_frames: crop box [" + std::to_string(l) + ", " + std::to_string(u) + ", " + std::to_string(r) + ", " + std::to_string(d) + "] is not inside the " +
                  std::to_string(src_w) + " x " + std::to_string(src_h) + " frame (PIL would pad with black; such datasets keep the host transform)");
        return nullptr;
    }
    FramesState* s = new FramesState();
    s->src_h = src_h; s->src_w = src_w; s->l = l; s->u = u; s->in_w = r - l; s->in_h = d - u; s->W = out_w; s->H = out_h;
    s->hpass = s->in_w != out_w; s->vpass = s->in_h != out_h;
    axis_table(s->in_w, out_w, &s->ax[0]);
    axis_table(s->in_h, out_h, &s->ax[1]);
    s->pitchA = (s->in_w * 3 + 3) / 4 * 4;
    s->pitchB = (out_w + 3) / 4 * 12;
    for (int R = FR_MAX_R; R >= 1; R >>= 1)
        if (plan_rows(s, R, FR_LDS_LARGE)) return s;
    set_error("caddy_frames: a " + std::to_string(out_w) + " x " + std::to_string(out_h) + " output from a " + std::to_string(s->in_w) + " x " + std::to_string(s->in_h) +
              " crop does not fit the kernel's " + std::to_string(FR_LDS_LARGE) + " bytes of LDS even with one output row per workgroup");
    delete s;
    return nullptr;
}

// the kind: fill builds the plan of its context (the dry context of the sizing walk builds and releases one of its own)
struct FrGeomArgs { int max_frames, src_h, src_w, out_h, out_w; bool has_crop; int crop[4]; };
FrGeomArgs geom_args(int max_frames, int src_h, int src_w, const int* crop4, int out_h, int out_w) {
    FrGeomArgs g{max_frames, src_h, src_w, out_h, out_w, crop4 != nullptr, {0, 0, 0, 0}};
    if (crop4) memcpy(g.crop, crop4, sizeof(g.crop));
    return g;
}
bool frames_args_ok(const FrGeomArgs& g) {
    FramesState* s = frames_plan(g.max_frames, g.src_h, g.src_w, g.has_crop ? g.crop : nullptr, g.out_h, g.out_w);
    delete s;
    return s != nullptr;
}
EvalKind frames_kind(const FrGeomArgs& g) {
    return {CTX_FRAMES, g.max_frames, g.out_h, g.out_w,
            [=](caddy_ctx* c) {
                FramesState* s = frames_plan(g.max_frames, g.src_h, g.src_w, g.has_crop ? g.crop : nullptr, g.out_h, g.out_w);
                c->frs = s;
                s->d_xb = (int*)c->persist.alloc(sizeof(int) * s->ax[0].bounds.size());
                s->d_xk = (int*)c->persist.alloc(sizeof(int) * s->ax[0].kk.size());
                s->d_yb = (int*)c->persist.alloc(sizeof(int) * s->ax[1].bounds.size());
                s->d_yk = (int*)c->persist.alloc(sizeof(int) * s->ax[1].kk.size());
                s->d_blk = (int*)c->persist.alloc(sizeof(int) * s->blk.size());
                s->d_lut = (float*)c->persist.alloc(sizeof(float) * 512);
                s->d_wstats = (unsigned*)c->persist.alloc(sizeof(unsigned) * FW_WORDS);
            },
            [](caddy_ctx*) {},
            "caddy_frames_workspace_bytes"};
}

}  // namespace

void frames_free(caddy_ctx* c) {
    if (!c || !c->frs) return;
    delete c->frs;
    c->frs = nullptr;
}

extern "C" {
size_t caddy_frames_workspace_bytes(int max_frames, int src_h, int src_w, const int* crop4, int out_h, int out_w) {
    const FrGeomArgs g = geom_args(max_frames, src_h, src_w, crop4, out_h, out_w);
    return frames_args_ok(g) ? eval_workspace_bytes(frames_kind(g)) : 0;
}
caddy_ctx* caddy_frames_ctx_create(int max_frames, int src_h, int src_w, const int* crop4, int out_h, int out_w, const float* lut512, void* workspace, size_t bytes) {
    if (!lut512) { set_error("null input"); return nullptr; }
    const FrGeomArgs g = geom_args(max_frames, src_h, src_w, crop4, out_h, out_w);
    caddy_ctx* c = frames_args_ok(g) ? eval_ctx_create(frames_kind(g), workspace, bytes) : nullptr;
    if (!c) return nullptr;
    FramesState* s = c->frs;
    memcpy(s->lut, lut512, sizeof(s->lut));
    hipMemcpy(s->d_xb, s->ax[0].bounds.data(), sizeof(int) * s->ax[0].bounds.size(), hipMemcpyHostToDevice);
    hipMemcpy(s->d_xk, s->ax[0].kk.data(), sizeof(int) * s->ax[0].kk.size(), hipMemcpyHostToDevice);
    hipMemcpy(s->d_yb, s->ax[1].bounds.data(), sizeof(int) * s->ax[1].bounds.size(), hipMemcpyHostToDevice);
    hipMemcpy(s->d_yk, s->ax[1].kk.data(), sizeof(int) * s->ax[1].kk.size(), hipMemcpyHostToDevice);
    hipMemcpy(s->d_blk, s->blk.data(), sizeof(int) * s->blk.size(), hipMemcpyHostToDevice);
    hipMemcpy(s->d_lut, s->lut, sizeof(s->lut), hipMemcpyHostToDevice);
    if (hipGetLastError() != hipSuccess) { set_error("caddy_frames_ctx_create: uploading the filter tables failed"); caddy_ctx_destroy(c); return nullptr; }
    return c;
}
int caddy_frames_tables_get(caddy_ctx* c, int axis, int* ksize, int* bounds, int* kk) {
    if (!ctx_needs(c, CTX_FRAMES, "caddy_frames_tables_get")) return -2;
    if (axis != 0 && axis != 1) { set_error("caddy_frames_tables_get: axis must be 0 (horizontal) or 1 (vertical)"); return -2; }
    const FrAxis& t = c->frs->ax[axis];
    if (ksize) *ksize = t.ksize;
    if (bounds) memcpy(bounds, t.bounds.data(), sizeof(int) * t.bounds.size());
    if (kk) memcpy(kk, t.kk.data(), sizeof(int) * t.kk.size());
    return (axis == 0 ? c->frs->hpass : c->frs->vpass) ? 1 : 0;
}
int caddy_debug_frames_plan(caddy_ctx* c, int* plan5) {
    if (!ctx_needs(c, CTX_FRAMES, "caddy_debug_frames_plan")) return -2;
    if (!plan5) { set_error("null input"); return -2; }
    const FramesState* s = c->frs;
    plan5[0] = s->R; plan5[1] = s->ns_max; plan5[2] = s->ch; plan5[3] = s->lds_used; plan5[4] = s->lds_variant;
    return 0;
}
int caddy_frames_to_observations(caddy_ctx* c, const unsigned char* frames, int n_frames, const int* slot_src, int n_slots, int mode, float* out) {
    if (!ctx_needs(c, CTX_FRAMES, "caddy_frames_to_observations")) return -2;
    c->fail = false;
    if (!frames || !slot_src || !out) { set_error("null input"); return -2; }
    if (((uintptr_t)frames & 3) || ((uintptr_t)slot_src & 3) || ((uintptr_t)out & 3)) { set_error("caddy_frames_to_observations: frames, slot_src and out must be 4-byte aligned"); return -2; }
    if (mode != 0 && mode != 1) { set_error("caddy_frames_to_observations: mode must be 0 ([-1, 1]) or 1 ([0, 1])"); return -2; }
    if (n_frames < 1 || n_slots < 1) { set_error("caddy_frames_to_observations: n_frames and n_slots must be positive"); return -2; }
    if (n_frames > c->cfg.batch) { set_error("caddy_frames_to_observations: " + std::to_string(n_frames) + " frames, the context was created for " + std::to_string(c->cfg.batch)); return -2; }
    const FramesState* s = c->frs;
    if ((long)n_slots * s->nblk > 0x7fffffffL) { set_error("caddy_frames_to_observations: too many slots for one launch"); return -2; }
    FrArgs a{};
    a.frames = (const uint32_t*)frames; a.frame_bytes = (long)s->src_h * s->src_w * 3; a.total_bytes = a.frame_bytes * n_frames; a.n_frames = n_frames;
    a.slot_src = slot_src; a.lut = s->d_lut + 256 * mode; a.out = out;
    a.xb = s->d_xb; a.xk = s->d_xk; a.yb = s->d_yb; a.yk = s->d_yk; a.blk = s->d_blk; a.ksx = s->ax[0].ksize; a.ksy = s->ax[1].ksize;
    a.src_w = s->src_w; a.l = s->l; a.u = s->u; a.row_bytes = s->in_w * 3; a.W = s->W; a.H = s->H; a.R = s->R; a.nblk = s->nblk;
    a.pitchA = s->pitchA; a.pitchB = s->pitchB; a.b_bytes = s->ns_max * s->pitchB; a.ch = s->ch; a.hpass = s->hpass; a.vpass = s->vpass;
    const dim3 grid((unsigned)(n_slots * s->nblk)), block(FR_THREADS);
    if (s->lds_variant == FR_LDS_SMALL) hipLaunchKernelGGL(k_frames<FR_LDS_SMALL>, grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL(k_frames<FR_LDS_LARGE>, grid, block, 0, c->stream, a);
    c->ck(hipGetLastError() == hipSuccess ? 0 : -1, "frame pipeline");
    return finish(c, "caddy_frames_workspace_bytes");
}
int caddy_frames_write(caddy_ctx* c, const float* rec, int B, int Trec, const float* first, long first_stride, int map, unsigned char* out_u8, float* out_f32) {
    if (!ctx_needs(c, CTX_FRAMES, "caddy_frames_write")) return -2;
    c->fail = false;
    if (!rec) { set_error("null input"); return -2; }
    if (!out_u8 && !out_f32) { set_error("caddy_frames_write: out_u8 and out_f32 are both null"); return -2; }
    if (((uintptr_t)rec & 3) || ((uintptr_t)first & 3) || ((uintptr_t)out_u8 & 3) || ((uintptr_t)out_f32 & 3)) { set_error("caddy_frames_write: rec, first, out_u8 and out_f32 must be 4-byte aligned"); return -2; }
    if (map < 0 || map > 2) { set_error("caddy_frames_write: map must be 0 (values in [0, 1]), 1 ((x + 1) / 2) or 2 ((x + 1) / 2 when the minimum is negative)"); return -2; }
    if (B < 1 || Trec < 1) { set_error("caddy_frames_write: B and Trec must be positive"); return -2; }
    const FramesState* s = c->frs;
    const long T = (long)Trec + (first ? 1 : 0), N = (long)B * T, frame_floats = 3L * s->H * s->W;
    if (N > c->cfg.batch) { set_error("caddy_frames_write: " + std::to_string(N) + " frames, the context was created for " + std::to_string(c->cfg.batch)); return -2; }
    if (first && B > 1 && first_stride < frame_floats) { set_error("caddy_frames_write: first_stride below one frame (3 height width floats)"); return -2; }
    FwArgs a{};
    a.rec = rec; a.first = first; a.first_stride = first ? first_stride : 0; a.frame_floats = frame_floats;
    a.rec_floats = (long)B * Trec * frame_floats; a.first_floats = first ? (long)B * frame_floats : 0;
    a.Trec = Trec; a.T = (int)T; a.H = s->H; a.W = s->W; a.ngx = (s->W + 3) >> 2; a.map = map;
    a.N = (int)N; a.groups_per_frame = s->H * a.ngx;      // (sides <= 32768: below 2^31)
    a.lut = s->d_lut + 256; a.stats = s->d_wstats; a.out_u8 = out_u8; a.out_f32 = out_f32;
    const dim3 grid((unsigned)((a.groups_per_frame + FW_THREADS - 1) / FW_THREADS), (unsigned)std::min<long>(N, 65535));
    hipMemsetAsync(s->d_wstats, 0, sizeof(unsigned) * FW_WORDS, c->stream);
    if (map == 2) {
        const long n4 = (a.rec_floats + a.first_floats + 3) >> 2, want = (n4 + FW_THREADS - 1) / FW_THREADS;
        hipLaunchKernelGGL(k_frame_writer_scan, dim3((unsigned)std::min<long>(want, FW_SCAN_BLOCKS)), dim3(FW_THREADS), 0, c->stream, a);
    }
    hipLaunchKernelGGL(k_frame_writer, grid, dim3(FW_THREADS), 0, c->stream, a);
    c->ck(hipGetLastError() == hipSuccess ? 0 : -1, "frame writer");
    return finish(c, "caddy_frames_workspace_bytes");
}
int caddy_frames_write_stats_get(caddy_ctx* c, unsigned* stats3) {
    if (!ctx_needs(c, CTX_FRAMES, "caddy_frames_write_stats_get")) return -2;
    if (!stats3) { set_error("null input"); return -2; }
    unsigned v[FW_WORDS];
    hipMemcpyAsync(v, c->frs->d_wstats, sizeof(v), hipMemcpyDeviceToHost, c->stream);
    if (hipStreamSynchronize(c->stream) != hipSuccess) { set_error("caddy_frames_write_stats_get: reading the counts failed"); return -1; }
    stats3[0] = v[FW_MAPPED]; stats3[1] = v[FW_SATURATED]; stats3[2] = v[FW_NANS];
    return 0;
}
}
