// FVD feature network (fvd.h).  Reference: evaluation/metrics/fvd.py:67-126 feeds 16 videos at a time through TensorFlow-Hub's Kinetics-400 I3D (Inception-v1 inflated to 3-D:
// every unit conv3d(no bias) -> batch norm(eval, eps 1e-3) -> ReLU, everything SAME-padded) and keeps the 400 values of RGB/inception_i3d/Mean:0 per video; fvd.py:49-56 resizes
// the frames to 224 x 224 with TF1's resize_bilinear and maps them to [-1, 1].  This file holds what no other part of the library has -- a 3-D implicit-GEMM convolution, 3-D max
// pools with SAME padding, the legacy bilinear input stage, the averaging head --, the walk over the 57 convolutions + logits, and the C ABI of the FVD context.
//
// k_conv3d_igemm is the tile of conv_igemm.h with K running over (kt, kh, kw, 32-channel chunk); the tap counters advance incrementally (no division in the K loop).  The Cin = 3
// first layer gathers one (kt, kh) ROW of the window per K chunk from the pitch-4 image: KW taps x 4 channels = 28 contiguous floats (two 16-byte loads per thread), 49 chunks
// instead of 343.
//
// Determinism: no atomics except the integer OR of the range flag; every output element has one writer and a fixed summation order (the head sums in fp64 in index order), so two
// runs -- and two chunkings of the same videos -- give identical bits.
#include "conv_igemm.h"
#include "eval_ctx.h"
#include "fvd.h"
#include <cstdio>
#include <cstring>

namespace {

template <bool F16>
__global__ __launch_bounds__(256) void k_conv3d_igemm(Conv3dArgs a) {
    const int hw = a.Ho * a.Wo;
    const long thw = (long)a.To * hw;
    const long M = (long)a.N * thw;
    // ---- loader role: tile position lrow, channels 8 lq .. 8 lq + 7 of the chunk (gather: taps 2 lq, 2 lq + 1 of the row) ----
    const int lrow = threadIdx.x >> 2, lq = threadIdx.x & 3;
    const long lm = (long)blockIdx.x * CG_BM + lrow;
    const bool lvalid = lm < M;
    int ln = 0, lot = 0, loy = 0, lox = 0;
    if (lvalid) {
        ln = (int)(lm / thw); const long r1 = lm - (long)ln * thw;
        lot = (int)(r1 / hw); const int r2 = (int)(r1 - (long)lot * hw);
        loy = r2 / a.Wo; lox = r2 - loy * a.Wo;
    }
    const float* lbase = a.in + (long)ln * a.in_sn;
    const int it0 = lot * a.st - a.pt, iy0 = loy * a.sh - a.ph, ix0 = lox * a.sw - a.pw;
    int kt = 0, ky = 0, kx = 0, ch = 0;      // tap and chunk of the NEXT load
    auto load = [&](int, float4& r0, float4& r1) {
        r0 = make_float4(0.f, 0.f, 0.f, 0.f); r1 = r0;
        const int it = it0 + kt, iy = iy0 + ky;
        const bool row_ok = lvalid && it >= 0 && it < a.Ti && iy >= 0 && iy < a.Hi;
        if (a.gather) {
            if (row_ok) {
                const float* row = lbase + ((long)it * a.Hi + iy) * a.Wi * 4;
                const int kx0 = 2 * lq, xa = ix0 + kx0, xb = xa + 1;
                if (kx0 < a.KW && xa >= 0 && xa < a.Wi) r0 = *reinterpret_cast<const float4*>(row + (long)xa * 4);
                if (kx0 + 1 < a.KW && xb >= 0 && xb < a.Wi) r1 = *reinterpret_cast<const float4*>(row + (long)xb * 4);
            }
            if (++ky == a.KH) { ky = 0; kt++; }
        } else {
            const int ix = ix0 + kx, c = ch * CG_KC + lq * 8;
            if (row_ok && ix >= 0 && ix < a.Wi && c < a.Cin) {
                const float4* p = reinterpret_cast<const float4*>(lbase + (((long)it * a.Hi + iy) * a.Wi + ix) * a.in_ld + c);
                r0 = p[0]; r1 = p[1];
            }
            if (++ch == a.nchunk) { ch = 0; if (++kx == a.KW) { kx = 0; if (++ky == a.KH) { ky = 0; kt++; } } }
        }
    };
    const ConvTile t{a.w, a.Cout, a.bias, a.relu, a.out, a.out_sn, a.out_ld, a.sat_flag, M, thw, a.gather ? a.KT * a.KH : a.KT * a.KH * a.KW * a.nchunk};
    conv_igemm_tile<F16>(t, load);
}

// one thread per padded (K chunk, channel block, element of the chunk, output channel of the block) element: both packed forms + the folded bias
__global__ __launch_bounds__(256) void k_conv3d_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, const float* bias_in,
                                                     int Cin, int Cout, int taps, int KW, int gather, int nchunk, int ncb, long total, float* w32, _Float16* w16, float* bias_out) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ol = (int)(i & 31), cl = (int)((i >> 5) & 31);
        const long tile = i >> 10;                       // K chunk * ncb + cb
        const int cb = (int)(tile % ncb); const long kc = tile / ncb;
        const int o = cb * 32 + ol;
        const double s = o < Cout ? conv_fold_scale(gamma, mean, var, eps, o) : 1.0;
        long tap = -1; int c = 0;
        if (gather) { const int kx = cl >> 2; c = cl & 3; if (kx < KW && c < Cin) tap = kc * KW + kx; }      // chunk = (kt, kh) row; element = 4 kx + channel, the pad lane is zero
        else { c = (int)(kc % nchunk) * 32 + cl; if (c < Cin) tap = kc / nchunk; }
        float v = 0.f;
        if (o < Cout && tap >= 0 && tap < taps) v = (float)((double)w[(tap * Cin + c) * Cout + o] * s);
        conv_pack_store(w32, w16, tile, cl, ol, v);
        if (bias_out && kc == 0 && cl == 0 && o < Cout) bias_out[o] = conv_fold_bias(beta, mean, bias_in, s, o);
    }
}

// ---- 3-D max pooling, one thread per (output position, 4 channels); lt / lh / lw: leading SAME padding ----
__global__ __launch_bounds__(256) void k_fvd_pool(V5 in, V5 out, int kt, int kh, int kw, int st, int sh, int sw, int lt, int lh, int lw, long total) {
    const int C4 = out.C >> 2;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4); long q = i / C4;
        const int x = (int)(q % out.W); q /= out.W; const int y = (int)(q % out.H); q /= out.H; const int t = (int)(q % out.T); const long n = q / out.T;
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int dt = 0; dt < kt; dt++) {
            const int it = t * st - lt + dt;
            if (it < 0 || it >= in.T) continue;
            for (int dy = 0; dy < kh; dy++) {
                const int iy = y * sh - lh + dy;
                if (iy < 0 || iy >= in.H) continue;
                for (int dx = 0; dx < kw; dx++) {
                    const int ix = x * sw - lw + dx;
                    if (ix < 0 || ix >= in.W) continue;
                    const float4 v = *reinterpret_cast<const float4*>(in.p + n * in.sn + (((long)it * in.H + iy) * in.W + ix) * in.ld + 4 * c);
                    m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
                }
            }
        }
        *reinterpret_cast<float4*>(out.p + n * out.sn + (((long)t * out.H + y) * out.W + x) * out.ld + 4 * c) = m;
    }
}

// head, first half: VALID stride-1 average over a (wt, wh, ww) window, fp32 values summed in fp64 in (t, y, x) order
__global__ __launch_bounds__(256) void k_fvd_avg(V5 in, V5 out, int wt, int wh, int ww, long total) {
    const int C4 = out.C >> 2;
    const double inv = 1.0 / ((double)wt * wh * ww);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4); long q = i / C4;
        const int x = (int)(q % out.W); q /= out.W; const int y = (int)(q % out.H); q /= out.H; const int t = (int)(q % out.T); const long n = q / out.T;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int dt = 0; dt < wt; dt++)
            for (int dy = 0; dy < wh; dy++)
                for (int dx = 0; dx < ww; dx++) {
                    const float4 v = *reinterpret_cast<const float4*>(in.p + n * in.sn + (((long)(t + dt) * in.H + y + dy) * in.W + x + dx) * in.ld + 4 * c);
                    s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
                }
        *reinterpret_cast<float4*>(out.p + n * out.sn + (((long)t * out.H + y) * out.W + x) * out.ld + 4 * c) =
            make_float4((float)(s0 * inv), (float)(s1 * inv), (float)(s2 * inv), (float)(s3 * inv));
    }
}
// head, last step: the mean of the logits over the remaining positions, fp64 in position order: out[n * C + c]
__global__ __launch_bounds__(256) void k_fvd_mean(V5 in, double* out, long total) {
    const long P = (long)in.T * in.H * in.W;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % in.C); const long n = i / in.C;
        double s = 0.0;
        const float* p = in.p + n * in.sn + c;
        for (long q = 0; q < P; q++) s += p[q * in.ld];
        out[i] = s / (double)P;
    }
}

// TF1 resize_bilinear, align_corners=False, no half-pixel centres: src = dst * (in / out) in fp32, i1 = min(i0 + 1, in - 1); v = top + (bottom - top) * ly with
// top = tl + (tr - tl) * lx, as the TensorFlow kernel evaluates it
__global__ __launch_bounds__(256) void k_fvd_stage(const float* src, float* out, long npix, int Hs, int Ws, int Ho, int Wo, float sy, float sx) {
    const long hws = (long)Hs * Ws;
    const bool same = Hs == Ho && Ws == Wo;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < npix; q += (long)gridDim.x * 256) {
        const long n = q / ((long)Ho * Wo); const int rem = (int)(q - n * Ho * Wo); const int y = rem / Wo, x = rem - y * Wo;
        const float* s = src + n * 3 * hws;
        float v[3];
        if (same) { for (int c = 0; c < 3; c++) v[c] = s[c * hws + (long)y * Ws + x]; }
        else {
            const float fy = (float)y * sy, fx = (float)x * sx;
            int y0 = (int)fy, x0 = (int)fx;
            if (y0 > Hs - 1) y0 = Hs - 1;
            if (x0 > Ws - 1) x0 = Ws - 1;
            const int y1 = y0 + 1 < Hs ? y0 + 1 : Hs - 1, x1 = x0 + 1 < Ws ? x0 + 1 : Ws - 1;
            const float ly = fy - (float)y0, lx = fx - (float)x0;
            for (int c = 0; c < 3; c++) {
                const float* p = s + c * hws;
                const float tl = p[(long)y0 * Ws + x0], tr = p[(long)y0 * Ws + x1], bl = p[(long)y1 * Ws + x0], br = p[(long)y1 * Ws + x1];
                const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
                v[c] = top + (bot - top) * ly;
            }
        }
        reinterpret_cast<float4*>(out)[q] = make_float4(2.f * v[0] - 1.f, 2.f * v[1] - 1.f, 2.f * v[2] - 1.f, 0.f);
    }
}

inline bool v5_ok(const V5& v) { return v.p && v.N >= 1 && v.T >= 1 && v.H >= 1 && v.W >= 1 && v.C >= 4 && !(v.C % 4) && !(v.ld % 4) && v.ld >= v.C && !(v.sn % 4) && !((uintptr_t)v.p & 15); }

}  // namespace

size_t conv3d_weight_bytes(int Cin, int Cout, int KT, int KH, int KW) {
    return (size_t)conv3d_ksteps(Cin, KT, KH, KW) * CG_KC * round_up(Cout, CG_BN) * 4;
}

int conv3d_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, const float* bias_in, int Cin, int Cout, int KT, int KH, int KW,
                void* w32, void* w16, float* bias_out, hipStream_t st) {
    if (!w || Cin < 1 || Cout < 1 || KT < 1 || KH < 1 || KW < 1 || KT > 7 || KH > 7 || KW > 7) return -1;
    if ((beta || mean || var) && !(beta && mean && var)) return -1;
    if (gamma && !mean) return -1;
    const int gather = conv3d_gather(Cin, KW);
    if (!gather && (Cin % 8)) return -1;
    if (gather && Cin > 4) return -1;
    const long total = (long)(conv3d_weight_bytes(Cin, Cout, KT, KH, KW) / 4);
    hipLaunchKernelGGL(k_conv3d_pack, dim3(grid_for(total)), dim3(256), 0, st, w, gamma, beta, mean, var, eps, bias_in, Cin, Cout, KT * KH * KW, KW, gather,
                       conv3d_nchunk(Cin, KW), round_up(Cout, CG_BN) / 32, total, (float*)w32, (_Float16*)w16, bias_out);
    return launch_ok();
}

int conv3d_launch(const Conv3dArgs& a, hipStream_t st) {
    if (!a.in || !a.w || !a.out || a.N < 1 || a.To < 1 || a.Ho < 1 || a.Wo < 1 || a.Ti < 1 || a.Hi < 1 || a.Wi < 1 || a.Cin < 1 || a.Cout < 1) return -1;
    if (a.KT < 1 || a.KH < 1 || a.KW < 1 || a.KT > 7 || a.KH > 7 || a.KW > 7) return -1;
    if ((a.st != 1 && a.st != 2) || (a.sh != 1 && a.sh != 2) || (a.sw != 1 && a.sw != 2) || a.pt < 0 || a.ph < 0 || a.pw < 0 || a.pt >= a.KT || a.ph >= a.KH || a.pw >= a.KW) return -1;
    // the last output position's window starts inside the (leading-padded) input: every output has at least one real tap and trailing padding stays below the window
    if ((a.To - 1) * a.st - a.pt >= a.Ti || (a.Ho - 1) * a.sh - a.ph >= a.Hi || (a.Wo - 1) * a.sw - a.pw >= a.Wi) return -1;
    if (a.gather != conv3d_gather(a.Cin, a.KW) || a.nchunk != conv3d_nchunk(a.Cin, a.KW)) return -1;
    if (((uintptr_t)a.in & 15) || (a.in_sn % 4) || (a.in_ld % 4) || a.in_ld < a.Cin || a.out_ld < a.Cout) return -1;      // 16-byte loads
    if (a.gather ? (a.in_ld != 4 || a.Cin > 4) : (a.Cin % 8) != 0) return -1;
    if (a.precision != PREC_FP32 && a.precision != PREC_F16X3) return -1;
    const long M = (long)a.N * a.To * a.Ho * a.Wo;
    if (cdiv(M, CG_BM) < 1 || M > (long)CG_BM * 0x7fffffffL) return -1;
    const dim3 g((unsigned)cdiv(M, CG_BM), (unsigned)(round_up(a.Cout, CG_BN) / CG_BN));
    if (a.precision == PREC_FP32) hipLaunchKernelGGL((k_conv3d_igemm<false>), g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_conv3d_igemm<true>), g, dim3(256), 0, st, a);
    return launch_ok();
}

int fvd_pool_launch(const V5& in, const V5& out, int kt, int kh, int kw, int st, int sh, int sw, hipStream_t stream) {
    if (!v5_ok(in) || !v5_ok(out) || in.C != out.C || in.N != out.N) return -1;
    if (kt < 1 || kh < 1 || kw < 1 || kt > 3 || kh > 3 || kw > 3 || st < 1 || sh < 1 || sw < 1 || st > 2 || sh > 2 || sw > 2) return -1;
    if (out.T != same_out(in.T, st) || out.H != same_out(in.H, sh) || out.W != same_out(in.W, sw)) return -1;
    const long total = (long)out.N * out.T * out.H * out.W * (out.C / 4);
    hipLaunchKernelGGL(k_fvd_pool, dim3(grid_for(total)), dim3(256), 0, stream, in, out, kt, kh, kw, st, sh, sw, same_lead(in.T, kt, st), same_lead(in.H, kh, sh),
                       same_lead(in.W, kw, sw), total);
    return launch_ok();
}

int fvd_stage_launch(const float* src, long frames, int Hs, int Ws, float* out, int Ho, int Wo, hipStream_t st) {
    if (!src || !out || frames < 1 || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || ((uintptr_t)out & 15)) return -1;
    const long npix = frames * Ho * Wo;
    hipLaunchKernelGGL(k_fvd_stage, dim3(grid_for(npix)), dim3(256), 0, st, src, out, npix, Hs, Ws, Ho, Wo, (float)Hs / (float)Ho, (float)Ws / (float)Wo);
    return launch_ok();
}

// ---------------------------------------------------------------------------------------------------------------------
// The network: Kinetics I3D (Carreira & Zisserman, "Quo Vadis, Action Recognition?", the graph behind the hub module of evaluation/metrics/fvd.py:67-71), TF variable names
// ---------------------------------------------------------------------------------------------------------------------
#define FVD_EPS 0.001f
#define FVD_DIM 400
#define FVD_SIZE 224
struct FvdSpec { char name[96]; int cin, cout, kt, kh, kw, stride, bn; };      // bn 0: the logits layer (bias, no batch norm, no activation)
struct FvdLayer : PackedConv { FvdSpec s; long off = 0, gamma_off = 0; };
struct FvdState : TrunkState {
    int T = 0, resize = 1, Hn = FVD_SIZE, Wn = FVD_SIZE;      // frames per video; size the trunk runs at
    std::vector<FvdLayer> L;
    double* emb = nullptr;                   // max_videos x 400
    V5 taps[4]{};                            // outputs of Conv3d_2c, Mixed_3c, Mixed_4f, Mixed_5c of the last chunk
    int last_n = 0;
};

namespace {
inline V5 cslice(const V5& m, int c0, int C) { V5 s = m; s.p = m.p + c0; s.C = C; return s; }

// One description of the graph for its three uses: the parameter table (spec: nothing is allocated), workspace sizing (dry) and execution
struct FvdWalk {
    caddy_ctx* c = nullptr; FvdState* F = nullptr;
    std::vector<FvdSpec>* spec = nullptr;
    int li = 0;
    double macs = 0.0;
    V5 make(float* p, int N, int T, int H, int W, int C) { return V5{p, N, T, H, W, C, (long)T * H * W * C, C}; }
    V5 temp(int N, int T, int H, int W, int C) { return make(spec ? nullptr : (float*)c->act.alloc((size_t)N * T * H * W * C * 4), N, T, H, W, C); }
    // a unit: SAME-padded conv3d (k x k x k, one stride for the three axes) -> folded batch norm -> ReLU; bn 0: bias only
    V5 conv(const std::string& name, const V5& x, int cout, int k, int stride, const V5* into = nullptr, int bn = 1) {
        const int To = same_out(x.T, stride), Ho = same_out(x.H, stride), Wo = same_out(x.W, stride);
        V5 out = into ? *into : temp(x.N, To, Ho, Wo, cout);
        macs += (double)x.N * To * Ho * Wo * cout * k * k * k * x.C;
        if (spec) {
            FvdSpec s{}; snprintf(s.name, sizeof(s.name), "%s", name.c_str());
            s.cin = x.C; s.cout = cout; s.kt = s.kh = s.kw = k; s.stride = stride; s.bn = bn;
            spec->push_back(s);
            return out;
        }
        const int i = li++;
        if (i >= (int)F->L.size() || out.T != To || out.H != Ho || out.W != Wo || out.C != cout) { c->fail = true; set_error("internal: FVD graph walk out of step with its table"); return out; }
        if (c->dry) return out;
        const FvdLayer& L = F->L[i];
        Conv3dArgs a{};
        a.in = x.p; a.in_sn = x.sn; a.in_ld = x.ld; a.Cin = x.C; a.Ti = x.T; a.Hi = x.H; a.Wi = x.W;
        a.N = x.N; a.To = To; a.Ho = Ho; a.Wo = Wo; a.KT = a.KH = a.KW = k; a.st = a.sh = a.sw = stride;
        a.pt = same_lead(x.T, k, stride); a.ph = same_lead(x.H, k, stride); a.pw = same_lead(x.W, k, stride);
        a.precision = (F->precision == PREC_FP32 || c->layer_fallback[i]) ? PREC_FP32 : PREC_F16X3;      // a layer whose input left the f16 range runs exact from then on
        a.w = a.precision == PREC_FP32 ? L.w32 : L.w16;
        a.nchunk = conv3d_nchunk(x.C, k); a.gather = conv3d_gather(x.C, k);
        a.Cout = cout; a.bias = L.bias; a.relu = bn;
        a.out = out.p; a.out_sn = out.sn; a.out_ld = out.ld;
        a.sat_flag = c->sat_flag + i;
        c->ck(conv3d_launch(a, c->stream), L.s.name);
        return out;
    }
    V5 pool(const V5& x, int kt, int khw, int st, int shw, const V5* into = nullptr) {
        V5 out = into ? *into : temp(x.N, same_out(x.T, st), same_out(x.H, shw), same_out(x.W, shw), x.C);
        if (!spec && !c->dry) c->ck(fvd_pool_launch(x, out, kt, khw, khw, st, shw, shw, c->stream), "fvd pool");
        return out;
    }
    // Inception module: [1x1x1 | 1x1x1 -> 3x3x3 | 1x1x1 -> 3x3x3 | max pool 3x3x3 / 1 -> 1x1x1]; b2_alias: the published checkpoint's name of Mixed_5b's Branch_2 second convolution
    void mixed(const std::string& n, const V5& x, int b0, int b1a, int b1b, int b2a, int b2b, int b3, const V5& out) {
        V5 s = cslice(out, 0, b0); conv(n + "/Branch_0/Conv3d_0a_1x1", x, b0, 1, 1, &s);
        V5 t = conv(n + "/Branch_1/Conv3d_0a_1x1", x, b1a, 1, 1);
        s = cslice(out, b0, b1b); conv(n + "/Branch_1/Conv3d_0b_3x3", t, b1b, 3, 1, &s);
        t = conv(n + "/Branch_2/Conv3d_0a_1x1", x, b2a, 1, 1);
        s = cslice(out, b0 + b1b, b2b); conv(n + "/Branch_2/Conv3d_0b_3x3", t, b2b, 3, 1, &s);
        t = pool(x, 3, 3, 1, 1);
        s = cslice(out, b0 + b1b + b2b, b3); conv(n + "/Branch_3/Conv3d_0b_1x1", t, b3, 1, 1, &s);
    }
    void mark(int k) { if (!spec && !c->dry && F->timed) hipEventRecord(F->ev[k], c->stream); }

    // videos: (N, T, 3, H, W) device; the 400 logits of the N videos go to F->emb
    void run(const float* videos, int N, int T, int H, int W, int Hn, int Wn) {
        Arena* A = spec ? nullptr : &c->act;
        if (A) A->reset();
        const int T1 = same_out(T, 2), T2 = same_out(T1, 2), T3 = same_out(T2, 2);
        auto half = [](int s, int times) { for (int i = 0; i < times; i++) s = same_out(s, 2); return s; };
        const int h56 = half(Hn, 2), w56 = half(Wn, 2), h28 = half(Hn, 3), w28 = half(Wn, 3), h14 = half(Hn, 4), w14 = half(Wn, 4), h7 = half(Hn, 5), w7 = half(Wn, 5);
        // maps that outlive a phase first: the four tapped outputs and two block-output slots used in turn; temporaries of a phase above them, released at its end
        V5 tap0 = temp(N, T1, h56, w56, 192), tap1 = temp(N, T1, h28, w28, 480), tap2 = temp(N, T2, h14, w14, 832), tap3 = temp(N, T3, h7, w7, 1024);
        const size_t slot = std::max((size_t)T1 * h28 * w28 * 256, std::max((size_t)T2 * h14 * w14 * 528, (size_t)T3 * h7 * w7 * 832)) * (size_t)N * 4;
        float* P[2] = {spec ? nullptr : (float*)A->alloc(slot), spec ? nullptr : (float*)A->alloc(slot)};
        const size_t base = spec ? 0 : A->off;
        auto release = [&]() { if (A) A->off = base; };
        mark(0);
        V5 img = make(spec ? nullptr : (float*)A->alloc((size_t)N * T * Hn * Wn * 16), N, T, Hn, Wn, 3);
        img.ld = 4; img.sn = (long)T * Hn * Wn * 4;
        if (!spec && !c->dry) c->ck(fvd_stage_launch(videos, (long)N * T, H, W, img.p, Hn, Wn, c->stream), "fvd stage");
        mark(1);
        V5 x = conv("Conv3d_1a_7x7", img, 64, 7, 2);
        x = pool(x, 1, 3, 1, 2);
        x = conv("Conv3d_2b_1x1", x, 64, 1, 1);
        conv("Conv3d_2c_3x3", x, 192, 3, 1, &tap0);
        release();
        x = pool(tap0, 1, 3, 1, 2);
        mark(2);
        V5 a = make(P[0], N, T1, h28, w28, 256); mixed("Mixed_3b", x, 64, 96, 128, 16, 32, 32, a); release();
        mixed("Mixed_3c", a, 128, 128, 192, 32, 96, 64, tap1); release();
        x = pool(tap1, 3, 3, 2, 2);
        mark(3);
        a = make(P[0], N, T2, h14, w14, 512); mixed("Mixed_4b", x, 192, 96, 208, 16, 48, 64, a); release();
        V5 b = make(P[1], N, T2, h14, w14, 512); mixed("Mixed_4c", a, 160, 112, 224, 24, 64, 64, b); release();
        a = make(P[0], N, T2, h14, w14, 512); mixed("Mixed_4d", b, 128, 128, 256, 24, 64, 64, a); release();
        b = make(P[1], N, T2, h14, w14, 528); mixed("Mixed_4e", a, 112, 144, 288, 32, 64, 64, b); release();
        mixed("Mixed_4f", b, 256, 160, 320, 32, 128, 128, tap2); release();
        x = pool(tap2, 2, 2, 2, 2);
        mark(4);
        a = make(P[0], N, T3, h7, w7, 832); mixed("Mixed_5b", x, 256, 160, 320, 32, 128, 128, a); release();
        mixed("Mixed_5c", a, 384, 192, 384, 48, 128, 128, tap3); release();
        // head (fvd.py:118-125): average over (2, 7, 7) VALID stride 1 (the window clipped to the map), 1x1x1 convolution to the logits with bias, mean over what remains
        const int wt = std::min(2, T3), wh = std::min(7, h7), ww = std::min(7, w7);
        V5 avg = temp(N, T3 - wt + 1, h7 - wh + 1, w7 - ww + 1, 1024);
        if (!spec && !c->dry) {
            const long total = (long)avg.N * avg.T * avg.H * avg.W * (avg.C / 4);
            hipLaunchKernelGGL(k_fvd_avg, dim3(grid_for(total)), dim3(256), 0, c->stream, tap3, avg, wt, wh, ww, total);
            c->ck(launch_ok(), "fvd average pool");
        }
        V5 logits = conv("Logits/Conv3d_0c_1x1", avg, FVD_DIM, 1, 1, nullptr, 0);
        if (!spec && !c->dry) {
            hipLaunchKernelGGL(k_fvd_mean, dim3(grid_for((long)N * FVD_DIM)), dim3(256), 0, c->stream, logits, F->emb, (long)N * FVD_DIM);
            c->ck(launch_ok(), "fvd logits mean");
        }
        mark(5);
        if (!spec && !c->dry && F->timed) F->timed_ran = true;
        if (!spec) { F->taps[0] = tap0; F->taps[1] = tap1; F->taps[2] = tap2; F->taps[3] = tap3; F->last_n = N; }
    }
};

const std::vector<FvdSpec>& fvd_specs() {
    static std::vector<FvdSpec> S;
    if (S.empty()) { FvdWalk w; w.spec = &S; w.run(nullptr, 1, 16, FVD_SIZE, FVD_SIZE, FVD_SIZE, FVD_SIZE); }
    return S;
}
// flat parameter buffer: per layer [w (DHWIO) | beta | moving_mean | moving_variance] (logits: [w | b]), in graph order; then the optional batch-norm gammas of the 57 units
long fvd_weight_floats(const FvdSpec& s) { return (long)s.kt * s.kh * s.kw * s.cin * s.cout; }
long fvd_layer_floats(const FvdSpec& s) { return fvd_weight_floats(s) + (s.bn ? 3L : 1L) * s.cout; }
int fvd_required_params() { int n = 0; for (const FvdSpec& s : fvd_specs()) n += s.bn ? 4 : 2; return n; }
long fvd_required_floats() { long n = 0; for (const FvdSpec& s : fvd_specs()) n += fvd_layer_floats(s); return n; }

bool fvd_args_ok(int max_videos, int T, int H, int W) {
    if (max_videos < 1 || T < 1 || H < 1 || W < 1) { set_error("caddy_fvd: max_videos, frames, height and width must be positive"); return false; }
    if ((long)T * H * W > (1L << 28)) { set_error("caddy_fvd: videos of more than 2^28 pixels"); return false; }
    return true;
}
void fvd_chunk(caddy_ctx* c, const float* videos, int nv) {
    FvdWalk w; w.c = c; w.F = c->fvd;
    w.run(videos, nv, c->fvd->T, c->cfg.height, c->cfg.width, c->fvd->Hn, c->fvd->Wn);
}
const char* const FVD_SIZER = "caddy_fvd_workspace_bytes";
// FVD kind (caddy_fvd_ctx_create): both packed forms and the folded bias of every I3D layer, 400 logit doubles per video; the activation arena of one chunk of the walk
EvalKind fvd_kind(int max_videos, int T, int H, int W, int resize) {
    return {CTX_FVD, max_videos, H, W,
            [=](caddy_ctx* c) {
                FvdState* F = new FvdState();
                c->fvd = F;
                F->T = T; F->resize = resize ? 1 : 0; F->Hn = resize ? FVD_SIZE : H; F->Wn = resize ? FVD_SIZE : W;
                long off = 0, goff = fvd_required_floats();
                for (const FvdSpec& s : fvd_specs()) {
                    FvdLayer L{TrunkState::alloc_layer(c, conv3d_weight_bytes(s.cin, s.cout, s.kt, s.kh, s.kw), s.cout), s, off};
                    off += fvd_layer_floats(s);
                    if (s.bn) { L.gamma_off = goff; goff += s.cout; }
                    F->L.push_back(L);
                }
                F->emb = (double*)c->persist.alloc(sizeof(double) * FVD_DIM * (size_t)max_videos);
            },
            [=](caddy_ctx* c) { fvd_chunk(c, nullptr, max_videos); },
            FVD_SIZER};
}
bool fvd_ctx_ok(caddy_ctx* c, const char* who) {
    if (!ctx_needs(c, CTX_FVD, who)) return false;
    c->fail = false;
    return true;
}
}  // namespace

void fvd_free(caddy_ctx* c) {
    if (!c) return;
    delete c->fvd;
    c->fvd = nullptr;
}

extern "C" {
size_t caddy_fvd_workspace_bytes(int max_videos, int frames, int height, int width, int resize) {
    return fvd_args_ok(max_videos, frames, height, width) ? eval_workspace_bytes(fvd_kind(max_videos, frames, height, width, resize)) : 0;
}
caddy_ctx* caddy_fvd_ctx_create(int max_videos, int frames, int height, int width, int resize, void* workspace, size_t bytes) {
    return fvd_args_ok(max_videos, frames, height, width) ? eval_ctx_create(fvd_kind(max_videos, frames, height, width, resize), workspace, bytes) : nullptr;
}
int caddy_fvd_param_count(void) { int bn = 0; for (const FvdSpec& s : fvd_specs()) bn += s.bn; return fvd_required_params() + bn; }
long caddy_fvd_param_floats(void) { long n = fvd_required_floats(); for (const FvdSpec& s : fvd_specs()) if (s.bn) n += s.cout; return n; }
int caddy_fvd_param_info_get(int index, caddy_param_info* out, int* dhwio5) {
    const std::vector<FvdSpec>& S = fvd_specs();
    if (index < 0 || index >= caddy_fvd_param_count() || !out) return -1;
    memset(out, 0, sizeof(*out));
    out->kind = 3; out->ndim = 1; out->shape[1] = out->shape[2] = out->shape[3] = 1;
    if (dhwio5) for (int k = 0; k < 5; k++) dhwio5[k] = 0;
    long off = 0;
    int at = 0;
    const int req = fvd_required_params();
    if (index >= req) {      // optional gammas (kind 4: absent means 1)
        off = fvd_required_floats();
        for (const FvdSpec& s : S) {
            if (!s.bn) continue;
            if (at++ == index - req) { snprintf(out->name, sizeof(out->name), "%s/batch_norm/gamma", s.name); out->offset = off; out->shape[0] = s.cout; out->kind = 4; return 0; }
            off += s.cout;
        }
        return -1;
    }
    for (const FvdSpec& s : S) {
        const int leaves = s.bn ? 4 : 2;
        if (index < at + leaves) {
            const int leaf = index - at;
            const long nw = fvd_weight_floats(s);
            static const char* const BN_LEAVES[4] = {"conv_3d/w", "batch_norm/beta", "batch_norm/moving_mean", "batch_norm/moving_variance"};
            snprintf(out->name, sizeof(out->name), "%s/%s", s.name, s.bn ? BN_LEAVES[leaf] : (leaf ? "conv_3d/b" : "conv_3d/w"));
            if (leaf == 0) {
                out->offset = off; out->ndim = 3; out->shape[0] = s.kt * s.kh * s.kw; out->shape[1] = s.cin; out->shape[2] = s.cout;
                if (dhwio5) { dhwio5[0] = s.kt; dhwio5[1] = s.kh; dhwio5[2] = s.kw; dhwio5[3] = s.cin; dhwio5[4] = s.cout; }
            } else { out->offset = off + nw + (long)(leaf - 1) * s.cout; out->shape[0] = s.cout; }
            return 0;
        }
        at += leaves; off += fvd_layer_floats(s);
    }
    return -1;
}
int caddy_load_fvd_i3d(caddy_ctx* c, const float* flat) {
    if (!fvd_ctx_ok(c, "caddy_load_fvd_i3d")) return -2;
    if (!flat) { set_error("null input"); return -2; }
    for (FvdLayer& L : c->fvd->L) {
        const FvdSpec& s = L.s;
        const float* w = flat + L.off;
        const float* v = w + fvd_weight_floats(s);
        if (s.bn) c->ck(conv3d_pack(w, flat + L.gamma_off, v, v + s.cout, v + 2 * s.cout, FVD_EPS, nullptr, s.cin, s.cout, s.kt, s.kh, s.kw, L.w32, L.w16, L.bias, c->stream), s.name);
        else c->ck(conv3d_pack(w, nullptr, nullptr, nullptr, nullptr, 0.f, v, s.cin, s.cout, s.kt, s.kh, s.kw, L.w32, L.w16, L.bias, c->stream), s.name);
    }
    hipStreamSynchronize(c->stream);      // the caller's buffer is not referenced after this call
    c->fvd->loaded = !c->fail;
    return finish(c, FVD_SIZER);
}
int caddy_set_fvd_precision(caddy_ctx* c, int forward) {
    if (!fvd_ctx_ok(c, "caddy_set_fvd_precision")) return -2;
    return trunk_set_precision(*c->fvd, forward, "caddy_set_fvd_precision");
}
int caddy_fvd_embeddings(caddy_ctx* c, const float* videos, int n, double* out_host) {
    if (!fvd_ctx_ok(c, "caddy_fvd_embeddings")) return -2;
    if (!videos || !out_host) { set_error("null input"); return -2; }
    if (n < 1) { set_error("caddy_fvd_embeddings: n must be positive"); return -2; }
    FvdState* F = c->fvd;
    if (!F->loaded) { set_error("caddy_fvd_embeddings: no I3D weights were loaded (caddy_load_fvd_i3d)"); return -2; }
    const long vid = 3L * F->T * c->cfg.height * c->cfg.width;
    trunk_run_chunks(c, *F, n, (int)F->L.size(), [&](long n0, int nv) { fvd_chunk(c, videos + n0 * vid, nv); },
                     [&](long n0, int nv) { hipMemcpyAsync(out_host + n0 * FVD_DIM, F->emb, sizeof(double) * FVD_DIM * nv, hipMemcpyDeviceToHost, c->stream); });
    return finish(c, FVD_SIZER);
}
int caddy_debug_fvd_block(caddy_ctx* c, int block, float* dst_ncdhw) {
    if (!fvd_ctx_ok(c, "caddy_debug_fvd_block")) return -2;
    FvdState* F = c->fvd;
    if (block < 0 || block > 3 || !dst_ncdhw || F->last_n < 1) { set_error("caddy_debug_fvd_block: block 0..3 of a context that has run caddy_fvd_embeddings"); return -2; }
    const V5& t = F->taps[block];
    const TV v{t.p, t.N, t.T * t.H, t.W, t.C, t.sn, t.ld, 0};      // frames of a video are adjacent: (T, H) is one axis of T * H rows
    c->ck(pw_nhwc_to_nchw(v, dst_ncdhw, (long)t.C * t.T * t.H * t.W, 0, c->stream), "fvd block");
    hipStreamSynchronize(c->stream);
    return finish(c, FVD_SIZER);
}
int caddy_debug_fvd_fallback_layers(caddy_ctx* c) { return (c && c->kind == CTX_FVD) ? c->n_fallback : -1; }
/* on: the next chunks record events at the stage boundaries; ms5 (nullable) receives input stage, stem, Mixed_3, Mixed_4 and Mixed_5 + head times of the LAST chunk */
int caddy_debug_fvd_stage_ms(caddy_ctx* c, int on, float* ms5) {
    if (!fvd_ctx_ok(c, "caddy_debug_fvd_stage_ms")) return -2;
    return trunk_stage_ms(c, *c->fvd, on, ms5, 5, "caddy_debug_fvd_stage_ms");
}
double caddy_fvd_macs_per_video(int frames, int height, int width, int resize) {
    if (frames < 1 || height < 1 || width < 1) return 0.0;
    std::vector<FvdSpec> S; FvdWalk w; w.spec = &S;
    w.run(nullptr, 1, frames, height, width, resize ? FVD_SIZE : height, resize ? FVD_SIZE : width);
    return w.macs;
}
size_t caddy_k_conv3d_weight_bytes(int Cin, int Cout, int KT, int KH, int KW) { return conv3d_weight_bytes(Cin, Cout, KT, KH, KW); }
int caddy_k_conv3d_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, const float* bias_in, int Cin, int Cout, int KT, int KH,
                        int KW, void* w32, void* w16, float* bias_out, void* stream) {
    return conv3d_pack(w, gamma, beta, mean, var, eps, bias_in, Cin, Cout, KT, KH, KW, w32, w16, bias_out, (hipStream_t)stream);
}
int caddy_k_conv3d_igemm(const Conv3dArgs* a, void* stream) { return conv3d_launch(*a, (hipStream_t)stream); }
int caddy_k_fvd_pool(const V5* in, const V5* out, int kt, int kh, int kw, int st, int sh, int sw, void* stream) {
    return fvd_pool_launch(*in, *out, kt, kh, kw, st, sh, sw, (hipStream_t)stream);
}
int caddy_k_fvd_stage(const float* src, long frames, int Hs, int Ws, float* out, int Ho, int Wo, void* stream) { return fvd_stage_launch(src, frames, Hs, Ws, out, Ho, Wo, (hipStream_t)stream); }
}
