// FID feature network (fid.h).  Reference: evaluation/metrics/fid.py:98-159 feeds every frame of both datasets through pytorch_fid/inception.py's InceptionV3([3]) -- torchvision's
// Inception-v3 with the FID patches (inception.py:205-322: padding-excluding average pools in the A / C / E_1 blocks, a max pool in E_2) and the pt_inception-2015-12-05 weights --
// and keeps the 2048 pool_3 values per frame.  This file holds the kernels no other part of the library has (a general implicit-GEMM convolution, the 3x3 poolings, the global
// average, the 299 x 299 bilinear input stage), the walk over the 94 convolutions, and the C ABI of the FID context.
//
// k_conv_igemm is the tile of conv_igemm.h with K running over (tap, 32-channel chunk); a thread finds the tap and chunk of a K step by division.  The Cin = 3 first layer gathers
// its whole 27-element window from the pitch-4 image into ONE K chunk.
//
// Determinism: no atomics except the integer OR of the range flag; every output element has one writer and a fixed summation order, so two runs -- and two chunkings of the same
// frames -- give identical bits.
#include "conv_igemm.h"
#include "eval_ctx.h"
#include "fid.h"
#include <cstdio>
#include <cstring>

namespace {

template <bool F16>
__global__ __launch_bounds__(256) void k_conv_igemm(IgemmArgs a) {
    const int hw = a.Ho * a.Wo;
    const long M = (long)a.N * hw;
    // ---- loader role: tile pixel lrow, channels 8 lq .. 8 lq + 7 of the chunk ----
    const int lrow = threadIdx.x >> 2, lq = threadIdx.x & 3;
    const long lm = (long)blockIdx.x * CG_BM + lrow;
    const bool lvalid = lm < M;
    int ln = 0, loy = 0, lox = 0;
    if (lvalid) { ln = (int)(lm / hw); const int rem = (int)(lm - (long)ln * hw); loy = rem / a.Wo; lox = rem - loy * a.Wo; }
    const float* lbase = a.in + (long)ln * a.in_sn;
    const int iy0 = loy * a.stride - a.ph, ix0 = lox * a.stride - a.pw;
    auto load = [&](int step, float4& r0, float4& r1) {
        r0 = make_float4(0.f, 0.f, 0.f, 0.f); r1 = r0;
        if (a.gather) {
            float v[8];
            for (int e = 0; e < 8; e++) {
                const int k = lq * 8 + e, t = k / a.Cin, cc = k - t * a.Cin, ky = t / a.KW, kx = t - ky * a.KW;
                const int iy = iy0 + ky, ix = ix0 + kx;
                v[e] = (lvalid && t < a.KH * a.KW && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi) ? lbase[((long)iy * a.Wi + ix) * a.in_ld + cc] : 0.f;
            }
            r0 = make_float4(v[0], v[1], v[2], v[3]); r1 = make_float4(v[4], v[5], v[6], v[7]);
        } else {
            const int tap = step / a.nchunk, ch = step - tap * a.nchunk, ky = tap / a.KW, kx = tap - ky * a.KW;
            const int iy = iy0 + ky, ix = ix0 + kx, c = ch * CG_KC + lq * 8;
            if (lvalid && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi && c < a.Cin) {
                const float4* p = reinterpret_cast<const float4*>(lbase + ((long)iy * a.Wi + ix) * a.in_ld + c);
                r0 = p[0]; r1 = p[1];
            }
        }
    };
    const ConvTile t{a.w, a.Cout, a.bias, a.relu, a.out, a.out_sn, a.out_ld, a.sat_flag, M, hw, a.gather ? 1 : a.KH * a.KW * a.nchunk};
    conv_igemm_tile<F16>(t, load);
}

// one thread per padded (tap, chunk, channel block, channel of the chunk, output channel of the block) element: both packed forms + the folded bias
__global__ __launch_bounds__(256) void k_igemm_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, const float* bias_in,
                                                    int Cin, int Cout, int KH, int KW, int gather, int nchunk, int ncb, long total, float* w32, _Float16* w16, float* bias_out) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ol = (int)(i & 31), cl = (int)((i >> 5) & 31);
        const long tile = i >> 10;                       // (tap * nchunk + ch) * ncb + cb
        const int cb = (int)(tile % ncb); const long tc = tile / ncb;
        const int ch = (int)(tc % nchunk), tap = (int)(tc / nchunk);
        const int o = cb * 32 + ol;
        const double s = o < Cout ? conv_fold_scale(gamma, mean, var, eps, o) : 1.0;
        float v = 0.f;
        if (o < Cout) {
            if (gather) { const int t = cl / Cin, cc = cl - t * Cin; if (t < KH * KW) v = (float)((double)w[((long)o * Cin + cc) * KH * KW + t] * s); }
            else { const int c = ch * 32 + cl; if (c < Cin) v = (float)((double)w[((long)o * Cin + c) * KH * KW + tap] * s); }
        }
        conv_pack_store(w32, w16, tile, cl, ol, v);
        if (bias_out && tc == 0 && cl == 0 && o < Cout) bias_out[o] = conv_fold_bias(beta, mean, bias_in, s, o);
    }
}

// ---- 3 x 3 poolings, one thread per (output pixel, 4 channels) ----
template <int MODE>
__global__ __launch_bounds__(256) void k_fid_pool(TV in, TV out, long total) {
    const int C4 = out.C >> 2;
    const int stride = MODE == 0 ? 2 : 1, pad = MODE == 0 ? 0 : 1;
    constexpr bool AVG = MODE == 1 || MODE == 3;      // 3: count_include_pad=True, the padding adds zeros and the divisor is 9 everywhere
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4); long q = i / C4; const int x = (int)(q % out.W); q /= out.W; const int y = (int)(q % out.H); const long n = q / out.H;
        float4 m = AVG ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        int cnt = 0;
        for (int dy = 0; dy < 3; dy++) {
            const int iy = y * stride - pad + dy;
            if (iy < 0 || iy >= in.H) continue;
            for (int dx = 0; dx < 3; dx++) {
                const int ix = x * stride - pad + dx;
                if (ix < 0 || ix >= in.W) continue;
                const float4 v = *reinterpret_cast<const float4*>(in.p + n * in.sn + ((long)iy * in.W + ix) * in.ld + 4 * c);
                if (AVG) { m.x += v.x; m.y += v.y; m.z += v.z; m.w += v.w; cnt++; }
                else { m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w); }
            }
        }
        if (MODE == 1) { const float d = (float)cnt; m.x /= d; m.y /= d; m.z /= d; m.w /= d; }
        if (MODE == 3) { m.x /= 9.f; m.y /= 9.f; m.z /= 9.f; m.w /= 9.f; }
        *reinterpret_cast<float4*>(out.p + n * out.sn + ((long)y * out.W + x) * out.ld + 4 * c) = m;
    }
}

__global__ __launch_bounds__(256) void k_fid_global_avg(TV in, double* out, long total) {
    const int C4 = in.C >> 2, hw = in.H * in.W;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4); const long n = i / C4;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        const float* p = in.p + n * in.sn + 4 * c;
        for (int q = 0; q < hw; q++) { const float4 v = *reinterpret_cast<const float4*>(p + (long)q * in.ld); s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w; }
        double* o = out + n * in.C + 4 * c;
        o[0] = s0 / hw; o[1] = s1 / hw; o[2] = s2 / hw; o[3] = s3 / hw;
    }
}
__global__ __launch_bounds__(256) void k_fid_d2f(const double* src, float* dst, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = (float)src[i];
}

// source index and weights of torch's bilinear kernel for align_corners=False: src = max(scale (dst + 0.5) - 0.5, 0), scale = in / out in fp32
__device__ __forceinline__ void lerp_coord(int d, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
    float s = scale * ((float)d + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s; if (i0 > in - 1) i0 = in - 1;
    i1 = i0 < in - 1 ? i0 + 1 : i0;
    l1 = s - (float)i0; l0 = 1.f - l1;
}
template <bool NORM>      // NORM: pytorch_fid's 2 x - 1; without it the frames enter the first convolution as they are (torchvision's transform_input=False)
__global__ __launch_bounds__(256) void k_fid_stage(const float* src, float* out, long npix, int Hs, int Ws, int Ho, int Wo, float sy, float sx) {
    const long hws = (long)Hs * Ws;
    const bool same = Hs == Ho && Ws == Wo;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < npix; q += (long)gridDim.x * 256) {
        const long n = q / ((long)Ho * Wo); const int rem = (int)(q - n * Ho * Wo); const int y = rem / Wo, x = rem - y * Wo;
        const float* s = src + n * 3 * hws;
        float v[3];
        if (same) { for (int c = 0; c < 3; c++) v[c] = s[c * hws + (long)y * Ws + x]; }
        else {
            int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
            lerp_coord(y, sy, Hs, y0, y1, ly0, ly1);
            lerp_coord(x, sx, Ws, x0, x1, lx0, lx1);
            for (int c = 0; c < 3; c++) {
                const float* p = s + c * hws;
                v[c] = ly0 * (lx0 * p[(long)y0 * Ws + x0] + lx1 * p[(long)y0 * Ws + x1]) + ly1 * (lx0 * p[(long)y1 * Ws + x0] + lx1 * p[(long)y1 * Ws + x1]);
            }
        }
        reinterpret_cast<float4*>(out)[q] = NORM ? make_float4(2.f * v[0] - 1.f, 2.f * v[1] - 1.f, 2.f * v[2] - 1.f, 0.f) : make_float4(v[0], v[1], v[2], 0.f);
    }
}

// F.softmax over the C logits of a frame (evaluation/metrics/inception_score.py:43).  One wave64 per frame, four frames per workgroup; lane l holds columns l, l + 64, ...
// Max, then sum of exp(z - max), each by an xor-butterfly over the 64 lanes: every lane ends with the same bits, the order of the additions is fixed by the lane
// number alone, so a frame's probabilities depend on nothing but its logits.  No LDS, no atomics; ~10 VGPRs, so occupancy is bounded by the grid, not by registers.
__global__ __launch_bounds__(256) void k_is_softmax(const float* logits, float* probs, int n, int C, long ld_in, long ld_out) {
    const int lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n) return;      // (wave-uniform: the whole wave leaves)
    const float* z = logits + f * ld_in;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, z[c]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(z[c] - mx);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    float* p = probs + f * ld_out;
    for (int c = lane; c < C; c += 64) p[c] = expf(z[c] - mx) / s;
}

}  // namespace

size_t igemm_weight_bytes(int Cin, int Cout, int KH, int KW) {
    const long taps = igemm_gather(Cin, KH, KW) ? 1 : KH * KW;
    return (size_t)taps * igemm_nchunk(Cin, KH, KW) * CG_KC * round_up(Cout, CG_BN) * 4;
}

int igemm_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, const float* bias_in, int Cin, int Cout, int KH, int KW,
               void* w32, void* w16, float* bias_out, hipStream_t st) {
    if (!w || Cin < 1 || Cout < 1 || KH < 1 || KW < 1 || KH > 7 || KW > 7) return -1;
    if ((gamma || beta || mean || var) && !(gamma && beta && mean && var)) return -1;
    const int gather = igemm_gather(Cin, KH, KW);
    if (!gather && (Cin % 8)) return -1;
    const long total = (long)(igemm_weight_bytes(Cin, Cout, KH, KW) / 4);
    hipLaunchKernelGGL(k_igemm_pack, dim3(grid_for(total)), dim3(256), 0, st, w, gamma, beta, mean, var, eps, bias_in, Cin, Cout, KH, KW, gather,
                       igemm_nchunk(Cin, KH, KW), round_up(Cout, CG_BN) / 32, total, (float*)w32, (_Float16*)w16, bias_out);
    return launch_ok();
}

int igemm_launch(const IgemmArgs& a, hipStream_t st) {
    if (!a.in || !a.w || !a.out || a.N < 1 || a.Ho < 1 || a.Wo < 1 || a.Cout < 1 || (a.stride != 1 && a.stride != 2) || a.KH < 1 || a.KW < 1 || a.KH > 7 || a.KW > 7) return -1;
    if (a.Ho != igemm_out(a.Hi, a.KH, a.stride, a.ph) || a.Wo != igemm_out(a.Wi, a.KW, a.stride, a.pw)) return -1;
    if (a.gather != igemm_gather(a.Cin, a.KH, a.KW) || a.nchunk != igemm_nchunk(a.Cin, a.KH, a.KW)) return -1;
    if (!a.gather && ((a.Cin % 8) || (a.in_ld % 4) || ((uintptr_t)a.in & 15) || (a.in_sn % 4))) return -1;      // 16-byte loads of 8-channel groups
    if (a.precision != PREC_FP32 && a.precision != PREC_F16X3) return -1;
    const long M = (long)a.N * a.Ho * a.Wo;
    const dim3 g((unsigned)cdiv(M, CG_BM), (unsigned)(round_up(a.Cout, CG_BN) / CG_BN));
    if (a.precision == PREC_FP32) hipLaunchKernelGGL((k_conv_igemm<false>), g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_conv_igemm<true>), g, dim3(256), 0, st, a);
    return launch_ok();
}

int fid_pool_launch(const TV& in, const TV& out, int mode, hipStream_t st) {
    if (mode < 0 || mode > 3 || in.C != out.C || (in.C % 4) || (in.ld % 4) || (out.ld % 4) || in.N != out.N) return -1;
    const int Ho = mode == 0 ? (in.H - 3) / 2 + 1 : in.H, Wo = mode == 0 ? (in.W - 3) / 2 + 1 : in.W;
    if (in.H < 3 && mode == 0) return -1;
    if (out.H != Ho || out.W != Wo) return -1;
    const long total = (long)out.N * Ho * Wo * (out.C / 4);
    const dim3 g(grid_for(total)), b(256);
    if (mode == 0) hipLaunchKernelGGL((k_fid_pool<0>), g, b, 0, st, in, out, total);
    else if (mode == 1) hipLaunchKernelGGL((k_fid_pool<1>), g, b, 0, st, in, out, total);
    else if (mode == 2) hipLaunchKernelGGL((k_fid_pool<2>), g, b, 0, st, in, out, total);
    else hipLaunchKernelGGL((k_fid_pool<3>), g, b, 0, st, in, out, total);
    return launch_ok();
}

int fid_global_avg_launch(const TV& in, double* out, hipStream_t st) {
    if ((in.C % 4) || (in.ld % 4) || !out) return -1;
    const long total = (long)in.N * (in.C / 4);
    hipLaunchKernelGGL(k_fid_global_avg, dim3(grid_for(total)), dim3(256), 0, st, in, out, total);
    return launch_ok();
}

int fid_stage_launch(const float* src, int n, int Hs, int Ws, float* out, int Ho, int Wo, hipStream_t st, int normalise) {
    if (!src || !out || n < 1 || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1) return -1;
    const long npix = (long)n * Ho * Wo;
    const dim3 g(grid_for(npix)), b(256);
    const float sy = (float)Hs / (float)Ho, sx = (float)Ws / (float)Wo;
    if (normalise) hipLaunchKernelGGL((k_fid_stage<true>), g, b, 0, st, src, out, npix, Hs, Ws, Ho, Wo, sy, sx);
    else hipLaunchKernelGGL((k_fid_stage<false>), g, b, 0, st, src, out, npix, Hs, Ws, Ho, Wo, sy, sx);
    return launch_ok();
}

int is_softmax_launch(const float* logits, float* probs, int n, int C, long ld_in, long ld_out, hipStream_t st) {
    if (!logits || !probs || n < 1 || C < 1 || ld_in < C || ld_out < C) return -1;
    hipLaunchKernelGGL(k_is_softmax, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, logits, probs, n, C, ld_in, ld_out);
    return launch_ok();
}

// ---------------------------------------------------------------------------------------------------------------------
// The network: torchvision's Inception3 constructors (BasicConv2d = Conv2d(bias=False) -> BatchNorm2d(eps=0.001) -> ReLU) with the forward passes of
// pytorch_fid/inception.py:205-322, blocks as InceptionV3.__init__ groups them (inception.py:83-123)
// ---------------------------------------------------------------------------------------------------------------------
#define FID_EPS 0.001f
#define FID_DIM 2048
#define IS_CLASSES 1000
enum { FLAVOUR_FID = 0,      // pytorch_fid's patched network to pool_3
       FLAVOUR_TV = 1 };     // torchvision's inception_v3(transform_input=False).eval() to the softmax (evaluation/metrics/inception_score.py:20-22,41-43)
struct FidSpec { char name[96]; int cin, cout, kh, kw, stride, ph, pw; int linear; };      // linear: nn.Linear as a 1 x 1 convolution (weight + bias, no BatchNorm, no ReLU)
struct FidLayer : PackedConv { FidSpec s; long off = 0; };
struct FidState : TrunkState {
    int resize = 1, Hn = 299, Wn = 299;      // size the trunk runs at
    int flavour = FLAVOUR_FID;
    std::vector<FidLayer> L;
    double* feat = nullptr;                  // max_frames x 2048
    float *feat32 = nullptr, *logits = nullptr, *probs = nullptr;      // FLAVOUR_TV: the narrowed features (fc's input), max_frames x 1000 logits and probabilities
    TV taps[3]{};                            // block outputs 0 .. 2 of the last chunk (InceptionV3.BLOCK_INDEX_BY_DIM: 64, 192, 768 channels)
    int last_nf = 0;
};

namespace {
struct FMap { float* p; int N, H, W, C; long sn; int ld; };
inline TV tv(const FMap& m) { return TV{m.p, m.N, m.H, m.W, m.C, m.sn, m.ld, 0}; }
inline FMap cslice(const FMap& m, int c0, int C) { FMap s = m; s.p = m.p + c0; s.C = C; return s; }

// One description of the graph for its three uses: the parameter table (spec: nothing is allocated), workspace sizing (dry) and execution
struct FidWalk {
    caddy_ctx* c = nullptr; FidState* F = nullptr;
    std::vector<FidSpec>* spec = nullptr;
    int li = 0;
    int flavour = FLAVOUR_FID;
    double macs = 0.0;
    FMap make(float* p, int N, int H, int W, int C) { return FMap{p, N, H, W, C, (long)H * W * C, C}; }
    FMap temp(int N, int H, int W, int C) { return make(spec ? nullptr : (float*)c->act.alloc((size_t)N * H * W * C * 4), N, H, W, C); }
    FMap conv(const std::string& name, const FMap& x, int cout, int kh, int kw, int stride, int ph, int pw, const FMap* into = nullptr, int linear = 0) {
        const int Ho = igemm_out(x.H, kh, stride, ph), Wo = igemm_out(x.W, kw, stride, pw);
        FMap out = into ? *into : temp(x.N, Ho, Wo, cout);
        macs += (double)x.N * Ho * Wo * cout * kh * kw * x.C;
        if (spec) {
            FidSpec s{}; snprintf(s.name, sizeof(s.name), "%s", name.c_str());
            s.cin = x.C; s.cout = cout; s.kh = kh; s.kw = kw; s.stride = stride; s.ph = ph; s.pw = pw; s.linear = linear;
            spec->push_back(s);
            return out;
        }
        const int i = li++;
        if (i >= (int)F->L.size() || out.H != Ho || out.W != Wo || out.C != cout || Ho < 1 || Wo < 1) { c->fail = true; set_error("internal: FID graph walk out of step with its table"); return out; }
        if (c->dry) return out;
        const FidLayer& L = F->L[i];
        IgemmArgs a{};
        a.in = x.p; a.in_sn = x.sn; a.in_ld = x.ld; a.Cin = x.C; a.Hi = x.H; a.Wi = x.W;
        a.N = x.N; a.Ho = Ho; a.Wo = Wo; a.KH = kh; a.KW = kw; a.stride = stride; a.ph = ph; a.pw = pw;
        a.precision = (F->precision == PREC_FP32 || c->layer_fallback[i]) ? PREC_FP32 : PREC_F16X3;      // a layer whose input left the f16 range runs exact from then on
        a.w = a.precision == PREC_FP32 ? L.w32 : L.w16;
        a.nchunk = igemm_nchunk(x.C, kh, kw); a.gather = igemm_gather(x.C, kh, kw);
        a.Cout = cout; a.bias = L.bias; a.relu = linear ? 0 : 1;
        a.out = out.p; a.out_sn = out.sn; a.out_ld = out.ld;
        a.sat_flag = c->sat_flag + i;
        c->ck(igemm_launch(a, c->stream), L.s.name);
        return out;
    }
    FMap pool(const FMap& x, int mode, const FMap* into = nullptr) {
        const int Ho = mode == 0 ? (x.H - 3) / 2 + 1 : x.H, Wo = mode == 0 ? (x.W - 3) / 2 + 1 : x.W;
        FMap out = into ? *into : temp(x.N, Ho, Wo, x.C);
        if (!spec && !c->dry) c->ck(fid_pool_launch(tv(x), tv(out), mode, c->stream), "fid pool");
        return out;
    }
    // the A / C / E_1 average: padding-excluding under the FID patches, torchvision's own F.avg_pool2d(x, 3, 1, 1) (count_include_pad=True) otherwise
    int avg_mode() const { return flavour == FLAVOUR_TV ? 3 : 1; }
    // inception.py:205-227
    void blockA(const std::string& n, const FMap& x, int pf, const FMap& out) {
        FMap s;
        s = cslice(out, 0, 64); conv(n + ".branch1x1", x, 64, 1, 1, 1, 0, 0, &s);
        FMap t = conv(n + ".branch5x5_1", x, 48, 1, 1, 1, 0, 0);
        s = cslice(out, 64, 64); conv(n + ".branch5x5_2", t, 64, 5, 5, 1, 2, 2, &s);
        t = conv(n + ".branch3x3dbl_1", x, 64, 1, 1, 1, 0, 0);
        t = conv(n + ".branch3x3dbl_2", t, 96, 3, 3, 1, 1, 1);
        s = cslice(out, 128, 96); conv(n + ".branch3x3dbl_3", t, 96, 3, 3, 1, 1, 1, &s);
        t = pool(x, avg_mode());
        s = cslice(out, 224, pf); conv(n + ".branch_pool", t, pf, 1, 1, 1, 0, 0, &s);
    }
    // torchvision InceptionB (not patched)
    void blockB(const std::string& n, const FMap& x, const FMap& out) {
        FMap s;
        s = cslice(out, 0, 384); conv(n + ".branch3x3", x, 384, 3, 3, 2, 0, 0, &s);
        FMap t = conv(n + ".branch3x3dbl_1", x, 64, 1, 1, 1, 0, 0);
        t = conv(n + ".branch3x3dbl_2", t, 96, 3, 3, 1, 1, 1);
        s = cslice(out, 384, 96); conv(n + ".branch3x3dbl_3", t, 96, 3, 3, 2, 0, 0, &s);
        s = cslice(out, 480, x.C); pool(x, 0, &s);
    }
    // inception.py:230-255
    void blockC(const std::string& n, const FMap& x, int c7, const FMap& out) {
        FMap s;
        s = cslice(out, 0, 192); conv(n + ".branch1x1", x, 192, 1, 1, 1, 0, 0, &s);
        FMap t = conv(n + ".branch7x7_1", x, c7, 1, 1, 1, 0, 0);
        t = conv(n + ".branch7x7_2", t, c7, 1, 7, 1, 0, 3);
        s = cslice(out, 192, 192); conv(n + ".branch7x7_3", t, 192, 7, 1, 1, 3, 0, &s);
        t = conv(n + ".branch7x7dbl_1", x, c7, 1, 1, 1, 0, 0);
        t = conv(n + ".branch7x7dbl_2", t, c7, 7, 1, 1, 3, 0);
        t = conv(n + ".branch7x7dbl_3", t, c7, 1, 7, 1, 0, 3);
        t = conv(n + ".branch7x7dbl_4", t, c7, 7, 1, 1, 3, 0);
        s = cslice(out, 384, 192); conv(n + ".branch7x7dbl_5", t, 192, 1, 7, 1, 0, 3, &s);
        t = pool(x, avg_mode());
        s = cslice(out, 576, 192); conv(n + ".branch_pool", t, 192, 1, 1, 1, 0, 0, &s);
    }
    // torchvision InceptionD (not patched)
    void blockD(const std::string& n, const FMap& x, const FMap& out) {
        FMap s;
        FMap t = conv(n + ".branch3x3_1", x, 192, 1, 1, 1, 0, 0);
        s = cslice(out, 0, 320); conv(n + ".branch3x3_2", t, 320, 3, 3, 2, 0, 0, &s);
        t = conv(n + ".branch7x7x3_1", x, 192, 1, 1, 1, 0, 0);
        t = conv(n + ".branch7x7x3_2", t, 192, 1, 7, 1, 0, 3);
        t = conv(n + ".branch7x7x3_3", t, 192, 7, 1, 1, 3, 0);
        s = cslice(out, 320, 192); conv(n + ".branch7x7x3_4", t, 192, 3, 3, 2, 0, 0, &s);
        s = cslice(out, 512, x.C); pool(x, 0, &s);
    }
    // inception.py:258-322 (pool_mode 1: E_1's padding-excluding average, 2: E_2's max pool; torchvision's own E blocks both take mode 3)
    void blockE(const std::string& n, const FMap& x, int pool_mode, const FMap& out) {
        FMap s;
        s = cslice(out, 0, 320); conv(n + ".branch1x1", x, 320, 1, 1, 1, 0, 0, &s);
        FMap t = conv(n + ".branch3x3_1", x, 384, 1, 1, 1, 0, 0);
        s = cslice(out, 320, 384); conv(n + ".branch3x3_2a", t, 384, 1, 3, 1, 0, 1, &s);
        s = cslice(out, 704, 384); conv(n + ".branch3x3_2b", t, 384, 3, 1, 1, 1, 0, &s);
        t = conv(n + ".branch3x3dbl_1", x, 448, 1, 1, 1, 0, 0);
        t = conv(n + ".branch3x3dbl_2", t, 384, 3, 3, 1, 1, 1);
        s = cslice(out, 1088, 384); conv(n + ".branch3x3dbl_3a", t, 384, 1, 3, 1, 0, 1, &s);
        s = cslice(out, 1472, 384); conv(n + ".branch3x3dbl_3b", t, 384, 3, 1, 1, 1, 0, &s);
        t = pool(x, pool_mode);
        s = cslice(out, 1856, 192); conv(n + ".branch_pool", t, 192, 1, 1, 1, 0, 0, &s);
    }
    void mark(int k) { if (!spec && !c->dry && F->timed) hipEventRecord(F->ev[k], c->stream); }

    // frames: (N, 3, H, W) device; the 2048 features of the N frames go to F->feat
    void run(const float* frames, int N, int H, int W, int Hn, int Wn) {
        Arena* A = spec ? nullptr : &c->act;
        if (A) A->reset();
        mark(0);
        FMap img = make(spec ? nullptr : (float*)A->alloc((size_t)N * Hn * Wn * 16), N, Hn, Wn, 3);
        img.ld = 4; img.sn = (long)Hn * Wn * 4;
        if (!spec && !c->dry) c->ck(fid_stage_launch(frames, N, H, W, img.p, Hn, Wn, c->stream, flavour == FLAVOUR_FID), "fid stage");
        mark(1);
        const int h1 = igemm_out(Hn, 3, 2, 0), w1 = igemm_out(Wn, 3, 2, 0), h2 = h1 - 2, w2 = w1 - 2, h3 = (h2 - 3) / 2 + 1, w3 = (w2 - 3) / 2 + 1;
        const int h4 = h3 - 2, w4 = w3 - 2, h35 = (h4 - 3) / 2 + 1, w35 = (w4 - 3) / 2 + 1, h17 = (h35 - 3) / 2 + 1, w17 = (w35 - 3) / 2 + 1, h8 = (h17 - 3) / 2 + 1, w8 = (w17 - 3) / 2 + 1;
        // maps that outlive a phase first: the three tapped block outputs and two block-output slots used in turn; temporaries of a phase above them, released at its end
        FMap tap0 = temp(N, h3, w3, 64), tap1 = temp(N, h35, w35, 192), tap2 = temp(N, h17, w17, 768);
        const size_t slot = std::max((size_t)h35 * w35 * 288, std::max((size_t)h17 * w17 * 768, (size_t)h8 * w8 * 2048)) * (size_t)N * 4;
        float* P[2] = {spec ? nullptr : (float*)A->alloc(slot), spec ? nullptr : (float*)A->alloc(slot)};
        const size_t base = spec ? 0 : A->off;
        auto release = [&]() { if (A) A->off = base; };
        // block 0 / 1 (inception.py:84-99)
        FMap x = conv("Conv2d_1a_3x3", img, 32, 3, 3, 2, 0, 0);
        x = conv("Conv2d_2a_3x3", x, 32, 3, 3, 1, 0, 0);
        x = conv("Conv2d_2b_3x3", x, 64, 3, 3, 1, 1, 1);
        pool(x, 0, &tap0);
        release();
        x = conv("Conv2d_3b_1x1", tap0, 80, 1, 1, 1, 0, 0);
        x = conv("Conv2d_4a_3x3", x, 192, 3, 3, 1, 0, 0);
        pool(x, 0, &tap1);
        release();
        mark(2);
        // block 2 (inception.py:103-112)
        FMap a = make(P[0], N, h35, w35, 256); blockA("Mixed_5b", tap1, 32, a); release();
        FMap b = make(P[1], N, h35, w35, 288); blockA("Mixed_5c", a, 64, b); release();
        a = make(P[0], N, h35, w35, 288); blockA("Mixed_5d", b, 64, a); release();
        mark(3);
        b = make(P[1], N, h17, w17, 768); blockB("Mixed_6a", a, b); release();
        a = make(P[0], N, h17, w17, 768); blockC("Mixed_6b", b, 128, a); release();
        blockC("Mixed_6c", a, 160, b); release();
        blockC("Mixed_6d", b, 160, a); release();
        blockC("Mixed_6e", a, 192, tap2); release();
        mark(4);
        // block 3 (inception.py:116-122)
        a = make(P[0], N, h8, w8, 1280); blockD("Mixed_7a", tap2, a); release();
        b = make(P[1], N, h8, w8, 2048); blockE("Mixed_7b", a, avg_mode(), b); release();
        a = make(P[0], N, h8, w8, 2048); blockE("Mixed_7c", b, flavour == FLAVOUR_TV ? 3 : 2, a); release();
        if (!spec && !c->dry) c->ck(fid_global_avg_launch(tv(a), F->feat, c->stream), "fid global average");
        mark(5);
        if (flavour == FLAVOUR_TV) {      // torchvision's tail: dropout is the identity in eval mode, then fc and (inception_score.py:43) the softmax
            const bool live = !spec && !c->dry;
            if (live) hipLaunchKernelGGL(k_fid_d2f, dim3(grid_for((long)N * FID_DIM)), dim3(256), 0, c->stream, (const double*)F->feat, F->feat32, (long)N * FID_DIM);
            FMap pooled = make(spec ? nullptr : F->feat32, N, 1, 1, FID_DIM), lg = make(spec ? nullptr : F->logits, N, 1, 1, IS_CLASSES);
            conv("fc", pooled, IS_CLASSES, 1, 1, 1, 0, 0, &lg, 1);
            if (live) c->ck(is_softmax_launch(F->logits, F->probs, N, IS_CLASSES, IS_CLASSES, IS_CLASSES, c->stream), "is softmax");
            mark(6);
        }
        if (!spec && !c->dry && F->timed) F->timed_ran = true;
        if (!spec) { F->taps[0] = tv(tap0); F->taps[1] = tv(tap1); F->taps[2] = tv(tap2); F->last_nf = N; }
    }
};

const std::vector<FidSpec>& fid_specs(int flavour = FLAVOUR_FID) {
    static std::vector<FidSpec> S[2];
    if (S[flavour].empty()) { FidWalk w; w.spec = &S[flavour]; w.flavour = flavour; w.run(nullptr, 1, 299, 299, 299, 299); }
    return S[flavour];
}
const char* const FID_LEAVES[5] = {"conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"};
const char* const FC_LEAVES[2] = {"weight", "bias"};
inline int fid_layer_leaves(const FidSpec& s) { return s.linear ? 2 : 5; }
long fid_layer_floats(const FidSpec& s) { return (long)s.cout * s.cin * s.kh * s.kw + (s.linear ? 1L : 4L) * s.cout; }
int fid_param_count(int flavour) { int n = 0; for (const FidSpec& s : fid_specs(flavour)) n += fid_layer_leaves(s); return n; }
long fid_param_floats(int flavour) { long n = 0; for (const FidSpec& s : fid_specs(flavour)) n += fid_layer_floats(s); return n; }
int fid_param_info(int flavour, int index, caddy_param_info* out) {
    if (index < 0 || !out) return -1;
    long off = 0;
    for (const FidSpec& s : fid_specs(flavour)) {
        const int leaves = fid_layer_leaves(s);
        if (index >= leaves) { index -= leaves; off += fid_layer_floats(s); continue; }
        const long nw = (long)s.cout * s.cin * s.kh * s.kw;
        memset(out, 0, sizeof(*out));
        snprintf(out->name, sizeof(out->name), "%s.%s", s.name, s.linear ? FC_LEAVES[index] : FID_LEAVES[index]);
        out->kind = 3;
        out->shape[0] = s.cout; out->shape[1] = out->shape[2] = out->shape[3] = 1;
        if (index == 0) {
            out->offset = off; out->shape[1] = s.cin;
            if (s.linear) out->ndim = 2; else { out->ndim = 4; out->shape[2] = s.kh; out->shape[3] = s.kw; }
        } else { out->offset = off + nw + (long)(index - 1) * s.cout; out->ndim = 1; }
        return 0;
    }
    return -1;
}

bool fid_args_ok(int max_frames, int H, int W, int resize, const char* who = "caddy_fid") {
    if (max_frames < 1 || H < 1 || W < 1) { set_error(std::string(who) + ": max_frames, height and width must be positive"); return false; }
    if (!resize && (H < 75 || W < 75)) { set_error(std::string(who) + ": without the 299 x 299 resize the Inception trunk needs frames of at least 75 x 75"); return false; }
    return true;
}
void fid_chunk(caddy_ctx* c, const float* frames, int nf) {
    FidWalk w; w.c = c; w.F = c->fid; w.flavour = c->fid->flavour;
    w.run(frames, nf, c->cfg.height, c->cfg.width, c->fid->Hn, c->fid->Wn);
}
const char* const FID_SIZER = "caddy_fid_workspace_bytes";
const char* const IS_SIZER = "caddy_is_workspace_bytes";
// FID kind (caddy_fid_ctx_create): both packed forms and the folded bias of every Inception layer, 2048 feature doubles per frame; the activation arena of one chunk of the walk.
// IS kind (caddy_is_ctx_create): the same with the torchvision flavour of the walk, its fc layer, and per frame the narrowed features, 1000 logits and 1000 probabilities.
EvalKind fid_kind(int max_frames, int H, int W, int resize, int flavour = FLAVOUR_FID) {
    return {flavour == FLAVOUR_TV ? CTX_IS : CTX_FID, max_frames, H, W,
            [=](caddy_ctx* c) {
                FidState* F = new FidState();
                c->fid = F;
                F->flavour = flavour;
                F->resize = resize ? 1 : 0; F->Hn = resize ? 299 : H; F->Wn = resize ? 299 : W;
                long off = 0;
                for (const FidSpec& s : fid_specs(flavour)) {
                    FidLayer L{TrunkState::alloc_layer(c, igemm_weight_bytes(s.cin, s.cout, s.kh, s.kw), s.cout), s, off};
                    off += fid_layer_floats(s);
                    F->L.push_back(L);
                }
                F->feat = (double*)c->persist.alloc(sizeof(double) * FID_DIM * (size_t)max_frames);
                if (flavour == FLAVOUR_TV) {
                    F->feat32 = (float*)c->persist.alloc(sizeof(float) * FID_DIM * (size_t)max_frames);
                    F->logits = (float*)c->persist.alloc(sizeof(float) * IS_CLASSES * (size_t)max_frames);
                    F->probs = (float*)c->persist.alloc(sizeof(float) * IS_CLASSES * (size_t)max_frames);
                }
            },
            [=](caddy_ctx* c) { fid_chunk(c, nullptr, max_frames); },
            flavour == FLAVOUR_TV ? IS_SIZER : FID_SIZER};
}
bool fid_ctx_ok(caddy_ctx* c, const char* who, int kind = CTX_FID) {
    if (!ctx_needs(c, kind, who)) return false;
    c->fail = false;
    return true;
}
int fid_load(caddy_ctx* c, const float* flat, const char* sizer) {
    if (!flat) { set_error("null input"); return -2; }
    for (FidLayer& L : c->fid->L) {
        const FidSpec& s = L.s;
        const float* w = flat + L.off;
        const float* bn = w + (long)s.cout * s.cin * s.kh * s.kw;      // the four BatchNorm vectors, or fc's bias
        if (s.linear) c->ck(igemm_pack(w, nullptr, nullptr, nullptr, nullptr, 0.f, bn, s.cin, s.cout, s.kh, s.kw, L.w32, L.w16, L.bias, c->stream), s.name);
        else c->ck(igemm_pack(w, bn, bn + s.cout, bn + 2 * s.cout, bn + 3 * s.cout, FID_EPS, nullptr, s.cin, s.cout, s.kh, s.kw, L.w32, L.w16, L.bias, c->stream), s.name);
    }
    hipStreamSynchronize(c->stream);      // the caller's buffer is not referenced after this call
    c->fid->loaded = !c->fail;
    return finish(c, sizer);
}
// every chunk of n frames through the walk, range-guarded (trunk_run_chunks).  copy(n0, nf) fetches a chunk's result.
template <class Copy> void fid_run_chunks(caddy_ctx* c, const float* frames, int n, Copy copy) {
    const long fr = 3L * c->cfg.height * c->cfg.width;
    trunk_run_chunks(c, *c->fid, n, (int)c->fid->L.size(), [&](long n0, int nf) { fid_chunk(c, frames + n0 * fr, nf); }, copy);
}
}  // namespace

void fid_free(caddy_ctx* c) {
    if (!c) return;
    delete c->fid;
    c->fid = nullptr;
}

extern "C" {
size_t caddy_fid_workspace_bytes(int max_frames, int height, int width, int resize) {
    return fid_args_ok(max_frames, height, width, resize) ? eval_workspace_bytes(fid_kind(max_frames, height, width, resize)) : 0;
}
caddy_ctx* caddy_fid_ctx_create(int max_frames, int height, int width, int resize, void* workspace, size_t bytes) {
    return fid_args_ok(max_frames, height, width, resize) ? eval_ctx_create(fid_kind(max_frames, height, width, resize), workspace, bytes) : nullptr;
}
int caddy_fid_param_count(void) { return fid_param_count(FLAVOUR_FID); }
long caddy_fid_param_floats(void) { return fid_param_floats(FLAVOUR_FID); }
int caddy_fid_param_info_get(int index, caddy_param_info* out) { return fid_param_info(FLAVOUR_FID, index, out); }
int caddy_load_fid_inception(caddy_ctx* c, const float* flat) {
    if (!fid_ctx_ok(c, "caddy_load_fid_inception")) return -2;
    return fid_load(c, flat, FID_SIZER);
}
int caddy_set_fid_precision(caddy_ctx* c, int forward) {
    if (!fid_ctx_ok(c, "caddy_set_fid_precision")) return -2;
    return trunk_set_precision(*c->fid, forward, "caddy_set_fid_precision");
}
int caddy_fid_features(caddy_ctx* c, const float* frames, int n, double* out_host) {
    if (!fid_ctx_ok(c, "caddy_fid_features")) return -2;
    if (!frames || !out_host) { set_error("null input"); return -2; }
    if (n < 1) { set_error("caddy_fid_features: n must be positive"); return -2; }
    FidState* F = c->fid;
    if (!F->loaded) { set_error("caddy_fid_features: no Inception weights were loaded (caddy_load_fid_inception)"); return -2; }
    fid_run_chunks(c, frames, n, [&](long n0, int nf) { hipMemcpyAsync(out_host + n0 * FID_DIM, F->feat, sizeof(double) * FID_DIM * nf, hipMemcpyDeviceToHost, c->stream); });
    return finish(c, FID_SIZER);
}
int caddy_debug_fid_block(caddy_ctx* c, int block, float* dst_nchw) {
    if (!fid_ctx_ok(c, "caddy_debug_fid_block")) return -2;
    FidState* F = c->fid;
    if (block < 0 || block > 3 || !dst_nchw || F->last_nf < 1) { set_error("caddy_debug_fid_block: block 0..3 of a context that has run caddy_fid_features"); return -2; }
    if (block == 3) hipLaunchKernelGGL(k_fid_d2f, dim3(grid_for((long)F->last_nf * FID_DIM)), dim3(256), 0, c->stream, (const double*)F->feat, dst_nchw, (long)F->last_nf * FID_DIM);
    else c->ck(pw_nhwc_to_nchw(F->taps[block], dst_nchw, (long)F->taps[block].C * F->taps[block].H * F->taps[block].W, 0, c->stream), "fid block");
    hipStreamSynchronize(c->stream);
    return finish(c, FID_SIZER);
}
int caddy_debug_fid_fallback_layers(caddy_ctx* c) { return (c && c->kind == CTX_FID) ? c->n_fallback : -1; }
/* on: the next chunks record events at the stage boundaries; ms5 (nullable) receives resize, stem, 35 x 35, 17 x 17 and 8 x 8 times of the LAST chunk */
int caddy_debug_fid_stage_ms(caddy_ctx* c, int on, float* ms5) {
    if (!fid_ctx_ok(c, "caddy_debug_fid_stage_ms")) return -2;
    return trunk_stage_ms(c, *c->fid, on, ms5, 5, "caddy_debug_fid_stage_ms");
}
double caddy_fid_macs_per_frame(int height, int width, int resize) {
    std::vector<FidSpec> S; FidWalk w; w.spec = &S;
    w.run(nullptr, 1, height, width, resize ? 299 : height, resize ? 299 : width);
    return w.macs;
}
size_t caddy_k_igemm_weight_bytes(int Cin, int Cout, int KH, int KW) { return igemm_weight_bytes(Cin, Cout, KH, KW); }
int caddy_k_igemm_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, const float* bias_in, int Cin, int Cout, int KH, int KW,
                       void* w32, void* w16, float* bias_out, void* stream) {
    return igemm_pack(w, gamma, beta, mean, var, eps, bias_in, Cin, Cout, KH, KW, w32, w16, bias_out, (hipStream_t)stream);
}
int caddy_k_conv_igemm(const IgemmArgs* a, void* stream) { return igemm_launch(*a, (hipStream_t)stream); }
int caddy_k_fid_pool(const TV* in, const TV* out, int mode, void* stream) { return fid_pool_launch(*in, *out, mode, (hipStream_t)stream); }
int caddy_k_fid_global_avg(const TV* in, double* out, void* stream) { return fid_global_avg_launch(*in, out, (hipStream_t)stream); }
int caddy_k_fid_stage(const float* src, int n, int Hs, int Ws, float* out, int Ho, int Wo, void* stream) { return fid_stage_launch(src, n, Hs, Ws, out, Ho, Wo, (hipStream_t)stream); }

// ---- Inception Score (evaluation/metrics/inception_score.py): the IS context and its entry points ----
size_t caddy_is_workspace_bytes(int max_frames, int height, int width, int resize) {
    return fid_args_ok(max_frames, height, width, resize, "caddy_is") ? eval_workspace_bytes(fid_kind(max_frames, height, width, resize, FLAVOUR_TV)) : 0;
}
caddy_ctx* caddy_is_ctx_create(int max_frames, int height, int width, int resize, void* workspace, size_t bytes) {
    return fid_args_ok(max_frames, height, width, resize, "caddy_is") ? eval_ctx_create(fid_kind(max_frames, height, width, resize, FLAVOUR_TV), workspace, bytes) : nullptr;
}
int caddy_is_param_count(void) { return fid_param_count(FLAVOUR_TV); }
long caddy_is_param_floats(void) { return fid_param_floats(FLAVOUR_TV); }
int caddy_is_param_info_get(int index, caddy_param_info* out) { return fid_param_info(FLAVOUR_TV, index, out); }
int caddy_load_is_inception(caddy_ctx* c, const float* flat) {
    if (!fid_ctx_ok(c, "caddy_load_is_inception", CTX_IS)) return -2;
    return fid_load(c, flat, IS_SIZER);
}
int caddy_set_is_precision(caddy_ctx* c, int forward) {
    if (!fid_ctx_ok(c, "caddy_set_is_precision", CTX_IS)) return -2;
    return trunk_set_precision(*c->fid, forward, "caddy_set_is_precision");
}
int caddy_is_probabilities(caddy_ctx* c, const float* frames, int n, float* out_host) {
    if (!fid_ctx_ok(c, "caddy_is_probabilities", CTX_IS)) return -2;
    if (!frames || !out_host) { set_error("null input"); return -2; }
    if (n < 1) { set_error("caddy_is_probabilities: n must be positive"); return -2; }
    FidState* F = c->fid;
    if (!F->loaded) { set_error("caddy_is_probabilities: no Inception weights were loaded (caddy_load_is_inception)"); return -2; }
    fid_run_chunks(c, frames, n, [&](long n0, int nf) { hipMemcpyAsync(out_host + n0 * IS_CLASSES, F->probs, sizeof(float) * IS_CLASSES * nf, hipMemcpyDeviceToHost, c->stream); });
    return finish(c, IS_SIZER);
}
int caddy_debug_is_logits(caddy_ctx* c, float* dst) {
    if (!fid_ctx_ok(c, "caddy_debug_is_logits", CTX_IS)) return -2;
    FidState* F = c->fid;
    if (!dst || F->last_nf < 1) { set_error("caddy_debug_is_logits: needs a context that has run caddy_is_probabilities"); return -2; }
    hipMemcpyAsync(dst, F->logits, sizeof(float) * IS_CLASSES * F->last_nf, hipMemcpyDeviceToDevice, c->stream);
    hipStreamSynchronize(c->stream);
    return finish(c, IS_SIZER);
}
int caddy_debug_is_fallback_layers(caddy_ctx* c) { return (c && c->kind == CTX_IS) ? c->n_fallback : -1; }
int caddy_debug_is_stage_ms(caddy_ctx* c, int on, float* ms6) {
    if (!fid_ctx_ok(c, "caddy_debug_is_stage_ms", CTX_IS)) return -2;
    return trunk_stage_ms(c, *c->fid, on, ms6, 6, "caddy_debug_is_stage_ms");
}
double caddy_is_macs_per_frame(int height, int width, int resize) {
    std::vector<FidSpec> S; FidWalk w; w.spec = &S; w.flavour = FLAVOUR_TV;
    w.run(nullptr, 1, height, width, resize ? 299 : height, resize ? 299 : width);
    return w.macs;
}
int caddy_k_is_stage(const float* src, int n, int Hs, int Ws, float* out, int Ho, int Wo, void* stream) { return fid_stage_launch(src, n, Hs, Ws, out, Ho, Wo, (hipStream_t)stream, 0); }
int caddy_k_is_softmax(const float* logits, float* probs, int n, int C, long ld_in, long ld_out, void* stream) { return is_softmax_launch(logits, probs, n, C, ld_in, ld_out, (hipStream_t)stream); }
}
