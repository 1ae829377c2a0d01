// VGG19 perceptual loss, forward + input gradient, fused into caddy_loss_backward.
//
// Reference: training/losses.py:379-491 (ParallelPerceptualLoss -> UnmeanedPerceptualLoss), model/layers/vgg.py:8-56 (slices of
// torchvision's vgg19().features up to relu5_1), training/trainer.py:442-466,494-500 (per-resolution sum, sum_loss_components, the
// term in the total loss).  Per resolution r in {1, 1/2, 1/4}: VGG19 features of the bilinearly resized ground truth (no gradient) and of
// the reconstruction at relu1_1 .. relu5_1, per level mean |f_gt - f_rec|, and the gradient of the weighted sum w.r.t. the reconstruction
// (the VGG weights are frozen: dgrad only, no wgrad).  Inputs in [-1, 1] are fed as they are -- the reference applies no ImageNet
// normalisation.
//
// Reference quirk reproduced on purpose (pinned by tests/golden/perc_*.npz): losses.py:483-487 binds `total_loss` to the level-0 tensor
// and then accumulates the other levels into it IN PLACE, so the "level 0" entry handed to Trainer.sum_loss_components IS the total:
//   term_r = lambda * (l0 + 2 (l1 + l2 + l3 + l4)),   logged perceptual_loss_r{r}_l0 == perceptual_loss_r{r}.
//
// Convolutions run on the conv kernels of this library (13 x conv3x3 + bias + ReLU forward on 2N images per resolution; the dgrad of the
// reconstruction branch with the ReLU mask and the L1 seed of the tapped feature maps fused into the epilogue: ConvArgs.mask / seed_ref).
// The kernels here are the 2x2 max-pool (forward; backward fused with the ReLU mask of the layer below) and the feature L1.
#include "net.h"
#include "perceptual.h"
#include "lpips.h"
#include <cstdio>
#include <cstring>

#define RUN_CK(c, expr) do { if (!(c)->dry) (c)->ck((expr), #expr); } while (0)

namespace {

// torchvision vgg19().features: (index, Cin, Cout) of the 13 convolutions the reference evaluates; pool_before: MaxPool2d(2,2) on the input
const VggSpec VGG19_SPEC[VGG_NCONV] = {
    {0, 3, 64, 0, 0}, {2, 64, 64, 0, -1}, {5, 64, 128, 1, 1}, {7, 128, 128, 0, -1}, {10, 128, 256, 1, 2}, {12, 256, 256, 0, -1}, {14, 256, 256, 0, -1},
    {16, 256, 256, 0, -1}, {19, 256, 512, 1, 3}, {21, 512, 512, 0, -1}, {23, 512, 512, 0, -1}, {25, 512, 512, 0, -1}, {28, 512, 512, 1, 4}};
// torchvision vgg16().features up to relu5_3 (the slices of lpips.LPIPS(net='vgg')): every tap is the last conv in front of a pool (or the last conv)
const VggSpec LPIPS_SPEC[VGG_NCONV] = {
    {0, 3, 64, 0, -1}, {2, 64, 64, 0, 0}, {5, 64, 128, 1, -1}, {7, 128, 128, 0, 1}, {10, 128, 256, 1, -1}, {12, 256, 256, 0, -1}, {14, 256, 256, 0, 2},
    {17, 256, 512, 1, -1}, {19, 512, 512, 0, -1}, {21, 512, 512, 0, 3}, {24, 512, 512, 1, -1}, {26, 512, 512, 0, -1}, {28, 512, 512, 0, 4}};
int tap_channels(const VggSpec* VS, int l) {      // channels of feature level l: the width of the conv whose ReLU is tapped
    for (int i = 0; i < VGG_NCONV; i++) if (VS[i].tap == l) return VS[i].cout;
    return 0;
}

// MaxPool2d(2, 2) on dense NHWC maps; odd sizes floor like torch (the last row / column is not covered by any window)
__global__ __launch_bounds__(256) void k_maxpool2(const float* in, float* out, long n_out4, int Hi, int Wi, int C4) {
    const int Ho = Hi >> 1, Wo = Wi >> 1;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n_out4; i += (long)gridDim.x * 256) {
        int c = (int)(i % C4); long q = i / C4; int x = (int)(q % Wo); q /= Wo; int y = (int)(q % Ho); long n = q / Ho;
        const float4* p = reinterpret_cast<const float4*>(in) + ((n * Hi + 2 * y) * (long)Wi + 2 * x) * C4 + c;
        float4 a = p[0], b = p[C4], d = p[(long)Wi * C4], e = p[(long)Wi * C4 + C4];
        float4 m;
        m.x = fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, e.x)); m.y = fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y));
        m.z = fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, e.z)); m.w = fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, e.w));
        reinterpret_cast<float4*>(out)[i] = m;
    }
}
// ---- S16 tensors (common.h): four consecutive channels at flat float index i4 (a multiple of 4) of a DENSE map (ld == C, C a multiple of 32) ----
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 s16_load4_f16(const float* p, long i4) {      // value = hi + lo
    const _Float16* h = reinterpret_cast<const _Float16*>(p + (i4 & ~31L)) + (i4 & 31);
    const f16x4_t hi = *reinterpret_cast<const f16x4_t*>(h), lo = *reinterpret_cast<const f16x4_t*>(h + 32);
    return make_float4((float)hi[0] + (float)lo[0], (float)hi[1] + (float)lo[1], (float)hi[2] + (float)lo[2], (float)hi[3] + (float)lo[3]);
}
__device__ __forceinline__ void s16_store4_bf16(float* p, long i4, float4 v) {      // the split of conv_hx.hip's loaders: hi = bf16(x), lo = bf16(x - hi)
    __bf16* h = reinterpret_cast<__bf16*>(p + (i4 & ~31L)) + (i4 & 31);
    bf16x4_t hi, lo;
    hi[0] = (__bf16)v.x; hi[1] = (__bf16)v.y; hi[2] = (__bf16)v.z; hi[3] = (__bf16)v.w;
    lo[0] = (__bf16)(v.x - (float)hi[0]); lo[1] = (__bf16)(v.y - (float)hi[1]); lo[2] = (__bf16)(v.z - (float)hi[2]); lo[3] = (__bf16)(v.w - (float)hi[3]);
    *reinterpret_cast<bf16x4_t*>(h) = hi;
    *reinterpret_cast<bf16x4_t*>(h + 32) = lo;
}
template <bool S> __device__ __forceinline__ float4 ld4(const float* p, long i) { return S ? s16_load4_f16(p, 4 * i) : reinterpret_cast<const float4*>(p)[i]; }
template <bool S> __device__ __forceinline__ void st4_grad(float* p, long i, float4 v) { if (S) s16_store4_bf16(p, 4 * i, v); else reinterpret_cast<float4*>(p)[i] = v; }

// gradient of [ReLU -> MaxPool2d(2,2)] in one pass: gz[pos] = g_pooled[window] if pos is the window's first maximum (torch's tie rule: strict >,
// scan order (0,0),(0,1),(1,0),(1,1)) and a[pos] > 0, else 0.  Every position of gz is ASSIGNED (no zero-fill needed), including the
// uncovered last row / column of odd-sized maps (zero).
__device__ __forceinline__ void route4(float a0, float a1, float a2, float a3, float g, float& z0, float& z1, float& z2, float& z3) {
    int k = 0; float m = a0;
    if (a1 > m) { m = a1; k = 1; }
    if (a2 > m) { m = a2; k = 2; }
    if (a3 > m) { m = a3; k = 3; }
    const float v = m > 0.f ? g : 0.f;
    z0 = k == 0 ? v : 0.f; z1 = k == 1 ? v : 0.f; z2 = k == 2 ? v : 0.f; z3 = k == 3 ? v : 0.f;
}
// AS: `a` (the forward activation) is an S16-f16 tensor; ZS: gz is written as S16-bf16 (the operand format of the dgrad that consumes it)
template <bool AS, bool ZS>
__global__ __launch_bounds__(256) void k_maxpool2_bwd_relu(const float* a, const float* gp, float* gz, long n_win4, int Hi, int Wi, int C4) {
    const int Ho = Hi >> 1, Wo = Wi >> 1, Hc = (Hi + 1) >> 1, Wc = (Wi + 1) >> 1;      // windows incl. the partial ones of odd sizes
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n_win4; i += (long)gridDim.x * 256) {
        int c = (int)(i % C4); long q = i / C4; int x = (int)(q % Wc); q /= Wc; int y = (int)(q % Hc); long n = q / Hc;
        const long base = ((n * Hi + 2 * y) * (long)Wi + 2 * x) * C4 + c;
        const long o1 = C4, o2 = (long)Wi * C4, o3 = o2 + C4;
        if (y >= Ho || x >= Wo) {      // partial window: no pooled output reads these positions
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            st4_grad<ZS>(gz, base, zero);
            if (2 * x + 1 < Wi) st4_grad<ZS>(gz, base + o1, zero);
            if (2 * y + 1 < Hi) { st4_grad<ZS>(gz, base + o2, zero); if (2 * x + 1 < Wi) st4_grad<ZS>(gz, base + o3, zero); }
            continue;
        }
        const float4 A = ld4<AS>(a, base), B = ld4<AS>(a, base + o1), D = ld4<AS>(a, base + o2), E = ld4<AS>(a, base + o3);
        const float4 G = reinterpret_cast<const float4*>(gp)[((n * Ho + y) * (long)Wo + x) * C4 + c];
        float4 zA, zB, zD, zE;
        route4(A.x, B.x, D.x, E.x, G.x, zA.x, zB.x, zD.x, zE.x);
        route4(A.y, B.y, D.y, E.y, G.y, zA.y, zB.y, zD.y, zE.y);
        route4(A.z, B.z, D.z, E.z, G.z, zA.z, zB.z, zD.z, zE.z);
        route4(A.w, B.w, D.w, E.w, G.w, zA.w, zB.w, zD.w, zE.w);
        st4_grad<ZS>(gz, base, zA); st4_grad<ZS>(gz, base + o1, zB); st4_grad<ZS>(gz, base + o2, zD); st4_grad<ZS>(gz, base + o3, zE);
    }
}
// sum |f_rec - f_gt| over a dense feature map (double atomics per block); optionally the masked L1 seed of the top level:
// gz = seed_w * sign(f_rec - f_gt) where f_rec > 0 (the ReLU that produced f_rec), else 0.  RS / GS: rec / gt are S16-f16 tensors; ZS: gz is written as S16-bf16
template <bool RS, bool GS, bool ZS>
__global__ __launch_bounds__(256) void k_feat_l1(const float* rec, const float* gt, long n4, float seed_w, float* gz, double* acc) {
    __shared__ double sh[4];
    double s = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 r = ld4<RS>(rec, i), g = ld4<GS>(gt, i);
        const float d[4] = {r.x - g.x, r.y - g.y, r.z - g.z, r.w - g.w};
        const float rv[4] = {r.x, r.y, r.z, r.w};
        float z[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            s += (double)fabsf(d[e]);
            z[e] = rv[e] > 0.f ? (d[e] > 0.f ? seed_w : (d[e] < 0.f ? -seed_w : 0.f)) : 0.f;
        }
        if (gz) st4_grad<ZS>(gz, i, make_float4(z[0], z[1], z[2], z[3]));
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(acc, sh[0] + sh[1] + sh[2] + sh[3]);
}
// per IMAGE: acc[n] += sum |f_rec - f_gt| over image n's feature map (blockIdx.y = image); the evaluator's per-position perceptual loss (evaluation/evaluator.py:193)
template <bool RS, bool GS>
__global__ __launch_bounds__(256) void k_feat_l1_img(const float* rec, const float* gt, long n4_img, double* acc) {
    __shared__ double sh[4];
    const float* r4 = rec + 4 * (long)blockIdx.y * n4_img;
    const float* g4 = gt + 4 * (long)blockIdx.y * n4_img;
    double s = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4_img; i += (long)gridDim.x * 256) {
        const float4 r = ld4<RS>(r4, i), g = ld4<GS>(g4, i);
        s += (double)fabsf(r.x - g.x) + (double)fabsf(r.y - g.y) + (double)fabsf(r.z - g.z) + (double)fabsf(r.w - g.w);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(acc + blockIdx.y, sh[0] + sh[1] + sh[2] + sh[3]);
}
// per IMAGE and block: the partials x.y, |x|^2, |y|^2 of image n's feature maps (blockIdx.y = image), written to part[(n * gridDim.x + blockIdx.x) * 3 + {0, 1, 2}] --
// no atomics, a fixed reduction order (the dataset evaluation's VGG cosine similarity, evaluation/metrics/vgg_cosine_similarity.py:47-55; finalised by k_feat_cos_finalize)
template <bool RS, bool GS>
__global__ __launch_bounds__(256) void k_feat_cos_img(const float* x, const float* y, long n4_img, double* part) {
    __shared__ double sh[4][3];
    const float* x4 = x + 4 * (long)blockIdx.y * n4_img;
    const float* y4 = y + 4 * (long)blockIdx.y * n4_img;
    double sxy = 0.0, sxx = 0.0, syy = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4_img; i += (long)gridDim.x * 256) {
        const float4 a = ld4<RS>(x4, i), b = ld4<GS>(y4, i);
        sxy += (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z + (double)a.w * b.w;
        sxx += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
        syy += (double)b.x * b.x + (double)b.y * b.y + (double)b.z * b.z + (double)b.w * b.w;
    }
    for (int o = 32; o > 0; o >>= 1) { sxy += __shfl_xor(sxy, o); sxx += __shfl_xor(sxx, o); syy += __shfl_xor(syy, o); }
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6][0] = sxy; sh[threadIdx.x >> 6][1] = sxx; sh[threadIdx.x >> 6][2] = syy; }
    __syncthreads();
    if (threadIdx.x < 3) part[((long)blockIdx.y * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}
struct CosLevels { long off[5]; int blocks[5]; };      // part region and blocks per image of each feature level
// one thread per image: the blocks of each level in order -> cosine x.y / (max(|x|, 1e-6) max(|y|, 1e-6)) (F.cosine_similarity(dim=1, eps=1e-6)), mean over the 5 levels
__global__ __launch_bounds__(64) void k_feat_cos_finalize(const double* part, CosLevels lv, int nf, double* out) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= nf) return;
    double sim = 0.0;
    for (int l = 0; l < 5; l++) {
        const double* p = part + lv.off[l] + (long)n * lv.blocks[l] * 3;
        double sxy = 0.0, sxx = 0.0, syy = 0.0;
        for (int k = 0; k < lv.blocks[l]; k++) { sxy += p[3 * k]; sxx += p[3 * k + 1]; syy += p[3 * k + 2]; }
        sim += sxy / (fmax(sqrt(sxx), 1e-6) * fmax(sqrt(syy), 1e-6));
    }
    out[n] = sim / 5.0;
}
// frames of the dataset evaluation for VGG19: (N, 3, H, W) -> NHWC (pitch 4) with vgg_cosine_similarity.py:31-37's normalisation (v / range - 0.5) / (0.5 + 1e-6)
__global__ __launch_bounds__(256) void k_metric_stage(const float* src, float* out, long npix, long hw, float range) {
    for (long q = blockIdx.x * 256L + threadIdx.x; q < npix; q += (long)gridDim.x * 256) {
        const long n = q / hw, p = q - n * hw;
        const float* s = src + n * 3 * hw + p;
        const float d = (float)(0.5 + 1e-6);
        reinterpret_cast<float4*>(out)[q] = make_float4((s[0] / range - 0.5f) / d, (s[hw] / range - 0.5f) / d, (s[2 * hw] / range - 0.5f) / d, 0.f);
    }
}
// ground-truth frames for the VGG19 branch: first 3 channels of observation t + t_off, bilinearly resized like F.interpolate(align_corners=False)
// does for exact factors (losses.py:450): f = 2 -> 2x2 mean, f = 4 -> mean of the central 2x2 of each 4x4 block (same arithmetic as k_loss_l1)
__global__ __launch_bounds__(256) void k_gt_resize(TV gt, float* out, int Ho, int Wo, long npix, int f, int t_off, int Tobs, int Trec) {
    for (long q = blockIdx.x * 256L + threadIdx.x; q < npix; q += (long)gridDim.x * 256) {
        const long fr = q / ((long)Ho * Wo); const int rem = (int)(q - fr * Ho * Wo); const int y = rem / Wo, x = rem - y * Wo;
        const long b = fr / Trec, t = fr - b * Trec;
        const float* g = gt.p + (b * Tobs + t + t_off) * gt.sn;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        float* ov = &o.x;
        for (int ch = 0; ch < 3; ch++) {
            if (f == 1) ov[ch] = g[((long)y * gt.W + x) * gt.ld + ch];
            else {
                const int y0 = f == 2 ? 2 * y : 4 * y + 1, x0 = f == 2 ? 2 * x : 4 * x + 1;
                const float* gp = g + ((long)y0 * gt.W + x0) * gt.ld + ch;
                ov[ch] = 0.5f * (0.5f * gp[0] + 0.5f * gp[gt.ld]) + 0.5f * (0.5f * gp[(long)gt.W * gt.ld] + 0.5f * gp[(long)(gt.W + 1) * gt.ld]);
            }
        }
        reinterpret_cast<float4*>(out)[q] = o;
    }
}
// frames of the time steps [t0, t0 + len) of every sample, (B, Tfull) sample-major <-> (B, len) sample-major; F4 = float4 per frame.  add = 0: chunk[q] = full[...] (gather);
// add = 1: full[...] += chunk[q] (the chunk's gradient back onto the seeds; each element has one writer per launch)
__global__ __launch_bounds__(256) void k_time_chunk(float4* full, float4* chunk, long F4, int Tfull, int t0, int len, long total4, int add) {
    for (long q = blockIdx.x * 256L + threadIdx.x; q < total4; q += (long)gridDim.x * 256) {
        const long fr = q / F4, i = q - fr * F4;
        const long b = fr / len, j = fr - b * len;
        const long s = ((b * Tfull + t0 + j) * F4) + i;
        if (add) { float4 a = full[s]; const float4 v = chunk[q]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; full[s] = a; }
        else chunk[q] = full[s];
    }
}
__global__ void k_copy_f(const float* src, float* dst, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = src[i];
}
inline unsigned grid_for(long items) { long b = (items + 255) / 256; return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }

T4 valloc(caddy_ctx* c, int N, int H, int W, int C) {      // bottom-up allocation past the forward graph (released per resolution); gradient at the mirror
    const int ld = round_up(C, 4);
    float* d = (float*)c->act.alloc((size_t)N * H * W * ld * 4);
    return T4{d, (float*)((char*)d + c->grad_delta), N, H, W, C, (long)H * W * ld, ld, true};
}
// format dispatch of the point-wise kernels (S16 flags -> template instances: with_bools, common.h)
void launch_feat_l1(hipStream_t st, const T4& rec, const T4& gt, float seed_w, float* gz, bool gz_s16, double* acc) {
    const long n4 = (long)rec.N * rec.H * rec.W * (rec.C / 4);
    // (dispatched on the NEGATED flags -- "is plain fp32" -- so that the eight instances are emitted all-fp32 first, the order the code object has always had them in)
    with_bools([&](auto RF, auto GF, auto ZF) {
        hipLaunchKernelGGL((k_feat_l1<!decltype(RF)::value, !decltype(GF)::value, !decltype(ZF)::value>), dim3(grid_for(n4)), dim3(256), 0, st, (const float*)rec.d, (const float*)gt.d, n4, seed_w, gz, acc);
    }, !rec.fmt, !gt.fmt, !(gz && gz_s16));
}
int cos_blocks(const T4& f) { const long n4 = (long)f.H * f.W * (f.C / 4); return (int)(n4 / 1024 < 1 ? 1 : (n4 / 1024 > 64 ? 64 : n4 / 1024)); }      // workgroups per image of the per-image kernels
void launch_feat_l1_img(hipStream_t st, const T4& rec, const T4& gt, double* acc) {
    const long n4 = (long)rec.H * rec.W * (rec.C / 4);
    with_bools([&](auto RS, auto GS) {
        hipLaunchKernelGGL((k_feat_l1_img<decltype(RS)::value, decltype(GS)::value>), dim3(cos_blocks(rec), rec.N), dim3(256), 0, st, (const float*)rec.d, (const float*)gt.d, n4, acc);
    }, rec.fmt != 0, gt.fmt != 0);
}
void launch_feat_cos_img(hipStream_t st, const T4& x, const T4& y, double* part) {
    const long n4 = (long)x.H * x.W * (x.C / 4);
    with_bools([&](auto RS, auto GS) {
        hipLaunchKernelGGL((k_feat_cos_img<decltype(RS)::value, decltype(GS)::value>), dim3(cos_blocks(x), x.N), dim3(256), 0, st, (const float*)x.d, (const float*)y.d, n4, part);
    }, x.fmt != 0, y.fmt != 0);
}
void launch_maxpool_bwd(hipStream_t st, const T4& pre, const float* gp, bool gz_s16) {
    const long n4 = (long)pre.N * ((pre.H + 1) / 2) * ((pre.W + 1) / 2) * (pre.C / 4);
    with_bools([&](auto AS, auto ZS) {
        hipLaunchKernelGGL((k_maxpool2_bwd_relu<decltype(AS)::value, decltype(ZS)::value>), dim3(grid_for(n4)), dim3(256), 0, st, (const float*)pre.d, gp, pre.g, n4, pre.H, pre.W, pre.C / 4);
    }, pre.fmt != 0, gz_s16);
}
}  // namespace

const VggSpec* vgg_spec_table(int kind) { return kind == VGG_KIND_LPIPS ? LPIPS_SPEC : VGG19_SPEC; }
static long spec_param_floats(const VggSpec* VS) {
    long n = 0;
    for (int i = 0; i < VGG_NCONV; i++) n += (long)VS[i].cout * VS[i].cin * 9 + round_up(VS[i].cout, 4);
    return n;
}
static int spec_param_info(const VggSpec* VS, int index, caddy_param_info* out) {
    if (index < 0 || index >= 2 * VGG_NCONV) return -1;
    long off = 0;
    for (int i = 0; i < VGG_NCONV; i++) {
        const long nw = (long)VS[i].cout * VS[i].cin * 9;
        if (index == 2 * i || index == 2 * i + 1) {
            memset(out, 0, sizeof(*out));
            const bool w = index == 2 * i;
            snprintf(out->name, sizeof(out->name), "features.%d.%s", VS[i].idx, w ? "weight" : "bias");
            out->offset = w ? off : off + nw; out->kind = 3;
            if (w) { out->ndim = 4; out->shape[0] = VS[i].cout; out->shape[1] = VS[i].cin; out->shape[2] = 3; out->shape[3] = 3; }
            else { out->ndim = 1; out->shape[0] = VS[i].cout; out->shape[1] = out->shape[2] = out->shape[3] = 1; }
            return 0;
        }
        off += nw + round_up(VS[i].cout, 4);
    }
    return -1;
}
int vgg_param_count() { return 2 * VGG_NCONV; }
long vgg_param_floats() { return spec_param_floats(VGG19_SPEC); }
int vgg_param_info(int index, caddy_param_info* out) { return spec_param_info(VGG19_SPEC, index, out); }
// the LPIPS network (evaluation/metrics/lpips.py:14): the 13 convolutions of its VGG16 trunk under torchvision's names, then the five 1x1 "lin" layers (1, C_l, 1, 1)
int lpips_param_count() { return 2 * VGG_NCONV + 5; }
long lpips_param_floats() { long n = spec_param_floats(LPIPS_SPEC); for (int l = 0; l < 5; l++) n += tap_channels(LPIPS_SPEC, l); return n; }
int lpips_param_info(int index, caddy_param_info* out) {
    if (index < 2 * VGG_NCONV) return spec_param_info(LPIPS_SPEC, index, out);
    const int l = index - 2 * VGG_NCONV;
    if (l >= 5) return -1;
    long off = spec_param_floats(LPIPS_SPEC);
    for (int k = 0; k < l; k++) off += tap_channels(LPIPS_SPEC, k);
    memset(out, 0, sizeof(*out));
    snprintf(out->name, sizeof(out->name), "lin%d.model.1.weight", l);
    out->offset = off; out->kind = 3; out->ndim = 4; out->shape[0] = 1; out->shape[1] = tap_channels(LPIPS_SPEC, l); out->shape[2] = out->shape[3] = 1;
    return 0;
}

// persistent packed weights (forward + dgrad form) and biases: carved out of the caller's workspace when caddy_config.perceptual != 0
void vgg_build(caddy_ctx* c, int kind) {
    VggState& V = c->vgg;
    V.enabled = true; V.loaded = false;
    V.kind = kind; V.spec = vgg_spec_table(kind);
    const VggSpec* VS = V.spec;
    for (int i = 0; i < VGG_NCONV; i++) {
        VggLayer& L = V.conv[i];
        PackDesc& d = L.pd;
        d = PackDesc{};
        d.nw = 1; d.Co_each = VS[i].cout; d.Cin = VS[i].cin; d.KS = 3; d.nseg = 1;
        d.seg_off[0] = 0; d.seg_C[0] = VS[i].cin; d.seg_Cpad[0] = round_up(VS[i].cin, CONV_BK);
        d.Cout = VS[i].cout; d.Cout_pad = round_up(d.Cout, conv_pick_bn(d.Cout)); d.Ktot = d.seg_Cpad[0];
        L.wp = (float*)c->persist.alloc((size_t)9 * d.Cout_pad * d.Ktot * 4);
        L.kd = round_up(d.Cout, CONV_BK);
        L.cd_pad = round_up(VS[i].cin, conv_pick_bn(VS[i].cin));
        L.wpd = (float*)c->persist.alloc((size_t)9 * L.cd_pad * L.kd * 4);
        L.bias = (float*)c->persist.alloc((size_t)round_up(d.Cout, 4) * 4);
        for (int pl = 0; pl < 2; pl++) {
            L.wq[pl] = c->persist.alloc(hx_weight_bytes(d, -1, round_up(d.Cout, hx_pick_bn(d.Cout)), 2 - pl));
            L.wqd[pl] = VS[i].cin >= 32 ? c->persist.alloc(hx_weight_bytes(d, 0, round_up(VS[i].cin, hx_pick_bn(VS[i].cin)), 2 - pl)) : nullptr;
        }
        L.wq[2] = c->persist.alloc(hx_weight_bytes(d, -1, round_up(d.Cout, hx_pick_bn(d.Cout)), 2));
    }
    if (kind == VGG_KIND_LPIPS) for (int l = 0; l < 5; l++) V.lin[l] = (float*)c->persist.alloc((size_t)tap_channels(VS, l) * 4);
}

// caddy_load_vgg: `flat` = device buffer laid out per vgg_param_info (torchvision names features.{idx}.weight / .bias, OIHW fp32)
int vgg_load(caddy_ctx* c, const float* flat) {
    VggState& V = c->vgg;
    if (!V.enabled) { set_error("caddy_load_vgg: the context was created with caddy_config.perceptual = 0"); return -2; }
    bool dry = c->dry;
    const VggSpec* VS = V.spec;
    long off = 0;
    for (int i = 0; i < VGG_NCONV; i++) {
        VggLayer& L = V.conv[i];
        const long nw = (long)VS[i].cout * VS[i].cin * 9;
        L.pd.w[0] = flat + off;
        RUN_CK(c, pack_fwd(L.pd, L.wp, c->stream));
        RUN_CK(c, pack_dgrad(L.pd, 0, L.wpd, L.cd_pad, L.kd, c->stream));
        for (int pl = 0; pl < 2; pl++) {
            RUN_CK(c, pack_hx(L.pd, L.wq[pl], round_up(L.pd.Cout, hx_pick_bn(L.pd.Cout)), -1, pl == 0 ? PREC_F16X3 : PREC_F16X1, c->stream));
            if (L.wqd[pl]) RUN_CK(c, pack_hx(L.pd, L.wqd[pl], round_up(VS[i].cin, hx_pick_bn(VS[i].cin)), 0, pl == 0 ? PREC_BF16X3 : PREC_BF16X1, c->stream));
        }
        RUN_CK(c, pack_hx(L.pd, L.wq[2], round_up(L.pd.Cout, hx_pick_bn(L.pd.Cout)), -1, PREC_BF16X3, c->stream));
        if (!dry) hipLaunchKernelGGL(k_copy_f, dim3(1), dim3(256), 0, c->stream, flat + off + nw, L.bias, (long)VS[i].cout);
        L.pd.w[0] = nullptr;      // the caller's buffer is not referenced after this call
        off += nw + round_up(VS[i].cout, 4);
    }
    if (V.kind == VGG_KIND_LPIPS) for (int l = 0; l < 5; l++) {
        if (!dry) hipLaunchKernelGGL(k_copy_f, dim3(1), dim3(256), 0, c->stream, flat + off, V.lin[l], (long)tap_channels(VS, l));
        off += tap_channels(VS, l);
    }
    V.loaded = true;
    return c->fail ? -1 : 0;
}

namespace {
struct Branch { T4 a[VGG_NCONV]; T4 p[VGG_NCONV]; };      // a walk that is back-propagated: a[i] ReLU output of conv i; p[i] pooled input of conv i (pool_before)

int conv_call(caddy_ctx* c, const ConvArgs& a, double flops, int kind) {
    Scoped<int> prof_kind(c->prof_kind_override, kind);
    return c->timed_conv_fwd(a, flops);
}
// the five tapped maps of an N x H x W batch (MaxPool2d floors odd sizes); with `b` a second pyramid, allocated level by level behind the first (a[l], b[l], a[l + 1], ...)
void tap_alloc(caddy_ctx* c, int N, int H, int W, T4* a, T4* b = nullptr) {
    for (int l = 0; l < 5; l++, H /= 2, W /= 2) {
        const int C = tap_channels(c->vgg.spec, l);
        a[l] = valloc(c, N, H, W, C);
        if (b) b[l] = valloc(c, N, H, W, C);
    }
}
// does the context keep VGG19 feature maps / feature gradients of well-filled layers as S16 tensors?  (both passes on the split-operand kernels: an exact-fp32 pass would have to
// read them)
bool vgg_use_s16(const caddy_ctx* c) { return c->vgg_s16 && c->vgg_precision == PREC_F16X3 && c->vgg_precision_bwd == PREC_BF16X3; }
// is conv i's launch on an N x H x W input one of the k_conv_hx variants that read / write S16 tensors?
bool vgg_io_ok(const caddy_ctx* c, int i, int N, int H, int W) {
    const VggSpec* VS = c->vgg.spec;
    return vgg_use_s16(c) && VS[i].cin >= 32 && !c->layer_fallback[CADDY_VGG_FLAG0 + i] && conv_hx_s16_ok(N, H, W, VS[i].cout);      // (a layer on the split-bf16 fallback exchanges fp32 tensors)
}

// 13 x (conv3x3 + bias + ReLU) with the 2x2 max-pools; taps[] (if given) receive the five tapped feature maps in place, and the format each was written in (T4::fmt).
// keep (the branch that is back-propagated): every full-resolution map is stored, and every map and pooled input is recorded in *keep.
// Formats (round 5): a feature map is written PRE-SPLIT (S16-f16, T4::fmt) by the epilogue of its producer when that launch and the launch of the convolution that consumes it
// are both on the S16-capable tile variants (conv_hx_s16_ok: the well-filled ones) -- the consumer then copies operand rows instead of converting every halo element in every
// one of its output-channel blocks; the point-wise consumers (feature L1, max-pool backward, ReLU masks) read either format.
void vgg_forward(caddy_ctx* c, const T4& img, T4* taps, Branch* keep = nullptr) {
    bool dry = c->dry;
    VggState& V = c->vgg;
    const VggSpec* VS = V.spec;
    T4 x = img;
    T4 pooled{};                                              // output of a max-pool fused into the previous conv's epilogue
    bool have_pooled = false;
    for (int i = 0; i < VGG_NCONV; i++) {
        VggLayer& L = V.conv[i];
        if (VS[i].pool_before) {
            if (have_pooled) { x = pooled; have_pooled = false; }
            else {
                T4 p = valloc(c, x.N, x.H / 2, x.W / 2, x.C);
                const long n4 = (long)p.N * p.H * p.W * (p.C / 4);
                if (x.fmt) { c->fail = true; set_error("internal: S16 feature map handed to the stand-alone max-pool"); }
                if (!dry) hipLaunchKernelGGL(k_maxpool2, dim3(grid_for(n4)), dim3(256), 0, c->stream, (const float*)x.d, p.d, n4, x.H, x.W, p.C / 4);
                x = p;
            }
            if (keep) keep->p[i] = x;
        }
        T4 out = (taps && VS[i].tap >= 0) ? taps[VS[i].tap] : valloc(c, x.N, x.H, x.W, VS[i].cout);
        out.fmt = 0;
        ConvArgs a{};
        a.src[0] = ConvSrc{x.d, x.sn, x.ld, x.C, round_up(x.C, CONV_BK), 0};
        a.nsrc = 1; a.N = x.N; a.H = x.H; a.W = x.W; a.KS = 3; a.wp = L.wp; a.Ktot = L.pd.Ktot; a.Cout = L.pd.Cout; a.Cout_pad = L.pd.Cout_pad;
        a.bias = L.bias; a.act = 2; a.out = out.d; a.out_sn = out.sn; a.out_ld = out.ld;
        a.beside_chain = c->vgg_beside;
        a.precision = c->vgg_precision == PREC_F16X1 ? PREC_F16X1 : (c->vgg_precision == PREC_FP32 ? PREC_FP32 : (c->vgg_precision == PREC_BF16X3 ? PREC_BF16X3 : PREC_F16X3));
        // f16 range guard: real VGG19 weights on un-normalised inputs are where a forward activation could leave the f16 range.  A layer that reported it (caddy_f16_saturated) runs
        // on split bf16 from then on -- 8 + 8 mantissa bits, the full fp32 exponent range -- and only that layer (round 4 moved the whole context to exact fp32: 2.2 x slower)
        if (a.precision == PREC_F16X3 && c->layer_fallback[CADDY_VGG_FLAG0 + i]) a.precision = PREC_BF16X3;
        if (a.precision != PREC_FP32) a.wq = L.wq[a.precision == PREC_F16X1 ? 1 : (a.precision == PREC_BF16X3 ? 2 : 0)];
        a.sat_flag = c->sat_flag + CADDY_VGG_FLAG0 + i;
        const bool io_here = vgg_io_ok(c, i, x.N, x.H, x.W);
        const bool pool_next = i + 1 < VGG_NCONV && VS[i + 1].pool_before;
        a.in_s16 = x.fmt;
        if (x.fmt && !io_here) { c->fail = true; set_error("internal: S16 input for a VGG19 launch that cannot read it"); }
        // MaxPool2d(2, 2) in front of the next conv: written by THIS conv's epilogue on the split-operand kernel (the window's four pixels sit in
        // one lane) -- no separate pass over the full-resolution map; a branch that is never back-propagated (no `keep`: the ground truth)
        // does not even store the full-resolution map of such a layer unless it is a tap (VGG19: never, its taps are the first convs AFTER a pool; the VGG16 trunk of LPIPS: always)
        if (pool_next && a.wq && a.precision == PREC_F16X3 && VS[i].cin >= 32 && conv_hx_pool_ok(x.N, x.H, x.W, VS[i].cout)) {
            pooled = valloc(c, x.N, x.H / 2, x.W / 2, VS[i].cout);
            a.pool_out = pooled.d; a.pool_sn = pooled.sn; a.pool_ld = pooled.ld;
            a.skip_out = (!keep && VS[i].tap < 0) ? 1 : 0;
            have_pooled = true;
            // the pooled map as S16 when its consumer (conv i + 1 on the pooled geometry) reads S16; the full-resolution map (read by the max-pool backward only) in the same format
            if (io_here && vgg_io_ok(c, i + 1, x.N, x.H / 2, x.W / 2)) { a.pool_s16 = 1; pooled.fmt = 1; if (!a.skip_out) { a.out_s16 = 1; out.fmt = 1; } }
        } else if (io_here && !pool_next) {
            // consumed by conv i + 1 on the same geometry (or, for relu5_1, by the feature L1 alone)
            if (i + 1 == VGG_NCONV || vgg_io_ok(c, i + 1, x.N, x.H, x.W)) { a.out_s16 = 1; out.fmt = 1; }
        }
        a.sat_out_next = ((a.out_s16 || a.pool_s16) && i + 1 < VGG_NCONV) ? 1 : 0;      // a clamped OUTPUT value is the next layer's range problem (flag words are consecutive per layer)
        if (!dry) c->ck(conv_call(c, a, 2.0 * x.N * x.H * x.W * 9.0 * VS[i].cin * VS[i].cout, 3), "vgg conv");
        if (taps && VS[i].tap >= 0) taps[VS[i].tap].fmt = out.fmt;      // (a tapped map may be an S16 tensor)
        if (keep) keep->a[i] = out;
        x = out;
    }
}
}  // namespace

// Ground-truth branch ahead of time: called from the forward pass right after the observations are in NHWC, it runs the resize + the 13
// convolutions of the ground-truth frames at the three resolutions on the driver's SIDE stream, concurrently with the model's forward pass
// (whose recurrent convolutions on 16x16 / 32x32 maps leave most of the chip idle).  The five tapped maps per resolution stay in the
// activation arena until caddy_loss_backward; the other feature maps go through one scratch region reused by the three resolutions.
void vgg_gt_prefetch(caddy_ctx* c, int Trec, int t_off) {
    const caddy_config& g = c->cfg;
    // chunk table of this forward pass (caddy_ctx::perc_plan): the taps are laid out per chunk, whatever the loss call then does with them.  Pretraining (no BPTT chain to run
    // beside) and evaluation passes keep one chunk.
    c->perc_plan(Trec, c->training && !c->pretraining);
    c->gt_lo = (c->act.off + 255) & ~(size_t)255;
    T4 gimg[caddy_ctx::PERC_MAX_CHUNKS][3];
    // (caddy_ctx::perc_range: the full-resolution level follows the chunk table, the half- and quarter-resolution levels are cut once)
    c->perc_for_each([&](int k, int r, int, int len) {
        gimg[k][r] = valloc(c, g.batch * len, g.height >> r, g.width >> r, 3);                 // (ld 4)
        tap_alloc(c, g.batch * len, g.height >> r, g.width >> r, c->gt_taps_c[k][r]);
    });
    for (int r = 0; r < 3; r++) c->gt_img[r] = gimg[0][r];
    {   // scratch for the non-tapped maps: the largest walk of vgg_forward over EVERY (chunk, level) the side stream will run -- with many short chunks the half of a smaller
        // level that goes with chunk nch / 2 can need more than the longest full-resolution chunk and than the half that goes with chunk 0
        const size_t m0 = c->act.off;
        size_t end = m0;
        Scoped<bool> sizing(c->dry, true);
        c->perc_for_each([&](int k, int r, int, int) {
            c->act.off = m0;
            vgg_forward(c, gimg[k][r], c->gt_taps_c[k][r]);
            if (c->act.off > end) end = c->act.off;
        });
        // keep the region allocated (the main stream goes on allocating past it: act.off is NOT put back); the side stream re-walks it for every chunk and resolution
        c->act.off = end;
        c->gt_scratch_off = m0; c->gt_scratch_end = end;
    }
    c->gt_hi = c->act.off;
    c->gt_prefetched = false;
    if (c->dry || !c->vgg.loaded || !c->perc_prefetch || !c->training) return;
    c->ensure_side();
    if (!c->use_side || !c->side) return;
    const hipStream_t side = c->wgrad_stream();             // ordered after everything enqueued so far (the NHWC observations)
    {
        Scoped<hipStream_t> on_side(c->stream, side);
        Scoped<int> beside(c->vgg_beside, 1);                // (the model's forward pass runs on the main stream meanwhile)
        c->perc_for_each([&](int k, int r, int t0, int len) {      // (the order the loss call consumes them in: last time steps first)
            const T4& gi = gimg[k][r];
            const long npix = (long)gi.N * gi.H * gi.W;
            hipLaunchKernelGGL(k_gt_resize, dim3(grid_for(npix)), dim3(256), 0, side, dv(c->obs), gi.d, gi.H, gi.W, npix, 1 << r, t_off + t0, g.seq_len, len);
            ArenaMark keep(c->act);
            c->act.off = c->gt_scratch_off;                    // (host-side bump pointer only: the region is private to the side stream)
            vgg_forward(c, gi, c->gt_taps_c[k][r]);
            if (c->act.off > c->gt_scratch_end) { c->fail = true; set_error("internal: a ground-truth VGG19 walk passes the side stream's scratch region"); }
        });
    }
    hipEventRecord(c->gt_done, side);
    c->gt_prefetched = true;
}

int caddy_debug_gt_scratch_check(caddy_ctx* c, int trec, long* out) {
    if (!c->cfg.perceptual) { set_error("caddy_debug_gt_scratch_check needs a context created with caddy_config.perceptual = 1"); return -2; }
    // a sizing pass in training mode; put back at exit in reverse order of declaration: act.off, act.high (a probe must not raise the high-water mark either), dry, training, pretraining
    Scoped<bool> pre(c->pretraining, false), training(c->training, true), sizing(c->dry, true);
    Scoped<size_t> high(c->act.high);
    ArenaMark keep(c->act);
    vgg_gt_prefetch(c, trec, 1);
    size_t need = 0;
    c->perc_for_each([&](int k, int r, int, int) {
        const T4& t = c->gt_taps_c[k][r][0];
        const T4 gi = valloc(c, t.N, t.H, t.W, 3);
        c->act.off = c->gt_scratch_off;
        vgg_forward(c, gi, c->gt_taps_c[k][r]);
        if (c->act.off - c->gt_scratch_off > need) need = c->act.off - c->gt_scratch_off;
    });
    out[0] = (long)(c->gt_scratch_end - c->gt_scratch_off); out[1] = (long)need; out[2] = c->perc_nch;
    return 0;
}

// Called from loss_backward after the L1 terms (which also wrote the resized ground-truth images gt_img[r]) and before the tape is replayed:
// accumulates d(perceptual term)/d(rec_r) into the gradients of c->frames[r] and the raw level sums into c->loss_acc.
// Round 6: chunk by chunk of time steps (caddy_ctx::perc_t0, last steps first).  One chunk: the form of rounds 2 - 5 (the half- and quarter-resolution levels on the side stream
// beside the full-resolution one, the dgrad of conv1_1 accumulating straight onto the L1 seeds).  Several chunks: a chunk's frames are gathered into a contiguous batch
// (k_time_chunk), its gradient is assigned to the gathered copy and added onto the seeds of its time steps; with caddy_ctx::perc_pipelined ALL of it runs on the side stream and
// an event per chunk tells the tape replay which time steps may start (perc_wait).
void vgg_perceptual(caddy_ctx* c, double lambda, const T4* gt_img, VggLevels* lv) {
    bool dry = c->dry;
    VggState& V = c->vgg;
    const VggSpec* VS = V.spec;
    hipStream_t st = c->stream;
    const caddy_config& g = c->cfg;
    const bool pre = c->gt_prefetched && !dry;      // the ground-truth branch already ran beside the forward pass (vgg_gt_prefetch)
    const int nch = c->perc_nch, Trec = c->perc_trec, B = g.batch;
    const bool pipe = c->perc_pipelined && nch > 1 && !dry;
    // The half- and quarter-resolution levels (24 % of the work, most of it in under-filled launches on 8x8 ... 64x64 maps) run on the driver's side
    // stream BESIDE the full-resolution level (one-chunk form): separate memory (they are allocated first and stay live until the join), their own thin-kernel
    // scratch, the three levels only meet in the loss accumulators (atomics) and write disjoint gradient tensors (d rec_r).
    const bool no_par = caddy_serial_streams();
    const bool par = nch == 1 && !no_par && !dry && c->use_side && c->side != nullptr && !c->prof;
    hipStream_t side = (par || pipe) ? c->wgrad_stream() : st;      // (ordered after the L1 kernels that wrote the seeds / resized ground truth)
    if (pre) { hipStreamWaitEvent(st, c->gt_done, 0); if (pipe) hipStreamWaitEvent(side, c->gt_done, 0); }
    // put back at exit, in this order: vgg_beside (0 between the driver's entry points), the stream, the arena (everything below is released)
    ArenaMark all(c->act);
    Scoped<hipStream_t> stream_guard(c->stream);
    Scoped<int> beside(c->vgg_beside);
    const size_t mark_all = all.old;
    size_t side_end = mark_all;                             // memory layout is the parallel one whether or not the levels really overlap (dry-run sizing)
    // Pipelined form: nothing runs beside the FIRST chunk (the tape replay waits for it), so that chunk keeps the level parallelism of the one-pass form -- its full-resolution
    // level on the main stream (in front of the replay's launches), its half- and quarter-resolution levels on the side stream; the later chunks run on the side stream alone,
    // beside the replay.  Memory: [mark_all, main_end) the first chunk's full-resolution level, everything the side stream touches above it.
    size_t side_base = mark_all;
    for (int k = 0; k < nch; k++) {
    const bool first_par = nch > 1 && k == 0 && (pipe || dry);      // (dry run: the same layout)
    c->vgg_beside = (pipe && k >= 1) ? 2 : 0;                // the tape replay runs beside every chunk but the first (incl. the early halves of the smaller levels)
    for (int oi = 0; oi < 3; oi++) {
        const int r = first_par ? oi : (oi == 2 ? 0 : oi + 1);      // levels 1, 2, 0 -- the first chunk of the pipelined form 0 (main stream), 1, 2
        int t0, len;
        if (!c->perc_range(r, k, &t0, &len)) continue;      // (the half- and quarter-resolution levels are cut once: caddy_ctx::perc_range)
        const bool whole = len == Trec;                     // this level's batch is the frame tensor itself
        const bool on_side = (pipe && !(first_par && r == 0)) || (par && r != 0);
        c->stream = on_side ? side : st;
        hipStream_t st = c->stream;                         // (shadows the outer one for the point-wise launches below)
        float* const aux = on_side ? c->conv_aux2 : c->conv_aux;
        if (nch > 1) c->act.off = (first_par && r == 0) ? mark_all : side_base;      // chunks and levels that follow each other on one stream share their region
        else if (r == 0 && !no_par) c->act.off = side_end;      // above everything levels 1 / 2 may still be using
        const T4& full = c->frames[r];
        const size_t mark = c->act.off;
        const long F4 = (long)full.H * full.W * (full.ld / 4);
        // this chunk's reconstructed frames: the tensor itself (one chunk) or a gathered copy
        T4 rec = full;
        if (!whole) {
            rec = valloc(c, B * len, full.H, full.W, 3);
            if (full.ld != 4 || full.sn != F4 * 4) { c->fail = true; set_error("internal: frame tensor layout of the chunked perceptual pass"); }
            if (!dry) hipLaunchKernelGGL(k_time_chunk, dim3(grid_for((long)rec.N * F4)), dim3(256), 0, st, (float4*)full.d, (float4*)rec.d, F4, Trec, t0, len, (long)rec.N * F4, 0);
        }
        // ground-truth branch: keeps only the five tapped maps
        T4 taps[5];
        Branch R{};
        if (pre) { for (int l = 0; l < 5; l++) taps[l] = c->gt_taps_c[k][r][l]; }
        else {
            tap_alloc(c, rec.N, rec.H, rec.W, taps);
            T4 gi = gt_img[r];
            if (!whole) {
                gi = valloc(c, rec.N, rec.H, rec.W, 3);
                if (!dry) hipLaunchKernelGGL(k_time_chunk, dim3(grid_for((long)rec.N * F4)), dim3(256), 0, st, (float4*)gt_img[r].d, (float4*)gi.d, F4, Trec, t0, len, (long)rec.N * F4, 0);
            }
            ArenaMark gt_walk(c->act);           // stream order: the temporaries of the ground-truth branch are dead before anything below overwrites them
            vgg_forward(c, gi, taps);
        }
        vgg_forward(c, rec, nullptr, &R);
        auto input_of = [&](int i) -> const T4& { return VS[i].pool_before ? R.p[i] : (i > 0 ? R.a[i - 1] : rec); };      // what conv i read
        // per-level sums and weights.  w_l = lambda * (l == 0 ? 1 : 2) / 3 / numel_l   (aliasing of level 0 with the total, see the header); numel_l counts ALL B x Trec frames
        float wl[5];
        int li[5];
        for (int i = 0; i < VGG_NCONV; i++) if (VS[i].tap >= 0) li[VS[i].tap] = i;
        // formats of the feature gradients gz_i = d/d(pre-ReLU output of conv i), stored at the gradient mirror of a[i]: S16-bf16 when the dgrad of conv i that consumes it runs on an
        // S16-capable launch AND its producer can write it -- the point-wise producers (feature L1 seed of relu5_1, max-pool backward) always can, the dgrad of conv i + 1 when it is
        // such a launch itself
        bool io_d[VGG_NCONV], gzs[VGG_NCONV];
        for (int i = 0; i < VGG_NCONV; i++) {
            const T4& in = input_of(i);
            io_d[i] = vgg_use_s16(c) && i > 0 && V.conv[i].wqd[0] != nullptr && conv_hx_s16_ok(in.N, in.H, in.W, VS[i].cin);
        }
        for (int i = 0; i < VGG_NCONV; i++) gzs[i] = io_d[i] && (i + 1 == VGG_NCONV || VS[i + 1].pool_before || io_d[i + 1]);
        for (int l = 0; l < 5; l++) {
            const T4& f = R.a[li[l]];
            const double numel = (double)B * Trec * f.H * f.W * f.C;
            lv->numel[r][l] = numel;
            wl[l] = (float)(lambda * (l == 0 ? 1.0 : 2.0) / 3.0 / numel);
        }
        // the dgrad launch of conv i (backward of the reconstruction branch)
        auto dgrad_args = [&](int i) {
                VggLayer& L = V.conv[i];
                const T4& gz = R.a[i];
                const T4& in = input_of(i);
                ConvArgs d{};
                d.src[0] = ConvSrc{gz.g, gz.sn, gz.ld, L.pd.Cout, L.kd, 0};
                d.nsrc = 1; d.N = in.N; d.H = in.H; d.W = in.W; d.KS = 3; d.wp = L.wpd; d.Ktot = L.kd;
                d.Cout = VS[i].cin; d.Cout_pad = L.cd_pad; d.bias = nullptr; d.act = 0; d.aux = aux;
                d.precision = c->vgg_precision_bwd == PREC_BF16X1 ? PREC_BF16X1 : (c->vgg_precision_bwd == PREC_FP32 ? PREC_FP32 : PREC_BF16X3);
                if (d.precision != PREC_FP32 && L.wqd[0]) d.wq = L.wqd[d.precision == PREC_BF16X1 ? 1 : 0];
                d.out = in.g; d.out_sn = in.sn; d.out_ld = in.ld;
                d.in_s16 = gzs[i] ? 1 : 0;
                d.beside_chain = c->vgg_beside;
                if (i == 0) d.accumulate = whole ? 1 : 0;                     // whole batch: += into d(rec_r), next to the L1 seed; a chunk: assigned to the gathered copy, added below
                else if (!VS[i].pool_before) {                               // direct input a[i-1]: ReLU mask (+ L1 seed when a[i-1] is tapped) in the epilogue; the output IS gz_{i-1}
                    d.mask = in.d; d.mask_s16 = in.fmt;
                    if (VS[i - 1].tap >= 0) { const T4& tp = taps[VS[i - 1].tap]; d.seed_ref = tp.d; d.seed_w = wl[VS[i - 1].tap]; d.seed_s16 = tp.fmt; }
                    d.out_s16 = gzs[i - 1] ? 1 : 0;
                }
                return d;
        };
        // Level sums.  relu1_1 .. relu4_1: the dgrad of the layer above the tap loads both maps for the sign of the L1 seed -- where that launch runs on a kernel that also sums
        // |f_rec - f_gt| (conv_hx_l1_ok) it is handed the level's accumulator and the stand-alone pass over the two maps is skipped (caddy_ctx::perc_fuse_l1).  relu5_1 keeps
        // k_feat_l1 (it writes the top seed), and so does every level when nothing is back-propagated.
        bool l1_fused[5] = {false, false, false, false, false};
        for (int l = 0; l < 5; l++) {
            const T4& f = R.a[li[l]];
            double* const lacc = c->loss_acc + LOSS_PERC_R0 + 6 * r + 1 + l;
            if (l < 4 && lambda != 0.0 && c->perc_fuse_l1 && li[l] + 1 < VGG_NCONV && !VS[li[l] + 1].pool_before) {
                const ConvArgs d = dgrad_args(li[l] + 1);
                l1_fused[l] = d.seed_ref != nullptr && conv_hx_l1_ok(d);
            }
            if (!dry && !l1_fused[l]) launch_feat_l1(st, f, taps[l], wl[l], l == 4 ? f.g : (float*)nullptr, gzs[li[4]], lacc);
        }
        if (lambda != 0.0) {
            // backward of the reconstruction branch
            for (int i = VGG_NCONV - 1; i >= 0; i--) {
                const T4& in = input_of(i);
                ConvArgs d = dgrad_args(i);
                if (i > 0 && VS[i - 1].tap >= 0 && l1_fused[VS[i - 1].tap]) d.l1_acc = c->loss_acc + LOSS_PERC_R0 + 6 * r + 1 + VS[i - 1].tap;
                if (!dry) c->ck(conv_call(c, d, 2.0 * in.N * in.H * in.W * 9.0 * VS[i].cin * VS[i].cout, 4), "vgg dgrad");
                if (VS[i].pool_before) {                                     // pooled input: route through the max-pool and the ReLU of a[i-1] (fp32 gradient of the pooled map -> gz_{i-1})
                    if (!dry) launch_maxpool_bwd(st, R.a[i - 1], (const float*)in.g, gzs[i - 1]);
                }
            }
            if (!whole && !dry)      // the chunk's d(rec_r) onto the seeds of its time steps
                hipLaunchKernelGGL(k_time_chunk, dim3(grid_for((long)rec.N * F4)), dim3(256), 0, st, (float4*)full.g, (float4*)rec.g, F4, Trec, t0, len, (long)rec.N * F4, 1);
        }
        if (r != 0 && c->act.off > side_end) side_end = c->act.off;
        if (nch == 1) c->act.off = mark;                    // levels 1 and 2 share memory (same stream, in order)
        if (first_par && r == 0) side_base = c->act.off;
    }
    if (pipe) hipEventRecord(c->perc_ev[k], side);          // the seeds of the time steps [t0, t0 + len) are final (first chunk: its full-resolution level is ordered by the main stream itself)
    }
    if (par) {                                               // join: the tape replay reads d(rec_1), d(rec_2)
        hipEvent_t e = c->sev();
        hipEventRecord(e, side);
        hipStreamWaitEvent(st, e, 0);
    }
}

namespace {
// The walk the three evaluation passes share: the tap pyramids of two staged image batches, interleaved level by level with ta[l] in front of tb[l]; what reserve() allocates
// behind them (the head's partial sums); the trunk on `ia`, then on `ib` through the same temporaries.  The caller holds the ArenaMark that releases all of it.
template <class Reserve> int paired_walk(caddy_ctx* c, const T4& ia, const T4& ib, T4* ta, T4* tb, const char* overflow_msg, Reserve&& reserve) {
    tap_alloc(c, ia.N, ia.H, ia.W, ta, tb);
    reserve();
    { ArenaMark first(c->act); vgg_forward(c, ia, ta); }
    vgg_forward(c, ib, tb);
    if (c->act.overflow()) { set_error(overflow_msg); return -1; }
    return 0;
}
}  // namespace

// Evaluation: the full-resolution perceptual distance PER RECONSTRUCTED FRAME and feature level -- out_host[l * N + n] = mean |f_l(rec_n) - f_l(gt_n)|, n = b * Trec + t --
// after a forward pass (any mode).  The reference evaluator applies ParallelPerceptualLoss to one sequence position at a time (evaluation/evaluator.py:55,62,193-197,
// training/losses.py:652-713): position t's value is sum_l mean_b out[l][b, t].  Same VGG19 kernels as the training loss; nothing is back-propagated.
int vgg_eval_per_frame(caddy_ctx* c, double* out_host) {
    const caddy_config& g = c->cfg;
    if (!g.perceptual || !c->vgg.loaded) { set_error("caddy_perceptual_per_frame needs a context created with caddy_config.perceptual = 1 and loaded VGG19 weights"); return -2; }
    if (!c->have_forward) { set_error("caddy_perceptual_per_frame: no forward results available"); return -2; }
    const int Trec = c->pretraining ? g.seq_len : g.seq_len - 1, t_off = c->pretraining ? 0 : 1;
    const T4& rec = c->frames[0];
    const int N = rec.N;
    hipStream_t st = c->stream;
    if (c->gt_prefetched) hipStreamWaitEvent(st, c->gt_done, 0);      // (a training-mode forward started the ground-truth branch on the side stream: its scratch lies below fwd_off, untouched here)
    c->act.off = c->fwd_off;
    ArenaMark mark(c->act);                                           // (leaves the arena at fwd_off, wherever it stood at entry)
    T4 gi = valloc(c, N, g.height, g.width, 3);
    const long npix = (long)N * g.height * g.width;
    hipLaunchKernelGGL(k_gt_resize, dim3(grid_for(npix)), dim3(256), 0, st, dv(c->obs), gi.d, g.height, g.width, npix, 1, t_off, g.seq_len, Trec);
    T4 tg[5], tr[5];
    double* acc = nullptr;
    if (paired_walk(c, gi, rec, tg, tr, "caddy_perceptual_per_frame: workspace too small", [&] {
            acc = c->dalloc(5 * (size_t)N);
            hipMemsetAsync(acc, 0, sizeof(double) * 5 * (size_t)N, st);
        })) return -1;
    for (int l = 0; l < 5; l++) launch_feat_l1_img(st, tr[l], tg[l], acc + (size_t)l * N);
    hipMemcpyAsync(out_host, acc, sizeof(double) * 5 * (size_t)N, hipMemcpyDeviceToHost, st);
    hipStreamSynchronize(st);
    for (int l = 0; l < 5; l++) { const double numel = (double)tr[l].H * tr[l].W * tr[l].C; for (int n = 0; n < N; n++) out_host[(size_t)l * N + n] /= numel; }
    return c->fail ? -1 : 0;
}

// Dataset evaluation (evaluation/metrics/vgg_cosine_similarity.py:22-57, on a metrics context: caddy_metrics_ctx_create): the VGG19 cosine similarity of frames [0, nf) of
// `ref` / `gen` ((nf, 3, H, W) fp32), out[n] = mean over relu1_1 .. relu5_1 of cos(f_l(ref_n), f_l(gen_n)).  With c->dry nothing is launched (workspace sizing).
int vgg_metric_chunk(caddy_ctx* c, const float* ref, const float* gen, int nf, float range, double* out) {
    const bool dry = c->dry;
    const int H = c->cfg.height, W = c->cfg.width;
    hipStream_t st = c->stream;
    ArenaMark mark(c->act);
    T4 gr = valloc(c, nf, H, W, 3), gg = valloc(c, nf, H, W, 3);
    const long npix = (long)nf * H * W;
    if (!dry) {
        hipLaunchKernelGGL(k_metric_stage, dim3(grid_for(npix)), dim3(256), 0, st, ref, gr.d, npix, (long)H * W, range);
        hipLaunchKernelGGL(k_metric_stage, dim3(grid_for(npix)), dim3(256), 0, st, gen, gg.d, npix, (long)H * W, range);
    }
    T4 tr[5], tg[5];
    CosLevels lv{};
    double* part = nullptr;
    if (paired_walk(c, gr, gg, tr, tg, "caddy_frame_metrics: workspace too small", [&] {
            long total = 0;
            for (int l = 0; l < 5; l++) { lv.off[l] = total; lv.blocks[l] = cos_blocks(tr[l]); total += (long)nf * lv.blocks[l] * 3; }
            part = c->dalloc((size_t)total);
        })) return -1;
    if (!dry) {
        for (int l = 0; l < 5; l++) launch_feat_cos_img(st, tr[l], tg[l], part + lv.off[l]);
        hipLaunchKernelGGL(k_feat_cos_finalize, dim3((nf + 63) / 64), dim3(64), 0, st, (const double*)part, lv, nf, out);
    }
    return c->fail ? -1 : 0;
}

// Dataset evaluation (evaluation/metrics/lpips.py:14,33: lpips.LPIPS(net='vgg') per observation, on a context from caddy_lpips_ctx_create): LPIPS of frames [0, nf) of `ref` / `gen`
// ((nf, 3, H, W) fp32 in [0, range]).  out[0 * ldo + n] = the distance, out[(1 + l) * ldo + n] = its level-l term.  The walk of vgg_metric_chunk with the VGG16 trunk; the head is
// lpips.hip.  With c->dry nothing is launched (workspace sizing).
int vgg_lpips_chunk(caddy_ctx* c, const float* ref, const float* gen, int nf, float range, double* out, int ldo) {
    const bool dry = c->dry;
    const int H = c->cfg.height, W = c->cfg.width;
    hipStream_t st = c->stream;
    ArenaMark mark(c->act);
    T4 gr = valloc(c, nf, H, W, 3), gg = valloc(c, nf, H, W, 3);
    const long npix = (long)nf * H * W;
    if (!dry) {
        lpips_stage_launch(st, ref, gr.d, npix, (long)H * W, range);
        lpips_stage_launch(st, gen, gg.d, npix, (long)H * W, range);
    }
    T4 tr[5], tg[5];
    LpipsLevels lv{};
    double* part = nullptr;
    if (paired_walk(c, gr, gg, tr, tg, "caddy_frame_lpips: workspace too small", [&] {
            long total = 0;
            for (int l = 0; l < 5; l++) { lv.off[l] = total; lv.blocks[l] = lpips_blocks(tr[l].H * tr[l].W); lv.inv_px[l] = 1.0 / ((double)tr[l].H * tr[l].W); total += (long)nf * lv.blocks[l]; }
            part = c->dalloc((size_t)total);
        })) return -1;
    if (!dry) {
        for (int l = 0; l < 5; l++) {
            if (tr[l].fmt && tg[l].fmt) c->vgg.tap_s16 |= 1u << l;
            c->ck(lpips_head_launch(st, tr[l].d, tr[l].fmt != 0, tg[l].d, tg[l].fmt != 0, c->vgg.lin[l], nf, tr[l].H * tr[l].W, tr[l].C, lv.blocks[l], part + lv.off[l]), "lpips head");
        }
        lpips_finalize_launch(st, part, lv, nf, out, ldo);
    }
    return c->fail ? -1 : 0;
}

// ---- per-kernel entry points (unit-parity tests; include/caddy_hip.h) ----
// Each launches one point-wise kernel of this file on caller-supplied device buffers through the drivers' own dispatch (launch_* / grid_for / cos_blocks above: the same flag-to-
// instance mapping, no kernel instance of its own).  Maps are dense NHWC (pitch == C).  Arguments are validated BEFORE anything is launched: -1 and no launch for a null pointer,
// a non-positive size, C % 4 != 0, an S16 operand with C % 32 != 0, and what each entry point names below.
namespace {
bool kmap_ok(const void* p, int N, int H, int W, int C, int s16) { return p && N >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && N <= 65535 && (!s16 || C % 32 == 0); }
T4 kmap(const float* d, float* g, int N, int H, int W, int C, int s16) {
    T4 t{};
    t.d = const_cast<float*>(d); t.g = g; t.N = N; t.H = H; t.W = W; t.C = C; t.sn = (long)H * W * C; t.ld = C; t.fmt = s16 ? 1 : 0;
    return t;
}
int klaunched() { return hipGetLastError() == hipSuccess ? 0 : -1; }
}  // namespace

int caddy_k_vgg_maxpool2(const float* in, float* out, int N, int H, int W, int C, void* stream) {      // fp32 only, as vgg_forward launches it
    if (!kmap_ok(in, N, H, W, C, 0) || !out) return -1;
    const long n4 = (long)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(k_maxpool2, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, in, out, n4, H, W, C / 4);
    return klaunched();
}
int caddy_k_vgg_maxpool2_bwd_relu(const float* a, int a_s16, const float* gp, float* gz, int gz_s16, int N, int H, int W, int C, void* stream) {
    if (!kmap_ok(a, N, H, W, C, a_s16 || gz_s16) || !gp || !gz) return -1;
    launch_maxpool_bwd((hipStream_t)stream, kmap(a, gz, N, H, W, C, a_s16), gp, gz_s16 != 0);
    return klaunched();
}
int caddy_k_vgg_feat_l1(const float* rec, int rec_s16, const float* gt, int gt_s16, int N, int H, int W, int C, float seed_w, float* gz, int gz_s16, double* acc, void* stream) {
    if (!kmap_ok(rec, N, H, W, C, rec_s16 || gt_s16 || (gz && gz_s16)) || !gt || !acc) return -1;
    launch_feat_l1((hipStream_t)stream, kmap(rec, nullptr, N, H, W, C, rec_s16), kmap(gt, nullptr, N, H, W, C, gt_s16), seed_w, gz, gz_s16 != 0, acc);
    return klaunched();
}
int caddy_k_vgg_feat_l1_img(const float* rec, int rec_s16, const float* gt, int gt_s16, int N, int H, int W, int C, double* acc, void* stream) {
    if (!kmap_ok(rec, N, H, W, C, rec_s16 || gt_s16) || !gt || !acc) return -1;
    launch_feat_l1_img((hipStream_t)stream, kmap(rec, nullptr, N, H, W, C, rec_s16), kmap(gt, nullptr, N, H, W, C, gt_s16), acc);
    return klaunched();
}
int caddy_k_vgg_cos_blocks(int H, int W, int C) {      // workgroups (= partial triples) per image of the per-image kernels on an H x W x C map
    if (H < 1 || W < 1 || C < 4 || C % 4) return -1;
    return cos_blocks(kmap(nullptr, nullptr, 1, H, W, C, 0));
}
// the cosine path of vgg_metric_chunk on the caller's five levels: part = the partial slab (part_doubles >= sum_l 3 * nf * cos_blocks_l doubles, level regions in order), out = nf
// doubles.  -1 if the slab is too small
int caddy_k_vgg_feat_cos(const VggCosArgs* a, int nf, double* part, long part_doubles, double* out, void* stream) {
    if (!a || !part || !out || nf < 1) return -1;
    T4 tx[5], ty[5];
    CosLevels lv{};
    long total = 0;
    for (int l = 0; l < 5; l++) {
        if (!kmap_ok(a->x[l], nf, a->H[l], a->W[l], a->C[l], a->x_s16[l] || a->y_s16[l]) || !a->y[l]) return -1;
        tx[l] = kmap(a->x[l], nullptr, nf, a->H[l], a->W[l], a->C[l], a->x_s16[l]);
        ty[l] = kmap(a->y[l], nullptr, nf, a->H[l], a->W[l], a->C[l], a->y_s16[l]);
        lv.off[l] = total; lv.blocks[l] = cos_blocks(tx[l]); total += (long)nf * lv.blocks[l] * 3;
    }
    if (total > part_doubles) return -1;
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < 5; l++) launch_feat_cos_img(st, tx[l], ty[l], part + lv.off[l]);
    hipLaunchKernelGGL(k_feat_cos_finalize, dim3((nf + 63) / 64), dim3(64), 0, st, (const double*)part, lv, nf, out);
    return klaunched();
}
int caddy_k_vgg_metric_stage(const float* src, float* out, int N, int H, int W, float range, void* stream) {      // (N, 3, H, W) -> (N, H, W, 4)
    if (!src || !out || N < 1 || H < 1 || W < 1 || !(range > 0.f)) return -1;
    const long npix = (long)N * H * W;
    hipLaunchKernelGGL(k_metric_stage, dim3(grid_for(npix)), dim3(256), 0, (hipStream_t)stream, src, out, npix, (long)H * W, range);
    return klaunched();
}
// obs: B * Tobs frames of f Ho x f Wo pixels, pitch ld >= 3; out: (B * Trec, Ho, Wo, 4).  -1 for f outside {1, 2, 4}, an observation that is not f times the output, or a time
// window [t_off, t_off + Trec) that leaves the sequence
int caddy_k_vgg_gt_resize(const TV* obs, float* out, int Ho, int Wo, int B, int Tobs, int Trec, int t_off, int f, void* stream) {
    if (!obs || !obs->p || !out || Ho < 1 || Wo < 1 || B < 1 || Tobs < 1 || Trec < 1 || t_off < 0) return -1;
    if (f != 1 && f != 2 && f != 4) return -1;
    if (obs->H % f || obs->W % f || obs->H != f * Ho || obs->W != f * Wo || obs->ld < 3 || obs->sn < (long)obs->H * obs->W * obs->ld) return -1;
    if (t_off + Trec > Tobs || obs->N != B * Tobs) return -1;
    const long npix = (long)B * Trec * Ho * Wo;
    hipLaunchKernelGGL(k_gt_resize, dim3(grid_for(npix)), dim3(256), 0, (hipStream_t)stream, *obs, out, Ho, Wo, npix, f, t_off, Tobs, Trec);
    return klaunched();
}
// full: (B, Tfull) frames of F4 float4, chunk: (B, len) frames; add = 0 gathers the time steps [t0, t0 + len) into chunk, add = 1 adds chunk onto them.  -1 unless 0 <= t0 and t0 + len <= Tfull
int caddy_k_vgg_time_chunk(float* full, float* chunk, int B, int Tfull, long F4, int t0, int len, int add, void* stream) {
    if (!full || !chunk || B < 1 || Tfull < 1 || F4 < 1 || t0 < 0 || len < 1 || t0 + len > Tfull) return -1;
    const long total4 = (long)B * len * F4;
    hipLaunchKernelGGL(k_time_chunk, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, (float4*)full, (float4*)chunk, F4, Tfull, t0, len, total4, add ? 1 : 0);
    return klaunched();
}
int caddy_k_vgg_copy_f(const float* src, float* dst, long n, void* stream) {      // one workgroup, as vgg_load launches it
    if (!src || !dst || n < 0) return -1;
    hipLaunchKernelGGL(k_copy_f, dim3(1), dim3(256), 0, (hipStream_t)stream, src, dst, n);
    return klaunched();
}
