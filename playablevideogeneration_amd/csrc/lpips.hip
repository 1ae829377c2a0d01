// LPIPS head (lpips.h).  Reference: evaluation/metrics/lpips.py:14,33 evaluates lpips.LPIPS(net='vgg') per observation; the package's arithmetic for one frame pair is
//   v = (2 x / range - 1 - shift) / scale;  f_l = relu1_2, 2_2, 3_3, 4_3, 5_3 of VGG16(v);  n(f) = f / (sqrt(sum_c f_c^2) + 1e-10) per pixel;
//   level_l = mean_{h,w} sum_c w_{l,c} (n(f0)_c - n(f1)_c)^2;  lpips = sum_l level_l.
//
// k_lpips_head reads the two tapped maps of a level ONCE and writes nothing but one fp64 partial per (frame, workgroup).  A group of 16 lanes owns a pixel: lane j holds channels
// 4 (j + 16 k) .. + 3, k < C / 64, of BOTH maps in registers (16-byte loads, a group reads 256 contiguous bytes per k), the two squared norms are reduced across the group with four
// xor shuffles, and the weighted squared difference of the unit vectors is formed directly -- not expanded into |a|^2, |b|^2 and a.b sums, which cancel by two orders of magnitude
// for near-identical frames.  Identical maps give exactly 0; swapping the maps gives the same bits.
//
// Determinism: no float atomics.  A workgroup reduces in a fixed tree (fp32 inside a pixel, fp64 across pixels: wave shuffles, then the four waves in order); k_lpips_finalize sums
// each frame's partials in block order.  Two calls on the same input are bit-identical.
#include "lpips.h"

namespace {

typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
// float4 number i of a dense map: plain fp32, or an S16-f16 tensor (common.h: every 32 channels as 32 f16 hi halves followed by 32 f16 lo halves; value = hi + lo)
template <bool S> __device__ __forceinline__ float4 ld4(const float* p, long i) {
    if (!S) return reinterpret_cast<const float4*>(p)[i];
    const long i4 = 4 * i;
    const _Float16* h = reinterpret_cast<const _Float16*>(p + (i4 & ~31L)) + (i4 & 31);
    const f16x4_t hi = *reinterpret_cast<const f16x4_t*>(h), lo = *reinterpret_cast<const f16x4_t*>(h + 32);
    return make_float4((float)hi[0] + (float)lo[0], (float)hi[1] + (float)lo[1], (float)hi[2] + (float)lo[2], (float)hi[3] + (float)lo[3]);
}
__device__ __forceinline__ float sq4(float4 v) { return v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }
__device__ __forceinline__ float wd4(float4 w, float4 a, float na, float4 b, float nb) {
    const float dx = a.x / na - b.x / nb, dy = a.y / na - b.y / nb, dz = a.z / na - b.z / nb, dw = a.w / na - b.w / nb;
    return w.x * (dx * dx) + w.y * (dy * dy) + w.z * (dz * dz) + w.w * (dw * dw);
}

// grid (blocks, frames); NK = C / 64 float4 per lane and map; S0 / S1: f0 / f1 are S16-f16 tensors
template <int NK, bool S0, bool S1>
__global__ __launch_bounds__(256) void k_lpips_head(const float* f0, const float* f1, const float* w, int npix, double* part) {
    constexpr int C4 = NK * 16;      // float4 per pixel
    __shared__ double sh[4];
    const int tid = threadIdx.x, gl = tid & 15, gp = tid >> 4;      // lane in its pixel group, pixel group in the workgroup
    const long img4 = (long)blockIdx.y * npix * C4;
    float4 wv[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) wv[k] = reinterpret_cast<const float4*>(w)[gl + 16 * k];
    double acc = 0.0;
    // (trip count uniform over the workgroup: every lane takes part in the shuffles; pixels past the end contribute zero maps)
    for (int p0 = blockIdx.x * 16; p0 < npix; p0 += gridDim.x * 16) {
        const int p = p0 + gp;
        const bool in = p < npix;
        const long q = img4 + (long)(in ? p : 0) * C4 + gl;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 a[NK], b[NK];
#pragma unroll
        for (int k = 0; k < NK; k++) { a[k] = in ? ld4<S0>(f0, q + 16 * k) : zero; b[k] = in ? ld4<S1>(f1, q + 16 * k) : zero; }
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int k = 0; k < NK; k++) { sa += sq4(a[k]); sb += sq4(b[k]); }
        for (int o = 8; o > 0; o >>= 1) { sa += __shfl_xor(sa, o, 16); sb += __shfl_xor(sb, o, 16); }
        const float na = sqrtf(sa) + 1e-10f, nb = sqrtf(sb) + 1e-10f;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NK; k++) s += wd4(wv[k], a[k], na, b[k], nb);
        acc += (double)s;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((tid & 63) == 0) sh[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one thread per frame: the blocks of each level in order, / (H_l W_l); the levels in order
__global__ __launch_bounds__(64) void k_lpips_finalize(const double* part, LpipsLevels lv, int nf, double* out, int ldo) {
#pragma clang fp contract(off)      // the total is the sum of the level values AS STORED: no fused multiply-add of the last level's product onto it
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= nf) return;
    double total = 0.0;
    for (int l = 0; l < 5; l++) {
        const double* p = part + lv.off[l] + (long)n * lv.blocks[l];
        double s = 0.0;
        for (int k = 0; k < lv.blocks[l]; k++) s += p[k];
        s *= lv.inv_px[l];
        out[(long)(1 + l) * ldo + n] = s;
        total += s;
    }
    out[n] = total;
}

// ScalingLayer constants of the package (per RGB channel)
__global__ __launch_bounds__(256) void k_lpips_stage(const float* src, float* out, long npix, long hw, float range) {
    for (long q = blockIdx.x * 256L + threadIdx.x; q < npix; q += (long)gridDim.x * 256) {
        const long n = q / hw, p = q - n * hw;
        const float* s = src + n * 3 * hw + p;
        const float u0 = 2.f * s[0] / range - 1.f, u1 = 2.f * s[hw] / range - 1.f, u2 = 2.f * s[2 * hw] / range - 1.f;
        reinterpret_cast<float4*>(out)[q] = make_float4((u0 - -.030f) / .458f, (u1 - -.088f) / .448f, (u2 - -.188f) / .450f, 0.f);
    }
}

template <int NK>
void head_launch_nk(hipStream_t st, dim3 g, const float* f0, bool s0, const float* f1, bool s1, const float* w, int npix, double* part) {
    with_bools([&](auto S0, auto S1) { hipLaunchKernelGGL((k_lpips_head<NK, decltype(S0)::value, decltype(S1)::value>), g, dim3(256), 0, st, f0, f1, w, npix, part); }, s0, s1);
}

}  // namespace

int lpips_blocks(int npix) { const int b = (npix + 15) / 16; return b < 1 ? 1 : (b > 128 ? 128 : b); }

void lpips_stage_launch(hipStream_t st, const float* src, float* out, long npix, long hw, float range) {
    long b = (npix + 255) / 256;
    b = b < 1 ? 1 : (b > 4096 ? 4096 : b);
    hipLaunchKernelGGL(k_lpips_stage, dim3((unsigned)b), dim3(256), 0, st, src, out, npix, hw, range);
}

int lpips_head_launch(hipStream_t st, const float* f0, bool s0, const float* f1, bool s1, const float* w, int nf, int npix, int C, int blocks, double* part) {
    if (nf < 1 || npix < 1 || blocks < 1) return -1;
    const dim3 g(blocks, nf);
    switch (C) {
        case 64: head_launch_nk<1>(st, g, f0, s0, f1, s1, w, npix, part); break;
        case 128: head_launch_nk<2>(st, g, f0, s0, f1, s1, w, npix, part); break;
        case 256: head_launch_nk<4>(st, g, f0, s0, f1, s1, w, npix, part); break;
        case 512: head_launch_nk<8>(st, g, f0, s0, f1, s1, w, npix, part); break;
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

void lpips_finalize_launch(hipStream_t st, const double* part, const LpipsLevels& lv, int nf, double* out, int ldo) {
    hipLaunchKernelGGL(k_lpips_finalize, dim3((nf + 63) / 64), dim3(64), 0, st, part, lv, nf, out, ldo);
}
