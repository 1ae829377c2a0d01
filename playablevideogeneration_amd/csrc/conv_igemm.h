// The implicit-GEMM convolution tile of the evaluation trunks: everything k_conv_igemm (fid.hip) and k_conv3d_igemm (fvd.hip) share.  A kernel decodes its tile position, supplies
// a loader for the eight floats a thread fetches per K step, and calls conv_igemm_tile; a pack kernel finds its source element and calls conv_pack_store.
//
// Workgroup = 256 threads = 2 x 2 waves on a 64 position x 64 channel tile, one 32 x 32 accumulator block per wave.  K runs in 32-deep steps in the order the loader defines.  Per
// K step every thread fetches 8 consecutive K elements of one tile position (bounds, padding and the channel tail give zeros), one step AHEAD of the matrix instructions (register
// prefetch), and stores them to LDS in operand form: fp32 for the exact path, an f16 (hi, lo) pair of planes for the split path (hi = f16(x), lo = f16(x - hi), |x| clamped to the
// f16 range with the sticky flag of ConvArgs.sat_flag).  The weight fragments never pass through LDS: the packers lay them out FRAGMENT-MAJOR (per K step and 32-channel block the
// 64 lanes' 16-byte pieces in lane order), so a wave reads each with one fully coalesced 1 KiB load that the other tiles of the launch find in L2.
// Split f16: acc += hi_a hi_w + hi_a lo_w + lo_a hi_w with the weights pre-scaled by HX_WSCALE (common.h) and the accumulator scaled back in the epilogue.
// Row padding of the LDS tiles (36 floats / 40 halves per 32 channels) makes the 16-byte fragment reads of 16 consecutive rows hit 16 distinct bank quads.
#pragma once
#include "common.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
constexpr float CG_F16_MAX = 65504.f;
constexpr int CG_BM = 64, CG_BN = 64, CG_KC = 32;
constexpr int CG_LDF = 36;      // floats per LDS row (fp32 operands)
constexpr int CG_LDH = 40;      // halves per LDS row and plane (split f16 operands)

struct ConvTile {
    const void* w;          // packed for the arithmetic of the instantiation
    int Cout;
    const float* bias;      // nullable
    int relu;
    float* out; long out_sn; int out_ld;      // channel slice of a (possibly wider) map
    unsigned* sat_flag;     // nullable
    long M, per;            // output positions of the launch / of one sample (Ho * Wo or To * Ho * Wo)
    int nsteps;             // K steps
};

// load(step, r0, r1) fills the calling thread's eight floats of K step `step`: tile position threadIdx.x >> 2, K elements 8 (threadIdx.x & 3) .. + 7.  It is called once per step
// in ascending order.
template <bool F16, class Loader>
__device__ __forceinline__ void conv_igemm_tile(const ConvTile& t, Loader& load) {
    __shared__ __attribute__((aligned(16))) float smem[F16 ? (2 * CG_BM * CG_LDH) / 2 : CG_BM * CG_LDF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const long m0 = (long)blockIdx.x * CG_BM;
    const int ncb = (int)gridDim.y * 2, cb = (int)blockIdx.y * 2 + wn;      // 32-channel blocks of the packed weights / this wave's block
    const int lrow = tid >> 2, lq = tid & 3;
    float4 r0, r1;
    f32x16 acc;
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    unsigned sat = 0;
    load(0, r0, r1);
    for (int step = 0; step < t.nsteps; step++) {
        // ---- registers -> LDS in operand form ----
        if (F16) {
            _Float16* sh = reinterpret_cast<_Float16*>(smem);
            const float x[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
            h8 hi, lo;
            for (int e = 0; e < 8; e++) {
                const float c = __builtin_amdgcn_fmed3f(x[e], -CG_F16_MAX, CG_F16_MAX);
                if (!(c == x[e])) sat |= (x[e] != x[e]) ? 3u : 1u;
                hi[e] = (_Float16)c;
                lo[e] = (_Float16)(c - (float)hi[e]);
            }
            *reinterpret_cast<h8*>(sh + lrow * CG_LDH + lq * 8) = hi;
            *reinterpret_cast<h8*>(sh + (CG_BM + lrow) * CG_LDH + lq * 8) = lo;
        } else {
            float4* d = reinterpret_cast<float4*>(smem + lrow * CG_LDF + lq * 8);
            d[0] = r0; d[1] = r1;
        }
        __syncthreads();
        if (step + 1 < t.nsteps) load(step + 1, r0, r1);
        // ---- matrix instructions: this wave's 32 positions x 32 channels over the step ----
        const int arow = wm * 32 + (lane & 31), half = lane >> 5;
        const long wt = ((long)step * ncb + cb);      // (K step, channel block) tile of the packed weights
        if (F16) {
            const _Float16* sh = reinterpret_cast<const _Float16*>(smem);
            const h8* wq = reinterpret_cast<const h8*>(t.w) + wt * 256 + lane;      // [K half kk][plane][lane]
#pragma unroll
            for (int kk = 0; kk < 2; kk++) {
                const h8 ah = *reinterpret_cast<const h8*>(sh + arow * CG_LDH + kk * 16 + half * 8);
                const h8 al = *reinterpret_cast<const h8*>(sh + (CG_BM + arow) * CG_LDH + kk * 16 + half * 8);
                const h8 bh = wq[(kk * 2 + 0) * 64], bl = wq[(kk * 2 + 1) * 64];
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
            }
        } else {
            const float4* wp = reinterpret_cast<const float4*>(t.w) + wt * 256 + lane;      // [g][lane]: channels 16 half + 4 g .. + 3
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const float4 av = *reinterpret_cast<const float4*>(smem + arow * CG_LDF + half * 16 + 4 * g);
                const float4 bv = wp[g * 64];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (F16 && sat && t.sat_flag) atomicOr(t.sat_flag, sat);
    // ---- epilogue: D fragment map col = lane & 31 (output channel), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (position of the tile) ----
    const int o = cb * 32 + (lane & 31);
    if (o >= t.Cout) return;
    const float b = t.bias ? t.bias[o] : 0.f;
    const float sc = F16 ? 1.f / HX_WSCALE : 1.f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const long m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= t.M) continue;
        const long n = m / t.per, rem = m - n * t.per;
        float v = acc[r] * sc + b;
        if (t.relu) v = v > 0.f ? v : 0.f;
        t.out[n * t.out_sn + rem * t.out_ld + o] = v;
    }
}

// ---- the packed weights: element (cl, ol) = (K element of the step, output channel of the 32-channel block) of tile = K step * ncb + cb, in both forms ----
__device__ __forceinline__ void conv_pack_store(float* w32, _Float16* w16, long tile, int cl, int ol, float v) {
    if (w32) {      // [g = (cl & 15) >> 2][lane = 32 (cl >> 4) + ol][e = cl & 3]
        w32[tile * 1024 + ((((cl & 15) >> 2) * 64 + (cl >> 4) * 32 + ol) * 4 + (cl & 3))] = v;
    }
    if (w16) {      // [kk = cl >> 4][plane][lane = 32 ((cl >> 3) & 1) + ol][e = cl & 7], values x HX_WSCALE
        const float vs = v * HX_WSCALE;
        const _Float16 hi = (_Float16)vs, lo = (_Float16)(vs - (float)hi);
        const long base = tile * 2048 + (long)(cl >> 4) * 1024 + (((cl >> 3) & 1) * 32 + ol) * 8 + (cl & 7);
        w16[base] = hi; w16[base + 512] = lo;
    }
}
// eval-mode batch norm behind the convolution, folded in fp64: w' = w s with s = gamma / sqrt(var + eps) (gamma null: 1), b' = beta - mean s.  mean null: no batch norm, s = 1 and
// the bias is bias_in (or zero).  o must be a real output channel.
__device__ __forceinline__ double conv_fold_scale(const float* gamma, const float* mean, const float* var, float eps, int o) {
    return mean ? (gamma ? (double)gamma[o] : 1.0) / sqrt((double)var[o] + (double)eps) : 1.0;
}
__device__ __forceinline__ float conv_fold_bias(const float* beta, const float* mean, const float* bias_in, double s, int o) {
    return mean ? (float)((double)beta[o] - (double)mean[o] * s) : (bias_in ? bias_in[o] : 0.f);
}
