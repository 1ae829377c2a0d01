// FID feature network of the dataset evaluation (evaluation/metrics/fid.py:140-159 -> pytorch_fid/inception.py: InceptionV3([3]) with the FID patches): kernels and launchers
// of fid.hip.  Everything here is inference only; activations are NHWC fp32 through (p, sn, ld) views like the rest of the library, a block's branches write channel slices of
// one wider map (torch.cat(outputs, 1) is a free view).
#pragma once
#include "common.h"

// General implicit-GEMM forward convolution: KH x KW in {1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1} (any KH, KW <= 7 runs), stride 1 | 2, independent zero padding (ph, pw), folded
// BatchNorm bias + ReLU in the epilogue.  GEMM view: M = N * Ho * Wo output pixels (frames are batched into M: the 17 x 17 and 8 x 8 stages fill the machine through N, not by
// splitting K), N = Cout, K = KH * KW * round_up(Cin, 32).  Cin is a multiple of 8 -- or 3 with `gather`: a pitch-4 image whose K = KH * KW * 3 <= 32 is ONE K chunk.
struct IgemmArgs {
    const float* in; long in_sn; int in_ld; int Cin, Hi, Wi;
    int N, Ho, Wo, KH, KW, stride, ph, pw;
    const void* w;          // packed by igemm_pack for `precision`
    int nchunk;             // 32-channel chunks per tap (1 with gather)
    int gather;
    int Cout;
    const float* bias;      // nullable
    int relu;
    float* out; long out_sn; int out_ld;      // channel slice of a (possibly wider) map
    int precision;          // PREC_F16X3 (split f16 hi + lo, three products on v_mfma_f32_32x32x16_f16, weights pre-scaled by HX_WSCALE) | PREC_FP32 (v_mfma_f32_32x32x2_f32)
    unsigned* sat_flag;     // nullable; split f16 only: |x| > 65504 was clamped while staging (| 2: a NaN), see ConvArgs.sat_flag
};
static inline int igemm_out(int in, int k, int stride, int pad) { return (in + 2 * pad - k) / stride + 1; }
static inline int igemm_gather(int Cin, int KH, int KW) { return Cin < 8 && KH * KW * Cin <= 32; }
static inline int igemm_nchunk(int Cin, int KH, int KW) { return igemm_gather(Cin, KH, KW) ? 1 : (Cin + 31) / 32; }
// bytes of the packed weights of ONE arithmetic (both forms have 4 bytes per padded element: fp32, or an f16 hi + lo pair)
size_t igemm_weight_bytes(int Cin, int Cout, int KH, int KW);
// w: OIHW fp32.  gamma .. var: eval-mode BatchNorm2d(eps) behind the convolution (all four or none): folded into the packed weights and bias_out[o] = beta - mean * s (else
// bias_out, if given, receives bias_in or zeros).  Writes the fp32 form to w32 and the split-f16 form to w16 (either may be null).
int igemm_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, const float* bias_in, int Cin, int Cout, int KH, int KW,
               void* w32, void* w16, float* bias_out, hipStream_t st);
int igemm_launch(const IgemmArgs& a, hipStream_t st);

// 3 x 3 poolings on NHWC views (C a multiple of 4).  mode 0: MaxPool2d(3, 2) unpadded; 1: avg_pool2d(3, 1, 1, count_include_pad=False); 2: max_pool2d(3, 1, 1);
// 3: avg_pool2d(3, 1, 1) with torch's default count_include_pad=True (the sum over the window inside the map, divided by 9 everywhere)
int fid_pool_launch(const TV& in, const TV& out, int mode, hipStream_t st);
// mean over H x W of every channel, fp32 values summed in fp64 in pixel order: out[n * C + c]
int fid_global_avg_launch(const TV& in, double* out, hipStream_t st);
// (n, 3, Hs, Ws) planar fp32 in [0, 1] -> NHWC pitch-4 image of Ho x Wo: F.interpolate(mode='bilinear', align_corners=False) when the sizes differ, then 2 x - 1 (normalise) or
// the value as it is (the Inception Score's network: evaluation/metrics/inception_score.py:20-22,41)
int fid_stage_launch(const float* src, int n, int Hs, int Ws, float* out, int Ho, int Wo, hipStream_t st, int normalise = 1);
// softmax over the C columns of each of n rows (pitches ld_in / ld_out floats), fp32, one wave64 per row: evaluation/metrics/inception_score.py:43
int is_softmax_launch(const float* logits, float* probs, int n, int C, long ld_in, long ld_out, hipStream_t st);

struct caddy_ctx;
void fid_free(caddy_ctx* c);      // releases caddy_ctx::fid (caddy_ctx_destroy)
