// FVD feature network of the dataset evaluation (evaluation/metrics/fvd.py:67-126: the Kinetics-400 I3D of TensorFlow-Hub, output RGB/inception_i3d/Mean:0): kernels and
// launchers of fvd.hip.  Inference only; activations are NDHWC fp32 through (p, sn, ld) views with the frames of a video adjacent, a block's branches write channel slices of one
// wider map (tf.concat(..., 4) is a free view), as in fid.h.
#pragma once
#include "common.h"

// NDHWC view: element (n, t, y, x, c) at p[n * sn + ((t * H + y) * W + x) * ld + c]
struct V5 {
    float* p;
    int N, T, H, W, C;
    long sn;
    int ld;
};

// Implicit-GEMM forward 3-D convolution: any KT, KH, KW <= 7, strides in {1, 2}, independent LEADING zero padding (pt, ph, pw) with explicit output sizes (TensorFlow's SAME
// padding is asymmetric: taps outside the input read zero on either side), folded-BatchNorm bias + ReLU in the epilogue.  GEMM view: M = N * To * Ho * Wo output positions (videos
// and frames are batched into M), N = Cout, K = KT * KH * KW * round_up(Cin, 32).  Tile and arithmetic are those of k_conv_igemm (conv_igemm.h).  Cin is a multiple of 8 -- or < 8 with
// `gather`: a pitch-4 image, ONE K chunk per (kt, kh) row of the window (its KW taps x 4 channels are contiguous floats, the weights of the pad lane are zero): K = KT * KH * 32.
struct Conv3dArgs {
    const float* in; long in_sn; int in_ld; int Cin, Ti, Hi, Wi;
    int N, To, Ho, Wo, KT, KH, KW, st, sh, sw, pt, ph, pw;
    const void* w;          // packed by conv3d_pack for `precision`
    int nchunk;             // 32-channel chunks per tap (1 with gather)
    int gather;
    int Cout;
    const float* bias;      // nullable
    int relu;
    float* out; long out_sn; int out_ld;      // channel slice of a (possibly wider) map
    int precision;          // PREC_F16X3 | PREC_FP32, as IgemmArgs.precision
    unsigned* sat_flag;     // nullable; as IgemmArgs.sat_flag
};
static inline int conv3d_gather(int Cin, int KW) { return Cin < 8 && KW * 4 <= 32; }
static inline int conv3d_nchunk(int Cin, int KW) { return conv3d_gather(Cin, KW) ? 1 : (Cin + 31) / 32; }
static inline int conv3d_ksteps(int Cin, int KT, int KH, int KW) { return conv3d_gather(Cin, KW) ? KT * KH : KT * KH * KW * conv3d_nchunk(Cin, KW); }      // K chunks of 32
// TensorFlow SAME: out = ceil(in / stride), total padding max((out - 1) stride + k - in, 0), the smaller half in front
static inline int same_out(int in, int stride) { return (in + stride - 1) / stride; }
static inline int same_lead(int in, int k, int stride) { const int t = (same_out(in, stride) - 1) * stride + k - in; return t > 0 ? t / 2 : 0; }
size_t conv3d_weight_bytes(int Cin, int Cout, int KT, int KH, int KW);      // one arithmetic (4 bytes per padded element)
// w: DHWIO fp32 (TensorFlow's conv3d filter).  mean / var / beta (all three or none) with optional gamma: eval-mode batch norm behind the convolution, folded as igemm_pack does.
int conv3d_pack(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps, const float* bias_in, int Cin, int Cout, int KT, int KH, int KW,
                void* w32, void* w16, float* bias_out, hipStream_t st);
int conv3d_launch(const Conv3dArgs& a, hipStream_t st);

// 3-D max pooling with TensorFlow SAME padding (padded positions do not take part); window <= 3 and stride <= 2 per axis, C a multiple of 4
int fvd_pool_launch(const V5& in, const V5& out, int kt, int kh, int kw, int st, int sh, int sw, hipStream_t stream);
// (n, T, 3, Hs, Ws) planar fp32 in [0, 1] -> NDHWC pitch-4 image of Ho x Wo: TF1 resize_bilinear(align_corners=False) without half-pixel centres when the sizes differ
// (src = dst * in / out, i1 = min(i0 + 1, in - 1)), then 2 x - 1
int fvd_stage_launch(const float* src, long frames, int Hs, int Ws, float* out, int Ho, int Wo, hipStream_t st);

struct caddy_ctx;
void fvd_free(caddy_ctx* c);      // releases caddy_ctx::fvd (caddy_ctx_destroy)
