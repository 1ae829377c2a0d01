// VGG19 perceptual loss (training/losses.py:379-491, model/layers/vgg.py:8-56): state kept in the context and the driver entry points.
#pragma once
#include "common.h"
#include "pack.h"

#define VGG_NCONV 13      // conv1_1 .. conv5_1: what model/layers/vgg.py:25-34 evaluates of torchvision's vgg19().features

struct VggLayer { PackDesc pd; float* wp; float* wpd; float* bias; int kd, cd_pad;
                  void* wq[3]; void* wqd[2]; };      // split 16-bit forms (conv_hx.hip): [0] two planes (3 products), [1] one plane; forward f16, dgrad bf16; wq[2]: forward as split bf16
// The trunk a context runs: (torchvision features index, Cin, Cout) of its 13 convolutions; pool_before: MaxPool2d(2, 2) on the input; tap: feature level this conv's ReLU is, or -1
struct VggSpec { int idx, cin, cout, pool_before, tap; };
enum { VGG_KIND_VGG19 = 0,        // vgg19().features up to relu5_1, taps relu{1..5}_1 (model/layers/vgg.py:25-34): perceptual loss, VGG cosine similarity
       VGG_KIND_LPIPS = 1 };      // vgg16().features up to relu5_3, taps relu1_2, 2_2, 3_3, 4_3, 5_3: the trunk of lpips.LPIPS(net='vgg') (evaluation/metrics/lpips.py:14)
const VggSpec* vgg_spec_table(int kind);
struct VggState { bool enabled = false, loaded = false; int kind = VGG_KIND_VGG19; const VggSpec* spec = nullptr; VggLayer conv[VGG_NCONV];
                  float* lin[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // LPIPS: the per-channel weights of lin{l}.model[1] (C_l floats each)
                  unsigned tap_s16 = 0; };                                             // LPIPS: bit l set = level l's taps travelled as S16 tensors in some chunk of the last caddy_frame_lpips
struct VggLevels { double numel[3][5]; };      // elements of the level-l feature map at resolution r (N * C * H * W)
// caddy_k_vgg_feat_cos (unit-parity tests): the five tapped maps of both image batches, dense NHWC of H[l] x W[l] x C[l] per frame, fp32 or (x_s16 / y_s16) S16-f16
struct VggCosArgs { const float* x[5]; const float* y[5]; int x_s16[5]; int y_s16[5]; int H[5]; int W[5]; int C[5]; };

struct caddy_ctx;
struct caddy_param_info;
struct T4;
int vgg_param_count();
long vgg_param_floats();
int vgg_param_info(int index, caddy_param_info* out);
int lpips_param_count();
long lpips_param_floats();
int lpips_param_info(int index, caddy_param_info* out);
void vgg_build(caddy_ctx* c, int kind = VGG_KIND_VGG19);
int vgg_load(caddy_ctx* c, const float* flat);      // (an LPIPS context: the 13 convolutions, then lin0 .. lin4 -- lpips_param_info's layout)
void vgg_perceptual(caddy_ctx* c, double lambda, const T4* gt_img, VggLevels* lv);
void vgg_gt_prefetch(caddy_ctx* c, int Trec, int t_off);
int vgg_eval_per_frame(caddy_ctx* c, double* out_host);      // evaluation: per reconstructed frame and level, full resolution (5 x N doubles, host)
int vgg_metric_chunk(caddy_ctx* c, const float* ref, const float* gen, int nf, float range, double* out);      // dataset evaluation: VGG19 cosine similarity per frame (nf doubles, device)
int vgg_lpips_chunk(caddy_ctx* c, const float* ref, const float* gen, int nf, float range, double* out, int ldo);      // dataset evaluation: LPIPS per frame (6 x ldo doubles, device: total, level 0 .. 4)
