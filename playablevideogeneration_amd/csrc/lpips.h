// LPIPS head of the dataset evaluation (evaluation/metrics/lpips.py:14,33 -> lpips.LPIPS(net='vgg'), version 0.1, spatial=False, normalize=True): input scaling and, per tapped
// VGG16 level, mean over the pixels of sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2.  The trunk runs on the VGG kernels of perceptual.hip (vgg_lpips_chunk).
#pragma once
#include "common.h"

struct LpipsLevels { long off[5]; int blocks[5]; double inv_px[5]; };      // region of the partial slab, blocks per frame and 1 / (H_l W_l) of each level
int lpips_blocks(int npix);      // workgroups (= partials) per frame of a level with npix pixels
// (N, 3, H, W) fp32 in [0, range] -> NHWC (pitch 4): u = 2 x / range - 1, v = (u - shift) / scale (the package's ScalingLayer)
void lpips_stage_launch(hipStream_t st, const float* src, float* out, long npix, long hw, float range);
// one level: f0 / f1 = dense NHWC maps of nf frames, npix pixels and C channels each (fp32, or S16-f16 when s0 / s1), w = C weights; part[n * blocks + b] = the partial of frame n,
// block b.  C must be 64, 128, 256 or 512 (-1 otherwise)
int lpips_head_launch(hipStream_t st, const float* f0, bool s0, const float* f1, bool s1, const float* w, int nf, int npix, int C, int blocks, double* part);
// per frame n: level_l = (sum of its blocks, in order) / (H_l W_l) -> out[(1 + l) * ldo + n], their sum in level order -> out[n]
void lpips_finalize_launch(hipStream_t st, const double* part, const LpipsLevels& lv, int nf, double* out, int ldo);
