// Frame-quality metrics of the dataset evaluation (evaluation/dataset_evaluator.py:165-170): one fused pass per reference / generated frame pair.
#pragma once
#include "common.h"

// tile of the SSIM map one workgroup produces (rows x columns); it stages (FM_TH + 10) x (FM_TW + 10) pixels of the frame pair
#define FM_TH 16
#define FM_TW 64
#define FM_WIN 11
#define FM_PART 8          // doubles per (frame, tile) of the partial slab: sum d^2, sum d^2 m, sum ssim, ref min, ref max, gen min, gen max, (pad)
#define FM_SLOTS 9         // CADDY_FM_COUNT

struct FmGeom { int H, W, f, Hp, Wp, tx, ty; };      // f: SSIM down-sampling factor; Hp x Wp: the (pooled) frame SSIM sees; tx x ty tiles per frame
// false: the pooled frame is smaller than the SSIM window (no valid position)
bool fm_geometry(int H, int W, FmGeom* g);
// ref / gen: (N, 3, H, W) fp32; frames [n0, n0 + nf) of sequences of T frames; out: FM_SLOTS x ldo doubles (device), slot s of frame n0 + j at out[s * ldo + j]
// (the VGG slot is left alone); slab: nf * tx * ty * FM_PART doubles
int fm_launch(const float* ref, const float* gen, int n0, int nf, int T, const FmGeom& g, float value_range, double* slab, double* out, int ldo, hipStream_t st);
