// Detector of the Breakout dataset evaluation (evaluation/metrics/breakout_platform_position.py): the platform's left edge in every frame.
#pragma once
#include "common.h"

#define DET_MAX_W 4096      // widest frame row the scan stages in LDS (one byte per column)

// obs: (N, 3, H, W) fp32 (device); frames [n0, n0 + nf); out[j] (device int32) = platform position of frame n0 + j, or -1.
// Mask of channel 0 of row `row`: lo <= v <= hi, the last column outside it; the answer is the start of the first run of >= min_run masked columns.
int det_platform_launch(const float* obs, int n0, int nf, int H, int W, int row, float lo, float hi, int min_run, int* out, hipStream_t st);
