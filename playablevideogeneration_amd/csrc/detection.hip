// Platform position of every frame for the Breakout dataset evaluation.
//
// Reference: evaluation/metrics/breakout_platform_position.py (BreakoutPlatformPosition.forward + detect_platform).  The reference builds the colour mask on
// all three channels, copies it to the host and walks row int(188 / 208 * H) of every frame in Python; detect_platform reads channel 0 only and treats the
// last column as outside the mask (`idx != width - 1`), so a run that reaches the right edge ends at W - 2.  It returns the start of the first run longer
// than 11 columns, or -1.
//
// Here: one wave64 per frame, four frames per 256-thread workgroup.  The wave loads its frame's row of channel 0 coalesced and writes the mask (lo <= v <= hi,
// false for NaN and for the last column) to LDS; after the barrier each lane tests its columns s = lane, lane + 64, ... as run starts (m[s], s == 0 or
// !m[s - 1], m[s .. s + min_run - 1] all set) and stops at its first hit; a shuffle min-reduction picks the smallest start.  No atomics: deterministic.
#include "detection.h"

namespace {

constexpr int NO_RUN = 0x7fffffff;

__global__ __launch_bounds__(256) void k_platform_positions(const float* obs, int n0, int nf, int H, int W, int row, float lo, float hi, int min_run, int* out) {
    __shared__ unsigned char msk[4][DET_MAX_W];
    const int w = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + w;
    const bool live = j < nf;      // whole waves: every lane of a wave sees the same j
    unsigned char* m = msk[w];
    if (live) {
        const float* p = obs + ((long)(n0 + j) * 3 * H + row) * W;      // channel 0, row `row`
        for (int x = ln; x < W; x += 64) {
            const float v = p[x];
            m[x] = (x != W - 1 && lo <= v && v <= hi) ? 1 : 0;
        }
    }
    __syncthreads();      // (no wave returns before this barrier)
    if (!live) return;
    int best = NO_RUN;
    for (int s = ln; s < W - min_run; s += 64) {      // a run needs s + min_run - 1 <= W - 2
        if (!m[s] || (s > 0 && m[s - 1])) continue;
        int k = 1;
        while (k < min_run && m[s + k]) k++;
        if (k == min_run) { best = s; break; }      // this lane's columns rise: its first hit is its smallest
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(best, o);
        best = other < best ? other : best;
    }
    if (ln == 0) out[j] = best == NO_RUN ? -1 : best;
}

}  // namespace

int det_platform_launch(const float* obs, int n0, int nf, int H, int W, int row, float lo, float hi, int min_run, int* out, hipStream_t st) {
    if (nf <= 0) return 0;
    hipLaunchKernelGGL(k_platform_positions, dim3((nf + 3) / 4), dim3(256), 0, st, obs, n0, nf, H, W, row, lo, hi, min_run, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
