// Per-frame quality metrics of the dataset evaluation in ONE pass over every reference / generated frame pair.
//
// Reference: evaluation/dataset_evaluator.py:150-170 (check_range + the per-frame metrics), evaluation/metrics/mse.py:13-24,
// evaluation/metrics/motion_masked_mse.py:16-28 with evaluation/metrics/motion_mask.py:14-37 (frame-difference mask of the REFERENCE sequence,
// summed over the channels / 3, zero at t = 0, not divided by the value range), evaluation/metrics/psnr.py:11-31, evaluation/metrics/ssim.py:13-35
// (piq.ssim(generated, reference, data_range, reduction="none"), piq 0.5.1 as env.yml pins it: x = gen / range, y = ref / range, 11 x 11 Gaussian
// window with sigma 1.5, valid padding, c1 = 0.01^2, c2 = 0.03^2, mean over the map, then over the channels).
//
// piq first average-pools both frames by f = max(1, round(min(H, W) / 256)) (Python's round: half to even).  piq's source is not at hand to check
// that rule against; every shipped configuration has a shorter side of at most 256 (f = 1), so no shipped configuration takes the f > 1 branch.
//
// Structure: one workgroup per (frame, FM_TH x FM_TW tile of the SSIM map).  The tile plus its 10-pixel halo of BOTH frames (3 channels, divided by
// the range and pooled when f > 1) is staged in LDS once; per channel an 11-tap horizontal pass writes the five moments x, y, x^2, y^2, xy of every
// staged row to LDS, an 11-tap vertical pass forms the SSIM terms of the tile's valid positions.  The squared error, the motion-masked squared error
// and the value ranges are accumulated while staging, over the pixels the tile OWNS (its halo-free rows / columns; the last tile row / column
// also owns the image's remaining rows / columns), so that every pixel counts once.  With f > 1 the staged pixels are pooled ones: the full-resolution
// sums then come from a separate loop over the owned full-resolution rectangle.
//
// Determinism: no float atomics.  Every workgroup reduces in a fixed tree (wave shuffles, then the four waves in order) and writes FM_PART fp64
// partials of its (frame, tile) to a slab; k_fm_finalize sums each frame's tiles in tile order.  Two calls on the same input are bit-identical.
#include "frame_metrics.h"
#include <cfloat>

namespace {

constexpr int RH = FM_TH + FM_WIN - 1, RW = FM_TW + FM_WIN - 1;      // staged rows / columns

struct FmArgs {
    const float* ref; const float* gen;
    int n0, T, H, W, f, Hp, Wp, tx, ty;
    float range;
    float g[FM_WIN];      // normalised 1-D Gaussian: the window is its outer product
    double* slab;
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// squared error, motion-masked squared error and value ranges of one full-resolution pixel (3 channels)
struct PixAcc {
    float sse = 0.f, msse = 0.f, rmin = FLT_MAX, rmax = -FLT_MAX, gmin = FLT_MAX, gmax = -FLT_MAX;
    __device__ __forceinline__ void add(const float r[3], const float g[3], const float* prev) {      // prev: the previous reference frame's channels, or null (t = 0)
        float d2[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float d = r[c] - g[c];
            d2[c] = d * d;
            sse += d2[c];
            rmin = fminf(rmin, r[c]); rmax = fmaxf(rmax, r[c]); gmin = fminf(gmin, g[c]); gmax = fmaxf(gmax, g[c]);
        }
        if (prev) {      // motion_mask.py:29-34: |ref_t - ref_{t-1}| summed over the channels, / 3
            const float m = (fabsf(r[0] - prev[0]) + fabsf(r[1] - prev[1]) + fabsf(r[2] - prev[2])) / 3.f;
            msse += d2[0] * m + d2[1] * m + d2[2] * m;
        }
    }
};

__global__ __launch_bounds__(256) void k_frame_metrics(FmArgs a) {
    __shared__ float sx[3][RH][RW], sy[3][RH][RW];      // x = gen / range, y = ref / range (pooled when f > 1)
    __shared__ float hm[5][RH][FM_TW];                   // horizontal pass: x, y, x^2, y^2, xy
    __shared__ double red[4][4];
    __shared__ float redm[4][4];
    const int tid = threadIdx.x;
    const int n = a.n0 + blockIdx.z, t = n % a.T;
    const int oy0 = blockIdx.y * FM_TH, ox0 = blockIdx.x * FM_TW;
    const long plane = (long)a.H * a.W;
    const float* R = a.ref + (long)n * 3 * plane;
    const float* G = a.gen + (long)n * 3 * plane;
    const float* P = t > 0 ? R - 3 * plane : nullptr;      // previous reference frame of the same sequence
    // pixels this tile owns (in staged coordinates): its FM_TH x FM_TW block; the last tile row / column also owns the rest of the frame
    const int own_h = blockIdx.y + 1 == gridDim.y ? a.Hp - oy0 : FM_TH;
    const int own_w = blockIdx.x + 1 == gridDim.x ? a.Wp - ox0 : FM_TW;
    PixAcc acc;
    // ---- staging ----
    if (a.f == 1) {
        // all loads of a thread's pixels are issued before the first is used (8 pixels x 3 channels x up to 3 frames in flight): with two workgroups per CU
        // (the LDS footprint) a load-use loop would leave the memory latency exposed
        constexpr int NI = (RH * RW + 255) / 256;
        float r[NI][3], g[NI][3], q[NI][3];
#pragma unroll
        for (int j = 0; j < NI; j++) {
            const int i = tid + j * 256, ry = i / RW, rx = i - ry * RW, py = oy0 + ry, px = ox0 + rx;
            const bool in = i < RH * RW && py < a.Hp && px < a.Wp;
            const long p = in ? (long)py * a.W + px : 0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                r[j][c] = in ? R[p + c * plane] : 0.f;
                g[j][c] = in ? G[p + c * plane] : 0.f;
                q[j][c] = (in && P && ry < own_h && rx < own_w) ? P[p + c * plane] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < NI; j++) {
            const int i = tid + j * 256, ry = i / RW, rx = i - ry * RW, py = oy0 + ry, px = ox0 + rx;
            if (i >= RH * RW) break;
            const bool in = py < a.Hp && px < a.Wp;
#pragma unroll
            for (int c = 0; c < 3; c++) { sx[c][ry][rx] = in ? g[j][c] / a.range : 0.f; sy[c][ry][rx] = in ? r[j][c] / a.range : 0.f; }
            if (in && ry < own_h && rx < own_w) acc.add(r[j], g[j], P ? q[j] : nullptr);
        }
    } else {
        for (int i = tid; i < RH * RW; i += 256) {      // avg_pool2d(kernel f, stride f) of the range-normalised frames
            const int ry = i / RW, rx = i - ry * RW, py = oy0 + ry, px = ox0 + rx;
            const bool in = py < a.Hp && px < a.Wp;
            const float inv = 1.f / (float)(a.f * a.f);
            for (int c = 0; c < 3; c++) {
                float sg = 0.f, sr = 0.f;
                for (int dy = 0; in && dy < a.f; dy++)
                    for (int dx = 0; dx < a.f; dx++) {
                        const long p = (long)(py * a.f + dy) * a.W + px * a.f + dx + c * plane;
                        sg += G[p] / a.range; sr += R[p] / a.range;
                    }
                sx[c][ry][rx] = sg * inv; sy[c][ry][rx] = sr * inv;
            }
        }
    }
    if (a.f > 1) {      // full-resolution sums over the owned rectangle (pooling drops the remainder rows / columns; they are still owned by the last tiles)
        const int y0 = oy0 * a.f, x0 = ox0 * a.f;
        const int y1 = blockIdx.y + 1 == gridDim.y ? a.H : y0 + FM_TH * a.f, x1 = blockIdx.x + 1 == gridDim.x ? a.W : x0 + FM_TW * a.f;
        const int w = x1 - x0;
        for (long i = tid; i < (long)(y1 - y0) * w; i += 256) {
            const int yy = y0 + (int)(i / w), xx = x0 + (int)(i % w);
            const long p = (long)yy * a.W + xx;
            float r[3], g[3], q[3];
#pragma unroll
            for (int c = 0; c < 3; c++) { r[c] = R[p + c * plane]; g[c] = G[p + c * plane]; q[c] = P ? P[p + c * plane] : 0.f; }
            acc.add(r, g, P ? q : nullptr);
        }
    }
    __syncthreads();
    // ---- SSIM: per channel, horizontal then vertical 11-tap pass ----
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    const int vh = a.Hp - (FM_WIN - 1), vw = a.Wp - (FM_WIN - 1);      // valid map
    float ss = 0.f;
    for (int c = 0; c < 3; c++) {
        for (int i = tid; i < RH * FM_TW; i += 256) {
            const int ry = i / FM_TW, ox = i - ry * FM_TW;
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < FM_WIN; k++) {
                const float x = sx[c][ry][ox + k], y = sy[c][ry][ox + k], w = a.g[k];
                m0 += w * x; m1 += w * y; m2 += w * (x * x); m3 += w * (y * y); m4 += w * (x * y);
            }
            hm[0][ry][ox] = m0; hm[1][ry][ox] = m1; hm[2][ry][ox] = m2; hm[3][ry][ox] = m3; hm[4][ry][ox] = m4;
        }
        __syncthreads();
        for (int i = tid; i < FM_TH * FM_TW; i += 256) {
            const int oy = i / FM_TW, ox = i - oy * FM_TW;
            if (oy0 + oy >= vh || ox0 + ox >= vw) continue;
            float mx = 0.f, my = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
            for (int k = 0; k < FM_WIN; k++) {
                const float w = a.g[k];
                mx += w * hm[0][oy + k][ox]; my += w * hm[1][oy + k][ox]; exx += w * hm[2][oy + k][ox]; eyy += w * hm[3][oy + k][ox]; exy += w * hm[4][oy + k][ox];
            }
            const float mxx = mx * mx, myy = my * my, mxy = mx * my;
            const float sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
            const float cs = (2.f * sxy + c2) / (sxx + syy + c2);
            ss += (2.f * mxy + c1) / (mxx + myy + c1) * cs;
        }
        __syncthreads();      // hm is rewritten by the next channel
    }
    // ---- fixed-order workgroup reduction -> this (frame, tile)'s partials ----
    const int wv = tid >> 6, ln = tid & 63;
    const double s0 = wave_sum((double)acc.sse), s1 = wave_sum((double)acc.msse), s2 = wave_sum((double)ss);
    const float q0 = wave_min(acc.rmin), q1 = wave_max(acc.rmax), q2 = wave_min(acc.gmin), q3 = wave_max(acc.gmax);
    if (ln == 0) { red[wv][0] = s0; red[wv][1] = s1; red[wv][2] = s2; redm[wv][0] = q0; redm[wv][1] = q1; redm[wv][2] = q2; redm[wv][3] = q3; }
    __syncthreads();
    if (tid < FM_PART) {
        double v;
        if (tid < 3) v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        else if (tid < 7) {
            const int j = tid - 3;
            const bool mn = j == 0 || j == 2;
            float m = redm[0][j];
            for (int w = 1; w < 4; w++) m = mn ? fminf(m, redm[w][j]) : fmaxf(m, redm[w][j]);
            v = (double)m;
        } else v = 0.0;
        a.slab[(((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * FM_PART + tid] = v;
    }
}

// one wave per frame: lane l sums tiles l, l + 64, ... in order, then a fixed shuffle tree -> MSE, motion-masked MSE, PSNR, SSIM, value ranges (slots of caddy_hip.h: CADDY_FM_*)
__global__ __launch_bounds__(256) void k_fm_finalize(const double* slab, int nf, int tiles, double inv_px, double inv_ssim, double inv_range2, double* out, int ldo) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), ln = threadIdx.x & 63;
    if (j >= nf) return;      // (whole waves: the shuffles below see every lane of a live wave)
    const double* s = slab + (long)j * tiles * FM_PART;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, rmn = s[3], rmx = s[4], gmn = s[5], gmx = s[6];
    for (int k = ln; k < tiles; k += 64) {
        const double* q = s + (long)k * FM_PART;
        a0 += q[0]; a1 += q[1]; a2 += q[2];
        rmn = fmin(rmn, q[3]); rmx = fmax(rmx, q[4]); gmn = fmin(gmn, q[5]); gmx = fmax(gmx, q[6]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o);
        rmn = fmin(rmn, __shfl_xor(rmn, o)); rmx = fmax(rmx, __shfl_xor(rmx, o)); gmn = fmin(gmn, __shfl_xor(gmn, o)); gmx = fmax(gmx, __shfl_xor(gmx, o));
    }
    if (ln != 0) return;
    const double mse = a0 * inv_px;
    out[0 * (long)ldo + j] = mse;
    out[1 * (long)ldo + j] = a1 * inv_px;
    out[2 * (long)ldo + j] = -10.0 * log10(mse * inv_range2 + 1e-8);      // metrics.psnr / psnr.py:27-29
    out[3 * (long)ldo + j] = a2 * inv_ssim;
    out[5 * (long)ldo + j] = rmn; out[6 * (long)ldo + j] = rmx; out[7 * (long)ldo + j] = gmn; out[8 * (long)ldo + j] = gmx;
}

}  // namespace

bool fm_geometry(int H, int W, FmGeom* g) {
    const int m = H < W ? H : W, q = m / 256, r = m % 256;
    g->H = H; g->W = W;
    g->f = q + (r > 128 || (r == 128 && (q & 1)) ? 1 : 0);      // round(m / 256), half to even
    if (g->f < 1) g->f = 1;
    g->Hp = H / g->f; g->Wp = W / g->f;
    if (g->Hp < FM_WIN || g->Wp < FM_WIN) return false;
    g->ty = (g->Hp - (FM_WIN - 1) + FM_TH - 1) / FM_TH;
    g->tx = (g->Wp - (FM_WIN - 1) + FM_TW - 1) / FM_TW;
    return true;
}

int fm_launch(const float* ref, const float* gen, int n0, int nf, int T, const FmGeom& g, float value_range, double* slab, double* out, int ldo, hipStream_t st) {
    if (nf <= 0) return 0;
    FmArgs a{};
    a.ref = ref; a.gen = gen; a.n0 = n0; a.T = T; a.H = g.H; a.W = g.W; a.f = g.f; a.Hp = g.Hp; a.Wp = g.Wp; a.tx = g.tx; a.ty = g.ty;
    a.range = value_range; a.slab = slab;
    double w[FM_WIN], sum = 0.0;
    for (int k = 0; k < FM_WIN; k++) { const double d = k - (FM_WIN - 1) / 2; w[k] = exp(-d * d / (2.0 * 1.5 * 1.5)); sum += w[k]; }
    for (int k = 0; k < FM_WIN; k++) a.g[k] = (float)(w[k] / sum);
    hipLaunchKernelGGL(k_frame_metrics, dim3(g.tx, g.ty, nf), dim3(256), 0, st, a);
    const double vh = g.Hp - (FM_WIN - 1), vw = g.Wp - (FM_WIN - 1);
    hipLaunchKernelGGL(k_fm_finalize, dim3((nf + 3) / 4), dim3(256), 0, st, (const double*)slab, nf, g.tx * g.ty, 1.0 / (3.0 * g.H * g.W), 1.0 / (3.0 * vh * vw),
                       1.0 / ((double)value_range * value_range), out, ldo);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
