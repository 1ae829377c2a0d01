// Host side of the split-operand 3x3 convolution: weight packing and the launcher (tile selection) of k_conv_hx (conv_hx_kernel.h).
#include "conv_hx_kernel.h"

namespace {

// ---- weight packing: OIHW fp32 (reference state_dict layout) -> split 16-bit tiles [tap][chunk][Cout_pad][hi 32 | lo 32] ----
template <typename T, int NPL>
__device__ __forceinline__ void pk_hx_elem(const PackDesc& d, T* wq, int Cout_pad, int dgrad_seg, int nch, long i) {
    // forward (dgrad_seg < 0): rows = output channels, k = concatenated input segments, each padded to KC.
    // dgrad of segment s: rows = input channels of s, k = output channels (padded to KC), taps flipped.
    const int taps = d.KS * d.KS;
    const int kk = (int)(i % KC); long r = i / KC; const int row = (int)(r % Cout_pad); r /= Cout_pad; const int ch = (int)(r % nch); const int tap = (int)(r / nch);
    const int k = ch * KC + kk;
    float v = 0.f;
    if (dgrad_seg < 0) {
        int base = 0, cin = -1;
        for (int s = 0; s < d.nseg; s++) {
            const int pad = (d.seg_C[s] + KC - 1) / KC * KC;
            if (k < base + pad) { if (k - base < d.seg_C[s]) cin = d.seg_off[s] + k - base; break; }
            base += pad;
        }
        if (row < d.Cout && cin >= 0) v = d.w[row / d.Co_each][((long)(row % d.Co_each) * d.Cin + cin) * taps + tap] * (d.oscale ? d.oscale[row] : 1.f);
    } else {
        if (row < d.seg_C[dgrad_seg] && k < d.Cout) v = d.w[k / d.Co_each][((long)(k % d.Co_each) * d.Cin + d.seg_off[dgrad_seg] + row) * taps + (taps - 1 - tap)];
    }
    if (sizeof(T) == 2 && !is_bf16<T>::value) v *= HX_WSCALE;      // f16 forms only (see HX_WSCALE)
    const T hi = (T)v;
    // FRAGMENT-MAJOR order inside every 32-row block of a (tap, chunk) tile (round 6; same bytes, permuted): [K half kh = kk >> 4][plane][lane = 32 (kk >> 3 & 1) + row & 31][8 halves]
    // -- the 1-KB run of (row block, kh, plane) IS the B operand of one v_mfma_f32_32x32x16 (lane l: row l & 31, eight channels (l >> 5) of the K half), so the kernels that take
    // their weight fragments straight from global memory (k_conv_hx<BG>) read it with one fully coalesced 16-byte load per lane; the LDS-staged kernels undo the permutation
    // when they store their 16-byte pieces (HX_STORE_B), conv_direct.hip addresses its 16 x 16 x 32 fragments through hx_wq_piece
    T* o = wq + ((long)tap * nch + ch) * Cout_pad * (NPL * KC) + hx_wq_piece<NPL>(row, kk >> 3) * 8 + (kk & 7);
    o[0] = hi;
    if (NPL == 2) o[64 * 8] = (T)(v - (float)hi);            // (plane 1: the next 64 pieces)
}
__device__ __forceinline__ int pk_hx_nch(const PackDesc& d, int dgrad_seg) {
    int Kq = 0;
    if (dgrad_seg < 0) { for (int s = 0; s < d.nseg; s++) Kq += (d.seg_C[s] + KC - 1) / KC * KC; }
    else Kq = (d.Cout + KC - 1) / KC * KC;
    return Kq / KC;
}
template <typename T, int NPL>
__global__ void k_pack_hx(PackDesc d, T* wq, int Cout_pad, int dgrad_seg) {
    const int nch = pk_hx_nch(d, dgrad_seg);
    const long total = (long)d.KS * d.KS * nch * Cout_pad * KC;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) pk_hx_elem<T, NPL>(d, wq, Cout_pad, dgrad_seg, nch, i);
}

// one launch over a job table (pack.h): workgroup -> job by binary search over the jobs' first blocks
__global__ __launch_bounds__(256) void k_pack_jobs(const PackJob* jobs, int njobs) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    const PackJob& j = jobs[lo];
    const long first = ((long)blockIdx.x - j.block0) * 256 + threadIdx.x, stride = (long)j.nblocks * 256;
    switch (j.kind) {
        case PJ_FWD: for (long i = first; i < j.total; i += stride) pk_fwd_elem(j.d, (float*)j.buf, i); break;
        case PJ_DGRAD: for (long i = first; i < j.total; i += stride) pk_dgrad_elem(j.d, j.seg, (float*)j.buf, j.p0, j.p1, i); break;
        case PJ_UNPACK: for (long i = first; i < j.total; i += stride) pk_unpack_elem(j.d, (const float*)j.buf, i); break;
        case PJ_HX_FWD_F16: { const int nch = pk_hx_nch(j.d, -1); for (long i = first; i < j.total; i += stride) pk_hx_elem<_Float16, 2>(j.d, (_Float16*)j.buf, j.p0, -1, nch, i); break; }
        case PJ_HX_DGRAD_BF16: { const int nch = pk_hx_nch(j.d, j.seg); for (long i = first; i < j.total; i += stride) pk_hx_elem<__bf16, 2>(j.d, (__bf16*)j.buf, j.p0, j.seg, nch, i); break; }
    }
}

}  // namespace

// bytes of the split weight buffer of a layer: forward form (seg < 0) or dgrad form of input segment `seg`
size_t hx_weight_bytes(const PackDesc& d, int seg, int rows_pad, int planes) {
    int Kq = 0;
    if (seg < 0) { for (int s = 0; s < d.nseg; s++) Kq += round_up(d.seg_C[s], HX_KC); }
    else Kq = round_up(d.Cout, HX_KC);
    return (size_t)d.KS * d.KS * Kq * rows_pad * planes * 2;
}
int hx_kq(const PackDesc& d, int seg) {
    int Kq = 0;
    if (seg < 0) { for (int s = 0; s < d.nseg; s++) Kq += round_up(d.seg_C[s], HX_KC); }
    else Kq = round_up(d.Cout, HX_KC);
    return Kq;
}
int pack_hx(const PackDesc& d, void* wq, int rows_pad, int seg, int precision, hipStream_t st) {
    const long total = (long)d.KS * d.KS * hx_kq(d, seg) * rows_pad;
    const unsigned grid = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    switch (precision) {
        case PREC_F16X3: hipLaunchKernelGGL((k_pack_hx<_Float16, 2>), dim3(grid), dim3(256), 0, st, d, (_Float16*)wq, rows_pad, seg); break;
        case PREC_BF16X3: hipLaunchKernelGGL((k_pack_hx<__bf16, 2>), dim3(grid), dim3(256), 0, st, d, (__bf16*)wq, rows_pad, seg); break;
        case PREC_F16X1: hipLaunchKernelGGL((k_pack_hx<_Float16, 1>), dim3(grid), dim3(256), 0, st, d, (_Float16*)wq, rows_pad, seg); break;
        case PREC_BF16X1: hipLaunchKernelGGL((k_pack_hx<__bf16, 1>), dim3(grid), dim3(256), 0, st, d, (__bf16*)wq, rows_pad, seg); break;
        default: return -1;
    }
    return 0;
}
int pack_jobs_launch(const PackJob* jobs_dev, int njobs, int total_blocks, hipStream_t st) {
    if (njobs <= 0 || total_blocks <= 0) return 0;
    hipLaunchKernelGGL(k_pack_jobs, dim3((unsigned)total_blocks), dim3(256), 0, st, jobs_dev, njobs);
    return 0;
}
int hx_pick_bn(int cout) { return cout > 64 ? 128 : (cout > 32 ? 64 : 32); }
int g_hx_big_override = -1;      // tests: force (1) / forbid (0) the 8-wave 16x16x128 tile variant regardless of the grid size
int g_hx_bg = -1;                // tests / A-B runs: >= 0 overrides CADDY_HX_BG (which under-filled tile variants take their weight fragments straight from global memory)
// Co-resident instance of the 16x16x128 tile (conv_hx_co.hip) for the launches that run beside the model chain.  A mask over ConvArgs.beside_chain: bit 0 the launches beside the
// forward pass (VGG19 ground-truth branch), bit 1 the launches beside the tape replay (pipelined VGG19 chunks), bit 2 every launch that takes the 8-wave tile (tests).
// -1: CADDY_VGG_BESIDE, default 1 -- measured on the MI355X (profiles/r07_vgg_coresidency.md): beside the forward pass the step gains, beside the replay it does not
int g_vgg_beside = -1;
thread_local int g_last_conv_co = 0;      // 1: the last conv_hx_try of this thread launched the co-resident instance

// does conv_hx_try run a launch of this geometry on one of the two tile variants that carry the fused max-pool epilogue (EP = 1)?
// (the same decisions as below, incl. the test override)
bool conv_hx_pool_ok(int N, int H, int W, int Cout) {
    const int bn = hx_pick_bn(Cout);
    const long wgs = (long)N * cdiv(W, 16) * cdiv(H, 16) * (round_up(Cout, bn) / bn);
    const int force_big = g_hx_big_override;
    if (bn == 128) return force_big >= 0 ? force_big == 1 : wgs >= 384;
    if (bn == 64) return force_big == 1 || wgs >= 384;
    return false;
}

bool conv_hx_s16_ok(int N, int H, int W, int Cout) { return (Cout & 31) == 0 && conv_hx_pool_ok(N, H, W, Cout); }

// does conv_fwd_launch hand this masked launch (the dgrad behind a tapped VGG19 map: mask + seed_ref) to conv_hx_try, whose masked instances (EP = 2 / 3: every tile variant)
// all sum ConvArgs.l1_acc?  The tests that make conv_hx_try pass a launch on (return 0) or that keep it off the masked whole-K epilogue; everything else it runs or refuses (-1).
bool conv_hx_l1_ok(const ConvArgs& a) {
    if (a.KS != 3 || !a.wq || (a.precision != PREC_BF16X3 && a.precision != PREC_BF16X1) || a.act == 1) return false;
    if (!a.mask || !a.seed_ref || a.accumulate || a.res || a.pool_out || a.skip_out || a.avgpool) return false;
    for (int s = 0; s < a.nsrc; s++) if ((a.src[s].ld & 3) || (a.src[s].sn & 3)) return false;
    return (long)a.H * a.W * a.out_ld < (1L << 30);
}

// will conv_fwd_launch hand this launch to k_conv_hx (the only forward kernel that applies ConvSrc.bn_* while staging its input)?
bool conv_src_lazy_ok(const ConvArgs& a) {
    if (a.KS != 3 || !a.wq || a.precision < PREC_F16X3 || a.precision > PREC_BF16X1 || a.act == 1) return false;
    for (int s = 0; s < a.nsrc; s++) if ((a.src[s].ld & 3) || (a.src[s].sn & 3)) return false;
    return true;
}
thread_local int g_last_conv_stats_tiles = 0;
thread_local int g_last_conv_direct = 0;

// would an average-pooled launch (ConvArgs.avgpool) of this split-f16 layer run here (latency kernel, or K-split tile launch + pooling slab reduce)?  `out` need not be set.
int conv_hx_avgpool_ok(const ConvArgs& a0) {
    ConvArgs a = a0;
    a.avgpool = 1;
    return conv_hx_try(a, nullptr, true) == 1 ? 1 : 0;
}

// 1 = handled.  Requirements: 3x3, split weights present (a.wq, packed for a.precision with rows padded to hx_pick_bn(Cout)).
int conv_hx_try(const ConvArgs& a0, hipStream_t st, bool dry) {
    ConvArgs a = a0;
    if (a.KS != 3 || !a.wq || a.precision < PREC_F16X3 || a.precision > PREC_BF16X1 || a.act == 1) return 0;      // (tanh: FinalBlocks, 3 output channels -- never an hx layer)
    int kq = 0;
    for (int s = 0; s < a.nsrc; s++) { if ((a.src[s].ld & 3) || (a.src[s].sn & 3)) return -1; kq += round_up(a.src[s].C, HX_KC); }
    a.Kq = kq;
    a.out_scale = (a.precision == PREC_F16X3 || a.precision == PREC_F16X1) ? 1.0f / HX_WSCALE : 1.0f;
    int bn = hx_pick_bn(a.Cout);
    a.Cout_pad = round_up(a.Cout, bn);      // (row padding of the packed weights: independent of the tile width chosen below)
    if (a.mask && a.accumulate) return -1;
    if (a.l1_acc && !conv_hx_l1_ok(a)) return -1;      // (the caller asks first: no launch may drop the sum it was given)
    if (a.pool_out && (a.accumulate || a.mask)) return -1;
    if (a.avgpool) {      // average-pooled result (the caller asked conv_avgpool_ok): the latency kernel's pooled epilogue, or -- below -- a K-split launch whose slab reduce pools
        if ((a.H | a.W) & 1 || a.accumulate || a.mask || a.pool_out || a.skip_out || a.stats || a.lstm || a.precision != PREC_F16X3 || a.in_s16 || a.out_s16) return dry ? 0 : -1;
        if (a.direct_ok && conv_direct_try(a, st, dry) == 1) {
            if (!dry) { g_last_conv_kernel = CK_HX_32; g_last_conv_stats_tiles = 0; g_last_conv_direct = 1; }
            return 1;
        }
    }
    if ((long)a.H * a.W * a.out_ld >= (1L << 30) || (a.res && (long)a.H * a.W * a.res_ld >= (1L << 30))) return 0;      // (the epilogue addresses one sample with 32-bit byte offsets)
    const int nchunks = kq / HX_KC;
    // under-filled wide layers (R's gate / SameBlock convolutions on 16x16 .. 32x32 maps, A, D's first stage at batch 8): 64-channel tiles on the same
    // 128-row packed weights -> twice the workgroups, two co-resident per CU hiding each other's barrier / LDS latencies (one 4-wave workgroup per CU
    // runs its serial chain of (tap, chunk) steps at ~30 % of the MFMA rate).  Measured, E/R/A/D step: 79.5 -> 78.2 ms, flat for thresholds 256 / 512 / 1024.
    if (bn == 128 && g_hx_big_override < 0 && !a.pool_out && !a.skip_out && !a.mask &&
        (long)a.N * cdiv(a.W, 16) * cdiv(a.H, 8) * (a.Cout_pad / 128) <= 256) bn = 64;
    // tiles: 128-channel layers -> 16x16 pixels x 128 channels on 8 waves with the 3-deep weight-tile ring when that fills the chip, else
    // 8x16 pixels on 4 waves (R's small feature maps); 16x16 x 64 / 32 channels for the narrower layers
    const int force_big = g_hx_big_override;                   // tests: 0 never, 1 always (128-channel layers)
    bool big = bn == 128 && (long)a.N * cdiv(a.W, 16) * cdiv(a.H, 16) * (a.Cout_pad / bn) >= 384;
    if (force_big >= 0) big = bn == 128 && force_big == 1;
    // narrower layers: 16x16-pixel tiles, or 8x16 when those would leave CUs idle (E / A on one time step's frames, R's side branches)
    const bool small_tiles = bn < 128 && force_big != 1 && (long)a.N * cdiv(a.W, 16) * cdiv(a.H, 16) * (a.Cout_pad / bn) < 384;      // (tests force the well-filled variants with 1)
    // inference launches (ConvArgs.direct_ok) and gradient launches whose 8x16 x 64-channel grid is under-filled (< 200 workgroups: it would be split over K): 4x16-pixel tiles -- twice the
    // workgroups from the pixel side, half the K slices and slabs (D's 128x128 layers of a batch-1 roll-out frame run unsplit: 256 workgroups of 18 - 36 steps, no slab
    // reduce).  Measured, roll-out: only where 4x16 tiles reach 200 workgroups 2012 -> 2067 frames/s, for every under-filled launch 2144.
    const long blocks8 = (long)a.N * cdiv(a.W, 16) * cdiv(a.H, 8) * (a.Cout_pad / bn);
    // The same for the under-filled split-bf16 launches of a training step (dgrads of E / A / R's small maps: fewer K slices = fewer atomics / slabs): E/R/A/D step
    // 66.73 / 66.79 -> 66.37 / 66.46 ms.  (Not the training FORWARD: a different K slicing changes its summation order, and the parity bounds of the closed-loop forward are
    // calibrated on the 8x16 form.)
    const bool th4 = bn == 64 && small_tiles && !a.pool_out && !a.skip_out && !a.mask && !a.stats && blocks8 < 200 &&
                     ((a.direct_ok && a.precision == PREC_F16X3 && !a.accumulate) || a.precision == PREC_BF16X3);
    const int th = th4 ? 4 : ((bn == 128 && !big) || small_tiles) ? 8 : 16;
    const int tx = cdiv(a.W, 16), ty = cdiv(a.H, th);
    const long blocks = (long)a.N * tx * ty * (a.Cout_pad / bn);
    // under-filled launches: split the channel chunks across blockIdx.z.  Accumulating launches (dgrad +=) combine with fp32 atomics; assigning
    // launches use the caller's slab scratch + the fixed-order k_split_reduce (bit-reproducible forward), as k_conv_fwd does.
    // latency-bound assigning launches (batch-1 roll-out): one launch without slabs on conv_direct.hip
    g_last_conv_direct = 0;
    if (!dry && !a.avgpool && a.direct_ok && blocks < 200 && conv_direct_try(a, st) == 1) { g_last_conv_kernel = CK_HX_32; g_last_conv_stats_tiles = 0; g_last_conv_direct = 1; return 1; }
    a.splitk = 1; a.split_stride = 0;
    bool det_accum = false;
    float* real_out = a.out; long real_sn = a.out_sn; int real_ld = a.out_ld; const float* real_bias = a.bias; const int real_act = a.act;
    const float* real_res = a.res;
    const long P = (long)a.N * a.H * a.W;
    if (blocks < 200 && nchunks >= 2 && !a.mask && !a.pool_out) {
        int want = (int)((512 + blocks - 1) / blocks);         // two workgroups per CU (inference launches, 256 / 384 / 768 / 1024: roll-out within 0.5 %)
        if (want > nchunks) want = nchunks;                     // a slice is at least one chunk (= one staged halo tile) x nine taps
        if (want > 16) want = 16;
        if (want >= 2) {
            const bool acc_ok = a.accumulate && a.act == 0 && !a.bias && !a.res;
            if (acc_ok && !a.deterministic) a.splitk = want;      // fp32 atomics in arrival order
            else if ((acc_ok || !a.accumulate) && a.split_scratch) {      // slabs + fixed-order reduce (deterministic mode: accumulating launches too; the reduce adds the old contents)
                const int ldc = round_up(a.Cout, 4);
                while (want >= 2 && (long)want * P * ldc > a.split_cap) want--;
                if (want >= 2) { a.splitk = want; a.split_stride = P * ldc; a.out = a.split_scratch; a.out_sn = (long)a.H * a.W * ldc; a.out_ld = ldc; a.bias = nullptr; a.act = 0; a.res = nullptr;
                                 det_accum = a.accumulate != 0; a.accumulate = 0; }
            }
        }
    }
    a.xcd_map = 1;
    // the co-resident instance, only where the 8-wave tile is picked today: split operands, and for the pooled / masked epilogues the whole-K assigning launches VGG19 makes
    static const int beside_env = []() { const char* e = getenv("CADDY_VGG_BESIDE"); return e ? atoi(e) : 1; }();
    const int beside = g_vgg_beside >= 0 ? g_vgg_beside : beside_env;
    const int co_io = (a.in_s16 ? 1 : 0) | ((a.out_s16 || a.pool_s16) ? 2 : 0);
    const int co_ep = (a.pool_out || a.skip_out) ? 1 : (a.mask ? 2 : 0);
    const bool co = big && ((beside & 4) || (beside & a.beside_chain & 3)) &&
                    ((a.precision == PREC_F16X3 && co_ep != 2) || (a.precision == PREC_BF16X3 && (co_ep == 2 || (co_ep == 0 && co_io < 2)))) &&
                    !(co_ep != 0 && (a.splitk > 1 || a.res || a.accumulate));
    g_last_conv_co = (co && !dry) ? 1 : 0;
    // BatchNorm partial sums: from the epilogue of EP = 0 instances when one workgroup holds the whole K range, from the slab reduce of a split launch otherwise
    float* const stats_req = a.stats; const int stats_req_ld = a.stats_ld;
    const long stats_cap = conv_stats_tiles_cap(a.N, a.H, a.W);                // tiles the caller sized the buffer for
    if (a.stats && (a.splitk != 1 || a.mask || a.pool_out || a.skip_out || a.precision == PREC_F16X1 || a.precision == PREC_BF16X1)) a.stats = nullptr;
    g_last_conv_stats_tiles = a.stats ? (int)((long)a.N * tx * ty) : 0;
    dim3 grid((unsigned)((long)a.N * tx * ty), a.Cout_pad / bn, a.splitk);
    // 4-wave variants: 3-deep register ring of weight tiles (with one step of prefetch the next tile has ~0.4 us to arrive from L2, less than its latency under load; measured,
    // E/R/A/D step: ring on launches of <= 256 / 512 / 1024 workgroups / always: 77.2 / 75.5 / 75.8 / 75.5 ms, batch-1 roll-out frame -3 %).  The single-product study
    // precisions (PREC_*X1, tools/bench_hx.py) keep one step of prefetch.
    // round 6: the under-filled variants with the weight fragments straight into registers (template parameter BG of k_conv_hx) -- split operands, plain epilogue, fp32 output.
    // g_hx_bg / CADDY_HX_BG: bit 0 the 4 x 16 x 64 tile, bit 1 8 x 16 x 64, bit 2 8 x 16 x 32 (tests and A/B runs; default all)
    static const int bg_env = []() { const char* e = getenv("CADDY_HX_BG"); return e ? atoi(e) : 7; }();
    // ... and only where a workgroup walks at least four 32-channel chunks: the nine-deep ring's prologue and the exchange of the partial tiles are pure overhead for the 1 - 2 chunks
    // of a K-split 64-channel layer (measured alone: E res 64 -> 64 @32 15.0 -> 15.9 us, R same 272 -> 128 @16 (8 K slices) 22.5 -> 23.6 us; 4+ chunks: -10 ... -25 %)
    const int bgm = (nchunks + a.splitk - 1) / a.splitk >= 4 || g_hx_bg >= 8 ? ((g_hx_bg >= 0 ? g_hx_bg : bg_env) & 7) : 0;
#define HX_LAUNCH(T_, NPL_, EP_, IO_)                                                                                             \
    do {                                                                                                                          \
        constexpr int D_ = NPL_ == 2 ? 3 : 1;                                                                                     \
        constexpr int BG_ = (NPL_ == 2 && EP_ == 0 && ((IO_) & 2) == 0) ? 1 : 0;                                                  \
        if (big && co) { if (conv_hx_co_launch(a, grid, tx, ty, EP_, IO_, st) != 1) return -1; }                                  \
        else if (big) hipLaunchKernelGGL((k_conv_hx<T_, NPL_, 16, 16, 128, 4, 2, 3, EP_, IO_>), grid, dim3(512), 0, st, a, tx, ty);    \
        else if (bn == 128) hipLaunchKernelGGL((k_conv_hx<T_, NPL_, 8, 16, 128, 2, 2, D_, EP_, IO_>), grid, dim3(256), 0, st, a, tx, ty);   \
        else if (th4) { if (bgm & 1) hipLaunchKernelGGL((k_conv_hx<T_, 2, 4, 16, 64, 2, 2, 3, 0, IO_, 1>), grid, dim3(256), 0, st, a, tx, ty);       /* (plain epilogue only) */ \
                        else hipLaunchKernelGGL((k_conv_hx<T_, 2, 4, 16, 64, 2, 2, 3, 0, IO_>), grid, dim3(256), 0, st, a, tx, ty); }   \
        else if (bn == 64 && small_tiles) { if ((bgm & 2) && BG_) hipLaunchKernelGGL((k_conv_hx<T_, NPL_, 8, 16, 64, 2, 2, D_, EP_, IO_, BG_>), grid, dim3(256), 0, st, a, tx, ty);   \
                                            else hipLaunchKernelGGL((k_conv_hx<T_, NPL_, 8, 16, 64, 2, 2, D_, EP_, IO_>), grid, dim3(256), 0, st, a, tx, ty); }   \
        else if (bn == 64) hipLaunchKernelGGL((k_conv_hx<T_, NPL_, 16, 16, 64, 4, 1, D_, EP_, IO_>), grid, dim3(256), 0, st, a, tx, ty);    \
        else if (small_tiles) { if ((bgm & 4) && BG_) hipLaunchKernelGGL((k_conv_hx<T_, NPL_, 8, 16, 32, 4, 1, D_, EP_, IO_, BG_>), grid, dim3(256), 0, st, a, tx, ty); \
                                else hipLaunchKernelGGL((k_conv_hx<T_, NPL_, 8, 16, 32, 4, 1, D_, EP_, IO_>), grid, dim3(256), 0, st, a, tx, ty); } \
        else hipLaunchKernelGGL((k_conv_hx<T_, NPL_, 16, 16, 32, 4, 1, D_, EP_, IO_>), grid, dim3(256), 0, st, a, tx, ty);                  \
    } while (0)
    if (a.avgpool && !a.split_stride) return dry ? 0 : -1;      // (a whole-K tile launch has no pooled epilogue)
    if (dry) return 1;
    const bool vgg_bwd = a.mask != nullptr;      // ReLU mask / L1 seed epilogue (VGG19 dgrad chain): split-bf16 instances with EP = 2
    const int io = (a.in_s16 ? 1 : 0) | ((a.out_s16 || a.pool_s16) ? 2 : 0);
    // round 6: a PRE-SPLIT input alone (the model's gradient tensors, written as S16-bf16 by their point-wise producers) is a property of the loader only: every split-bf16 tile
    // variant has such an instance, with the full plain epilogue (accumulate, K split, slabs) -- handled by the general launch below
    const bool ps_grad = io == 1 && a.precision == PREC_BF16X3 && !vgg_bwd && !a.pool_out && !a.skip_out;
    if (ps_grad && (a.nsrc != 1 || (a.src[0].C & 31) || a.src[0].bcast || a.src[0].bn_scale)) return -1;
    if (io && !ps_grad) {      // S16 tensors at the boundary: the two well-filled tile variants only (conv_hx_s16_ok), whole-K workgroups, plain or VGG19 epilogues
        const bool wide = big || (bn == 64 && !small_tiles);
        if (!wide || a.splitk != 1 || a.accumulate || a.res || a.stats || (a.precision != PREC_F16X3 && a.precision != PREC_BF16X3)) return -1;
        if (a.in_s16 && (a.nsrc != 1 || (a.src[0].C & 31) || a.src[0].bcast || a.src[0].bn_scale)) return -1;
        if ((a.out_s16 || a.pool_s16) && (a.Cout & 31)) return -1;
        if (a.pool_out && !a.skip_out && (a.out_s16 != 0) != (a.pool_s16 != 0)) return -1;      // one epilogue format per launch
        if (a.precision == PREC_BF16X3 && (a.pool_out || a.skip_out)) return -1;
        if (a.precision == PREC_F16X3 && vgg_bwd) return -1;
#define HX_IO_LAUNCH(T_, EP_)                                                                                                       \
        do {                                                                                                                       \
            if (big && co) { if (conv_hx_co_launch(a, grid, tx, ty, EP_, io, st) != 1) return -1; }                                \
            else if (big) { if (io == 1) hipLaunchKernelGGL((k_conv_hx<T_, 2, 16, 16, 128, 4, 2, 3, EP_, 1>), grid, dim3(512), 0, st, a, tx, ty);      \
                       else if (io == 2) hipLaunchKernelGGL((k_conv_hx<T_, 2, 16, 16, 128, 4, 2, 3, EP_, 2>), grid, dim3(512), 0, st, a, tx, ty); \
                       else hipLaunchKernelGGL((k_conv_hx<T_, 2, 16, 16, 128, 4, 2, 3, EP_, 3>), grid, dim3(512), 0, st, a, tx, ty); }            \
            else { constexpr int D_ = EP_ == 1 ? 1 : 3;      /* (ring depths of the plain instances) */                                  \
                   if (io == 1) hipLaunchKernelGGL((k_conv_hx<T_, 2, 16, 16, 64, 4, 1, D_, EP_, 1>), grid, dim3(256), 0, st, a, tx, ty);          \
                   else if (io == 2) hipLaunchKernelGGL((k_conv_hx<T_, 2, 16, 16, 64, 4, 1, D_, EP_, 2>), grid, dim3(256), 0, st, a, tx, ty);     \
                   else hipLaunchKernelGGL((k_conv_hx<T_, 2, 16, 16, 64, 4, 1, D_, EP_, 3>), grid, dim3(256), 0, st, a, tx, ty); }                \
        } while (0)
        if (a.precision == PREC_F16X3) { if (a.pool_out || a.skip_out) HX_IO_LAUNCH(_Float16, 1); else HX_IO_LAUNCH(_Float16, 0); }
        else if (vgg_bwd) HX_IO_LAUNCH(__bf16, 2);
        else { if (io != 1) return -1;      // (dgrad of a layer behind a max-pool: its output is the fp32 gradient of the pooled map)
               if (big && co) { if (conv_hx_co_launch(a, grid, tx, ty, 0, 1, st) != 1) return -1; }
               else if (big) hipLaunchKernelGGL((k_conv_hx<__bf16, 2, 16, 16, 128, 4, 2, 3, 0, 1>), grid, dim3(512), 0, st, a, tx, ty);
               else hipLaunchKernelGGL((k_conv_hx<__bf16, 2, 16, 16, 64, 4, 1, 3, 0, 1>), grid, dim3(256), 0, st, a, tx, ty); }
#undef HX_IO_LAUNCH
        g_last_conv_kernel = big ? CK_HX_128_8W : CK_HX_64;
        return 1;
    }
    if (a.mask_s16 || a.seed_s16) { if (!vgg_bwd) return -1; }
    if (a.pool_out || a.skip_out) {      // VGG19 layers in front of a max-pool: the two tile variants those layers run on (perceptual.hip asks only when this holds)
        if (a.precision != PREC_F16X3 || !(big || (bn == 64 && !small_tiles))) return -1;
        if (big && co) { if (conv_hx_co_launch(a, grid, tx, ty, 1, 0, st) != 1) return -1; }
        else if (big) hipLaunchKernelGGL((k_conv_hx<_Float16, 2, 16, 16, 128, 4, 2, 3, 1>), grid, dim3(512), 0, st, a, tx, ty);
        else hipLaunchKernelGGL((k_conv_hx<_Float16, 2, 16, 16, 64, 4, 1, 1, 1>), grid, dim3(256), 0, st, a, tx, ty);
        g_last_conv_kernel = big ? CK_HX_128_8W : CK_HX_64;
        return 1;
    }
    switch (a.precision) {
        case PREC_F16X3:
            if (vgg_bwd) return -1;      // (masks exist on the gradient side only)
            HX_LAUNCH(_Float16, 2, 0, 0);
            break;
        case PREC_BF16X3:
            if (vgg_bwd) HX_LAUNCH(__bf16, 2, 2, 0); else if (ps_grad) HX_LAUNCH(__bf16, 2, 0, 1); else HX_LAUNCH(__bf16, 2, 0, 0);
            break;
        case PREC_F16X1: HX_LAUNCH(_Float16, 1, 3, 0); break;
        default: HX_LAUNCH(__bf16, 1, 3, 0); break;
    }
#undef HX_LAUNCH
    g_last_conv_kernel = bn == 128 ? (big ? CK_HX_128_8W : CK_HX_128) : (bn == 64 ? CK_HX_64 : CK_HX_32);
    if (a.split_stride && a.lstm && !det_accum && real_act == 0 && !real_res && !stats_req && a.Cout == 4 * a.lstm->C && (a.lstm->C & 3) == 0 && (a.out_ld & 3) == 0)
        conv_split_reduce_lstm_launch(a.split_scratch, a.split_stride, a.splitk, a.out_ld, a.H * a.W, P, real_bias, *a.lstm, st);      // roll-out ConvLSTM cell: the reduce applies the cell update
    else if (a.split_stride && a.avgpool)
        conv_split_reduce_pool_launch(a.split_scratch, a.split_stride, a.splitk, a.out_ld, a.N, a.H, a.W, a.Cout, real_out, real_sn, real_ld, real_bias, real_act, real_res, a.res_sn, a.res_ld, st);
    else if (a.split_stride) conv_split_reduce_launch(a.split_scratch, a.split_stride, a.splitk, a.out_ld, a.H * a.W, P, a.Cout, real_out, real_sn, real_ld, real_bias, real_act, real_res, a.res_sn, a.res_ld, st,
                                                 stats_req, stats_req_ld, stats_cap, det_accum ? 1 : 0);
    return 1;
}

