"""Per-kernel parity cases of csrc/perceptual.hip and csrc/lpips.hip (the point-wise and reduction kernels around the VGG trunks), shared by tests/test_vgg_pointwise_emu.py
(host simulator) and tests/test_vgg_pointwise_gpu.py (MI355X).  Every case takes (lib, dev) and goes through the caddy_k_vgg_* / caddy_k_lpips_* entry points, which use the
drivers' own dispatch (launch_feat_l1, launch_maxpool_bwd, lpips_head_launch, grid_for, cos_blocks, ...): the flag-to-instance mapping is part of what is tested.

Reference: a restatement written here, in float64 or as exact selection logic, on the float32 values the kernel sees.  An S16 operand (csrc/common.h: 16-bit hi | lo halves per 32
channels) is uploaded as kernel_cases.s16_encode(v) of values v that the split represents exactly (q() below; asserted through s16_decode), so one reference serves every format
instance of a kernel.

Output hygiene: Out() puts GUARD elements in front of and behind every output; assigned outputs start as NaN, accumulating ones from a non-zero value; guards() is called by
every case.

Bounds (fixed before the first run; every case prints the figure it saw, run with -s):

  exact      selections, copies, L1 seeds, S16 encodings, k_lpips_finalize: torch.equal / bitwise.
  sums       k_feat_l1, k_feat_l1_img and the three sums of k_feat_cos_img accumulate float64 over terms that the restatement forms exactly as the kernel does (|r - g| in float32;
             products of float32 values are exact in float64) and adds without error (math.fsum).  Only the kernel's own additions round: fewer than n of them for n terms, each by
             at most 2**-53 of a partial sum that is at most base + sum|term| (base: what the accumulator held), so |error| <= n * 2**-53 * (base + sum|term|).
  cosine     per level 4 * n_l * 2**-53 + 1e-15 (three such sums through two square roots, a product and a division); the output is the mean of five levels, at most
             mean_l(4 * n_l * 2**-53) + 1e-15, and another 8 * 2**-53 for the four additions and the division of values <= 1.
  staging    k_metric_stage, k_lpips_stage, k_gt_resize against the float64 restatement with the kernel's float32 constants widened: 8 * 2**-24 * max(1, |v|) (at most four
             rounded operations, the early ones amplified by the final division by at most 1 / 0.448).
  lpips head lpips_cases.check_levels' rule: relative, 8 x the spread between the float32 and the float64 restatement of the same case, floor 1e-6; the spread comes from the
             restatement alone and is asserted to stay below 1e-5 (head_reference), so the rule cannot quietly widen.

Instance -> case (each runs on both backends; T / F = S16 / fp32 operand):

  k_maxpool2                       maxpool_case                    POOL_SHAPES
  k_maxpool2_bwd_relu<AS,ZS>       maxpool_bwd_case(a_s16, z_s16)  4 instances x POOL_BWD_SHAPES
  k_feat_l1<RS,GS,ZS>              feat_l1_case(rs, gs, zs)        8 instances at (2,5,7,64); gz == nullptr: feat_l1_case(zs=None) -> <RS,GS,false>
  k_feat_l1<F,F,F> second trip     feat_l1_two_trip_case           (1,258,256,64)
  k_feat_l1_img<RS,GS>             feat_l1_img_case(rs, gs)        4 instances x IMG_SHAPES
  k_feat_cos_img<RS,GS>            feat_cos_case(rs, gs, cfg)      4 instances x COS_CONFIGS, with k_feat_cos_finalize
  k_metric_stage, k_lpips_stage    stage_case(which)               STAGE_SHAPES x range 1, 255
  k_gt_resize                      gt_resize_case                  f = 1, 2, 4 x ld = 4, 12 x GT_TIMES
  k_time_chunk, k_copy_f           time_chunk_case, copy_f_case
  k_lpips_head<NK,S0,S1>           lpips_head_case(C, s0, s1)      C = 64 NK, 16 instances x HEAD_NPIX x blocks
  k_lpips_finalize                 lpips_finalize_case(nf)         nf = 3, 70

Largest error / allowed seen per case group (every check prints its own figure; the simulator and the MI355X gave the same figures to the digits shown):

    group          simulator   MI355X
    feat_l1        0           0          (also the two-trip case: float32 terms of this size add exactly in float64)
    feat_l1_img    0           0
    feat_cos_sums  0.004       0.004      (the partial sums of k_feat_cos_img)
    feat_cos       0.001       0.001      (the output of k_feat_cos_finalize)
    metric_stage   0.185       0.185      ((2,33,31), range 255)
    lpips_stage    0.447       0.447      ((2,33,31), range 255)
    gt_resize      0.218       0.218      (f = 4, ld = 12)
    lpips_head     0.100       0.100      (error 1.0e-7 against the floor 1e-6; the restatement's spread is 6e-9 .. 1e-7 on these inputs)

Found by lpips_finalize_case on the MI355X (nf = 70): the compiler fused the last level's `s *= inv_px; total += s` into one multiply-add, so the total was not the sum of the level
values the kernel stores (one unit in the last place, and not what the simulator computes).  k_lpips_finalize now compiles with contraction off.
"""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from playablevideogeneration_amd import _lib as L
from playablevideogeneration_amd._lib import TV
from tests.kernel_cases import P, s16_decode, s16_encode, stream, sync

U53, U24 = 2.0 ** -53, 2.0 ** -24
GUARD = 64            # elements in front of and behind every output (a multiple of the 16-byte access width)
GUARD_F = -123.5      # their content
WORST = {}            # group -> largest error / allowed seen by this process


def f32(x):
    return float(np.float32(x))


def declare(lib):
    V, I, Lg, Fl = C.c_void_p, C.c_int, C.c_long, C.c_float
    lib.caddy_k_vgg_maxpool2.argtypes = [V, V, I, I, I, I, V]
    lib.caddy_k_vgg_maxpool2_bwd_relu.argtypes = [V, I, V, V, I, I, I, I, I, V]
    lib.caddy_k_vgg_feat_l1.argtypes = [V, I, V, I, I, I, I, I, Fl, V, I, V, V]
    lib.caddy_k_vgg_feat_l1_img.argtypes = [V, I, V, I, I, I, I, I, V, V]
    lib.caddy_k_vgg_cos_blocks.argtypes = [I, I, I]
    lib.caddy_k_vgg_feat_cos.argtypes = [V, I, V, Lg, V, V]
    lib.caddy_k_vgg_metric_stage.argtypes = [V, V, I, I, I, Fl, V]
    lib.caddy_k_vgg_gt_resize.argtypes = [V, V, I, I, I, I, I, I, I, V]
    lib.caddy_k_vgg_time_chunk.argtypes = [V, V, I, I, Lg, I, I, I, V]
    lib.caddy_k_vgg_copy_f.argtypes = [V, V, Lg, V]
    lib.caddy_k_lpips_blocks.argtypes = [I]
    lib.caddy_k_lpips_stage.argtypes = [V, V, I, I, I, Fl, V]
    lib.caddy_k_lpips_head.argtypes = [V, I, V, I, V, I, I, I, I, V, V]
    lib.caddy_k_lpips_finalize.argtypes = [V, V, Lg, I, V, I, V]
    return lib


def check_structs(lib):
    L.check_head_structs(lib)


class Out:
    """an output buffer of n elements with GUARD elements on both sides; .t is the view of the n elements, .p the pointer to hand to the kernel"""

    def __init__(self, n, dev, fill=float("nan"), dtype=torch.float32):
        host = torch.full((n + 2 * GUARD,), GUARD_F, dtype=dtype)
        if torch.is_tensor(fill):
            host[GUARD:GUARD + n] = fill.reshape(-1).to(dtype)
        else:
            host[GUARD:GUARD + n] = fill
        self.n, self.buf = n, host.to(dev)
        self.t = self.buf[GUARD:GUARD + n]
        self.p = C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def cpu(self):
        return self.t.cpu()

    def guards(self, name):
        b = self.buf.cpu()
        g = torch.full((GUARD,), GUARD_F, dtype=b.dtype)
        assert torch.equal(b[:GUARD], g) and torch.equal(b[GUARD + self.n:], g), f"{name}: guard elements changed"


def record(group, name, err, tol):
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    print(f"[{group}] {name}: error {err:.3e}  allowed {tol:.3e}  ratio {ratio:.3f}")
    assert err <= tol, f"{group} {name}: error {err:.3e} > allowed {tol:.3e}"


def bits(t):
    return t.contiguous().view(torch.int32)


def q(x):
    """x -> the nearest values an S16-f16 tensor holds exactly (hi = f16(x), lo = f16(x - hi), value hi + lo); a plain fp32 operand can hold them too"""
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return hi.float() + lo.float()


def upload(v, s16, dev):
    """(N,H,W,C) float32 values -> device buffer in the asked format; the S16 form must decode to exactly these values"""
    if not s16:
        return v.contiguous().to(dev)
    raw = s16_encode(v, torch.float16)
    hi, lo = s16_decode(raw, v.shape[-1], torch.float16)
    assert torch.equal(hi.float() + lo.float(), v), "test input not representable as an S16-f16 tensor"
    return raw.to(dev)


def fsum(t):
    return math.fsum(t.double().reshape(-1).tolist())


# ====================================================================================================================================================================================
# k_maxpool2, k_maxpool2_bwd_relu
# ====================================================================================================================================================================================
POOL_SHAPES = [(2, 6, 8, 64), (1, 7, 9, 64), (2, 5, 5, 128)]
POOL_BWD_SHAPES = [(2, 6, 8, 64), (1, 7, 9, 64)]
WIN = [(0, 0), (0, 1), (1, 0), (1, 1)]      # scan order of a window


def maxpool_case(lib, dev, shape, seed=0):
    """bit-equal to the maximum of the four window positions (and to F.max_pool2d); the uncovered last row / column of an odd size holds 1e30 and must not be read"""
    declare(lib)
    N, H, W, Cc = shape
    Ho, Wo = H // 2, W // 2
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(N, H, W, Cc, generator=g)
    x[:, 2 * Ho:] = 1e30
    x[:, :, 2 * Wo:] = 1e30
    want = x[:, 0:2 * Ho:2, 0:2 * Wo:2]
    for dy, dx in WIN[1:]:
        want = torch.maximum(want, x[:, dy:2 * Ho:2, dx:2 * Wo:2])
    assert torch.equal(want, F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
    xd = x.to(dev)
    out = Out(N * Ho * Wo * Cc, dev)
    assert lib.caddy_k_vgg_maxpool2(P(xd), out.p, N, H, W, Cc, stream(dev)) == 0
    sync(dev)
    assert torch.equal(out.cpu().reshape(N, Ho, Wo, Cc), want), "k_maxpool2"
    out.guards("k_maxpool2")
    assert torch.equal(xd.cpu(), x)


def pool_bwd_rule(a, gp):
    """gz[pos] = gp[window] where pos is the window's first maximum in scan order (strict >) and that maximum is > 0; else 0, also in the uncovered row / column"""
    N, H, W, Cc = a.shape
    Ho, Wo = H // 2, W // 2
    w = [a[:, dy:2 * Ho:2, dx:2 * Wo:2] for dy, dx in WIN]
    m, k = w[0].clone(), torch.zeros(N, Ho, Wo, Cc, dtype=torch.long)
    for j in (1, 2, 3):
        better = w[j] > m
        m = torch.where(better, w[j], m)
        k = torch.where(better, torch.full_like(k, j), k)
    v = torch.where(m > 0, gp, torch.zeros_like(gp))
    gz = torch.zeros_like(a)
    for j, (dy, dx) in enumerate(WIN):
        gz[:, dy:2 * Ho:2, dx:2 * Wo:2] = torch.where(k == j, v, torch.zeros_like(v))
    return gz, k


def maxpool_bwd_case(lib, dev, shape, a_s16, z_s16, seed=0):
    """Planted in window (0, 0) of image 0, one channel each: the maximum at each of the four positions (channels 0-3); all four equal and positive (4: position 0); positions
    1, 2, 3 tied above position 0 (5: position 1); all negative (6: zero); maximum exactly 0 (7, 8: zero, the check is > 0).  A quarter of the other values is exactly 0."""
    declare(lib)
    N, H, W, Cc = shape
    Ho, Wo = H // 2, W // 2
    g = torch.Generator().manual_seed(200 + seed)
    a = torch.randn(N, H, W, Cc, generator=g)
    a[torch.rand(N, H, W, Cc, generator=g) < 0.25] = 0.0
    a = q(a)
    planted = {4: [1.5, 1.5, 1.5, 1.5], 5: [1.0, 3.0, 3.0, 3.0], 6: [-1.0, -2.0, -0.5, -3.0], 7: [0.0, -1.0, -2.0, -0.5], 8: [-1.0, 0.0, 0.0, -2.0]}
    for kmax in range(4):
        planted[kmax] = [2.0 if j == kmax else 0.5 ** (1 + j) for j in range(4)]
    for ch, vals in planted.items():
        for (dy, dx), v in zip(WIN, vals):
            a[0, dy, dx, ch] = v
    gp = torch.randn(N, Ho, Wo, Cc, generator=g)
    want, k = pool_bwd_rule(a, gp)
    # the planted windows do what they were planted for
    assert k[0, 0, 0, :9].tolist() == [0, 1, 2, 3, 0, 1, 2, 0, 1]
    for ch in range(9):
        hit = want[0, :2, :2, ch].reshape(-1)
        if ch <= 5:
            assert hit[k[0, 0, 0, ch]] == gp[0, 0, 0, ch] and (hit != 0).sum() == 1
        else:
            assert (hit == 0).all()
    # torch's own rule (float64 autograd of max_pool2d(relu(a), 2)): the same routing
    x = a.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(torch.relu(x), 2).backward(gp.double().permute(0, 3, 1, 2))
    auto = x.grad.permute(0, 2, 3, 1)
    assert torch.equal(auto, want.double()), "the restated rule differs from torch's autograd"

    ad, gpd = upload(a, a_s16, dev), gp.to(dev)
    gz = Out(a.numel(), dev)
    assert lib.caddy_k_vgg_maxpool2_bwd_relu(P(ad), int(a_s16), P(gpd), gz.p, int(z_s16), N, H, W, Cc, stream(dev)) == 0
    sync(dev)
    got = gz.cpu().reshape(N, H, W, Cc)
    name = f"k_maxpool2_bwd_relu<{int(a_s16)},{int(z_s16)}> {shape}"
    if z_s16:
        assert torch.equal(bits(got), bits(s16_encode(want, torch.bfloat16))), name + ": S16-bf16 gradient"
    else:
        assert not torch.isnan(got).any(), name + ": a position was not assigned"
        assert torch.equal(got, want), name
        assert torch.equal(got.double(), auto), name + " against autograd"
    gz.guards(name)


# ====================================================================================================================================================================================
# k_feat_l1, k_feat_l1_img
# ====================================================================================================================================================================================
L1_SHAPE = (2, 5, 7, 64)
L1_TWO_TRIP_SHAPE = (1, 258, 256, 64)      # 1,056,768 float4 > 4096 x 256 (grid_for's cap): the grid-stride loop of some workgroups runs twice
IMG_SHAPES = [(3, 3, 5, 64), (2, 64, 65, 64)]      # n4 = 240 < 1024: one block; n4 / 1024 = 65: capped at 64 blocks
SEED_W = f32(0.37)
ACC0 = 3.25


def l1_inputs(shape, seed, planted=True):
    N, H, W, Cc = shape
    g = torch.Generator().manual_seed(300 + seed)
    rec, gt = q(torch.randn(shape, generator=g)), q(torch.relu(torch.randn(shape, generator=g)))
    if planted:
        rec, gt = rec.reshape(-1), gt.reshape(-1)
        idx = torch.randperm(rec.numel(), generator=g)
        same = idx[:40][rec[idx[:40]] > 0]
        gt[same] = rec[same]                                  # rec == gt at positive rec: seed 0
        rec[idx[40:60]] = 0.0                                 # rec == 0 exactly: seed 0, |gt| counted
        neg = idx[60:80]
        rec[neg] = -rec[neg].abs() - 0.125                    # rec < 0, rec != gt: seed 0, the difference counted
        assert same.numel() >= 5 and (gt[idx[40:60]] > 0).any() and (rec[neg] != gt[neg]).all()
        rec, gt = rec.reshape(shape), gt.reshape(shape)
    return rec, gt


def l1_seed(rec, gt):
    d = rec - gt      # float32, as the kernel forms it
    z = torch.where(d > 0, torch.full_like(d, SEED_W), torch.where(d < 0, torch.full_like(d, -SEED_W), torch.zeros_like(d)))
    return torch.where(rec > 0, z, torch.zeros_like(d))


def feat_l1_case(lib, dev, rs, gs, zs, shape=L1_SHAPE, seed=0, planted=True):
    """zs None: gz == nullptr (sum only).  Largest error seen: 0 on the simulator and on the MI355X, at (2,5,7,64) (allowed 2.4e-10) and at the two-trip shape (allowed 1.9e-3)"""
    declare(lib)
    N, H, W, Cc = shape
    rec, gt = l1_inputs(shape, seed, planted)
    terms = (rec - gt).abs()      # float32
    want_sum, n = fsum(terms), terms.numel()
    recd, gtd = upload(rec, rs, dev), upload(gt, gs, dev)
    acc = Out(1, dev, fill=ACC0, dtype=torch.float64)
    gz = Out(rec.numel(), dev) if zs is not None else None
    rc = lib.caddy_k_vgg_feat_l1(P(recd), int(rs), P(gtd), int(gs), N, H, W, Cc, SEED_W, gz.p if gz else None, int(bool(zs)), acc.p, stream(dev))
    assert rc == 0
    sync(dev)
    name = f"k_feat_l1<{int(rs)},{int(gs)},{'-' if zs is None else int(zs)}> {shape}"
    record("feat_l1", name, abs(acc.cpu().item() - (ACC0 + want_sum)), n * U53 * (ACC0 + want_sum))
    acc.guards(name)
    if gz:
        want = l1_seed(rec, gt)
        got = gz.cpu().reshape(shape)
        if zs:
            assert torch.equal(bits(got), bits(s16_encode(want, torch.bfloat16))), name + ": S16-bf16 seed"
        else:
            assert torch.equal(got, want), name + ": seed"
        gz.guards(name)


def feat_l1_img_case(lib, dev, rs, gs, shape, seed=0):
    """per-image sums onto pre-loaded accumulators; image n's differences are scaled by n + 1, so a wrong image offset shows"""
    declare(lib)
    N, H, W, Cc = shape
    g = torch.Generator().manual_seed(400 + seed)
    rec = torch.randn(shape, generator=g)
    gt = rec + torch.randn(shape, generator=g) * (1 + torch.arange(N, dtype=torch.float32)).reshape(N, 1, 1, 1)
    rec, gt = q(rec), q(gt)
    terms = (rec - gt).abs()
    base = [ACC0 + 2 * i for i in range(N)]
    recd, gtd = upload(rec, rs, dev), upload(gt, gs, dev)
    acc = Out(N, dev, fill=torch.tensor(base, dtype=torch.float64), dtype=torch.float64)
    assert lib.caddy_k_vgg_feat_l1_img(P(recd), int(rs), P(gtd), int(gs), N, H, W, Cc, acc.p, stream(dev)) == 0
    sync(dev)
    got = acc.cpu().tolist()
    for i in range(N):
        s = fsum(terms[i])
        record("feat_l1_img", f"k_feat_l1_img<{int(rs)},{int(gs)}> {shape} image {i}", abs(got[i] - (base[i] + s)), terms[i].numel() * U53 * (base[i] + s))
    acc.guards("k_feat_l1_img")


# ====================================================================================================================================================================================
# k_feat_cos_img + k_feat_cos_finalize
# ====================================================================================================================================================================================
VggCosArgs = L.VggCosArgs
COS_CONFIGS = {
    # nf, (H, W, C) of the five levels
    "maps": (3, [(3, 5, 64), (64, 65, 64), (2, 3, 128), (1, 2, 256), (1, 1, 512)]),      # one block; the 64-block cap; one block each
    "frames": (70, [(3, 5, 64), (2, 2, 128), (1, 3, 256), (1, 1, 512), (1, 1, 512)]),    # two blocks of the finaliser
}


def cos_blocks(H, W, Cc):
    return min(max(H * W * (Cc // 4) // 1024, 1), 64)


def feat_cos_case(lib, dev, rs, gs, cfg):
    """out[n] = mean over the five levels of x.y / (max(|x|, 1e-6) * max(|y|, 1e-6)): every level contributes a fifth.  Planted per (frame, level), counted from the last frame:
    x all zero (cosine 0, not NaN); x of norm ~2e-7 against an ordinary y (the clamp of |x| alone is active); x == y; y == -x.
    Largest error / allowed seen (simulator and MI355X alike): 0.004 for the partial sums, 0.001 for the output."""
    declare(lib)
    nf, levels = COS_CONFIGS[cfg]
    g = torch.Generator().manual_seed(500 + nf)
    xs, ys = [], []
    for H, W, Cc in levels:
        x = torch.relu(torch.randn(nf, H, W, Cc, generator=g))
        xs.append(x)
        ys.append(torch.relu(x + 0.5 * torch.randn(nf, H, W, Cc, generator=g)))
    last = nf - 1
    xs[0][last] = 0.0
    tiny = torch.zeros(levels[2][0] * levels[2][1] * levels[2][2])
    tiny[::37] = 2.0 ** -24 * (1 + torch.arange(tiny[::37].numel()) % 3)
    xs[2][last - 1] = tiny.reshape(levels[2])
    ys[2][last - 1] += 0.5
    ys[1][last - 2] = xs[1][last - 2]
    ys[3][last - 1] = -xs[3][last - 1]
    xs, ys = [q(x) for x in xs], [q(y) for y in ys]
    assert 0 < xs[2][last - 1].double().pow(2).sum().sqrt().item() < 1e-6 < xs[2][last - 1].double().pow(2).sum().sqrt().item() * ys[2][last - 1].double().pow(2).sum().sqrt().item()

    xd, yd = [upload(x, rs, dev) for x in xs], [upload(y, gs, dev) for y in ys]
    a = VggCosArgs()
    blocks, off, total = [], [], 0
    for l, (H, W, Cc) in enumerate(levels):
        a.x[l], a.y[l], a.x_s16[l], a.y_s16[l], a.H[l], a.W[l], a.C[l] = xd[l].data_ptr(), yd[l].data_ptr(), int(rs), int(gs), H, W, Cc
        blocks.append(cos_blocks(H, W, Cc))
        assert lib.caddy_k_vgg_cos_blocks(H, W, Cc) == blocks[l]
        off.append(total)
        total += nf * blocks[l] * 3
    if cfg == "maps":
        assert blocks == [1, 64, 1, 1, 1]
    part, out = Out(total, dev, dtype=torch.float64), Out(nf, dev, dtype=torch.float64)
    assert lib.caddy_k_vgg_feat_cos(C.byref(a), nf, part.p, total, out.p, stream(dev)) == 0
    sync(dev)
    name = f"k_feat_cos_img<{int(rs)},{int(gs)}> {cfg}"
    pt, got = part.cpu(), out.cpu()
    assert not torch.isnan(pt).any() and not torch.isnan(got).any(), name + ": NaN"
    want = [0.0] * nf
    tol = [0.0] * nf
    cos_nl = {}
    for l in range(5):
        x, y = xs[l].double().reshape(nf, -1), ys[l].double().reshape(nf, -1)
        n_l = x.shape[1]
        p = pt[off[l]:off[l] + nf * blocks[l] * 3].reshape(nf, blocks[l], 3)
        for n in range(nf):
            t = [x[n] * y[n], x[n] * x[n], y[n] * y[n]]      # exact products
            s = [fsum(v) for v in t]
            for j, what in enumerate(("x.y", "|x|^2", "|y|^2")):      # the partials of frame n, level l: part[off_l + (n * blocks_l + b) * 3 + j]
                err = abs(math.fsum(p[n, :, j].tolist()) - s[j])
                bound = n_l * U53 * fsum(t[j].abs())
                WORST["feat_cos_sums"] = max(WORST.get("feat_cos_sums", 0.0), err / bound if bound else (0.0 if err == 0 else float("inf")))
                assert err <= bound, f"{name}: {what} of frame {n}, level {l}: error {err:.3e} > allowed {bound:.3e}"
            cos_nl[n, l] = s[0] / (max(math.sqrt(s[1]), 1e-6) * max(math.sqrt(s[2]), 1e-6))
            want[n] += cos_nl[n, l] / 5.0
            tol[n] += 4 * n_l * U53 / 5.0
    assert cos_nl[last, 0] == 0.0 and abs(cos_nl[last - 2, 1] - 1.0) < 1e-12 and abs(cos_nl[last - 1, 3] + 1.0) < 1e-12 and 0 < abs(cos_nl[last - 1, 2]) < 1
    worst = max(abs(got[n].item() - want[n]) / (tol[n] + 1e-15 + 8 * U53) for n in range(nf))
    WORST["feat_cos"] = max(WORST.get("feat_cos", 0.0), worst)
    print(f"[feat_cos] {name}: largest error / allowed {worst:.3f} (sums {WORST['feat_cos_sums']:.3f})")
    for n in range(nf):
        assert abs(got[n].item() - want[n]) <= tol[n] + 1e-15 + 8 * U53, f"{name}: frame {n}: {got[n].item()!r} against {want[n]!r}"
    part.guards(name)
    out.guards(name)


# ====================================================================================================================================================================================
# k_metric_stage, k_lpips_stage, k_gt_resize
# ====================================================================================================================================================================================
STAGE_SHAPES = [(3, 5, 7), (2, 33, 31)]      # (N, H, W): one block; 2046 pixels, more than one block


def stage_case(lib, dev, which, shape, rng, seed=0):
    """(N, 3, H, W) in [0, range], with exact 0 and exact range among the values -> NHWC of pitch 4, the fourth channel exactly 0.
    metric: (v / range - 0.5) / f32(0.5 + 1e-6); lpips: ((2 v / range - 1) - shift_c) / scale_c.  Largest error / allowed seen (simulator and MI355X alike): metric 0.185,
    lpips 0.447, both at (2,33,31) with range 255."""
    declare(lib)
    N, H, W = shape
    rng = f32(rng)
    g = torch.Generator().manual_seed(600 + seed)
    src = torch.rand(N, 3, H, W, generator=g) * rng
    src.reshape(-1)[::11] = 0.0
    src.reshape(-1)[5::13] = rng
    s = src.double()
    if which == "metric":
        want = (s / rng - 0.5) / f32(0.5 + 1e-6)
        fn = lib.caddy_k_vgg_metric_stage
    else:
        shift = torch.tensor([f32(-.030), f32(-.088), f32(-.188)], dtype=torch.float64).reshape(1, 3, 1, 1)
        scale = torch.tensor([f32(.458), f32(.448), f32(.450)], dtype=torch.float64).reshape(1, 3, 1, 1)
        want = ((2.0 * s / rng - 1.0) - shift) / scale
        fn = lib.caddy_k_lpips_stage
    sd = src.to(dev)
    out = Out(N * H * W * 4, dev)
    assert fn(P(sd), out.p, N, H, W, rng, stream(dev)) == 0
    sync(dev)
    got = out.cpu().reshape(N, H, W, 4)
    assert torch.equal(got[..., 3], torch.zeros(N, H, W)), which + " stage: pad channel"
    want = want.permute(0, 2, 3, 1)
    ratio = ((got[..., :3].double() - want).abs() / (8 * U24 * want.abs().clamp(min=1.0))).max().item()
    record(which + "_stage", f"{shape} range {rng}", ratio, 1.0)
    out.guards(which + " stage")


GT_SIZES = {1: (5, 6), 2: (6, 5), 4: (3, 4)}      # f -> output (Ho, Wo); the observations are f times as large
GT_TIMES = [(2, 0), (3, 1)]                       # (Trec, t_off) with Tobs = 4


def gt_resize_case(lib, dev, f, ld, Trec, t_off, B=2, Tobs=4, seed=0):
    """first 3 of ld channels of observation (b, t + t_off), resized like float64 F.interpolate(scale_factor=1/f, bilinear, align_corners=False); frame k holds values around 4 k, so
    a wrong frame shows; the other channels hold 1e30.  Largest error / allowed seen (simulator and MI355X alike): 0.218 at f = 4, ld = 12."""
    declare(lib)
    Ho, Wo = GT_SIZES[f]
    Hi, Wi = f * Ho, f * Wo
    g = torch.Generator().manual_seed(700 + seed)
    frames = torch.rand(B * Tobs, Hi, Wi, 3, generator=g) * 2 - 1 + 4.0 * torch.arange(B * Tobs, dtype=torch.float32).reshape(-1, 1, 1, 1)
    obs = torch.full((B * Tobs, Hi, Wi, ld), 1e30)
    obs[..., :3] = frames
    sel = frames.reshape(B, Tobs, Hi, Wi, 3)[:, t_off:t_off + Trec].reshape(B * Trec, Hi, Wi, 3).permute(0, 3, 1, 2).double()
    want = F.interpolate(sel, scale_factor=1.0 / f, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert want.shape == (B * Trec, Ho, Wo, 3)
    od = obs.to(dev)
    tv = TV(od.data_ptr(), B * Tobs, Hi, Wi, 3, Hi * Wi * ld, ld)
    out = Out(B * Trec * Ho * Wo * 4, dev)
    assert lib.caddy_k_vgg_gt_resize(C.byref(tv), out.p, Ho, Wo, B, Tobs, Trec, t_off, f, stream(dev)) == 0
    sync(dev)
    got = out.cpu().reshape(B * Trec, Ho, Wo, 4)
    assert torch.equal(got[..., 3], torch.zeros(B * Trec, Ho, Wo)), "k_gt_resize: pad lane"
    ratio = ((got[..., :3].double() - want).abs() / (8 * U24 * want.abs().clamp(min=1.0))).max().item()
    record("gt_resize", f"f={f} ld={ld} Trec={Trec} t_off={t_off}", ratio, 1.0)
    out.guards("k_gt_resize")


# ====================================================================================================================================================================================
# k_time_chunk, k_copy_f
# ====================================================================================================================================================================================
CHUNKS = [(0, 2), (2, 3), (4, 1)]      # (t0, len) with Tfull = 5


def time_chunk_case(lib, dev, t0, ln, B=3, Tfull=5, F4=7, seed=0):
    """gather: chunk[b, j] = full[b, t0 + j]; add: full[b, t0 + j] += chunk[b, j] on a non-zero `full`, every other element of `full` untouched.  Exact."""
    declare(lib)
    g = torch.Generator().manual_seed(800 + seed)
    full = torch.randn(B, Tfull, F4 * 4, generator=g)
    fd = Out(full.numel(), dev, fill=full)
    chunk = Out(B * ln * F4 * 4, dev)
    assert lib.caddy_k_vgg_time_chunk(fd.p, chunk.p, B, Tfull, F4, t0, ln, 0, stream(dev)) == 0
    sync(dev)
    assert torch.equal(chunk.cpu().reshape(B, ln, F4 * 4), full[:, t0:t0 + ln]), "k_time_chunk gather"
    assert torch.equal(fd.cpu().reshape(full.shape), full), "k_time_chunk gather changed `full`"
    chunk.guards("k_time_chunk gather")
    fd.guards("k_time_chunk gather")
    add = torch.randn(B, ln, F4 * 4, generator=g)
    cd = Out(add.numel(), dev, fill=add)
    assert lib.caddy_k_vgg_time_chunk(fd.p, cd.p, B, Tfull, F4, t0, ln, 1, stream(dev)) == 0
    sync(dev)
    want = full.clone()
    want[:, t0:t0 + ln] += add
    assert torch.equal(bits(fd.cpu().reshape(full.shape)), bits(want)), "k_time_chunk add"
    assert torch.equal(cd.cpu().reshape(add.shape), add), "k_time_chunk add changed the chunk"
    fd.guards("k_time_chunk add")
    cd.guards("k_time_chunk add")


def copy_f_case(lib, dev, n=1000):
    declare(lib)
    src = torch.randn(n, generator=torch.Generator().manual_seed(900))
    sd, dst = src.to(dev), Out(n, dev)
    assert lib.caddy_k_vgg_copy_f(P(sd), dst.p, n, stream(dev)) == 0
    sync(dev)
    assert torch.equal(bits(dst.cpu()), bits(src)), "k_copy_f"
    dst.guards("k_copy_f")


# ====================================================================================================================================================================================
# k_lpips_head, k_lpips_finalize
# ====================================================================================================================================================================================
HEAD_NPIX = [1, 16, 23, 70]
HEAD_NF = 3
EPS_N = f32(1e-10)


def lpips_blocks(npix):
    return min(max((npix + 15) // 16, 1), 128)


def head_inputs(Cc, npix, seed=0):
    """ReLU outputs of randn scale, f1 = relu(z + 0.2 noise).  Planted: frame 0 pixel 0 all zero in f0 only; frame 1 last pixel all zero in both, and (npix > 1) pixel 0 of norm
    ~1e-5 in f0 (multiples of 2**-24: the 1e-10 under the norm matters there); frame 2 pixel npix // 2 equal in both.  Weights in [0, 1), a tenth zero, a tenth negative."""
    g = torch.Generator().manual_seed(1000 + 10 * Cc + npix + seed)
    z = torch.randn(HEAD_NF, npix, Cc, generator=g)
    f0, f1 = torch.relu(z), torch.relu(z + 0.2 * torch.randn(HEAD_NF, npix, Cc, generator=g))
    f0[0, 0] = 0.0
    f0[1, npix - 1] = 0.0
    f1[1, npix - 1] = 0.0
    if npix > 1:
        f0[1, 0] = 2.0 ** -24 * torch.randint(0, 16, (Cc,), generator=g)
    f1[2, npix // 2] = f0[2, npix // 2]
    w = torch.rand(Cc, generator=g)
    w[1::10] = 0.0
    w[2::10] *= -0.1
    return q(f0), q(f1), w


def head_restated(f0, f1, w, dt, blocks=1):
    """per frame and block: sum over the block's pixels (16 b + 16 blocks k + j) of sum_c w_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2, every step in dt -> float64"""
    a, b = f0.to(dt), f1.to(dt)
    ua = a / (torch.sqrt((a * a).sum(-1, keepdim=True)) + EPS_N)
    ub = b / (torch.sqrt((b * b).sum(-1, keepdim=True)) + EPS_N)
    px = (((ua - ub) ** 2) * w.to(dt)).sum(-1).double()      # (nf, npix)
    owner = (torch.arange(px.shape[1]) // 16) % blocks
    return torch.stack([px[:, owner == b].sum(1) for b in range(blocks)], dim=1)      # (nf, blocks)


def head_reference(f0, f1, w):
    """(float64 per-frame sums, the relative spread of the float32 restatement against them); the spread condition of the bound is asserted here"""
    s64, s32 = head_restated(f0, f1, w, torch.float64).sum(1), head_restated(f0, f1, w, torch.float32).sum(1)
    live = s64 > 0
    assert live.any()
    spread = ((s32 - s64).abs()[live] / s64[live]).max().item()
    assert spread < 1e-5, f"restatement spread {spread:.2e}: choose other inputs"
    assert (s32[~live] == 0).all()
    return s64, spread


def lpips_head_case(lib, dev, Cc, s0, s1):
    """one instance <C / 64, S0, S1> at every npix of HEAD_NPIX and blocks in {1, 2, lpips_blocks(npix)}: per-frame sums of part[n * blocks + b]; identical maps exactly 0; the
    swapped call and a second call the same bits.  Largest relative error seen (simulator and MI355X alike): 1.0e-7 against the floor 1e-6 (<4,1,1>, npix 1)"""
    declare(lib)
    st = stream(dev)
    for npix in HEAD_NPIX:
        f0, f1, w = head_inputs(Cc, npix)
        s64, spread = head_reference(f0, f1, w)
        tol = max(8 * spread, 1e-6)
        d0, d1, wd = upload(f0.reshape(HEAD_NF, 1, npix, Cc), s0, dev), upload(f1.reshape(HEAD_NF, 1, npix, Cc), s1, dev), w.to(dev)
        assert lib.caddy_k_lpips_blocks(npix) == lpips_blocks(npix)
        for blocks in sorted({1, 2, lpips_blocks(npix)}):
            name = f"k_lpips_head<{Cc // 64},{int(s0)},{int(s1)}> npix {npix} blocks {blocks}"
            part = Out(HEAD_NF * blocks, dev, dtype=torch.float64)
            assert lib.caddy_k_lpips_head(P(d0), int(s0), P(d1), int(s1), P(wd), HEAD_NF, npix, Cc, blocks, part.p, st) == 0
            sync(dev)
            got = part.cpu().reshape(HEAD_NF, blocks)
            assert not torch.isnan(got).any(), name + ": a partial was not written"
            per_block = head_restated(f0, f1, w, torch.float64, blocks)
            worst = 0.0
            for n in range(HEAD_NF):
                gs = math.fsum(got[n].tolist())
                if s64[n] == 0:
                    assert gs == 0.0, name + f": frame {n} must be exactly 0"
                    continue
                worst = max(worst, abs(gs - s64[n].item()) / s64[n].item())
                # block by block (the layout part[n * blocks + b] and the pixels a block owns), relative to the frame's sum
                assert (got[n] - per_block[n]).abs().max().item() <= tol * s64[n].item(), name + f": partials of frame {n}"
            record("lpips_head", name + f" (spread {spread:.1e})", worst, tol)
            part.guards(name)
            again = Out(HEAD_NF * blocks, dev, dtype=torch.float64)
            assert lib.caddy_k_lpips_head(P(d0), int(s0), P(d1), int(s1), P(wd), HEAD_NF, npix, Cc, blocks, again.p, st) == 0
            swapped = Out(HEAD_NF * blocks, dev, dtype=torch.float64)
            assert lib.caddy_k_lpips_head(P(d1), int(s1), P(d0), int(s0), P(wd), HEAD_NF, npix, Cc, blocks, swapped.p, st) == 0
            same = Out(HEAD_NF * blocks, dev, dtype=torch.float64)
            assert lib.caddy_k_lpips_head(P(d0), int(s0), P(d0), int(s0), P(wd), HEAD_NF, npix, Cc, blocks, same.p, st) == 0
            sync(dev)
            assert torch.equal(again.cpu().view(torch.int64), part.cpu().view(torch.int64)), name + ": a second call differs"
            assert torch.equal(swapped.cpu().view(torch.int64), part.cpu().view(torch.int64)), name + ": the swapped call differs"
            assert torch.equal(same.cpu().view(torch.int64), torch.zeros(HEAD_NF * blocks, dtype=torch.int64)), name + ": identical maps are not exactly 0.0"
            for o in (again, swapped, same):
                o.guards(name)


FINALIZE_BLOCKS = (1, 2, 5, 128, 3)


def lpips_finalize_case(lib, dev, nf):
    """bit-equal to the kernel's additions and its one multiplication per level done in Python floats in the same order; columns >= nf of the (6, ldo) output untouched.  The
    regions of the partial slab are laid out with gaps, so lv.off is honoured."""
    declare(lib)
    g = torch.Generator().manual_seed(1100 + nf)
    ldo = nf + 5
    lv = L.LpipsLevels()
    total = 0
    for l, b in enumerate(FINALIZE_BLOCKS):
        total += 3 * l      # a gap in front of each region
        lv.off[l], lv.blocks[l], lv.inv_px[l] = total, b, 1.0 / (3 + 7 * l)
        total += nf * b
    part = torch.randn(total, generator=g, dtype=torch.float64)
    pd = part.to(dev)
    fill = torch.full((6, ldo), 7.5, dtype=torch.float64)
    fill[:, :nf] = float("nan")
    out = Out(6 * ldo, dev, fill=fill, dtype=torch.float64)
    assert lib.caddy_k_lpips_finalize(P(pd), C.byref(lv), total, nf, out.p, ldo, stream(dev)) == 0
    sync(dev)
    want = fill.clone()
    pl = part.tolist()
    for n in range(nf):
        tot = 0.0
        for l, b in enumerate(FINALIZE_BLOCKS):
            s = 0.0
            for k in range(b):
                s += pl[lv.off[l] + n * b + k]
            s *= lv.inv_px[l]
            want[1 + l, n] = s
            tot += s
        want[0, n] = tot
    got = out.cpu().reshape(6, ldo)
    assert torch.equal(got[:, nf:], fill[:, nf:]), "k_lpips_finalize: columns >= nf"
    assert torch.equal(got[:, :nf].contiguous().view(torch.int64), want[:, :nf].contiguous().view(torch.int64)), "k_lpips_finalize: not bit-equal"
    out.guards("k_lpips_finalize")
    assert torch.equal(pd.cpu(), part)


# ====================================================================================================================================================================================
# refusals: every entry point validates before it launches
# ====================================================================================================================================================================================
def refusals_case(lib, dev):
    """null pointers, C % 4, S16 without C % 32, head widths other than 64 / 128 / 256 / 512, f outside {1, 2, 4} or sizes that f does not divide, t0 + len > Tfull, a partial slab
    too small for the levels: a negative status, and the output untouched"""
    declare(lib)
    st = stream(dev)
    a, b = torch.zeros(2 * 4 * 4 * 64).to(dev), torch.zeros(2 * 4 * 4 * 64).to(dev)
    w = torch.zeros(512).to(dev)
    out, acc = Out(2 * 4 * 4 * 64, dev), Out(8, dev, fill=ACC0, dtype=torch.float64)
    o, ac, pa, pb, pw = out.p, acc.p, P(a), P(b), P(w)
    calls = [
        lambda: lib.caddy_k_vgg_maxpool2(None, o, 2, 4, 4, 64, st),
        lambda: lib.caddy_k_vgg_maxpool2(pa, None, 2, 4, 4, 64, st),
        lambda: lib.caddy_k_vgg_maxpool2(pa, o, 2, 4, 4, 62, st),
        lambda: lib.caddy_k_vgg_maxpool2(pa, o, 0, 4, 4, 64, st),
        lambda: lib.caddy_k_vgg_maxpool2_bwd_relu(None, 0, pb, o, 0, 2, 4, 4, 64, st),
        lambda: lib.caddy_k_vgg_maxpool2_bwd_relu(pa, 0, None, o, 0, 2, 4, 4, 64, st),
        lambda: lib.caddy_k_vgg_maxpool2_bwd_relu(pa, 0, pb, None, 0, 2, 4, 4, 64, st),
        lambda: lib.caddy_k_vgg_maxpool2_bwd_relu(pa, 0, pb, o, 0, 2, 4, 4, 66, st),
        lambda: lib.caddy_k_vgg_maxpool2_bwd_relu(pa, 1, pb, o, 0, 2, 4, 8, 16, st),      # S16 needs C % 32 == 0
        lambda: lib.caddy_k_vgg_maxpool2_bwd_relu(pa, 0, pb, o, 1, 2, 4, 8, 16, st),
        lambda: lib.caddy_k_vgg_feat_l1(None, 0, pb, 0, 2, 4, 4, 64, SEED_W, o, 0, ac, st),
        lambda: lib.caddy_k_vgg_feat_l1(pa, 0, None, 0, 2, 4, 4, 64, SEED_W, o, 0, ac, st),
        lambda: lib.caddy_k_vgg_feat_l1(pa, 0, pb, 0, 2, 4, 4, 64, SEED_W, o, 0, None, st),
        lambda: lib.caddy_k_vgg_feat_l1(pa, 0, pb, 0, 2, 4, 4, 63, SEED_W, o, 0, ac, st),
        lambda: lib.caddy_k_vgg_feat_l1(pa, 1, pb, 0, 2, 4, 4, 48, SEED_W, o, 0, ac, st),
        lambda: lib.caddy_k_vgg_feat_l1(pa, 0, pb, 1, 2, 4, 4, 48, SEED_W, o, 0, ac, st),
        lambda: lib.caddy_k_vgg_feat_l1(pa, 0, pb, 0, 2, 4, 4, 48, SEED_W, o, 1, ac, st),
        lambda: lib.caddy_k_vgg_feat_l1_img(pa, 0, pb, 0, 2, 4, 4, 64, None, st),
        lambda: lib.caddy_k_vgg_feat_l1_img(pa, 0, pb, 1, 2, 4, 4, 16, ac, st),
        lambda: lib.caddy_k_vgg_feat_l1_img(pa, 0, pb, 0, 2, 4, 4, 6, ac, st),
        lambda: lib.caddy_k_vgg_metric_stage(None, o, 2, 4, 4, 1.0, st),
        lambda: lib.caddy_k_vgg_metric_stage(pa, None, 2, 4, 4, 1.0, st),
        lambda: lib.caddy_k_vgg_metric_stage(pa, o, 2, 4, 4, 0.0, st),
        lambda: lib.caddy_k_lpips_stage(None, o, 2, 4, 4, 1.0, st),
        lambda: lib.caddy_k_lpips_stage(pa, None, 2, 4, 4, 1.0, st),
        lambda: lib.caddy_k_lpips_stage(pa, o, 2, 0, 4, 1.0, st),
        lambda: lib.caddy_k_vgg_time_chunk(None, o, 2, 4, 4, 0, 2, 0, st),
        lambda: lib.caddy_k_vgg_time_chunk(pa, None, 2, 4, 4, 0, 2, 0, st),
        lambda: lib.caddy_k_vgg_time_chunk(pa, o, 2, 4, 4, 3, 2, 0, st),      # t0 + len > Tfull
        lambda: lib.caddy_k_vgg_time_chunk(pa, o, 2, 4, 4, -1, 2, 0, st),
        lambda: lib.caddy_k_vgg_time_chunk(pa, o, 2, 4, 4, 0, 0, 0, st),
        lambda: lib.caddy_k_vgg_copy_f(None, o, 10, st),
        lambda: lib.caddy_k_vgg_copy_f(pa, None, 10, st),
        lambda: lib.caddy_k_vgg_copy_f(pa, o, -1, st),
        lambda: lib.caddy_k_lpips_head(None, 0, pb, 0, pw, 2, 16, 64, 1, ac, st),
        lambda: lib.caddy_k_lpips_head(pa, 0, None, 0, pw, 2, 16, 64, 1, ac, st),
        lambda: lib.caddy_k_lpips_head(pa, 0, pb, 0, None, 2, 16, 64, 1, ac, st),
        lambda: lib.caddy_k_lpips_head(pa, 0, pb, 0, pw, 2, 16, 64, 1, None, st),
        lambda: lib.caddy_k_lpips_head(pa, 0, pb, 0, pw, 2, 16, 96, 1, ac, st),
        lambda: lib.caddy_k_lpips_head(pa, 0, pb, 0, pw, 2, 16, 32, 1, ac, st),
        lambda: lib.caddy_k_lpips_head(pa, 0, pb, 0, pw, 2, 16, 1024, 1, ac, st),
        lambda: lib.caddy_k_lpips_head(pa, 0, pb, 0, pw, 0, 16, 64, 1, ac, st),
        lambda: lib.caddy_k_lpips_head(pa, 0, pb, 0, pw, 2, 0, 64, 1, ac, st),
        lambda: lib.caddy_k_lpips_head(pa, 0, pb, 0, pw, 2, 16, 64, 0, ac, st),
        lambda: lib.caddy_k_lpips_head(pa, 0, pb, 0, pw, 2, 16, 64, 129, ac, st),
    ]
    # k_gt_resize: f outside {1, 2, 4}; an observation size that is not f times the output; the time window past the sequence
    for f, Hi, Wi, Tobs, Trec, t_off, ld, ptr in [(3, 12, 12, 4, 2, 0, 4, pa), (2, 9, 8, 4, 2, 0, 4, pa), (2, 8, 9, 4, 2, 0, 4, pa), (4, 8, 8, 4, 2, 0, 4, pa), (2, 8, 8, 4, 3, 2, 4, pa),
                                                  (2, 8, 8, 4, 2, -1, 4, pa), (2, 8, 8, 4, 2, 0, 2, pa), (2, 8, 8, 4, 2, 0, 4, None)]:
        tv = TV(ptr.value if ptr else None, 2 * Tobs, Hi, Wi, 3, Hi * Wi * ld, ld)
        calls.append(lambda tv=tv, f=f, Tobs=Tobs, Trec=Trec, t_off=t_off: lib.caddy_k_vgg_gt_resize(C.byref(tv), o, 4, 4, 2, Tobs, Trec, t_off, f, st))
    tv = TV(a.data_ptr(), 8, 8, 8, 3, 8 * 8 * 4, 4)
    calls.append(lambda: lib.caddy_k_vgg_gt_resize(C.byref(tv), None, 4, 4, 2, 4, 2, 0, 2, st))
    calls.append(lambda: lib.caddy_k_vgg_gt_resize(None, o, 4, 4, 2, 4, 2, 0, 2, st))
    # the cosine path: a null map, C % 4, S16 without C % 32, a partial slab one element short, nf < 1
    def cos_args(**over):
        ca = VggCosArgs()
        for l in range(5):
            ca.x[l], ca.y[l], ca.x_s16[l], ca.y_s16[l], ca.H[l], ca.W[l], ca.C[l] = a.data_ptr(), b.data_ptr(), 0, 0, 2, 2, 64
        for k, (l, v) in over.items():
            getattr(ca, k)[l] = v
        return ca
    need = 2 * 5 * 3
    for ca, nf, plen, part, outp in [(cos_args(x=(2, None)), 2, need, ac, o), (cos_args(y=(4, None)), 2, need, ac, o), (cos_args(C=(1, 62)), 2, need, ac, o),
                                     (cos_args(C=(3, 16), y_s16=(3, 1)), 2, need, ac, o), (cos_args(C=(3, 16), x_s16=(3, 1)), 2, need, ac, o), (cos_args(H=(0, 0)), 2, need, ac, o),
                                     (cos_args(), 2, need - 1, ac, o), (cos_args(), 0, need, ac, o), (cos_args(), 2, need, None, o), (cos_args(), 2, need, ac, None)]:
        calls.append(lambda ca=ca, nf=nf, plen=plen, part=part, outp=outp: lib.caddy_k_vgg_feat_cos(C.byref(ca), nf, part, plen, outp, st))
    calls.append(lambda: lib.caddy_k_vgg_feat_cos(None, 2, ac, need, o, st))
    # the LPIPS finaliser: a region past the slab, no blocks, ldo < nf, null pointers
    def levels(**over):
        lv = L.LpipsLevels()
        for l in range(5):
            lv.off[l], lv.blocks[l], lv.inv_px[l] = 2 * l, 1, 1.0
        for k, (l, v) in over.items():
            getattr(lv, k)[l] = v
        return lv
    for lv, plen, nf, ldo, part, outp in [(levels(off=(4, 9)), 10, 2, 2, pa, o), (levels(off=(0, -1)), 10, 2, 2, pa, o), (levels(blocks=(2, 0)), 10, 2, 2, pa, o),
                                          (levels(blocks=(4, 2)), 10, 2, 2, pa, o), (levels(), 10, 2, 1, pa, o), (levels(), 10, 0, 2, pa, o), (levels(), 10, 2, 2, None, o),
                                          (levels(), 10, 2, 2, pa, None)]:
        calls.append(lambda lv=lv, plen=plen, nf=nf, ldo=ldo, part=part, outp=outp: lib.caddy_k_lpips_finalize(part, C.byref(lv), plen, nf, outp, ldo, st))
    calls.append(lambda: lib.caddy_k_lpips_finalize(pa, None, 10, 2, o, 2, st))
    for i, call in enumerate(calls):
        rc = call()
        assert rc < 0, f"refusal {i}: status {rc}"
    sync(dev)
    assert torch.isnan(out.cpu()).all() and torch.equal(acc.cpu(), torch.full((8,), ACC0, dtype=torch.float64)), "a refused call wrote"
    out.guards("refusals")
    acc.guards("refusals")
    assert lib.caddy_k_vgg_cos_blocks(2, 2, 62) < 0 and lib.caddy_k_lpips_blocks(0) < 0


INSTANCES2 = [(False, False), (False, True), (True, False), (True, True)]
INSTANCES3 = [(r, g_, z) for r in (False, True) for g_ in (False, True) for z in (False, True)]
HEAD_INSTANCES = [(Cc, s0, s1) for Cc in (64, 128, 256, 512) for s0, s1 in INSTANCES2]
