"""Plain-torch restatement of the Inception Score's network and score, seeded stand-in weights and the kernel cases shared by tests/test_is_emu.py and tests/test_is_gpu.py.

`tv_restated` is torchvision's inception_v3(aux_logits=True, transform_input=False).eval() as evaluation/metrics/inception_score.py:20-22,41-43 runs it, written from the published
architecture (Szegedy et al. 2015, torchvision/models/inception.py): BasicConv2d = Conv2d(bias=False) -> BatchNorm2d(eps=0.001) -> ReLU; InceptionA / C / E pool with
F.avg_pool2d(x, 3, 1, 1), torch's default count_include_pad=True, in BOTH E blocks; adaptive average pool, dropout (identity in eval mode), fc = Linear(2048, 1000); AuxLogits
does not run in eval mode.  The frames enter as they are: no 2 x - 1 (transform_input=False, and the metric normalises nothing).  It reuses the BasicConv2d, InceptionB and
InceptionD of tests/inception_cases.py, which pytorch_fid does not patch, and its seeded trunk parameters (the trunk's names are the same)."""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import inception_cases as IC

CLASSES = 1000
# Scale of the seeded N(0, scale^2) fc weights, chosen on the CPU from the fp64 restatement so that the softmax stays informative on the frames of varied_frames (check_informative
# asserts it).  The logits' spread over the classes is ~ scale |f| with f the 2048 pool features.  With the seeded trunk |f| is 17 .. 51 at 299 x 299 and 4 .. 8 at the simulator's
# 75 x 107 (a 1 x 2 final map, where the padding-including averages dilute the features), so each geometry class has its scale:
#   network at 299 x 299, scale 0.08: per-frame entropy 2.0 .. 5.8 nats, IS 1.28 (3 frames of 64 x 64) and 1.29 (4 frames of 256 x 256)
#   network at the frames' own size, scale 0.5: entropy 4.1 .. 4.9 nats, IS 1.18 (3 frames of 75 x 107); 4.6 .. 5.2 nats, IS 1.07 (4 frames of 76 x 80)
FC_SCALE_299, FC_SCALE_OWN_SIZE = 0.08, 0.5
FC_BIAS_SCALE = 0.5


class _TvNet(IC._Net):
    """torchvision's forward passes where pytorch_fid patches them (tests/inception_cases.py has the patched ones)"""

    def A(self, x, n, pf):      # torchvision InceptionA._forward
        b1 = self.basic(x, n + ".branch1x1", 64, 1)
        b5 = self.basic(self.basic(x, n + ".branch5x5_1", 48, 1), n + ".branch5x5_2", 64, 5, 1, 2)
        b3 = self.basic(x, n + ".branch3x3dbl_1", 64, 1)
        b3 = self.basic(b3, n + ".branch3x3dbl_2", 96, 3, 1, 1)
        b3 = self.basic(b3, n + ".branch3x3dbl_3", 96, 3, 1, 1)
        bp = self.basic(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1), n + ".branch_pool", pf, 1)
        return torch.cat([b1, b5, b3, bp], 1)

    def Cb(self, x, n, c7):     # torchvision InceptionC._forward
        b1 = self.basic(x, n + ".branch1x1", 192, 1)
        b7 = self.basic(x, n + ".branch7x7_1", c7, 1)
        b7 = self.basic(b7, n + ".branch7x7_2", c7, (1, 7), 1, (0, 3))
        b7 = self.basic(b7, n + ".branch7x7_3", 192, (7, 1), 1, (3, 0))
        bd = self.basic(x, n + ".branch7x7dbl_1", c7, 1)
        bd = self.basic(bd, n + ".branch7x7dbl_2", c7, (7, 1), 1, (3, 0))
        bd = self.basic(bd, n + ".branch7x7dbl_3", c7, (1, 7), 1, (0, 3))
        bd = self.basic(bd, n + ".branch7x7dbl_4", c7, (7, 1), 1, (3, 0))
        bd = self.basic(bd, n + ".branch7x7dbl_5", 192, (1, 7), 1, (0, 3))
        bp = self.basic(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1), n + ".branch_pool", 192, 1)
        return torch.cat([b1, b7, bd, bp], 1)

    def E(self, x, n, max_pool=False):      # torchvision InceptionE._forward: an average pool in Mixed_7b AND Mixed_7c
        b1 = self.basic(x, n + ".branch1x1", 320, 1)
        b3 = self.basic(x, n + ".branch3x3_1", 384, 1)
        b3 = torch.cat([self.basic(b3, n + ".branch3x3_2a", 384, (1, 3), 1, (0, 1)), self.basic(b3, n + ".branch3x3_2b", 384, (3, 1), 1, (1, 0))], 1)
        bd = self.basic(x, n + ".branch3x3dbl_1", 448, 1)
        bd = self.basic(bd, n + ".branch3x3dbl_2", 384, 3, 1, 1)
        bd = torch.cat([self.basic(bd, n + ".branch3x3dbl_3a", 384, (1, 3), 1, (0, 1)), self.basic(bd, n + ".branch3x3dbl_3b", 384, (3, 1), 1, (1, 0))], 1)
        bp = self.basic(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1), n + ".branch_pool", 192, 1)
        return torch.cat([b1, b3, bd, bp], 1)

    def forward(self, frames, resize):
        x = frames.to(self.dtype)
        if resize:
            x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)      # nn.Upsample(size=(299, 299), mode='bilinear') (inception_score.py:22,41)
        x = self.basic(x, "Conv2d_1a_3x3", 32, 3, 2)                                          # transform_input=False: no normalisation
        x = self.basic(x, "Conv2d_2a_3x3", 32, 3)
        x = self.basic(x, "Conv2d_2b_3x3", 64, 3, 1, 1)
        x = F.max_pool2d(x, 3, 2)
        x = self.basic(x, "Conv2d_3b_1x1", 80, 1)
        x = self.basic(x, "Conv2d_4a_3x3", 192, 3)
        x = F.max_pool2d(x, 3, 2)
        x = self.A(x, "Mixed_5b", 32)
        x = self.A(x, "Mixed_5c", 64)
        x = self.A(x, "Mixed_5d", 64)
        x = self.B(x, "Mixed_6a")
        x = self.Cb(x, "Mixed_6b", 128)
        x = self.Cb(x, "Mixed_6c", 160)
        x = self.Cb(x, "Mixed_6d", 160)
        x = self.Cb(x, "Mixed_6e", 192)
        x = self.D(x, "Mixed_7a")
        x = self.E(x, "Mixed_7b")
        x = self.E(x, "Mixed_7c")
        x = F.adaptive_avg_pool2d(x, (1, 1)).flatten(1)                                       # dropout: identity in eval mode
        return F.linear(x, self.P["fc.weight"].to(self.dtype), self.P["fc.bias"].to(self.dtype))


def tv_logits(frames, P, dtype=torch.float64, resize=True, batch=8):
    """(n, 3, H, W) frames in [0, 1] -> (n, 1000) logits in `dtype`"""
    frames = frames.reshape((-1,) + tuple(frames.shape[-3:]))
    with torch.no_grad():
        return torch.cat([_TvNet(P, dtype).forward(frames[i:i + batch], resize) for i in range(0, frames.shape[0], batch)])


def tv_probabilities(frames, P, dtype=torch.float64, resize=True):
    """F.softmax of the logits (inception_score.py:43)"""
    return torch.softmax(tv_logits(frames, P, dtype, resize), dim=1)


def make_is_params(resize=True, seed=11, fc_seed=12):
    """the seeded trunk of tests/inception_cases.py plus fc.weight / fc.bias under torchvision's names, fc scaled for the network at 299 x 299 (resize) or at the frames' own size"""
    P = dict(IC.make_inception_params(seed))
    g = torch.Generator().manual_seed(fc_seed)
    P["fc.weight"] = torch.randn(CLASSES, 2048, generator=g) * (FC_SCALE_299 if resize else FC_SCALE_OWN_SIZE)
    P["fc.bias"] = torch.randn(CLASSES, generator=g) * FC_BIAS_SCALE
    return P


def varied_frames(n, H, W, seed):
    """inception_cases.seeded_frames made to differ the way frames of a dataset do -- brightness falling from 1 to 0.25 over the n frames, every other frame noisy -- so that the
    class distributions of the seeded network differ between frames (the seeded trunk maps similar frames to nearly the same features, and IS would be 1)"""
    x = IC.seeded_frames(n, H, W, seed=seed)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 100))
    k = torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1)
    return ((x + 0.3 * (k % 2) * noise).clamp(0, 1) * (1.0 - 0.75 * k / max(n - 1, 1))).contiguous()


def longest_path():
    """convolutions on the longest input -> logits path, counted from the graph: the trunk's 47 and fc"""
    return IC.longest_path() + 1


def reference_score(preds, splits=1):
    """the reference's loop (evaluation/metrics/inception_score.py:48-65) with scipy.stats.entropy, on the rows it is given"""
    from scipy.stats import entropy
    preds = np.asarray(preds)
    split_scores = []
    samples_count = preds.shape[0]
    for k in range(splits):
        part = preds[k * (samples_count // splits): (k + 1) * (samples_count // splits), :]
        py = np.mean(part, axis=0)
        scores = []
        for i in range(part.shape[0]):
            scores.append(entropy(part[i, :], py))
        split_scores.append(np.exp(np.mean(scores)))
    return {"is/mean": np.mean(split_scores), "is/std": np.std(split_scores)}


def check_informative(p64, label=""):
    """the seeded fc keeps the softmax informative on these frames: per-frame entropy in [0.5, ln 1000 - 0.5] nats and an Inception Score above 1.05, on the fp64 restatement"""
    p = p64.double()
    ent = -(p * torch.log(p.clamp_min(1e-300))).sum(1)
    score = reference_score(p.numpy())["is/mean"]
    print(f"restated fp64 {label}: per-frame entropy {ent.min().item():.3f} .. {ent.max().item():.3f} nats (ln 1000 = {math.log(CLASSES):.3f}), IS {score:.4f}")
    assert ent.min().item() >= 0.5 and ent.max().item() <= math.log(CLASSES) - 0.5, ent.tolist()
    assert score > 1.05, score
    return score


def log_is_bound(d1):
    """Bound on |d ln IS| of one split when every row of the probabilities moves by at most d1 in L1.  ln IS = mean_i KL(p_i || pbar) = H(pbar) - mean_i H(p_i) with H the
    Shannon entropy and pbar the mean row; pbar moves by at most d1 in L1 as well.  The entropy's continuity bound (Fannes-Audenaert, classical form, T = |p - q|_1 / 2 <= 1/2):
    |H(p) - H(q)| <= T ln(K - 1) + h(T), h the binary entropy in nats, applied to both terms: |d ln IS| <= 2 (T ln 999 + h(T)) with T = d1 / 2."""
    T = d1 / 2
    assert 0 < T <= 0.5
    h = -T * math.log(T) - (1 - T) * math.log1p(-T)
    return 2 * (T * math.log(CLASSES - 1) + h)


# ---- kernel cases shared by the simulator and the MI355X tests ----
def bind_kernels(lib):
    IC.bind_kernels(lib)
    lib.caddy_k_is_stage.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.caddy_k_is_softmax.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_long, C.c_void_p]
    return lib


def pool_cases(lib, device, sync=None):
    """mode 3 = F.avg_pool2d(x, 3, 1, 1) (count_include_pad=True) at C = 4 and 8 on 1 x 1, 2 x 3, 5 x 7 and 8 x 8 maps; on the 1 x 1 map it is mode 1 over 9; modes 0..2 as before.
    Bound of the averages as in inception_cases.pool_cases: one fp32 sum of <= 9 terms and a division, 10 roundings of 2^-24 relative to the sum of |x| over the window."""
    bind_kernels(lib)
    g = torch.Generator().manual_seed(5)

    def run(x, mode, want_hw):
        n, c, H, W = x.shape
        xin = torch.full((n, H, W, c + 8), 5.0)
        xin[..., 4:4 + c] = x.permute(0, 2, 3, 1)
        xin = xin.to(device)
        out = torch.full((n, want_hw[0], want_hw[1], c + 4), -7.0, device=device)
        assert lib.caddy_k_fid_pool(C.byref(IC.tv_of(xin, c, 4)), C.byref(IC.tv_of(out, c, 0)), mode, None) == 0
        if sync:
            sync()
        got = out.cpu()
        assert (got[..., c:] == -7.0).all(), "the launch wrote outside its channel slice"
        return got[..., :c].permute(0, 3, 1, 2)

    for c in (4, 8):
        for H, W in [(1, 1), (2, 3), (5, 7), (8, 8)]:
            x = torch.randn(2, c, H, W, generator=g)
            want = F.avg_pool2d(x, 3, 1, 1)
            got = run(x, 3, (H, W))
            tol = 10 * 2.0 ** -24 * F.avg_pool2d(x.abs(), 3, 1, 1).max().item() * 9
            err = (got - want).abs().max().item()
            print(f"pool mode 3 C {c} {H} x {W}: max error {err:.2e} (bound {tol:.2e})")
            assert err <= tol, (c, H, W, err)
            excl = run(x, 1, (H, W))
            tol1 = 10 * 2.0 ** -24 * F.avg_pool2d(x.abs(), 3, 1, 1, count_include_pad=False).max().item() * 9
            assert (excl - F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)).abs().max().item() <= tol1
            if (H, W) == (1, 1):
                assert torch.equal(excl, x) and (got - x / 9).abs().max().item() <= tol      # the two averages differ by the factor 9
            assert torch.equal(run(x, 2, (H, W)), F.max_pool2d(x, 3, 1, 1))
            if H >= 3:
                assert torch.equal(run(x, 0, ((H - 3) // 2 + 1, (W - 3) // 2 + 1)), F.max_pool2d(x, 3, 2))
    t = IC.tv_of(torch.zeros(1, 2, 2, 4).to(device))
    assert lib.caddy_k_fid_pool(C.byref(t), C.byref(t), 4, None) != 0      # no mode 4


def stage_cases(lib, device, sync=None):
    """the input stage without 2 x - 1: F.interpolate(align_corners=False) at 64 x 64 -> 299 x 299, and the copy at 75 x 107 with the resize off.  Bound: that of
    inception_cases.resize_cases without its final doubling (9 roundings of the three lerps and the source coordinate's rounding once per axis): 9 * 2^-24 + 2 * 2^-15."""
    bind_kernels(lib)
    tol = 9 * 2.0 ** -24 + 2 * 2.0 ** -15
    for (H, W), (Ho, Wo) in [((64, 64), (299, 299)), ((75, 107), (75, 107))]:
        x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H + W))
        want = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False) if (H, W) != (Ho, Wo) else x
        xd = x.to(device).contiguous()
        out = torch.full((2, Ho, Wo, 4), -7.0, device=device)
        assert lib.caddy_k_is_stage(xd.data_ptr(), 2, H, W, out.data_ptr(), Ho, Wo, None) == 0
        if sync:
            sync()
        got = out.cpu()
        err = (got[..., :3].permute(0, 3, 1, 2) - want).abs().max().item()
        print(f"stage without 2x-1 {H} x {W} -> {Ho} x {Wo}: max error {err:.2e} (bound {tol:.2e})")
        assert (got[..., 3] == 0).all() and err <= tol, (H, W, err)
        assert got[..., :3].min().item() >= 0.0      # values of [0, 1] stay there: nothing was mapped to [-1, 1]
        if (H, W) == (Ho, Wo):
            assert err == 0.0


def run_softmax(lib, device, z, ld_in=None, ld_out=None, sync=None):
    """rows of z through caddy_k_is_softmax, with pitches wider than the row on request; returns the probabilities and checks that the padding stayed untouched"""
    bind_kernels(lib)
    n, c = z.shape
    ld_in, ld_out = ld_in or c, ld_out or c
    zin = torch.full((n, ld_in), 1e30)
    zin[:, :c] = z
    zin = zin.to(device)
    out = torch.full((n + 1, ld_out), -7.0, device=device)      # (one canary row behind the last frame)
    assert lib.caddy_k_is_softmax(zin.data_ptr(), out.data_ptr(), n, c, ld_in, ld_out, None) == 0
    if sync:
        sync()
    got = out.cpu()
    assert (got[:n, c:] == -7.0).all() and (got[n] == -7.0).all(), "the softmax wrote outside its rows"
    return got[:n, :c]


# fp32 softmax against torch's fp32 softmax: both compute exp(z - max) / sum; the exponentials differ by a few ulp between two libraries (<= 4 ulp = 2^-22 relative each), the
# sums of <= 1000 positive terms by <= 1000 * 2^-24 relative in any order, the division by one rounding: relative error of a probability <= 2^-22 + 2^-14 + 2^-24 < 7e-5
SOFTMAX_RTOL = 7e-5


def softmax_cases(lib, device, sync=None):
    g = torch.Generator().manual_seed(9)
    for n in (1, 3, 65):
        z = 3 * torch.randn(n, CLASSES, generator=g)
        got = run_softmax(lib, device, z, sync=sync)
        want = torch.softmax(z, 1)
        rel = ((got - want).abs() / want).max().item()
        print(f"softmax {n} x {CLASSES}: max relative error {rel:.2e} (bound {SOFTMAX_RTOL:.0e}), row sums within {(got.double().sum(1) - 1).abs().max().item():.1e}")
        assert rel <= SOFTMAX_RTOL and (got.double().sum(1) - 1).abs().max().item() <= 1e-6
        assert torch.equal(got, run_softmax(lib, device, z, sync=sync))                                   # two calls: identical bits
        assert torch.equal(got[:1], run_softmax(lib, device, z[:1], sync=sync))                           # a row depends on that row alone
        flat = run_softmax(lib, device, torch.full((n, CLASSES), 2.5), sync=sync)
        assert (flat == np.float32(1.0) / np.float32(CLASSES)).all()                                      # exp(0) = 1, the sum 1000 and 1 / 1000 are exact or correctly rounded
        for shift in (80.0, -80.0):
            moved = run_softmax(lib, device, z + shift, sync=sync)
            assert torch.isfinite(moved).all() and (moved.double().sum(1) - 1).abs().max().item() <= 1e-6
            # z + shift rounds every logit by <= ulp(128) / 2 = 2^-18 (|z| + 80 < 128): the probabilities move by a factor within exp(+-2 * 2^-18), i.e. 2^-17 relative to first
            # order, on top of the bound above
            assert (z.abs().max().item() + 80 < 128) and ((moved - want).abs() / want).max().item() <= 1.001 * 2.0 ** -17 + SOFTMAX_RTOL
    for c in (64, 1):      # the raw launcher: one full pass of the lanes, and a single column (63 idle lanes)
        z = torch.randn(5, c, generator=g)
        got = run_softmax(lib, device, z, ld_in=c + 3, ld_out=c + 5, sync=sync)
        want = torch.softmax(z, 1)
        assert ((got - want).abs() / want).max().item() <= SOFTMAX_RTOL
        if c == 1:
            assert (got == 1.0).all()
    assert lib.caddy_k_is_softmax(None, None, 1, 1, 1, 1, None) != 0


def fc_cases(lib, device, sync=None):
    """fc on k_conv_igemm as a 1 x 1 convolution: N rows x 2048 -> 1000 with bias and no ReLU against F.linear in fp64, both arithmetics, the partial tile 960..999 on its own,
    and the 16 floats past column 999 of every row untouched (run_conv writes into a map 16 floats wider than Cout).  Bound: inception_cases.CONV_TOL."""
    g = torch.Generator().manual_seed(13)
    w = torch.randn(CLASSES, 2048, generator=g) * (1.0 / 2048) ** 0.5
    b = torch.randn(CLASSES, generator=g) * 0.1
    for n in (1, 3, 65):
        x = torch.randn(n, 2048, generator=g)
        want = F.linear(x.double(), w.double(), b.double())
        assert (want < 0).any()      # (no ReLU: negative logits survive)
        for precision in (0, 16):
            got, rest, flag = IC.run_conv(lib, device, x.reshape(n, 2048, 1, 1), w.reshape(CLASSES, 2048, 1, 1), b, 1, (0, 0), precision, relu=False, ld_extra=16, c0=0, sync=sync)
            got = got.reshape(n, CLASSES).double()
            scale = max(1.0, want.abs().max().item())
            err, tail = (got - want).abs().max().item() / scale, (got[:, 960:] - want[:, 960:]).abs().max().item() / scale
            print(f"fc {n} x 2048 -> 1000 precision {precision}: max error {err:.2e}, columns 960..999 {tail:.2e} (bound {IC.CONV_TOL:.0e})")
            assert flag == 0 and err < IC.CONV_TOL and tail < IC.CONV_TOL, (n, precision, err, tail)
            assert rest.shape[-1] == 16 and (rest == -7.0).all(), "fc wrote past column 999"
