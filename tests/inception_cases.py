"""Plain-torch restatement of the FID feature network and seeded stand-in weights (tests of csrc/fid.hip and metrics.InceptionFeatures).

`inception_restated` is pytorch_fid.InceptionV3 (pytorch_fid/inception.py:16-160) over torchvision's Inception3 with the FID patches (inception.py:180-322), written as one
function over a state dict with the pt_inception-2015-12-05 names: BasicConv2d = Conv2d(bias=False) -> BatchNorm2d(eps=0.001) -> ReLU.  The same function, run without weights,
creates them (`make_inception_params`), so the structure is stated once on the test side -- independently of the table in csrc/fid.hip, which the tests compare it with."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from playablevideogeneration_amd._lib import TV

BN_EPS = 0.001
BLOCK_CHANNELS = (64, 192, 768, 2048)      # InceptionV3.BLOCK_INDEX_BY_DIM (inception.py:24-29)


class IgemmArgs(C.Structure):      # csrc/fid.h
    _fields_ = [("inp", C.c_void_p), ("in_sn", C.c_long), ("in_ld", C.c_int), ("Cin", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int),
                ("N", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int), ("KH", C.c_int), ("KW", C.c_int), ("stride", C.c_int), ("ph", C.c_int), ("pw", C.c_int),
                ("w", C.c_void_p), ("nchunk", C.c_int), ("gather", C.c_int), ("Cout", C.c_int), ("bias", C.c_void_p), ("relu", C.c_int),
                ("out", C.c_void_p), ("out_sn", C.c_long), ("out_ld", C.c_int), ("precision", C.c_int), ("sat_flag", C.c_void_p)]


class _Net:
    """walks the graph; with P it evaluates, without it records (name, shape) of every tensor and draws seeded values"""

    def __init__(self, P, dtype, gen=None):
        self.P, self.dtype, self.gen, self.made, self.depth = P, dtype, gen, {}, {}

    def basic(self, x, name, cout, k, stride=1, padding=0):
        kh, kw = (k, k) if isinstance(k, int) else k
        cin = x.shape[1]
        if self.P is None:
            fan_in = cin * kh * kw
            self.made[name + ".conv.weight"] = torch.randn(cout, cin, kh, kw, generator=self.gen) * (2.0 / fan_in) ** 0.5      # He: keeps the second moment through ReLU
            self.made[name + ".bn.weight"] = 0.8 + 0.4 * torch.rand(cout, generator=self.gen)
            self.made[name + ".bn.bias"] = 0.2 * torch.rand(cout, generator=self.gen) - 0.1
            self.made[name + ".bn.running_mean"] = 0.2 * torch.rand(cout, generator=self.gen) - 0.1
            self.made[name + ".bn.running_var"] = 0.6 + 0.8 * torch.rand(cout, generator=self.gen)
            P = self.made
        else:
            P = self.P
        w = P[name + ".conv.weight"].to(self.dtype)
        assert tuple(w.shape) == (cout, cin, kh, kw), (name, tuple(w.shape), (cout, cin, kh, kw))
        x = F.conv2d(x, w, None, stride, padding)
        x = F.batch_norm(x, P[name + ".bn.running_mean"].to(self.dtype), P[name + ".bn.running_var"].to(self.dtype), P[name + ".bn.weight"].to(self.dtype),
                         P[name + ".bn.bias"].to(self.dtype), False, 0.0, BN_EPS)
        return F.relu(x)

    def A(self, x, n, pf):      # inception.py:205-227
        b1 = self.basic(x, n + ".branch1x1", 64, 1)
        b5 = self.basic(self.basic(x, n + ".branch5x5_1", 48, 1), n + ".branch5x5_2", 64, 5, 1, 2)
        b3 = self.basic(x, n + ".branch3x3dbl_1", 64, 1)
        b3 = self.basic(b3, n + ".branch3x3dbl_2", 96, 3, 1, 1)
        b3 = self.basic(b3, n + ".branch3x3dbl_3", 96, 3, 1, 1)
        bp = self.basic(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), n + ".branch_pool", pf, 1)
        return torch.cat([b1, b5, b3, bp], 1)

    def B(self, x, n):          # torchvision InceptionB
        b3 = self.basic(x, n + ".branch3x3", 384, 3, 2)
        bd = self.basic(x, n + ".branch3x3dbl_1", 64, 1)
        bd = self.basic(bd, n + ".branch3x3dbl_2", 96, 3, 1, 1)
        bd = self.basic(bd, n + ".branch3x3dbl_3", 96, 3, 2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)

    def Cb(self, x, n, c7):     # inception.py:230-255
        b1 = self.basic(x, n + ".branch1x1", 192, 1)
        b7 = self.basic(x, n + ".branch7x7_1", c7, 1)
        b7 = self.basic(b7, n + ".branch7x7_2", c7, (1, 7), 1, (0, 3))
        b7 = self.basic(b7, n + ".branch7x7_3", 192, (7, 1), 1, (3, 0))
        bd = self.basic(x, n + ".branch7x7dbl_1", c7, 1)
        bd = self.basic(bd, n + ".branch7x7dbl_2", c7, (7, 1), 1, (3, 0))
        bd = self.basic(bd, n + ".branch7x7dbl_3", c7, (1, 7), 1, (0, 3))
        bd = self.basic(bd, n + ".branch7x7dbl_4", c7, (7, 1), 1, (3, 0))
        bd = self.basic(bd, n + ".branch7x7dbl_5", 192, (1, 7), 1, (0, 3))
        bp = self.basic(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), n + ".branch_pool", 192, 1)
        return torch.cat([b1, b7, bd, bp], 1)

    def D(self, x, n):          # torchvision InceptionD
        b3 = self.basic(self.basic(x, n + ".branch3x3_1", 192, 1), n + ".branch3x3_2", 320, 3, 2)
        b7 = self.basic(x, n + ".branch7x7x3_1", 192, 1)
        b7 = self.basic(b7, n + ".branch7x7x3_2", 192, (1, 7), 1, (0, 3))
        b7 = self.basic(b7, n + ".branch7x7x3_3", 192, (7, 1), 1, (3, 0))
        b7 = self.basic(b7, n + ".branch7x7x3_4", 192, 3, 2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)

    def E(self, x, n, max_pool):      # inception.py:258-322
        b1 = self.basic(x, n + ".branch1x1", 320, 1)
        b3 = self.basic(x, n + ".branch3x3_1", 384, 1)
        b3 = torch.cat([self.basic(b3, n + ".branch3x3_2a", 384, (1, 3), 1, (0, 1)), self.basic(b3, n + ".branch3x3_2b", 384, (3, 1), 1, (1, 0))], 1)
        bd = self.basic(x, n + ".branch3x3dbl_1", 448, 1)
        bd = self.basic(bd, n + ".branch3x3dbl_2", 384, 3, 1, 1)
        bd = torch.cat([self.basic(bd, n + ".branch3x3dbl_3a", 384, (1, 3), 1, (0, 1)), self.basic(bd, n + ".branch3x3dbl_3b", 384, (3, 1), 1, (1, 0))], 1)
        pooled = F.max_pool2d(x, 3, 1, 1) if max_pool else F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)      # inception.py:314-319
        bp = self.basic(pooled, n + ".branch_pool", 192, 1)
        return torch.cat([b1, b3, bd, bp], 1)

    def forward(self, frames, resize):
        x = frames.to(self.dtype)
        if resize:
            x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)      # inception.py:143-147
        x = 2 * x - 1                                                                          # inception.py:149-150
        x = self.basic(x, "Conv2d_1a_3x3", 32, 3, 2)
        x = self.basic(x, "Conv2d_2a_3x3", 32, 3)
        x = self.basic(x, "Conv2d_2b_3x3", 64, 3, 1, 1)
        t0 = F.max_pool2d(x, 3, 2)
        x = self.basic(t0, "Conv2d_3b_1x1", 80, 1)
        x = self.basic(x, "Conv2d_4a_3x3", 192, 3)
        t1 = F.max_pool2d(x, 3, 2)
        x = self.A(t1, "Mixed_5b", 32)
        x = self.A(x, "Mixed_5c", 64)
        x = self.A(x, "Mixed_5d", 64)
        x = self.B(x, "Mixed_6a")
        x = self.Cb(x, "Mixed_6b", 128)
        x = self.Cb(x, "Mixed_6c", 160)
        x = self.Cb(x, "Mixed_6d", 160)
        t2 = self.Cb(x, "Mixed_6e", 192)
        x = self.D(t2, "Mixed_7a")
        x = self.E(x, "Mixed_7b", False)
        x = self.E(x, "Mixed_7c", True)
        return [t0, t1, t2, F.adaptive_avg_pool2d(x, (1, 1))]


def inception_restated(frames, P, dtype=torch.float64, resize=True):
    """frames (n, 3, H, W) in [0, 1] -> the four block outputs of InceptionV3([0, 1, 2, 3], resize_input=resize) in `dtype`"""
    with torch.no_grad():
        return _Net(P, dtype).forward(frames, resize)


def restated_features(frames, P, dtype=torch.float64, resize=True, batch=8):
    """(n, 2048) pool_3 features as evaluation/metrics/fid.py:119-137 collects them"""
    frames = frames.reshape((-1,) + tuple(frames.shape[-3:]))
    return torch.cat([inception_restated(frames[i:i + batch], P, dtype, resize)[3].flatten(1) for i in range(0, frames.shape[0], batch)])


def make_inception_params(seed=11):
    """seeded stand-in weights under the pt_inception names: He-scaled convolutions and a non-trivial BatchNorm (weight, running_var away from 1; bias, running_mean away from 0)"""
    net = _Net(None, torch.float32, torch.Generator().manual_seed(seed))
    with torch.no_grad():
        net.forward(torch.rand(1, 3, 75, 75, generator=torch.Generator().manual_seed(0)), False)
    return net.made


def longest_path():
    """convolutions on the longest input -> pool_3 path, counted from the graph: stem 5 + A 3 x 3 + B 3 + C 4 x 5 + D 4 + E 2 x 3"""
    return 5 + 3 * 3 + 3 + 4 * 5 + 4 + 2 * 3


def seeded_frames(n, H, W, seed=0, noise=0.0):
    """smooth frames in [0, 1] (random low-frequency images, as natural frames are), optionally degraded by clipped noise"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, max(H // 8, 2), max(W // 8, 2), generator=g)
    x = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = x + 0.05 * torch.randn(n, 3, H, W, generator=g)
    if noise:
        x = x + noise * torch.randn(n, 3, H, W, generator=g)
    return x.clamp(0, 1).contiguous()


def rel_l2(got, want):
    """per frame relative L2 error"""
    got, want = got.double().flatten(1), want.double().flatten(1)
    return ((got - want).norm(dim=1) / want.norm(dim=1)).max().item()


def tv_of(t_nhwc, C_=None, c0=0):
    """TV view of a contiguous (N, H, W, ld) NHWC tensor's channels [c0, c0 + C_)"""
    N, H, W, ld = t_nhwc.shape
    return TV(t_nhwc.data_ptr() + 4 * c0, N, H, W, C_ if C_ is not None else ld, H * W * ld, ld, 0)


def bind_kernels(lib):
    lib.caddy_k_igemm_weight_bytes.restype = C.c_size_t
    lib.caddy_k_igemm_weight_bytes.argtypes = [C.c_int] * 4
    lib.caddy_k_igemm_pack.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4
    lib.caddy_k_conv_igemm.argtypes = [C.c_void_p, C.c_void_p]
    lib.caddy_k_fid_pool.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.caddy_k_fid_global_avg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.caddy_k_fid_stage.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def run_conv(lib, device, x, w, bias, stride, pad, precision, relu=True, ld_extra=0, c0=0, sync=None, packed=None):
    """x (N, Cin, H, W), w OIHW on the CPU -> the kernel's (N, Cout, Ho, Wo) output (written into channels [c0, c0 + Cout) of a map of pitch Cout + ld_extra) and the
    untouched rest of that map.  packed: a list that receives the packer's fp32 and split-f16 buffers as int32 words"""
    bind_kernels(lib)
    N, Cin, H, W = x.shape
    Cout, _, KH, KW = w.shape
    ph, pw = pad
    Ho, Wo = (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1
    in_ld = 4 if Cin == 3 else Cin
    xin = torch.zeros(N, H, W, in_ld)
    xin[..., :Cin] = x.permute(0, 2, 3, 1)
    xin = xin.to(device).contiguous()
    nb = lib.caddy_k_igemm_weight_bytes(Cin, Cout, KH, KW)
    w32, w16 = torch.zeros(nb // 4, device=device), torch.zeros(nb // 4, device=device)
    wd, bd, bo = w.to(device).contiguous(), bias.to(device).contiguous(), torch.zeros(Cout, device=device)
    assert lib.caddy_k_igemm_pack(wd.data_ptr(), None, None, None, None, 0.0, bd.data_ptr(), Cin, Cout, KH, KW, w32.data_ptr(), w16.data_ptr(), bo.data_ptr(), None) == 0
    ld = Cout + ld_extra
    out = torch.full((N, Ho, Wo, ld), -7.0, device=device)
    flag = torch.zeros(4, dtype=torch.int32, device=device)
    gather = int(Cin < 8 and KH * KW * Cin <= 32)
    a = IgemmArgs(xin.data_ptr(), H * W * in_ld, in_ld, Cin, H, W, N, Ho, Wo, KH, KW, stride, ph, pw, (w32 if precision == 0 else w16).data_ptr(),
                  1 if gather else (Cin + 31) // 32, gather, Cout, bo.data_ptr(), int(relu), out.data_ptr() + 4 * c0, Ho * Wo * ld, ld, precision, flag.data_ptr())
    assert lib.caddy_k_conv_igemm(C.byref(a), None) == 0
    if sync is not None:
        sync()
    out = out.cpu()
    if packed is not None:
        packed += [w32.cpu().view(torch.int32), w16.cpu().view(torch.int32)]
    rest = torch.cat([out[..., :c0], out[..., c0 + Cout:]], -1)
    return out[..., c0:c0 + Cout].permute(0, 3, 1, 2).contiguous(), rest, int(flag.cpu()[0])


def frechet_sqrtm(mu1, s1, mu2, s2):
    """the reference's formula (evaluation/metrics/fid.py:54-75) with scipy's sqrtm"""
    from scipy import linalg
    covmean, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    covmean = covmean.real if np.iscomplexobj(covmean) else covmean
    d = mu1 - mu2
    return float(d.dot(d) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))


# ---- cases shared by the simulator and the MI355X tests ----
# (Cin, Cout, (KH, KW), stride, (ph, pw), H, W): every (kernel, stride, padding) class of the trunk with channel pairs of its table; odd sizes; the tile tails (M = N H W and
# Cout not multiples of 64: 80, 48, 320, 448)
CONV_CASES = [
    (3, 32, (3, 3), 2, (0, 0), 31, 37),        # Conv2d_1a_3x3: the pitch-4 image, K = 27 in one chunk
    (32, 32, (3, 3), 1, (0, 0), 17, 19),       # Conv2d_2a_3x3
    (32, 64, (3, 3), 1, (1, 1), 13, 15),       # Conv2d_2b_3x3
    (64, 80, (1, 1), 1, (0, 0), 9, 11),        # Conv2d_3b_1x1
    (80, 192, (3, 3), 1, (0, 0), 9, 11),       # Conv2d_4a_3x3: unpadded, Cin = 2.5 chunks
    (48, 64, (5, 5), 1, (2, 2), 7, 9),         # branch5x5_2
    (288, 384, (3, 3), 2, (0, 0), 9, 11),      # Mixed_6a.branch3x3
    (128, 128, (1, 7), 1, (0, 3), 7, 9),       # branch7x7_2
    (160, 192, (7, 1), 1, (3, 0), 7, 5),       # branch7x7_3
    (384, 384, (1, 3), 1, (0, 1), 3, 5),       # branch3x3_2a
    (384, 384, (3, 1), 1, (1, 0), 3, 5),       # branch3x3_2b
    (448, 384, (3, 3), 1, (1, 1), 3, 4),       # Mixed_7b.branch3x3dbl_2
    (2048, 320, (1, 1), 1, (0, 0), 8, 8),      # Mixed_7c.branch1x1 at 8 x 8
]
CONV_TOL = 2e-5      # tests/kernel_cases.py: fp32-class arithmetic against F.conv2d


def conv_case(lib, device, case, precision, seed=0, N=2, sync=None):
    Cin, Cout, (KH, KW), stride, pad, H, W = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KH, KW, generator=g) * (2.0 / (Cin * KH * KW)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    want = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride, pad))
    got, rest, flag = run_conv(lib, device, x, w, b, stride, pad, precision, relu=True, ld_extra=16, c0=8, sync=sync)
    err = (got.double() - want).abs().max().item() / max(1.0, want.abs().max().item())
    print(f"conv {case} precision {precision}: max error {err:.2e} (bound {CONV_TOL:.0e})")
    assert got.shape == want.shape and (rest == -7.0).all(), "the launch wrote outside its channel slice"
    assert flag == 0 and err < CONV_TOL, (case, precision, err)


def pool_cases(lib, device, sync=None):
    bind_kernels(lib)
    g = torch.Generator().manual_seed(3)
    for mode, (H, W) in [(0, (9, 11)), (0, (8, 7)), (1, (7, 5)), (1, (3, 3)), (1, (1, 4)), (2, (5, 7)), (2, (1, 1))]:
        x = torch.randn(2, 16, H, W, generator=g)
        want = F.max_pool2d(x, 3, 2) if mode == 0 else (F.avg_pool2d(x, 3, 1, 1, count_include_pad=False) if mode == 1 else F.max_pool2d(x, 3, 1, 1))
        xin = torch.full((2, H, W, 24), 5.0)
        xin[..., 4:20] = x.permute(0, 2, 3, 1)
        xin = xin.to(device)
        out = torch.full((2, want.shape[2], want.shape[3], 20), -7.0, device=device)
        assert lib.caddy_k_fid_pool(C.byref(tv_of(xin, 16, 4)), C.byref(tv_of(out, 16, 0)), mode, None) == 0
        if sync:
            sync()
        got = out.cpu()
        assert (got[..., 16:] == -7.0).all()
        got = got[..., :16].permute(0, 3, 1, 2)
        # max pools select: exact.  The average divides one fp32 sum of <= 9 terms by the window's count: 9 roundings of 2^-24 relative to sum |x|
        tol = 0.0 if mode != 1 else 10 * 2.0 ** -24 * F.avg_pool2d(x.abs(), 3, 1, 1, count_include_pad=False).max().item() * 9
        assert (got - want).abs().max().item() <= tol, (mode, H, W)
    x = torch.randn(3, 5, 7, 32, generator=g).to(device)
    out = torch.zeros(3, 32, dtype=torch.float64, device=device)
    assert lib.caddy_k_fid_global_avg(C.byref(tv_of(x)), out.data_ptr(), None) == 0
    if sync:
        sync()
    assert (out.cpu() - x.cpu().double().mean(dim=(1, 2))).abs().max().item() < 1e-14      # fp64 sums of 35 fp32 values


def resize_cases(lib, device, sizes, sync=None):
    """Bound: an output value is a two-tap lerp in y of two two-tap lerps in x of values in [0, 1], then 2 v - 1.  The kernel and F.interpolate compute the same fp32 expression up to
    the order / fusing of its operations: each of the 3 lerps rounds at most 3 times (two products, one sum) with results in [0, 1], <= 2^-24 each; the weights l1 = src - floor(src)
    carry the rounding of src = scale (dst + 0.5) - 0.5 <= 299, i.e. <= 2^-24 * 512 = 2^-15 absolute in the worst case if the two sides evaluated it differently (a fused multiply-add
    against a separate product and sum), which moves a lerp of values in [0, 1] by at most that much, once per axis; doubling for 2 v - 1:
    2 * (9 * 2^-24 + 2 * 2^-15) < 1.3e-4.  With identical evaluation of src on both sides only the first term remains (1.1e-6); the bound does not assume that."""
    bind_kernels(lib)
    tol = 2 * (9 * 2.0 ** -24 + 2 * 2.0 ** -15)
    for H, W in sizes:
        x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H + W))
        want = 2 * F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) - 1
        xd = x.to(device).contiguous()
        out = torch.full((2, 299, 299, 4), -7.0, device=device)
        assert lib.caddy_k_fid_stage(xd.data_ptr(), 2, H, W, out.data_ptr(), 299, 299, None) == 0
        if sync:
            sync()
        got = out.cpu()
        err = (got[..., :3].permute(0, 3, 1, 2) - want).abs().max().item()
        print(f"resize {H} x {W} -> 299 x 299: max error {err:.2e} (bound {tol:.2e})")
        assert (got[..., 3] == 0).all() and err <= tol, (H, W, err)
        if (H, W) == (299, 299):
            assert err == 0.0      # the identity: weights (1, 0) exactly


def trunk_case(ctx, frames, P, resize, label=""):
    """The four block taps and the 2048-vector of an exact-fp32 context against the fp64 restatement, relative L2 per frame.  Bound: 8 x the spread of the fp32 restatement against
    the fp64 one on the same case, floor 1e-6 -- the rule of tests/lpips_cases.check_levels for two fp32 pipelines that differ in summation order (and here in where the BatchNorm
    scale is rounded: folded into the weights, or applied to the sum).  Depth: the longest path has 47 convolutions against VGG16's 13, but depth enters the restatement's own
    spread the same way it enters the kernel's error -- both accumulate one fp32-rounding-sized relative perturbation per layer -- so the RATIO the factor 8 bounds does not grow
    with depth; fixed before the first run.
    Measured on the simulator (75 x 107, resize off), blocks 0..3: spread 2.3e-7 / 2.7e-7 / 6.0e-7 / 6.3e-7, kernel error 2.9e-7 / 4.2e-7 / 8.6e-7 / 1.0e-6 (bounds 1.8e-6 ..
    5.1e-6).  Not yet measured on the MI355X."""
    n = frames.shape[0]
    feats = ctx(frames)
    assert feats.shape == (n, 2048) and feats.dtype == torch.float64
    w64 = inception_restated(frames[n - ctx.last_frames:], P, torch.float64, resize)
    w32 = inception_restated(frames[n - ctx.last_frames:], P, torch.float32, resize)
    assert (w64[3].flatten(1) != 0).sum(1).min().item() >= 1024, "the stand-in weights let the features die"
    assert w64[3].abs().max().item() < 1e4, "the stand-in weights let the features blow up"
    for b in range(4):
        got = ctx.block(b) if b < 3 else feats[n - ctx.last_frames:].reshape(-1, 2048, 1, 1)
        assert tuple(got.shape) == tuple(w64[b].shape), (b, got.shape, w64[b].shape)
        spread, err = rel_l2(w32[b], w64[b]), rel_l2(got, w64[b])
        tol = max(8 * spread, 1e-6)
        print(f"fid trunk {label} block {b}: restatement spread {spread:.2e}, kernel error {err:.2e}, bound {tol:.2e}")
        assert err <= tol, (label, b, err, tol)
    return feats
