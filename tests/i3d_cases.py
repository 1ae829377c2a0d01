"""Plain-torch restatement of the FVD feature network and seeded stand-in weights (tests of csrc/fvd.hip and metrics.I3DEmbeddings).

`i3d_restated` is the Kinetics-400 I3D behind evaluation/metrics/fvd.py:67-126 (Inception-v1 inflated to 3-D; every unit conv3d(no bias) -> batch norm(eval, eps 1e-3, no scale
unless a gamma is supplied) -> ReLU, everything TensorFlow-SAME padded) written as one function over a state dict with the module's TF variable names (DHWIO filters), from
F.conv3d, an explicit F.pad to SAME, F.max_pool3d on -inf-padded input, a hand-written gather for TF1's resize_bilinear and the averaging head.  The same function, run without
weights, creates them (`make_i3d_params`), so the structure is stated once on the test side -- independently of the table in csrc/fvd.hip, which the tests compare it with.
Off 224 x 224 (resize off) the head's (2, 7, 7) window is clipped to the final map and the logits are averaged over what remains: the library's definition, restated here."""
import ctypes as C

import torch
import torch.nn.functional as F

from tests.inception_cases import CONV_TOL, rel_l2, run_conv

BN_EPS = 0.001
BLOCK_CHANNELS = (192, 480, 832, 1024)
SIZE = 224


class Conv3dArgs(C.Structure):      # csrc/fvd.h
    _fields_ = [("inp", C.c_void_p), ("in_sn", C.c_long), ("in_ld", C.c_int), ("Cin", C.c_int), ("Ti", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int),
                ("N", C.c_int), ("To", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int), ("KT", C.c_int), ("KH", C.c_int), ("KW", C.c_int),
                ("st", C.c_int), ("sh", C.c_int), ("sw", C.c_int), ("pt", C.c_int), ("ph", C.c_int), ("pw", C.c_int),
                ("w", C.c_void_p), ("nchunk", C.c_int), ("gather", C.c_int), ("Cout", C.c_int), ("bias", C.c_void_p), ("relu", C.c_int),
                ("out", C.c_void_p), ("out_sn", C.c_long), ("out_ld", C.c_int), ("precision", C.c_int), ("sat_flag", C.c_void_p)]


class V5(C.Structure):              # csrc/fvd.h
    _fields_ = [("p", C.c_void_p), ("N", C.c_int), ("T", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("sn", C.c_long), ("ld", C.c_int)]


def same_pads(size, k, s):
    """TensorFlow SAME: (output size, padding in front, padding behind)"""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2, total - total // 2


def pad_same(x, k, s, value=0.0):
    """(N, C, T, H, W) padded so that an unpadded window op of size k / stride s gives TensorFlow's SAME result"""
    pads = []
    for dim in (4, 3, 2):      # F.pad takes the last axis first
        _, lead, trail = same_pads(x.shape[dim], k[dim - 2], s[dim - 2])
        pads += [lead, trail]
    return F.pad(x, pads, value=value)


def max_pool_same(x, k, s):
    return F.max_pool3d(pad_same(x, k, s, float("-inf")), k, s)


def tf_resize_bilinear(x, Ho, Wo):
    """TF1 tf.image.resize_bilinear(align_corners=False), no half-pixel centres (fvd.py:52), on (..., H, W): src = dst * in / out, i1 = min(i0 + 1, in - 1)"""
    H, W = x.shape[-2:]
    def axis(n_in, n_out):
        src = torch.arange(n_out, dtype=torch.float64) * (n_in / n_out)
        i0 = src.floor().long().clamp(max=n_in - 1)
        return i0, (i0 + 1).clamp(max=n_in - 1), (src - i0).to(x.dtype)
    y0, y1, ly = axis(H, Ho)
    x0, x1, lx = axis(W, Wo)
    top = x[..., y0, :][..., x0] + (x[..., y0, :][..., x1] - x[..., y0, :][..., x0]) * lx
    bot = x[..., y1, :][..., x0] + (x[..., y1, :][..., x1] - x[..., y1, :][..., x0]) * lx
    return top + (bot - top) * ly[:, None]


class _Net:
    """walks the graph; with P it evaluates, without it records every tensor under its TF name and draws seeded values; counts the convolutions in front of every tensor"""

    def __init__(self, P, dtype, gen=None, gamma=False):
        self.P, self.dtype, self.gen, self.gamma, self.made, self.convs = P, dtype, gen, gamma, {}, 0
        self._depth, self._keep = {}, []

    def depth(self, x):
        return self._depth.get(id(x), 0)

    def _mark(self, x, d):
        self._keep.append(x)
        self._depth[id(x)] = d
        return x

    def unit(self, x, name, cout, k, stride=1, bn=True):
        cin = x.shape[1]
        if self.P is None:
            self.made[name + "/conv_3d/w"] = torch.randn(k, k, k, cin, cout, generator=self.gen) * (2.0 / (cin * k ** 3)) ** 0.5      # He: keeps the second moment through ReLU
            if bn:
                self.made[name + "/batch_norm/beta"] = 0.2 * torch.rand(1, 1, 1, 1, cout, generator=self.gen) - 0.1
                self.made[name + "/batch_norm/moving_mean"] = 0.2 * torch.rand(1, 1, 1, 1, cout, generator=self.gen) - 0.1
                self.made[name + "/batch_norm/moving_variance"] = 0.6 + 0.8 * torch.rand(1, 1, 1, 1, cout, generator=self.gen)
                if self.gamma:
                    self.made[name + "/batch_norm/gamma"] = 0.8 + 0.4 * torch.rand(cout, generator=self.gen)
            else:
                self.made[name + "/conv_3d/b"] = 0.2 * torch.rand(cout, generator=self.gen) - 0.1
            P = self.made
        else:
            P = self.P
        w = P[name + "/conv_3d/w"].to(self.dtype)
        assert tuple(w.shape) == (k, k, k, cin, cout), (name, tuple(w.shape), (k, k, k, cin, cout))
        self.convs += 1
        d = self.depth(x) + 1
        s3, k3 = (stride,) * 3, (k,) * 3
        x = F.conv3d(pad_same(x, k3, s3), w.permute(4, 3, 0, 1, 2), None if bn else P[name + "/conv_3d/b"].to(self.dtype).reshape(-1), s3)
        if bn:
            gamma = P.get(name + "/batch_norm/gamma")
            x = F.batch_norm(x, P[name + "/batch_norm/moving_mean"].to(self.dtype).reshape(-1), P[name + "/batch_norm/moving_variance"].to(self.dtype).reshape(-1),
                             None if gamma is None else gamma.to(self.dtype).reshape(-1), P[name + "/batch_norm/beta"].to(self.dtype).reshape(-1), False, 0.0, BN_EPS)
            x = F.relu(x)
        return self._mark(x, d)

    def pool(self, x, k, s):
        return self._mark(max_pool_same(x, k, s), self.depth(x))

    def mixed(self, x, n, b0, b1a, b1b, b2a, b2b, b3):
        y0 = self.unit(x, n + "/Branch_0/Conv3d_0a_1x1", b0, 1)
        y1 = self.unit(self.unit(x, n + "/Branch_1/Conv3d_0a_1x1", b1a, 1), n + "/Branch_1/Conv3d_0b_3x3", b1b, 3)
        y2 = self.unit(self.unit(x, n + "/Branch_2/Conv3d_0a_1x1", b2a, 1), n + "/Branch_2/Conv3d_0b_3x3", b2b, 3)
        y3 = self.unit(self.pool(x, (3, 3, 3), (1, 1, 1)), n + "/Branch_3/Conv3d_0b_1x1", b3, 1)
        return self._mark(torch.cat([y0, y1, y2, y3], 1), max(self.depth(y) for y in (y0, y1, y2, y3)))

    def forward(self, videos, resize):
        """videos (n, T, 3, H, W) in [0, 1] -> [Conv3d_2c, Mixed_3c, Mixed_4f, Mixed_5c outputs (NCDHW), (n, 400) logits]"""
        x = videos.to(self.dtype)
        if resize and tuple(x.shape[-2:]) != (SIZE, SIZE):
            x = tf_resize_bilinear(x, SIZE, SIZE)                       # fvd.py:49-52
        x = (2 * x - 1).permute(0, 2, 1, 3, 4)                          # fvd.py:55,212: * 255, then / 255 * 2 - 1
        x = self.unit(x, "Conv3d_1a_7x7", 64, 7, 2)
        x = self.pool(x, (1, 3, 3), (1, 2, 2))
        x = self.unit(x, "Conv3d_2b_1x1", 64, 1)
        t0 = self.unit(x, "Conv3d_2c_3x3", 192, 3)
        x = self.pool(t0, (1, 3, 3), (1, 2, 2))
        x = self.mixed(x, "Mixed_3b", 64, 96, 128, 16, 32, 32)
        t1 = self.mixed(x, "Mixed_3c", 128, 128, 192, 32, 96, 64)
        x = self.pool(t1, (3, 3, 3), (2, 2, 2))
        x = self.mixed(x, "Mixed_4b", 192, 96, 208, 16, 48, 64)
        x = self.mixed(x, "Mixed_4c", 160, 112, 224, 24, 64, 64)
        x = self.mixed(x, "Mixed_4d", 128, 128, 256, 24, 64, 64)
        x = self.mixed(x, "Mixed_4e", 112, 144, 288, 32, 64, 64)
        t2 = self.mixed(x, "Mixed_4f", 256, 160, 320, 32, 128, 128)
        x = self.pool(t2, (2, 2, 2), (2, 2, 2))
        x = self.mixed(x, "Mixed_5b", 256, 160, 320, 32, 128, 128)
        t3 = self.mixed(x, "Mixed_5c", 384, 192, 384, 48, 128, 128)
        window = tuple(min(a, b) for a, b in zip((2, 7, 7), t3.shape[2:]))      # (2, 7, 7) VALID stride 1; clipped to the map off 224 x 224
        x = self._mark(F.avg_pool3d(t3, window, 1), self.depth(t3))
        logits = self.unit(x, "Logits/Conv3d_0c_1x1", 400, 1, bn=False)
        self.longest = self.depth(logits)
        return [t0, t1, t2, t3, logits.mean(dim=(2, 3, 4))]


def i3d_restated(videos, P, dtype=torch.float64, resize=True):
    with torch.no_grad():
        return _Net(P, dtype).forward(videos, resize)


def restated_embeddings(videos, P, dtype=torch.float64, resize=True, batch=8):
    return torch.cat([i3d_restated(videos[i:i + batch], P, dtype, resize)[4] for i in range(0, videos.shape[0], batch)])


def _walk(gamma=False, seed=13):
    net = _Net(None, torch.float32, torch.Generator().manual_seed(seed), gamma)
    with torch.no_grad():
        net.forward(torch.rand(1, 2, 3, 16, 16, generator=torch.Generator().manual_seed(0)), False)
    return net


def make_i3d_params(seed=13, gamma=False):
    """seeded stand-in weights under the TF names: He-scaled filters, non-trivial batch-norm statistics (moving_variance away from 1; beta, moving_mean away from 0)"""
    return _walk(gamma, seed).made


def longest_path():
    """convolutions on the longest input -> logits path, counted from the walk"""
    return _walk().longest


def conv_count():
    return _walk().convs


def block_depths():
    """convolutions in front of each tapped output and the logits on the longest path"""
    net = _Net(make_i3d_params(), torch.float32)
    with torch.no_grad():
        outs = net.forward(torch.rand(1, 2, 3, 16, 16, generator=torch.Generator().manual_seed(0)), False)
    return [net.depth(t) for t in outs[:4]] + [net.longest]


def seeded_videos(n, T, H, W, seed=0, noise=0.0):
    """smooth, slowly moving videos in [0, 1] (a random low-frequency volume, trilinearly up-sampled), optionally degraded by clipped noise"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, max(T // 4, 2), max(H // 8, 2), max(W // 8, 2), generator=g)
    x = F.interpolate(low, size=(T, H, W), mode="trilinear", align_corners=False)
    x = x + 0.05 * torch.randn(n, 3, T, H, W, generator=g)
    if noise:
        x = x + noise * torch.randn(n, 3, T, H, W, generator=g)
    return x.clamp(0, 1).permute(0, 2, 1, 3, 4).contiguous()


def v5_of(t, C_=None, c0=0):
    """V5 view of a contiguous (N, T, H, W, ld) tensor's channels [c0, c0 + C_)"""
    N, T, H, W, ld = t.shape
    return V5(t.data_ptr() + 4 * c0, N, T, H, W, C_ if C_ is not None else ld, T * H * W * ld, ld)


def bind_kernels(lib):
    lib.caddy_k_conv3d_weight_bytes.restype = C.c_size_t
    lib.caddy_k_conv3d_weight_bytes.argtypes = [C.c_int] * 5
    lib.caddy_k_conv3d_pack.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4
    lib.caddy_k_conv3d_igemm.argtypes = [C.c_void_p, C.c_void_p]
    lib.caddy_k_fvd_pool.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    lib.caddy_k_fvd_stage.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def ksteps(Cin, k):
    """32-deep K chunks of one launch, from its arguments (csrc/fvd.h: conv3d_ksteps)"""
    KT, KH, KW = k
    return KT * KH if Cin < 8 else KT * KH * KW * ((Cin + 31) // 32)


def run_conv3d(lib, device, x, w, bias, stride, precision, relu=True, ld_extra=0, c0=0, bn=None, sync=None, packed=None):
    """x (N, Cin, T, H, W), w OIDHW on the CPU, SAME padding -> the kernel's (N, Cout, To, Ho, Wo) output (written into channels [c0, c0 + Cout) of a map of pitch Cout + ld_extra),
    the untouched rest of that map, the range flag and the launch's K steps.  bn: (gamma or None, beta, mean, var) folded by the packer instead of `bias`.  packed: a list that
    receives the packer's fp32 and split-f16 buffers as int32 words"""
    bind_kernels(lib)
    N, Cin, T, H, W = x.shape
    Cout, _, KT, KH, KW = w.shape
    (To, pt, _), (Ho, ph, _), (Wo, pw, _) = same_pads(T, KT, stride[0]), same_pads(H, KH, stride[1]), same_pads(W, KW, stride[2])
    in_ld = 4 if Cin < 8 else Cin
    xin = torch.zeros(N, T, H, W, in_ld)
    xin[..., :Cin] = x.permute(0, 2, 3, 4, 1)
    xin = xin.to(device).contiguous()
    nb = lib.caddy_k_conv3d_weight_bytes(Cin, Cout, KT, KH, KW)
    assert nb == ksteps(Cin, (KT, KH, KW)) * 32 * (-(-Cout // 64) * 64) * 4
    w32, w16 = torch.zeros(nb // 4, device=device), torch.zeros(nb // 4, device=device)
    wd, bo = w.permute(2, 3, 4, 1, 0).contiguous().to(device), torch.zeros(Cout, device=device)      # DHWIO
    ptr = lambda t: None if t is None else t.data_ptr()
    if bn is None:
        bd = bias.to(device).contiguous()
        args = (None, None, None, None, 0.0, bd.data_ptr())
    else:
        keep = [None if t is None else t.to(device).contiguous() for t in bn]
        args = (ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), BN_EPS, None)
    assert lib.caddy_k_conv3d_pack(wd.data_ptr(), *args, Cin, Cout, KT, KH, KW, w32.data_ptr(), w16.data_ptr(), bo.data_ptr(), None) == 0
    ld = Cout + ld_extra
    out = torch.full((N, To, Ho, Wo, ld), -7.0, device=device)
    flag = torch.zeros(4, dtype=torch.int32, device=device)
    gather = int(Cin < 8)
    a = Conv3dArgs(xin.data_ptr(), T * H * W * in_ld, in_ld, Cin, T, H, W, N, To, Ho, Wo, KT, KH, KW, *stride, pt, ph, pw, (w32 if precision == 0 else w16).data_ptr(),
                   1 if gather else (Cin + 31) // 32, gather, Cout, bo.data_ptr(), int(relu), out.data_ptr() + 4 * c0, To * Ho * Wo * ld, ld, precision, flag.data_ptr())
    assert lib.caddy_k_conv3d_igemm(C.byref(a), None) == 0
    if sync is not None:
        sync()
    out = out.cpu()
    if packed is not None:
        packed += [w32.cpu().view(torch.int32), w16.cpu().view(torch.int32)]
    rest = torch.cat([out[..., :c0], out[..., c0 + Cout:]], -1)
    return out[..., c0:c0 + Cout].permute(0, 4, 1, 2, 3).contiguous(), rest, int(flag.cpu()[0]), ksteps(Cin, (KT, KH, KW))


# ---- cases shared by the simulator and the MI355X tests ----
# (Cin, Cout, (KT, KH, KW), (st, sh, sw), (T, H, W)): the smallest shapes that reach each way the kernel can go wrong
CONV3D_CASES = [
    (16, 16, (1, 1, 1), (1, 1, 1), (3, 5, 7)),          # 1x1x1, half a chunk, a quarter of a channel tile; M = 2 * 105: not a multiple of 64, four workgroups
    (24, 48, (3, 3, 3), (1, 1, 1), (3, 5, 4)),          # 3x3x3 stride 1: chunk tail 24, tile tail 48
    (48, 16, (3, 3, 3), (2, 2, 2), (8, 9, 5)),          # stride (2, 2, 2): in 8, k 3 pads (0, 1); in 9 -> out 5 pads (1, 1); chunk tail 48 = 1.5 chunks
    (16, 48, (1, 3, 3), (1, 2, 2), (2, 8, 9)),          # a (1, 3, 3)-like window with its own strides
    (16, 16, (3, 1, 1), (2, 1, 1), (9, 3, 4)),          # a (3, 1, 1)-like window: in 9 -> out 5 in time
    (112, 208, (3, 3, 3), (1, 1, 1), (2, 3, 3)),        # Mixed_4c / 4b channel pairs: 3.5 chunks, 3.25 channel tiles
    (3, 64, (7, 7, 7), (2, 2, 2), (9, 18, 22)),         # Conv3d_1a_7x7: the row-gather layer, asymmetric padding (2, 3) on every axis that is even
    (3, 16, (3, 5, 7), (1, 2, 1), (4, 7, 9)),           # any KT, KH, KW <= 7 through the row gather
    (16, 16, (2, 5, 7), (1, 1, 2), (3, 6, 10)),         # ... and through the chunked path (even windows pad (0, 1))
]


def conv3d_case(lib, device, case, precision, seed=0, N=2, sync=None):
    Cin, Cout, k, stride, (T, H, W) = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, T, H, W, generator=g)
    w = torch.randn(Cout, Cin, *k, generator=g) * (2.0 / (Cin * k[0] * k[1] * k[2])) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    want = F.relu(F.conv3d(pad_same(x.double(), k, stride), w.double(), b.double(), stride))
    got, rest, flag, steps = run_conv3d(lib, device, x, w, b, stride, precision, relu=True, ld_extra=16, c0=8, sync=sync)
    err = (got.double() - want).abs().max().item() / max(1.0, want.abs().max().item())
    print(f"conv3d {case} precision {precision}: max error {err:.2e} (bound {CONV_TOL:.0e}), K = {32 * steps}")
    assert got.shape == want.shape and (rest == -7.0).all(), "the launch wrote outside its channel slice"
    assert flag == 0 and err < CONV_TOL, (case, precision, err)
    if Cin == 3 and k == (7, 7, 7):
        assert 32 * steps <= 1.6 * 1029, steps      # the first layer must not pay a 32-channel chunk per tap (343 x 32 = 10 976)


# (Cin, Cout, (KH, KW), stride, (ph, pw), H, W): 2-D convolutions whose symmetric padding is also TensorFlow's SAME, so the 3-D kernel runs the same problem with KT = 1, T = 1.
# The Cin = 3 gather layers are not here: their K layouts differ by design (27-element window against one window row per chunk).
CROSS_CASES = [
    (32, 64, (3, 3), 1, (1, 1), 13, 15),        # one full chunk; M = 390 is not a multiple of 64
    (48, 64, (5, 5), 1, (2, 2), 7, 9),          # chunk tail: 1.5 chunks
    (64, 80, (1, 1), 1, (0, 0), 9, 11),         # channel-tile tail: Cout = 80
    (16, 48, (3, 3), 2, (1, 1), 9, 7),          # stride 2, half a chunk, odd sizes
    (128, 128, (1, 7), 1, (0, 3), 7, 9),        # asymmetric window, four chunks
]


def cross_case(lib, device, case, precision, seed=0, N=2, sync=None):
    """k_conv_igemm and k_conv3d_igemm walk K in the same order through the same tile body (csrc/conv_igemm.h) where their problems overlap: outputs and packed weights are
    identical, not close"""
    Cin, Cout, (KH, KW), stride, (ph, pw), H, W = case
    assert same_pads(H, KH, stride)[1:] == (ph, ph) and same_pads(W, KW, stride)[1:] == (pw, pw), "the case's padding is not SAME"
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KH, KW, generator=g) * (2.0 / (Cin * KH * KW)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    p2, p3 = [], []
    got2, rest2, flag2 = run_conv(lib, device, x, w, b, stride, (ph, pw), precision, relu=True, ld_extra=16, c0=8, sync=sync, packed=p2)
    got3, rest3, flag3, _ = run_conv3d(lib, device, x[:, :, None], w[:, :, None], b, (1, stride, stride), precision, relu=True, ld_extra=16, c0=8, sync=sync, packed=p3)
    assert got3.shape == got2.shape[:2] + (1,) + got2.shape[2:] and torch.equal(got2, got3[:, :, 0]), (case, precision, (got2 - got3[:, :, 0]).abs().max().item())
    assert flag2 == 0 and flag3 == 0 and (got2 > 0).any(), (case, precision, flag2, flag3)
    assert (rest2 == -7.0).all() and (rest3 == -7.0).all(), "a launch wrote outside its channel slice"
    assert torch.equal(p2[0], p3[0]) and torch.equal(p2[1], p3[1]), "the two packers lay the same weights out differently"


POOL_FORMS = [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1))]


def pool_cases(lib, device, sync=None):
    bind_kernels(lib)
    g = torch.Generator().manual_seed(3)
    for k, s in POOL_FORMS:
        for T, H, W in [(3, 7, 8), (4, 5, 5), (1, 1, 2)]:
            x = torch.randn(2, 16, T, H, W, generator=g) - 1.0      # mostly negative: a padded zero would win
            want = max_pool_same(x, k, s)
            xin = torch.full((2, T, H, W, 24), 5.0)
            xin[..., 4:20] = x.permute(0, 2, 3, 4, 1)
            xin = xin.to(device)
            out = torch.full((2,) + tuple(want.shape[2:]) + (20,), -7.0, device=device)
            assert lib.caddy_k_fvd_pool(C.byref(v5_of(xin, 16, 4)), C.byref(v5_of(out, 16, 0)), *k, *s, None) == 0
            if sync:
                sync()
            got = out.cpu()
            assert (got[..., 16:] == -7.0).all()
            assert torch.equal(got[..., :16].permute(0, 4, 1, 2, 3), want), (k, s, T, H, W)      # a max pool selects: exact


def stage_cases(lib, device, sizes, sync=None):
    """Bound: an output is a lerp in y of two lerps in x of values in [0, 1], then 2 v - 1.  The kernel evaluates src = dst * (in / out) in fp32 (as TensorFlow does), the
    restatement in fp64: scale carries 2^-24 relative, the product another, so src <= 256 differs by at most 2 * 2^-24 * 256 = 2^-15 and a lerp of values in [0, 1] moves by at most
    that, once per axis (where the floor differs the lerp is continuous across it); each of the 3 lerps rounds at most 3 times at <= 2^-24; doubling for 2 v - 1:
    2 * (9 * 2^-24 + 2 * 2^-15) < 1.3e-4.  F.interpolate's half-pixel rule differs from the legacy rule by a sizeable fraction of the local contrast, asserted to be > 100 x that."""
    bind_kernels(lib)
    tol = 2 * (9 * 2.0 ** -24 + 2 * 2.0 ** -15)
    for H, W in sizes:
        x = torch.rand(1, 2, 3, H, W, generator=torch.Generator().manual_seed(H + W))
        want = 2 * tf_resize_bilinear(x.double(), SIZE, SIZE) - 1 if (H, W) != (SIZE, SIZE) else 2 * x.double() - 1
        xd = x.to(device).contiguous()
        out = torch.full((2, SIZE, SIZE, 4), -7.0, device=device)
        assert lib.caddy_k_fvd_stage(xd.data_ptr(), 2, H, W, out.data_ptr(), SIZE, SIZE, None) == 0
        if sync:
            sync()
        got = out.cpu()
        err = (got[..., :3].permute(0, 3, 1, 2).double() - want[0]).abs().max().item()
        print(f"fvd stage {H} x {W} -> {SIZE} x {SIZE}: max error {err:.2e} (bound {tol:.2e})")
        assert (got[..., 3] == 0).all() and err <= tol, (H, W, err)
        if (H, W) == (SIZE, SIZE):
            assert err <= 2.0 ** -23      # only 2 x - 1
        else:
            other = 2 * F.interpolate(x[0], size=(SIZE, SIZE), mode="bilinear", align_corners=False).double() - 1
            assert (other - want[0]).abs().max().item() > 100 * tol and (got[..., :3].permute(0, 3, 1, 2).double() - other).abs().max().item() > 100 * tol


def trunk_case(ctx, videos, P, resize, label=""):
    """The four tapped outputs and the 400 logits of an exact-fp32 context against the fp64 restatement, relative L2 per video.  Bound: the FID exact-path rule
    (inception_cases.trunk_case): 8 x the spread of the fp32 restatement against the fp64 one on the same case, floor 1e-6."""
    n = videos.shape[0]
    emb = ctx(videos)
    assert emb.shape == (n, 400) and emb.dtype == torch.float64
    last = videos[n - ctx.last_videos:]
    w64, w32 = i3d_restated(last, P, torch.float64, resize), i3d_restated(last, P, torch.float32, resize)
    assert (w64[3].flatten(1) != 0).sum(1).min().item() >= w64[3][0].numel() // 8, "the stand-in weights let the features die"
    assert w64[4].abs().max().item() < 1e4, "the stand-in weights let the logits blow up"
    for b in range(5):
        got = ctx.block(b) if b < 4 else emb[n - ctx.last_videos:]
        assert tuple(got.shape) == tuple(w64[b].shape), (b, got.shape, w64[b].shape)
        spread, err = rel_l2(w32[b], w64[b]), rel_l2(got, w64[b])
        tol = max(8 * spread, 1e-6)
        print(f"fvd trunk {label} block {b}: restatement spread {spread:.2e}, kernel error {err:.2e}, bound {tol:.2e}")
        assert err <= tol, (label, b, err, tol)
    return emb
