"""Plain-torch restatement of LPIPS as lpips.LPIPS(net='vgg', version='0.1', spatial=False) computes it with normalize=True (what evaluation/metrics/lpips.py:14,33
evaluates per observation), the yardstick of tests/test_lpips_emu.py and tests/test_lpips_gpu.py, and seeded stand-in weights in the style of
oracle.caddy_oracle.make_vgg_params.  For a frame pair x0 = reference, x1 = generated in [0, value_range]:

    1. u = 2 x / value_range - 1;  v = (u - shift) / scale                      (the package's scaling layer)
    2. f_l = relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of torchvision's vgg16().features
    3. n(f) = f / (sqrt(sum_c f_c^2) + 1e-10) per pixel;  d_c = (n(f0)_c - n(f1)_c)^2
    4. level_l = mean_{h,w} sum_c w_{l,c} d_c,  w_l = lin{l}.model[1].weight (1, C_l, 1, 1), no bias
    5. lpips = sum_l level_l
"""
import math

import torch
import torch.nn.functional as F

SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
VGG16_LAYERS = [(0, 3, 64), (2, 64, 64), "M", (5, 64, 128), (7, 128, 128), "M", (10, 128, 256), (12, 256, 256), (14, 256, 256), "M",
                (17, 256, 512), (19, 512, 512), (21, 512, 512), "M", (24, 512, 512), (26, 512, 512), (28, 512, 512)]
TAPS = (2, 7, 14, 21, 28)
CHANNELS = (64, 128, 256, 512, 512)
SLICE_OF = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}      # the package's net.slice{k} that holds features index idx


def make_lpips_params(seed: int = 4321):
    """He-scaled convolutions, small biases, non-negative lin weights |randn| / C_l (the trained ones are non-negative too); torchvision names + lin{l}.model.1.weight"""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for l in VGG16_LAYERS:
        if l == "M":
            continue
        idx, cin, cout = l
        P[f"features.{idx}.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * math.sqrt(2.0 / (cin * 9))
        P[f"features.{idx}.bias"] = 0.05 * torch.randn((cout,), generator=g)
    for l, c in enumerate(CHANNELS):
        P[f"lin{l}.model.1.weight"] = torch.randn((1, c, 1, 1), generator=g).abs() / c
    return P


def as_package_state_dict(P):
    """the same tensors under the names of lpips.LPIPS(net='vgg').state_dict(): net.slice{k}.{idx}.*, lin{l}.model.1.weight, scaling_layer.shift / .scale"""
    out = {"scaling_layer.shift": torch.tensor(SHIFT).reshape(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).reshape(1, 3, 1, 1)}
    for k, v in P.items():
        if k.startswith("features."):
            idx, leaf = k.split(".")[1:]
            out[f"net.slice{SLICE_OF[int(idx)]}.{idx}.{leaf}"] = v
        else:
            out[k] = v
    return out


def split_state_dicts(P):
    """(torchvision vgg16().features.state_dict() naming `{idx}.*`, the lin tensors alone)"""
    return ({k[len("features."):]: v for k, v in P.items() if k.startswith("features.")}, {k: v for k, v in P.items() if k.startswith("lin")})


def vgg16_features(x, P):
    feats = []
    for l in VGG16_LAYERS:
        if l == "M":
            x = F.max_pool2d(x, 2, 2)
        else:
            x = torch.relu(F.conv2d(x, P[f"features.{l[0]}.weight"].to(x.dtype), P[f"features.{l[0]}.bias"].to(x.dtype), padding=1))
            if l[0] in TAPS:
                feats.append(x)
    return feats


def lpips_restated(ref, gen, P, value_range=1.0, dtype=torch.float32):
    """(B, T, 3, H, W) x 2 -> (total (B, T), levels (5, B, T)) float64, every step in `dtype` (fp32 like the package, or fp64)"""
    B, T, C, H, W = ref.shape
    shift = torch.tensor(SHIFT, dtype=dtype).reshape(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).reshape(1, 3, 1, 1)

    def feats(x):
        u = 2 * x.reshape(B * T, C, H, W).to(dtype) / value_range - 1
        return vgg16_features((u - shift) / scale, P)

    def unit(f):
        return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + 1e-10)
    levels = []
    with torch.no_grad():
        for l, (f0, f1) in enumerate(zip(feats(ref), feats(gen))):
            d = (unit(f0) - unit(f1)) ** 2
            w = P[f"lin{l}.model.1.weight"].to(dtype)
            levels.append(F.conv2d(d, w).mean(dim=[2, 3]).reshape(B, T).double())
    levels = torch.stack(levels)
    return levels.sum(0), levels


def check_levels(got_total, got_levels, ref, gen, P, value_range=1.0, label=""):
    """Per level and for the total, relative: 8 x the spread the fp32 restatement itself shows against the fp64 one on this case, floor 1e-6.  Both the restatement and the
    exact-fp32 kernels are fp32 pipelines that differ only in the summation order of <= 4608-term sums; 8 covers the 13-layer depth.  Fixed before the first run.
    Measured (simulator and MI355X alike): kernel error 8e-9 .. 1.7e-6 where the restatement's spread is 2e-8 .. 8e-7; worst case relu5_3 at noise 0.01, 9.4e-6 against 4.1e-5."""
    t32, l32 = lpips_restated(ref, gen, P, value_range, torch.float32)
    t64, l64 = lpips_restated(ref, gen, P, value_range, torch.float64)
    assert (l64 > 0).all()
    for name, got, w32, w64 in [(f"level {l}", got_levels[l], l32[l], l64[l]) for l in range(5)] + [("total", got_total, t32, t64)]:
        spread = float(((w32 - w64).abs() / w64).max())
        err = float(((got - w64).abs() / w64).max())
        tol = max(8 * spread, 1e-6)
        print(f"lpips {label} {name}: restatement spread {spread:.2e}, kernel error {err:.2e}, bound {tol:.2e}")
        assert err <= tol, (label, name, err, tol)
