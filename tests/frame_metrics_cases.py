"""fp64 torch restatement of the dataset evaluation's per-frame metrics (the definitions the fused HIP pass of csrc/frame_metrics.hip implements):
MSE (evaluation/metrics/mse.py), the motion-masked MSE (motion_masked_mse.py + motion_mask.py), PSNR (psnr.py), piq 0.5.1's SSIM as
evaluation/metrics/ssim.py calls it, and the VGG19 cosine similarity (vgg_cosine_similarity.py) on oracle.caddy_oracle's VGG19."""
import torch
import torch.nn.functional as F

from oracle import caddy_oracle as O


def gauss1d(dtype=torch.float64):
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-k ** 2 / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def ssim_restated(ref, gen, value_range=1.0, dtype=torch.float64):
    """(B, T, 3, H, W) -> (B, T): piq.ssim(gen / range, ref / range, reduction="none") with f = max(1, round(min(H, W) / 256)) average pooling,
    an 11 x 11 Gaussian window (sigma 1.5, outer product of the normalised 1-D one), valid padding, c1 = 0.01^2, c2 = 0.03^2"""
    B, T, C, H, W = ref.shape
    x = gen.reshape(B * T, C, H, W).to(dtype) / value_range
    y = ref.reshape(B * T, C, H, W).to(dtype) / value_range
    f = max(1, round(min(H, W) / 256))
    if f > 1:
        x, y = F.avg_pool2d(x, kernel_size=f), F.avg_pool2d(y, kernel_size=f)
    g = gauss1d(dtype).to(x.device)
    w = torch.outer(g, g).expand(C, 1, 11, 11).contiguous()

    def conv(t):
        return F.conv2d(t, w, groups=C)
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    ss = (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs
    return ss.mean(dim=(-1, -2)).mean(1).reshape(B, T)


def metrics_restated(ref, gen, value_range=1.0):
    """{slot: (B, T) float64} for mse, motion_masked_mse, psnr, ssim and the value ranges"""
    r, g = ref.double(), gen.double()
    d2 = (r - g) ** 2
    mask = torch.abs(r[:, 1:] - r[:, :-1]).sum(dim=2, keepdim=True) / 3
    mask = torch.cat([torch.zeros_like(r[:, 0:1, 0:1]), mask], dim=1)
    mse = d2.mean(dim=[2, 3, 4])
    return {"mse": mse, "motion_masked_mse": (d2 * mask).mean(dim=[2, 3, 4]), "psnr": -10 * torch.log10(mse / value_range ** 2 + 1e-8),
            "ssim": ssim_restated(ref, gen, value_range),
            "ref_min": r.amin(dim=[2, 3, 4]), "ref_max": r.amax(dim=[2, 3, 4]), "gen_min": g.amin(dim=[2, 3, 4]), "gen_max": g.amax(dim=[2, 3, 4])}


def vgg_cos_restated(ref, gen, V, value_range=1.0):
    """vgg_cosine_similarity.py:22-57 on the oracle's VGG19 (fp32, like the reference) -> (B, T)"""
    B, T, C, H, W = ref.shape
    d = 0.5 + 1e-6
    fr = O.vgg_features(((ref.float() / value_range - 0.5) / d).reshape(B * T, C, H, W), V)
    fg = O.vgg_features(((gen.float() / value_range - 0.5) / d).reshape(B * T, C, H, W), V)
    sim = torch.zeros(B * T, dtype=torch.float64)
    for a, b in zip(fr, fg):
        sim += F.cosine_similarity(a.reshape(B * T, -1), b.reshape(B * T, -1), dim=1, eps=1e-6).double()
    return (sim / len(fr)).reshape(B, T)


def seeded_pair(B, T, H, W, seed=0, noise=0.1):
    """reference frames with motion between time steps, generated = reference + noise, both in [0, 1]"""
    gen_ = torch.Generator().manual_seed(seed)
    base = torch.rand(B, 1, 3, H, W, generator=gen_)
    drift = torch.rand(B, T, 3, H, W, generator=gen_) * 0.3
    ref = (base * 0.7 + drift).clamp(0, 1)
    gen = (ref + noise * torch.randn(B, T, 3, H, W, generator=gen_)).clamp(0, 1)
    return ref.contiguous(), gen.contiguous()


CASES_GOLDEN = {"a": (2, 4, 24, 20, 3), "b": (1, 5, 16, 33, 4)}      # tests/golden/frame_metrics_ref.npz (tools/gen_metrics_golden.py): name -> (B, T, H, W, seed)
