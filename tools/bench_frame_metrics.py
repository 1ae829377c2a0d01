"""Timing of the dataset evaluation's per-frame metrics at the BAIR evaluation geometry (configs/evaluation/01_bair.yaml: 8 sequences x 30 frames x 256 x 256):

    fused      caddy_frame_metrics without VGG19: the fused pass (csrc/frame_metrics.hip) + its finalize + the 9 x 240 doubles back to the host
    fused_vgg  caddy_frame_metrics with the VGG19 cosine similarity (seeded weights; 30 frames per VGG19 chunk, the default split-f16 arithmetic)
    eager      the same MSE / motion-masked MSE / SSIM in torch eager on the GPU (fp32, the F.conv2d restatement of tests/frame_metrics_cases.py)

Device events around each call after warm-up; one JSON line.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_frame_metrics.py --iters 5`.
    Usage:  python tools/bench_frame_metrics.py [--iters 20] [--no-vgg]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import caddy_oracle as O  # noqa: E402
from playablevideogeneration_amd import metrics as M  # noqa: E402
from tests.frame_metrics_cases import seeded_pair, ssim_restated  # noqa: E402

B, T, H, W = 8, 30, 256, 256


def eager(ref, gen):
    d2 = (ref - gen) ** 2
    mask = torch.abs(ref[:, 1:] - ref[:, :-1]).sum(dim=2, keepdim=True) / 3
    mask = torch.cat([torch.zeros_like(mask[:, 0:1]), mask], dim=1)
    return d2.mean(dim=[2, 3, 4]), (d2 * mask).mean(dim=[2, 3, 4]), ssim_restated(ref, gen, 1.0, dtype=torch.float32)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]      # median, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-vgg", action="store_true")
    args = ap.parse_args()
    ref, gen = (t.cuda() for t in seeded_pair(B, T, H, W, seed=1))
    N = B * T
    out = torch.empty(len(M.SLOTS) * N, dtype=torch.float64)
    fm = M.FrameMetrics(H, W, N)
    fm._stream()

    def fused():
        fm._check(fm.lib.caddy_frame_metrics(fm.ctx, ref.data_ptr(), gen.data_ptr(), B, T, C.c_float(1.0), 0, out.data_ptr()))
    res = {"metric": "frame_metrics_bair_240x256x256", "frames": N, "fused_ms": timed(fused, args.iters)}
    res["eager_ms"] = timed(lambda: eager(ref, gen), args.iters)
    if not args.no_vgg:
        fv = M.FrameMetrics(H, W, 30, O.make_vgg_params())
        fv._stream()

        def fused_vgg():
            fv._check(fv.lib.caddy_frame_metrics(fv.ctx, ref.data_ptr(), gen.data_ptr(), B, T, C.c_float(1.0), 1, out.data_ptr()))
        res["fused_vgg_ms"] = timed(fused_vgg, max(3, args.iters // 4), warmup=1)
        res["vgg_workspace_gib"] = fv.ws_bytes / 2 ** 30
    nbytes = 2 * ref.numel() * 4      # each frame pair read once (the previous reference frame of the motion mask is re-read through the caches)
    res["bytes_read_mb"] = nbytes / 1e6
    res["fused_gbps"] = nbytes / (res["fused_ms"] * 1e-3) / 1e9
    res["speedup_vs_eager"] = res["eager_ms"] / res["fused_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
