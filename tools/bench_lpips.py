"""Timing of one LPIPS chunk (30 frames of 256 x 256, the BAIR evaluation geometry) next to one chunk of the VGG19 cosine similarity on the same frames:

    lpips_ms    caddy_frame_lpips: staging, VGG16 to relu5_3 on both frames, the head of csrc/lpips.hip, 6 x 30 doubles back to the host
    vgg_sim_ms  caddy_frame_metrics with want_vgg = 1: the fused pass, VGG19 to relu5_1 on both frames, the cosine kernels; `--vgg-lib` times it on another build of the
                library (the commit before LPIPS)

Seeded weights, the default split-f16 arithmetic, device events around each call after warm-up, median; one JSON line.  Per-kernel times (the head per level:
k_lpips_head<1 | 2 | 4 | 8, ...> are relu1_2 | relu2_2 | relu3_3 | relu4_3 and relu5_3): `rocprofv3 --kernel-trace --stats -- python tools/bench_lpips.py --iters 5`.
    Usage:  python tools/bench_lpips.py [--iters 20] [--vgg-lib PATH]
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
from playablevideogeneration_amd import _lib, metrics as M  # noqa: E402
from tests.frame_metrics_cases import seeded_pair  # noqa: E402
from tests.lpips_cases import CHANNELS, make_lpips_params  # noqa: E402
from tools.bench_frame_metrics import timed  # noqa: E402

B, T, H, W = 1, 30, 256, 256


def load_other_build(path):
    """another build of the library for the vgg_sim side; one from before LPIPS lacks its entry points, so only what FrameMetrics calls is bound"""
    from playablevideogeneration_amd.engine import _bind as bind_engine
    lib = bind_engine(_lib.load(path))
    lib.caddy_metrics_workspace_bytes.restype = C.c_size_t
    lib.caddy_metrics_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.caddy_metrics_ctx_create.restype = C.c_void_p
    lib.caddy_metrics_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.caddy_frame_metrics.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
    lib._caddy_metrics_bound = True
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--vgg-lib", default=None)
    args = ap.parse_args()
    ref, gen = (t.cuda() for t in seeded_pair(B, T, H, W, seed=1))
    N = B * T
    lp = M.LPIPS(H, W, N, make_lpips_params())
    lp._stream()
    out6 = torch.empty(6 * N, dtype=torch.float64)

    def lpips():
        lp._check(lp.lib.caddy_frame_lpips(lp.ctx, ref.data_ptr(), gen.data_ptr(), B, T, C.c_float(1.0), out6.data_ptr()))
    res = {"metric": "lpips_chunk_30x256x256", "frames": N, "lpips_ms": timed(lpips, args.iters), "lpips_workspace_gib": lp.ws_bytes / 2 ** 30,
           "lpips_s16_taps": f"{lp.tap_formats():05b}"}
    del lp
    fv = M.FrameMetrics(H, W, N, O.make_vgg_params(), lib=load_other_build(args.vgg_lib) if args.vgg_lib else None)
    fv._stream()
    out9 = torch.empty(len(M.SLOTS) * N, dtype=torch.float64)

    def vgg_sim():
        fv._check(fv.lib.caddy_frame_metrics(fv.ctx, ref.data_ptr(), gen.data_ptr(), B, T, C.c_float(1.0), 1, out9.data_ptr()))
    res["vgg_sim_ms"] = timed(vgg_sim, args.iters)
    res["vgg_sim_library"] = args.vgg_lib or "this build"
    res["vgg_workspace_gib"] = fv.ws_bytes / 2 ** 30
    res["lpips_over_vgg_sim"] = res["lpips_ms"] / res["vgg_sim_ms"]
    # the head reads both tapped maps of a level once: 2 x 30 x H_l W_l C_l x 4 bytes
    res["head_bytes_mb_per_level"] = [2 * N * (H >> l) * (W >> l) * c * 4 / 1e6 for l, c in enumerate(CHANNELS)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
