"""Throughput of the FVD feature network (metrics.I3DEmbeddings, csrc/fvd.hip) on the MI355X:  python tools/bench_fvd.py [--videos 8] [--frames 30] [--size 256] [--out FILE]

Device only; reads nothing outside the repository.  Prints one JSON line: videos/s at the BAIR evaluation geometry (8 x 30 x 3 x 256 x 256 resized to 224 x 224) in both
arithmetics, steady state (one warm-up call, then the mean of `--repeats` calls), the per-stage times of the last chunk (caddy_debug_fvd_stage_ms), the TMAC/s of the trunk from
caddy_fvd_macs_per_video -- and, for Mixed_4b's 3x3x3 layer (96 -> 208 on 8 x 14 x 14 per video), the rate of k_conv3d_igemm next to the rate of the existing 2-D k_conv_igemm on a
problem of equal M, N and K.  The 2-D launcher takes windows up to 7 x 7, so the 27 taps x 96 channels are posed to it as 9 taps x 288 channels (3 x 3, 64 frames of 14 x 14): the same
81 K chunks of 32, the same 12 544 positions, the same 208 channels."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, repeats):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats / 1e3


def layer_rates(lib, repeats=20):
    """TMAC/s of the 3-D kernel on Mixed_4b/Branch_1/Conv3d_0b_3x3 for 8 videos and of the 2-D kernel on the equal-(M, N, K) problem, both arithmetics"""
    from tests import i3d_cases as I3
    from tests import inception_cases as IC
    I3.bind_kernels(lib)
    IC.bind_kernels(lib)
    dev, out = torch.device("cuda"), {}
    N, T, H, W, Cin, Cout = 8, 8, 14, 14, 96, 208
    stream = torch.cuda.current_stream().cuda_stream
    x3 = torch.randn(N, T, H, W, Cin, device=dev)
    w3 = torch.randn(3, 3, 3, Cin, Cout, device=dev) * 0.02
    x2 = torch.randn(N * T, H, W, 3 * Cin, device=dev)
    w2 = torch.randn(Cout, 3 * Cin, 3, 3, device=dev) * 0.02
    bias = torch.zeros(Cout, device=dev)
    nb3, nb2 = lib.caddy_k_conv3d_weight_bytes(Cin, Cout, 3, 3, 3), lib.caddy_k_igemm_weight_bytes(3 * Cin, Cout, 3, 3)
    assert nb3 == nb2
    p3 = [torch.zeros(nb3 // 4, device=dev) for _ in range(2)]
    p2 = [torch.zeros(nb2 // 4, device=dev) for _ in range(2)]
    bo = torch.zeros(Cout, device=dev)
    assert lib.caddy_k_conv3d_pack(w3.data_ptr(), None, None, None, None, 0.0, bias.data_ptr(), Cin, Cout, 3, 3, 3, p3[0].data_ptr(), p3[1].data_ptr(), bo.data_ptr(), stream) == 0
    assert lib.caddy_k_igemm_pack(w2.data_ptr(), None, None, None, None, 0.0, bias.data_ptr(), 3 * Cin, Cout, 3, 3, p2[0].data_ptr(), p2[1].data_ptr(), bo.data_ptr(), stream) == 0
    o3 = torch.zeros(N, T, H, W, Cout, device=dev)
    o2 = torch.zeros(N * T, H, W, Cout, device=dev)
    macs = N * T * H * W * Cout * 27 * Cin
    for name, prec, k in (("split_f16", 16, 1), ("exact_fp32", 0, 0)):
        a3 = I3.Conv3dArgs(x3.data_ptr(), T * H * W * Cin, Cin, Cin, T, H, W, N, T, H, W, 3, 3, 3, 1, 1, 1, 1, 1, 1, p3[k].data_ptr(), 3, 0, Cout, bo.data_ptr(), 1,
                           o3.data_ptr(), T * H * W * Cout, Cout, prec, None)
        a2 = IC.IgemmArgs(x2.data_ptr(), H * W * 3 * Cin, 3 * Cin, 3 * Cin, H, W, N * T, H, W, 3, 3, 1, 1, 1, p2[k].data_ptr(), 9, 0, Cout, bo.data_ptr(), 1,
                          o2.data_ptr(), H * W * Cout, Cout, prec, None)
        def run3():
            assert lib.caddy_k_conv3d_igemm(C.byref(a3), stream) == 0
        def run2():
            assert lib.caddy_k_conv_igemm(C.byref(a2), stream) == 0
        t3, t2 = _time(run3, repeats), _time(run2, repeats)
        out[name] = {"conv3d_tmacs": macs / t3 / 1e12, "conv2d_equal_mnk_tmacs": macs / t2 / 1e12, "ratio": t2 / t3, "conv3d_us": t3 * 1e6, "conv2d_us": t2 * 1e6}
    return out


def main():
    from playablevideogeneration_amd import metrics as M
    from tests import i3d_cases as I3
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P = I3.make_i3d_params()
    videos = I3.seeded_videos(a.videos, a.frames, a.size, a.size, seed=1).cuda()
    ctx = M._cached_fvd(videos, P, None)
    macs = ctx.lib.caddy_fvd_macs_per_video(a.frames, a.size, a.size, 1)
    res = {"bench": "fvd_i3d_embeddings", "videos": a.videos, "frames": a.frames, "size": a.size, "max_videos": ctx.max_videos, "gmac_per_video": macs / 1e9,
           "workspace_gib": ctx.ws_bytes / 2 ** 30}
    for name, prec in (("split_f16", 16), ("exact_fp32", 0)):
        ctx.set_precision(prec)
        ctx(videos)                                                 # warm-up
        ctx.stage_times(on=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.repeats):
            ctx(videos)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.repeats
        ms = ctx.stage_times(on=False, read=True)
        res[name] = {"videos_per_s": a.videos / dt, "seconds": dt, "trunk_tmacs": macs * a.videos / dt / 1e12, "last_chunk_videos": ctx.last_videos,
                     "last_chunk_stage_ms": dict(zip(("input_stage", "stem", "mixed_3", "mixed_4", "mixed_5_head"), ms)), "fallback_layers": ctx.fallback_layers()}
    res["mixed_4b_3x3x3"] = layer_rates(ctx.lib)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
