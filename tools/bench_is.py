"""Throughput of the Inception Score's classifier (metrics.InceptionProbabilities, csrc/fid.hip) on the MI355X:  python tools/bench_is.py [--frames 240] [--size 256] [--out FILE]

Prints one JSON line: frames/s of caddy_is_probabilities on `frames` frames of size x size (resized to 299 x 299) in chunks of `--max-frames` in both arithmetics, steady state
(one warm-up call, then the mean of `--repeats` calls), the per-stage times of the last chunk (input stage, stem, 35 x 35, 17 x 17, 8 x 8, fc + softmax), and the times of the
fc launch (k_conv_igemm, M = max_frames, K = 2048, Cout = 1000) and of k_is_softmax alone.  With --fid the same frames also go through metrics.InceptionFeatures (the FID
flavour of the same graph) for comparison; tools/bench_fid.py run against another build of the library gives that build's figure."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("input_stage", "stem", "35x35", "17x17", "8x8", "fc_softmax")


def time_launch(launch, repeats=20):
    """mean milliseconds of `launch()` between two events on the current stream, after one warm-up"""
    launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats


def head_times(lib, n):
    """fc as the context launches it (both arithmetics) and the softmax, on n rows"""
    from tests import inception_cases as IC
    from tests import inception_score_cases as SC
    SC.bind_kernels(lib)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, 2048, generator=g).cuda()
    w = (torch.randn(1000, 2048, generator=g) * 0.02).cuda()
    b = torch.zeros(1000).cuda()
    nb = lib.caddy_k_igemm_weight_bytes(2048, 1000, 1, 1)
    w32, w16, bo = torch.zeros(nb // 4).cuda(), torch.zeros(nb // 4).cuda(), torch.zeros(1000).cuda()
    assert lib.caddy_k_igemm_pack(w.data_ptr(), None, None, None, None, 0.0, b.data_ptr(), 2048, 1000, 1, 1, w32.data_ptr(), w16.data_ptr(), bo.data_ptr(), st) == 0
    z, p = torch.zeros(n, 1000).cuda(), torch.zeros(n, 1000).cuda()
    out = {}
    for name, prec, wp in (("fc_split_f16_ms", 16, w16), ("fc_exact_fp32_ms", 0, w32)):
        a = IC.IgemmArgs(x.data_ptr(), 2048, 2048, 2048, 1, 1, n, 1, 1, 1, 1, 1, 0, 0, wp.data_ptr(), 64, 0, 1000, bo.data_ptr(), 0, z.data_ptr(), 1000, 1000, prec, None)
        out[name] = time_launch(lambda: lib.caddy_k_conv_igemm(C.byref(a), st))
    out["softmax_ms"] = time_launch(lambda: lib.caddy_k_is_softmax(z.data_ptr(), p.data_ptr(), n, 1000, 1000, 1000, st))
    return out


def run(ctx, frames, repeats, stages):
    ctx(frames)                                                 # warm-up
    ctx.stage_times(on=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        ctx(frames)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / repeats
    ms = ctx.stage_times(on=False, read=True)
    n = frames.shape[0]
    return {"frames_per_s": n / dt, "seconds": dt, "last_chunk_frames": ctx.last_frames, "last_chunk_stage_ms": dict(zip(stages, ms)), "fallback_layers": ctx.fallback_layers()}


def main():
    from playablevideogeneration_amd import metrics as M
    from tests import inception_cases as IC
    from tests import inception_score_cases as SC
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--max-frames", type=int, default=M.FID_FRAMES_256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fid", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P = SC.make_is_params(resize=True)
    frames = IC.seeded_frames(a.frames, a.size, a.size, seed=1).cuda()
    ctx = M.InceptionProbabilities(a.size, a.size, min(a.max_frames, a.frames), P)
    res = {"bench": "is_inception_probabilities", "frames": a.frames, "size": a.size, "max_frames": ctx.max_frames,
           "gmac_per_frame": ctx.lib.caddy_is_macs_per_frame(a.size, a.size, 1) / 1e9, "workspace_gib": ctx.ws_bytes / 2 ** 30}
    for name, prec in (("split_f16", 16), ("exact_fp32", 0)):
        ctx.set_precision(prec)
        res[name] = run(ctx, frames, a.repeats, STAGES)
    res["head"] = dict(head_times(ctx.lib, ctx.max_frames), rows=ctx.max_frames)
    if a.fid:
        del ctx
        fid = M.InceptionFeatures(a.size, a.size, min(a.max_frames, a.frames), {k: v for k, v in P.items() if not k.startswith("fc.")})
        for name, prec in (("fid_split_f16", 16), ("fid_exact_fp32", 0)):
            fid.set_precision(prec)
            res[name] = run(fid, frames, a.repeats, STAGES[:5])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
