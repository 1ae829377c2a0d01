"""Throughput of the FID feature network (metrics.InceptionFeatures, csrc/fid.hip) on the MI355X:  python tools/bench_fid.py [--frames 240] [--size 256] [--out FILE]

Prints one JSON line: frames/s on `frames` frames of size x size (resized to 299 x 299) in both arithmetics, steady state (one warm-up call, then the mean of `--repeats`
calls), the per-stage times of the last chunk (input stage, stem, 35 x 35, 17 x 17, 8 x 8), the achieved TFLOP/s against the peak bench.py uses for the arithmetic, and the
frames/s of the plain-torch fp32 restatement on the CPU as the baseline."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MATRIX_PEAK_TFLOPS, MFMA16_DENSE_PEAK_TFLOPS, SPLIT_PRODUCTS = 157.3, 2500.0, 3      # as bench.py


def main():
    from playablevideogeneration_amd import metrics as M
    from tests import inception_cases as IC
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--max-frames", type=int, default=M.FID_FRAMES_256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P = IC.make_inception_params()
    frames = IC.seeded_frames(a.frames, a.size, a.size, seed=1).cuda()
    ctx = M.InceptionFeatures(a.size, a.size, min(a.max_frames, a.frames), P)
    macs = ctx.lib.caddy_fid_macs_per_frame(a.size, a.size, 1)
    res = {"bench": "fid_inception_features", "frames": a.frames, "size": a.size, "max_frames": ctx.max_frames, "gmac_per_frame": macs / 1e9,
           "workspace_gib": ctx.ws_bytes / 2 ** 30}
    for name, prec, peak in (("split_f16", 16, MFMA16_DENSE_PEAK_TFLOPS / SPLIT_PRODUCTS), ("exact_fp32", 0, FP32_MATRIX_PEAK_TFLOPS)):
        ctx.set_precision(prec)
        ctx(frames)                                                 # warm-up
        ctx.stage_times(on=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.repeats):
            ctx(frames)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.repeats
        ms = ctx.stage_times(on=False, read=True)
        tf = 2 * macs * a.frames / dt / 1e12
        res[name] = {"frames_per_s": a.frames / dt, "seconds": dt, "tflops": tf, "peak_tflops": peak, "frac_of_peak": tf / peak, "last_chunk_frames": ctx.last_frames,
                     "last_chunk_stage_ms": dict(zip(("input_stage", "stem", "35x35", "17x17", "8x8"), ms)), "fallback_layers": ctx.fallback_layers()}
    cpu = frames[:a.cpu_frames].cpu()
    IC.restated_features(cpu[:2], P, torch.float32)
    t0 = time.perf_counter()
    IC.restated_features(cpu, P, torch.float32)
    res["cpu_restatement_fp32_frames_per_s"] = a.cpu_frames / (time.perf_counter() - t0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
