"""Measurements of the frame writer (csrc/frames.hip: caddy_frames_write) and of what is built on it, on the MI355X; writes profiles/frame_writer.md.

    kernel      256 x 256 frames, (B, T) = (8, 16) and 64 frames (one batched roll-out step), map 1 (one launch) and map 2 (reduction + writer), uint8 output: device events
                around back-to-back calls of the C entry point on preallocated buffers (the time per call on the stream, not a profiler's kernel time), and the bytes the
                algorithm moves over that time.  Beside it, in the same run, a device-to-device copy that moves the same number of bytes (half read, half written).
    builder     EvaluationDatasetBuilder.build(write=False) per batch with evaluation_dataset.device_quantise true against false: same process, same model, alternating.
    end to end  wall time of `evaluate-model` against `build-dataset` + `evaluate` on a synthetic on-disk test split (generic evaluator, frame metrics only).

    Usage:  python tools/bench_frame_writer.py [--out profiles/frame_writer.md] [--reps 5] [--calls 200] [--videos 16] [--size 256]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from playablevideogeneration_amd import drivers as D  # noqa: E402
from playablevideogeneration_amd import frame_pipeline as FP  # noqa: E402
from playablevideogeneration_amd import model_evaluation as ME  # noqa: E402
from playablevideogeneration_amd import video_dataset as VD  # noqa: E402
from playablevideogeneration_amd.evaluation_dataset_builder import EvaluationVideo  # noqa: E402
from tests.test_host_api_emu import _config  # noqa: E402


def spread(xs):
    return f"{statistics.median(xs):.4g} (min {min(xs):.4g}, max {max(xs):.4g}, n = {len(xs)})"


def events_ms(fn, calls, reps, warmup=20):
    """ms per call: device events around `calls` back-to-back calls, `reps` times after a warm-up"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def kernel_section(lines, calls, reps):
    H = W = 256
    lines += ["## Kernel", "",
              "Time per call of `caddy_frames_write` on the stream (device events around back-to-back calls on preallocated buffers, uint8 output) and the bytes the algorithm moves "
              "(12 read + 3 written per pixel; map 2 reads the 12 twice) over it; `copy` is a device-to-device `Tensor.copy_` moving the same number of bytes, half read and half "
              "written, timed the same way in the same run.", "",
              "| frames | map | bytes moved | writer ms, median (min, max) | writer GB/s | copy ms, median (min, max) | copy GB/s | writer / copy |", "|---|---|---|---|---|---|---|---|"]
    for B, T in ((8, 16), (64, 1)):
        rec = torch.rand(B, T, 3, H, W, device="cuda") * 2 - 1
        u8 = torch.empty(B, T, H, W, 3, dtype=torch.uint8, device="cuda")
        w = FP.FrameWriter(H, W, B * T)
        w._stream()
        for map in (1, 2):
            moved = B * T * H * W * (15 if map == 1 else 27)
            src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)

            def call():
                w._check(w.lib.caddy_frames_write(w.ctx, rec.data_ptr(), B, T, None, 0, map, u8.data_ptr(), None))
            tw = events_ms(call, calls, reps)
            tc = events_ms(lambda: dst.copy_(src), calls, reps)
            assert w.stats() == {"mapped": True, "saturated": 0, "nan": 0}
            mw, mc = statistics.median(tw), statistics.median(tc)
            lines.append(f"| {B} x {T} | {map} | {moved / 1e6:.1f} MB | {spread(tw)} | {moved / mw / 1e6:.0f} | {spread(tc)} | {moved / mc / 1e6:.0f} | {mw / mc:.2f} |")
    lines.append("")


def synthetic_split(root, videos, frames, size, seed=0):
    """train / val / test folders in the on-disk video format; smooth frames with a moving block, so that the PNGs stay small"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    for split, n in (("train", 1), ("val", 1), ("test", videos)):
        for vi in range(n):
            fr = np.zeros((frames, size, size, 3), np.uint8)
            phase = rng.randint(0, 255, 3)
            for t in range(frames):
                for c in range(3):
                    fr[t, :, :, c] = (xx * (c + 1) + yy * 2 + phase[c] + 3 * t) % 256
                x0 = (11 * t + 17 * vi) % (size - 32)
                fr[t, size // 2:size // 2 + 16, x0:x0 + 32] = 255
            EvaluationVideo(fr, [int(rng.randint(0, 3)) for _ in range(frames)], [0.0] * frames, [{} for _ in range(frames)], [False] * frames).save(
                os.path.join(root, split, f"{vi:05d}"))


def training_config(tmp, size, frames, batch):
    cfg = _config(res=(size // 8, size // 8))
    cfg["data"].update({"data_root": os.path.join(tmp, "data")})
    cfg["evaluation_dataset"] = {"builder": "playablevideogeneration_amd.evaluation_dataset_builder", "ground_truth_observations_init": 2}
    cfg["model"]["representation_network"]["target_input_size"] = [size, size]
    cfg["logging"] = {"output_root": os.path.join(tmp, "out"), "save_root": os.path.join(tmp, "ckpt"), "run_name": "bench"}
    cfg["training"]["batching"].update({"batch_size": batch, "skip_frames": 0, "num_workers": 0, "observations_count": frames, "observations_count_start": frames})
    cfg["evaluation"] = {"batching": {"batch_size": batch, "observations_count": frames, "observation_stacking": 1, "skip_frames": 0, "num_workers": 0}}
    return D.finish_configuration(cfg)


class Quiet:
    def print(self, *a, **k):
        pass


def builder_section(lines, cfg, model, datasets, reps):
    from playablevideogeneration_amd import evaluation_dataset_builder as EB
    batches = -(-len(datasets["test"]) // cfg["evaluation"]["batching"]["batch_size"])
    times = {False: [], True: []}
    for rep in range(reps + 1):      # (the first round warms both paths up and is dropped)
        for on in (False, True):
            c = dict(cfg, evaluation_dataset=dict(cfg["evaluation_dataset"], device_quantise=on))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            EB.builder(c, datasets["test"], Quiet()).build(model, write=False)
            torch.cuda.synchronize()
            if rep:
                times[on].append((time.perf_counter() - t0) / batches * 1e3)
    b = cfg["evaluation"]["batching"]
    size = cfg["model"]["representation_network"]["target_input_size"][0]
    lines += ["## Builder", "",
              f"`EvaluationDatasetBuilder.build(write=False)`, ms per batch of {b['batch_size']} sequences x {b['observations_count']} frames of {size} x {size} (decoding, the roll-out, "
              "the quantisation, the copy to the host; wall clock around the whole call, device synchronised), the two settings alternating in one process on one model.", "",
              "| evaluation_dataset.device_quantise | ms per batch, median (min, max) |", "|---|---|",
              f"| false (host) | {spread(times[False])} |", f"| true (frame writer) | {spread(times[True])} |", ""]


def end_to_end_section(lines, cfg, model, datasets, tmp, reps):
    import yaml
    ref_root = os.path.join(cfg["data"]["data_root"], "test")
    ev = {"logging": {"run_name": "bench_eval", "output_root": os.path.join(tmp, "results")},
          "data": {"target_input_size": cfg["model"]["representation_network"]["target_input_size"], "actions_count": cfg["data"]["actions_count"]},
          "reference_data": {"data_root": ref_root, "crop": None},
          "generated_data": {"data_root": cfg["logging"]["evaluation_dataset_directory"], "crop": None},
          "evaluation": {"batching": dict(cfg["evaluation"]["batching"])}}
    path = os.path.join(tmp, "eval.yaml")
    yaml.safe_dump(ev, open(path, "w"))
    times = {"two": [], "build": [], "one": []}
    last = {}
    for rep in range(reps + 1):      # (the first round warms both routes up and is dropped)
        shutil.rmtree(cfg["logging"]["evaluation_dataset_directory"])
        os.makedirs(cfg["logging"]["evaluation_dataset_directory"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D.build_dataset_loop(cfg, model, datasets, Quiet())
        t1 = time.perf_counter()
        ev_cfg = D.load_evaluation_configuration(path)
        last["two"] = D.evaluate_loop(ev_cfg, Quiet())
        t2 = time.perf_counter()
        last["one"] = ME.evaluate_model_loop(cfg, model, datasets, Quiet())
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if rep:
            times["build"].append(t1 - t0); times["two"].append(t2 - t0); times["one"].append(t3 - t2)
    same = last["one"].keys() == last["two"].keys() and all(last["one"][k] == last["two"][k] for k in last["one"])
    b = cfg["evaluation"]["batching"]
    n = len(datasets["test"])
    lines += ["## End to end", "",
              f"Wall time in seconds on a synthetic on-disk test split of {n} videos of {b['observations_count']} frames, batches of {b['batch_size']}, generic evaluator with the frame "
              "metrics (no pretrained networks), the routes alternating in one process on one model.  The two routes returned " +
              ("identical metric dicts." if same else "DIFFERENT metric dicts."), "",
              "| route | seconds, median (min, max) |", "|---|---|",
              f"| `build-dataset` + `evaluate` | {spread(times['two'])} |", f"| of which `build-dataset` | {spread(times['build'])} |",
              f"| `evaluate-model` | {spread(times['one'])} |", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_writer.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--videos", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the measurements need the MI355X"
    lines = ["# Frame writer (csrc/frames.hip: caddy_frames_write) on the MI355X", "",
             f"Written by `tools/bench_frame_writer.py` ({torch.cuda.get_device_name(0)}); every figure is the median of repeated timings after a warm-up, with the smallest and the "
             "largest beside it.", ""]
    kernel_section(lines, args.calls, args.reps)
    tmp = tempfile.mkdtemp(prefix="frame_writer_bench_")
    try:
        synthetic_split(os.path.join(tmp, "data"), args.videos, args.frames, args.size)
        cfg = training_config(tmp, args.size, args.frames, args.batch)
        datasets = VD.build_datasets(cfg)
        model = D.build_model(cfg)
        builder_section(lines, cfg, model, datasets, args.reps)
        end_to_end_section(lines, cfg, model, datasets, tmp, max(2, args.reps // 2))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
