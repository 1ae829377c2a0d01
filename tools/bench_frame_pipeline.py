"""Measurements of the device-side frame pipeline (csrc/frames.hip, frame_pipeline.py) on the GPU; writes a markdown record (default profiles/frame_pipeline.md).

    1. kernel   device time of caddy_frames_to_observations from events, against the bytes the call must move (fp32 written + uint8 read once) over the HBM rate
    2. host     wall time per batch from a collated batch to a device-resident tuple through DevicePrefetcher: fp32 `Batch` against uint8 `RawBatch`, alternating,
                plus what a DataLoader worker spends per sample and per collate, and the bytes over the bus
    3. step     `train_epoch` step time at the BAIR geometry from a seeded on-disk dataset it writes itself, `data.device_transforms` off and on, alternating; the
                spread of the repeated "off" runs is recorded beside the difference

    Usage:  python tools/bench_frame_pipeline.py [--out profiles/frame_pipeline.md] [--iters 20] [--steps 12] [--workers 8] [--skip-step]
"""
import argparse
import importlib
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from playablevideogeneration_amd import batching as BT  # noqa: E402
from playablevideogeneration_amd import configs  # noqa: E402
from playablevideogeneration_amd import frame_pipeline as FP  # noqa: E402
from playablevideogeneration_amd import video_dataset as VD  # noqa: E402
from playablevideogeneration_amd.prefetch import DevicePrefetcher  # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12      # bytes / s: spec and what streaming kernels reach on the MI355X
FBN_APPLY_RATE = 46.56e6 / 13.21e-6            # k_map<FBnApply, true>: bytes per launch (profiles/r06_pmc_traffic_bair256_t16_b8_erad.json) over its mean time
                                               # (profiles/r06_kernel_stats_bair256_t16_b8_timed_step_only.txt)

# (name, source h, source w, crop, target (W, H), B, T, S)
GEOMETRIES = [
    ("BAIR 256x256, no resize", 256, 256, None, (256, 256), 8, 16, 1),
    ("BAIR 64x64 -> 256x256", 64, 64, None, (256, 256), 8, 16, 1),
    ("Tennis 256x96, no resize, S=4", 96, 256, None, (256, 96), 8, 16, 4),
    ("Tennis 960x540 -> 256x96, S=4", 540, 960, None, (256, 96), 8, 16, 4),
]


def median_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def kernel_part(iters):
    rows = []
    for name, h, w, crop, size, B, T, S in GEOMETRIES:
        _, stacks = BT.observation_indices(S - 1, T, 0, S)                      # a sample's stacks over its T + S - 1 distinct frames
        per = T + S - 1
        slot = torch.tensor([[[b * per + i for i in st] for st in stacks] for b in range(B)], dtype=torch.int32)
        frames = torch.randint(0, 256, (B * per, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        slot_dev = slot.cuda()
        pipe = FP.FramePipeline(h, w, crop, size, B * per, 0)
        out = pipe(frames, slot_dev)
        lib, args = pipe.lib, (pipe.ctx, frames.data_ptr(), int(frames.shape[0]), slot_dev.data_ptr(), int(slot.numel()), 0, out.data_ptr())
        pipe._stream()
        med, lo, hi = median_ms(lambda: lib.caddy_frames_to_observations(*args), iters)
        written, read = out.numel() * 4, frames.numel()
        least = (written + read) / HBM_ACHIEVABLE * 1e3
        rate = (written + read) / (med * 1e-3)
        rows.append((name, pipe.plan(), frames.shape[0], slot.numel(), written, read, med, lo, hi, least, rate))
        del pipe, frames, out
    return rows


def write_dataset(root, videos, frames, h, w, seed=0):
    """seeded videos in the on-disk format: blocky colour fields plus a little noise (they compress like frames, not like noise)"""
    from playablevideogeneration_amd.evaluation_dataset_builder import EvaluationVideo
    rng = np.random.RandomState(seed)
    for v in range(videos):
        coarse = rng.randint(0, 256, (frames, h // 16, w // 16, 3))
        fr = np.kron(coarse, np.ones((1, 16, 16, 1), dtype=np.int64)) + rng.randint(-4, 5, (frames, h, w, 3))
        EvaluationVideo(np.clip(fr, 0, 255).astype(np.uint8), [int(a) for a in rng.randint(0, 7, frames)], [0.0] * frames, [{} for _ in range(frames)], [False] * frames).save(
            os.path.join(root, f"{v:05d}"))


def host_part(root, wl, rounds):
    B, T, S = wl["batch"], wl["seq_len"], wl["stacking"]
    batching = {"batch_size": B, "observations_count": T, "observation_stacking": S, "skip_frames": 0}
    size = (wl["width"], wl["height"])
    tf = VD.final_transform({"data": {"crop": None}, "model": {"representation_network": {"target_input_size": list(size)}}})
    host_ds = VD.VideoDataset(root, batching, tf)
    raw_ds = VD.VideoDataset(root, batching, VD.raw_frame_spec(None, size, 0))
    idx = [int(i) for i in torch.randperm(len(host_ds), generator=torch.Generator().manual_seed(0))[:4 * B]]
    res = {}
    for name, ds in (("fp32", host_ds), ("uint8", raw_ds)):
        t0 = time.perf_counter()
        els = [ds[i] for i in idx]
        t1 = time.perf_counter()
        collate = BT.collate_fn_for(els[0])
        batches = [collate(els[k * B:(k + 1) * B]) for k in range(4)]
        t2 = time.perf_counter()
        tensors = [batches[0].observations] if name == "fp32" else [batches[0].frames, batches[0].slot_src]
        res[name] = {"item_ms": (t1 - t0) / len(idx) * 1e3, "collate_ms": (t2 - t1) / 4 * 1e3, "batches": batches,
                     "bus_bytes": sum(t.numel() * t.element_size() for t in tensors + [batches[0].actions, batches[0].rewards, batches[0].dones])}
    dev = torch.device("cuda", 0)
    want = [b.to_tuple(cuda=False)[0] for b in res["fp32"]["batches"]]
    got = [t[0].cpu() for t in DevicePrefetcher(res["uint8"]["batches"], dev)]
    same = all(torch.equal(a, b) for a, b in zip(want, got))
    times = {"fp32": [], "uint8": []}
    for _ in range(rounds):                                                      # alternate the two paths; every tuple is waited for, as a consumer would
        for name in ("fp32", "uint8"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for tup in DevicePrefetcher(res[name]["batches"] * 3, dev):
                n += 1
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / n * 1e3)
    for name in times:
        res[name]["stage_ms"] = sorted(times[name][1:])                          # (the first round warms the pinned buffers and the pipeline context)
        del res[name]["batches"]
    res["same_bits"] = same
    return res


def step_part(root, wl, steps, workers, order):
    B, T = wl["batch"], wl["seq_len"]
    from playablevideogeneration_amd.init import random_vgg19_state
    cfg = bench.plugin_config(wl, B, T)
    cfg["training"]["vgg19_weights"] = random_vgg19_state(0)
    cfg["training"]["batching"].update({"num_workers": workers, "skip_frames": 0})
    cfg["data"].update({"data_root": root, "dataset_style": "flat", "dataset_splits": [1.0, 0.0, 0.0], "crop": None})
    cfg["model"]["representation_network"]["target_input_size"] = [wl["width"], wl["height"]]
    cfg["evaluation"] = {"batching": dict(cfg["training"]["batching"])}
    model = getattr(importlib.import_module(cfg["model"]["architecture"]), "model")(cfg).cuda()
    trainer_cls = getattr(importlib.import_module(cfg["training"]["trainer"]), "trainer")
    runs = []
    for on in order:
        cfg["data"]["device_transforms"] = bool(on)
        cfg["training"]["max_steps_per_epoch"] = steps - 1                       # (an epoch ends after max_steps_per_epoch + 1 steps)
        ds = VD.build_datasets(cfg)["train"]
        trainer = trainer_cls(cfg, model, ds, None)
        trainer.global_step = 20000
        model.train()
        torch.manual_seed(0)
        cfg["training"]["max_steps_per_epoch"] = 2
        trainer.train_epoch(model)                                               # warm-up: workers start, kernels load
        cfg["training"]["max_steps_per_epoch"] = steps - 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = trainer.train_epoch(model)
        torch.cuda.synchronize()
        runs.append((bool(on), (time.perf_counter() - t0) / max(1, done) * 1e3, done))
        del trainer, ds
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_pipeline.md"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the measurements need the GPU"
    wl = configs.WORKLOADS["bair256_t16_b8"]
    L = ["# Device-side frame pipeline: measurements", "",
         f"`python tools/bench_frame_pipeline.py --iters {a.iters} --steps {a.steps} --workers {a.workers}` on {torch.cuda.get_device_name(0)}; "
         "every figure below is from that one run.", ""]
    L += ["## 1. Kernel device time (events around the launch, median of %d after 3 warm-up launches)" % a.iters, "",
          "Least time = (fp32 written + uint8 read once) / 6.3 TB/s (the achievable HBM rate; the peak is 8 TB/s).", "",
          "| geometry | frames | slots | rows/block, LDS | written MB | read MB | median us (min .. max) | least us | share of 6.3 TB/s | GB/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name, plan, nf, ns, wr, rd, med, lo, hi, least, rate in kernel_part(a.iters):
        L.append(f"| {name} | {nf} | {ns} | {plan['rows_per_block']}, {plan['lds_bytes']} of {plan['lds_variant']} | {wr / 1e6:.1f} | {rd / 1e6:.1f} | "
                 f"{med * 1e3:.1f} ({lo * 1e3:.1f} .. {hi * 1e3:.1f}) | {least * 1e3:.1f} | {least / med * 100:.0f} % | {rate / 1e9:.0f} |")
    L += ["", f"For comparison `k_map<FBnApply, true>` moves 46.6 MB per launch in 13.2 us in the round-6 profiles: {FBN_APPLY_RATE / 1e9:.0f} GB/s; half of that is "
              f"{FBN_APPLY_RATE / 2e9:.0f} GB/s.", ""]
    root = tempfile.mkdtemp(prefix="frame_pipeline_ds_")
    try:
        t0 = time.perf_counter()
        write_dataset(root, a.videos, 30, wl["height"], wl["width"])
        L += [f"Dataset for parts 2 and 3: {a.videos} seeded videos x 30 frames of {wl['width']} x {wl['height']} PNG, written in {time.perf_counter() - t0:.1f} s.", ""]
        h = host_part(root, wl, a.rounds)
        L += ["## 2. Host time per batch (B = 8, T = 16, 256 x 256), one process", "",
              "| path | DataLoader worker: per sample ms | collate per batch ms | bytes over the bus per batch | collated batch -> device tuple, ms per batch (rounds, sorted) |", "|---|---|---|---|---|"]
        for name, label in (("fp32", "fp32 `Batch` + DevicePrefetcher (the default path)"), ("uint8", "uint8 `RawBatch` + DevicePrefetcher + kernel")):
            r = h[name]
            L.append(f"| {label} | {r['item_ms']:.1f} | {r['collate_ms']:.1f} | {r['bus_bytes'] / 1e6:.1f} MB | {', '.join(f'{t:.1f}' for t in r['stage_ms'])} |")
        L += ["", f"The tuples of the two paths are bit-identical on these batches: {h['same_bits']}.", ""]
        if not a.skip_step:
            order = [0, 1, 0, 1, 0]
            runs = step_part(root, wl, a.steps, a.workers, order)
            off = [ms for on, ms, _ in runs if not on]
            on_ = [ms for on, ms, _ in runs if on]
            spread = max(off) - min(off)
            L += [f"## 3. `train_epoch` step time, bair256_t16_b8 from the on-disk dataset, num_workers = {a.workers}, {a.steps} steps per run after a 3-step warm-up epoch", "",
                  "| run | device_transforms | ms per step |", "|---|---|---|"]
            L += [f"| {i} | {'on' if on else 'off'} | {ms:.1f} |" for i, (on, ms, _) in enumerate(runs)]
            verdict = "not slower beyond the spread" if max(on_) <= max(off) + spread else "SLOWER beyond the spread"
            L += ["", f"off: {min(off):.1f} .. {max(off):.1f} ms (spread {spread:.1f} ms); on: {min(on_):.1f} .. {max(on_):.1f} ms.  Gate (on <= slowest off + spread): {verdict}.", ""]
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
