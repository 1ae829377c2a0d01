"""Measurements of the evaluation example sheets (csrc/sheets.hip: caddy_sheet_examples) on the MI355X; writes profiles/example_sheets.md.

    device   the four sheets of one BAIR-size batch (B = 8, T = 16, 256 x 256: observations_r0 / r1 / r2 and the motion-weighted sheet): device events around back-to-back
             calls of the C entry point on preallocated buffers (the time per sheet on the stream: memset + reduction + compose), and the bytes the algorithm must move over
             that time -- both launches read channels 0..2 of the observations and the reconstruction once each, the compose launch writes the image.
    copy     in the same run, a device-to-device copy that moves the same number of bytes (half read, half written), timed the same way.
    host     in the same run, the host restatement of the reference's path (tests/example_sheet_cases.py: F.interpolate, the range checks, the mask, the colour lookup, make_grid,
             astype(uint8)) on the same tensors, from device tensors to the uint8 image, wall clock; and ExampleSheets.examples end to end (image on the host) beside it.

    Usage:  python tools/bench_example_sheets.py [--out profiles/example_sheets.md] [--reps 5] [--calls 1000] [--host-reps 3]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from playablevideogeneration_amd import example_sheets as ES  # noqa: E402
from tests import example_sheet_cases as SC  # noqa: E402


def spread(xs):
    return f"{statistics.median(xs):.4g} (min {min(xs):.4g}, max {max(xs):.4g}, n = {len(xs)})"


def events_ms(fn, calls, reps, warmup=10):
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


def wall_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "example_sheets.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the measurements need the MI355X"
    B, T, H = args.batch, args.frames, args.size
    g = torch.Generator().manual_seed(0)
    obs = (torch.rand(B, T, 3, H, H, generator=g) * 2 - 1).cuda()
    recs = [(torch.rand(B, T - 1, 3, H >> r, H >> r, generator=g) * 2 - 1).cuda() for r in range(3)]
    s = ES.ExampleSheets(2 * B, T, colour_table=SC.LUT)
    s._stream()
    sheets = [(f"observations_r{r}", recs[r], False) for r in range(3)] + [("motion_weighted_observations_", recs[0], True)]
    lines = ["# Evaluation example sheets (csrc/sheets.hip: caddy_sheet_examples) on the MI355X", "",
             f"Written by `tools/bench_example_sheets.py` ({torch.cuda.get_device_name(0)}); B = {B}, T = {T}, {H} x {H}, reconstructions of T - 1 frames; every figure is the median of "
             "repeated timings after a warm-up, with the smallest and the largest beside it.", "",
             "## Device time per sheet", "",
             "Time per call of `caddy_sheet_examples` on the stream (device events around back-to-back calls on preallocated buffers: the memset of the flag words, the reduction "
             "launch and the compose launch) and the bytes the algorithm must move over it (each launch reads channels 0..2 of the observations and the reconstruction once, the "
             "compose launch writes the image); `copy` is a device-to-device `Tensor.copy_` moving the same number of bytes, half read and half written, timed the same way in the "
             "same run.", "",
             "| sheet | image | bytes moved | sheet ms, median (min, max) | sheet GB/s | copy ms, median (min, max) | copy GB/s | sheet / copy |", "|---|---|---|---|---|---|---|---|"]
    total = 0.0
    for name, rec, weighted in sheets:
        h, w = rec.shape[-2:]
        shape = ES.sheet_shape(2 * B, T, h, w)
        out = torch.empty(*shape, dtype=torch.uint8, device="cuda")
        moved = 2 * 4 * (B * T * 3 * H * H + rec.numel()) + out.numel()
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def call():
            s._check(s.lib.caddy_sheet_examples(s.ctx, obs.data_ptr(), B, T, 3, H, H, rec.data_ptr(), T - 1, h, w, int(weighted), 0.0, s.lut.data_ptr(), out.data_ptr()))
        ts = events_ms(call, args.calls, args.reps)
        tc = events_ms(lambda: dst.copy_(src), args.calls, args.reps)
        st = s.stats()
        assert st["mapped_gt"] and st["mapped_rec"] and st["saturated"] == 0 and st["nan"] == 0 and not st["mask_invalid"], st
        ms, mc = statistics.median(ts), statistics.median(tc)
        total += ms
        lines.append(f"| {name} | {shape[0]} x {shape[1]} | {moved / 1e6:.1f} MB | {spread(ts)} | {moved / ms / 1e6:.0f} | {spread(tc)} | {moved / mc / 1e6:.0f} | {ms / mc:.2f} |")
    lines += ["", f"The four sheets together: {total:.4g} ms of stream time (sum of the medians).", "",
              "## Against the host path", "",
              "Wall clock, from the device tensors of the forward pass to the four uint8 images on the host, device synchronised before and after: `host` is the restatement of the "
              "reference's path (`tests/example_sheet_cases.expected_examples` on the downloaded tensors: `F.interpolate`, the range checks, the mask, the colour lookup, `make_grid`, "
              "`astype(uint8)`; the reference does its tensor arithmetic on the GPU and its colouring on the host a frame at a time, which this restatement does not imitate), "
              "`device` is `ExampleSheets.examples` (two launches and the download of the image) for the same four sheets.  The images of the two paths were compared: " ]
    same = True
    for name, rec, weighted in sheets:
        same &= bool(np.array_equal(s.examples(obs, rec, weighted=weighted), SC.expected_examples(obs.cpu(), rec.cpu(), weighted)["image"]))
    lines[-1] += "identical." if same else "DIFFERENT."
    th = wall_ms(lambda: [SC.expected_examples(obs.cpu(), rec.cpu(), weighted) for _, rec, weighted in sheets], args.host_reps)
    td = wall_ms(lambda: [s.examples(obs, rec, weighted=weighted) for _, rec, weighted in sheets], max(args.host_reps, 5))
    lines += ["", "| path | ms for the four sheets, median (min, max) |", "|---|---|", f"| host (restated reference path) | {spread(th)} |", f"| device (`ExampleSheets`) | {spread(td)} |", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
