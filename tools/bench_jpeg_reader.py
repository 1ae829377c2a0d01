"""Measurements of the device-side JPEG reader (csrc/jpeg_read.hip: caddy_jpeg_decode) on the MI355X; writes profiles/jpeg_reader.md.

The workload is B = 8 sequences of T = 16 frames of 256 x 256 (128 files) at quality 90, as Pillow writes them: model-like frames (smooth content plus a little noise) and
uniform noise, 4:4:4 and 4:2:0, without restart markers (one entropy stream, one lane) and with one restart interval per MCU row (32 or 16 intervals, as many lanes).  For
each, in the same run:

    decode   device events around back-to-back calls of the C entry point on preallocated buffers: the files and their offsets on the device in, uint8 frames and the status out
             (three launches per chunk of 128 images)
    floor    a device-to-device copy of the output bytes (n H W 3), timed the same way
    host     the same files through Pillow (Image.open + convert("RGB")) on one thread and on a pool of 16 threads (Pillow's decoder releases the interpreter lock), wall clock
    bytes    what JpegDecoder sends to the device (the files and their offsets) against the raw uint8 frames the host-decode path sends

No figure here is a pass / fail condition; where the host pool is faster the table says so.

    Usage:  python tools/bench_jpeg_reader.py [--out profiles/jpeg_reader.md] [--reps 5] [--calls 3]
"""
import argparse
import io
import os
import statistics
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from playablevideogeneration_amd import jpeg_reader as JR  # noqa: E402
from playablevideogeneration_amd.frame_pipeline import MAP_ALWAYS, cached_writer  # noqa: E402
from tools.bench_png_writer import events_ms, frames_of, spread, wall_ms  # noqa: E402


def pillow_decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB")).copy()


def pillow_save(image, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def workloads(n, size, quality):
    """[(name, [files])]"""
    writer = cached_writer(size, size, n, None, torch.device("cuda"))
    out = []
    for content in ("model-like", "noise"):
        frames = writer(frames_of(content, n, size, size).cuda()[None], map=MAP_ALWAYS)[0].cpu().numpy()
        for label, sub in (("4:4:4", 0), ("4:2:0", 2)):
            row = -(-size // (8 if sub == 0 else 16))
            for rs_label, kw in (("no restarts", {}), ("one interval per MCU row", {"restart_marker_blocks": row})):
                out.append((f"{content}, {label}, {rs_label}", [pillow_save(f, quality=quality, subsampling=sub, **kw) for f in frames]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_reader.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the measurements need the MI355X"
    n, size = args.frames, args.size
    pool = ThreadPoolExecutor(16)
    lines = ["# Device-side JPEG reader (csrc/jpeg_read.hip: caddy_jpeg_decode) on the MI355X", "",
             f"Written by `tools/bench_jpeg_reader.py` ({torch.cuda.get_device_name(0)}); {n} files of {size} x {size} at quality {args.quality} as Pillow writes them; every "
             "figure is the median of repeated timings after a warm-up, with the smallest and the largest beside it.  Entropy decoding is serial per restart interval: one wave "
             "per image, one lane per interval, so a file without restart markers keeps one lane of its wave busy and a file with one interval per MCU row 32 (4:4:4) or 16 "
             "(4:2:0); the IDCT and the colour stage are block- and pixel-parallel.  No figure is a pass / fail condition.", "",
             "`decode` is the time per call of `caddy_jpeg_decode` on the stream (device events around back-to-back calls on preallocated buffers, the files on the device in, "
             "uint8 frames out); `floor` is a device-to-device `Tensor.copy_` of the output bytes timed the same way; `Pillow` is `Image.open` + `convert(\"RGB\")` of the same "
             "files on the host, wall clock, on one thread and on a pool of 16; `sent` is what `JpegDecoder` copies to the device (the files and their offsets) against the raw "
             "uint8 frames; `frames` says whether the device's frames equal Pillow's byte for byte.", "",
             "| files | decode ms, median (min, max) | floor ms | Pillow, 1 thread, ms | Pillow, 16 threads, ms | decode / Pillow 16 | sent to the device | of the raw bytes | frames |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, files in workloads(n, size, args.quality):
        H = W = size
        raw = n * H * W * 3
        dec = JR.JpegDecoder(H, W, n)
        blob, offsets = JR.pack_files(files)
        d_blob = torch.from_numpy(blob).cuda()
        d_off = torch.from_numpy(offsets.astype(np.int32)).cuda()
        frames = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        dec._stream()

        def call():
            dec._check(dec.lib.caddy_jpeg_decode(dec.ctx, d_blob.data_ptr(), d_off.data_ptr(), n, frames.data_ptr(), status.data_ptr()))
        td = events_ms(call, args.calls, args.reps, warmup=1)
        same = bool(status.eq(0).all()) and np.array_equal(frames.cpu().numpy(), np.stack([pillow_decode(f) for f in files]))
        src, dst = frames.reshape(-1), torch.empty(raw, dtype=torch.uint8, device="cuda")
        tf = events_ms(lambda: dst.copy_(src), 20, args.reps)
        t1, t16 = [], []
        for _ in range(args.reps):
            t1.append(wall_ms(lambda: [pillow_decode(f) for f in files]))
            t16.append(wall_ms(lambda: list(pool.map(pillow_decode, files))))
        sent = blob.size + 4 * offsets.size
        lines.append(f"| {name} | {spread(td)} | {statistics.median(tf):.4g} | {spread(t1)} | {spread(t16)} | {statistics.median(td) / statistics.median(t16):.2f} | "
                     f"{sent / 1e6:.2f} MB | {100.0 * sent / raw:.1f} % | {'equal' if same else 'DIFFERENT'} |")
        del dec, d_blob, frames, dst
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
