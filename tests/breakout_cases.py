"""Seeded Breakout-like frames for the platform detector (csrc/detection.hip, metrics.breakout_platform_positions) and a plain-Python restatement of
its scan rule.  tests/golden/breakout_platform.npz holds the reference's positions on these frames (tools/gen_breakout_golden.py), not the frames.

Row `row` of channel 0 of each frame: black, optionally 8-column side walls in the mask colour (142 / 255), optionally a platform of a drawn start and
length, decoy runs of 11 columns, runs that reach the last column, values exactly at the bounds and one float32 ulp outside them, NaN pixels.  The other
rows and channels 1-2 carry uniform noise."""
import numpy as np
import torch

# name -> (B, T, H, W, seed): the evaluation geometry, a tiny frame, W not a multiple of 64 (row 189), W > 256
CASES = {
    "eval_208x160": (2, 6, 208, 160, 1),
    "tiny_16x20": (2, 5, 16, 20, 2),
    "odd_210x200": (2, 4, 210, 200, 3),
    "wide_64x320": (1, 6, 64, 320, 4),
}


def bounds():
    """(row scale, lo, hi, min_run) as the reference computes them: fp32 channel-0 bounds of BreakoutPlatformPosition"""
    lo = float(torch.tensor([100], dtype=torch.float) / 255 - 0.15)
    hi = float(torch.tensor([200], dtype=torch.float) / 255 + 0.15)
    return lo, hi


def platform_row(H):
    return int(188 / 208 * H)


def breakout_frames(B, T, H, W, seed):
    """(B, T, 3, H, W) float32 numpy frames (not clipped to [0, 1]: NaN and out-of-bound values are part of the cases)"""
    rng = np.random.RandomState(seed)
    lo, hi = bounds()
    f32 = np.float32
    inside = [f32(142 / 255), f32(200 / 255), f32(lo), f32(hi), f32(0.5)]
    outside = [f32(0.0), np.nextafter(f32(lo), f32(-1)), np.nextafter(f32(hi), f32(2)), f32(np.nan), f32(1.0), f32(0.1)]
    row = platform_row(H)
    x = rng.uniform(0, 1, size=(B, T, 3, H, W)).astype(np.float32)
    for b in range(B):
        for t in range(T):
            r = np.zeros(W, dtype=np.float32)
            if W >= 40 and rng.rand() < 0.8:                                  # side walls: a short run on the left, a run reaching the last column
                r[:8] = f32(142 / 255)
                r[W - 8:] = f32(142 / 255)
            for _ in range(rng.randint(0, 3)):                                # decoys of 11 columns
                s = rng.randint(0, max(1, W - 11))
                r[s:s + 11] = inside[rng.randint(len(inside))]
                if s + 11 < W:
                    r[s + 11] = outside[rng.randint(len(outside))]
                if s > 0:
                    r[s - 1] = outside[rng.randint(len(outside))]
            if rng.rand() < 0.75:                                             # the platform: 11 .. 24 columns, anywhere (touching a wall or the edge too)
                n = rng.randint(11, min(25, W + 1))
                s = rng.randint(0, W - n + 1)
                r[s:s + n] = inside[rng.randint(len(inside))]
                k = rng.randint(0, 3)                                         # bound values inside it
                r[s + rng.randint(n, size=k)] = [inside[rng.randint(len(inside))] for _ in range(k)]
            for _ in range(rng.randint(0, 3)):                                # single out-of-mask pixels (ulp outside a bound, NaN, ...) anywhere
                r[rng.randint(W)] = outside[rng.randint(len(outside))]
            x[b, t, 0, row] = r
    return x


def positions_restated(frames, row, lo, hi, min_run=12):
    """(B, T, 3, H, W) -> (B, T) int64: the smallest s with m[s], (s == 0 or not m[s - 1]) and m[s .. s + min_run - 1] all set, where m[x] = lo <= v <= hi
    for v = frames[b, t, 0, row, x] and m[W - 1] is False; -1 when there is none"""
    frames = np.asarray(frames)
    B, T, _, _, W = frames.shape
    out = np.full((B, T), -1, dtype=np.int64)
    for b in range(B):
        for t in range(T):
            v = frames[b, t, 0, row]
            m = [bool(lo <= float(v[x]) <= hi) and x != W - 1 for x in range(W)]
            for s in range(W):
                if m[s] and (s == 0 or not m[s - 1]) and s + min_run <= W and all(m[s:s + min_run]):
                    out[b, t] = s
                    break
    return out


# ---- action metrics: seeded inputs (tools/gen_breakout_golden.py records the reference's results on them in tests/golden/action_metrics.npz) ----
def action_cases():
    """name -> (actions, vectors, actions_count)"""
    rng = np.random.RandomState(7)
    out = {}
    a = rng.randint(0, 3, size=(6, 9))                                        # Breakout-like: integer platform movements, -1 detections left in
    out["breakout"] = (a, ((a - 1) * 4 + rng.randint(-3, 4, size=a.shape))[..., None].astype(np.int64), 3)
    a = rng.randint(0, 7, size=(5, 12))                                       # BAIR-like: 3-d state differences, an absent action (of 8)
    a[a == 5] = 6
    d = np.stack([np.cos(a), np.sin(a), 0.1 * a], axis=-1) * 0.02 + rng.normal(0, 0.01, size=a.shape + (3,))
    out["bair"] = (a, d, 8)
    a = np.array([0, 0, 0, 1, 1, 2, 0, 1, 0, 1])                              # one sample of action 2 (kurtosis NaN), constant component
    v = np.stack([rng.normal(size=10), np.full(10, 3.0)], axis=-1)
    out["degenerate"] = (a, v, 3)
    return out


def detection_cases():
    """name -> (reference, generated) detections, -1 where missing"""
    rng = np.random.RandomState(8)
    ref = rng.randint(-1, 40, size=(7, 5))
    gen = np.where(rng.rand(7, 5) < 0.3, -1, ref + rng.randint(-5, 6, size=(7, 5)))
    ref[:, 2] = -1                                                            # a position with no successful detection: NaN distance
    gen[:, 3] = -1
    return {"mixed": (ref, gen), "none_found": (np.full((3, 4), -1), np.full((3, 4), -1))}
