"""Generate tests/golden/breakout_platform.npz and tests/golden/action_metrics.npz from the REAL reference (build container only; needs the reference
tree, see tools/ref_harness.py):
  evaluation.metrics.breakout_platform_position.BreakoutPlatformPosition on the seeded frames of tests/breakout_cases.py (CASES; the frames are re-derived
  by the tests, only the generator parameters and the positions are stored), and evaluation.metrics.detection_metric_1d.DetectionMetric1D,
  evaluation.metrics.action_variance.ActionVariance and evaluation.metrics.action_linear_classification.ActionClassificationScore on the seeded inputs
  of tests/breakout_cases.py (action_cases, detection_cases; stored with their results, as JSON text, and the sklearn version used).
    Usage:  python tools/gen_breakout_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as rh  # noqa: E402
from tests.breakout_cases import CASES, action_cases, breakout_frames, detection_cases  # noqa: E402


def main():
    rh.install()
    # DetectionMetric1D allocates with np.int / np.float, which numpy 2 no longer has
    np.int, np.float = int, float
    import sklearn
    from evaluation.metrics.action_linear_classification import ActionClassificationScore
    from evaluation.metrics.action_variance import ActionVariance
    from evaluation.metrics.breakout_platform_position import BreakoutPlatformPosition
    from evaluation.metrics.detection_metric_1d import DetectionMetric1D

    platform = {}
    for name, (B, T, H, W, seed) in CASES.items():
        frames = torch.from_numpy(breakout_frames(B, T, H, W, seed))
        with torch.no_grad():
            platform[f"{name}_positions"] = np.asarray(BreakoutPlatformPosition()(frames), dtype=np.int64)
        platform[f"{name}_params"] = np.array([B, T, H, W, seed], dtype=np.int64)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "breakout_platform.npz"), **platform)

    metrics = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (ref, gen) in detection_cases().items():
        metrics[f"detection_{name}"] = np.array(json.dumps(DetectionMetric1D()(ref, gen, "detection")))
    for name, (actions, vectors, count) in action_cases().items():
        metrics[f"variance_{name}"] = np.array(json.dumps(ActionVariance()(actions, vectors, count)))
        np.random.seed(0)      # LinearSVC without random_state draws from the global generator
        metrics[f"accuracy_{name}"] = np.array(json.dumps(ActionClassificationScore()(actions, vectors, count)))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "action_metrics.npz"), **metrics)


if __name__ == "__main__":
    main()
