"""Generate tests/golden/frame_metrics_ref.npz from the REAL reference's frame metrics (build container only; needs the reference tree, see
tools/ref_harness.py): evaluation.metrics.mse.MSE, evaluation.metrics.motion_masked_mse.MotionMaskedMSE (with motion_mask.MotionMaskCalculator) and
evaluation.metrics.psnr.PSNR on the seeded frame pairs of tests/test_frame_metrics_emu.py (tests.frame_metrics_cases.seeded_pair).  SSIM and the VGG
cosine similarity need piq / torchvision, which are not installed: their tests use the fp64 restatement of tests/frame_metrics_cases.py instead.
    Usage:  python tools/gen_metrics_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as rh  # noqa: E402
from tests.frame_metrics_cases import CASES_GOLDEN, seeded_pair  # noqa: E402


def main():
    rh.install()
    from evaluation.metrics.mse import MSE
    from evaluation.metrics.motion_masked_mse import MotionMaskedMSE
    from evaluation.metrics.psnr import PSNR
    data = {}
    for name, (B, T, H, W, seed) in CASES_GOLDEN.items():
        ref, gen = seeded_pair(B, T, H, W, seed=seed)
        with torch.no_grad():
            data[f"{name}_mse"] = MSE()(ref, gen).numpy()
            data[f"{name}_motion_masked_mse"] = MotionMaskedMSE()(ref, gen).numpy()
            data[f"{name}_psnr"] = PSNR()(ref, gen).numpy()
            data[f"{name}_psnr_range255"] = PSNR()(ref * 255, gen * 255, range=255.0).numpy()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "frame_metrics_ref.npz"), **data)


if __name__ == "__main__":
    main()
