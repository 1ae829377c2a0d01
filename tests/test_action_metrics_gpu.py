"""Breakout / BAIR dataset evaluation on the MI355X: the platform detector (csrc/detection.hip) on the device against the restated scan rule of
tests/breakout_cases.py and the reference's positions (tests/golden/breakout_platform.npz), and train -> build-dataset -> evaluate through the drivers
with the Breakout evaluator on Breakout-like videos."""
import os
import pickle
import shutil

import numpy as np
import pytest
import torch
import yaml

from playablevideogeneration_amd import metrics as M
from tests.breakout_cases import CASES, bounds, breakout_frames, platform_row, positions_restated

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _hip_library():
    M.set_library(None)
    yield


@pytest.mark.parametrize("shape", [(8, 32, 208, 160), (2, 4, 210, 200), (1, 6, 64, 320)])
def test_positions_on_gpu(shape):
    frames = breakout_frames(*shape, seed=sum(shape))
    x = torch.from_numpy(frames).cuda()
    got = M.breakout_platform_positions(x)
    lo, hi = bounds()
    want = positions_restated(frames, platform_row(shape[2]), lo, hi)
    assert np.array_equal(got, want)
    assert (want >= 0).any() and (want == -1).any()
    assert np.array_equal(M.breakout_platform_positions(x), got)             # deterministic


@pytest.mark.parametrize("name", list(CASES))
def test_positions_match_reference_on_gpu(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "breakout_platform.npz"))
    frames = breakout_frames(*CASES[name])
    assert np.array_equal(M.breakout_platform_positions(torch.from_numpy(frames).cuda()), z[f"{name}_positions"])


def _breakout_dataset(root, videos=6, frames=8, H=32, W=32, seed=0):
    """videos whose platform (rows around int(188 / 208 * H), red 200) moves by -2, 0, +2 with the action of each step, between grey side walls"""
    from playablevideogeneration_amd.evaluation_dataset_builder import EvaluationVideo
    rng = np.random.RandomState(seed)
    row = platform_row(H)
    for vi in range(videos):
        actions = [int(rng.randint(0, 3)) for _ in range(frames)]
        x, fr = 9, []
        for t in range(frames):
            f = np.zeros((H, W, 3), dtype=np.uint8)
            f[: row - 3] = rng.randint(0, 256, size=(row - 3, W, 3))
            f[:, :3] = 142
            f[:, W - 3:] = 142
            f[row - 1: row + 2, x:x + 14] = (200, 72, 72)
            fr.append(f)
            x = min(max(x + 2 * (actions[t] - 1), 5), W - 3 - 16)
        EvaluationVideo(np.stack(fr), actions, [0.0] * frames, [{} for _ in range(frames)], [False] * frames).save(os.path.join(root, f"{vi:05d}"))


def test_train_build_dataset_evaluate_breakout_on_gpu(tmp_path):
    from playablevideogeneration_amd import drivers as D
    from tests.test_drivers_emu import _yaml_config
    path = _yaml_config(tmp_path)
    cfg = D.load_configuration(path)
    root = cfg["data"]["data_root"]
    shutil.rmtree(root)
    _breakout_dataset(root)
    assert D.main(["train", "--config", path, "--max-steps", "2"]) == 0
    assert D.main(["build-dataset", "--config", path]) == 0
    ref_root = str(tmp_path / "reference_test")
    for name in sorted(os.listdir(root))[4:]:                                  # the test split (dataset_splits [0.5, 0.25, 0.25] of 6 videos)
        shutil.copytree(os.path.join(root, name), os.path.join(ref_root, name))
    b = cfg["evaluation"]["batching"]
    T = b["observations_count"]
    ev = {"logging": {"run_name": "eval_breakout", "output_root": str(tmp_path / "evaluation_results")},
          "data": {"target_input_size": [32, 32], "actions_count": 3, "ground_truth_available": False},
          "reference_data": {"data_root": ref_root, "crop": [0, 0, 32, 32]},
          "generated_data": {"data_root": cfg["logging"]["evaluation_dataset_directory"], "crop": [0, 0, 32, 32]},
          "evaluation": {"evaluator": "playablevideogeneration_amd.dataset_evaluator_breakout",
                         "batching": {"batch_size": 2, "observations_count": T, "skip_frames": 0, "observation_stacking": 1, "num_workers": 0}}}
    epath = str(tmp_path / "eval.yaml")
    with open(epath, "w") as f:
        yaml.safe_dump(ev, f)
    assert D.main(["evaluate", "--config", epath]) == 0
    data = yaml.safe_load(open(os.path.join(str(tmp_path / "evaluation_results"), "eval_breakout", "data.yml")))
    # position 0 of a generated sequence is the ground-truth frame: its platform is found in both
    assert data["detection/successful_detections/global"] > 0 and data["detection/successful_detections/0"] > 0
    assert data["detection/center_distance/0"] == 0.0
    assert np.isfinite(data["action_variance/avg_variance/global"])
    keys = set()
    for m in ("mse", "psnr", "ssim"):
        keys |= {f"{m}/avg", f"{m}/var"} | {f"{m}/{i}" for i in range(T)} | {f"{m}/{i}/var" for i in range(T)}
    for m in ("center_distance", "successful_detections", "missed_detections", "reference_detections"):
        keys |= {f"detection/{m}/{i}" for i in list(range(T)) + ["global"]}
    gen_root = cfg["logging"]["evaluation_dataset_directory"]
    inferred = set()
    for name in os.listdir(gen_root):
        with open(os.path.join(gen_root, name, "metadata.pkl"), "rb") as f:
            inferred |= {m["inferred_action"] for m in pickle.load(f)[:-1]}
    for a in sorted(inferred):
        keys |= {f"action_variance/{k}/{a}" for k in ("mean_vector", "kurtosis", "quantiles", "variance_vector", "avg_variance", "frequency")}
    keys |= {"action_variance/avg_variance/mean"} | {f"action_variance/{k}/global" for k in ("mean_vector", "quantiles", "variance_vector", "avg_variance")}
    accuracy = {k for k in data if "action_accuracy" in k}
    assert set(data) - accuracy == keys
    try:
        import sklearn  # noqa: F401
        if len(inferred) > 1:
            assert accuracy == {f"{n}/action_accuracy{s}" for n in ("linear", "rbf", "poly", "linear_ovo") for s in [""] + [f"/{a}" for a in sorted(inferred)]}
    except ImportError:
        pass
