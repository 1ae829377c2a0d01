"""Dataset evaluation on the MI355X: the fused frame-metric pass (csrc/frame_metrics.hip) against the fp64 restatement of tests/frame_metrics_cases.py on
the device, determinism, the VGG19 cosine similarity in both VGG arithmetics, and train -> build-dataset -> evaluate through the drivers."""
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

from oracle import caddy_oracle as O
from playablevideogeneration_amd import metrics as M
from tests.frame_metrics_cases import metrics_restated, seeded_pair, vgg_cos_restated

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_library():
    M.set_library(None)
    yield


def _check(got, ref, gen, value_range=1.0):
    want = {k: v.cpu() for k, v in metrics_restated(ref, gen, value_range).items()}
    for k in ("mse", "motion_masked_mse"):
        np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), rtol=1e-6, atol=1e-12, err_msg=k)
    np.testing.assert_allclose(got["ssim"].numpy(), want["ssim"].numpy(), rtol=0, atol=1e-5, err_msg="ssim")
    np.testing.assert_allclose(got["psnr"].numpy(), want["psnr"].numpy(), rtol=0, atol=1e-4, err_msg="psnr")
    for k in ("ref_min", "ref_max", "gen_min", "gen_max"):
        np.testing.assert_array_equal(got[k].numpy(), want[k].numpy(), err_msg=k)


@pytest.mark.parametrize("shape", [(2, 4, 64, 64), (2, 4, 96, 128), (2, 4, 11, 13), (1, 2, 384, 384)])
def test_fused_pass_on_gpu(shape):
    ref, gen = (t.cuda() for t in seeded_pair(*shape, seed=sum(shape)))
    _check(M.frame_metrics(ref, gen), ref, gen)


def test_bair_evaluation_geometry_on_gpu():
    # evaluation of configs/evaluation/01_bair.yaml: 30 observations of 256 x 256; 8 sequences at once
    ref, gen = (t.cuda() for t in seeded_pair(8, 30, 256, 256, seed=1))
    got = M.frame_metrics(ref, gen)
    _check(got, ref, gen)
    again = M.frame_metrics(ref, gen)
    for k in M.SLOTS:
        assert torch.equal(got[k].nan_to_num(), again[k].nan_to_num()), k      # bit-identical: fixed-order reductions, no float atomics


@pytest.mark.parametrize("precision", ["split_f16", "exact"])
def test_vgg_cosine_on_gpu(precision):
    V = O.make_vgg_params()
    ref, gen = seeded_pair(2, 3, 64, 64, seed=9, noise=0.2)
    fm = M.FrameMetrics(64, 64, max_frames=4, vgg_state_dict=V)                 # 6 frames: two chunks
    if precision == "exact":
        fm.set_vgg_precision(0)
    got = fm(ref.cuda(), gen.cuda(), want_vgg=True)
    want = vgg_cos_restated(ref, gen, V)
    # Bounds fixed before the run.  Exact fp32: the oracle's CPU convolutions and the fp32 MFMA path differ only in the summation order (fp32 rounding of
    # K <= 4608-term sums, ~1e-6 relative on the features), 1e-5 on the cosine.  Split f16 (the default): each operand is hi + lo with an 11-bit lo, so a
    # product x w misses at most |x w| (2^-22 for the lo roundings + 2^-22 for the dropped lo x lo term); 13 layers of such products, compounding with a
    # cancellation factor of ~10, leave <= 13 * 3 * 2^-22 * 10 ~ 1e-4 relative on the features, and a relative perturbation e of both feature vectors moves
    # the cosine by <= 2e: 2e-4.  Measured on the MI355X: max |diff| 3.96e-07 (split f16), 3.91e-07 (exact).
    tol = 1e-5 if precision == "exact" else 2e-4
    print(f"vgg_sim {precision}: max |diff| {float((got['vgg_sim'] - want).abs().max()):.2e}")
    np.testing.assert_allclose(got["vgg_sim"].numpy(), want.numpy(), rtol=0, atol=tol)
    _check(got, ref, gen)


def test_train_build_dataset_evaluate_on_gpu(tmp_path):
    from playablevideogeneration_amd import drivers as D
    from tests.test_drivers_emu import _yaml_config
    path = _yaml_config(tmp_path)
    assert D.main(["train", "--config", path, "--max-steps", "2"]) == 0
    assert D.main(["build-dataset", "--config", path]) == 0
    cfg = D.load_configuration(path)
    # the reference side: the test split of the flat dataset (dataset_splits [0.5, 0.25, 0.25] of 6 videos -> the last 2)
    root = cfg["data"]["data_root"]
    ref_root = str(tmp_path / "reference_test")
    for name in sorted(os.listdir(root))[4:]:
        shutil.copytree(os.path.join(root, name), os.path.join(ref_root, name))
    b = cfg["evaluation"]["batching"]
    ev = {"logging": {"run_name": "eval0", "output_root": str(tmp_path / "evaluation_results")},
          "data": {"target_input_size": [32, 32], "actions_count": 3, "ground_truth_available": False},
          "reference_data": {"data_root": ref_root, "crop": [0, 0, 32, 32]},
          "generated_data": {"data_root": cfg["logging"]["evaluation_dataset_directory"], "crop": [0, 0, 32, 32]},
          "evaluation": {"evaluator": "playablevideogeneration_amd.dataset_evaluator",
                         "batching": {"batch_size": 2, "observations_count": b["observations_count"], "skip_frames": 0, "observation_stacking": 1, "num_workers": 0}}}
    epath = str(tmp_path / "eval.yaml")
    with open(epath, "w") as f:
        yaml.safe_dump(ev, f)
    assert D.main(["evaluate", "--config", epath]) == 0
    data = yaml.safe_load(open(os.path.join(str(tmp_path / "evaluation_results"), "eval0", "data.yml")))
    T = b["observations_count"]
    for m in ("mse", "motion_masked_mse", "psnr", "ssim"):
        assert {f"{m}/avg", f"{m}/var"} | {f"{m}/{i}" for i in range(T)} | {f"{m}/{i}/var" for i in range(T)} <= set(data)
    assert data["mse/0"] < 1e-4 and data["ssim/0"] > 0.99      # position 0 of a generated sequence is the ground-truth frame (up to the uint8 round trip)
    assert data["mse/1"] > 0.0 and "vgg_sim/avg" not in data
