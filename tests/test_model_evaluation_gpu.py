"""One-pass model evaluation on the MI355X (model_evaluation.py; the frame writer behind the dataset builder and the play / interpolate drivers): the device-side
quantisation against the host code path, and `evaluate-model` against `build-dataset` followed by `evaluate` with the generic evaluator -- exactly, and with the
yielded tensors on the device."""
import importlib

import pytest

from playablevideogeneration_amd import metrics as M
from tests import model_evaluation_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_library():
    M.set_library(None)
    yield


def _build(cfg):
    model = getattr(importlib.import_module(cfg["model"]["architecture"]), "model")(cfg)          # train.py:38-39
    return model.cuda()


def test_builder_device_quantise_equals_the_host_path_on_gpu(tmp_path):
    MC.check_builder(_build, tmp_path)


def test_play_and_interpolate_device_frames_equal_the_host_path_on_gpu(tmp_path):
    MC.check_play_and_interpolate(_build, tmp_path, "cuda")


def test_one_pass_equals_build_dataset_then_evaluate_on_gpu(tmp_path):
    """`evaluate` run twice on the same trees gives bit-identical metrics (asserted inside), so every key of `evaluate-model` is required to be equal, not close"""
    MC.check_one_pass_against_two_steps(_build, tmp_path, ["playablevideogeneration_amd.dataset_evaluator"], "cuda")
