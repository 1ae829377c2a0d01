"""Shared by the one-pass evaluation tests (model_evaluation.py, the `device_quantise` builder, `device_frames` in play / interpolate): the tiny model and on-disk dataset of
the driver tests, and the two routes -- `build-dataset` followed by `evaluate` against `evaluate-model` -- on the same model.  `make_model(cfg)` is the simulator build's
model or the HIP library's; every comparison is exact."""
import os
import shutil

import numpy as np
import torch
import yaml

from playablevideogeneration_amd import drivers as D
from playablevideogeneration_amd import model_evaluation as ME
from playablevideogeneration_amd import video_dataset as VD
from tests.test_drivers_emu import _dataset, _yaml_config

T = 4      # evaluation.batching.observations_count of the driver tests' config


def fixed_length_config(tmp_path, videos=12):
    """the driver tests' config over videos of exactly observations_count frames (the fixed-length protocol of the paper's datasets): one sample per video, so that the
    two-step route pairs its two directory trees one to one.  12 videos, splits 0.5 / 0.25 / 0.25: 3 test sequences, batches of 2 and 1."""
    path = _yaml_config(tmp_path)
    cfg = yaml.safe_load(open(path))
    root = str(tmp_path / "data_fixed")
    os.makedirs(root)
    _dataset(root, videos=videos, frames=T, seed=1)
    cfg["data"]["data_root"] = root
    yaml.safe_dump(cfg, open(path, "w"))
    return D.load_configuration(path)


def build_videos(cfg, model, datasets, device_quantise):
    from playablevideogeneration_amd import evaluation_dataset_builder as EB
    cfg = dict(cfg, evaluation_dataset=dict(cfg["evaluation_dataset"], device_quantise=device_quantise))
    lines = []

    class Log:
        def print(self, *a, **k): lines.append(" ".join(str(x) for x in a))
    torch.manual_seed(3)
    return EB.builder(cfg, datasets["test"], Log()).build(model, write=False), lines


def check_builder(make_model, tmp_path):
    cfg = fixed_length_config(tmp_path)
    datasets = VD.build_datasets(cfg)
    model = make_model(cfg)
    host, _ = build_videos(cfg, model, datasets, False)
    dev, lines = build_videos(cfg, model, datasets, True)
    assert len(host) == len(dev) == len(datasets["test"]) == 3 and not lines
    for a, b in zip(host, dev):
        assert a.frames.dtype == b.frames.dtype == np.uint8 and np.array_equal(a.frames, b.frames)
        assert a.metadata == b.metadata and a.actions == b.actions and a.rewards == b.rewards and a.dones == b.dones


def check_play_and_interpolate(make_model, tmp_path, dev):
    cfg = fixed_length_config(tmp_path)
    datasets = VD.build_datasets(cfg)
    model = make_model(cfg)
    start = D._first_observations(datasets["validation"], 2)[1, 0].to(dev)
    a = D.play_loop(model, start, [1, 3, 2])
    b = D.play_loop(model, start, [1, 3, 2], device_frames=True)
    assert a["frames"].shape == (4, 32, 32, 3) and b["frames"].dtype == np.uint8 and np.array_equal(a["frames"], b["frames"]) and a["actions"] == b["actions"]
    for batched in (False, True):
        x = D.interpolate_loop(model, start, 0, 1, steps=2, frames_count=2, batched=batched)
        y = D.interpolate_loop(model, start, 0, 1, steps=2, frames_count=2, batched=batched, device_frames=True)
        assert len(x) == len(y) == 3
        for s, t in zip(x, y):
            assert s.shape == t.shape == (3, 32, 32, 3) and np.array_equal(s, t)


def evaluation_config(cfg, tmp_path, evaluator, run_name):
    """the EVALUATION config of the two-step route: the test split's folders, in order, as the reference tree; the builder's output as the generated tree"""
    ref_root = str(tmp_path / ("reference_" + run_name))
    os.makedirs(ref_root)
    _, _, names = VD.generate_splits(cfg)["test"]
    for i, name in enumerate(names):
        shutil.copytree(os.path.join(cfg["data"]["data_root"], name), os.path.join(ref_root, f"{i:05d}"))
    ev = {"logging": {"run_name": run_name, "output_root": str(tmp_path / "results")},
          "data": {"target_input_size": cfg["model"]["representation_network"]["target_input_size"], "actions_count": cfg["data"]["actions_count"]},
          "reference_data": {"data_root": ref_root, "crop": cfg["data"]["crop"]},
          "generated_data": {"data_root": cfg["logging"]["evaluation_dataset_directory"], "crop": None},
          "evaluation": {"evaluator": evaluator, "batching": dict(cfg["evaluation"]["batching"])}}
    path = str(tmp_path / (run_name + ".yaml"))
    yaml.safe_dump(ev, open(path, "w"))
    return D.load_evaluation_configuration(path)


def two_loaders(ev_cfg):
    """the two DataLoaders `evaluate` zips, rebuilt here to look at their tensors"""
    from playablevideogeneration_amd import dataset_evaluator as DE
    size = ev_cfg["data"]["target_input_size"]
    ref = VD.VideoDataset(ev_cfg["reference_data"]["data_root"], ev_cfg["evaluation"]["batching"], VD.evaluation_transform(ev_cfg["reference_data"]["crop"], size))
    gen = VD.VideoDataset(ev_cfg["generated_data"]["data_root"], ev_cfg["evaluation"]["batching"], VD.evaluation_transform(None, size))
    e = DE.DatasetEvaluator(ev_cfg, D.HeadlessLogger(ev_cfg, echo=False), ref, gen)
    return e.reference_dataloader, e.generated_dataloader


def check_one_pass_against_two_steps(make_model, tmp_path, evaluators, dev):
    """-> nothing; asserts that ModelRollouts yields the tensors and inferred actions of the two DataLoaders, batch by batch, and that `evaluate-model` returns the metrics
    dict of `build-dataset` + `evaluate`.  The two-step route is first run against itself: where its own two runs agree bit for bit the comparison is exact."""
    cfg = fixed_length_config(tmp_path)
    logger = D.HeadlessLogger(cfg, echo=False)
    datasets = VD.build_datasets(cfg)
    model = make_model(cfg)
    torch.manual_seed(3)
    assert D.build_dataset_loop(cfg, model, datasets, logger) == 3
    for evaluator in evaluators:
        tag = evaluator.rsplit(".", 1)[1]
        ev_cfg = evaluation_config(cfg, tmp_path, evaluator, tag)
        two = [D.evaluate_loop(ev_cfg, D.HeadlessLogger(ev_cfg, echo=False)) for _ in range(2)]
        assert two[0].keys() == two[1].keys()
        unstable = [k for k in two[0] if not _same(two[0][k], two[1][k])]
        assert not unstable, unstable      # same kernels, same inputs: the two-step route reproduces itself, so the one-pass route is held to exact equality
        one_cfg = dict(cfg, evaluation=dict(cfg["evaluation"], dataset_evaluator=evaluator))
        torch.manual_seed(3)
        one = ME.evaluate_model_loop(one_cfg, model, datasets, logger)
        assert one.keys() == two[0].keys() and "mse/avg" in one and "ssim/0" in one
        if "breakout" in evaluator:
            assert "action_variance/avg" in one or any(k.startswith("action_variance") for k in one)
        diff = [k for k in one if not _same(one[k], two[0][k])]
        assert not diff, {k: (one[k], two[0][k]) for k in diff}
        assert yaml.safe_load(open(os.path.join(cfg["logging"]["output_directory"], "model_metrics.yml"))).keys() == one.keys()
    # batch by batch
    ref_loader, gen_loader = two_loaders(ev_cfg)
    torch.manual_seed(3)
    rollouts = ME.ModelRollouts(cfg, model, datasets["test"], logger)
    assert len(rollouts) == len(ref_loader) == 2
    pairs = list(rollouts)      # (first: the sampled action directions in the metadata follow the global generator, which the iterators of the two loaders draw from as well)
    n = 0
    for (ref, gen), rb, gb in zip(pairs, ref_loader, gen_loader):
        for got, want in ((ref, rb), (gen, gb)):
            assert got.device_observations.device.type == dev and got.observations.dtype == torch.float32
            assert torch.equal(got.observations.cpu(), want.to_tuple(cuda=False)[0])
        assert [v.metadata for v in gen.video] == [v.metadata for v in gb.video]
        assert [[m["inferred_action"] for m in v.metadata[:-1]] for v in gen.video] == [[m["inferred_action"] for m in v.metadata[:-1]] for v in gb.video]
        assert len(ref.video) == len(rb.video) and all(hasattr(v, "frames_path") and v.metadata == w.metadata for v, w in zip(ref.video, rb.video))      # the dataset's own videos
        n += 1
    assert n == 2 and rollouts.last_stats == {"mapped": True, "saturated": 0, "nan": 0}


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b):
        return True
    return a == b
