"""One-pass model evaluation: what `build-dataset` followed by `evaluate` computes (build_evaluation_dataset.py:17-77 + evaluate_dataset.py:22-64), in one process and
without the round trip through PNG files.

What reaches the metric kernels after that round trip is fully determined: the generated frames are byte / 255 of the truncating cast of
evaluation/evaluation_dataset_builder.py:60-81,140-153, the reference frames are byte / 255 of the decoded test frames (dataset/transforms.py:67-87).  Both are produced
on the device here: per batch the decoded uint8 frames are staged once and go through the frame pipeline twice (csrc/frames.hip: mode 0 with every slot -> the observations
of the roll-out; mode 1 with the slot of stack position 0 of every observation -> the reference frames in [0, 1]), the roll-out is the builder's, and the frame writer
(frame_pipeline.FrameWriter, map 2, its fp32 output) turns it into what `evaluation_transform` would read back from the builder's PNGs.  `ModelRollouts` yields the pairs,
the dataset evaluators take them through their `batches=` seam, and no frame leaves the device.

    python -m playablevideogeneration_amd.drivers evaluate-model --config cfg.yaml

takes the TRAINING config; the metric weights come from the `evaluation.*` keys `evaluate` reads (evaluation.vgg19_weights, lpips_weights, fid_inception_weights, ...) and
`evaluation.dataset_evaluator` names the evaluator module (default: playablevideogeneration_amd.dataset_evaluator).  There is no torch fallback.
"""
import copy
import os
from typing import Dict

import torch

from . import metrics as M
from .action_samplers import OneHotActionSampler, ZeroActionVariationSampler
from .batching import coded_batch_elements_collate_fn, raw_batch_elements_collate_fn
from .drivers import DEFAULT_DATASET_EVALUATOR, _factory
from .evaluation_dataset_builder import sequence_metadata
from .frame_pipeline import MAP_IF_NEGATIVE, cached_pipeline, cached_writer
from .video_dataset import raw_frame_spec



class GeneratedVideo:
    """what the evaluators read of a generated sequence: its metadata, as EvaluationDatasetBuilder.predictions_to_videos builds it"""

    def __init__(self, metadata):
        self.metadata = metadata


class DeviceBatch:
    """A batch whose observations are on the device already: (bs, T, 3, H, W) fp32 in [0, 1].  `device_observations` is what dataset_evaluator.batch_observations hands
    on without a copy; `video[i]` carries the metadata (and, on the reference side, is the dataset's own video object)."""

    def __init__(self, observations: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor, videos, initial_frames=None):
        self.size = int(observations.shape[1])
        self.observations = self.device_observations = observations
        self.actions, self.rewards, self.dones = actions, rewards, dones
        self.video, self.initial_frames = videos, initial_frames

    def to_tuple(self, cuda=True):
        return self.observations, self.actions, self.rewards, self.dones


class ModelRollouts:
    """Iterable with __len__ over the TEST split: (reference DeviceBatch, generated DeviceBatch) per batch of evaluation.batching.batch_size sequences.  The dataset is read
    through `raw_frame_spec` whatever `data.device_transforms` says (the workers only decode, or with `data.device_decode` only read the files); the roll-out is the
    builder's: `ground_truth_observations_init` from `evaluation_dataset`, OneHotActionSampler, ZeroActionVariationSampler, temperature `gumbel_temperature_end`, eval mode."""

    def __init__(self, config, model, dataset, logger):
        self.config, self.model, self.logger = config, model, logger
        size = config["model"]["representation_network"]["target_input_size"]
        self.dataset = copy.copy(dataset)      # the same videos and sample grid, undecorated frames
        jpeg = bool(config["data"].get("device_decode_jpeg", False))      # opt-in: .jpg frame folders too (jpeg_reader.py); implies device_decode
        self.device_decode = jpeg or bool(config["data"].get("device_decode", False))      # opt-in: the workers ship the PNG files, the device decodes them (png_reader.py)
        self.dataset.final_transform = raw_frame_spec(config["data"].get("crop"), size, 0, "device" if self.device_decode else "host", ("png", "jpeg") if jpeg else ("png",))
        self.ground_truth_observations_init = config["evaluation_dataset"]["ground_truth_observations_init"]
        self.temperature = config["training"]["gumbel_temperature_end"]
        b = config["evaluation"]["batching"]
        self.batch_size, self.num_workers = b["batch_size"], int(b.get("num_workers", 0))
        self.lib = getattr(getattr(model, "module", model), "_lib", None)
        self.device = M.device(self.lib)
        self.last_stats = None
        from .video_writer import ComparisonVideos      # evaluation_dataset.save_videos: <output_directory>/videos/<sequence index>.avi
        self.videos = ComparisonVideos(config, os.path.join(config["logging"]["output_directory"], "videos"), self.lib)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _loader(self):
        from torch.utils.data import DataLoader
        collate = coded_batch_elements_collate_fn if self.device_decode else raw_batch_elements_collate_fn
        return DataLoader(self.dataset, batch_size=self.batch_size, shuffle=False, collate_fn=collate, num_workers=self.num_workers, pin_memory=self.device.type == "cuda")

    def __iter__(self):
        model = self.model
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                for raw in self._loader():
                    yield self.pair(raw)
        finally:
            model.train(was_training)

    def pair(self, raw):
        """one RawBatch (or CodedBatch: its files are decoded on the device first) -> (reference DeviceBatch, generated DeviceBatch)"""
        dev = self.device
        n, (h, w) = raw.n_frames, raw.frame_hw
        frames = raw.device_frames(tuple(t.to(dev, non_blocking=True) for t in raw.staged()), self.lib, dev)      # staged (and, as files, decoded) once, read by both pipelines
        bs, T, S = raw.slot_src.shape
        to_model = cached_pipeline(h, w, raw.spec.crop, raw.spec.size, 0, n, self.lib, dev)
        to_metric = cached_pipeline(h, w, raw.spec.crop, raw.spec.size, 1, n, self.lib, dev)
        H, W = to_model.H, to_model.W
        observations = to_model(frames, raw.slot_src).view(bs, T, 3 * S, H, W)
        reference = to_metric(frames, raw.slot_src[:, :, 0].contiguous()).view(bs, T, 3, H, W)
        rest = tuple(t.to(dev, non_blocking=True) for t in (raw.actions, raw.rewards, raw.dones))
        results = self.model((observations,) + rest, ground_truth_observations_init=self.ground_truth_observations_init, action_sampler=OneHotActionSampler(),
                             action_variation_sampler=ZeroActionVariationSampler(), gumbel_temperature=self.temperature)
        rec, selected_actions, sampled_dirs = results[0], results[5], results[11]
        writer = cached_writer(H, W, bs * (int(rec.shape[1]) + 1), self.lib, dev)
        if self.videos.wanted():      # the bytes too: reference | generated, joined and JPEG-encoded on the device (the reference's bytes are its [0, 1] values * 255, exactly)
            generated_u8, generated = writer(rec, first=observations, map=MAP_IF_NEGATIVE, want_u8=True, want_f32=True)
            self.videos.add((reference * 255.0).round().to(torch.uint8).permute(0, 1, 3, 4, 2), generated_u8)
        else:
            generated = writer(rec, first=observations, map=MAP_IF_NEGATIVE, want_u8=False, want_f32=True)
        self.last_stats = stats = writer.stats()
        if (stats["saturated"] or stats["nan"]) and self.logger is not None:
            self.logger.print(f"- Warning: {stats['saturated']} values outside the uint8 range after the range mapping (saturated to 0 / 255) and {stats['nan']} NaNs "
                              f"(taken as 0) in a batch of generated frames")
        actions, mus = selected_actions.cpu().numpy(), sampled_dirs.cpu().numpy()
        if actions.shape[1] != generated.shape[1] - 1:
            raise Exception(f"Images have sequence length {generated.shape[1]} but actions have sequence length {actions.shape[1]}")
        videos = [GeneratedVideo(sequence_metadata(actions[b], mus[b])) for b in range(bs)]
        zeros = torch.zeros(bs, generated.shape[1])
        return (DeviceBatch(reference, *rest, raw.video, raw.initial_frames),
                DeviceBatch(generated, zeros.to(torch.int), zeros, zeros.to(torch.bool), videos))


def evaluate_model_loop(config, model, datasets, logger) -> Dict:
    """roll out, quantise and score the test split in one pass -> the metrics dict `build-dataset` + `evaluate` would give, also written to
    <output_directory>/model_metrics.yml"""
    import yaml
    rollouts = ModelRollouts(config, model, datasets["test"], logger)
    path = config["evaluation"].get("dataset_evaluator", DEFAULT_DATASET_EVALUATOR)
    if path.startswith("evaluation.dataset_evaluator"):      # the reference's own evaluator modules: this package's evaluator takes their place, as in `evaluate`
        path = DEFAULT_DATASET_EVALUATOR
    logger.print("- Creating evaluator")
    ev = _factory(path, "evaluator")(config, logger, None, None, batches=rollouts)
    logger.print("===== Computing metrics =====")
    metrics = ev.compute_metrics()
    logger.print("===== Computing metrics finished =====")
    logger.print(metrics)
    with open(os.path.join(config["logging"]["output_directory"], "model_metrics.yml"), "w") as f:
        yaml.dump(metrics, f)
    return metrics
