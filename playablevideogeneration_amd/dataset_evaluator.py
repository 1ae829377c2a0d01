"""Dataset evaluation: a reference dataset against a generated one (evaluation/dataset_evaluator.py:29-256), the `config["evaluation"]["evaluator"]`
seam of evaluate_dataset.py (factory `evaluator(config, logger, reference_dataset, generated_dataset)`, `.compute_metrics()` -> the dict written to data.yml).
The factory's optional `batches=` takes ready (reference, generated) batch pairs in place of the two datasets (model_evaluation.ModelRollouts: `evaluate-model`).

Per frame, on the device: mse, motion_masked_mse, psnr, ssim and -- when VGG19 weights are configured (`evaluation.vgg19_weights` or
`evaluation.vgg19_from_torchvision`, the loader of Trainer._find_vgg_weights) -- vgg_sim, all from one fused HIP pass (metrics.FrameMetrics).  The
keys are those of compute_positional_statistics: {m}/avg, {m}/var, {m}/{i}, {m}/{i}/var.  With LPIPS weights (`evaluation.lpips_weights`, or
`evaluation.lpips_vgg16_weights` + `evaluation.lpips_linear_weights`: metrics.find_lpips_weights) `lpips` is added (evaluation/metrics/lpips.py:14,33, on the
HIP path: metrics.LPIPS); without them the keys are unchanged.  With Inception weights (`evaluation.fid_inception_weights`: metrics.find_fid_weights; `evaluation.fid_resize_input`,
default true, is InceptionV3's resize_input) `fid` is added (evaluation/metrics/fid.py:140-159): the features of every frame of both datasets are collected inside the one batch
loop (the reference makes two further passes over each loader), the statistics and the Frechet distance are host fp64.  With I3D weights (`evaluation.fvd_i3d_weights`:
metrics.find_fvd_weights; `evaluation.fvd_resize_input`, default true, is the 224 x 224 resize of evaluation/metrics/fvd.py:49-56) `fvd` is added (fvd.py:229-330): the I3D logits of
the sequences are collected inside the same loop, and as IncrementalFVD feeds I3D 16 sequences at a time and drops the incomplete tail, only the first 16 floor(n / 16) sequences of
each dataset enter the statistics (fewer than 16 raise).  With torchvision Inception weights (`evaluation.is_inception_weights`: metrics.find_is_weights; `evaluation.is_splits`,
default 1; `evaluation.is_resize_input`, default true as the reference always resizes, false only for small test geometries) `is/mean` and `is/std` are added
(evaluation/metrics/inception_score.py:24-65, whose call the reference has commented out at dataset_evaluator.py:74): the class probabilities of the generated dataset's frames are
collected inside the same loop and the score is host fp64.  The plots are not computed.  The per-dataset evaluators that add the detection and action metrics of Breakout and BAIR are
dataset_evaluator_breakout and dataset_evaluator_bair (ActionSpaceEvaluator below).
"""
from typing import Dict

import numpy as np
import torch

from . import metrics as M

METRICS = ("mse", "motion_masked_mse", "psnr", "ssim", "vgg_sim")


def batch_observations(batch) -> torch.Tensor:
    """the observations of one batch: a batch that already lives on the device (model_evaluation.DeviceBatch) hands its tensor over as it is, every other
    batch its host tensor"""
    observations = getattr(batch, "device_observations", None)
    return observations if observations is not None else batch.to_tuple(cuda=False)[0]


class DatasetEvaluator:
    NOT_COMPUTED = ("- lpips, fid, fvd, inception score, detection metrics, action variance / accuracy and plots are not computed: "
                    "they need pretrained networks or detectors that are not available")

    def __init__(self, config, logger, reference_dataset, generated_dataset, batches=None):
        """batches: an iterable with __len__ of ready (reference_batch, generated_batch) pairs (model_evaluation.ModelRollouts) that takes the place of the two datasets"""
        from .trainer import Trainer
        self.config, self.logger = config, logger
        self.reference_dataset, self.generated_dataset = reference_dataset, generated_dataset
        self.batches = batches
        if batches is None:
            self._make_dataloaders(config["evaluation"]["batching"], reference_dataset, generated_dataset)
        self.vgg_state = Trainer._find_vgg_weights(config["evaluation"])
        if self.vgg_state is None:
            self.logger.print("- vgg_sim skipped: no VGG19 weights configured (evaluation.vgg19_weights / evaluation.vgg19_from_torchvision)")
        self.lpips_state = M.find_lpips_weights(config["evaluation"])
        if self.lpips_state is None:
            self.logger.print("- lpips skipped: no LPIPS weights configured (evaluation.lpips_weights, or evaluation.lpips_vgg16_weights + evaluation.lpips_linear_weights)")
        self.fid_state = M.find_fid_weights(config["evaluation"])
        self.fid_resize = bool(config["evaluation"].get("fid_resize_input", True))
        self._fid_features = ([], [])
        if self.fid_state is None:
            self.logger.print("- fid skipped: no Inception weights configured (evaluation.fid_inception_weights)")
        self.fvd_state = M.find_fvd_weights(config["evaluation"])
        self.fvd_resize = bool(config["evaluation"].get("fvd_resize_input", True))
        self._fvd_embeddings = ([], [])
        if self.fvd_state is None:
            self.logger.print("- fvd skipped: no I3D weights configured (evaluation.fvd_i3d_weights)")
        self.is_state = M.find_is_weights(config["evaluation"])
        self.is_splits = int(config["evaluation"].get("is_splits", 1))
        self.is_resize = bool(config["evaluation"].get("is_resize_input", True))
        self._is_probabilities = []
        if self.is_state is None:
            self.logger.print("- is skipped: no Inception weights configured (evaluation.is_inception_weights)")
        self.logger.print(self.NOT_COMPUTED)
        if self.lpips_state is not None:
            self.logger.print("- lpips is computed (LPIPS weights configured): the line above applies to it no longer")
        if self.fid_state is not None:
            self.logger.print("- fid is computed (Inception weights configured): the line above applies to it no longer")
        if self.fvd_state is not None:
            self.logger.print("- fvd is computed (I3D weights configured): the line above applies to it no longer")
        if self.is_state is not None:
            self.logger.print("- is is computed (Inception weights configured): the line above applies to it no longer")

    def _make_dataloaders(self, b, reference_dataset, generated_dataset):
        from torch.utils.data import DataLoader
        from .batching import collate_fn_for, single_batch_elements_collate_fn

        def collate(ds):      # raw and coded elements (evaluation.device_transforms / device_decode) bring their own collate function; their batches decode in to_tuple()
            return (collate_fn_for(ds[0]) if len(ds) else None) or single_batch_elements_collate_fn
        self.reference_dataloader = DataLoader(reference_dataset, batch_size=b["batch_size"], shuffle=False, collate_fn=collate(reference_dataset),
                                               num_workers=b.get("num_workers", 0), pin_memory=torch.cuda.is_available())
        self.generated_dataloader = DataLoader(generated_dataset, batch_size=b["batch_size"], shuffle=False, collate_fn=collate(generated_dataset),
                                               num_workers=b.get("num_workers", 0), pin_memory=torch.cuda.is_available())
        if len(self.reference_dataloader) != len(self.generated_dataloader):
            raise Exception(f"Reference and generated datasets should have the same sequences, but their length differs:"
                            f"Reference ({len(self.reference_dataloader)}), Generated({len(self.generated_dataloader)})")

    def batch_pairs(self):
        """-> (number of batches, iterable of (reference_batch, generated_batch)): the two DataLoaders side by side, or the pairs handed in as `batches`"""
        if self.batches is not None:
            return len(self.batches), self.batches
        return len(self.reference_dataloader), zip(self.reference_dataloader, self.generated_dataloader)

    @staticmethod
    def check_range(values: Dict[str, torch.Tensor], which: str):
        M.check_range(values, which)

    @staticmethod
    def compute_positional_statistics(values: np.ndarray, prefix: str) -> Dict:
        """evaluation/dataset_evaluator.py:85-113"""
        results = {}
        positional_values = values.mean(axis=0)
        positional_variances = values.var(axis=0).tolist()
        global_variance = float(positional_values.var())
        positional_values = positional_values.tolist()
        global_value = float(sum(positional_values) / len(positional_values))
        results[f"{prefix}/avg"] = global_value
        results[f"{prefix}/var"] = global_variance
        for idx, current_value in enumerate(positional_values):
            results[f"{prefix}/{idx}"] = current_value
        for idx, current_variance in enumerate(positional_variances):
            results[f"{prefix}/{idx}/var"] = current_variance
        return results

    def frame_values(self, reference_observations: torch.Tensor, generated_observations: torch.Tensor) -> Dict[str, torch.Tensor]:
        """the fused pass's slots, plus `lpips` when LPIPS weights are configured"""
        values = M.frame_metrics(reference_observations, generated_observations, 1.0, self.vgg_state)
        if self.lpips_state is not None:
            values["lpips"] = M.lpips(reference_observations, generated_observations, self.lpips_state, 1.0)
        return values

    def collect_fid_features(self, reference_observations: torch.Tensor, generated_observations: torch.Tensor) -> None:
        """Inception features of this batch's frames, every frame of every sequence a sample (evaluation/metrics/fid.py:119-135); nothing without weights"""
        if self.fid_state is None:
            return
        self._fid_features[0].append(M.inception_features(reference_observations, self.fid_state, resize=self.fid_resize).numpy())
        self._fid_features[1].append(M.inception_features(generated_observations, self.fid_state, resize=self.fid_resize).numpy())

    def fid_results(self) -> Dict:
        """{"fid": float} over the features collected since the last call (evaluation/metrics/fid.py:140-159); {} without weights"""
        if self.fid_state is None:
            return {}
        ref, gen = (np.concatenate(f, axis=0) for f in self._fid_features)
        self._fid_features = ([], [])
        return {"fid": float(M.fid_from_features(ref, gen))}

    def collect_fvd_embeddings(self, reference_observations: torch.Tensor, generated_observations: torch.Tensor) -> None:
        """I3D logits of this batch's sequences (evaluation/metrics/fvd.py:188-226); nothing without weights"""
        if self.fvd_state is None:
            return
        self._fvd_embeddings[0].append(M.i3d_embeddings(reference_observations, self.fvd_state, resize=self.fvd_resize).numpy())
        self._fvd_embeddings[1].append(M.i3d_embeddings(generated_observations, self.fvd_state, resize=self.fvd_resize).numpy())

    def fvd_results(self) -> Dict:
        """{"fvd": float} over the logits collected since the last call, complete batches of 16 sequences in loader order only (evaluation/metrics/fvd.py:270-280,322-324);
        {} without weights"""
        if self.fvd_state is None:
            return {}
        ref, gen = (np.concatenate(e, axis=0) for e in self._fvd_embeddings)
        self._fvd_embeddings = ([], [])
        return {"fvd": float(M.fvd_from_embeddings(ref[:M.fvd_batched_count(len(ref))], gen[:M.fvd_batched_count(len(gen))]))}

    def collect_is_probabilities(self, generated_observations: torch.Tensor) -> None:
        """class probabilities of this batch's generated frames, sequence after sequence (evaluation/metrics/inception_score.py:34-46); nothing without weights"""
        if self.is_state is None:
            return
        self._is_probabilities.append(M.inception_probabilities(generated_observations, self.is_state, resize=self.is_resize).numpy())

    def is_results(self) -> Dict:
        """{"is/mean", "is/std"} over the probabilities collected since the last call (evaluation/metrics/inception_score.py:48-65); {} without weights"""
        if self.is_state is None:
            return {}
        probs = np.concatenate(self._is_probabilities, axis=0)
        self._is_probabilities = []
        return M.inception_score_from_probabilities(probs, self.is_splits)

    def metric_names(self, names):
        return [m for m in names if m != "vgg_sim" or self.vgg_state is not None] + (["lpips"] if self.lpips_state is not None else [])

    def compute_metrics(self) -> Dict:
        names = self.metric_names(METRICS)
        acc = {m: [] for m in names}
        batches, pairs = self.batch_pairs()
        with torch.no_grad():
            for idx, (reference_batch, generated_batch) in enumerate(pairs):
                self.logger.print(f"- Computing metrics for batch [{idx}/{batches}]")
                reference_observations = batch_observations(reference_batch)
                generated_observations = batch_observations(generated_batch)
                values = self.frame_values(reference_observations, generated_observations)
                self.check_range(values, "ref")
                self.check_range(values, "gen")
                for m in names:
                    acc[m].append(values[m].numpy())
                self.collect_fid_features(reference_observations, generated_observations)
                self.collect_fvd_embeddings(reference_observations, generated_observations)
                self.collect_is_probabilities(generated_observations)
        results = {}
        for m in names:
            results.update(self.compute_positional_statistics(np.concatenate(acc[m], axis=0), m))
        results.update(self.fid_results())
        results.update(self.fvd_results())
        results.update(self.is_results())
        return results


class ActionSpaceEvaluator(DatasetEvaluator):
    """The loop of the reference's per-dataset evaluators (evaluation/dataset_evaluator_breakout.py, dataset_evaluator_bair.py): per frame mse, psnr,
    ssim (and vgg_sim with VGG19 weights, lpips with LPIPS weights; no motion_masked_mse, as there), plus the action variance and action accuracy of the inferred actions of the
    generated sequences against the movement that follows each of them in the reference sequences.  Subclasses say how a movement is measured
    (`movements`) and may add detections (`detect`, `detection_results`)."""
    NOT_COMPUTED = "- lpips, fid, fvd and the density plots are not computed: they need pretrained networks that are not available"
    FRAME_METRICS = ("mse", "psnr", "ssim", "vgg_sim")

    def detect(self, reference_observations: torch.Tensor, generated_observations: torch.Tensor) -> Dict[str, np.ndarray]:
        """per-batch detections to accumulate: {name: (bs, observations_count) array}"""
        return {}

    def movements(self, reference_batch, detections: Dict[str, np.ndarray], observations_count: int) -> np.ndarray:
        """-> (bs, observations_count - 1, vector_size): the movement of each transition of the reference sequences"""
        raise NotImplementedError

    def detection_results(self, detections: Dict[str, np.ndarray]) -> Dict:
        return {}

    @staticmethod
    def sequence_name(batch, sequence_idx: int) -> str:
        return str(getattr(batch.video[sequence_idx], "frames_path", sequence_idx))

    def inferred_actions(self, generated_batch, observations_count: int) -> np.ndarray:
        """(bs, observations_count - 1): metadata[i]["inferred_action"] of every transition of the generated sequences"""
        rows = []
        for b, video in enumerate(generated_batch.video):
            meta = video.metadata
            if len(meta) - 1 != observations_count - 1:
                raise Exception(f"Generated sequence {self.sequence_name(generated_batch, b)} has {len(meta) - 1} transitions in its metadata, but the "
                                f"evaluated sequences have {observations_count - 1}")
            if any("inferred_action" not in m for m in meta[:-1]):
                raise Exception(f"Generated sequence {self.sequence_name(generated_batch, b)} has metadata without an inferred_action")
            rows.append([m["inferred_action"] for m in meta[:-1]])
        return np.asarray(rows)

    def compute_metrics(self) -> Dict:
        from . import action_metrics as A
        names = self.metric_names(self.FRAME_METRICS)
        acc = {m: [] for m in names}
        detections, actions, movements = {}, [], []
        device = M.device()
        batches, pairs = self.batch_pairs()
        with torch.no_grad():
            for idx, (reference_batch, generated_batch) in enumerate(pairs):
                self.logger.print(f"- Computing metrics for batch [{idx}/{batches}]")
                reference_observations = batch_observations(reference_batch).to(device)
                generated_observations = batch_observations(generated_batch).to(device)
                values = self.frame_values(reference_observations, generated_observations)
                self.check_range(values, "ref")
                self.check_range(values, "gen")
                for m in names:
                    acc[m].append(values[m].numpy())
                self.collect_fid_features(reference_observations, generated_observations)
                self.collect_fvd_embeddings(reference_observations, generated_observations)
                self.collect_is_probabilities(generated_observations)
                found = self.detect(reference_observations, generated_observations)
                for k, v in found.items():
                    detections.setdefault(k, []).append(v)
                T = int(reference_observations.shape[1])
                actions.append(self.inferred_actions(generated_batch, T))
                movements.append(self.movements(reference_batch, found, T))
        results = {}
        for m in names:
            results.update(self.compute_positional_statistics(np.concatenate(acc[m], axis=0), m))
        results.update(self.detection_results({k: np.concatenate(v, axis=0) for k, v in detections.items()}))
        actions, movements = np.concatenate(actions, axis=0), np.concatenate(movements, axis=0)
        actions_count = self.config["data"]["actions_count"]
        results.update(A.action_variance(actions, movements, actions_count))
        accuracy = A.action_classification_score(actions, movements, actions_count)
        if not accuracy:
            self.logger.print("- Warning: action accuracy results could not be computed")
        results.update(accuracy)
        results.update(self.fid_results())
        results.update(self.fvd_results())
        results.update(self.is_results())
        return results


def evaluator(config, logger, reference_dataset, generated_dataset, batches=None):
    return DatasetEvaluator(config, logger, reference_dataset, generated_dataset, batches)
