"""BAIR dataset evaluation (evaluation/dataset_evaluator_bair.py): the frame metrics of DatasetEvaluator plus the action metrics.

The movement that follows each inferred action is the change of the robot `state` stored in the metadata of the REFERENCE video:
state[t] - state[t - 1] for t = 1 .. observations_count - 1.  It feeds action_variance/* and the action accuracy keys.
Select it with evaluation.evaluator: playablevideogeneration_amd.dataset_evaluator_bair."""
from typing import Dict

import numpy as np

from .dataset_evaluator import ActionSpaceEvaluator


class DatasetEvaluatorBair(ActionSpaceEvaluator):

    def movements(self, reference_batch, detections: Dict[str, np.ndarray], observations_count: int) -> np.ndarray:
        out = []
        for b, video in enumerate(reference_batch.video):
            meta = video.metadata
            if len(meta) < observations_count or any("state" not in meta[t] for t in range(observations_count)):
                raise Exception(f"Reference sequence {self.sequence_name(reference_batch, b)} lacks the robot state of some of its {observations_count} "
                                f"observations (metadata length {len(meta)})")
            states = [np.asarray(meta[t]["state"]) for t in range(observations_count)]
            out.append([states[t] - states[t - 1] for t in range(1, observations_count)])
        return np.asarray(out)


def evaluator(config, logger, reference_dataset, generated_dataset, batches=None):
    return DatasetEvaluatorBair(config, logger, reference_dataset, generated_dataset, batches)
