"""Host statistics of the dataset evaluation that say whether the inferred action space is playable (numpy; sklearn for the classifiers).

    detection_metric_1d           evaluation/metrics/detection_metric_1d.py           reference vs generated detections, per position and global
    action_variance               evaluation/metrics/action_variance.py               spread of the movement that follows each inferred action (Delta-MSE)
    action_classification_score   evaluation/metrics/action_linear_classification.py  SVM recovery of the action from its movement (Delta-Acc)

`actions` are integers in [0, actions_count), `vectors` the movements that follow them, one vector (last axis) per action.  Results are dicts of
plain Python ints, floats and (nested) lists under the reference's keys, so yaml.dump writes them."""
import logging
import statistics
from typing import Dict

import numpy as np

QUANTILE_LEVELS = [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]

_log = logging.getLogger(__name__)


def detection_metric_1d(reference: np.ndarray, generated: np.ndarray, prefix: str) -> Dict:
    """(sequences, observations_count) detections, -1 where missing -> {prefix}/{center_distance, successful_detections, missed_detections,
    reference_detections}/{i} and /global.  center_distance is the mean |reference - generated| over the successful detections: NaN where there are none."""
    reference, generated = np.asarray(reference), np.asarray(generated)
    ref_found, gen_found = reference != -1, generated != -1
    both = ref_found & gen_found
    successful = both.sum(axis=0).astype(np.int64)
    missed = (ref_found & ~gen_found).sum(axis=0).astype(np.int64)
    distances = np.where(both, np.abs(reference - generated), 0).sum(axis=0).astype(np.float64)      # integer sums: exact in float64
    with np.errstate(divide="ignore", invalid="ignore"):
        center = distances / successful
        center_global = distances.sum() / successful.sum()
    results = {}
    for i in range(reference.shape[1]):
        results[f"{prefix}/center_distance/{i}"] = float(center[i])
        results[f"{prefix}/successful_detections/{i}"] = int(successful[i])
        results[f"{prefix}/missed_detections/{i}"] = int(missed[i])
        results[f"{prefix}/reference_detections/{i}"] = int(missed[i] + successful[i])
    results[f"{prefix}/center_distance/global"] = float(center_global)
    results[f"{prefix}/successful_detections/global"] = int(successful.sum())
    results[f"{prefix}/missed_detections/global"] = int(missed.sum())
    results[f"{prefix}/reference_detections/global"] = int(missed.sum() + successful.sum())
    return results


def _flatten(actions: np.ndarray, vectors: np.ndarray):
    vectors = np.asarray(vectors)
    return np.asarray(actions).reshape(-1), vectors.reshape(-1, vectors.shape[-1])


def action_variance(actions: np.ndarray, vectors: np.ndarray, actions_count: int) -> Dict:
    """per present action a: mean_vector/a, kurtosis/a (Fisher, biased), quantiles/a (QUANTILE_LEVELS), variance_vector/a, avg_variance/a (mean of the
    per-component variances) and frequency/a; avg_variance/mean over the present actions; mean_vector, quantiles, variance_vector and avg_variance of all
    vectors as /global.  Every key under action_variance/."""
    from scipy.stats import kurtosis
    actions, vectors = _flatten(actions, vectors)
    results, averages = {}, []
    for a in range(actions_count):
        sel = actions == a
        if not sel.any():
            continue
        v = vectors[sel]
        variance = np.var(v, axis=0)
        avg = float(np.mean(variance))
        averages.append(avg)
        results[f"action_variance/mean_vector/{a}"] = np.mean(v, axis=0).tolist()
        results[f"action_variance/kurtosis/{a}"] = kurtosis(v, axis=0, fisher=True, bias=True).tolist()
        results[f"action_variance/quantiles/{a}"] = np.quantile(v, QUANTILE_LEVELS, axis=0).tolist()
        results[f"action_variance/variance_vector/{a}"] = variance.tolist()
        results[f"action_variance/avg_variance/{a}"] = avg
        results[f"action_variance/frequency/{a}"] = float(v.shape[0] / vectors.shape[0])
    results["action_variance/avg_variance/mean"] = statistics.mean(averages)
    variance = np.var(vectors, axis=0)
    results["action_variance/mean_vector/global"] = np.mean(vectors, axis=0).tolist()
    results["action_variance/quantiles/global"] = np.quantile(vectors, QUANTILE_LEVELS, axis=0).tolist()
    results["action_variance/variance_vector/global"] = variance.tolist()
    results["action_variance/avg_variance/global"] = float(np.mean(variance))
    return results


def _accuracies(name: str, actions: np.ndarray, predicted: np.ndarray, actions_count: int) -> Dict:
    results = {f"{name}/action_accuracy": float(np.mean(predicted == actions))}
    for a in range(actions_count):
        sel = actions == a
        if sel.any():
            results[f"{name}/action_accuracy/{a}"] = float(np.mean(predicted[sel] == a))
    return results


def action_classification_score(actions: np.ndarray, vectors: np.ndarray, actions_count: int) -> Dict:
    """training-set accuracy of four SVMs that predict the action from its movement: linear (LinearSVC), rbf (SVC), poly (SVC, polynomial kernel) and
    linear_ovo (one-vs-one LinearSVC), each {name}/action_accuracy plus {name}/action_accuracy/{a} per present action.  {} with a logged warning when
    sklearn is missing or a fit fails (for example when only one action is present)."""
    actions, vectors = _flatten(actions, vectors)
    try:
        from sklearn import svm
        from sklearn.multiclass import OneVsOneClassifier
    except ImportError as e:
        _log.warning("action accuracy not computed: sklearn is not available (%s)", e)
        return {}
    classifiers = (("linear", lambda: svm.LinearSVC(max_iter=10000)),
                   ("rbf", lambda: svm.SVC(max_iter=10000)),
                   ("poly", lambda: svm.SVC(kernel="poly", max_iter=10000)),
                   ("linear_ovo", lambda: OneVsOneClassifier(svm.LinearSVC(random_state=0, max_iter=10000))))
    results = {}
    try:
        for name, make in classifiers:
            predicted = make().fit(vectors, actions).predict(vectors)
            results.update(_accuracies(name, actions, predicted, actions_count))
    except Exception as e:
        _log.warning("action accuracy could not be computed: %s", e)
        return {}
    return results
