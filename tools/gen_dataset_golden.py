"""Generate tests/golden/video_dataset_ref.npz from the REAL reference's dataset classes (build container only; needs the reference tree, see
tools/ref_harness.py): every BatchElement of dataset.video_dataset.VideoDataset, the collate of elements 0 and 2 and DatasetSplitter's splits, on
the seeded on-disk dataset of tests/test_video_dataset.py (_write_dataset(root, seed=5), crop [1, 2, 21, 18], 12x10); and the reference's
evaluation.metrics.psnr.PSNR on the seeded frames of test_mse_psnr_metrics.
    Usage:  python tools/gen_dataset_golden.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as rh  # noqa: E402
from tests.test_video_dataset import VD, _config, _write_dataset  # noqa: E402


def main():
    rh.install()
    from dataset.video_dataset import VideoDataset as RefDataset
    from dataset.dataset_splitter import DatasetSplitter
    from dataset.batching import single_batch_elements_collate_fn as ref_collate
    root = os.path.join(tempfile.mkdtemp(), "ds")
    os.makedirs(root)
    _write_dataset(root, seed=5)
    cfg = _config(root, [1, 2, 21, 18], (12, 10))
    tf = VD.final_transform(cfg)
    data = {}
    for key in ("training", "evaluation"):
        ref = RefDataset(root, cfg[key]["batching"], tf)
        data[f"{key}_len"] = np.int64(len(ref))
        for i in range(len(ref)):
            b = ref[i]
            data[f"{key}_{i}_actions"] = np.asarray(b.actions, np.int64)
            data[f"{key}_{i}_rewards"] = np.asarray(b.rewards, np.float64)
            data[f"{key}_{i}_dones"] = np.asarray(b.dones, bool)
            data[f"{key}_{i}_initial_frame_index"] = np.int64(b.initial_frame_index)
            data[f"{key}_{i}_observations"] = torch.stack([torch.stack(list(s)) for s in b.observations]).numpy()
        for j, t in enumerate(ref_collate([ref[0], ref[2]]).to_tuple(cuda=False)):
            data[f"{key}_collate_{j}"] = t.numpy()
    splits = DatasetSplitter.generate_splits(cfg)
    assert all(v[0] == root for v in splits.values())
    data["splits"] = np.array(repr({k: v[2] for k, v in splits.items()}))
    sys.path.insert(0, rh.REF)
    from evaluation.metrics.psnr import PSNR
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(2, 3, 3, 8, 9, generator=g), torch.rand(2, 3, 3, 8, 9, generator=g)
    data["psnr"] = PSNR()(a, b).numpy()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "video_dataset_ref.npz"), **data)


if __name__ == "__main__":
    main()
