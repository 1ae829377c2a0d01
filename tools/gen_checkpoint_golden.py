"""Generate tests/golden/ckpt_mirror_to_reference.npz from the REAL reference trainer (build container only; needs the reference tree, see
tools/ref_harness.py, and the simulator build of tests/emu for the mirror side): the mirror takes one step (seed 20) and writes latest.pth.tar,
training/smooth_mi_trainer.py LOADS it and takes the next step (seed 31).  Stored: that step's loss, global step and MI estimator, a fixed
seeded sample of every parameter (indices stored beside it), and the layout of the checkpoint the reference itself writes after one step
(tests/test_checkpoint_vs_reference.py::_layout).  A whole checkpoint is 36 MB of incompressible fp32, so none is stored.
    Usage:  python tools/gen_checkpoint_golden.py
"""
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as rh  # noqa: E402
from oracle import caddy_oracle as O  # noqa: E402
from tests.test_checkpoint_vs_reference import _cfg, _inputs, _layout, _mirror_side, _mirror_step  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SAMPLE = 256           # elements stored of each parameter tensor


def _reference_side(cfg, P):
    rh.install()
    rcfg = dict(cfg, model=dict(cfg["model"], architecture="model.reduced_model.model"))
    rcfg["model"]["action_network"] = dict(cfg["model"]["action_network"], use_variations=True)
    ref = nn.DataParallel(rh.build_reference_model(rcfg, P))
    import training.smooth_mi_trainer as SM
    logger = types.SimpleNamespace(print=lambda *a, **k: None, get_wandb=lambda: types.SimpleNamespace(log=lambda *a, **k: None))
    tr = SM.SmoothMITrainer(rcfg, ref, [0] * 8, logger)
    ref.train()
    tr.global_step = 5000
    return ref, tr


def _ref_step(ref, tr, obs, seed):
    acts = torch.zeros(obs.shape[0], obs.shape[1], dtype=torch.int32)
    batch = types.SimpleNamespace(observations=obs, actions=acts, size=obs.shape[1], to_tuple=lambda cuda=True: (obs, acts, None, None))
    torch.manual_seed(seed); random.seed(seed)
    tr.global_step += 1
    loss, info, _ = tr.compute_losses(ref, batch, obs.shape[1])
    tr.optimizer.zero_grad(); loss.backward(); tr.optimizer.step(); tr.lr_scheduler.step()
    return loss.item()


def _result(ref, tr, loss):
    data = {"loss": np.float64(loss), "global_step": np.int64(tr.global_step),
            "mi_ema": tr.mutual_information_loss.matrix_estimator.estimated_matrix.detach().numpy()}
    for n, p in ref.module.named_parameters():
        flat = p.detach().reshape(-1)
        idx = torch.randint(flat.numel(), (min(SAMPLE, flat.numel()),), generator=torch.Generator().manual_seed(0)).sort().values
        data["idx." + n], data["param." + n] = idx.numpy(), flat[idx].numpy()
    return data


def main():
    # the layout of the reference's own checkpoint
    tmp = tempfile.mkdtemp()
    cfg = _cfg(tmp)
    P, obs = _inputs(cfg)
    ref, rtr = _reference_side(cfg, P)
    _ref_step(ref, rtr, obs, 20)
    rtr.save_checkpoint(ref)
    layout = _layout(torch.load(os.path.join(tmp, "latest.pth.tar"), map_location="cpu", weights_only=True))
    # mirror -> reference: the reference loads the mirror's checkpoint (unwrapped module: no "module." prefix) and steps
    tmp = tempfile.mkdtemp()
    cfg = _cfg(tmp)
    m, mtr = _mirror_side(cfg, P)
    _mirror_step(m, mtr, obs, 20)
    mtr.save_checkpoint(m)
    ref, rtr = _reference_side(cfg, P)
    rtr.load_checkpoint(ref.module)
    data = _result(ref, rtr, _ref_step(ref, rtr, obs, 31))
    data["reference_layout"] = np.array(repr(layout))
    np.savez_compressed(os.path.join(GOLDEN, "ckpt_mirror_to_reference.npz"), **data)


if __name__ == "__main__":
    main()
