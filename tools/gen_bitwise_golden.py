"""Generate tests/golden/oracle_bitwise_*.npz from the REAL reference (build container only; needs the reference tree, see tools/ref_harness.py).

The outputs of the reference Model.forward for the two cases of tests/test_oracle.py::test_oracle_bitwise_vs_reference_golden: a reduced model
with observation stacking 2 on a 32x48 frame, and an ensemble of three action networks over four passes (with the member each pass drew).  Inputs
and weights are re-derived from seeds (oracle.caddy_oracle.make_params, torch generators); no reference source or weights are stored.
    Usage:  python tools/gen_bitwise_golden.py
"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as rh  # noqa: E402
from oracle import caddy_oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def _flat(outs, prefix, data):
    for i, o in enumerate(outs):
        if isinstance(o, (list, tuple)):
            for j, t in enumerate(o):
                data[f"{prefix}out{i}_{j}"] = t.detach().numpy()
        else:
            data[f"{prefix}out{i}"] = o.detach().numpy()


def main():
    rh.install()
    cfg = rh.make_config(variant="reduced", actions=3, action_dim=1, hidden=64, stacking=2, state_res=(4, 6))
    ref = rh.build_reference_model(cfg, O.make_params(O.Dims.from_config(cfg), seed=11))
    ref.train()
    obs = torch.rand(2, 4, 6, 32, 48, generator=torch.Generator().manual_seed(13)) * 2 - 1
    torch.manual_seed(3); random.seed(3)
    data = {}
    with torch.no_grad():
        _flat(ref((obs, torch.zeros(2, 4, dtype=torch.int32), None, None), 2, gumbel_temperature=0.6), "", data)
    np.savez_compressed(os.path.join(OUT, "oracle_bitwise_reduced_s2.npz"), **data)

    cfg3 = rh.make_config(variant="reduced", actions=3, action_dim=1, hidden=64, stacking=1, state_res=(4, 4), ensamble_size=3)
    ref3 = rh.build_reference_model(cfg3, O.make_params(O.Dims.from_config(cfg3), seed=12))
    ref3.train()
    obs3 = torch.rand(2, 3, 3, 32, 32, generator=torch.Generator().manual_seed(14)) * 2 - 1
    data = {}
    for it in range(4):
        torch.manual_seed(20 + it); random.seed(40 + it)
        with torch.no_grad():
            _flat(ref3((obs3, torch.zeros(2, 3, dtype=torch.int32), None, None), 1, gumbel_temperature=0.8), f"pass{it}_", data)
    np.savez_compressed(os.path.join(OUT, "oracle_bitwise_ens3.npz"), **data)


if __name__ == "__main__":
    main()
