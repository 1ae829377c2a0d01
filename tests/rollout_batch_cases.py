"""Batched roll-out (caddy_start_inference_batch / caddy_generate_next_batch / caddy_rollout_copy_state): cases shared by the simulator and the GPU tests.

Geometries are the roll-out goldens' own.  n = 3 and n = 5 are odd, and at 1/8 resolution a sequence is 16 (32x32) or 24 (32x48) pixels, so every pixel tile of R's
convolutions straddles sequences and the per-sequence rows of the auxiliary input are exercised.  The oracle references are computed once per (geometry, n, steps) and shared."""
import functools

import numpy as np
import torch

from oracle import caddy_oracle as O
from playablevideogeneration_amd.engine import CaddyError
from tests import helpers as H
from tests import model_cases as M

MAIN = dict(variant="main", K=7, Da=5, Ch=128, S=4, H=32, W=32)           # tests/golden/rollout_main_s4.npz
REDUCED = dict(variant="reduced", K=3, Da=1, Ch=64, S=1, H=32, W=48)     # tests/golden/rollout_reduced_s1.npz
GOLDEN_TOL, GOLDEN_MSE = 2e-4, 1e-5                     # model_cases.rollout_case
ORACLE_TOL, ORACLE_MSE = 2e-3, 1e-6                     # model_cases.rollout_oracle_case


def _engine(c, n, lib, dev, fold=True):
    d, P, _ = H.inputs_of(dict(c, B=1, T=1))
    eng = M.make_engine(dict(c, B=n, T=2), lib, dev)
    eng.load_state_dict(P)
    if not fold:
        eng.set_rollout_fold(False)
    return eng, P


def _inputs(c, n, steps, seed=17):
    """per-sequence start observations (helpers.inputs_of at B = n), action scripts and variations (one sequence with non-zero ones) from a fixed seed"""
    _, _, obs = H.inputs_of(dict(c, B=n, T=1))
    g = torch.Generator().manual_seed(seed)
    scripts = torch.randint(0, c["K"], (steps, n), generator=g)
    var = torch.zeros(steps, n, c["Da"])
    var[:, n // 2] = torch.randn(steps, c["Da"], generator=g) * 0.5
    return obs[:, 0].contiguous(), scripts, var


def _roll(eng, n, obs, scripts, var=None, reset_at=None):
    """start_inference(n) + one generate_next_batch per row of `scripts`; reset_at = (step, slot).  -> (frames (steps, n, 3, H, W), final observations) on the host"""
    eng.start_inference(n)
    o, frames = obs, []
    for i in range(scripts.shape[0]):
        reset = None
        if reset_at is not None and reset_at[0] == i:
            reset = [1 if s == reset_at[1] else 0 for s in range(n)]
        f, o = eng.generate_next_batch(o, scripts[i], None if var is None else var[i], reset)
        frames.append(f.cpu())
    return torch.stack(frames), o.cpu()


def golden_case(name, lib, dev, fold=True):
    """slot 0 of an n = 3 batch follows the golden's sequence (its observation, actions i % K, then the two interpolation steps) while slots 1 and 2 run other observations
    and scripts: slot 0 must meet the reference's frames under rollout_case's bounds"""
    c, z = H.load_case(name)
    n, K = 3, c["K"]
    _, _, obs = H.inputs_of(c)
    eng, P = _engine(c, n, lib, dev, fold)
    other = torch.rand(2, 3 * c["S"], c["H"], c["W"], generator=torch.Generator().manual_seed(11)) * 2 - 1
    o = torch.cat([obs[0, 0][None], other])
    eng.start_inference(n)
    for i in range(c["steps"]):
        f, o = eng.generate_next_batch(o, [i % K, (i + 1) % K, (2 * i + 2) % K])
        err = f[0].cpu().numpy() - z["frames"][i]
        print(name, "step", i, "max", np.abs(err).max(), "mse", (err ** 2).mean())
        assert np.abs(err).max() < GOLDEN_TOL and (err ** 2).mean() < GOLDEN_MSE, (i, np.abs(err).max())
    assert np.abs(o[0].cpu().numpy() - z["last_obs"]).max() < GOLDEN_TOL
    cen = P["centroid_estimator.estimated_centroids"]
    for j, (a1, a2, al) in enumerate(H.INTERP):
        a1, a2 = a1 % K, a2 % K
        sel = a2 if al > 0.5 else a1
        v = torch.zeros(n, c["Da"])
        v[0] = (cen[a2] - cen[a1]) * al + cen[a1] - cen[sel]
        v[2] = 0.25
        f, _ = eng.generate_next_batch(o, [sel, (sel + 1) % K, j % K], v)      # (as rollout_case: both interpolation steps start from the last observation)
        assert np.abs(f[0].cpu().numpy() - z["interp_frames"][j]).max() < GOLDEN_TOL, ("interpolation", j)


def single_equal_case(name, lib, dev):
    """at n = 1 the batched entry returns the frames and observations of the existing single-sequence entry bit for bit"""
    c, _ = H.load_case(name)
    _, _, obs = H.inputs_of(c)
    eng, _ = _engine(c, 1, lib, dev)
    v = torch.full((c["Da"],), 0.3)
    eng.start_inference()
    o, single = obs[0, 0], []
    for i in range(4):
        f, o = eng.generate_next(o, i % c["K"], v if i == 2 else None)
        single.append((f.cpu(), o.cpu()))
    eng.start_inference(1)
    o = obs[0, 0][None]
    for i in range(4):
        f, o = eng.generate_next_batch(o, [i % c["K"]], v[None] if i == 2 else None)
        assert torch.equal(f[0].cpu(), single[i][0]) and torch.equal(o[0].cpu(), single[i][1]), i


@functools.lru_cache(maxsize=None)
def _oracle_reference(key, n, steps):
    c = dict(key)
    d, P, _ = H.inputs_of(dict(c, B=1, T=1))
    obs, scripts, var = _inputs(c, n, steps)
    frames, last = [], []
    with torch.no_grad():
        for s in range(n):
            orc = O.Oracle(d, {k: v.clone() for k, v in P.items()}, training=False)
            orc.start_inference()
            o, fs = obs[s], []
            for i in range(steps):
                f, o = orc.generate_next(o, int(scripts[i, s]), var[i, s] if var[i, s].abs().sum() > 0 else None)
                fs.append(f)
            frames.append(torch.stack(fs))
            last.append(o)
    return torch.stack(frames, dim=1), torch.stack(last)      # (steps, n, 3, H, W), (n, 3S, H, W): never modified by the callers


def oracle_case(lib, dev, c, n=5, steps=6):
    """every sequence of the batch has its own start and action script (one has non-zero variations): each against its own Oracle.start_inference / generate_next run"""
    ref_frames, ref_last = _oracle_reference(tuple(sorted(c.items())), n, steps)
    obs, scripts, var = _inputs(c, n, steps)
    eng, _ = _engine(c, n, lib, dev)
    frames, last = _roll(eng, n, obs, scripts, var)
    worst = worst_mse = 0.0
    for i in range(steps):
        for s in range(n):
            err = frames[i, s] - ref_frames[i, s]
            worst, worst_mse = max(worst, err.abs().max().item()), max(worst_mse, (err ** 2).mean().item())
    print(c, "n", n, "worst abs", worst, "worst frame mse", worst_mse, "final observation", (last - ref_last).abs().max().item())
    for i in range(steps):
        for s in range(n):
            err = frames[i, s] - ref_frames[i, s]
            assert err.abs().max().item() < ORACLE_TOL and (err ** 2).mean().item() < ORACLE_MSE, (i, s, err.abs().max().item(), (err ** 2).mean().item())
    assert (last - ref_last).abs().max().item() < ORACLE_TOL
    return dict(worst_abs=worst, worst_mse=worst_mse)


def no_coupling_case(lib, dev, c, n=3, steps=3):
    """a sequence's frames do not depend on its slot nor on what the other slots hold (bit for bit)"""
    obs, scripts, var = _inputs(c, n, steps)
    eng, _ = _engine(c, n, lib, dev)
    base, base_last = _roll(eng, n, obs, scripts, var)
    perm = [(s + 1) % n for s in range(n)]      # slot s of the second run holds sequence perm[s]
    moved, moved_last = _roll(eng, n, obs[perm].contiguous(), scripts[:, perm], var[:, perm])
    for s in range(n):
        assert torch.equal(moved[:, s], base[:, perm[s]]) and torch.equal(moved_last[s], base_last[perm[s]]), ("moved", s)
    obs2, scripts2, var2 = obs.clone(), scripts.clone(), var.clone()
    keep = n // 2
    for s in range(n):
        if s != keep:
            obs2[s] = -obs[s].flip(-1)
            scripts2[:, s] = (scripts[:, s] + 1) % c["K"]
            var2[:, s] = 0.7
    other, other_last = _roll(eng, n, obs2, scripts2, var2)
    assert torch.equal(other[:, keep], base[:, keep]) and torch.equal(other_last[keep], base_last[keep])
    assert not torch.equal(other[:, 0], base[:, 0])


def reset_and_fork_case(lib, dev, c, n=3, steps=5):
    obs, scripts, var = _inputs(c, n, steps)
    eng, _ = _engine(c, n, lib, dev)
    base, base_last = _roll(eng, n, obs, scripts, var)
    # reset[j] at step 3 with sequence j's inputs rewound to its start: j reproduces its own steps 0.., the others do not notice
    j, at = 1, 3
    eng.start_inference(n)
    o, frames = obs, []
    for i in range(steps):
        reset = None
        acts, v = scripts[i].clone(), var[i].clone()
        if i >= at:
            acts[j], v[j] = scripts[i - at, j], var[i - at, j]
        if i == at:
            reset = [1 if s == j else 0 for s in range(n)]
            o = o.clone()
            o[j] = obs[j]
        f, o = eng.generate_next_batch(o, acts, v, reset)
        frames.append(f.cpu())
    frames = torch.stack(frames)
    for s in range(n):
        if s != j:
            assert torch.equal(frames[:, s], base[:, s]), ("reset disturbed", s)
    assert torch.equal(frames[:at, j], base[:at, j]) and torch.equal(frames[at:, j], base[:steps - at, j])
    assert not torch.equal(frames[at, j], base[at, j])
    # graph replay: a second start_inference(n) followed by the same calls reproduces the first roll-out bit for bit
    again, again_last = _roll(eng, n, obs, scripts, var)
    assert torch.equal(again, base) and torch.equal(again_last, base_last)
    # fork: after copy_rollout_state(a, b), slot b fed slot a's observation and action continues exactly as slot a
    a, b = 0, 2
    eng.start_inference(n)
    o = obs
    for i in range(2):
        _, o = eng.generate_next_batch(o, scripts[i], var[i])
    eng.copy_rollout_state(a, b)
    o = o.clone()
    o[b] = o[a]
    for i in range(2, steps):
        acts, v = scripts[i].clone(), var[i].clone()
        acts[b], v[b] = acts[a], v[a]
        f, o = eng.generate_next_batch(o, acts, v)
        assert torch.equal(f[a], f[b]) and torch.equal(o[a], o[b]), ("fork", i)
        assert torch.equal(f[a].cpu(), base[i, a])
    return eng, (obs, scripts, var, base, base_last)


def change_n_case(lib, dev, c, steps=3):
    """roll-outs of 3, 5, then 3 sequences on one engine: the graph of another batch extent is dropped, the first results come back bit for bit"""
    eng, _ = _engine(c, 5, lib, dev)
    obs3, scripts3, var3 = _inputs(c, 3, steps)
    obs5, scripts5, var5 = _inputs(c, 5, steps, seed=23)
    first, first_last = _roll(eng, 3, obs3, scripts3, var3)
    five, _ = _roll(eng, 5, obs5, scripts5, var5)
    again, again_last = _roll(eng, 3, obs3, scripts3, var3)
    assert torch.equal(again, first) and torch.equal(again_last, first_last)
    five_again, _ = _roll(eng, 5, obs5, scripts5, var5)
    assert torch.equal(five_again, five)


def error_case(lib, dev, c):
    """every misuse is refused with -2 / CaddyError naming its cause before any work is enqueued, and leaves a roll-out under way as it was"""
    import ctypes as C
    import pytest
    eng, _ = _engine(c, 3, lib, dev)
    obs, scripts, _ = _inputs(c, 3, 4)
    obs, scripts = obs[:2], scripts[:, :2]
    eng._roll_n = 3      # (past the Python-side guard: the C entry must refuse by itself)
    with pytest.raises(CaddyError, match="caddy_start_inference_batch first"):
        eng.generate_next_batch(_inputs(c, 3, 1)[0], [0, 0, 0])
    with pytest.raises(CaddyError, match="caddy_start_inference_batch first"):
        eng.copy_rollout_state(0, 1)
    want, _ = _roll(eng, 2, obs, scripts)      # recorded before the refused calls below
    # the same roll-out again, with every refused call between its steps 1 and 2
    eng.start_inference(2)
    o, got = obs, []
    for i in range(2):
        f, o = eng.generate_next_batch(o, scripts[i])
        got.append(f.cpu())
    for bad in (0, 4, -1):      # n = 0, n > caddy_config.batch
        with pytest.raises(CaddyError, match="outside"):
            eng.start_inference(bad)
        assert eng.lib.caddy_start_inference_batch(eng.ctx, bad) == -2
    with pytest.raises(CaddyError, match="out of range"):
        eng.generate_next_batch(o, [0, c["K"]])
    with pytest.raises(CaddyError, match="out of range"):
        eng.generate_next_batch(o, [-1, 0])
    for slots in ((0, 2), (2, 0), (-1, 0)):
        with pytest.raises(CaddyError, match="outside"):
            eng.copy_rollout_state(*slots)
    with pytest.raises(CaddyError, match="caddy_generate_next_batch"):
        eng.generate_next(o[0], 0)      # the single-sequence entry while two sequences are under way
    # overlapping buffers, through the C entry itself
    dev_obs = o.to(eng.device).contiguous()
    frames = torch.empty((2, 3, c["H"], c["W"]), device=eng.device)
    acts = (C.c_int * 2)(0, 1)
    rc = eng.lib.caddy_generate_next_batch(eng.ctx, dev_obs.data_ptr(), acts, None, None, frames.data_ptr(), dev_obs.data_ptr())
    assert rc == -2 and "must not overlap" in eng._err()
    rc = eng.lib.caddy_generate_next_batch(eng.ctx, dev_obs.data_ptr(), acts, None, None, dev_obs.data_ptr() + 4 * dev_obs[0].numel(), None)
    assert rc == -2 and "must not overlap" in eng._err()
    rc = eng.lib.caddy_generate_next_batch(eng.ctx, dev_obs.data_ptr(), None, None, None, frames.data_ptr(), None)
    assert rc == -2 and "null" in eng._err()
    # none of the refused calls touched the roll-out: its remaining steps give the frames recorded before them, bit for bit
    for i in range(2, 4):
        f, o = eng.generate_next_batch(o, scripts[i])
        got.append(f.cpu())
    assert torch.equal(want, torch.stack(got))
