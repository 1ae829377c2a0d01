"""LPIPS of the dataset evaluation on the MI355X: the VGG16 trunk on the convolution kernels in both arithmetics and the head of csrc/lpips.hip against the
plain-torch restatement of tests/lpips_cases.py per level, the invariants, and the BAIR evaluation geometry in chunks."""
import numpy as np
import pytest
import torch

from playablevideogeneration_amd import metrics as M
from tests.frame_metrics_cases import seeded_pair
from tests.lpips_cases import CHANNELS, check_levels, lpips_restated, make_lpips_params

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_library():
    M.set_library(None)
    yield


@pytest.fixture(scope="module")
def P():
    return make_lpips_params()


# the cases and the bound of tests/test_lpips_emu.py (lpips_cases.check_levels: per level, relative, 8 x the fp32-vs-fp64 spread of the restatement on the case, floor 1e-6)
@pytest.mark.parametrize("shape,seed,noise,max_frames", [((2, 3, 64, 64), 9, 0.2, 4), ((1, 2, 96, 128), 5, 0.2, 2), ((1, 2, 64, 64), 7, 0.01, 1)])
def test_lpips_exact_fp32_on_gpu(P, shape, seed, noise, max_frames):
    ref, gen = seeded_pair(*shape, seed=seed, noise=noise)
    ctx = M.LPIPS(shape[2], shape[3], max_frames, P)
    ctx.set_vgg_precision(0)
    total, levels = ctx(ref.cuda(), gen.cuda(), return_levels=True)
    check_levels(total, levels, ref, gen, P, label=f"{shape} noise {noise}")


def check_split_f16(total, levels, ref, gen, P, label):
    """Bound fixed before the first run, from the feature-error bound of test_vgg_cosine_on_gpu: the split-f16 convolutions leave e <= 1e-4 relative on a feature vector (13 layers
    of hi + lo products, cancellation factor ~10; an S16 tap adds 2^-22).  A relative perturbation e of f moves the unit vector f / |f| by <= 2e, so the difference d of the two unit
    vectors is off by <= 4e in norm, and |d|^2 -- what a level averages, weighted -- by <= 2 * 4e / |d| relative.  |d| comes from the restatement's own level value:
    level_l = mean_px sum_c w_c d_c^2 ~ mean_c(w_l) |d|^2 for weights that do not know d, so |d|_l = sqrt(level_l / mean_c(w_l)), per frame.  The total: the loosest level's bound.
    Measured on the MI355X (the run prints the figures): 24 x 128 x 128 -- 2.1e-8, 6.7e-8, 2.1e-7, 4.4e-7, 1.2e-6 per level against bounds of 1.4e-3 .. 4.7e-3,
    total 4.6e-8; two frames of a BAIR chunk -- 2.5e-8 .. 5.4e-7 against 2.2e-3 .. 5.5e-3, total 6.4e-8."""
    want_total, want = lpips_restated(ref, gen, P, dtype=torch.float64)
    e = 1e-4
    worst = 0.0
    for l in range(5):
        wbar = float(P[f"lin{l}.model.1.weight"].mean())
        dnorm = torch.sqrt(want[l] / wbar)
        tol = 2 * 4 * e / dnorm
        err = (levels[l] - want[l]).abs() / want[l]
        print(f"lpips split f16 {label} level {l} (C {CHANNELS[l]}): |d| {float(dnorm.min()):.3f} .. {float(dnorm.max()):.3f}, bound {float(tol.min()):.2e}, "
              f"max relative error {float(err.max()):.2e}")
        assert (err <= tol).all(), (l, float(err.max()), float(tol.min()))
        worst = max(worst, float(tol.max()))
    err = float(((total - want_total).abs() / want_total).max())
    print(f"lpips split f16 {label} total: max relative error {err:.2e}, bound {worst:.2e}")
    assert err <= worst


def test_lpips_split_f16_and_s16_taps_on_gpu(P):
    # 24 frames of 128 x 128 in one chunk: conv1_2 and conv2_1 both run on the well-filled tile variants (>= 384 workgroups), so relu1_2 travels as an S16 tensor and the head
    # reads hi + lo halves; the deeper taps are fp32 here (asserted through the debug getter; the BAIR geometry below has more S16 taps)
    ref, gen = seeded_pair(2, 12, 128, 128, seed=9, noise=0.2)
    ctx = M.LPIPS(128, 128, 24, P)
    total, levels = ctx(ref.cuda(), gen.cuda(), return_levels=True)
    assert ctx.tap_formats() & 1, f"relu1_2 did not travel as S16 (formats {ctx.tap_formats():05b})"
    check_split_f16(total, levels, ref, gen, P, "24 x 128 x 128")


def test_lpips_invariants_on_gpu(P):
    ref, gen = (t.cuda() for t in seeded_pair(2, 3, 64, 64, seed=3, noise=0.2))
    ctx = M.LPIPS(64, 64, 4, P)                                                   # 6 frames: two chunks
    total, levels = ctx(ref, ref.clone(), return_levels=True)
    assert (total == 0).all() and (levels == 0).all()
    a, la = ctx(ref, gen, return_levels=True)
    b, lb = ctx(gen, ref, return_levels=True)
    np.testing.assert_allclose(la.numpy(), lb.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=0)
    again, lagain = ctx(ref, gen, return_levels=True)
    assert torch.equal(a, again) and torch.equal(la, lagain)
    c, lc = ctx(ref * 255, gen * 255, 255.0, return_levels=True)
    np.testing.assert_allclose(lc.numpy(), la.numpy(), rtol=1e-4, atol=0)


def test_lpips_bair_evaluation_geometry_on_gpu(P):
    # evaluation of configs/evaluation/01_bair.yaml: 30 observations of 256 x 256, 8 sequences at once -> 8 chunks of 30 frames
    ref, gen = (t.cuda() for t in seeded_pair(8, 30, 256, 256, seed=1))
    got, levels = M.lpips(ref, gen, P, return_levels=True)
    ctx = M._cached_lpips(ref, P, None)
    print(f"LPIPS context: {ctx.max_frames} frames per chunk, workspace {ctx.ws_bytes / 2 ** 30:.2f} GiB, S16 taps {ctx.tap_formats():05b}")
    assert ctx.max_frames == 30 and 2 ** 30 < ctx.ws_bytes < 8 * 2 ** 30
    assert got.shape == (8, 30) and torch.isfinite(got).all() and torch.isfinite(levels).all() and (levels > 0).all()
    again, lagain = M.lpips(ref, gen, P, return_levels=True)
    assert torch.equal(got, again) and torch.equal(levels, lagain)               # bit-identical: fixed-order reductions, no float atomics
    # two frames of the first chunk against the restatement, to the split-f16 bound (more taps travel as S16 here)
    check_split_f16(got[:1, :2], levels[:, :1, :2], ref[:1, :2].cpu(), gen[:1, :2].cpu(), P, "BAIR chunk")
