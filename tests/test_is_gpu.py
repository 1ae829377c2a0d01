"""Inception Score of the dataset evaluation on the MI355X: the new kernel modes of csrc/fid.hip, fc on the implicit-GEMM convolution, the torchvision flavour of the Inception
graph at 299 x 299 with the resize on (exact fp32 and the split-f16 default) against the plain-torch restatement of tests/inception_score_cases.py, one evaluation-geometry case,
and the FID features before and after an IS context has run.  Every test is one bounded pass.

Tolerances, fixed before the first run on the device.
Logits, exact fp32: relative L2 per frame against the fp64 restatement within 8 x the fp32 restatement's own error, floor 1e-6 -- the rule of inception_cases.trunk_case for two
fp32 pipelines that differ in summation order and in where the BatchNorm scale is rounded; fc adds one more layer of the same kind to both sides.
Logits, split f16: the project's feature bound 1e-4 for the 13-layer VGG trunks scaled by the depth of the longest path counted from the graph, fc included
(inception_score_cases.longest_path() = 48): E = 1e-4 * 48 / 13 = 3.69e-4 relative L2 per frame.
Probabilities: p = softmax(z) has the Jacobian diag(p) - p p^T, so dp = p * (dz - <p, dz>) and |dp|_1 <= sum_c p_c |dz_c - <p, dz>| <= 2 max|dz|; with max|dz| <= |dz|_2 <=
E |z|_2 this gives |dp|_1 <= 2 E |z|_2 per frame.  The fp32 softmax itself (exponentials within 4 ulp, a 1000-term sum, one division, the rounding of the stored value:
inception_score_cases.SOFTMAX_RTOL = 7e-5 relative per probability) adds at most 7e-5 to the L1 norm of a row.  D1 = 2 E max_i |z_i|_2 + 7e-5.
Score: ln IS = mean_i KL(p_i || pbar) = H(pbar) - mean_i H(p_i) for one split.  Every row moves by at most D1 in L1, and so does their mean.  The entropy's continuity bound
(Fannes-Audenaert in its classical form: |H(p) - H(q)| <= T ln(K - 1) + h(T) with T = |p - q|_1 / 2 and h the binary entropy in nats) applied to both terms gives
|d ln IS| <= 2 (T ln 999 + h(T)), T = D1 / 2 (inception_score_cases.log_is_bound).  It is a worst-case bound and far from tight: with E = 3.69e-4 and |z|_2 ~ 100 it allows
~0.8 in ln IS.  The case asserts that the fp32 restatement's score sits inside the same bound, and -- so that the bound cannot hide a dead network -- that the fp64 restatement's
per-frame entropy lies in [0.5, ln 1000 - 0.5] nats and its IS above 1.05 (inception_score_cases.check_informative).

Not yet measured on the MI355X: the tests print every figure before they assert; DESIGN.md section 9h records them once they exist."""
import numpy as np
import pytest
import torch

from playablevideogeneration_amd import metrics as M
from tests import inception_cases as IC
from tests import inception_score_cases as SC

pytestmark = pytest.mark.gpu
E_F16 = 1e-4 * SC.longest_path() / 13


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    M.set_library(None)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from playablevideogeneration_amd import _lib
    return M._bind(_lib.load())


@pytest.fixture(scope="module")
def P():
    return SC.make_is_params(resize=True)


@pytest.fixture(scope="module")
def net_case(P):
    """3 frames of 64 x 64 and the restatement's logits at 299 x 299, computed once and left unchanged"""
    frames = SC.varied_frames(3, 64, 64, seed=4)
    return frames, SC.tv_logits(frames, P, torch.float64, True), SC.tv_logits(frames, P, torch.float32, True)


def test_new_kernel_modes(lib, dev):
    sync = torch.cuda.synchronize
    SC.pool_cases(lib, dev, sync=sync)
    SC.stage_cases(lib, dev, sync=sync)
    SC.softmax_cases(lib, dev, sync=sync)


def test_fc_on_conv_igemm_matches_linear(lib, dev):
    SC.fc_cases(lib, dev, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("precision", [0, 16])
def test_network_at_299(dev, P, net_case, precision):
    frames, z64, z32 = net_case
    ctx = M.InceptionProbabilities(64, 64, 2, P, resize=True)      # 3 frames at max_frames 2: crosses a chunk boundary
    ctx.set_precision(precision)
    probs = ctx(frames)
    assert probs.shape == (3, 1000) and probs.dtype == torch.float32 and ctx.fallback_layers() == 0
    logits = ctx.logits()                                          # the last chunk: the third frame
    assert logits.shape == (1, 1000)
    spread = IC.rel_l2(z32, z64)
    tol = max(8 * spread, 1e-6) if precision == 0 else E_F16
    err = IC.rel_l2(logits, z64[2:])
    p64 = torch.softmax(z64, 1)
    want = SC.check_informative(p64, "64x64 -> 299")
    d1_bound = 2 * tol * z64.norm(dim=1).max().item() + SC.SOFTMAX_RTOL
    d1 = (probs.double() - p64).abs().sum(1).max().item()
    got = M.inception_score_from_probabilities(probs.numpy())["is/mean"]
    f32 = M.inception_score_from_probabilities(torch.softmax(z32, 1).numpy())["is/mean"]
    ln_bound = SC.log_is_bound(d1_bound)
    print(f"is network 64x64 -> 299 MI355X precision {precision}: restatement spread {spread:.2e}, logits error (last chunk) {err:.2e} (bound {tol:.2e}); |dp|_1 {d1:.2e} "
          f"(bound {d1_bound:.2e}); IS restated fp64 {want:.6f}, fp32 {f32:.6f}, device {got:.6f}, |d ln IS| {abs(np.log(got / want)):.2e} (bound {ln_bound:.2e})")
    assert err <= tol, (precision, err, tol)
    assert d1 <= d1_bound and (probs.double().sum(1) - 1).abs().max().item() <= 1e-6
    # every frame's logits, through the probabilities: ln p differs from z by a per-row constant, so centred ln p against centred z bounds dz for all three frames
    lz = torch.log(probs.double())
    dz_all = ((lz - lz.mean(1, keepdim=True)) - (z64 - z64.mean(1, keepdim=True)))
    # (the softmax's 7e-5 relative per probability is 7e-5 absolute per ln p: at most 7e-5 sqrt(1000) in L2)
    assert (dz_all.norm(dim=1) / z64.norm(dim=1)).max().item() <= tol + SC.SOFTMAX_RTOL * 1000 ** 0.5 / z64.norm(dim=1).min().item(), "a frame of the first chunk is off"
    assert abs(np.log(f32 / want)) <= ln_bound
    assert abs(np.log(got / want)) <= ln_bound
    assert torch.equal(probs, ctx(frames))                         # run to run: identical bits


def test_evaluation_geometry(dev, P):
    """4 frames of 256 x 256 in the default arithmetic: the input stage's scale factors of the workload (256 / 299), through the cached public entry point"""
    frames = SC.varied_frames(4, 256, 256, seed=5)
    z64 = SC.tv_logits(frames, P, torch.float64, True)
    p64 = torch.softmax(z64, 1)
    want = SC.check_informative(p64, "256x256 -> 299")
    probs = M.inception_probabilities(frames.reshape(2, 2, 3, 256, 256), P)
    ctx = M._cached_is(frames, P, None)
    assert probs.shape == (4, 1000) and ctx.fallback_layers() == 0 and ctx.resize
    err = IC.rel_l2(ctx.logits(), z64)
    d1_bound = 2 * E_F16 * z64.norm(dim=1).max().item() + SC.SOFTMAX_RTOL
    d1 = (probs.double() - p64).abs().sum(1).max().item()
    got = M.inception_score(frames, P)["is/mean"]
    print(f"is 256x256 -> 299 MI355X split f16: logits error {err:.2e} (bound {E_F16:.2e}), |dp|_1 {d1:.2e} (bound {d1_bound:.2e}), IS restated {want:.6f}, device {got:.6f}")
    assert err <= E_F16 and d1 <= d1_bound and abs(np.log(got / want)) <= SC.log_is_bound(d1_bound)


def test_fid_features_are_untouched(dev, P):
    """the shared kernels gained modes, not changes: FID features from a context created before an IS context has run and from one created after it are the same bits"""
    frames = IC.seeded_frames(3, 96, 80, seed=3)
    trunk = {k: v for k, v in P.items() if not k.startswith("fc.")}
    before = M.InceptionFeatures(96, 80, 2, trunk, resize=False)
    fa = before(frames)
    isc = M.InceptionProbabilities(96, 80, 2, P, resize=False)
    pa = isc(frames)
    assert torch.equal(before(frames), fa)
    after = M.InceptionFeatures(96, 80, 2, trunk, resize=False)
    assert torch.equal(after(frames), fa) and torch.equal(isc(frames), pa)
    want = IC.restated_features(frames, trunk, torch.float64, False)
    assert IC.rel_l2(fa, want) <= 1e-4 * IC.longest_path() / 13      # and they are still the FID flavour's features (tests/test_fid_gpu.py's bound)
