"""FID of the dataset evaluation on the MI355X: the kernels of csrc/fid.hip, the Inception trunk at 299 x 299 with the resize on (exact fp32 and the split-f16 default) against the
plain-torch restatement of tests/inception_cases.py, FID end to end, the invariants and the BAIR evaluation geometry.

Split-f16 feature error.  The project's figure for split f16 is e <= 1e-4 relative for the 13-layer VGG trunks (tests/test_lpips_gpu.py: check_split_f16).  Scaled by the depth of
the longest path, counted from the graph (inception_cases.longest_path() = 47): E = 1e-4 * 47 / 13 = 3.62e-4, relative L2 per frame on the 2048-vector; a tapped block of
depth d gets 1e-4 * max(d, 13) / 13.  Fixed before the first run on the device.

FID tolerance.  FID = |mu1 - mu2|^2 + Tr S1 + Tr S2 - 2 Tr sqrt(S1 S2) is homogeneous of degree 2 in the features.  Let every feature vector move by at most e |f_i| and
R_k^2 = mean_i |f_i|^2 = |mu_k|^2 + (N - 1) / N Tr S_k.  To first order in e: |d mu_k| <= e R_k, so d|mu1 - mu2|^2 <= 2 |mu1 - mu2| e (R1 + R2) <= 2 e (R1 + R2)^2 <= 4 e (R1^2 + R2^2);
d Tr S_k = d(mean |f|^2 - |mu|^2) N / (N - 1) <= 2 e R_k^2 + 2 e |mu_k| R_k <= 4 e R_k^2; Tr sqrt(S1 S2) is the nuclear norm of A1^T A2 with A_k the centred feature matrix over
sqrt(N - 1) (|A_k|_F^2 = Tr S_k, |dA_k|_F <= e R_k), so d 2 Tr sqrt(S1 S2) <= 2 e (R1 sqrt(Tr S2) + R2 sqrt(Tr S1)) <= 2 e (R1^2 + R2^2).  Sum: |d FID| <= 10 e (|mu1|^2 + |mu2|^2 +
Tr S1 + Tr S2).  The end-to-end case asserts that the restatement's FID is at least 5 % of Tr S1 + Tr S2 (cancellation cannot hide an error), and that the fp32 restatement
sits inside the same tolerance."""
import numpy as np
import pytest
import torch

from playablevideogeneration_amd import metrics as M
from tests import inception_cases as IC

pytestmark = pytest.mark.gpu
E_F16 = 1e-4 * IC.longest_path() / 13
BLOCK_DEPTH = (3, 5, 37, 47)      # convolutions in front of each block output on the longest path: stem 3, + 2, + A 3 x 3 + B 3 + C 4 x 5, + D 4 + E 2 x 3


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
    return IC.make_inception_params()


@pytest.mark.parametrize("precision", [0, 16])
def test_conv_igemm_matches_conv2d(lib, dev, precision):
    for case in IC.CONV_CASES:
        IC.conv_case(lib, dev, case, precision, N=3, sync=torch.cuda.synchronize)
    # the trunk's own geometries: odd sizes, stride 2, tile tails over several workgroups
    for case in [(3, 32, (3, 3), 2, (0, 0), 299, 299), (32, 32, (3, 3), 1, (0, 0), 149, 149), (288, 384, (3, 3), 2, (0, 0), 35, 35), (768, 192, (1, 1), 1, (0, 0), 17, 17)]:
        IC.conv_case(lib, dev, case, precision, N=2, sync=torch.cuda.synchronize)


def test_poolings_and_resize(lib, dev):
    IC.pool_cases(lib, dev, sync=torch.cuda.synchronize)
    IC.resize_cases(lib, dev, [(64, 64), (256, 256), (208, 160), (299, 299)], sync=torch.cuda.synchronize)


def test_trunk_exact_fp32_at_299(dev, P):
    frames = IC.seeded_frames(3, 256, 256, seed=4)
    ctx = M.InceptionFeatures(256, 256, 2, P, resize=True)
    ctx.set_precision(0)
    IC.trunk_case(ctx, frames, P, True, label="256x256 -> 299 MI355X exact fp32")


def test_trunk_split_f16_default(dev, P):
    frames = IC.seeded_frames(3, 256, 256, seed=5)
    ctx = M.InceptionFeatures(256, 256, 4, P, resize=True)      # the default arithmetic
    feats = ctx(frames)
    assert ctx.fallback_layers() == 0
    w64 = IC.inception_restated(frames, P, torch.float64, True)
    for b in range(4):
        got = ctx.block(b) if b < 3 else feats.reshape(-1, 2048, 1, 1)
        err, tol = IC.rel_l2(got, w64[b]), 1e-4 * max(BLOCK_DEPTH[b], 13) / 13
        print(f"fid trunk split f16 block {b}: error {err:.2e}, bound {tol:.2e}")
        assert err <= tol, (b, err, tol)


def test_invariants(dev, P):
    frames = IC.seeded_frames(20, 128, 160, seed=6)
    a = M.InceptionFeatures(128, 160, 4, P)
    b = M.InceptionFeatures(128, 160, 16, P)
    fa = a(frames)
    assert torch.equal(fa, a(frames))                      # two calls: identical bits
    assert torch.equal(fa, b(frames))                      # max_frames 4 and 16: identical bits (frames are independent)
    m, s = M.activation_statistics(fa.numpy())
    assert abs(M.frechet_distance(m, s, m, s)) <= 1e-8 * np.trace(s)
    assert abs(M.fid(frames, frames.clone(), P)) <= 1e-8 * np.trace(s)


def test_fid_end_to_end(dev, P):
    n = 64
    ref = IC.seeded_frames(n, 128, 128, seed=7)
    gen = IC.seeded_frames(n, 128, 128, seed=8, noise=0.25)      # visibly degraded
    f64r, f64g = IC.restated_features(ref, P, torch.float64).numpy(), IC.restated_features(gen, P, torch.float64).numpy()
    (m1, s1), (m2, s2) = M.activation_statistics(f64r), M.activation_statistics(f64g)
    want = M.frechet_distance(m1, s1, m2, s2)
    assert want >= 0.05 * (np.trace(s1) + np.trace(s2)), (want, np.trace(s1), np.trace(s2))
    tol = 10 * E_F16 * (m1.dot(m1) + m2.dot(m2) + np.trace(s1) + np.trace(s2))
    f32 = M.fid_from_features(IC.restated_features(ref, P, torch.float32).double().numpy(), IC.restated_features(gen, P, torch.float32).double().numpy())
    got = M.fid(ref, gen, P)
    print(f"fid end to end: restatement fp64 {want:.6f}, fp32 {f32:.6f}, MI355X split f16 {got:.6f}; |error| {abs(got - want):.3e} ({abs(got - want) / want:.2e} relative), "
          f"tolerance {tol:.3e}")
    assert abs(f32 - want) <= tol
    assert abs(got - want) <= tol


def test_bair_geometry(lib, dev, P):
    frames = IC.seeded_frames(8 * 30, 256, 256, seed=9).reshape(8, 30, 3, 256, 256)
    ctx = M._cached_fid(frames, P, None)
    act = ctx.max_frames * 147 * 147 * 64 * 4
    weights = 2 * lib.caddy_fid_param_floats() * 4 * 1.3      # both packed forms, channel padding to 32 / 64 (<= 30 % on this table)
    print(f"FID workspace, BAIR 8 x 30 x 256 x 256 in chunks of {ctx.max_frames}: {ctx.ws_bytes / 2 ** 30:.2f} GiB; largest activation {act / 2 ** 30:.2f} GiB")
    # live at once in the stem: the 149^2 x 32, 147^2 x 32 and 147^2 x 64 maps (2.03 largest maps), the image, the three tapped maps and the two block-output slots (< 1.4): < 4
    assert ctx.ws_bytes <= 4 * act + weights + 2 ** 20
    feats = ctx(frames)
    assert feats.shape == (240, 2048) and torch.isfinite(feats).all()
    want = IC.restated_features(frames[0, :2], P, torch.float64)
    assert IC.rel_l2(feats[:2], want) <= E_F16
