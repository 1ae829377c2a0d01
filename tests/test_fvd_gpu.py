"""FVD of the dataset evaluation on the MI355X: the kernels of csrc/fvd.hip, the I3D trunk at 224 x 224 with the legacy resize on (exact fp32 and the split-f16 default) against the
plain-torch restatement of tests/i3d_cases.py, FVD end to end, the invariants and the BAIR evaluation geometry.

Split-f16 embedding error.  The project's figure for split f16 is e <= 1e-4 relative L2 for the 13-convolution VGG trunks (tests/test_lpips_gpu.py: check_split_f16).  Scaled by the
depth of the longest path, counted from the restatement's walk (i3d_cases.longest_path() = 22): E = 1e-4 * 22 / 13 = 1.69e-4 per video on the 400 logits; a tapped block of depth d
gets 1e-4 * max(d, 13) / 13.  Fixed before the first run on the device.

FVD tolerance: |d FVD| <= 10 E (|mu1|^2 + |mu2|^2 + Tr S1 + Tr S2), the derivation of tests/test_fid_gpu.py's docstring (it holds for any embedding).  The end-to-end case asserts
that the restatement's FVD is at least 5 % of Tr S1 + Tr S2 (cancellation cannot hide an error) and that the fp32 restatement sits inside the same tolerance; its degradation level
(noise 0.25) was picked on the CPU with the restatement alone, before the first device run."""
import numpy as np
import pytest
import torch

from playablevideogeneration_amd import metrics as M
from tests import i3d_cases as I3

pytestmark = pytest.mark.gpu
sync = torch.cuda.synchronize


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    M.set_library(None)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from playablevideogeneration_amd import _lib
    return I3.bind_kernels(M._bind(_lib.load()))


@pytest.fixture(scope="module")
def P():
    return I3.make_i3d_params()


@pytest.fixture(scope="module")
def depths():
    d = I3.block_depths()
    assert d[4] == I3.longest_path() == 22
    return d


@pytest.mark.parametrize("precision", [0, 16])
def test_conv3d_igemm_matches_conv3d(lib, dev, precision):
    for case in I3.CONV3D_CASES:
        I3.conv3d_case(lib, dev, case, precision, N=2, sync=sync)
    # the trunk's own geometries at 224: conv1 on 10 x 224 x 224, Mixed_3b's 3x3x3 on 5 x 28 x 28, Mixed_5c's widest 1x1x1 on 2 x 7 x 7
    for case in [(3, 64, (7, 7, 7), (2, 2, 2), (10, 224, 224)), (96, 128, (3, 3, 3), (1, 1, 1), (5, 28, 28)), (832, 384, (1, 1, 1), (1, 1, 1), (2, 7, 7))]:
        I3.conv3d_case(lib, dev, case, precision, N=2, sync=sync)


@pytest.mark.parametrize("precision", [0, 16])
def test_conv3d_igemm_is_conv_igemm_bit_for_bit(lib, dev, precision):
    for case in I3.CROSS_CASES:
        I3.cross_case(lib, dev, case, precision, N=2, sync=sync)


def test_pools_and_stage(lib, dev):
    I3.pool_cases(lib, dev, sync=sync)
    I3.stage_cases(lib, dev, [(64, 64), (208, 160), (224, 224)], sync=sync)


@pytest.fixture(scope="module")
def trunk_videos():
    return I3.seeded_videos(2, 10, 64, 64, seed=4)


@pytest.fixture(scope="module")
def trunk_want(trunk_videos, P):
    """the fp64 and fp32 restatements of the two trunk videos, computed once"""
    return I3.i3d_restated(trunk_videos, P, torch.float64, True), I3.i3d_restated(trunk_videos, P, torch.float32, True)


def test_trunk_exact_fp32_at_224(dev, P, trunk_videos, trunk_want):
    ctx = M.I3DEmbeddings(10, 64, 64, 2, P, resize=True)
    ctx.set_precision(0)
    emb = ctx(trunk_videos)
    w64, w32 = trunk_want
    for b in range(5):
        got = ctx.block(b) if b < 4 else emb
        spread, err = I3.rel_l2(w32[b], w64[b]), I3.rel_l2(got, w64[b])
        tol = max(8 * spread, 1e-6)      # the FID exact-path rule (inception_cases.trunk_case)
        print(f"fvd trunk 64x64 -> 224 MI355X exact fp32 block {b}: restatement spread {spread:.2e}, kernel error {err:.2e}, bound {tol:.2e}")
        assert tuple(got.shape) == tuple(w64[b].shape) and err <= tol, (b, err, tol)


def test_trunk_split_f16_default(dev, P, trunk_videos, trunk_want, depths):
    ctx = M.I3DEmbeddings(10, 64, 64, 2, P, resize=True)      # the default arithmetic
    emb = ctx(trunk_videos)
    assert ctx.fallback_layers() == 0
    for b in range(5):
        got = ctx.block(b) if b < 4 else emb
        err, tol = I3.rel_l2(got, trunk_want[0][b]), 1e-4 * max(depths[b], 13) / 13
        print(f"fvd trunk split f16 block {b} (depth {depths[b]}): error {err:.2e}, bound {tol:.2e}")
        assert err <= tol, (b, err, tol)


def test_invariants(dev, P):
    videos = I3.seeded_videos(10, 6, 48, 40, seed=6)
    a = M.I3DEmbeddings(6, 48, 40, 2, P)
    b = M.I3DEmbeddings(6, 48, 40, 8, P)
    ea = a(videos)
    assert torch.equal(ea, a(videos))                      # two calls: identical bits
    assert torch.equal(ea, b(videos))                      # max_videos 2 and 8: identical bits (videos are independent)
    m, s = M.activation_statistics(ea.numpy())
    assert abs(M.frechet_distance(m, s, m, s)) <= 1e-8 * np.trace(s)
    assert abs(M.fvd_from_embeddings(ea.numpy(), b(videos.clone()).numpy())) <= 1e-8 * np.trace(s)


def test_fvd_end_to_end(dev, P):
    E = 1e-4 * I3.longest_path() / 13
    ref = I3.seeded_videos(32, 12, 64, 64, seed=7)
    gen = I3.seeded_videos(32, 12, 64, 64, seed=8, noise=0.25)      # visibly degraded
    e64r, e64g = I3.restated_embeddings(ref, P, torch.float64, False, batch=16).numpy(), I3.restated_embeddings(gen, P, torch.float64, False, batch=16).numpy()
    (m1, s1), (m2, s2) = M.activation_statistics(e64r), M.activation_statistics(e64g)
    want = M.frechet_distance(m1, s1, m2, s2)
    assert want >= 0.05 * (np.trace(s1) + np.trace(s2)), (want, np.trace(s1), np.trace(s2))
    tol = 10 * E * (m1.dot(m1) + m2.dot(m2) + np.trace(s1) + np.trace(s2))
    f32 = M.fvd_from_embeddings(I3.restated_embeddings(ref, P, torch.float32, False, batch=16).double().numpy(), I3.restated_embeddings(gen, P, torch.float32, False, batch=16).double().numpy())
    got = M.fvd(ref, gen, P, resize=False)
    print(f"fvd end to end: restatement fp64 {want:.6f}, fp32 {f32:.6f}, MI355X split f16 {got:.6f}; |error| {abs(got - want):.3e} ({abs(got - want) / want:.2e} relative), "
          f"tolerance {tol:.3e}")
    assert abs(f32 - want) <= tol
    assert abs(got - want) <= tol


def test_bair_geometry(lib, dev, P):
    E = 1e-4 * I3.longest_path() / 13
    videos = I3.seeded_videos(8, 30, 256, 256, seed=9)
    ctx = M._cached_fvd(videos, P, None)
    act = ctx.max_videos * 15 * 112 * 112 * 64 * 4      # the conv1 output of a chunk
    packed = sum(2 * lib.caddy_k_conv3d_weight_bytes(s[3], s[4], s[0], s[1], s[2]) for _, _, s, _ in M.fvd_param_table() if len(s) == 5)      # both packed forms
    print(f"FVD workspace, BAIR 8 x 30 x 256 x 256 in chunks of {ctx.max_videos}: {ctx.ws_bytes / 2 ** 30:.2f} GiB; largest activation {act / 2 ** 30:.2f} GiB, "
          f"packed weights {packed / 2 ** 20:.0f} MiB")
    # in units of the conv1 output (15 x 112^2 x 64): live through the chunk are the four tapped maps (0.75 + 0.47 + 0.11 + 0.02) and the two block-output slots (2 x 0.25); on
    # top of them the stem holds the pitch-4 image (0.5), the conv1 output (1), its pooled map (0.25) and Conv3d_2b's output (0.25): 3.85 < 4
    assert ctx.ws_bytes <= 4 * act + packed + 2 ** 20
    emb = ctx(videos)
    assert emb.shape == (8, 400) and torch.isfinite(emb).all()
    want = I3.restated_embeddings(videos[:1], P, torch.float64)
    assert I3.rel_l2(emb[:1], want) <= E
