"""VGG19 perceptual loss: the feature-L1 sums of relu1_1 .. relu4_1 taken out of the seed epilogue of the dgrad above each tap (ConvArgs.l1_acc, caddy_debug_set_perc_fuse_l1)
against the stand-alone pass over both feature maps, same library, same forward pass.

The seed, mask and routing expressions do not change, only who sums |f_rec - f_gt| does: every gradient must be BIT-IDENTICAL with the switch off and on, and the level sums
-- double sums of the same fp32 differences in another order -- may differ by reassociation in double only.  Bound on the level sums: 1e-12 relative.  They are sums of at most
~7e8 non-negative terms; reassociating such a sum in double moves it by a few 2^-53 ~ 1e-16 per level of the reduction tree, many orders below the bound, while a dropped or
doubled 16 x 16-pixel tile of the smallest map here moves it by > 1e-4.

Runs on the GPU with the two perceptual golden configurations and the odd-pooling geometry, and on the host simulator (split-operand kernels, the arithmetic of the MI355X
runs: the exact-fp32 path never takes the fused form) with the same checks at the smallest geometries the loss accepts.  The simulator needs about 7 minutes on 8 cores for ONE
pass over a golden configuration with the split-operand VGG19 (measured: perc_pre_reduced_s1) and six times that for the 208 x 160 frames, which is why the reference goldens
perc_* have always been GPU-only (test_model_emu.py: test_perceptual_loss_small); its cases here are a 64 x 64 clip in one and in several chunks of time steps and the 64 x 80
clip whose quarter resolution goes 16x20 -> 8x10 -> 4x5 -> 2x2 through the max-pools (floor)."""
import ctypes as C

import pytest
import torch

from oracle import caddy_oracle as O
from tests import helpers as H
from tests import model_cases as M

ODD_POOLING = dict(variant="reduced", K=3, Da=1, Ch=64, S=1, B=2, T=3, H=208, W=160, gt=1, tau=0.6, pre=False, perc=1.0)      # the sizes of test_perceptual_loss_odd_pooling_sizes
SMALL = dict(variant="reduced", K=3, Da=1, Ch=64, S=1, B=1, T=3, H=64, W=64, gt=1, tau=0.8, pre=False, perc=0.7)             # simulator: two reconstructed frames
SMALL_ODD = dict(variant="reduced", K=3, Da=1, Ch=64, S=1, B=1, T=2, H=64, W=80, gt=1, tau=0.8, pre=False, perc=0.7)         # simulator: the geometry of test_perceptual_loss_small
BACKENDS = [pytest.param("emu", marks=pytest.mark.emu), pytest.param("gpu", marks=pytest.mark.gpu)]
CASES = [pytest.param("gpu", n, ch, marks=pytest.mark.gpu) for n in ("perc_main_s1", "perc_pre_reduced_s1", "odd_pooling") for ch in (1, 3)] + \
        [pytest.param("emu", n, ch, marks=pytest.mark.emu) for n, ch in (("small", 1), ("small", 3), ("small_odd", 1))]      # (3 chunks of 2 frames: clamped to one per frame)


def _backend(which):
    if which == "gpu":
        from playablevideogeneration_amd import _lib
        assert torch.cuda.is_available()
        return _lib.load(), "cuda"
    from tests.emu.loader import load_emu
    return load_emu(), "cpu"


def _case(name):
    if name in ("odd_pooling", "small", "small_odd"):
        return dict({"odd_pooling": ODD_POOLING, "small": SMALL, "small_odd": SMALL_ODD}[name])
    return H.load_case(name)[0]


def _off_and_on(lib, dev, c, chunks, exact_vgg=False):
    """one forward pass, then loss_backward with the fusion off and on -> [(losses, flat parameter gradient, [d(total)/d(rec_r)])] x 2"""
    d, P, obs = H.inputs_of(c)
    nz = O.Noise()
    torch.manual_seed(H.NOISE_SEED)
    orc = O.Oracle(d, {k: v.clone() for k, v in P.items()}, training=True)
    with torch.no_grad():      # (records the noise the engine replays)
        orc.forward_pretraining(obs, tau=c["tau"], noise=nz) if c["pre"] else orc.forward_full(obs, c["gt"], tau=c["tau"], noise=nz)
    eng = M.make_engine(c, lib, dev, perceptual=True)
    if exact_vgg:
        eng.set_vgg_precision(0, 0)
    eng.load_state_dict(P)
    eng.load_vgg(O.make_vgg_params())
    for f in (lib.caddy_debug_set_perc_chunks, lib.caddy_debug_set_perc_fuse_l1):
        f.argtypes = [C.c_void_p, C.c_int]
    lib.caddy_debug_set_perc_chunks(eng.ctx, chunks)
    nd = M.noise_dict(nz.record, c["B"], c["T"], c["K"], c["Da"])
    out = eng.forward_pretraining(obs, c["tau"], nd, training=True) if c["pre"] else eng.forward_full(obs, c["gt"], c["tau"], nd, training=True)
    w = dict(H.LOSS_W, perceptual=c["perc"])
    res = []
    for fuse in (0, 1):
        lib.caddy_debug_set_perc_fuse_l1(eng.ctx, fuse)
        losses = eng.loss_backward(w, smooth_mi=True, mi_alpha=0.2, update_mi_ema=False)
        res.append((losses, eng.grads.clone().cpu(), [eng.output_grad(100 + r, out[1][r]).cpu() for r in range(3)]))
    return res


def _compare(res, what):
    (l0, g0, s0), (l1, g1, s1) = res
    for r in range(3):
        assert torch.isfinite(s0[r]).all() and s0[r].abs().sum().item() > 0, (what, r)
        assert torch.equal(s0[r], s1[r]), (what, "d(rec_r)", r, (s0[r] - s1[r]).abs().max().item())
    assert torch.isfinite(g0).all() and g0.abs().sum().item() > 0, what
    assert torch.equal(g0, g1), (what, "parameter gradient", (g0 - g1).abs().max().item())
    worst = 0.0
    for r in range(3):
        for l in range(5):
            k = f"perceptual_loss_r{r}_l{l}"
            assert l0[k] > 0, (what, k, l0[k])      # every term is there, fused or not
            rel = abs(l0[k] - l1[k]) / abs(l0[k])
            worst = max(worst, rel)
            print(what, k, l0[k], l1[k], rel)
            assert rel <= 1e-12, (what, k, l0[k], l1[k], rel)
    return worst


@pytest.mark.parametrize("backend,name,chunks", CASES)
def test_fused_feature_l1_matches_stand_alone_pass(backend, name, chunks):
    """GPU: the two perceptual golden configurations and one with odd pooled sizes; simulator: their small stand-ins -- one chunk of time steps and three: gradients
    bit-identical, level sums within 1e-12"""
    lib, dev = _backend(backend)
    M.SIM_SPLIT = True      # (simulator: the split-operand kernels, whose masked epilogue carries the sum)
    try:
        res = _off_and_on(lib, dev, _case(name), chunks)
    finally:
        M.SIM_SPLIT = False
    print(name, chunks, "worst relative difference of a level sum", _compare(res, f"{name} chunks={chunks}"))


@pytest.mark.parametrize("backend", BACKENDS)
def test_exact_fp32_vgg_keeps_the_stand_alone_pass(backend):
    """exact-fp32 VGG19 convolutions: the masked dgrads run on a kernel without the sum, conv_hx_l1_ok rejects them and the switch changes nothing -- every level sum is still
    produced (and, both settings launching the same kernels, agrees within the same bound)"""
    lib, dev = _backend(backend)
    res = _off_and_on(lib, dev, _case("perc_pre_reduced_s1" if backend == "gpu" else "small_odd"), 1, exact_vgg=True)
    _compare(res, "exact fp32")
