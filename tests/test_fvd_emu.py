"""FVD of the dataset evaluation on the host simulator build (tests/emu), exact fp32: the kernels of csrc/fvd.hip against their torch calls, the I3D trunk against the plain-torch
restatement of tests/i3d_cases.py (resize off, 9 frames of 32 x 32: the simulator stays fast), the weight loader, the C ABI error paths and the three evaluators.

Split f16 on the simulator: the convolution unit cases run both arithmetics; the trunk runs exact fp32 only (the split-f16 trunk is checked on the MI355X, tests/test_fvd_gpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from playablevideogeneration_amd import metrics as M
from playablevideogeneration_amd.engine import CaddyError
from tests import i3d_cases as I3
from tests.emu.loader import load_emu

pytestmark = pytest.mark.emu
T0, H0, W0 = 9, 32, 32


@pytest.fixture(scope="module")
def emu():
    lib = load_emu()
    M.set_library(lib)
    yield lib
    M.set_library(None)


@pytest.fixture(scope="module")
def P():
    return I3.make_i3d_params()


@pytest.mark.parametrize("case", I3.CONV3D_CASES, ids=lambda c: f"{c[0]}to{c[1]}_k{c[2][0]}x{c[2][1]}x{c[2][2]}_s{c[3][0]}{c[3][1]}{c[3][2]}")
@pytest.mark.parametrize("precision", [0, 16])
def test_conv3d_igemm_matches_conv3d(emu, case, precision):
    I3.conv3d_case(emu, torch.device("cpu"), case, precision, N=2)


@pytest.mark.parametrize("case", I3.CROSS_CASES, ids=lambda c: f"{c[0]}to{c[1]}_k{c[2][0]}x{c[2][1]}_s{c[3]}")
@pytest.mark.parametrize("precision", [0, 16])
def test_conv3d_igemm_is_conv_igemm_bit_for_bit(emu, case, precision):
    I3.cross_case(emu, torch.device("cpu"), case, precision, N=2)


def test_pools_match_max_pool3d(emu):
    I3.pool_cases(emu, torch.device("cpu"))


def test_stage_is_the_legacy_tf_resize(emu):
    I3.stage_cases(emu, torch.device("cpu"), [(64, 64), (208, 160), (224, 224)])


def test_parameter_table_is_the_restatement_s(emu, P):
    """the table of csrc/fvd.hip against the structure the restatement states: 57 convolutions + logits, TF names, DHWIO shapes, offsets; 22 on the longest path"""
    lib = M._bind(emu)
    assert I3.conv_count() == 58 and I3.longest_path() == 22 and len(P) == 57 * 4 + 2
    table = M.fvd_param_table(emu)
    required = [t for t in table if not t[3]]
    floats = 0
    for (name, off, shape, _), (want_name, want) in zip(required, P.items()):
        assert name == want_name and int(np.prod(shape)) == want.numel() and off == floats, (name, want_name)
        assert shape == tuple(want.shape) or (len(shape) == 1 and tuple(want.shape) == (1, 1, 1, 1) + shape), name
        floats += want.numel()
    assert len(required) == len(P)
    gammas = [t for t in table if t[3]]
    assert [g[0] for g in gammas] == [k.replace("/conv_3d/w", "/batch_norm/gamma") for k in P if k.endswith("/conv_3d/w") and not k.startswith("Logits")]
    for name, off, shape, _ in gammas:
        assert off == floats and shape == tuple(P[name.replace("/batch_norm/gamma", "/batch_norm/beta")].reshape(-1).shape)
        floats += shape[0]
    assert lib.caddy_fvd_param_count() == len(table) == 57 * 5 + 2 and lib.caddy_fvd_param_floats() == floats
    from playablevideogeneration_amd.engine import ParamInfo
    assert lib.caddy_fvd_param_info_get(len(table), C.byref(ParamInfo()), None) != 0 and lib.caddy_fvd_param_info_get(-1, C.byref(ParamInfo()), None) != 0
    # the multiply-accumulates of one 64-frame 224 x 224 video, counted from the graph (the commonly quoted figure is 108 G)
    macs = lib.caddy_fvd_macs_per_video(64, 224, 224, 1)
    print(f"I3D trunk: {macs / 1e9:.2f} GMAC per 64 x 224 x 224 video")
    assert 1.0e11 < macs < 1.2e11


def test_trunk_matches_restatement(emu, P):
    videos = I3.seeded_videos(3, T0, H0, W0, seed=4)
    ctx = M.I3DEmbeddings(T0, H0, W0, 2, P, resize=False, lib=emu)      # 3 videos at max_videos 2: crosses a chunk boundary
    ctx.set_precision(0)
    emb = I3.trunk_case(ctx, videos, P, False, label=f"{T0}x{H0}x{W0} emu")
    assert torch.equal(emb, ctx(videos))                                 # bit-identical: one writer per element, fixed summation order
    one = M.I3DEmbeddings(T0, H0, W0, 1, P, resize=False, lib=emu)
    one.set_precision(0)
    assert torch.equal(one(videos[:2]), emb[:2])                         # videos are independent: the chunking does not matter
    with pytest.raises(ValueError):
        ctx(videos[:, :, :, :30])
    with pytest.raises(ValueError):
        ctx(videos[:, :8])
    e = M.i3d_embeddings(videos[:1], P, lib=emu, resize=False)
    assert torch.equal(e, emb[:1])                                       # (the simulator default is exact fp32 too)
    assert M._cached_fvd(videos[:1], P, emu, False) is M._cached_fvd(videos[1:2], P, emu, False)
    with pytest.raises(ValueError):
        M.i3d_embeddings(videos, None, lib=emu)


@pytest.mark.parametrize("with_gamma", [False, True])
def test_packer_folds_batch_norm(emu, with_gamma):
    """DHWIO -> packed with the fold w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps) (g = 1 without gamma) against eval-mode F.batch_norm"""
    g = torch.Generator().manual_seed(1)
    Cin, Cout = 32, 48
    x = torch.randn(2, Cin, 3, 5, 4, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 0.05
    gam = 0.5 + torch.rand(Cout, generator=g) if with_gamma else None
    bet, mu, var = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g), 0.1 + torch.rand(Cout, generator=g)
    want = F.relu(F.batch_norm(F.conv3d(x.double(), w.double(), None, 1, 1), mu.double(), var.double(), None if gam is None else gam.double(), bet.double(), False, 0.0, I3.BN_EPS))
    got, _, flag, _ = I3.run_conv3d(emu, torch.device("cpu"), x, w, None, (1, 1, 1), 0, bn=(gam, bet, mu, var))
    err = (got.double() - want).abs().max().item() / max(1.0, want.abs().max().item())
    assert flag == 0 and err < I3.CONV_TOL, err
    lib = I3.bind_kernels(emu)
    wd = w.permute(2, 3, 4, 1, 0).contiguous()
    assert lib.caddy_k_conv3d_pack(wd.data_ptr(), None, bet.data_ptr(), None, None, I3.BN_EPS, None, Cin, Cout, 3, 3, 3, None, None, None, None) != 0      # beta without statistics
    assert lib.caddy_k_conv3d_pack(wd.data_ptr(), None, None, None, None, 0.0, None, Cin, Cout, 3, 3, 8, None, None, None, None) != 0                       # KW > 7


def test_loader_names(emu, P):
    full = {("RGB/inception_i3d/" + k + ":0"): v for k, v in P.items()} | {"RGB/inception_i3d/global_step:0": torch.zeros(1)}
    state = M.fvd_i3d_state(full)
    assert list(state) == list(P)
    assert set(M.fvd_i3d_state({"state_dict": {("module." + k): v for k, v in P.items()}})) == set(P)
    old, new = "Mixed_5b/Branch_2/Conv3d_0b_3x3/", "Mixed_5b/Branch_2/Conv3d_0a_3x3/"
    published = {(new + k[len(old):] if k.startswith(old) else k): v for k, v in P.items()}
    assert old + "conv_3d/w" not in published and new + "conv_3d/w" in published
    alias = M.fvd_i3d_state(published)
    assert list(alias) == list(P) and all(torch.equal(alias[k].reshape(-1), P[k].reshape(-1)) for k in P)
    with pytest.raises(CaddyError, match=r"Mixed_4c/Branch_2/Conv3d_0b_3x3/batch_norm/moving_variance"):
        M.fvd_i3d_state({k: v for k, v in P.items() if k != "Mixed_4c/Branch_2/Conv3d_0b_3x3/batch_norm/moving_variance"})
    wrong = dict(P)
    wrong["Mixed_3b/Branch_1/Conv3d_0b_3x3/conv_3d/w"] = torch.zeros(3, 3, 1, 96, 128)
    with pytest.raises(CaddyError, match=r"Mixed_3b/Branch_1/Conv3d_0b_3x3/conv_3d/w"):
        M.fvd_i3d_state(wrong)
    assert M.find_fvd_weights({}) is None
    assert list(M.find_fvd_weights({"fvd_i3d_weights": full})) == list(P)


def test_loader_reads_npz_and_torch_files_and_gamma_reaches_the_kernels(emu, tmp_path):
    Pg = I3.make_i3d_params(gamma=True)
    np.savez(str(tmp_path / "i3d.npz"), **{("RGB/inception_i3d/" + k + ":0"): v.numpy() for k, v in Pg.items()})
    torch.save(dict(Pg), str(tmp_path / "i3d.pth"))
    a, b = M.fvd_i3d_state(str(tmp_path / "i3d.npz")), M.fvd_i3d_state(str(tmp_path / "i3d.pth"))
    assert list(a) == list(b) and len(a) == 57 * 5 + 2 and all(torch.equal(a[k], b[k].reshape(a[k].shape)) for k in a)
    videos = I3.seeded_videos(1, 4, 16, 16, seed=2)
    ctx = M.I3DEmbeddings(4, 16, 16, 1, a, resize=False, lib=emu)
    ctx.set_precision(0)
    I3.trunk_case(ctx, videos, Pg, False, label="4x16x16 emu with gamma")


def test_fvd_c_abi(emu, P):
    lib = M._bind(emu)
    err = lambda: lib.caddy_last_error().decode()
    assert lib.caddy_fvd_workspace_bytes(0, 4, 16, 16, 0) == 0 and "positive" in err()
    assert lib.caddy_fvd_workspace_bytes(1, 0, 16, 16, 0) == 0 and lib.caddy_fvd_workspace_bytes(1, 4, 16, 0, 1) == 0
    assert lib.caddy_fvd_macs_per_video(0, 16, 16, 0) == 0.0
    n = lib.caddy_fvd_workspace_bytes(1, 4, 16, 16, 0)
    assert n > 0
    buf = torch.empty(n + 256, dtype=torch.uint8)
    base = buf.data_ptr() + (-buf.data_ptr()) % 256
    assert not lib.caddy_fvd_ctx_create(1, 4, 16, 16, 0, None, n) and "null" in err()
    assert not lib.caddy_fvd_ctx_create(1, 4, 16, 16, 0, base + 16, n) and "aligned" in err()
    assert not lib.caddy_fvd_ctx_create(1, 4, 16, 16, 0, base, n // 2) and "too small" in err() and "caddy_fvd_workspace_bytes" in err()
    bare = lib.caddy_fvd_ctx_create(1, 4, 16, 16, 0, base, n)
    assert bare
    x = torch.rand(1, 4, 3, 16, 16)
    out = torch.full((1, 400), -7.0, dtype=torch.float64)
    assert lib.caddy_fvd_embeddings(bare, x.data_ptr(), 1, out.data_ptr()) == -2 and "caddy_load_fvd_i3d" in err()
    assert lib.caddy_fvd_embeddings(bare, None, 1, out.data_ptr()) == -2 and lib.caddy_fvd_embeddings(bare, x.data_ptr(), 0, out.data_ptr()) == -2
    assert lib.caddy_load_fvd_i3d(bare, None) == -2 and lib.caddy_set_fvd_precision(bare, 17) == -2
    assert lib.caddy_debug_fvd_block(bare, 0, x.data_ptr()) == -2 and lib.caddy_debug_fvd_stage_ms(bare, 0, (C.c_float * 5)()) == -2
    nine = torch.full((9, 1, 1), -7.0, dtype=torch.float64)
    assert lib.caddy_frame_metrics(bare, x.data_ptr(), x.data_ptr(), 1, 1, 1.0, 0, nine.data_ptr()) == -2
    assert lib.caddy_fid_features(bare, x.data_ptr(), 1, out.data_ptr()) == -2 and "caddy_fid_ctx_create" in err()
    fm = M.FrameMetrics(32, 32, 2, lib=emu)
    assert lib.caddy_fvd_embeddings(fm.ctx, x.data_ptr(), 1, out.data_ptr()) == -2 and "caddy_fvd_ctx_create" in err()
    assert lib.caddy_debug_fvd_fallback_layers(fm.ctx) == -1 and lib.caddy_debug_fvd_fallback_layers(bare) == 0
    assert (out == -7).all() and (nine == -7).all()
    lib.caddy_ctx_destroy(bare)
    # bad geometry at the kernel entry points
    I3.bind_kernels(lib)
    t = torch.zeros(1, 2, 4, 4, 16)
    o = torch.zeros(1, 2, 2, 2, 16)
    assert lib.caddy_k_fvd_pool(C.byref(I3.v5_of(t)), C.byref(I3.v5_of(o)), 3, 3, 3, 1, 2, 2, None) == 0
    assert lib.caddy_k_fvd_pool(C.byref(I3.v5_of(t)), C.byref(I3.v5_of(o)), 3, 3, 3, 2, 2, 2, None) != 0      # out.T must be ceil(2 / 2)
    assert lib.caddy_k_fvd_pool(C.byref(I3.v5_of(t, 6)), C.byref(I3.v5_of(o, 6)), 3, 3, 3, 1, 2, 2, None) != 0   # C % 4
    a = I3.Conv3dArgs()
    assert lib.caddy_k_conv3d_igemm(C.byref(a), None) != 0
    assert lib.caddy_k_fvd_stage(None, 1, 4, 4, t.data_ptr(), 4, 4, None) != 0


# ---- the evaluators: 35 sequences (32 enter the statistics), resize off ----
N_SEQ = 35


def _sequences(cfg, size):
    from playablevideogeneration_amd.video_dataset import VideoDataset, evaluation_transform
    b = cfg["evaluation"]["batching"]
    out = []
    for side in ("reference_data", "generated_data"):
        ds = VideoDataset(cfg[side]["data_root"], b, evaluation_transform(cfg[side]["crop"], size))
        out.append((ds, torch.stack([torch.stack([s[0] for s in ds[i].observations]) for i in range(len(ds))])))
    return out


def _want_fvd(r, g, P):
    assert len(r) == N_SEQ and len(g) == N_SEQ
    return M.fvd_from_embeddings(I3.restated_embeddings(r[:32], P, torch.float64, False, batch=32).numpy(), I3.restated_embeddings(g[:32], P, torch.float64, False, batch=32).numpy())


def test_dataset_evaluator_adds_fvd_only_with_weights(emu, P, tmp_path):
    from playablevideogeneration_amd import dataset_evaluator as DE
    from playablevideogeneration_amd.drivers import HeadlessLogger, load_evaluation_configuration
    from tests.test_frame_metrics_emu import _write_videos
    EH, EW = 16, 20
    wpath = str(tmp_path / "i3d.npz")
    np.savez(wpath, **{("RGB/inception_i3d/" + k + ":0"): v.numpy() for k, v in P.items()})
    results, logs = {}, {}
    for name, extra, n in (("with", {"fvd_i3d_weights": wpath, "fvd_resize_input": False}, N_SEQ), ("without", {}, N_SEQ), ("few", {"fvd_i3d_weights": wpath, "fvd_resize_input": False}, 15)):
        sub = tmp_path / name
        sub.mkdir()
        _write_videos(str(sub / "ref"), 0, n_videos=n, frames=3, H=EH, W=EW)
        _write_videos(str(sub / "gen"), 1, n_videos=n, frames=3, H=EH, W=EW, noise=40)
        cfg = {"logging": {"run_name": "fvd_eval", "comments": "", "output_root": str(sub / "results")},
               "data": {"target_input_size": [EW, EH], "actions_count": 3, "ground_truth_available": False},
               "reference_data": {"data_root": str(sub / "ref"), "crop": None}, "generated_data": {"data_root": str(sub / "gen"), "crop": None},
               "evaluation": dict({"evaluator": "playablevideogeneration_amd.dataset_evaluator",
                                   "batching": {"batch_size": 12, "observations_count": 3, "skip_frames": 0, "observation_stacking": 1, "num_workers": 0}}, **extra)}
        path = sub / "eval.yaml"
        path.write_text(yaml.safe_dump(cfg))
        config = load_evaluation_configuration(str(path))
        logger = HeadlessLogger(config, echo=False)
        (ref_ds, r), (gen_ds, g) = _sequences(config, (EW, EH))
        ev = DE.evaluator(config, logger, ref_ds, gen_ds)
        if name == "few":
            with pytest.raises(Exception, match="at least 16 sequences"):
                ev.compute_metrics()
            continue
        results[name] = ev.compute_metrics()
        logs[name] = open(os.path.join(config["logging"]["output_directory"], "log.txt")).read()
        if name == "with":
            want = _want_fvd(r, g, P)
    assert set(results["with"]) == set(results["without"]) | {"fvd"} and "fvd" not in results["without"]
    for k, v in results["without"].items():
        assert results["with"][k] == v, k                                              # every other key and value as before
    got = results["with"]["fvd"]
    print(f"dataset evaluator fvd {got!r}, restatement over the first 32 sequences {want!r}")
    assert isinstance(got, float) and want > 0 and got == pytest.approx(want, rel=1e-4)      # exact fp32 against fp64 embeddings: the trunk's 1e-6-class error, amplified by the Frechet distance's cancellation
    line = "- fvd skipped: no I3D weights configured (evaluation.fvd_i3d_weights)"
    assert logs["without"].count(line) == 1 and "fvd skipped" not in logs["with"]
    assert "- fvd is computed (I3D weights configured): the line above applies to it no longer" in logs["with"] and "fvd is computed" not in logs["without"]
    assert DE.DatasetEvaluator.NOT_COMPUTED in logs["with"] and DE.DatasetEvaluator.NOT_COMPUTED in logs["without"]
    strip = lambda text: [l for l in text.splitlines() if "fvd" not in l or l == DE.DatasetEvaluator.NOT_COMPUTED]
    assert strip(logs["with"]) == strip(logs["without"])                               # the rest of the log is unchanged


@pytest.mark.parametrize("kind", ["breakout", "bair"])
def test_action_space_evaluators_add_fvd(emu, P, tmp_path, kind):
    """dataset_evaluator_breakout / dataset_evaluator_bair through `drivers evaluate`: data.yml without the key is today's; with it `fvd` joins, over the first 32 sequences"""
    from playablevideogeneration_amd import drivers
    from tests.test_action_metrics_emu import H, W, _eval_config as action_config
    cfg, path = action_config(tmp_path, kind, videos=N_SEQ, frames=3)
    cfg["evaluation"]["batching"]["observations_count"] = 3
    cfg["evaluation"]["batching"]["batch_size"] = 12
    wpath = str(tmp_path / "i3d.pth")
    torch.save(dict(P), wpath)
    runs = {}
    for name, extra in (("plain", {}), ("fvd", {"fvd_i3d_weights": wpath, "fvd_resize_input": False})):
        cfg["logging"]["run_name"] = f"{kind}_{name}"
        c = dict(cfg, evaluation=dict(cfg["evaluation"], **extra))
        with open(path, "w") as f:
            yaml.safe_dump(c, f)
        np.random.seed(0)
        assert drivers.main(["evaluate", "--config", path]) == 0
        out_dir = os.path.join(cfg["logging"]["output_root"], f"{kind}_{name}")
        runs[name] = (yaml.safe_load(open(os.path.join(out_dir, "data.yml"))), open(os.path.join(out_dir, "log.txt")).read())
    plain, with_fvd = runs["plain"][0], runs["fvd"][0]
    same = lambda a, b: a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))
    differ = [k for k in plain if not same(with_fvd.get(k), plain[k])]
    assert set(with_fvd) == set(plain) | {"fvd"} and not differ, differ
    (_, r), (_, g) = _sequences(cfg, (W, H))
    want = _want_fvd(r, g, P)
    print(f"{kind} evaluator fvd {with_fvd['fvd']!r}, restatement over the first 32 sequences {want!r}")
    assert with_fvd["fvd"] == pytest.approx(want, rel=1e-4) and np.isfinite(want) and want >= 0
    assert "fvd skipped" in runs["plain"][1] and "fvd is computed" in runs["fvd"][1] and "fvd skipped" not in runs["fvd"][1]
