"""LPIPS of the dataset evaluation on the host simulator build (tests/emu): the VGG16 trunk on the library's convolution kernels and the head of csrc/lpips.hip
against the plain-torch restatement of tests/lpips_cases.py, per level; invariants, the weight loader, the C ABI, the evaluators and the `evaluate` driver."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

from playablevideogeneration_amd import metrics as M
from playablevideogeneration_amd.engine import CaddyError, ParamInfo
from tests.frame_metrics_cases import seeded_pair
from tests.lpips_cases import as_package_state_dict, check_levels, lpips_restated, make_lpips_params, split_state_dicts
from tests.emu.loader import load_emu

pytestmark = pytest.mark.emu


@pytest.fixture(scope="module")
def emu():
    lib = load_emu()
    M.set_library(lib)
    yield lib
    M.set_library(None)


@pytest.fixture(scope="module")
def P():
    return make_lpips_params()


# (2, 3, 64, 64) at max_frames 4 crosses a chunk boundary; (1, 2, 96, 128) is non-square; noise 0.01 exposes cancellation between the two unit vectors
@pytest.mark.parametrize("shape,seed,noise,max_frames", [((2, 3, 64, 64), 9, 0.2, 4), ((1, 2, 96, 128), 5, 0.2, 2), ((1, 2, 64, 64), 7, 0.01, 1)])
def test_lpips_matches_restatement_per_level(emu, P, shape, seed, noise, max_frames):
    ref, gen = seeded_pair(*shape, seed=seed, noise=noise)
    ctx = M.LPIPS(shape[2], shape[3], max_frames, P, lib=emu)
    ctx.set_vgg_precision(0)
    total, levels = ctx(ref, gen, return_levels=True)
    assert total.shape == shape[:2] and levels.shape == (5,) + shape[:2] and total.dtype == torch.float64
    check_levels(total, levels, ref, gen, P, label=f"{shape} noise {noise}")


def test_lpips_invariants(emu, P):
    ref, gen = seeded_pair(1, 3, 32, 48, seed=3, noise=0.2)
    ctx = M.LPIPS(32, 48, 2, P, lib=emu)
    ctx.set_vgg_precision(0)
    total, levels = ctx(ref, ref.clone(), return_levels=True)
    assert (total == 0).all() and (levels == 0).all()                             # identical frames: exactly 0 in every level
    a, la = ctx(ref, gen, return_levels=True)
    b, lb = ctx(gen, ref, return_levels=True)
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(la.numpy(), lb.numpy(), rtol=1e-12, atol=0)
    again, lagain = ctx(ref, gen, return_levels=True)
    assert torch.equal(a, again) and torch.equal(la, lagain)                      # bit-identical: fixed-order reductions
    c, lc = ctx(ref * 255, gen * 255, 255.0, return_levels=True)                  # the staged inputs agree to fp32 rounding (2^-24 relative per pixel value)
    np.testing.assert_allclose(lc.numpy(), la.numpy(), rtol=1e-4, atol=0)
    np.testing.assert_allclose(c.numpy(), a.numpy(), rtol=1e-4, atol=0)
    assert (a > 0).all() and torch.allclose(la.sum(0), a, rtol=1e-15, atol=0)
    # the public function, its cache and the per-level terms kept on the object
    f = M.lpips(ref, gen, P, lib=emu)
    assert f.shape == (1, 3) and M._cached_lpips(ref, P, emu) is M._cached_lpips(gen, P, emu)
    np.testing.assert_allclose(f.numpy(), a.numpy(), rtol=1e-3)                   # (the simulator default is exact fp32 too; the context differs in max_frames only)
    with pytest.raises(ValueError):
        M.lpips(ref, gen, None, lib=emu)
    with pytest.raises(ValueError):
        ctx(ref[:, :, :, :16], gen[:, :, :, :16])


def test_weight_layouts_agree_and_missing_keys_raise(emu, P):
    ref, gen = seeded_pair(1, 2, 16, 32, seed=2, noise=0.2)
    trunk, lin = split_state_dicts(P)
    full = {("features." + k): v for k, v in trunk.items()} | lin | {"classifier.0.weight": torch.zeros(1)}      # a full vgg16 state dict carries more than the trunk
    layouts = {"torchvision": full, "features": trunk | lin, "package": as_package_state_dict(P), "two_files": M.lpips_state(trunk, lin)}
    results = {}
    for name, state in layouts.items():
        ctx = M.LPIPS(16, 32, 2, state, lib=emu)
        results[name] = ctx(ref, gen, return_levels=True)
    for name, (t, l) in results.items():
        assert torch.equal(t, results["torchvision"][0]) and torch.equal(l, results["torchvision"][1]), name
    renamed = {(f"lins.{k[3]}{k[4:]}" if k.startswith("lin") else k): v for k, v in P.items()}      # lins.{l}.model.1.weight
    assert set(M.lpips_state(renamed)) == set(M.lpips_state(P))
    with pytest.raises(CaddyError, match=r"lin3\.model\.1\.weight"):
        M.LPIPS(16, 32, 2, {k: v for k, v in P.items() if not k.startswith("lin3")}, lib=emu)
    with pytest.raises(CaddyError, match=r"features\.17\.bias"):
        M.lpips_state({k: v for k, v in P.items() if k != "features.17.bias"})
    bad = as_package_state_dict(P)
    bad["scaling_layer.shift"] = torch.tensor([-.03, -.088, -.2]).reshape(1, 3, 1, 1)
    with pytest.raises(CaddyError, match="scaling_layer.shift"):
        M.lpips_state(bad)
    wrong_shape = dict(P)
    wrong_shape["lin2.model.1.weight"] = torch.zeros(1, 128, 1, 1)
    with pytest.raises(CaddyError, match="lin2"):
        M.LPIPS(16, 32, 2, wrong_shape, lib=emu)
    with pytest.raises(CaddyError, match="together"):
        M.find_lpips_weights({"lpips_vgg16_weights": trunk})
    assert M.find_lpips_weights({}) is None


def test_lpips_c_abi(emu, P):
    lib = M._bind(emu)
    err = lambda: lib.caddy_last_error().decode()
    # the parameter table: 13 convolutions under torchvision's vgg16 names, then lin0 .. lin4
    assert lib.caddy_lpips_param_count() == 31
    info, names, floats = ParamInfo(), [], 0
    for i in range(31):
        assert lib.caddy_lpips_param_info_get(i, C.byref(info)) == 0
        names.append(info.name.decode())
        shape = tuple(info.shape[:info.ndim])
        assert shape == tuple(P[names[-1]].shape) and info.offset == floats
        floats = info.offset + int(np.prod(shape))
    assert names[:26] == [f"features.{i}.{leaf}" for i in M.LPIPS_CONVS for leaf in ("weight", "bias")]
    assert names[26:] == [f"lin{l}.model.1.weight" for l in range(5)]
    assert lib.caddy_lpips_param_floats() == floats and lib.caddy_lpips_param_info_get(31, C.byref(info)) != 0
    # the VGG19 table of the perceptual loss / cosine similarity is what it was
    assert lib.caddy_vgg_param_count() == 26
    vgg19 = []
    for i in range(26):
        lib.caddy_vgg_param_info_get(i, C.byref(info))
        vgg19.append(info.name.decode())
    assert vgg19 == [f"features.{i}.{leaf}" for i in (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28) for leaf in ("weight", "bias")]
    assert lib.caddy_vgg_param_floats() == sum(co * ci * 9 + co for ci, co in [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 256),
                                                                                   (256, 512), (512, 512), (512, 512), (512, 512), (512, 512)])
    # geometry
    assert lib.caddy_lpips_workspace_bytes(4, 24, 24) == 0 and "multiples of 16" in err()
    assert not lib.caddy_lpips_ctx_create(4, 24, 24, None, 0) and "multiples of 16" in err()
    assert lib.caddy_lpips_workspace_bytes(0, 32, 32) == 0 and lib.caddy_lpips_workspace_bytes(2, 16, 16) > 0
    n = lib.caddy_lpips_workspace_bytes(2, 32, 32)
    buf = torch.empty(n + 256, dtype=torch.uint8)
    base = buf.data_ptr() + (-buf.data_ptr()) % 256
    assert not lib.caddy_lpips_ctx_create(2, 32, 32, None, n) and "null" in err()
    assert not lib.caddy_lpips_ctx_create(2, 32, 32, base + 16, n) and "aligned" in err()
    assert not lib.caddy_lpips_ctx_create(2, 32, 32, base, n // 2) and "too small" in err()
    # calls: null pointers, bad counts, no weights, contexts of the wrong kind -- error codes and messages, nothing launched
    ctx = M.LPIPS(32, 32, 2, P, lib=emu)
    ref, gen = seeded_pair(1, 2, 32, 32, seed=1)
    out = torch.full((6, 1, 2), -7.0, dtype=torch.float64)
    assert lib.caddy_frame_lpips(ctx.ctx, None, gen.data_ptr(), 1, 2, 1.0, out.data_ptr()) == -2 and "null" in err()
    assert lib.caddy_frame_lpips(ctx.ctx, ref.data_ptr(), gen.data_ptr(), 1, 2, 1.0, None) == -2
    assert lib.caddy_frame_lpips(ctx.ctx, ref.data_ptr(), gen.data_ptr(), 0, 2, 1.0, out.data_ptr()) == -2
    assert lib.caddy_frame_lpips(ctx.ctx, ref.data_ptr(), gen.data_ptr(), 1, 2, 0.0, out.data_ptr()) == -2 and "positive" in err()
    assert lib.caddy_frame_lpips(None, ref.data_ptr(), gen.data_ptr(), 1, 2, 1.0, out.data_ptr()) == -2
    fm = M.FrameMetrics(32, 32, 2, lib=emu)
    assert lib.caddy_frame_lpips(fm.ctx, ref.data_ptr(), gen.data_ptr(), 1, 2, 1.0, out.data_ptr()) == -2 and "caddy_lpips_ctx_create" in err()
    assert lib.caddy_load_lpips(fm.ctx, ref.data_ptr()) == -2 and "caddy_lpips_ctx_create" in err()
    nine = torch.full((9, 1, 2), -7.0, dtype=torch.float64)
    assert lib.caddy_frame_metrics(ctx.ctx, ref.data_ptr(), gen.data_ptr(), 1, 2, 1.0, 0, nine.data_ptr()) == -2 and "caddy_metrics_ctx_create" in err()
    assert lib.caddy_load_vgg(ctx.ctx, ref.data_ptr()) == -2 and "caddy_load_lpips" in err()
    assert (out == -7).all() and (nine == -7).all()
    assert lib.caddy_debug_lpips_tap_formats(fm.ctx) == -1 and ctx.tap_formats() == 0
    raw = torch.empty(n + 256, dtype=torch.uint8)
    bare = lib.caddy_lpips_ctx_create(2, 32, 32, raw.data_ptr() + (-raw.data_ptr()) % 256, n)
    assert bare
    assert lib.caddy_frame_lpips(bare, ref.data_ptr(), gen.data_ptr(), 1, 2, 1.0, out.data_ptr()) == -2 and "caddy_load_lpips" in err()
    assert lib.caddy_load_lpips(bare, None) == -2
    lib.caddy_ctx_destroy(bare)
    assert (out == -7).all()
    assert lib.caddy_frame_lpips(ctx.ctx, ref.data_ptr(), gen.data_ptr(), 1, 2, 1.0, out.data_ptr()) == 0 and (out > 0).all()


def test_lpips_workspace_bytes(emu):
    lib = M._bind(emu)
    n = lib.caddy_lpips_workspace_bytes(30, 256, 256)
    print(f"LPIPS workspace, 30 frames of 256 x 256: {n / 2 ** 30:.2f} GiB")
    assert 2 ** 30 < n < 8 * 2 ** 30                                              # BAIR geometry, 30 frames per chunk: the order of the VGG19 context's
    assert lib.caddy_metrics_workspace_bytes(30, 256, 256, 0) < 2 * 2 ** 20      # (the plain metrics context is untouched)


# ---- the evaluators and the `evaluate` driver on two tiny on-disk datasets (32 x 32 frames: LPIPS needs multiples of 16) ----
def _lpips_eval_config(tmp_path, weights):
    from tests.test_frame_metrics_emu import _eval_config, _write_videos
    cfg = _eval_config(tmp_path)
    _write_videos(cfg["reference_data"]["data_root"] + "32", 0, H=32, W=32)
    _write_videos(cfg["generated_data"]["data_root"] + "32", 1, H=32, W=32, noise=20)
    cfg["reference_data"] = {"data_root": cfg["reference_data"]["data_root"] + "32", "crop": None}
    cfg["generated_data"] = {"data_root": cfg["generated_data"]["data_root"] + "32", "crop": [0, 0, 32, 32]}
    cfg["data"]["target_input_size"] = [32, 32]
    cfg["evaluation"]["evaluator"] = "playablevideogeneration_amd.dataset_evaluator"
    if weights is not None:
        cfg["evaluation"].update(weights)
    return cfg


def _datasets(config):
    from playablevideogeneration_amd.video_dataset import VideoDataset, evaluation_transform
    b = config["evaluation"]["batching"]
    ref_ds = VideoDataset(config["reference_data"]["data_root"], b, evaluation_transform(None, (32, 32)))
    gen_ds = VideoDataset(config["generated_data"]["data_root"], b, evaluation_transform([0, 0, 32, 32], (32, 32)))
    r = torch.stack([torch.stack([s[0] for s in ref_ds[i].observations]) for i in range(len(ref_ds))])
    g = torch.stack([torch.stack([s[0] for s in gen_ds[i].observations]) for i in range(len(gen_ds))])
    return ref_ds, gen_ds, r, g


def test_dataset_evaluator_adds_lpips_only_with_weights(emu, P, tmp_path):
    from playablevideogeneration_amd import dataset_evaluator as DE
    from playablevideogeneration_amd.drivers import HeadlessLogger, load_evaluation_configuration
    from tests.test_frame_metrics_emu import _positional_statistics
    wpath = str(tmp_path / "lpips_weights.pth")
    torch.save(as_package_state_dict(P), wpath)
    results, logs = {}, {}
    for name, weights in (("with", {"lpips_weights": wpath}), ("without", None)):
        sub = tmp_path / name
        sub.mkdir()
        path = sub / "eval.yaml"
        path.write_text(yaml.safe_dump(_lpips_eval_config(sub, weights)))
        config = load_evaluation_configuration(str(path))
        logger = HeadlessLogger(config, echo=False)
        ref_ds, gen_ds, r, g = _datasets(config)
        results[name] = DE.evaluator(config, logger, ref_ds, gen_ds).compute_metrics()
        logs[name] = open(os.path.join(config["logging"]["output_directory"], "log.txt")).read()
    assert r.shape == (6, 4, 3, 32, 32)
    want = _positional_statistics(lpips_restated(r, g, P, dtype=torch.float64)[0].numpy(), "lpips")
    assert set(want) == {"lpips/avg", "lpips/var"} | {f"lpips/{i}" for i in range(4)} | {f"lpips/{i}/var" for i in range(4)}
    assert set(results["with"]) == set(results["without"]) | set(want) and not any(k.startswith("lpips") for k in results["without"])
    for k, v in want.items():
        assert results["with"][k] == pytest.approx(v, rel=1e-4), k              # (statistics of values checked to the derived bound in the parity test)
    for k, v in results["without"].items():
        assert results["with"][k] == v, k                                          # the other metrics do not move
    assert "lpips skipped" in logs["without"] and "lpips skipped" not in logs["with"] and "lpips is computed" in logs["with"]
    assert DE.DatasetEvaluator.NOT_COMPUTED in logs["with"] and DE.DatasetEvaluator.NOT_COMPUTED in logs["without"]


def test_bair_evaluator_through_the_driver(emu, P, tmp_path):
    """dataset_evaluator_bair (ActionSpaceEvaluator, the loop the Breakout evaluator shares) through `drivers evaluate`: without weights the keys of data.yml are today's and
    the log says so; with the trunk and the lin tensors in two files lpips joins them"""
    from playablevideogeneration_amd import drivers
    from tests.test_action_metrics_emu import _eval_config as action_config, _loaded, _positional
    cfg, path = action_config(tmp_path, "bair")
    np.random.seed(0)
    assert drivers.main(["evaluate", "--config", path]) == 0
    out_dir = os.path.join(cfg["logging"]["output_root"], "bair_eval")
    plain = yaml.safe_load(open(os.path.join(out_dir, "data.yml")))
    assert not any(k.startswith("lpips") for k in plain) and "lpips skipped" in open(os.path.join(out_dir, "log.txt")).read()
    trunk, lin = split_state_dicts(P)
    torch.save(trunk, str(tmp_path / "vgg16_features.pth"))
    torch.save(lin, str(tmp_path / "lpips_lin.pth"))
    cfg["evaluation"].update({"lpips_vgg16_weights": str(tmp_path / "vgg16_features.pth"), "lpips_linear_weights": str(tmp_path / "lpips_lin.pth")})
    cfg["logging"]["run_name"] = "bair_lpips"
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    np.random.seed(0)
    assert drivers.main(["evaluate", "--config", path]) == 0
    out_dir = os.path.join(cfg["logging"]["output_root"], "bair_lpips")
    data = yaml.safe_load(open(os.path.join(out_dir, "data.yml")))
    (_, r), (_, g) = _loaded(cfg)
    want = _positional(lpips_restated(r, g, P, dtype=torch.float64)[0].numpy(), "lpips")
    assert set(data) == set(plain) | set(want)
    for k, v in want.items():
        assert data[k] == pytest.approx(v, rel=1e-4), k
    assert all(data[k] == plain[k] for k in plain if k.startswith(("mse", "psnr", "ssim")))
    log = open(os.path.join(out_dir, "log.txt")).read()
    assert "lpips skipped" not in log and "lpips is computed" in log and "lpips, fid, fvd and the density plots are not computed" in log
