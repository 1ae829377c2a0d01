"""Device-side frame pipeline (csrc/frames.hip, frame_pipeline.py) on the host simulator build: the restatement of PIL's 8-bit resize against PIL itself, the
kernel's tables against the restatement, the kernel against the host transforms bit for bit, RawBatch / DevicePrefetcher against Batch on an on-disk dataset, the
errors, the `train` and `evaluate` drivers with and without the device transforms, and the exported symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import yaml
from torch.utils.data import DataLoader

from playablevideogeneration_amd import batching as BT
from playablevideogeneration_amd import frame_pipeline as FP
from playablevideogeneration_amd import metrics as M
from playablevideogeneration_amd import video_dataset as VD
from playablevideogeneration_amd.engine import CaddyError
from playablevideogeneration_amd.prefetch import DevicePrefetcher
from tests import frame_pipeline_cases as FC
from tests.emu.loader import load_emu

pytestmark = pytest.mark.emu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    lib = load_emu()
    M.set_library(lib)
    yield lib
    M.set_library(None)


def _axis_sizes(case):
    h, w, size, crop = case
    in_w, in_h = (crop[2] - crop[0], crop[3] - crop[1]) if crop else (w, h)
    return (in_w, size[0]), (in_h, size[1])


@pytest.mark.parametrize("ci", range(len(FC.CASES)), ids=FC.CASE_IDS)
def test_restatement_equals_pil(ci):
    _, _, size, crop = FC.CASES[ci]
    for f in FC.case_frames(ci):
        assert np.array_equal(FC.resize(f, size, crop), FC.pil_resize(f, size, crop))


@pytest.mark.parametrize("ci", range(len(FC.CASES)), ids=FC.CASE_IDS)
def test_tables_equal_the_restatement(emu, ci):
    h, w, size, crop = FC.CASES[ci]
    p = FP.FramePipeline(h, w, crop, size, 4, 0)
    for axis, (n_in, n_out) in enumerate(_axis_sizes(FC.CASES[ci])):
        runs, ksize, bounds, kk = p.tables(axis)
        want_ksize, want_bounds, want_kk = FC.coeffs(n_in, n_out)
        assert runs == (n_in != n_out) and ksize == want_ksize
        assert np.array_equal(bounds, want_bounds) and np.array_equal(kk, want_kk)
    plan = p.plan()
    assert 1 <= plan["rows_per_block"] <= 16 and plan["lds_bytes"] <= plan["lds_variant"] and plan["lds_variant"] in (16384, 65536)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ci", range(len(FC.CASES)), ids=FC.CASE_IDS)
def test_kernel_equals_the_host_transform(emu, ci, mode):
    h, w, size, crop = FC.CASES[ci]
    p = FP.FramePipeline(h, w, crop, size, 4, mode)
    out = p(torch.from_numpy(FC.case_frames(ci)), torch.tensor(FC.SLOTS, dtype=torch.int32))
    want = FC.expected(ci, mode)
    assert out.shape == (len(FC.SLOTS), 3, size[1], size[0]) and out.dtype == torch.float32
    for i, f in enumerate(FC.SLOTS):
        assert torch.equal(out[i], want[f]), (i, f)


def test_both_kernel_variants_and_a_staging_loop_are_covered(emu):
    plans = [FP.FramePipeline(h, w, crop, size, 4, 0).plan() for h, w, size, crop in FC.CASES]
    assert {p["lds_variant"] for p in plans} == {16384, 65536}
    assert any(p["rows_per_round"] < p["max_source_rows"] for p in plans) and any(p["rows_per_block"] < 16 for p in plans)


@pytest.fixture(scope="module")
def dataset_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("frames_ds"))
    FC.write_dataset(root)
    return root


def _loaders(root, mode=0, size=(20, 16), crop=None):
    host, raw = FC.dataset_pair(root, mode, size, crop)
    assert len(host) == len(raw) == 15
    bs = FC.DATASET_BATCHING["batch_size"]
    return (DataLoader(host, batch_size=bs, shuffle=False, collate_fn=BT.collate_fn_for(host[0])),
            DataLoader(raw, batch_size=bs, shuffle=False, collate_fn=BT.collate_fn_for(raw[0])))


def _same_tuple(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu())


@pytest.mark.parametrize("mode,size,crop", [(0, (20, 16), None), (1, (24, 12), [1, 2, 19, 15])])
def test_raw_batch_equals_batch_on_a_dataset(emu, dataset_root, mode, size, crop):
    host, raw = _loaders(dataset_root, mode, size, crop)
    assert BT.collate_fn_for(next(iter(raw.dataset))) is BT.raw_batch_elements_collate_fn
    n = 0
    for hb, rb in zip(host, raw):
        assert isinstance(rb, BT.RawBatch) and rb.size == hb.size and rb.initial_frames == hb.initial_frames
        assert [v.frames_path for v in rb.video] == [v.frames_path for v in hb.video]
        assert rb.frames.dtype == torch.uint8 and rb.slot_src.shape == (rb.actions.shape[0], 3, 3) and rb.slot_src.dtype == torch.int32
        assert rb.frames.shape[0] < rb.slot_src.numel()                        # stacks share frames: each is shipped once per element
        _same_tuple(rb.to_tuple(), hb.to_tuple())
        _same_tuple(rb.to_tuple(cuda=False), hb.to_tuple(cuda=False))
        n += 1
    assert n == 8
    for got, want in zip(DevicePrefetcher(raw, "cpu"), DevicePrefetcher(host, "cpu")):
        _same_tuple(got, want)


def test_errors(emu, dataset_root, tmp_path):
    with pytest.raises(CaddyError, match="not inside"):
        FP.FramePipeline(16, 20, [0, 0, 21, 16], (20, 16), 4, 0)
    with pytest.raises(CaddyError, match="not inside"):
        FP.FramePipeline(16, 20, [5, 0, 5, 16], (20, 16), 4, 0)
    with pytest.raises(ValueError, match="mode"):
        FP.FramePipeline(16, 20, None, (20, 16), 4, 2)
    # a geometry whose single output row does not fit the LDS: no workspace size, a message that names it
    lib = FP._bind(emu)
    assert lib.caddy_frames_workspace_bytes(4, 2, 30000, None, 2, 30000) == 0
    msg = lib.caddy_last_error().decode()
    assert "LDS" in msg and "30000 x 2" in msg
    with pytest.raises(CaddyError, match="LDS"):
        FP.FramePipeline(2, 30000, None, (30000, 2), 4, 0)
    # more frames than the context was created for
    p = FP.FramePipeline(16, 20, None, (20, 16), 2, 0)
    frames = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (3, 16, 20, 3)).astype(np.uint8))
    with pytest.raises(CaddyError, match="created for 2"):
        p(frames, torch.tensor([0, 1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="slot_src names"):
        p(frames[:2], torch.tensor([0, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="uint8"):
        p(frames[:2].float(), torch.tensor([0], dtype=torch.int32))
    # the C level: a bad mode, null pointers, a context of another kind
    out = torch.empty(2, 3, 16, 20)
    slots = torch.tensor([0, 1], dtype=torch.int32)
    assert lib.caddy_frames_to_observations(p.ctx, frames.data_ptr(), 2, slots.data_ptr(), 2, 2, out.data_ptr()) == -2 and "mode" in lib.caddy_last_error().decode()
    assert lib.caddy_frames_to_observations(p.ctx, None, 2, slots.data_ptr(), 2, 0, out.data_ptr()) == -2
    fm = M.FrameMetrics(16, 20, 2)
    assert lib.caddy_frames_to_observations(fm.ctx, frames.data_ptr(), 2, slots.data_ptr(), 2, 0, out.data_ptr()) == -2
    assert "caddy_frames_ctx_create" in lib.caddy_last_error().decode()
    assert lib.caddy_frames_tables_get(fm.ctx, 0, None, None, None) == -2
    # the C level: a slot that names no frame is filled with NaN and reads nothing; its neighbours are right
    slots3 = torch.tensor([1, 7, 0, -1], dtype=torch.int32)
    out3 = torch.zeros(4, 3, 16, 20)
    assert lib.caddy_frames_to_observations(p.ctx, frames.data_ptr(), 2, slots3.data_ptr(), 4, 0, out3.data_ptr()) == 0
    assert torch.isnan(out3[1]).all() and torch.isnan(out3[3]).all()
    want = p(frames[:2], torch.tensor([1, 0], dtype=torch.int32))
    assert torch.equal(out3[0], want[0]) and torch.equal(out3[2], want[1])
    # a dataset of grey frames keeps the host path
    from playablevideogeneration_amd.evaluation_dataset_builder import EvaluationVideo
    grey = str(tmp_path / "grey")
    EvaluationVideo(np.zeros((9, 16, 20), np.uint8), [0] * 9, [0.0] * 9, [{}] * 9, [False] * 9).save(os.path.join(grey, "00000"))
    ds = VD.VideoDataset(grey, FC.DATASET_BATCHING, VD.raw_frame_spec(None, (20, 16), 0))
    with pytest.raises(Exception, match=r"00000\.png.*RGB"):
        ds[0]
    # frames of two sizes in one batch
    raw = FC.dataset_pair(dataset_root)[1]
    a, b = raw[0], raw[1]
    b.frames = [f[:, :-1] for f in b.frames]
    with pytest.raises(Exception, match=r"different sizes.*\(16, 20, 3\).*\(16, 19, 3\)"):
        BT.raw_batch_elements_collate_fn([a, b])


def test_set_library_drops_the_cached_pipeline(emu):
    p = FP.cached_pipeline(16, 20, None, (20, 16), 0, 3)
    assert FP.cached_pipeline(16, 20, None, (20, 16), 0, 5) is p and p.max_frames >= 64
    assert FP.cached_pipeline(16, 20, None, (20, 16), 1, 3) is not p
    assert FP.cached_pipeline(16, 20, None, (20, 16), 0, p.max_frames + 1) is not p      # too small: made again
    M.set_library(emu)
    assert not any(k[0] == "frames" for k in M._contexts)


def _step_lines(config):
    text = open(os.path.join(config["logging"]["output_directory"], "log.txt")).read()
    return [ln for ln in text.splitlines() if ln.startswith("step: ")]


def test_train_driver_with_and_without_device_transforms(emu, tmp_path, monkeypatch):
    from playablevideogeneration_amd import drivers as D
    from tests.test_drivers_emu import _yaml_config
    from tests.test_host_api_emu import _make_model
    monkeypatch.setattr(D, "build_model", _make_model)      # (the simulator build behind the plugin model, on the CPU)
    logs, states = [], []
    for name, on in (("off", False), ("on", True)):
        (tmp_path / name).mkdir()
        path = _yaml_config(tmp_path / name)
        cfg = yaml.safe_load(open(path))
        cfg["data"]["device_transforms"] = on
        yaml.safe_dump(cfg, open(path, "w"))
        torch.manual_seed(0)
        assert D.main(["train", "--config", path, "--max-steps", "2"]) == 0
        config = D.load_configuration(path)
        assert isinstance(VD.build_datasets(config)["train"][0], BT.RawBatchElement if on else BT.BatchElement)
        logs.append(_step_lines(config))
        states.append(torch.load(os.path.join(config["logging"]["save_root_directory"], "latest.pth.tar"), weights_only=False)["model"])
    assert len(logs[0]) >= 2 and logs[0] == logs[1]
    assert states[0].keys() == states[1].keys() and all(torch.equal(states[0][k], states[1][k]) for k in states[0])


def test_evaluate_driver_with_and_without_device_transforms(emu, tmp_path):
    from playablevideogeneration_amd import drivers as D
    from tests.test_frame_metrics_emu import _eval_config
    cfg = _eval_config(tmp_path)
    texts = []
    for name, on in (("off", False), ("on", True)):
        cfg["logging"]["run_name"] = name
        cfg["evaluation"]["device_transforms"] = on
        path = tmp_path / f"{name}.yaml"
        path.write_text(yaml.safe_dump(cfg))
        assert D.main(["evaluate", "--config", str(path)]) == 0
        texts.append(open(os.path.join(cfg["logging"]["output_root"], name, "data.yml")).read())
    assert "mse/avg" in texts[0] and texts[0] == texts[1]


def test_frames_symbols_are_exported(emu):
    hdr = open(os.path.join(ROOT, "include", "caddy_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(caddy_(?:\w+_)?frames_\w+)\s*\(", hdr))
    assert {"caddy_frames_workspace_bytes", "caddy_frames_ctx_create", "caddy_frames_tables_get", "caddy_frames_to_observations", "caddy_debug_frames_plan"} <= names
    from playablevideogeneration_amd.csrc import build as B
    libs = [emu] + ([C.CDLL(B.LIB)] if os.path.exists(B.LIB) else [])      # the simulator build, and the gfx950 library where it has been built (it loads without a GPU)
    for lib in libs:
        missing = [n for n in sorted(names) if not hasattr(lib, n)]
        assert not missing, missing
