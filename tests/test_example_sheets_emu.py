"""Evaluation example sheets (csrc/sheets.hip; example_sheets.ExampleSheets) on the host simulator build: the cases of tests/example_sheet_cases.py byte for byte against
the restated reference expressions, the errors, and the two places that use the sheets -- `Evaluator.evaluate` with evaluation.save_examples and `interpolate --sheet`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from playablevideogeneration_amd import drivers as D
from playablevideogeneration_amd import example_sheets as ES
from playablevideogeneration_amd import metrics as M
from playablevideogeneration_amd import video_dataset as VD
from playablevideogeneration_amd.engine import CaddyError
from playablevideogeneration_amd.evaluator import evaluator
from tests import example_sheet_cases as SC
from tests.emu.loader import load_emu
from tests.test_drivers_emu import _yaml_config
from tests.test_host_api_emu import _make_model

pytestmark = pytest.mark.emu


@pytest.fixture(scope="module", autouse=True)
def emu():
    lib = load_emu()
    M.set_library(lib)
    yield lib
    M.set_library(None)


@pytest.mark.parametrize("gi", range(len(SC.GEOMETRIES)), ids=SC.GEOMETRY_IDS)
def test_sheet_equals_the_reference_expressions(gi):
    SC.check_geometry("cpu", gi)


def test_full_length_reconstruction():
    SC.check_geometry("cpu", SC.FULL_LENGTH_GEOMETRY, full_length=True)


def test_thirty_one_sequences_draw_thirty_and_decide_on_all():
    SC.check_thirty_one_sequences("cpu")


def test_range_decisions_nan_negative_zero_and_saturation():
    SC.check_range_decisions("cpu")


def test_motion_weighted_sheet():
    SC.check_weighted("cpu")


def test_strip():
    SC.check_strip("cpu")


def test_second_call_is_bit_identical_and_a_smaller_batch_follows_a_larger():
    SC.check_context_reuse("cpu")


def test_colour_lookup_is_matplotlibs_call():
    """min((int)(w * 256), 255) into the `colors` table is what the reference's colormap(w) returns for float32 w in [0, 1] (upscale_and_color_weights, evaluator.py:282-291)"""
    table = ES.viridis_table()
    if table is None:      # (no matplotlib here: ExampleSheets then has no table and the evaluator leaves the weighted sheet out, which the evaluator test covers)
        assert ES.ExampleSheets(2, 2, device="cpu").lut is None
        return
    import matplotlib
    cmap = matplotlib.colormaps["viridis"] if hasattr(matplotlib, "colormaps") else matplotlib.cm.get_cmap("viridis")
    w = np.concatenate([np.random.RandomState(0).rand(1000), np.arange(257) / 256, [np.nextafter(np.float32(1), np.float32(0))]]).astype(np.float32)
    idx = np.minimum((w * np.float32(256)).astype(np.int64), 255)
    assert np.array_equal(cmap(w)[:, :3], table[idx])


def test_errors(emu):
    lib = ES._bind(emu)
    s = ES.ExampleSheets(4, 3, device="cpu", colour_table=SC.LUT)
    obs, rec = torch.rand(2, 3, 3, 16, 16), torch.rand(2, 2, 3, 16, 16)
    out = torch.empty(ES.sheet_shape(4, 3, 16, 16), dtype=torch.uint8)
    base = dict(ctx=s.ctx, obs=obs.data_ptr(), B=2, T=3, channels=3, H=16, W=16, rec=rec.data_ptr(), Trec=2, h=16, w=16, weighted=0, bias=0.0, lut=s.lut.data_ptr(), out=out.data_ptr())

    def call(**kw):
        a = dict(base, **kw)
        rc = lib.caddy_sheet_examples(a["ctx"], a["obs"], a["B"], a["T"], a["channels"], a["H"], a["W"], a["rec"], a["Trec"], a["h"], a["w"], a["weighted"], a["bias"], a["lut"], a["out"])
        return rc, lib.caddy_last_error().decode()
    assert call()[0] == 0 and call(weighted=1)[0] == 0 and call(lut=None)[0] == 0
    fm = M.FrameMetrics(16, 20, 2)
    rc, msg = call(ctx=fm.ctx)
    assert rc == -2 and "caddy_sheets_ctx_create" in msg                       # a context of another kind
    assert lib.caddy_sheet_stats_get(fm.ctx, (C.c_uint * 5)()) == -2 and lib.caddy_sheet_stats_get(s.ctx, None) == -2
    assert lib.caddy_sheet_strip(fm.ctx, rec.data_ptr(), 2, 2, 16, 16, 0, out.data_ptr()) == -2
    for name in ("obs", "rec", "out"):
        rc, msg = call(**{name: None})
        assert rc == -2 and "null" in msg, name
        rc, msg = call(**{name: base[name] + 2})
        assert rc == -2 and "aligned" in msg, name
    rc, msg = call(lut=base["lut"] + 4)
    assert rc == -2 and "aligned" in msg
    for trec in (1, 4, 0):
        rc, msg = call(Trec=trec)
        assert rc == -2 and "T or T - 1" in msg, trec
    for h, w in ((5, 5), (8, 16), (16, 8), (2, 2), (32, 32)):                  # ratios 3.2, mixed, 8 and 1 / 2
        rc, msg = call(h=h, w=w)
        assert rc == -2 and "ratios 1, 2 and 4" in msg, (h, w)
    rc, msg = call(weighted=1, h=8, w=8)
    assert rc == -2 and "full resolution" in msg
    rc, msg = call(weighted=1, lut=None)
    assert rc == -2 and "lut768" in msg
    rc, msg = call(B=3)                                                          # 6 rows on a context for 4
    assert rc == -2 and "created for 4 x 3" in msg
    rc, msg = call(T=4, Trec=3)
    assert rc == -2 and "created for 4 x 3" in msg
    assert call(channels=2)[0] == -2 and call(B=0)[0] == -2 and call(H=0, h=0)[0] == -2
    rc = lib.caddy_sheet_strip(s.ctx, rec.data_ptr(), 5, 2, 16, 16, 0, out.data_ptr())
    assert rc == -2 and "created for 4 x 3" in lib.caddy_last_error().decode()
    assert lib.caddy_sheet_strip(s.ctx, rec.data_ptr(), 2, 2, 16, 16, 2, out.data_ptr()) == -2 and "map" in lib.caddy_last_error().decode()
    assert lib.caddy_sheet_strip(s.ctx, None, 2, 2, 16, 16, 0, out.data_ptr()) == -2
    assert lib.caddy_sheets_workspace_bytes(0, 3) == 0 and not lib.caddy_sheets_ctx_create(4, 0, None, 0)
    # the Python layer
    with pytest.raises(CaddyError, match="created for 4 x 3"):
        s.examples(torch.rand(3, 3, 3, 16, 16), torch.rand(3, 2, 3, 16, 16))
    with pytest.raises(CaddyError, match="ratios"):
        s.examples(obs, torch.rand(2, 2, 3, 5, 5))
    with pytest.raises(ValueError, match="expected"):
        s.examples(obs, torch.rand(2, 2, 4, 16, 16))
    with pytest.raises(ValueError, match="expected"):
        s.strip(torch.rand(2, 2, 16, 16))
    # observations that are not contiguous in memory are copied, not misread
    wide = torch.rand(2, 3, 3, 16, 32) * (62 / 64) + 1 / 64
    view, rec2 = wide[..., ::2], torch.rand(2, 2, 3, 16, 16) * (62 / 64) + 1 / 64
    assert np.array_equal(s.examples(view, rec2), SC.expected_examples(view.contiguous(), rec2)["image"])


def test_set_library_drops_the_cached_sheets(emu):
    ES.cached_sheets(4, 3)
    assert any(k[0] == "example_sheets" for k in M._contexts)
    M.set_library(emu)
    assert not any(k[0] == "example_sheets" for k in M._contexts)


class _Spy:
    """the model, recording (observations, multiresolution reconstructions) of every forward pass"""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __call__(self, batch, *args, **kwargs):
        r = self.model(batch, *args, **kwargs)
        self.calls.append((batch[0].detach().clone(), [x.detach().clone() for x in r[1]]))
        return r

    def __getattr__(self, name):
        return getattr(self.model, name)


def _evaluate(cfg, model, datasets, step):
    lines = []

    class Log:
        def print(self, *a, **k): lines.append(" ".join(str(x) for x in a))
    spy = _Spy(model)
    torch.manual_seed(11)
    log_data = evaluator(cfg, datasets["validation"], Log(), logger_prefix="test").evaluate(spy, step)
    return log_data, spy.calls, lines


def test_evaluator_writes_the_four_sheets_of_its_first_forward_pass(tmp_path):
    cfg = D.load_configuration(_yaml_config(tmp_path))
    assert cfg["evaluation"]["save_examples"] is False                          # the default
    images = cfg["logging"]["output_images_directory"]
    datasets = VD.build_datasets(cfg)
    model = _make_model(cfg)
    off, calls_off, _ = _evaluate(cfg, model, datasets, 7)
    assert os.listdir(images) == [] and len(calls_off) == 1
    cfg["evaluation"]["save_examples"] = True
    cfg["training"]["motion_weights_bias"] = 0.1
    on, calls, lines = _evaluate(cfg, model, datasets, 7)
    assert on == off and len(calls) == 1                                        # the same numbers from the same single forward pass
    obs, recs = calls[0]
    assert len(recs) == 3 and [tuple(r.shape[-2:]) for r in recs] == [(32, 32), (16, 16), (8, 8)] and recs[0].shape[1] == obs.shape[1] - 1
    names = {f"{7:09}_observations_r{i}.png" for i in range(3)}
    for i, rec in enumerate(recs):
        got = np.asarray(Image.open(os.path.join(images, f"{7:09}_observations_r{i}.png")))
        assert np.array_equal(got, SC.expected_examples(obs, rec)["image"]), i
    if ES.viridis_table() is not None:
        names.add(f"{7:09}_motion_weighted_observations_.png")
        got = np.asarray(Image.open(os.path.join(images, f"{7:09}_motion_weighted_observations_.png")))
        want = SC.expected_examples(obs, recs[0], weighted=True, bias=0.1)
        assert not want["mask_invalid"] and np.array_equal(got, want["image"]) and not any("not written" in line for line in lines)
    else:
        assert any("matplotlib is not available" in line for line in lines)
    assert set(os.listdir(images)) == names
    # an invalid mask leaves the weighted sheet out and says why
    cfg["training"]["motion_weights_bias"] = -100.0
    _, _, lines = _evaluate(cfg, model, datasets, 8)
    assert any("not written" in line for line in lines) and not os.path.exists(os.path.join(images, f"{8:09}_motion_weighted_observations_.png"))
    assert os.path.exists(os.path.join(images, f"{8:09}_observations_r0.png"))


@pytest.mark.parametrize("batched", (False, True), ids=("sequential", "batched"))
def test_interpolate_sheet_cells_are_the_frames_it_writes(tmp_path, batched):
    cfg = D.load_configuration(_yaml_config(tmp_path))
    datasets = VD.build_datasets(cfg)
    model = _make_model(cfg)
    start = D._first_observations(datasets["validation"], 2)[1, 0]
    out = str(tmp_path / "interpolated")
    seqs = D.interpolate_loop(model, start, 0, 1, steps=2, frames_count=2, out_dir=out, batched=batched, sheet=True)
    sheet = np.asarray(Image.open(os.path.join(out, "sheet.png")))
    assert sheet.shape == ES.sheet_shape(3, 3, 32, 32)
    inside = np.zeros(sheet.shape[:2], bool)
    for si in range(3):
        for i in range(3):
            y, x = si * 34 + 2, i * 34 + 2
            frame = np.asarray(Image.open(os.path.join(out, str(si), f"{i}.png")))
            assert np.array_equal(sheet[y:y + 32, x:x + 32], frame) and np.array_equal(frame, seqs[si][i]), (si, i)
            inside[y:y + 32, x:x + 32] = True
    assert (sheet[~inside] == 255).all()
    plain = D.interpolate_loop(model, start, 0, 1, steps=2, frames_count=2, batched=batched)      # without the flag: the same frames, no sheet
    assert all(np.array_equal(a, b) for a, b in zip(plain, seqs))


def test_interpolate_subcommand_takes_the_flag(tmp_path, monkeypatch):
    monkeypatch.setattr(D, "build_model", _make_model)
    path = _yaml_config(tmp_path)
    with pytest.raises(SystemExit):      # interpolate needs a checkpoint (interpolate.py:44-70); the flag itself parses
        D.main(["interpolate", "--config", path, "--first", "1", "--second", "2", "--sheet", "--batched"])
    with pytest.raises(SystemExit):
        D.main(["interpolate", "--config", path, "--first", "1", "--second", "2", "--no-such-flag"])


def test_entry_points_under_address_and_undefined_sanitizers():
    """host-side memory safety: csrc/sheets.hip is compiled once more with -fsanitize=address,undefined together with a stand-alone driver (tests/
    example_sheets_sanitizer_main.cpp, its own main, exactly sized buffers) against the simulator build, and that program is run -- nothing sanitized is loaded into python.
    (pointer-overflow is left out: the scaffold's dry sizing walk counts bytes by offsetting a null arena base, net.h, by design.)"""
    from playablevideogeneration_amd.csrc import build as B
    from tests.emu import build_emu as E
    exe = os.path.join(os.path.dirname(E.EMU_LIB), "example_sheets_sanitizer")
    cxx = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fPIC", "-fsanitize=address,undefined", "-fno-sanitize=pointer-overflow", "-fno-sanitize-recover=undefined", "-Wno-psabi",
           "-Wno-unused-value", "-I", E.EMU_DIR, "-I", B.HERE, "-I", os.path.join(B.ROOT, "include"), "-x", "c++", os.path.join(B.HERE, "sheets.hip"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "example_sheets_sanitizer_main.cpp"), "-L", os.path.dirname(E.EMU_LIB), "-lcaddy_emu",
           "-Wl,-rpath," + os.path.dirname(E.EMU_LIB), "-lpthread", "-o", exe]
    subprocess.check_call(cmd)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "ok" in done.stdout, done.stdout + done.stderr
