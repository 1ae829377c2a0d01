"""The PNG writer (csrc/png.hip; png_writer.PngEncoder) on the host simulator build: the restated filter rule and the deflate walker of tests/png_writer_cases.py against
zlib and Pillow themselves, every fixture's file decoded and walked, the sizes against Pillow's, the errors, the drivers that use the writer on request -- `build-dataset`
with evaluation_dataset.device_png, `play` / `interpolate` with --device-png, the evaluator's sheets with evaluation.device_png -- and a sanitizer build of the entry points."""
import io
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from playablevideogeneration_amd import drivers as D
from playablevideogeneration_amd import metrics as M
from playablevideogeneration_amd import png_writer as PW
from playablevideogeneration_amd import video_dataset as VD
from playablevideogeneration_amd.engine import CaddyError
from tests import model_evaluation_cases as MC
from tests import png_writer_cases as PC
from tests.emu.loader import load_emu
from tests.test_host_api_emu import _make_model

pytestmark = pytest.mark.emu


@pytest.fixture(scope="module", autouse=True)
def emu():
    lib = load_emu()
    M.set_library(lib)
    yield lib
    M.set_library(None)


# ---- the yardsticks themselves -------------------------------------------------------------------------------------------------------------------------------------
def test_the_walker_reads_what_zlib_writes():
    """the minimal inflate against zlib's own streams: stored (level 0), fixed (Z_FIXED), dynamic with general matches (level 9) and distance-1 matches only (Z_RLE)"""
    rng = np.random.default_rng(0)
    text = bytes(rng.integers(0, 7, 5000, dtype=np.uint8)) + bytes(300) + bytes(rng.integers(0, 256, 500, dtype=np.uint8))
    kinds = set()
    for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_RLE)):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        raw = co.compress(text) + co.flush()
        got, blocks = PC.walk_deflate(raw)
        assert got == text
        kinds |= {b["type"] for b in blocks}
        if strategy == zlib.Z_RLE:
            assert all(b["distances"] <= {1} for b in blocks) and any(258 in b["matches"] for b in blocks)
    assert kinds == {0, 1, 2}


def test_the_restated_filters_are_the_png_filters():
    """Pillow's decoder undoes the restated filter: a file put together here from the restated stream and zlib decodes to the image, for every fixed type and the adaptive rule"""
    import struct
    image = np.array(PC.fixture("odd_stride")[0])
    H, W, _ = image.shape
    for mode in range(6):
        stream, types = PC.filtered_stream(image, mode)
        assert len(stream) == H * (1 + 3 * W) and (mode == PW.FILTER_ADAPTIVE or set(types) == {mode})

        def chunk(kind, payload):
            return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))
        data = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(stream)) + chunk(b"IEND", b"")
        with Image.open(io.BytesIO(data)) as im:
            assert np.array_equal(np.asarray(im), image)


def test_fixture_rows_on_which_each_filter_wins_and_the_ties():
    PC.check_filter_choices()


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.FIXTURE_IDS)
def test_file_decodes_to_the_input_and_holds_the_restated_stream(name):
    PC.check_fixture("cpu", name)


def test_streams_built_for_the_coder_contain_what_they_were_built_for():
    PC.check_special_streams("cpu")


def test_the_fixtures_cover_every_branch():
    total = PC.assert_the_fixtures_cover_every_branch("cpu")
    assert total["stored"] >= 1 and total["fixed"] >= 1 and total["dynamic"] >= 1 and total["max_ll_15"] >= 1 and total["max_cl_7"] >= 1


def test_several_images_in_one_call():
    PC.check_several_frames("cpu")


def test_more_images_than_the_context_holds_run_in_chunks():
    PC.check_chunking("cpu")


def test_second_call_is_bit_identical_and_a_flatter_batch_follows_a_noisier():
    PC.check_context_reuse("cpu")


def test_capacity_below_the_bound_is_refused_and_nothing_is_written_past_the_total():
    PC.check_capacity("cpu")


def test_fp32_frames_go_through_the_frame_writer_first():
    PC.check_fp32_input("cpu")


def test_unaligned_frame_bases():
    PC.check_unaligned_bases("cpu")


def test_noise_is_stored_and_meets_the_bound():
    PC.check_noise_meets_the_bound("cpu")


def test_more_blocks_than_one_pass_of_the_scan_holds():
    PC.check_many_blocks("cpu")


def test_files_are_not_larger_than_pillows_by_more_than_measured():
    """the sizes are deterministic: the ratios of png_writer_cases.MEASURED_RATIO were measured here and are recorded in profiles/png_writer.md"""
    figures = PC.check_sizes("cpu")
    for name, (ours, theirs, ratio) in figures.items():
        assert ours == PC.MEASURED_BYTES[name], (name, ours, theirs)      # (this build gives the recorded bytes)


def test_errors(emu):
    lib = PW._bind(emu)
    enc = PW.PngEncoder(16, 24, 2, device="cpu")
    frames = torch.zeros(2, 16, 24, 3, dtype=torch.uint8)
    bound = enc.stream_bound(2)
    out, off = torch.zeros(bound, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32)

    def call(ctx=enc.ctx, f=frames.data_ptr(), n=2, o=out.data_ptr(), cap=bound, offsets=off.data_ptr()):
        return lib.caddy_png_encode(ctx, f, n, o, cap, offsets), lib.caddy_last_error().decode()
    assert call()[0] == 0
    fm = M.FrameMetrics(16, 20, 2)
    rc, msg = call(ctx=fm.ctx)
    assert rc == -2 and "caddy_png_ctx_create" in msg
    for name in ("f", "o", "offsets"):
        rc, msg = call(**{name: None})
        assert rc == -2 and "null" in msg, name
    rc, msg = call(offsets=off.data_ptr() + 2)
    assert rc == -2 and "aligned" in msg
    assert call(n=0)[0] == -2
    rc, msg = call(cap=bound - 1)
    assert rc == -2 and "caddy_png_stream_bound" in msg
    for args in ((0, 16, 24), (2, 0, 24), (2, 16, 0)):
        assert lib.caddy_png_workspace_bytes(*args) == 0 and lib.caddy_png_stream_bound(*args) == 0
    # a geometry whose bound for one image passes 2^31 - 1 is refused at creation; the largest that does not is sized
    assert lib.caddy_png_stream_bound(1, 26000, 27000) == 63 + 26000 * 81001 + 5 * -(-26000 * 81001 // 16384)
    for args in ((1, 27000, 27000), (1, 1, 800000000), (1, 46341, 46341)):
        assert lib.caddy_png_workspace_bytes(*args) == 0 and lib.caddy_png_stream_bound(*args) == 0
        assert not lib.caddy_png_ctx_create(*args, PW.FILTER_ADAPTIVE, None, 0) and "2^31" in lib.caddy_last_error().decode()
    for mode in (-1, 6):
        assert not lib.caddy_png_ctx_create(2, 16, 24, mode, None, 0) and "filter_mode" in lib.caddy_last_error().decode()
    with pytest.raises(CaddyError, match="filter_mode"):
        PW.PngEncoder(16, 24, 2, 9, device="cpu")
    with pytest.raises(ValueError, match="expected"):
        enc(torch.zeros(2, 16, 20, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="expected"):
        enc(torch.zeros(2, 3, 16, 24, dtype=torch.float64))
    # frames that are not contiguous in memory are copied, not misread
    wide = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (3, 16, 24, 6), dtype=np.uint8))
    view = wide[1:, :, :, 1:4]
    for data, f in zip(enc(view), view.contiguous()):
        PC.check_file(data, f.numpy())


def test_save_png_and_the_cached_encoder(emu, tmp_path):
    image = np.array(PC.fixture("odd_stride")[0])
    path = str(tmp_path / "a.png")
    assert PW.save_png(None, torch.from_numpy(image), path) == os.path.getsize(path)
    assert np.array_equal(np.asarray(Image.open(path)), image)
    assert any(k[0] == "png_writer" for k in M._contexts)
    assert PW.cached_png_encoder(33, 17, 1) is PW.cached_png_encoder(33, 17, 1)
    M.set_library(emu)
    assert not any(k[0] == "png_writer" for k in M._contexts)


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------------------------------------
class _CountCalls:
    """counts the caddy_png_* calls made through the bound library"""

    def __init__(self, monkeypatch, lib):
        self.calls = 0
        lib = PW._bind(lib)
        for name in ("caddy_png_workspace_bytes", "caddy_png_ctx_create", "caddy_png_stream_bound", "caddy_png_encode"):
            monkeypatch.setattr(lib, name, self._wrap(getattr(lib, name)), raising=False)

    def _wrap(self, fn):
        def call(*a):
            self.calls += 1
            return fn(*a)
        return call


def _tree(root):
    """{relative path: bytes} of every file under root"""
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


def _same_trees(a, b):
    """the PNGs decode to identical arrays, every other file is identical; -> how many PNGs differ in their bytes"""
    ta, tb = _tree(a), _tree(b)
    assert sorted(ta) == sorted(tb) and ta
    differ = 0
    for name in ta:
        if name.endswith(".png"):
            with Image.open(io.BytesIO(ta[name])) as x, Image.open(io.BytesIO(tb[name])) as y:
                assert x.mode == y.mode == "RGB" and np.array_equal(np.asarray(x), np.asarray(y)), name
            differ += ta[name] != tb[name]
        else:
            assert ta[name] == tb[name], name
    return differ


def test_build_dataset_with_device_png_writes_folders_that_decode_to_the_same_arrays(emu, tmp_path, monkeypatch):
    from playablevideogeneration_amd import evaluation_dataset_builder as EB
    cfg = MC.fixed_length_config(tmp_path)
    logger = D.HeadlessLogger(cfg, echo=False)
    datasets = VD.build_datasets(cfg)
    model = _make_model(cfg)
    counter = _CountCalls(monkeypatch, emu)
    roots = {}
    for name, extra in (("host", {}), ("quantised", {"device_quantise": True}), ("png", {"device_png": True})):
        roots[name] = str(tmp_path / f"built_{name}")
        run = dict(cfg, logging=dict(cfg["logging"], evaluation_dataset_directory=roots[name]), evaluation_dataset=dict(cfg["evaluation_dataset"], **extra))
        torch.manual_seed(3)
        before = counter.calls
        videos = EB.builder(run, datasets["test"], logger).build(model)
        if name == "png":
            assert counter.calls > before and all(isinstance(f, bytes) for v in videos for f in v.frames)      # only the compressed files crossed
        else:
            assert counter.calls == before                                                                   # with the flag off no caddy_png_* call is made
    assert _same_trees(roots["host"], roots["quantised"]) == 0
    assert _same_trees(roots["host"], roots["png"]) > 0                  # other bytes, the same images; the pickles identical
    # the reference's dataset reader reads the device-written folder
    batching = cfg["evaluation"]["batching"]
    a = VD.VideoDataset(roots["host"], batching, VD.final_transform(cfg))
    b = VD.VideoDataset(roots["png"], batching, VD.final_transform(cfg))
    assert len(a) == len(b) == 3
    for i in range(len(a)):
        assert all(torch.equal(x[0], y[0]) for x, y in zip(a[i].observations, b[i].observations))
    assert [v.metadata for v in a.all_videos] == [v.metadata for v in b.all_videos]
    for data in (v for k, v in _tree(roots["png"]).items() if k.endswith(".png")):
        with Image.open(io.BytesIO(data)) as im:
            PC.check_file(data, np.asarray(im))


def test_play_and_interpolate_with_device_png_write_the_frames_their_plain_runs_write(emu, tmp_path, monkeypatch):
    cfg = MC.fixed_length_config(tmp_path)
    datasets = VD.build_datasets(cfg)
    model = _make_model(cfg)
    start = D._first_observations(datasets["validation"], 2)[1, 0]
    counter = _CountCalls(monkeypatch, emu)
    plain = D.play_loop(model, start, [1, 3, 2], str(tmp_path / "play_plain"))
    quantised = D.play_loop(model, start, [1, 3, 2], str(tmp_path / "play_frames"), device_frames=True)
    assert counter.calls == 0
    played = D.play_loop(model, start, [1, 3, 2], str(tmp_path / "play_png"), device_png=True)
    assert counter.calls > 0
    assert np.array_equal(plain["frames"], played["frames"]) and np.array_equal(plain["frames"], quantised["frames"]) and plain["actions"] == played["actions"]
    for name in os.listdir(str(tmp_path / "play_plain" / "0")):
        if name.endswith(".png"):
            data = open(str(tmp_path / "play_png" / "0" / name), "rb").read()
            PC.check_file(data, np.asarray(Image.open(str(tmp_path / "play_plain" / "0" / name))))
    assert sorted(os.listdir(str(tmp_path / "play_plain" / "0"))) == sorted(os.listdir(str(tmp_path / "play_png" / "0")))
    written = {}
    for batched in (False, True):
        base = counter.calls
        off = str(tmp_path / f"interpolated_plain_{batched}")
        want = D.interpolate_loop(model, start, 0, 1, steps=2, frames_count=2, out_dir=off, batched=batched, sheet=True)
        assert counter.calls == base
        on = str(tmp_path / f"interpolated_png_{batched}")
        calls = []
        real = PW.PngEncoder.__call__
        monkeypatch.setattr(PW.PngEncoder, "__call__", lambda self, frames, **kw: (calls.append(int(frames.shape[0])), real(self, frames, **kw))[1])
        got = D.interpolate_loop(model, start, 0, 1, steps=2, frames_count=2, out_dir=on, batched=batched, sheet=True, device_png=True)
        monkeypatch.setattr(PW.PngEncoder, "__call__", real)
        assert all(np.array_equal(a, b) for a, b in zip(want, got))
        assert calls == ([3, 3, 3, 1] if batched else [1] * 9 + [1])      # batched: all values of a step in one encoder call; then the sheet
        assert _same_trees(off, on) > 0
        data = open(os.path.join(on, "sheet.png"), "rb").read()
        PC.check_file(data, np.asarray(Image.open(os.path.join(off, "sheet.png"))))
        written[batched] = _tree(on)
    assert written[False] == written[True]      # the same files either way


def test_subcommands_take_the_flag(tmp_path, monkeypatch):
    from tests.test_drivers_emu import _yaml_config
    monkeypatch.setattr(D, "build_model", _make_model)
    path = _yaml_config(tmp_path)
    for argv in (["play", "--config", path, "--actions", "1,2", "--device-png"],
                 ["interpolate", "--config", path, "--first", "1", "--second", "2", "--device-png", "--batched", "--sheet"]):
        with pytest.raises(SystemExit) as e:      # both need a checkpoint (play.py:44-70); the flags themselves parse
            D.main(argv)
        assert e.value.code == 1


def test_evaluator_sheets_with_device_png_decode_to_the_sheets_of_the_plain_run(emu, tmp_path, monkeypatch):
    from tests.test_drivers_emu import _yaml_config
    from tests.test_example_sheets_emu import _evaluate
    cfg = D.load_configuration(_yaml_config(tmp_path))
    datasets = VD.build_datasets(cfg)
    model = _make_model(cfg)
    counter = _CountCalls(monkeypatch, emu)
    images = cfg["logging"]["output_images_directory"]
    cfg["evaluation"]["save_examples"] = True
    plain, _, _ = _evaluate(cfg, model, datasets, 7)
    assert counter.calls == 0
    want = _tree(images)
    assert len(want) >= 3
    for name in want:
        os.remove(os.path.join(images, name))
    cfg["evaluation"]["device_png"] = True
    on, _, _ = _evaluate(cfg, model, datasets, 7)
    assert on == plain and counter.calls > 0
    got = _tree(images)
    assert sorted(got) == sorted(want)
    for name in want:
        with Image.open(io.BytesIO(want[name])) as im:
            PC.check_file(got[name], np.asarray(im))


def test_entry_points_under_address_and_undefined_sanitizers():
    """host-side memory safety: csrc/png.hip is compiled once more with -fsanitize=address,undefined together with a stand-alone driver (tests/png_writer_sanitizer_main.cpp,
    its own main, exactly sized buffers) against the simulator build, and that program is run -- nothing sanitized is loaded into python.  (pointer-overflow is left out: the
    scaffold's dry sizing walk counts bytes by offsetting a null arena base, net.h, by design.)"""
    from playablevideogeneration_amd.csrc import build as B
    from tests.emu import build_emu as E
    exe = os.path.join(os.path.dirname(E.EMU_LIB), "png_writer_sanitizer")
    cxx = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fPIC", "-fsanitize=address,undefined", "-fno-sanitize=pointer-overflow", "-fno-sanitize-recover=undefined", "-Wno-psabi",
           "-Wno-unused-value", "-I", E.EMU_DIR, "-I", B.HERE, "-I", os.path.join(B.ROOT, "include"), "-x", "c++", os.path.join(B.HERE, "png.hip"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "png_writer_sanitizer_main.cpp"), "-L", os.path.dirname(E.EMU_LIB), "-lcaddy_emu",
           "-Wl,-rpath," + os.path.dirname(E.EMU_LIB), "-lpthread", "-o", exe]
    subprocess.check_call(cmd)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "ok" in done.stdout, done.stdout + done.stderr
