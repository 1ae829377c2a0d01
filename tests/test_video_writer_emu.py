"""The MJPEG video writer (csrc/video.hip; video_writer.JpegEncoder, write_avi) on the host simulator build: the oracle of tests/video_writer_cases.py against Pillow's whole
file, the cases byte for byte against the oracle (and against Pillow itself where it carries libjpeg-turbo), the container round trip, the errors, and the drivers that use
the writer -- `play --video`, `interpolate --video`, `evaluate-model` and `build-dataset` with evaluation_dataset.save_videos."""
import ctypes as C
import io
import os
import struct
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from playablevideogeneration_amd import drivers as D
from playablevideogeneration_amd import metrics as M
from playablevideogeneration_amd import model_evaluation as ME
from playablevideogeneration_amd import video_dataset as VD
from playablevideogeneration_amd import video_writer as VW
from playablevideogeneration_amd.engine import CaddyError
from tests import model_evaluation_cases as MC
from tests import video_writer_cases as VC
from tests.emu.loader import load_emu
from tests.test_host_api_emu import _make_model

pytestmark = pytest.mark.emu
QUALITIES = (1, 30, 50, 75, 90, 95, 100)


@pytest.fixture(scope="module", autouse=True)
def emu():
    lib = load_emu()
    M.set_library(lib)
    yield lib
    M.set_library(None)


# ---- the oracle itself ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.FIXTURE_IDS)
def test_restatement_equals_pillows_whole_file(name):
    frame, q, want, _ = VC.fixture(name)
    assert want == VC.pillow(frame, q)


def test_the_fixtures_cover_every_branch_of_the_entropy_coder():
    total = VC.assert_the_fixtures_cover_every_branch()
    assert total["zero_run_escape"] >= 2 and total["dc_category_11"] >= 1 and total["ac_category_10"] >= 1


@pytest.mark.parametrize("quality", QUALITIES)
def test_quantisation_tables_and_header_equal_pillows(quality):
    tables, hdr = VC.check_tables("cpu", quality)
    frame = VC.fixture("low_q")[0]
    file = VC.pillow(frame, quality)
    assert len(hdr) == 623 and file[:623] == hdr
    with Image.open(io.BytesIO(file)) as im:      # Pillow's own reading of its tables, whatever order it reports them in
        theirs = [sorted(im.quantization[i]) for i in (0, 1)]
    assert [sorted(t) for t in tables.tolist()] == theirs


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.FIXTURE_IDS)
def test_file_equals_the_oracle(name):
    VC.check_fixture("cpu", name)


def test_several_frames_in_one_call():
    VC.check_several_frames("cpu")


def test_more_frames_than_the_context_holds_run_in_chunks():
    VC.check_chunking("cpu")


def test_second_call_is_bit_identical_and_a_flatter_batch_follows_a_noisier():
    VC.check_context_reuse("cpu")


def test_capacity_below_the_bound_is_refused_and_nothing_is_written_past_the_total():
    VC.check_capacity("cpu")


def test_fp32_frames_go_through_the_frame_writer_first():
    VC.check_fp32_input("cpu")


def test_errors(emu):
    lib = VW._bind(emu)
    enc = VW.JpegEncoder(16, 24, 2, 75, device="cpu")
    frames = torch.zeros(2, 16, 24, 3, dtype=torch.uint8)
    bound = enc.stream_bound(2)
    out, off = torch.zeros(bound, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32)

    def call(ctx=enc.ctx, f=frames.data_ptr(), n=2, o=out.data_ptr(), cap=bound, offsets=off.data_ptr()):
        return lib.caddy_video_encode(ctx, f, n, o, cap, offsets), lib.caddy_last_error().decode()
    assert call()[0] == 0
    fm = M.FrameMetrics(16, 20, 2)
    rc, msg = call(ctx=fm.ctx)
    assert rc == -2 and "caddy_video_ctx_create" in msg
    assert lib.caddy_video_tables_get(fm.ctx, None, None, None) == -2
    for name in ("f", "o", "offsets"):
        rc, msg = call(**{name: None})
        assert rc == -2 and "null" in msg, name
    rc, msg = call(offsets=off.data_ptr() + 2)
    assert rc == -2 and "aligned" in msg
    assert call(n=0)[0] == -2
    rc, msg = call(cap=bound - 1)
    assert rc == -2 and "caddy_video_stream_bound" in msg
    for args in ((0, 16, 24), (2, 0, 24), (2, 16, 4097)):
        assert lib.caddy_video_workspace_bytes(*args) == 0 and lib.caddy_video_stream_bound(*args) == 0
    for q in (0, 101):
        assert not lib.caddy_video_ctx_create(2, 16, 24, q, None, 0) and "quality" in lib.caddy_last_error().decode()
    with pytest.raises(CaddyError, match="quality"):
        VW.JpegEncoder(16, 24, 2, 0, device="cpu")
    with pytest.raises(ValueError, match="expected"):
        enc(torch.zeros(2, 16, 20, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="expected"):
        enc(torch.zeros(2, 3, 16, 24, dtype=torch.float64))
    # frames that are not contiguous in memory are copied, not misread; a frame base off a word boundary is read byte by byte
    wide = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (3, 16, 24, 6), dtype=np.uint8))
    view = wide[1:, :, :, 1:4]
    assert enc(view) == [VC.oracle(f.numpy(), 75) for f in view.contiguous()]
    odd = VW.JpegEncoder(9, 9, 2, 75, device="cpu")      # 243 bytes per frame: the second frame starts at an odd address
    two = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (2, 9, 9, 3), dtype=np.uint8))
    assert odd(two) == [VC.oracle(f.numpy(), 75) for f in two]


def test_set_library_drops_the_cached_encoder(emu):
    VW.cached_encoder(16, 16, 3)
    assert any(k[0] == "video_writer" for k in M._contexts)
    M.set_library(emu)
    assert not any(k[0] == "video_writer" for k in M._contexts)


# ---- the container -------------------------------------------------------------------------------------------------------------------------------------------------
def _check_avi(path, n, width, height, fps):
    head, frames = VW.read_avi(path)
    size = os.path.getsize(path)
    assert head["riff_size"] == size - 8 and head["frames"] == head["length"] == n == len(frames) and len(head["index"]) == n
    assert head["microsec_per_frame"] == round(1e6 / fps) and abs(head["fps"] - fps) < 1e-3
    assert (head["width"], head["height"]) == (width, height) == (head["bitmap_width"], head["bitmap_height"])
    assert head["type"] == b"vids" and head["handler"] == b"MJPG" and head["compression"] == b"MJPG" and head["bit_count"] == 24 and head["flags"] & 0x10
    data = open(path, "rb").read()
    for (ckid, flags, offset, length), at, frame in zip(head["index"], head["chunk_offsets"], frames):
        assert ckid == b"00dc" and flags == 0x10 and head["movi_offset"] + offset == at and length == len(frame)
        assert data[at:at + 4] == b"00dc" and struct.unpack_from("<I", data, at + 4)[0] == length and at % 2 == 0
        with Image.open(io.BytesIO(frame)) as im:
            assert im.size == (width, height) and im.format == "JPEG"
            im.load()
    return head, frames


def test_avi_round_trip(tmp_path):
    frames = np.stack([VC.fixture("ragged")[0], VC.fixture("ragged")[0][::-1], VC._flat(20, 28)])
    jpegs, _ = VC.encode("cpu", frames, 75)
    assert any(len(j) & 1 for j in jpegs) and any(not len(j) & 1 for j in jpegs)      # odd-length chunks are padded, even ones are not
    path = str(tmp_path / "a.avi")
    assert VW.write_avi(path, jpegs, 28, 20, 5) == os.path.getsize(path)
    _, back = _check_avi(path, 3, 28, 20, 5)
    assert back == jpegs
    VW.write_avi(path, jpegs, 28, 20, 29.97)
    head, _ = _check_avi(path, 3, 28, 20, 29.97)
    assert (head["rate"], head["scale"]) == (2997, 100)      # a fractional rate is kept as a fraction
    with pytest.raises(ValueError, match="no frames"):
        VW.write_avi(path, [], 28, 20)
    with pytest.raises(ValueError, match="positive"):
        VW.write_avi(path, jpegs, 28, 20, 0)

    class Huge(bytes):
        def __len__(self): return 1 << 30
    with pytest.raises(ValueError, match="2 GiB"):
        VW.write_avi(path, [Huge(), Huge()], 28, 20)
    # save_video: host frames are staged on the library's device
    assert VW.save_video(None, torch.from_numpy(frames), path, fps=10, quality=75) == os.path.getsize(path)
    assert _check_avi(path, 3, 28, 20, 10)[1] == jpegs


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_play_and_interpolate_write_videos_of_the_frames_their_pngs_hold(tmp_path):
    cfg = MC.fixed_length_config(tmp_path)
    datasets = VD.build_datasets(cfg)
    model = _make_model(cfg)
    start = D._first_observations(datasets["validation"], 2)[1, 0]
    out = str(tmp_path / "play")
    played = D.play_loop(model, start, [1, 3, 2], out, video=True, video_quality=80)
    _, files = _check_avi(os.path.join(out, "0", "video.avi"), 4, 32, 32, 5)
    for i, data in enumerate(files):
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "0", f"{i}.png"))), played["frames"][i]) and data == VC.oracle(played["frames"][i], 80), i
    plain = D.play_loop(model, start, [1, 3, 2], str(tmp_path / "plain"))
    assert np.array_equal(plain["frames"], played["frames"]) and not os.path.exists(str(tmp_path / "plain" / "0" / "video.avi"))
    written = {}
    for batched in (False, True):
        out = str(tmp_path / f"interpolated_{batched}")
        seqs = D.interpolate_loop(model, start, 0, 1, steps=2, frames_count=2, out_dir=out, batched=batched, video=True, fps=8)
        for si in range(3):
            _, files = _check_avi(os.path.join(out, str(si), "video.avi"), 3, 32, 32, 8)
            assert files == [VC.oracle(f, 90) for f in seqs[si]], (batched, si)
            written[batched, si] = open(os.path.join(out, str(si), "video.avi"), "rb").read()
        again = D.interpolate_loop(model, start, 0, 1, steps=2, frames_count=2, batched=batched)      # without the flag: the same frames
        assert all(np.array_equal(a, b) for a, b in zip(again, seqs))
    assert all(written[False, si] == written[True, si] for si in range(3))


def test_subcommands_take_the_flags(tmp_path, monkeypatch):
    from tests.test_drivers_emu import _yaml_config
    monkeypatch.setattr(D, "build_model", _make_model)
    path = _yaml_config(tmp_path)
    for argv in (["play", "--config", path, "--actions", "1,2", "--video", "--fps", "12.5", "--video-quality", "75"],
                 ["interpolate", "--config", path, "--first", "1", "--second", "2", "--video", "--batched", "--fps", "5", "--video-quality", "95"]):
        with pytest.raises(SystemExit) as e:      # both need a checkpoint (play.py:44-70); the flags themselves parse
            D.main(argv)
        assert e.value.code == 1
    with pytest.raises(SystemExit) as e:
        D.main(["play", "--config", path, "--actions", "1", "--video-quality", "high"])
    assert e.value.code == 2


def test_evaluate_model_and_build_dataset_save_comparison_videos(tmp_path):
    cfg = MC.fixed_length_config(tmp_path)
    logger = D.HeadlessLogger(cfg, echo=False)
    datasets = VD.build_datasets(cfg)
    model = _make_model(cfg)
    videos = os.path.join(cfg["logging"]["output_directory"], "videos")
    torch.manual_seed(3)
    off = ME.evaluate_model_loop(cfg, model, datasets, logger)
    assert not os.path.exists(videos)                                            # the default: nothing is written
    on_cfg = dict(cfg, evaluation_dataset=dict(cfg["evaluation_dataset"], save_videos=True, max_saved_videos=2))
    torch.manual_seed(3)
    on = ME.evaluate_model_loop(on_cfg, model, datasets, logger)
    assert on.keys() == off.keys() and all(MC._same(on[k], off[k]) for k in on)  # the metrics are unchanged
    assert sorted(os.listdir(videos)) == ["0.avi", "1.avi"]                       # 3 test sequences, max_saved_videos = 2
    # what the two halves must hold: the reference frames the metrics saw and the builder's bytes
    built, _ = MC.build_videos(cfg, model, datasets, True)
    rollouts = ME.ModelRollouts(cfg, model, datasets["test"], None)
    torch.manual_seed(3)
    reference = torch.cat([ref.observations for ref, _ in rollouts])
    for i in range(2):
        _, files = _check_avi(os.path.join(videos, f"{i}.avi"), MC.T, 64, 32, 5)
        left = (reference[i] * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy()
        for t in range(MC.T):
            assert files[t] == VC.oracle(np.concatenate([left[t], built[i].frames[t]], axis=1), 90), (i, t)
    # build-dataset, both quantisation paths: the default of 30 covers all three sequences; the PNGs are what they were
    for device_quantise in (False, True):
        run = dict(cfg, logging=dict(cfg["logging"], output_directory=str(tmp_path / f"built_{device_quantise}")),
                   evaluation_dataset=dict(cfg["evaluation_dataset"], save_videos=True, device_quantise=device_quantise))
        from playablevideogeneration_amd import evaluation_dataset_builder as EB
        torch.manual_seed(3)
        got = EB.builder(run, datasets["test"], logger).build(model, write=False)
        assert all(np.array_equal(a.frames, b.frames) for a, b in zip(got, built))
        assert sorted(os.listdir(os.path.join(run["logging"]["output_directory"], "videos"))) == ["0.avi", "1.avi", "2.avi"]
        for i in range(3):
            _, files = _check_avi(os.path.join(run["logging"]["output_directory"], "videos", f"{i}.avi"), MC.T, 64, 32, 5)
            with Image.open(io.BytesIO(files[1])) as im:
                right = np.asarray(im.convert("RGB"))[:, 32:].astype(int)
            assert np.abs(right - built[i].frames[1].astype(int)).mean() < 8      # the right half is the generated frame (JPEG at quality 90)


def test_entry_points_under_address_and_undefined_sanitizers():
    """host-side memory safety: csrc/video.hip is compiled once more with -fsanitize=address,undefined together with a stand-alone driver (tests/
    video_writer_sanitizer_main.cpp, its own main, exactly sized buffers) against the simulator build, and that program is run -- nothing sanitized is loaded into python.
    (pointer-overflow is left out: the scaffold's dry sizing walk counts bytes by offsetting a null arena base, net.h, by design.)"""
    from playablevideogeneration_amd.csrc import build as B
    from tests.emu import build_emu as E
    exe = os.path.join(os.path.dirname(E.EMU_LIB), "video_writer_sanitizer")
    cxx = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fPIC", "-fsanitize=address,undefined", "-fno-sanitize=pointer-overflow", "-fno-sanitize-recover=undefined", "-Wno-psabi",
           "-Wno-unused-value", "-I", E.EMU_DIR, "-I", B.HERE, "-I", os.path.join(B.ROOT, "include"), "-x", "c++", os.path.join(B.HERE, "video.hip"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "video_writer_sanitizer_main.cpp"), "-L", os.path.dirname(E.EMU_LIB), "-lcaddy_emu",
           "-Wl,-rpath," + os.path.dirname(E.EMU_LIB), "-lpthread", "-o", exe]
    subprocess.check_call(cmd)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "ok" in done.stdout, done.stdout + done.stderr
