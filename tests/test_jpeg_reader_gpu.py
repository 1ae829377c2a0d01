"""The JPEG reader (csrc/jpeg_read.hip; jpeg_reader.JpegDecoder) on the MI355X: the cases of tests/jpeg_reader_cases.py through libcaddy_hip.so -- Pillow's files and the
token writer's against the reference decoder of the cases (which the CPU tests hold to Pillow byte for byte), the video writer's output decoded without a host copy, the refusals
between good neighbours with guard bytes around the outputs, and the mutation corpus, on which the decoder's verdict and frame must equal the reference's case by case.  The
files it must refuse come after the sanitizer program of tests/test_jpeg_reader_emu.py has passed on the same source; every input here is one the decoder answers with a
status, nothing is meant to fault.  (The argument errors and the sanitizer build are checked on the simulator only.)"""
import os

import pytest

from playablevideogeneration_amd import metrics as M
from tests import jpeg_reader_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_library():
    M.set_library(None)
    yield


@pytest.fixture(scope="module", autouse=True)
def _contexts_of_the_cases():
    yield
    RC._decoders.clear()      # (destroyed here, not when the interpreter goes down)


def test_pillow_files_of_every_size_sampling_quality_and_restart_interval_on_gpu():
    RC.check_pillow_files("cuda")


def test_handwritten_streams_on_gpu():
    RC.check_handwritten("cuda")


def test_round_trip_on_the_device_for_every_writer_fixture_and_read_video_on_gpu(tmp_path):
    RC.check_round_trip("cuda", tmp_path)


def test_chunks_unaligned_starts_and_a_second_call_on_gpu():
    RC.check_chunking_and_reuse("cuda")


def test_refusals_cost_their_own_status_only_on_gpu():
    RC.check_refusals("cuda")


def test_offsets_out_of_order_or_past_the_total_on_gpu():
    RC.check_offsets_out_of_order("cuda")


def test_mutation_corpus_verdicts_and_frames_equal_the_references_on_gpu():
    RC.check_corpus("cuda")


def test_coded_jpeg_batch_from_bytes_to_observations_equals_the_host_decode_path_on_gpu(tmp_path):
    """the integration: a .jpg dataset that ships file bytes, decoded and transformed on the device -- directly and through the prefetcher's pinned staging on its own stream --
    against the same dataset decoded by Pillow in the worker"""
    import torch
    from PIL import Image
    from torch.utils.data import DataLoader
    from playablevideogeneration_amd import batching as BT
    from playablevideogeneration_amd import video_dataset as VD
    from playablevideogeneration_amd.prefetch import DevicePrefetcher
    from tests import frame_pipeline_cases as FC
    root = str(tmp_path / "ds")
    FC.write_dataset(root)
    settings = [dict(quality=90, subsampling=0), dict(quality=75, subsampling=2, restart_marker_blocks=1), dict(quality=95, subsampling=1, optimize=True)]
    for name in sorted(os.listdir(root)):
        for i in range(9):
            png = os.path.join(root, name, f"{i:05d}.png")
            Image.open(png).save(png[:-4] + ".jpg", **settings[i % 3])
            os.remove(png)
    size, crop = (24, 12), [1, 2, 19, 15]
    raw = VD.VideoDataset(root, FC.DATASET_BATCHING, VD.raw_frame_spec(crop, size, 0))
    coded = VD.VideoDataset(root, FC.DATASET_BATCHING, VD.raw_frame_spec(crop, size, 0, decode="device", codecs=("png", "jpeg")))
    loaders = [DataLoader(ds, batch_size=4, shuffle=False, collate_fn=BT.collate_fn_for(ds[0])) for ds in (raw, coded)]
    want = []
    for rb, cb in zip(*loaders):
        got = cb.pin_memory().to_tuple()
        want.append(rb.to_tuple())
        assert cb.codec == "jpeg" and got[0].is_cuda and cb.blob.numel() + 4 * cb.offsets.numel() > 0
        assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(got, want[-1]))
        assert torch.equal(cb.decode().frames.cpu(), rb.frames)
    assert len(want) == 4
    for got, ref in zip(DevicePrefetcher(loaders[1], "cuda"), want):
        assert all(torch.equal(x, y) for x, y in zip(got, ref))
