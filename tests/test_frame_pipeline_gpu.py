"""Device-side frame pipeline (csrc/frames.hip, frame_pipeline.py) on the MI355X: the kernel against the host transforms bit for bit on every geometry of
tests/frame_pipeline_cases.py, RawBatch and the DevicePrefetcher against Batch on an on-disk dataset, determinism, and a context reused with another frame count.
(The out-of-range slot guard is checked on the simulator only.)"""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from playablevideogeneration_amd import batching as BT
from playablevideogeneration_amd import frame_pipeline as FP
from playablevideogeneration_amd import metrics as M
from playablevideogeneration_amd.prefetch import DevicePrefetcher
from tests import frame_pipeline_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_library():
    M.set_library(None)
    yield


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ci", range(len(FC.CASES)), ids=FC.CASE_IDS)
def test_kernel_equals_the_host_transform_on_gpu(ci, mode):
    h, w, size, crop = FC.CASES[ci]
    p = FP.FramePipeline(h, w, crop, size, 4, mode)
    out = p(torch.from_numpy(FC.case_frames(ci)).cuda(), torch.tensor(FC.SLOTS, dtype=torch.int32))
    assert out.is_cuda and out.shape == (len(FC.SLOTS), 3, size[1], size[0])
    want = FC.expected(ci, mode)
    out = out.cpu()
    for i, f in enumerate(FC.SLOTS):
        assert torch.equal(out[i], want[f]), (i, f)


def test_second_call_is_bit_identical_and_frame_count_may_change():
    ci = 8                                                   # 540 x 960 -> 256 x 96: both passes, several staging rounds
    h, w, size, crop = FC.CASES[ci]
    p = FP.FramePipeline(h, w, crop, size, 4, 0)
    frames = torch.from_numpy(FC.case_frames(ci)).cuda()
    slots = torch.tensor(FC.SLOTS, dtype=torch.int32).cuda()
    a = p(frames, slots)
    b = p(frames, slots)
    assert torch.equal(a, b)
    want = FC.expected(ci, 0)
    c = p(frames[1:].contiguous(), torch.tensor([1, 0, 1], dtype=torch.int32))      # two frames on the same context: frame k is frame k + 1 of the case
    assert torch.equal(c.cpu(), want[[2, 1, 2]])
    d = p(frames, slots)
    assert torch.equal(d, a)


@pytest.fixture(scope="module")
def dataset_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("frames_ds"))
    FC.write_dataset(root)
    return root


def _loaders(root, mode, size, crop):
    host, raw = FC.dataset_pair(root, mode, size, crop)
    bs = FC.DATASET_BATCHING["batch_size"]
    return (DataLoader(host, batch_size=bs, shuffle=False, collate_fn=BT.collate_fn_for(host[0])),
            DataLoader(raw, batch_size=bs, shuffle=False, collate_fn=BT.collate_fn_for(raw[0]), pin_memory=True))


def _same_tuple(got, want, cuda):
    assert len(got) == len(want) == 4
    for x, y in zip(got, want):
        assert x.is_cuda == cuda and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu())


@pytest.mark.parametrize("mode,size,crop", [(0, (20, 16), None), (1, (24, 12), [1, 2, 19, 15])])
def test_raw_batch_and_prefetcher_equal_batch_on_gpu(dataset_root, mode, size, crop):
    host, raw = _loaders(dataset_root, mode, size, crop)
    want = [hb.to_tuple(cuda=False) for hb in host]
    assert len(want) == 8
    for rb, w in zip(raw, want):
        assert isinstance(rb, BT.RawBatch) and rb.frames.is_pinned()
        _same_tuple(rb.to_tuple(), w, True)
        _same_tuple(rb.to_tuple(cuda=False), w, False)
    # the prefetcher keeps one batch in flight beside the one being consumed: hold on to every tuple and compare at the end
    got = list(DevicePrefetcher(raw, "cuda"))
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _same_tuple(g, w, True)
