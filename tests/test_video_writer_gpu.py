"""The MJPEG video writer (csrc/video.hip; video_writer.JpegEncoder) on the MI355X: the cases of tests/video_writer_cases.py through libcaddy_hip.so, byte for byte against
the integer restatement of libjpeg's baseline path kept there (which the CPU tests hold against Pillow's whole file, so nothing here depends on the libjpeg of this machine's
Pillow).  (The container, the error paths and the driver integration are checked on the simulator only.)"""
import pytest

from playablevideogeneration_amd import metrics as M
from tests import video_writer_cases as VC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_library():
    M.set_library(None)
    yield


@pytest.mark.parametrize("name", VC.FIXTURE_IDS)
def test_file_equals_the_oracle_on_gpu(name):
    VC.check_fixture("cuda", name)


def test_the_fixtures_cover_every_branch_of_the_entropy_coder():
    VC.assert_the_fixtures_cover_every_branch()


def test_tables_and_header_on_gpu():
    for quality in (1, 50, 100):
        VC.check_tables("cuda", quality)


def test_several_frames_in_one_call_on_gpu():
    VC.check_several_frames("cuda")


def test_more_frames_than_the_context_holds_run_in_chunks_on_gpu():
    VC.check_chunking("cuda")


def test_second_call_is_bit_identical_and_a_flatter_batch_follows_a_noisier_on_gpu():
    VC.check_context_reuse("cuda")


def test_capacity_below_the_bound_is_refused_and_nothing_is_written_past_the_total_on_gpu():
    VC.check_capacity("cuda")


def test_fp32_frames_go_through_the_frame_writer_first_on_gpu():
    VC.check_fp32_input("cuda")


def test_largest_scan_of_a_256_x_256_frame_on_gpu():
    VC.check_largest_scan("cuda")
