"""The PNG writer (csrc/png.hip; png_writer.PngEncoder) on the MI355X: the cases of tests/png_writer_cases.py through libcaddy_hip.so.  Every file is decoded by Pillow and by
zlib, its filtered stream compared byte for byte with the numpy restatement of the filter rule, its chunk lengths, CRCs and Adler value recomputed, and its deflate blocks walked
token by token.  (The error paths, the driver integration and the sanitizer build are checked on the simulator only.)"""
import pytest

from playablevideogeneration_amd import metrics as M
from tests import png_writer_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_library():
    M.set_library(None)
    yield


@pytest.mark.parametrize("name", PC.FIXTURE_IDS)
def test_file_decodes_to_the_input_and_holds_the_restated_stream_on_gpu(name):
    PC.check_fixture("cuda", name)


def test_streams_built_for_the_coder_contain_what_they_were_built_for_on_gpu():
    PC.check_special_streams("cuda")


def test_the_fixtures_cover_every_branch_on_gpu():
    PC.assert_the_fixtures_cover_every_branch("cuda")


def test_several_images_in_one_call_on_gpu():
    PC.check_several_frames("cuda")


def test_more_images_than_the_context_holds_run_in_chunks_on_gpu():
    PC.check_chunking("cuda")


def test_second_call_is_bit_identical_and_a_flatter_batch_follows_a_noisier_on_gpu():
    PC.check_context_reuse("cuda")


def test_capacity_below_the_bound_is_refused_and_nothing_is_written_past_the_total_on_gpu():
    PC.check_capacity("cuda")


def test_fp32_frames_go_through_the_frame_writer_first_on_gpu():
    PC.check_fp32_input("cuda")


def test_unaligned_frame_bases_on_gpu():
    PC.check_unaligned_bases("cuda")


def test_noise_is_stored_and_meets_the_bound_on_gpu():
    PC.check_noise_meets_the_bound("cuda")


def test_more_blocks_than_one_pass_of_the_scan_holds_on_gpu():
    PC.check_many_blocks("cuda")


def test_files_are_not_larger_than_pillows_by_more_than_measured_on_gpu():
    PC.check_sizes("cuda")
