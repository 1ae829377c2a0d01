"""The frame writer (csrc/frames.hip: caddy_frames_write; frame_pipeline.FrameWriter) on the MI355X: the cases of tests/frame_writer_cases.py through libcaddy_hip.so,
bit for bit against the host expressions.  (The error paths are checked on the simulator only.)"""
import pytest

from playablevideogeneration_amd import metrics as M
from tests import frame_writer_cases as WC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_library():
    M.set_library(None)
    yield


@pytest.mark.parametrize("gi", range(len(WC.GEOMETRIES)), ids=WC.GEOMETRY_IDS)
def test_writer_equals_the_host_expressions_on_gpu(gi):
    WC.check_geometry("cuda", gi)


def test_level_boundaries_on_gpu():
    WC.check_boundaries("cuda")


def test_map_2_decides_on_the_device_on_gpu():
    WC.check_map2("cuda")


def test_saturation_and_counts_on_gpu():
    WC.check_saturation("cuda")


def test_second_call_is_bit_identical_and_frame_count_may_change_on_gpu():
    WC.check_context_reuse("cuda")
