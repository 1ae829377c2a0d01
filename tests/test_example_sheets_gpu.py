"""Evaluation example sheets (csrc/sheets.hip; example_sheets.ExampleSheets) on the MI355X: the cases of tests/example_sheet_cases.py through libcaddy_hip.so, byte for byte
against the restated reference expressions.  (The error paths and the evaluator / driver integration are checked on the simulator only.)"""
import pytest

from playablevideogeneration_amd import metrics as M
from tests import example_sheet_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _hip_library():
    M.set_library(None)
    yield


@pytest.mark.parametrize("gi", range(len(SC.GEOMETRIES)), ids=SC.GEOMETRY_IDS)
def test_sheet_equals_the_reference_expressions_on_gpu(gi):
    SC.check_geometry("cuda", gi)


def test_full_length_reconstruction_on_gpu():
    SC.check_geometry("cuda", SC.FULL_LENGTH_GEOMETRY, full_length=True)


def test_thirty_one_sequences_draw_thirty_and_decide_on_all_on_gpu():
    SC.check_thirty_one_sequences("cuda")


def test_range_decisions_nan_negative_zero_and_saturation_on_gpu():
    SC.check_range_decisions("cuda")


def test_motion_weighted_sheet_on_gpu():
    SC.check_weighted("cuda")


def test_strip_on_gpu():
    SC.check_strip("cuda")


def test_second_call_is_bit_identical_and_a_smaller_batch_follows_a_larger_on_gpu():
    SC.check_context_reuse("cuda")
