"""Batched roll-out on the MI355X: n sequences per captured graph launch against the reference goldens and the oracle, sequence independence, reset / fork / replay."""
import pytest
import torch

from tests import rollout_batch_cases as R

pytestmark = pytest.mark.gpu

TENNIS_NATIVE = dict(variant="main", K=7, Da=5, Ch=128, S=4, H=96, W=256)      # the geometry of tests/test_model_gpu.py: 256 x 96 frames, state 12 x 32


@pytest.fixture(scope="module")
def lib():
    from playablevideogeneration_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


@pytest.mark.parametrize("name", ["rollout_main_s4", "rollout_reduced_s1"])
def test_slot0_of_three_meets_the_reference_goldens(lib, name):
    R.golden_case(name, lib, "cuda")


def test_slot0_of_three_meets_the_golden_unfolded(lib):
    R.golden_case("rollout_reduced_s1", lib, "cuda", fold=False)


@pytest.mark.parametrize("name", ["rollout_main_s4", "rollout_reduced_s1"])
def test_batch_of_one_equals_the_single_sequence_entry(lib, name):
    R.single_equal_case(name, lib, "cuda")


@pytest.mark.parametrize("c", [R.MAIN, R.REDUCED], ids=["main", "reduced"])
def test_five_sequences_against_their_own_oracle_runs(lib, c):
    R.oracle_case(lib, "cuda", c)


def test_two_sequences_at_the_tennis_native_geometry(lib):
    R.oracle_case(lib, "cuda", TENNIS_NATIVE, n=2, steps=4)


@pytest.mark.parametrize("c", [R.MAIN, R.REDUCED], ids=["main", "reduced"])
def test_no_coupling_between_sequences(lib, c):
    R.no_coupling_case(lib, "cuda", c)


@pytest.mark.parametrize("c", [R.MAIN, R.REDUCED], ids=["main", "reduced"])
def test_reset_fork_and_replay(lib, c):
    R.reset_and_fork_case(lib, "cuda", c)


def test_changing_n_between_rollouts(lib):
    R.change_n_case(lib, "cuda", R.MAIN)
