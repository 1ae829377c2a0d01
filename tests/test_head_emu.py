"""csrc/head.hip kernel by kernel on the host functional simulator (tests/emu), against float64 torch restatements: tests/head_cases.py."""
import pytest

from tests import head_cases as H
from tests.emu.loader import load_emu

pytestmark = pytest.mark.emu
DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    lib = load_emu()
    H.check_structs(lib)      # every ctypes mirror against the library's sizeof, once per module
    return lib


def test_struct_mirrors(lib):
    H.check_structs(lib)


@pytest.mark.parametrize("kw", H.HEAD_CASES)
def test_action_head(lib, kw):
    H.head_case(lib, DEV, **kw)


def test_head_sample_limits(lib):
    H.head_limits_case(lib, DEV)


@pytest.mark.parametrize("ema", H.SMALL_EMA)
@pytest.mark.parametrize("kw", H.SMALL_CASES)
def test_loss_small(lib, kw, ema):
    H.small_case(lib, DEV, use_ema=ema != "none", update_ema=int(ema == "ema_updated"), **kw)


@pytest.mark.parametrize("ema", ["none", "ema_updated"])
def test_loss_small_hook_and_grad_scale(lib, ema):
    """an all-reduce over two identical ranks (the hook doubles the joint matrix) with mi_grad_scale = 2: the same losses and gradients"""
    H.small_case(lib, DEV, use_ema=ema != "none", update_ema=1, hook=True, **H.SMALL_CASES[0])
    H.small_case(lib, DEV, use_ema=ema != "none", update_ema=1, hook=True, **H.SMALL_CASES[3])


def test_loss_small_adds_to_its_gradient_buffers(lib):
    H.small_case(lib, DEV, use_ema=True, update_ema=0, base=True, **H.SMALL_CASES[0])
    H.small_case(lib, DEV, base=True, **H.SMALL_CASES[3])


@pytest.mark.parametrize("f", [1, 2, 4])
@pytest.mark.parametrize("t_off", [0, 1])
@pytest.mark.parametrize("gt_out", [False, True])
def test_loss_l1(lib, f, t_off, gt_out):
    H.l1_case(lib, DEV, f=f, t_off=t_off, gt_out=gt_out, seed=f + t_off, ties=5 if f == 1 else 0)


def test_loss_l1_adds(lib):
    H.l1_case(lib, DEV, f=2, t_off=1, gt_out=True, base=True, seed=9)


def test_loss_l1_past_the_block_cap(lib):
    H.l1_case(lib, DEV, f=1, t_off=0, B=3, Tobs=3, h=256, w=256, seed=11, ties=7)      # 9 x 256 x 256 pixels > 2048 x 256: the grid-stride loop runs twice


@pytest.mark.parametrize("kw", H.MSE_CASES)
def test_loss_mse(lib, kw):
    H.mse_case(lib, DEV, **kw)


@pytest.mark.parametrize("size", H.DPF_SIZES)
@pytest.mark.parametrize("sq", [0, 1])
@pytest.mark.parametrize("a_off", [0, 1])
def test_loss_diff_per_frame(lib, size, sq, a_off):
    H.diff_per_frame_case(lib, DEV, sq=sq, a_off=a_off, seed=sq + 2 * a_off, **size)


@pytest.mark.parametrize("with_vgg,hidden", H.FINALIZE_CASES)
def test_loss_finalize(lib, with_vgg, hidden):
    H.finalize_case(lib, DEV, with_vgg=with_vgg, hidden=hidden)


def test_loss_report_flag(lib):
    H.report_flag_case(lib, DEV)


def test_head_softmax(lib):
    H.softmax_case(lib, DEV)
    H.softmax_case(lib, DEV, NS=3, K=1, seed=1)


@pytest.mark.parametrize("kw", H.DIAG_CASES)
def test_loss_diagnostics(lib, kw):
    H.diag_case(lib, DEV, **kw)
