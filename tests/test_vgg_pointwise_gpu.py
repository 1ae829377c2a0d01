"""csrc/perceptual.hip and csrc/lpips.hip kernel by kernel on the MI355X: the same cases and parameters as tests/test_vgg_pointwise_emu.py, through the C-ABI of libcaddy_hip.so."""
import pytest
import torch

from tests import vgg_pointwise_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from playablevideogeneration_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lib = _lib.load()
    V.check_structs(lib)
    return lib


def test_struct_mirrors(lib):
    V.check_structs(lib)


@pytest.mark.parametrize("shape", V.POOL_SHAPES)
def test_maxpool2(lib, shape):
    V.maxpool_case(lib, DEV, shape)


@pytest.mark.parametrize("shape", V.POOL_BWD_SHAPES)
@pytest.mark.parametrize("a_s16,z_s16", V.INSTANCES2)
def test_maxpool2_bwd_relu(lib, a_s16, z_s16, shape):
    V.maxpool_bwd_case(lib, DEV, shape, a_s16, z_s16)


@pytest.mark.parametrize("rs,gs,zs", V.INSTANCES3)
def test_feat_l1(lib, rs, gs, zs):
    V.feat_l1_case(lib, DEV, rs, gs, zs)


@pytest.mark.parametrize("rs,gs", V.INSTANCES2)
def test_feat_l1_without_seed(lib, rs, gs):
    V.feat_l1_case(lib, DEV, rs, gs, None)


def test_feat_l1_second_grid_stride_trip(lib):
    V.feat_l1_case(lib, DEV, False, False, False, shape=V.L1_TWO_TRIP_SHAPE, seed=1)


@pytest.mark.parametrize("shape", V.IMG_SHAPES)
@pytest.mark.parametrize("rs,gs", V.INSTANCES2)
def test_feat_l1_img(lib, rs, gs, shape):
    V.feat_l1_img_case(lib, DEV, rs, gs, shape)


@pytest.mark.parametrize("cfg", sorted(V.COS_CONFIGS))
@pytest.mark.parametrize("rs,gs", V.INSTANCES2)
def test_feat_cos(lib, rs, gs, cfg):
    V.feat_cos_case(lib, DEV, rs, gs, cfg)


@pytest.mark.parametrize("rng", [1.0, 255.0])
@pytest.mark.parametrize("shape", V.STAGE_SHAPES)
@pytest.mark.parametrize("which", ["metric", "lpips"])
def test_stage(lib, which, shape, rng):
    V.stage_case(lib, DEV, which, shape, rng)


@pytest.mark.parametrize("Trec,t_off", V.GT_TIMES)
@pytest.mark.parametrize("ld", [4, 12])
@pytest.mark.parametrize("f", [1, 2, 4])
def test_gt_resize(lib, f, ld, Trec, t_off):
    V.gt_resize_case(lib, DEV, f, ld, Trec, t_off)


@pytest.mark.parametrize("t0,ln", V.CHUNKS)
def test_time_chunk(lib, t0, ln):
    V.time_chunk_case(lib, DEV, t0, ln)


def test_copy_f(lib):
    V.copy_f_case(lib, DEV)


@pytest.mark.parametrize("Cc,s0,s1", V.HEAD_INSTANCES)
def test_lpips_head(lib, Cc, s0, s1):
    V.lpips_head_case(lib, DEV, Cc, s0, s1)


@pytest.mark.parametrize("nf", [3, 70])
def test_lpips_finalize(lib, nf):
    V.lpips_finalize_case(lib, DEV, nf)


def test_refusals(lib):
    V.refusals_case(lib, DEV)
