"""csrc/perceptual.hip and csrc/lpips.hip kernel by kernel on the host functional simulator (tests/emu), against float64 / exact restatements: tests/vgg_pointwise_cases.py.
The two-trip case of k_feat_l1 (4.2 M elements, past grid_for's cap) takes half a second here and runs on both backends."""
import os

import pytest

from tests import vgg_pointwise_cases as V
from tests.emu.loader import load_emu

pytestmark = pytest.mark.emu
DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    lib = load_emu()
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


def test_entry_points_under_address_and_undefined_sanitizers(lib):
    """host-side memory safety: csrc/perceptual.hip, csrc/lpips.hip and csrc/capi_kernels.cpp are compiled once more with -fsanitize=address,undefined together with a stand-alone
    driver (tests/emu/vgg_pointwise_sanitizer_main.cpp, its own main, exactly sized heap buffers at the odd-size, tail and cap cases) against the simulator build, and that program
    is run -- nothing sanitized is loaded into python.  (pointer-overflow is left out as in tests/test_frame_writer_emu.py: net.h's dry sizing walk offsets a null arena base.)"""
    import subprocess
    from playablevideogeneration_amd.csrc import build as B
    from tests.emu import build_emu as E
    exe = os.path.join(os.path.dirname(E.EMU_LIB), "vgg_pointwise_sanitizer")
    cxx = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fPIC", "-fsanitize=address,undefined", "-fno-sanitize=pointer-overflow", "-fno-sanitize-recover=undefined", "-Wno-psabi",
           "-Wno-unused-value", "-I", E.EMU_DIR, "-I", B.HERE, "-I", os.path.join(B.ROOT, "include"), "-x", "c++", os.path.join(B.HERE, "perceptual.hip"),
           os.path.join(B.HERE, "lpips.hip"), os.path.join(B.HERE, "capi_kernels.cpp"), os.path.join(E.EMU_DIR, "vgg_pointwise_sanitizer_main.cpp"),
           "-L", os.path.dirname(E.EMU_LIB), "-lcaddy_emu", "-Wl,-rpath," + os.path.dirname(E.EMU_LIB), "-lpthread", "-o", exe]
    subprocess.check_call(cmd)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "ok" in done.stdout, done.stdout + done.stderr
