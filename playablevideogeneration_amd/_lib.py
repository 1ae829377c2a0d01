"""ctypes binding of the C-ABI of libcaddy_hip.so (include/caddy_hip.h).

The product path has NO CPU fallback: `load()` raises if the HIP library has not been built
(`python -c "import __graft_entry__ as g; g.build()"` or `python -m playablevideogeneration_amd.csrc.build`).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libcaddy_hip.so")
CONV_MAX_SRC = 3
CONV_BK = 16


class TV(C.Structure):
    _fields_ = [("p", C.c_void_p), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("sn", C.c_long), ("ld", C.c_int), ("s16", C.c_int)]      # s16: csrc/common.h (pre-split gradient)


class ConvSrc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("sn", C.c_long), ("ld", C.c_int), ("C", C.c_int), ("Cpad", C.c_int), ("bcast", C.c_int),
                ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p), ("bn_act", C.c_int), ("bn_gn", C.c_int), ("bn_gs", C.c_long)]      # lazily applied BatchNorm of the producer (common.h)


class ConvArgs(C.Structure):
    _fields_ = [("src", ConvSrc * CONV_MAX_SRC), ("nsrc", C.c_int), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("KS", C.c_int),
                ("wp", C.c_void_p), ("Ktot", C.c_int), ("Cout", C.c_int), ("Cout_pad", C.c_int), ("bias", C.c_void_p), ("act", C.c_int),
                ("out", C.c_void_p), ("out_sn", C.c_long), ("out_ld", C.c_int), ("accumulate", C.c_int), ("precision", C.c_int), ("splitk", C.c_int), ("aux", C.c_void_p), ("split_scratch", C.c_void_p), ("split_cap", C.c_long), ("split_stride", C.c_long),
                ("mask", C.c_void_p), ("seed_ref", C.c_void_p), ("seed_w", C.c_float), ("wq", C.c_void_p), ("Kq", C.c_int), ("out_scale", C.c_float),
                ("res", C.c_void_p), ("res_sn", C.c_long), ("res_ld", C.c_int), ("xcd_map", C.c_int),
                ("pool_out", C.c_void_p), ("pool_sn", C.c_long), ("pool_ld", C.c_int), ("skip_out", C.c_int),
                ("stats", C.c_void_p), ("stats_ld", C.c_int), ("sat_flag", C.c_void_p), ("deterministic", C.c_int), ("direct_ok", C.c_int), ("lstm", C.c_void_p),
                ("in_s16", C.c_int), ("out_s16", C.c_int), ("pool_s16", C.c_int), ("mask_s16", C.c_int), ("seed_s16", C.c_int),
                ("avgpool", C.c_int), ("sat_out_next", C.c_int),      # S16 tensors (csrc/common.h): pre-split 16-bit operand pairs
                ("l1_acc", C.c_void_p),      # feature-L1 sum out of the seed epilogue (csrc/common.h)
                ("beside_chain", C.c_int)]      # the launch runs beside the model chain: co-resident tile instance (csrc/common.h)


class LstmFuse(C.Structure):      # csrc/common.h: cell update applied by the slab reduce of a roll-out gate convolution (ConvArgs.lstm)
    _fields_ = [("cprev", C.c_void_p), ("cprev_sn", C.c_long), ("cprev_ld", C.c_int), ("h", C.c_void_p), ("h_sn", C.c_long), ("h_ld", C.c_int),
                ("c", C.c_void_p), ("c_sn", C.c_long), ("c_ld", C.c_int), ("hb", C.c_void_p), ("hb_sn", C.c_long), ("hb_ld", C.c_int),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("C", C.c_int)]


class WgradArgs(C.Structure):
    _fields_ = [("src", ConvSrc * CONV_MAX_SRC), ("nsrc", C.c_int), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("KS", C.c_int),
                ("dy", C.c_void_p), ("dy_sn", C.c_long), ("dy_ld", C.c_int), ("Cout", C.c_int), ("Cout_pad", C.c_int), ("Ktot", C.c_int),
                ("dwp", C.c_void_p), ("slabs", C.c_int), ("group_n", C.c_int), ("src_gs", C.c_long * CONV_MAX_SRC), ("dy_gs", C.c_long), ("precision", C.c_int),
                ("src_bn_gs", C.c_long * CONV_MAX_SRC), ("det_slab", C.c_void_p), ("det_cap", C.c_long), ("det_stride", C.c_long), ("dy_s16", C.c_int)]


class PackDesc(C.Structure):
    _fields_ = [("w", C.c_void_p * 4), ("gw", C.c_void_p * 4), ("nw", C.c_int), ("Co_each", C.c_int), ("Cin", C.c_int), ("KS", C.c_int),
                ("nseg", C.c_int), ("seg_off", C.c_int * CONV_MAX_SRC), ("seg_C", C.c_int * CONV_MAX_SRC), ("seg_Cpad", C.c_int * CONV_MAX_SRC),
                ("Cout", C.c_int), ("Cout_pad", C.c_int), ("Ktot", C.c_int), ("oscale", C.c_void_p)]


# ---- csrc/head.h, csrc/perceptual.h: argument structs of the action head, sampling and loss kernels (caddy_k_head_* / caddy_k_loss_*) ----
AUX_LD = 16
LOSS_SLOTS = 56
LOSS_SLOT = dict(total=0, rec=1, states=2, entropy=3, dir_kl=4, mi=5, state_kl=6, hidden=7, l1_r0=8, l1_r1=9, l1_r2=10, perceptual=11, perceptual_term=12,
                 f16_saturated=13, perc_r0=16, diag_0=40)
_FP = C.c_void_p      # device pointers: always c_void_p (a bare int would be truncated to a C int when passed by value)


class HeadParams(C.Structure):
    _fields_ = [("F", C.c_int), ("Da", C.c_int), ("K", C.c_int)] + [(n, _FP) for n in ("Wm", "bm", "Wv", "bv", "Wf", "bf", "dWm", "dbm", "dWv", "dbv", "dWf", "dbf")]


class HeadBufs(C.Structure):
    _fields_ = [(n, _FP) for n in ("feat", "eps_s", "eps_d", "unif", "mu", "raw", "sdist", "ssamp", "ddist", "dirs", "logits", "logp", "prob", "ysoft", "samples", "variations", "aux",
                                   "cen_used", "selected", "d_feat", "d_logits", "d_ddist", "d_sdist", "d_aux", "g_dmu", "g_dvar", "g_mu", "g_raw")]


class SampleCfg(C.Structure):
    _fields_ = [("mode", C.c_int), ("hard", C.c_int), ("training", C.c_int), ("use_variations", C.c_int), ("tau", C.c_float), ("alpha", C.c_float),
                ("centroids", _FP), ("samples_in", _FP), ("variations_in", _FP)]


class SmallLossArgs(C.Structure):
    _fields_ = [("K", C.c_int), ("Da", C.c_int), ("NS", C.c_int), ("NT", C.c_int), ("Pbuf", _FP), ("mi_grad_scale", C.c_float),
                ("p", _FP), ("q", _FP), ("logp", _FP), ("ddist", _FP), ("sdist", _FP), ("sdist_r", _FP),
                ("d_logits", _FP), ("d_logits_r", _FP), ("d_ddist", _FP), ("d_sdist_r", _FP),
                ("ema", _FP), ("ema_alpha", C.c_float), ("update_ema", C.c_int),
                ("mi_lamb", C.c_float), ("w_mi", C.c_float), ("w_entropy", C.c_float), ("w_dirkl", C.c_float), ("w_statekl", C.c_float), ("acc", _FP)]


class DiagArgs(C.Structure):
    _fields_ = [("samples", _FP), ("ddist", _FP), ("rdist", _FP), ("variations", _FP), ("centroids", _FP), ("NS", C.c_int), ("K", C.c_int), ("Da", C.c_int), ("acc", _FP)]


class LossWeights(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("rec", "states", "entropy", "dir_kl", "mi", "state_kl", "hidden", "mi_entropy_lambda", "perceptual")]


class VggLevels(C.Structure):
    _fields_ = [("numel", (C.c_double * 5) * 3)]


class LpipsLevels(C.Structure):      # csrc/lpips.h: region of the partial slab, blocks per frame and 1 / (H_l W_l) of each level (caddy_k_lpips_finalize)
    _fields_ = [("off", C.c_long * 5), ("blocks", C.c_int * 5), ("inv_px", C.c_double * 5)]


class VggCosArgs(C.Structure):      # csrc/perceptual.h: the five tapped maps of both image batches (caddy_k_vgg_feat_cos)
    _fields_ = [("x", _FP * 5), ("y", _FP * 5), ("x_s16", C.c_int * 5), ("y_s16", C.c_int * 5), ("H", C.c_int * 5), ("W", C.c_int * 5), ("C", C.c_int * 5)]


ALLREDUCE_HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_void_p)      # allreduce_hook_t(float* device_ptr, int count, void* user)
HEAD_STRUCTS = (HeadParams, HeadBufs, SampleCfg, SmallLossArgs, DiagArgs, LossWeights, VggLevels, TV, LpipsLevels, VggCosArgs)      # index = the argument of caddy_k_struct_size


def check_head_structs(lib):
    """The ctypes mirrors above against the library's own sizeof (caddy_k_struct_size): a mirror that has drifted from csrc/head.h raises here instead of corrupting a launch."""
    for i, cls in enumerate(HEAD_STRUCTS):
        n = lib.caddy_k_struct_size(i)
        if n != C.sizeof(cls):
            raise RuntimeError(f"{cls.__name__}: ctypes mirror is {C.sizeof(cls)} bytes, the library's struct is {n}")
    assert lib.caddy_k_struct_size(len(HEAD_STRUCTS)) == -1


def round_up(a, b):
    return (a + b - 1) // b * b


_lib = None


def load(path=None):
    """Load the HIP shared library (cached).  Raises RuntimeError when it is missing -- there is no fallback."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    p = path or os.environ.get("CADDY_HIP_LIB") or LIB_PATH      # (CADDY_HIP_LIB: timing experiments with an alternative build of the same library)
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not found: the HIP extension is not built (run __graft_entry__.build()); "
                           "playablevideogeneration_amd has no CPU fallback")
    lib = C.CDLL(p)
    if path is None:
        _lib = lib
    return lib
