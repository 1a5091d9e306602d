"""ctypes binding of libevc_hip.so (the C ABI declared in include/evc.h).

The product path has no CPU fallback: if the library is missing or cannot be loaded,
`lib()` raises and every solver entry point fails with it.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# EVC_LIB overrides the library path (A/B builds during kernel tuning)
LIB_PATH = os.environ.get("EVC_LIB") or os.path.join(_HERE, "libevc_hip.so")

F64, F32 = 0, 1
FRAME_MAJOR, BIN_MAJOR = 0, 1
EPS_ADD, EPS_ZERO_REPLACE, EPS_NONE, EPS_CLAMP = 0, 1, 2, 3
ALGO_GRAM, ALGO_FACTORED, ALGO_LITERAL, ALGO_AUTO = 0, 1, 2, 3
INIT_GIVEN, INIT_SKLEARN, INIT_CONST = 0, 1, 2
STOP_NONE, STOP_SKLEARN, STOP_PYMF, STOP_DECOMP = 0, 1, 2, 3
PROX_POSITIVE, PROX_SIGNED = 0, 1
PROX_ISTA, PROX_FISTA, PROX_NESTEROV = 0, 1, 2
PROX_LIP_MEAN, PROX_LIP_MAX = 0, 1
LOSS_FROBENIUS, LOSS_KL = 0, 1
FLAG_NO_FUSED, FLAG_EXACT_DIV, FLAG_NO_EXCHANGE, FLAG_NO_ALL_RESIDENT, FLAG_PAIR_TILES, FLAG_NO_LONE_BIN = 1, 2, 4, 16, 32, 64
FLAG_NO_RANGE_HOIST = 128
FLAG_NO_QUAD_ROWS = 1 << 20
LEARN_SKLEARN, LEARN_PYMF = 0, 1
CDL_BOTH, CDL_DICT_ONLY = 0, 1
DCL_BOTH, DCL_DICT_ONLY = 0, 1
CONVEX_BOTH, CONVEX_H_ONLY, CONVEX_G_ONLY = 0, 1, 2
KM_BOTH, KM_ASSIGN_ONLY = 0, 1
KM_STOP_NONE, KM_STOP_PYMF, KM_STOP_LABELS = 0, 1, 2

# every symbol include/evc.h declares; tests check that the library exports all of them
SYMBOLS = ("evc_version", "evc_strerror", "evc_device_count", "evc_workspace_bytes",
           "evc_nmf_solve", "evc_nmf_convert", "evc_synthesize", "evc_residual",
           "evc_griffin_lim_workspace_bytes", "evc_griffin_lim", "evc_griffin_lim_batch_workspace_bytes",
           "evc_griffin_lim_batch", "evc_dtw_workspace_bytes", "evc_dtw_align",
           "evc_stft_frames", "evc_stft_workspace_bytes", "evc_stft", "evc_dict_bytes", "evc_dict_prepare",
           "evc_dtw_path_rows", "evc_dtw_gather_rows", "evc_cd_workspace_bytes", "evc_cd_solve",
           "evc_learn_workspace_bytes", "evc_learn_splits", "evc_nmf_learn",
           "evc_cd_learn_workspace_bytes", "evc_cd_learn_splits", "evc_cd_learn",
           "evc_mfcc_workspace_bytes", "evc_mfcc", "evc_beta_workspace_bytes", "evc_beta_solve",
           "evc_beta_learn_workspace_bytes", "evc_beta_learn_splits", "evc_beta_learn_route", "evc_beta_learn",
           "evc_online_workspace_bytes", "evc_online_splits", "evc_online_learn",
           "evc_online_transform_workspace_bytes", "evc_online_transform",
           "evc_online_fresh_workspace_bytes", "evc_online_learn_fresh",
           "evc_deconv_workspace_bytes", "evc_deconv_solve", "evc_deconv_synthesize",
           "evc_deconv_learn_workspace_bytes", "evc_deconv_learn_splits", "evc_deconv_learn",
           "evc_semi_workspace_bytes", "evc_semi_solve",
           "evc_convex_workspace_bytes", "evc_convex_splits", "evc_convex_learn",
           "evc_prox_workspace_bytes", "evc_prox_solve",
           "evc_prox_masked_workspace_bytes", "evc_prox_masked_solve",
           "evc_prox_learn_workspace_bytes", "evc_prox_learn_block", "evc_prox_learn",
           "evc_prox_masked_learn_workspace_bytes", "evc_prox_masked_learn",
           "evc_mu_masked_workspace_bytes", "evc_mu_masked_solve",
           "evc_mu_masked_learn_workspace_bytes", "evc_mu_masked_learn_splits", "evc_mu_masked_learn",
           "evc_mu_stoch_learn_workspace_bytes", "evc_mu_stoch_learn_route", "evc_mu_stoch_learn_splits", "evc_mu_stoch_learn",
           "evc_kmeans_workspace_bytes", "evc_kmeans_splits", "evc_kmeans")
BETA_MAX_M = 528
MU_MASKED_MAX_M, MU_MASKED_MAX_SLOTS = 528, 4097
MU_MASKED_LEARN_MAX_R = 4096
STOCH_ASG, STOCH_ASAG, STOCH_GSAG, STOCH_SVRMU = 0, 1, 2, 3
MU_STOCH_MAX_R, MU_STOCH_FUSED_MAX_R = 4096, 256
DECONV_MAX_M, DECONV_MAX_TAPS, DECONV_MAX_MB = 256, 16, 1056
DECONV_LEARN_MAX_R = 4096
SEMI_MAX_M, SEMI_MAX_N = 1056, 16384
CONVEX_MAX_M, CONVEX_MAX_T, CONVEX_MAX_R, CONVEX_MAX_S = 1056, 16384, 1024, 16
KMEANS_MAX_M, KMEANS_MAX_T, KMEANS_MAX_R, KMEANS_MAX_S = 1056, 1 << 20, 4096, 16
PROX_MAX_M, PROX_MAX_N, PROX_MAX_SLOTS = 1056, 16384, 4097
PROX_LEARN_MAX_M, PROX_LEARN_MAX_N = 1056, 4096
PROX_MASKED_LEARN_MAX_M, PROX_MASKED_LEARN_MAX_N, PROX_MASKED_LEARN_MAX_S = 1056, 1024, 1 << 28
MFCC_MAX_MELS, MFCC_MAX_FFT = 256, 8192


class SolveOpts(C.Structure):
    """Mirror of `evc_solve_opts` (include/evc.h)."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("algo", C.c_int),
        ("iters", C.c_int), ("eps_mode", C.c_int), ("init_mode", C.c_int),
        ("check_every", C.c_int), ("stop_rule", C.c_int), ("reserved", C.c_int),
        ("loss", C.c_int), ("test_abort_at", C.c_int),
        ("eps", C.c_double), ("l1", C.c_double), ("tol", C.c_double), ("init_value", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p), ("info", C.c_void_p), ("dict", C.c_void_p),
    ]


class CdOpts(C.Structure):
    """Mirror of `evc_cd_opts` (include/evc.h): options of the coordinate-descent solve."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("init_mode", C.c_int),
        ("max_iter", C.c_int), ("reserved", C.c_int),
        ("tol", C.c_double), ("l1", C.c_double), ("l2", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class LearnOpts(C.Structure):
    """Mirror of `evc_learn_opts` (include/evc.h): options of the solve that also learns the dictionary."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("surface", C.c_int),
        ("iters", C.c_int), ("check_every", C.c_int), ("reserved", C.c_int), ("loss", C.c_int),
        ("tol", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class CdLearnOpts(C.Structure):
    """Mirror of `evc_cd_learn_opts` (include/evc.h): options of the coordinate descent that also learns the dictionary."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("max_iter", C.c_int),
        ("update", C.c_int), ("reserved", C.c_int),
        ("tol", C.c_double), ("l1_h", C.c_double), ("l2_h", C.c_double), ("l1_w", C.c_double), ("l2_w", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class MfccOpts(C.Structure):
    """Mirror of `evc_mfcc_opts` (include/evc.h): options of the MFCC alignment features."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("sr", C.c_int), ("fft_size", C.c_int), ("hop", C.c_int),
        ("n_mels", C.c_int), ("n_mfcc", C.c_int), ("center", C.c_int), ("reserved", C.c_int),
        ("fmin", C.c_double), ("fmax", C.c_double), ("amin", C.c_double), ("top_db", C.c_double),
    ]


class BetaOpts(C.Structure):
    """Mirror of `evc_beta_opts` (include/evc.h): options of the beta-divergence activation solve."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("iters", C.c_int),
        ("init_mode", C.c_int), ("check_every", C.c_int), ("stop_rule", C.c_int), ("reserved", C.c_int),
        ("beta", C.c_double), ("tol", C.c_double), ("l1", C.c_double), ("l2", C.c_double), ("init_value", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class BetaLearnOpts(C.Structure):
    """Mirror of `evc_beta_learn_opts` (include/evc.h): options of the beta-divergence solve that also learns the dictionary."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("iters", C.c_int),
        ("check_every", C.c_int), ("reserved", C.c_int),
        ("beta", C.c_double), ("tol", C.c_double),
        ("l1_h", C.c_double), ("l2_h", C.c_double), ("l1_w", C.c_double), ("l2_w", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class OnlineOpts(C.Structure):
    """Mirror of `evc_online_opts` (include/evc.h): options of the mini-batch dictionary learning."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("batch_size", C.c_int),
        ("max_iter", C.c_int), ("max_no_improvement", C.c_int), ("resume", C.c_int), ("reserved", C.c_int),
        ("beta", C.c_double), ("tol", C.c_double), ("forget_factor", C.c_double),
        ("l1_h", C.c_double), ("l2_h", C.c_double), ("l1_w", C.c_double), ("l2_w", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class OnlineFreshOpts(C.Structure):
    """Mirror of `evc_online_fresh_opts` (include/evc.h): the mini-batch learning with fresh restarts."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("batch_size", C.c_int),
        ("max_iter", C.c_int), ("max_no_improvement", C.c_int), ("resume", C.c_int), ("reserved", C.c_int),
        ("fresh_max_iter", C.c_int), ("final_max_iter", C.c_int),
        ("beta", C.c_double), ("tol", C.c_double), ("forget_factor", C.c_double),
        ("l1_h", C.c_double), ("l2_h", C.c_double), ("l1_w", C.c_double), ("l2_w", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class TransformOpts(C.Structure):
    """Mirror of `evc_transform_opts` (include/evc.h): options of the mini-batch estimator's activation solve."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("max_iter", C.c_int),
        ("init_mode", C.c_int), ("reserved", C.c_int),
        ("beta", C.c_double), ("tol", C.c_double), ("l1", C.c_double), ("l2", C.c_double), ("init_value", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class DeconvOpts(C.Structure):
    """Mirror of `evc_deconv_opts` (include/evc.h): options of the activation solve with multi-frame exemplars."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("loss", C.c_int), ("taps", C.c_int),
        ("iters", C.c_int), ("init_mode", C.c_int), ("check_every", C.c_int), ("stop_rule", C.c_int), ("reserved", C.c_int),
        ("tol", C.c_double), ("l1", C.c_double), ("l2", C.c_double), ("init_value", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class DeconvLearnOpts(C.Structure):
    """Mirror of `evc_deconv_learn_opts` (include/evc.h): options of the convolutive dictionary learning."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("loss", C.c_int), ("taps", C.c_int),
        ("iters", C.c_int), ("check_every", C.c_int), ("update", C.c_int), ("reserved", C.c_int),
        ("tol", C.c_double), ("l1_h", C.c_double), ("l2_h", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class SemiOpts(C.Structure):
    """Mirror of `evc_semi_opts` (include/evc.h): options of the semi-NMF activation solve."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("iters", C.c_int),
        ("init_mode", C.c_int), ("check_every", C.c_int), ("stop_rule", C.c_int), ("reserved", C.c_int),
        ("eps", C.c_double), ("tol", C.c_double), ("init_value", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class ConvexOpts(C.Structure):
    """Mirror of `evc_convex_opts` (include/evc.h): options of the convex-NMF learner."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("iters", C.c_int),
        ("check_every", C.c_int), ("update", C.c_int), ("reserved", C.c_int),
        ("tol", C.c_double), ("eps", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class KmeansOpts(C.Structure):
    """Mirror of `evc_kmeans_opts` (include/evc.h): options of the device k-means."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("iters", C.c_int),
        ("update", C.c_int), ("stop_rule", C.c_int), ("reserved", C.c_int),
        ("tol", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class ProxOpts(C.Structure):
    """Mirror of `evc_prox_opts` (include/evc.h): options of the proximal-gradient activation solve."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("iters", C.c_int),
        ("mode", C.c_int), ("momentum", C.c_int), ("normalize", C.c_int), ("check_every", C.c_int),
        ("stop_rule", C.c_int), ("init_mode", C.c_int), ("reserved", C.c_int), ("reserved2", C.c_int),
        ("alpha", C.c_double), ("tol", C.c_double), ("init_value", C.c_double), ("lipschitz", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class ProxMaskedOpts(C.Structure):
    """Mirror of `evc_prox_masked_opts` (include/evc.h): `evc_prox_opts` plus the weights of the Gershgorin bound."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("iters", C.c_int),
        ("mode", C.c_int), ("momentum", C.c_int), ("normalize", C.c_int), ("check_every", C.c_int),
        ("stop_rule", C.c_int), ("init_mode", C.c_int), ("reserved", C.c_int), ("reserved2", C.c_int),
        ("lip_weights", C.c_int), ("reserved3", C.c_int),
        ("alpha", C.c_double), ("tol", C.c_double), ("init_value", C.c_double), ("lipschitz", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class ProxLearnOpts(C.Structure):
    """Mirror of `evc_prox_learn_opts` (include/evc.h): options of the sparse dictionary learning."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("batch_size", C.c_int),
        ("epochs", C.c_int), ("lasso_iters", C.c_int), ("lasso_check_every", C.c_int), ("mode", C.c_int),
        ("momentum", C.c_int), ("resume", C.c_int), ("reserved", C.c_int), ("reserved2", C.c_int),
        ("alpha", C.c_double), ("tol", C.c_double), ("lasso_tol", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class ProxMaskedLearnOpts(C.Structure):
    """Mirror of `evc_prox_masked_learn_opts` (include/evc.h): `evc_prox_learn_opts`' fields for the learning with a mask."""
    _fields_ = list(ProxLearnOpts._fields_)


class MuMaskedOpts(C.Structure):
    """Mirror of `evc_mu_masked_opts` (include/evc.h): options of the multiplicative-update solve with missing data."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("loss", C.c_int), ("iters", C.c_int),
        ("init_mode", C.c_int), ("check_every", C.c_int), ("stop_rule", C.c_int), ("reserved", C.c_int), ("reserved2", C.c_int),
        ("tol", C.c_double), ("init_value", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class MuMaskedLearnOpts(C.Structure):
    """Mirror of `evc_mu_masked_learn_opts` (include/evc.h): options of the multiplicative-update learning with missing data."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("loss", C.c_int), ("iters", C.c_int),
        ("check_every", C.c_int), ("reserved", C.c_int), ("reserved2", C.c_int),
        ("tol", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class MuStochOpts(C.Structure):
    """Mirror of `evc_mu_stoch_opts` (include/evc.h): options of the mini-batch multiplicative-update learning."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("dtype", C.c_int), ("layout", C.c_int), ("loss", C.c_int), ("method", C.c_int),
        ("batch_size", C.c_int), ("epochs", C.c_int), ("inner_iters", C.c_int), ("order_rows", C.c_int), ("route", C.c_int),
        ("reserved", C.c_int), ("reserved2", C.c_int),
        ("forget_rate", C.c_double), ("alpha", C.c_double), ("tol", C.c_double),
        ("ev_loop_start", C.c_void_p), ("ev_loop_stop", C.c_void_p),
    ]


class Dict(C.Structure):
    """Mirror of `evc_dict` (include/evc.h): a dictionary imported once (evc_dict_prepare)."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("magic", C.c_int), ("M", C.c_int), ("Mb", C.c_int), ("N", C.c_int),
        ("dtype", C.c_int), ("loss", C.c_int), ("reserved", C.c_int),
        ("eps", C.c_double), ("mem", C.c_void_p), ("bytes", C.c_size_t),
    ]


class SolveInfo(C.Structure):
    """Mirror of `evc_solve_info` (include/evc.h): what the library actually ran."""
    _fields_ = [
        ("struct_bytes", C.c_int), ("kernel", C.c_int), ("members", C.c_int), ("launches", C.c_int),
        ("redo", C.c_int), ("exchange", C.c_int), ("prepared", C.c_int), ("variant", C.c_int),
    ]


# block codes of evc_solve_info.variant for k_gemm_nt / k_gemm2 (include/evc.h): frames x rows, None: no such product
GEMM_BLOCKS = {0: None, 1: (64, 64), 2: (64, 128), 3: (128, 64), 4: (128, 128), 5: (128, 128)}


def decode_variant(kernel: int, v: int):
    """evc_solve_info.variant as a dict (None for the kernels that report none): schedule and template instance of the
    task-queue kernels.  k_gemm_nt / k_gemm2: the block (frames, rows) of the update contraction, of V = H Am^T with its
    k-split count and of the numerator P (None where a solve forms none), and whether a block is k_gemm2's deep-slab
    shape (diagnostic builds).  k_fused_wide: k_fused_wide<mt, w, tagged>; k_fused_wide64: k_fused_wide64<tpw>.  k_fused_all:
    set when its last launch formed Y itself (evc_nmf_convert), with whether that launch still stored the packed
    activations; None for every other solve on that kernel."""
    if kernel == 5 and v:      # k_fused_all: what the end of a frame tile did in the last launch
        return {"y_in_kernel": bool(v & 1), "packed_h_stored": bool(v & 2)}
    if kernel in (1, 2) and v:      # the contraction kernels: block (frames, rows) of each product, k-splits of V = H Am^T
        blk = lambda c: GEMM_BLOCKS[c & 15]
        return {"update": blk(v), "v": blk(v >> 4), "v_splits": (v >> 8) & 63, "p": blk(v >> 16),
                "deep": any(((v >> b) & 15) == 5 for b in (0, 4, 16))}
    if kernel not in (6, 7):
        return None
    d = {"static": bool(v & 1), "reduce": bool(v & 2), "tagged": bool(v & 4)}
    d.update({"w": (v >> 8) & 0xff, "mt": (v >> 16) & 0xff} if kernel == 6 else {"tpw": (v >> 8) & 0xff,
                                                                                  "tiles": (v >> 16) & 0xff})
    return d


KERNEL_NAMES = {0: "none", 1: "k_gemm_nt", 2: "k_gemm2", 3: "k_fused_mu", 4: "k_fused_res", 5: "k_fused_all",
                6: "k_fused_wide", 7: "k_fused_wide64", 8: "k_fused_xy"}


class EvcError(RuntimeError):
    def __init__(self, status, what):
        super().__init__(f"{what}: {strerror(status)} (status {status})")
        self.status = status


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -m exemplars_vc_amd.csrc.build` "
            "(hipcc, gfx950).  exemplars_vc_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64; import it FIRST so that
    # libevc_hip.so binds to the HIP runtime torch already initialised (one runtime per process:
    # shared device context, interoperable streams and events).  Loaded the other way round, two
    # HSA runtimes end up in the process and the second one sees no device.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    L.evc_version.restype = C.c_int
    L.evc_strerror.restype = C.c_char_p
    L.evc_strerror.argtypes = [C.c_int]
    L.evc_device_count.restype = C.c_int
    L.evc_workspace_bytes.restype = C.c_size_t
    L.evc_workspace_bytes.argtypes = [C.c_int] * 7
    L.evc_nmf_solve.restype = C.c_int
    L.evc_nmf_solve.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # A, X, H
        C.c_int, C.c_int, C.c_int,                                          # M, N, T
        C.POINTER(C.c_int), C.c_int,                                        # utt_offsets, n_utt
        C.POINTER(SolveOpts),
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, err_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_nmf_convert.restype = C.c_int
    L.evc_nmf_convert.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # A, X, B
        C.c_void_p, C.c_int, C.c_void_p, C.c_int,                           # H, Y
        C.c_int, C.c_int, C.c_int, C.c_int,                                 # M, Mb, N, T
        C.POINTER(C.c_int), C.c_int, C.POINTER(SolveOpts),
        C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p,
    ]
    L.evc_dict_bytes.restype = C.c_size_t
    L.evc_dict_bytes.argtypes = [C.c_int] * 5
    L.evc_dict_prepare.restype = C.c_int
    L.evc_dict_prepare.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_double, C.c_void_p, C.c_size_t, C.POINTER(Dict), C.c_void_p]
    L.evc_synthesize.restype = C.c_int
    L.evc_synthesize.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.evc_residual.restype = C.c_int
    L.evc_residual.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.evc_griffin_lim_workspace_bytes.restype = C.c_size_t
    L.evc_griffin_lim_workspace_bytes.argtypes = [C.c_int] * 4
    L.evc_griffin_lim.restype = C.c_int
    L.evc_griffin_lim.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.c_void_p]
    L.evc_griffin_lim_batch_workspace_bytes.restype = C.c_size_t
    L.evc_griffin_lim_batch_workspace_bytes.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int]
    L.evc_griffin_lim_batch.restype = C.c_int
    L.evc_griffin_lim_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.c_void_p]
    L.evc_stft_frames.restype = C.c_int
    L.evc_stft_frames.argtypes = [C.c_long, C.c_int, C.c_int, C.c_int]
    L.evc_stft_workspace_bytes.restype = C.c_size_t
    L.evc_stft_workspace_bytes.argtypes = [C.c_long, C.c_int, C.c_int, C.c_int]
    L.evc_stft.restype = C.c_int
    L.evc_stft.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                           C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    L.evc_dtw_workspace_bytes.restype = C.c_size_t
    L.evc_dtw_workspace_bytes.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    L.evc_dtw_align.restype = C.c_int
    L.evc_dtw_align.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_size_t, C.c_void_p]
    L.evc_dtw_path_rows.restype = C.c_int
    L.evc_dtw_path_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    L.evc_dtw_gather_rows.restype = C.c_int
    L.evc_dtw_gather_rows.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p]
    L.evc_cd_workspace_bytes.restype = C.c_size_t
    L.evc_cd_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_cd_solve.restype = C.c_int
    L.evc_cd_solve.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # A, X, H
        C.c_int, C.c_int, C.c_int,                                          # M, N, T
        C.POINTER(C.c_int), C.c_int, C.POINTER(CdOpts),                     # utt_offsets, n_utt, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, violation_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_learn_workspace_bytes.restype = C.c_size_t
    L.evc_learn_workspace_bytes.argtypes = [C.c_int] * 4
    L.evc_learn_splits.restype = C.c_int
    L.evc_learn_splits.argtypes = [C.c_int] * 3
    L.evc_nmf_learn.restype = C.c_int
    L.evc_nmf_learn.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # X, W, H
        C.c_int, C.c_int, C.c_int, C.POINTER(LearnOpts),                    # M, R, T, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, err_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_cd_learn_workspace_bytes.restype = C.c_size_t
    L.evc_cd_learn_workspace_bytes.argtypes = [C.c_int] * 4
    L.evc_cd_learn_splits.restype = C.c_int
    L.evc_cd_learn_splits.argtypes = [C.c_int] * 3
    L.evc_cd_learn.restype = C.c_int
    L.evc_cd_learn.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # X, W, H
        C.c_int, C.c_int, C.c_int, C.POINTER(CdLearnOpts),                  # M, R, T, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, violation_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_mfcc_workspace_bytes.restype = C.c_size_t
    L.evc_mfcc_workspace_bytes.argtypes = [C.POINTER(C.c_long), C.c_int, C.POINTER(MfccOpts)]
    L.evc_mfcc.restype = C.c_int
    L.evc_mfcc.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.c_int, C.POINTER(MfccOpts), C.c_void_p, C.c_int,
                           C.c_void_p, C.c_int, C.c_void_p, C.c_int,          # re, im
                           C.c_void_p, C.c_size_t, C.c_void_p]
    L.evc_beta_workspace_bytes.restype = C.c_size_t
    L.evc_beta_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_beta_solve.restype = C.c_int
    L.evc_beta_solve.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # A, X, H
        C.c_int, C.c_int, C.c_int,                                          # M, N, T
        C.POINTER(C.c_int), C.c_int, C.POINTER(BetaOpts),                   # utt_offsets, n_utt, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, err_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_beta_learn_workspace_bytes.restype = C.c_size_t
    L.evc_beta_learn_workspace_bytes.argtypes = [C.c_int] * 4
    L.evc_beta_learn_splits.restype = C.c_int
    L.evc_beta_learn_splits.argtypes = [C.c_int] * 3
    L.evc_beta_learn_route.restype = C.c_int
    L.evc_beta_learn_route.argtypes = [C.c_int] * 3
    L.evc_beta_learn.restype = C.c_int
    L.evc_beta_learn.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # X, W, H
        C.c_int, C.c_int, C.c_int, C.POINTER(BetaLearnOpts),                # M, R, T, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, err_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_online_workspace_bytes.restype = C.c_size_t
    L.evc_online_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_online_splits.restype = C.c_int
    L.evc_online_splits.argtypes = [C.c_int] * 3
    L.evc_online_learn.restype = C.c_int
    L.evc_online_learn.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # X, W, H
        C.c_void_p, C.c_void_p, C.c_int,                                    # acc_a, acc_b, ld_acc
        C.c_int, C.c_int, C.c_int, C.POINTER(OnlineOpts),                   # M, R, T, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),      # n_iter_out, n_steps_out, trace_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_online_transform_workspace_bytes.restype = C.c_size_t
    L.evc_online_transform_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_online_transform.restype = C.c_int
    L.evc_online_transform.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # W, X, H
        C.c_int, C.c_int, C.c_int,                                          # M, R, T
        C.POINTER(C.c_int), C.c_int, C.POINTER(TransformOpts),              # utt_offsets, n_utt, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, change_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_online_fresh_workspace_bytes.restype = C.c_size_t
    L.evc_online_fresh_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_online_learn_fresh.restype = C.c_int
    L.evc_online_learn_fresh.argtypes = L.evc_online_learn.argtypes[:12] + [C.POINTER(OnlineFreshOpts)] + \
        L.evc_online_learn.argtypes[13:]
    L.evc_deconv_workspace_bytes.restype = C.c_size_t
    L.evc_deconv_workspace_bytes.argtypes = [C.c_int] * 6
    L.evc_deconv_solve.restype = C.c_int
    L.evc_deconv_solve.argtypes = [
        C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_int,    # A (lda, tap_stride), X, H
        C.c_int, C.c_int, C.c_int,                                          # M, N, T
        C.POINTER(C.c_int), C.c_int, C.POINTER(DeconvOpts),                 # utt_offsets, n_utt, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, err_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_deconv_synthesize.restype = C.c_int
    L.evc_deconv_synthesize.argtypes = [
        C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_int,    # B (ldb, tap_stride), H, Y
        C.c_int, C.c_int, C.c_int,                                          # Mb, N, T
        C.POINTER(C.c_int), C.c_int,                                        # utt_offsets, n_utt
        C.c_int, C.c_int, C.c_int,                                          # taps, layout, dtype
        C.c_void_p,                                                         # stream
    ]
    L.evc_deconv_learn_workspace_bytes.restype = C.c_size_t
    L.evc_deconv_learn_workspace_bytes.argtypes = [C.c_int] * 7
    L.evc_deconv_learn_splits.restype = C.c_int
    L.evc_deconv_learn_splits.argtypes = [C.c_int] * 5
    L.evc_deconv_learn.restype = C.c_int
    L.evc_deconv_learn.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_int,    # X, W (ldw, tap_stride), H
        C.c_int, C.c_int, C.c_int,                                          # M, R, T
        C.POINTER(C.c_int), C.c_int, C.POINTER(DeconvLearnOpts),            # utt_offsets, n_utt, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, err_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_convex_workspace_bytes.restype = C.c_size_t
    L.evc_convex_workspace_bytes.argtypes = [C.c_int] * 4
    L.evc_convex_splits.restype = C.c_int
    L.evc_convex_splits.argtypes = [C.c_int] * 2
    L.evc_convex_learn.restype = C.c_int
    L.evc_convex_learn.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,   # X, G, H, W
        C.c_int, C.c_int, C.c_int,                                          # M, R, T
        C.POINTER(ConvexOpts), C.c_void_p, C.c_size_t,                      # opts, workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, err_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_semi_workspace_bytes.restype = C.c_size_t
    L.evc_semi_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_semi_solve.restype = C.c_int
    L.evc_semi_solve.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # A, X, H
        C.c_int, C.c_int, C.c_int,                                          # M, N, T
        C.POINTER(C.c_int), C.c_int, C.POINTER(SemiOpts),                   # utt_offsets, n_utt, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, err_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_prox_workspace_bytes.restype = C.c_size_t
    L.evc_prox_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_prox_solve.restype = C.c_int
    L.evc_prox_solve.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # A, X, H
        C.c_int, C.c_int, C.c_int,                                          # M, N, T
        C.POINTER(C.c_int), C.c_int, C.POINTER(ProxOpts),                   # utt_offsets, n_utt, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, change_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_prox_masked_workspace_bytes.restype = C.c_size_t
    L.evc_prox_masked_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_prox_masked_solve.restype = C.c_int
    L.evc_prox_masked_solve.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # A, X, mask, H
        C.c_int, C.c_int, C.c_int,                                          # M, N, T
        C.POINTER(C.c_int), C.c_int, C.POINTER(ProxMaskedOpts),             # utt_offsets, n_utt, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, change_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_prox_learn_workspace_bytes.restype = C.c_size_t
    L.evc_prox_learn_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_prox_learn_block.restype = C.c_int
    L.evc_prox_learn_block.argtypes = [C.c_int] * 2
    L.evc_prox_learn.restype = C.c_int
    L.evc_prox_learn.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # X, D, H
        C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int),   # stats, ld_stats, count_io, order
        C.c_int, C.c_int, C.c_int, C.POINTER(ProxLearnOpts),                # M, N, T, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),      # n_epochs_out, n_steps_out, trace_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_prox_masked_learn_workspace_bytes.restype = C.c_size_t
    L.evc_prox_masked_learn_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_prox_masked_learn.restype = C.c_int
    L.evc_prox_masked_learn.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # X, mask, D, H
        C.c_void_p, C.c_int, C.c_void_p, C.c_int,                           # stats_s, ld_s, stats_q, ld_q
        C.POINTER(C.c_longlong), C.POINTER(C.c_int),                        # count_io, order
        C.c_int, C.c_int, C.c_int, C.POINTER(ProxMaskedLearnOpts),          # M, N, T, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),      # n_epochs_out, n_steps_out, trace_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_mu_masked_workspace_bytes.restype = C.c_size_t
    L.evc_mu_masked_workspace_bytes.argtypes = [C.c_int] * 5
    L.evc_mu_masked_solve.restype = C.c_int
    L.evc_mu_masked_solve.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # A, X, mask, H
        C.c_int, C.c_int, C.c_int,                                          # M, N, T
        C.POINTER(C.c_int), C.c_int, C.POINTER(MuMaskedOpts),               # utt_offsets, n_utt, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, err_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_mu_masked_learn_workspace_bytes.restype = C.c_size_t
    L.evc_mu_masked_learn_workspace_bytes.argtypes = [C.c_int] * 4
    L.evc_mu_masked_learn_splits.restype = C.c_int
    L.evc_mu_masked_learn_splits.argtypes = [C.c_int] * 3
    L.evc_mu_masked_learn.restype = C.c_int
    L.evc_mu_masked_learn.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # X, mask, W, H
        C.c_int, C.c_int, C.c_int, C.POINTER(MuMaskedLearnOpts),            # M, R, T, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, stat_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_mu_stoch_learn_workspace_bytes.restype = C.c_size_t
    L.evc_mu_stoch_learn_workspace_bytes.argtypes = [C.c_int] * 6
    L.evc_mu_stoch_learn_route.restype = C.c_int
    L.evc_mu_stoch_learn_route.argtypes = [C.c_int] * 2
    L.evc_mu_stoch_learn_splits.restype = C.c_int
    L.evc_mu_stoch_learn_splits.argtypes = [C.c_int] * 4
    L.evc_mu_stoch_learn.restype = C.c_int
    L.evc_mu_stoch_learn.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,      # X, mask, W, H
        C.POINTER(C.c_int),                                                 # order
        C.c_int, C.c_int, C.c_int, C.POINTER(MuStochOpts),                  # M, R, T, opts
        C.c_void_p, C.c_size_t,                                             # workspace
        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),      # n_epochs_out, n_steps_out, trace_out
        C.c_void_p,                                                         # stream
    ]
    L.evc_kmeans_workspace_bytes.restype = C.c_size_t
    L.evc_kmeans_workspace_bytes.argtypes = [C.c_int] * 4
    L.evc_kmeans_splits.restype = C.c_int
    L.evc_kmeans_splits.argtypes = [C.c_int] * 2
    L.evc_kmeans.restype = C.c_int
    L.evc_kmeans.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,   # X, W, labels, counts
        C.c_int, C.c_int, C.c_int,                                          # M, R, T
        C.POINTER(KmeansOpts), C.c_void_p, C.c_size_t,                      # opts, workspace
        C.POINTER(C.c_int), C.POINTER(C.c_double),                          # n_iter_out, err_out
        C.c_void_p,                                                         # stream
    ]
    _lib = L
    return L


def strerror(status: int) -> str:
    return lib().evc_strerror(int(status)).decode()


def check(status: int, what: str):
    if status != 0:
        raise EvcError(status, what)
