"""ctypes binding of libglf.so -- the C-ABI declared in include/glf.h.

Python is plumbing only: torch tensors provide device memory and the current
HIP stream, torch.distributed (backend "nccl" = RCCL) provides the collectives
plugged into glf_comm. All compute happens in the HIP library; if libglf.so is
missing this module raises at import time (there is no CPU fallback).

Function names mirror the reference's stage functions (hpc/*.h) exactly as the
C-ABI does: ComputeAffinityMatrices, ComputeLaplacianMatrix,
InversePowerIteration, OrthonormaliseVecs, Nystroem, Permutation,
ComputeResultFromLaplacian, plus image_processing for the whole path.
"""
import collections
import ctypes as C
import functools
import os

import numpy as np
# torch bundles its own libamdhip64.so.7; it must be loaded BEFORE libglf.so so that the
# process ends up with one HIP runtime (the dynamic linker de-duplicates by SONAME and the
# first one wins). Loading libglf.so first pairs torch with /opt/rocm's runtime and
# hipGetDeviceCount then fails inside this library.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GLF_LIBRARY", os.path.join(_HERE, "libglf.so"))  # override: profiling builds only
if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libglf.so not found at %s: build it with `make` (or __graft_entry__.build()); "
        "there is no CPU fallback for the HIP path" % LIB_PATH)
_lib = C.CDLL(LIB_PATH)

OK = 0
ERR_INVALID, ERR_NOMEM, ERR_HIP, ERR_NODEVICE, ERR_COMM, ERR_NOCONV, ERR_IO, ERR_UNSUPPORTED = range(-1, -9, -1)
MAT_DENSE, MAT_DIAG, MAT_KERNEL_B = 0, 1, 2
ROWS_NA, ROWS_SAMPLE_FIRST, ROWS_RASTER = 0, 1, 2
KERNEL_BILATERAL, KERNEL_PHOTOMETRIC, KERNEL_SPATIAL, KERNEL_NLM, KERNEL_BILATERAL_RGB, KERNEL_BILATERAL_U16 = 0, 1, 2, 3, 4, 5
KERNEL_BILATERAL_F32 = 6
KERNEL_BILATERAL_RGBF32 = 7
CONTRACT_F32_MFMA, CONTRACT_F16_SPLIT = 1, 2
FILTER_REFERENCE, FILTER_POC, FILTER_SMOOTH, FILTER_SHARPEN = 0, 1, 2, 3
SAMPLING_UNIFORM, SAMPLING_RANDOM = 0, 1
MULTI_RCCL, MULTI_LOOPBACK = 0, 1
RCCL_ID_BYTES = 128

# every symbol include/glf.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "glf_strerror", "glf_ctx_create", "glf_ctx_destroy", "glf_ctx_synchronize", "glf_ctx_last_error",
    "glf_ctx_device_info", "glf_ctx_set_tuning", "glf_ctx_set_comm", "glf_rccl_unique_id", "glf_ctx_set_comm_rccl", "glf_ctx_comm_info", "glf_ctx_comm_counters", "glf_multi_create", "glf_multi_destroy",
    "glf_multi_size", "glf_multi_ctx", "glf_multi_last_error", "glf_multi_image_processing", "glf_shard_rows", "glf_band_plan", "glf_ctx_set_contraction", "glf_malloc", "glf_free", "glf_memcpy_h2d", "glf_memcpy_d2h",
    "glf_memset", "glf_mat_create_dense", "glf_mat_create_diag", "glf_mat_destroy", "glf_mat_get_column", "glf_Sampling",
    "glf_host_free", "glf_random_vectors", "glf_synth_image", "glf_RandomSampling", "glf_ComputeAffinityMatrices",
    "glf_ComputeLaplacianMatrix", "glf_InversePowerIteration", "glf_OrthonormaliseVecs", "glf_NormaliseVecs",
    "glf_InverseDiagMat", "glf_Nystroem", "glf_Permutation", "glf_ComputeResultFromLaplacian", "glf_Sinkhorn", "glf_SinkhornRows", "glf_Orthogonalisation",
    "glf_options_default", "glf_image_processing", "glf_image_processing_capture", "glf_ctx_debug_violations", "glf_ctx_cached_bytes", "glf_image_processing_batch", "glf_EntireComputation", "glf_read_png", "glf_write_png", "glf_read_png_rgb", "glf_write_png_rgb",
    "glf_image_processing_signals", "glf_multi_image_processing_signals",
    "glf_image_processing_rgb", "glf_multi_image_processing_rgb", "glf_image_processing_rgb_capture",
    "glf_image_processing_u16", "glf_multi_image_processing_u16", "glf_image_processing_u16_capture", "glf_read_png16", "glf_write_png16",
    "glf_image_processing_rgb_signals", "glf_image_processing_u16_signals",
    "glf_multi_image_processing_rgb_signals", "glf_multi_image_processing_u16_signals",
    "glf_image_processing_f32", "glf_image_processing_f32_capture", "glf_image_processing_f32_signals",
    "glf_multi_image_processing_f32", "glf_multi_image_processing_f32_signals", "glf_read_pfm", "glf_write_pfm",
    "glf_image_processing_rgbf32", "glf_image_processing_rgbf32_capture", "glf_image_processing_rgbf32_signals",
    "glf_multi_image_processing_rgbf32", "glf_multi_image_processing_rgbf32_signals", "glf_read_pfm_rgb", "glf_write_pfm_rgb",
    "glf_graph_build", "glf_graph_destroy", "glf_graph_get_info", "glf_graph_eigenvalues", "glf_graph_gram", "glf_graph_project",
    "glf_graph_synthesize", "glf_filter_coeffs", "glf_graph_normal_equations", "glf_fit_coeffs",
    "glf_robust_weight", "glf_robust_scale", "glf_graph_robust_step", "glf_graph_fit_robust",
    "glf_graph_cluster_step", "glf_cluster_update", "glf_cluster_seed", "glf_graph_segment",
    "glf_graph_cluster_step_ex", "glf_cluster_update_w", "glf_cluster_seed_w", "glf_graph_segment_ex",
    "glf_graph_transform", "glf_basis_orthonormal", "glf_graph_orthonormalize", "glf_graph_project_wide",
    "glf_graph_compact", "glf_graph_storage", "glf_graph_dequantize",
    "glf_graph_quadform", "glf_fit_factor", "glf_graph_rows",
    "glf_graph_edges", "glf_graph_samples",
    "glf_graph_classify",
    "glf_graph_softmax",
    "glf_graph_blend",
    "glf_operator_create", "glf_operator_apply", "glf_operator_solve", "glf_operator_stored", "glf_operator_destroy",
    "glf_Nystroem_ex", "glf_Degree_ex", "glf_Filter_ex",
]
MAX_SIGNALS = 4
PIX_U8, PIX_RGB8, PIX_U16, PIX_F32, PIX_RGBF32 = 0, 1, 2, 3, 4
# The guide formats, one row per PIX_*: everything the image_processing* methods of Context and Multi and Context.graph know of a
# format. torch_dtype / zeros_dtype are names (torch is looked up per context): torch fills no uint16, so the 16-bit outputs are
# allocated as int16 and viewed as uint16. float_out: the output is the float z itself, so the call takes and returns no zf.
# suffix: the entry points are glf_[multi_]image_processing<suffix>[_capture | _signals].
# wait_stream: the plain call orders the context's stream behind the caller's before the library reads the image; the 8-bit
# call never did (its callers hand it images that are complete), and it is the call the benchmark times.
_PixFormat = collections.namedtuple("_PixFormat", "np_dtype torch_dtype zeros_dtype channels float_out suffix wait_stream")
_PIX_FORMATS = {
    PIX_U8: _PixFormat(np.uint8, "uint8", "uint8", 1, False, "", False),
    PIX_RGB8: _PixFormat(np.uint8, "uint8", "uint8", 3, False, "_rgb", True),
    PIX_U16: _PixFormat(np.uint16, "uint16", "int16", 1, False, "_u16", True),
    PIX_F32: _PixFormat(np.float32, "float32", "float32", 1, True, "_f32", True),
    PIX_RGBF32: _PixFormat(np.float32, "float32", "float32", 3, True, "_rgbf32", True),
}
GRAPH_MAX_OUTPUTS = 32
GRAPH_MAX_PLANES = 32      # GLF_GRAPH_MAX_PLANES: the most planes of one glf_graph_project_wide call
GRAPH_NORMAL_CHAIN = 128   # GLF_GRAPH_NORMAL_CHAIN: the longest f32 chain (pixel terms) of glf_graph_normal_equations' G
QUAD_MAX_COLS = 64         # GLF_QUAD_MAX_COLS: the most columns of R of one glf_graph_quadform call
QUAD_MAX_CENTRES = 32      # GLF_QUAD_MAX_CENTRES: the most centres of one glf_graph_quadform call
EDGE_DIRS = {"E": 1, "S": 2, "SE": 4, "SW": 8}   # GLF_EDGE_*: the neighbour (row, col+1), (row+1, col), (row+1, col+1), (row+1, col-1)
CLASSIFY_MAX = 32          # GLF_CLASSIFY_MAX: the most classes of one glf_graph_classify call
SOFTMAX_MAX = 32           # GLF_SOFTMAX_MAX: the most classes of one glf_graph_softmax call
BLEND_MAX_SLOTS = 32       # GLF_BLEND_MAX_SLOTS: the most slots (outputs x levels) of one glf_graph_blend call
CLUSTER_MAX = 32           # GLF_CLUSTER_MAX: the most centroids of glf_graph_cluster_step / glf_graph_segment
PHI_F32, PHI_F16 = 0, 1    # GLF_PHI_*: how a graph handle stores Phi (glf_graph_compact)
BASIS_CHOLESKY, BASIS_RITZ = 0, 1
ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_TUKEY = 0, 1, 2
ROBUST_LOSSES = {"huber": ROBUST_HUBER, "cauchy": ROBUST_CAUCHY, "tukey": ROBUST_TUKEY}
ROBUST_DEFAULT_C = {ROBUST_HUBER: 1.345, ROBUST_CAUCHY: 2.385, ROBUST_TUKEY: 4.685}   # c = 0: 95 % efficiency under Gaussian noise
ROBUST_OBJECTIVES = 32     # GLF_ROBUST_OBJECTIVES: the iterations whose objective glf_graph_fit_robust reports


class Mat(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("row_order", C.c_int32), ("rows", C.c_int64), ("cols", C.c_int64),
        ("ld", C.c_int64), ("data", C.c_void_p), ("owns_data", C.c_int32),
        ("img", C.c_void_p), ("samples", C.c_void_p), ("mask", C.c_void_p), ("idx", C.c_void_p),
        ("width", C.c_int32), ("height", C.c_int32), ("p", C.c_uint32), ("scale", C.c_float),
        ("h_loc", C.c_float), ("h_val", C.c_float), ("kernel", C.c_int32), ("degree", C.c_void_p),
        ("owns_desc", C.c_int32),
    ]


class EigStats(C.Structure):
    _fields_ = [("outer_its", C.c_int32), ("inner_its_total", C.c_int32), ("residual", C.c_double),
                ("matvecs", C.c_int32), ("matvec_ms", C.c_float), ("matvec_bytes", C.c_double),
                ("narrow_sweeps", C.c_int32), ("reserved", C.c_int32)]


class Options(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("num_samples", C.c_uint32), ("sample_frac", C.c_double),
        ("num_eigvals", C.c_uint32), ("opti_gs", C.c_int32), ("epsilon", C.c_double),
        ("inner_rtol", C.c_double), ("max_outer", C.c_int32), ("seed", C.c_uint64), ("gain", C.c_float),
        ("h_loc", C.c_float), ("h_val", C.c_float), ("kernel", C.c_int32), ("filter_pow", C.c_int32),
        ("filter_mode", C.c_int32), ("skip_exact_zeros", C.c_int32), ("filter_beta", C.c_float),
        ("sampling", C.c_int32), ("reserved_", C.c_uint32), ("sampling_seed", C.c_uint64),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("p", C.c_uint32), ("m", C.c_uint32), ("alpha", C.c_double), ("eig", EigStats),
        ("ms_affinity", C.c_float), ("ms_laplacian", C.c_float), ("ms_eigen", C.c_float),
        ("ms_nystroem", C.c_float), ("ms_filter", C.c_float), ("ms_total", C.c_float),
        ("nystroem_launches", C.c_int32), ("nystroem_kernel_ms", C.c_float),
        ("row0", C.c_int32), ("row1", C.c_int32), ("contraction", C.c_int32), ("skip_exact_zeros", C.c_int32),
        ("nystroem_evaluated", C.c_double), ("degree_evaluated", C.c_double),
        ("nystroem_mfma_flops", C.c_double), ("nystroem_path", C.c_int32), ("matvec_path", C.c_int32),
        ("nystroem_rowpass_launches", C.c_int32), ("nystroem_rowpass_ms", C.c_float), ("nystroem_rowpass_flops", C.c_double),
        ("nystroem_colpass_launches", C.c_int32), ("nystroem_colpass_ms", C.c_float), ("nystroem_colpass_flops", C.c_double),
        ("rank_terms", C.c_int32), ("filter_fused", C.c_int32), ("eigen_sharded", C.c_int32), ("reserved_", C.c_int32),
    ]


class Capture(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("ld", C.c_uint32), ("d_phi_A", C.c_void_p), ("phi_A_floats", C.c_size_t),
                ("d_phi", C.c_void_p), ("phi_floats", C.c_size_t), ("h_c", C.c_void_p), ("h_degree", C.c_void_p),
                ("d_corr", C.c_void_p), ("corr_floats", C.c_size_t)]


class GraphInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("pix", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("p", C.c_uint32),
                ("m", C.c_uint32), ("ld", C.c_uint32), ("d_phi", C.c_void_p), ("phi_bytes", C.c_size_t)]


class SegmentOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_uint32), ("dim", C.c_uint32), ("max_iter", C.c_uint32), ("sample_rows", C.c_uint32),
                ("init", C.c_int32), ("seed", C.c_uint64), ("scale", C.c_void_p)]


class SegmentStats(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("converged", C.c_int32), ("changed_last", C.c_uint64), ("counts", C.c_uint64 * CLUSTER_MAX)]


class ClusterEmbed(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("normalize", C.c_int32), ("d_weight", C.c_void_p)]


class RobustLoss(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("c", C.c_double), ("sigma", C.c_double * MAX_SIGNALS)]


class RobustOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("loss", RobustLoss), ("penalty", C.c_void_p), ("max_iter", C.c_uint32), ("tol", C.c_double),
                ("sample_rows", C.c_uint32), ("estimate_sigma", C.c_int32)]


class RobustStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("converged", C.c_int32), ("sigma", C.c_double * MAX_SIGNALS),
                ("mass", C.c_double), ("objective", C.c_double * ROBUST_OBJECTIVES)]


class OperatorInfo(C.Structure):
    _fields_ = [("path", C.c_int32), ("ksplit", C.c_int32), ("skipping", C.c_int32), ("row0", C.c_int32), ("row1", C.c_int32)]


class SolveInfo(C.Structure):
    _fields_ = [("iters", C.c_int32), ("unconverged", C.c_int32), ("matvecs", C.c_int32), ("narrow_sweeps", C.c_int32),
                ("path", C.c_int32), ("reserved", C.c_int32)]


class NystroemInfo(C.Structure):
    _fields_ = [("path", C.c_int32), ("contraction", C.c_int32), ("skipping", C.c_int32), ("lut", C.c_int32), ("row0", C.c_uint32),
                ("row1", C.c_uint32), ("entries_evaluated", C.c_double)]


class DegreeInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("path", C.c_int32), ("shape", C.c_int32), ("skipping", C.c_int32), ("chunks", C.c_int32),
                ("mgroups", C.c_int32), ("row0", C.c_uint32), ("row1", C.c_uint32), ("entries_evaluated", C.c_double)]


DEG_DENSE, DEG_GRID, DEG_WINDOWED, DEG_ENTRYWISE, DEG_NLM = 0, 1, 2, 5, 6   # glf_degree_info.path
DEG_FIVES, DEG_TEN, DEG_WINDOW = 0, 1, 2                                    # glf_degree_info.shape (grid form)


class FilterRequest(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("pix", C.c_int32), ("d_img", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("phi", C.c_void_p), ("lam", C.c_void_p), ("filter_mode", C.c_int32), ("filter_pow", C.c_int32), ("filter_beta", C.c_float),
                ("gain", C.c_float), ("row0", C.c_uint32), ("row1", C.c_uint32), ("nsig", C.c_int32), ("reserved_", C.c_uint32),
                ("d_sig", C.c_void_p), ("d_sig_out", C.c_void_p), ("h_c_in", C.c_void_p), ("h_c_out", C.c_void_p), ("h_gram_out", C.c_void_p),
                ("d_out", C.c_void_p), ("d_zf", C.c_void_p), ("d_corr", C.c_void_p)]


class FilterInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kernels", C.c_uint32), ("ld", C.c_uint32), ("panels", C.c_uint32), ("proj_blocks", C.c_uint32),
                ("apply_blocks", C.c_uint32), ("grid_strided", C.c_uint32), ("reserved_", C.c_uint32), ("pix0", C.c_uint64), ("pix1", C.c_uint64)]


# glf_filter_info.kernels
(FK_PHI_T_Y, FK_PHI_T_SIGNALS, FK_PHI_T_PIX_SIGNALS, FK_PHI_GRAM, FK_APPLY, FK_APPLY_SIGNALS, FK_APPLY_PIX, FK_APPLY_PIX_SIGNALS, FK_PLANES,
 FK_ACCUM, FK_FINISH) = (1 << i for i in range(11))


class BasisStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("passes", C.c_uint32), ("defect_in", C.c_double), ("defect_out", C.c_double)]


ALLREDUCE_F32 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
ALLREDUCE_F64 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
ALLGATHER_F32 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)


class Comm(C.Structure):
    _fields_ = [("rank", C.c_int), ("size", C.c_int), ("allreduce_sum_f32", ALLREDUCE_F32),
                ("allreduce_sum_f64", ALLREDUCE_F64), ("allgather_f32", ALLGATHER_F32), ("user", C.c_void_p)]


_lib.glf_strerror.restype = C.c_char_p
_lib.glf_ctx_last_error.restype = C.c_char_p
_lib.glf_ctx_last_error.argtypes = [C.c_void_p]
_lib.glf_host_free.restype = None
_lib.glf_multi_ctx.restype = C.c_void_p
_lib.glf_multi_last_error.restype = C.c_char_p
_lib.glf_multi_last_error.argtypes = [C.c_void_p]
_lib.glf_options_default.restype = None
_lib.glf_ctx_cached_bytes.restype = C.c_size_t
_lib.glf_ctx_cached_bytes.argtypes = [C.c_void_p]
_lib.glf_graph_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
_lib.glf_graph_destroy.argtypes = [C.c_void_p]
_lib.glf_graph_get_info.argtypes = [C.c_void_p, C.c_void_p]
_lib.glf_graph_eigenvalues.argtypes = [C.c_void_p, C.c_void_p]
_lib.glf_graph_gram.argtypes = [C.c_void_p, C.c_void_p]
_lib.glf_graph_project.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
_lib.glf_graph_synthesize.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
_lib.glf_filter_coeffs.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_graph_cluster_step.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
_lib.glf_cluster_update.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_cluster_seed.argtypes = [C.c_void_p, C.c_size_t, C.c_uint, C.c_uint, C.c_uint64, C.c_void_p]
_lib.glf_graph_segment.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_graph_cluster_step_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_cluster_update_w.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_cluster_seed_w.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint, C.c_uint64, C.c_void_p]
_lib.glf_graph_segment_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_robust_weight.argtypes = [C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
_lib.glf_robust_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
_lib.glf_graph_robust_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_graph_fit_robust.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_graph_transform.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
_lib.glf_basis_orthonormal.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_graph_orthonormalize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
_lib.glf_graph_project_wide.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
_lib.glf_graph_compact.argtypes = [C.c_void_p, C.c_int]
_lib.glf_graph_storage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_graph_dequantize.argtypes = [C.c_void_p, C.c_void_p]
_lib.glf_graph_quadform.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p, C.c_int, C.c_void_p]
_lib.glf_fit_factor.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_graph_rows.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
_lib.glf_graph_edges.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_graph_samples.argtypes = [C.c_void_p, C.c_void_p]
_lib.glf_graph_softmax.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
_lib.glf_graph_blend.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_graph_classify.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
_lib.glf_operator_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
_lib.glf_operator_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_operator_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_double, C.c_int, C.c_void_p]
_lib.glf_operator_stored.argtypes = [C.c_void_p, C.c_void_p]
_lib.glf_operator_destroy.argtypes = [C.c_void_p]
_lib.glf_Nystroem_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
_lib.glf_Degree_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_uint,
                               C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
_lib.glf_Filter_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]


class GlfError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = _lib.glf_strerror(status).decode()
        super().__init__("glf status %d (%s)%s" % (status, msg, (": " + detail) if detail else ""))


def default_options(**kw):
    opt = Options()
    _lib.glf_options_default(C.byref(opt))
    for k, v in kw.items():
        if not hasattr(opt, k):
            raise AttributeError("glf_options has no field %r" % k)
        setattr(opt, k, v)
    return opt


# ---- host-side stages ---------------------------------------------------------------

def Sampling(width, height, sample_size):
    """hpc/sampling.c:6-33 -> (realised count, uint32 indices)."""
    n = C.c_uint(sample_size)
    ptr = C.POINTER(C.c_uint)()
    rc = _lib.glf_Sampling(C.c_int(width), C.c_int(height), C.byref(n), C.byref(ptr))
    if rc != OK:
        raise GlfError(rc, "Sampling(%d, %d, %d)" % (width, height, sample_size))
    idx = np.ctypeslib.as_array(ptr, shape=(max(n.value, 1),))[:n.value].astype(np.uint32).copy()
    _lib.glf_host_free(ptr)
    return idx


def RandomSampling(width, height, sample_size, seed=1):
    """python/sampling/random.py:8-16 -> sample_size distinct pixel indices, ascending (the library's own generator)."""
    n = C.c_uint(sample_size)
    ptr = C.POINTER(C.c_uint)()
    rc = _lib.glf_RandomSampling(C.c_int(width), C.c_int(height), C.byref(n), C.byref(ptr), C.c_uint64(seed))
    if rc != OK:
        raise GlfError(rc, "RandomSampling(%d, %d, %d)" % (width, height, sample_size))
    idx = np.ctypeslib.as_array(ptr, shape=(max(n.value, 1),))[:n.value].astype(np.uint32).copy()
    _lib.glf_host_free(ptr)
    return idx


def random_vectors(p, m, seed=1):
    X0 = np.empty((m, p), dtype=np.float64)
    rc = _lib.glf_random_vectors(X0.ctypes.data_as(C.c_void_p), C.c_uint(p), C.c_uint(m), C.c_uint64(seed))
    if rc != OK:
        raise GlfError(rc)
    return X0


def synth_image(width, height, seed=0):
    out = np.empty((height, width), dtype=np.uint8)
    rc = _lib.glf_synth_image(out.ctypes.data_as(C.c_void_p), C.c_int(width), C.c_int(height), C.c_uint64(seed))
    if rc != OK:
        raise GlfError(rc)
    return out


def read_png(path):
    rows = C.POINTER(C.POINTER(C.c_uint8))()
    w, h = C.c_int(), C.c_int()
    rc = _lib.glf_read_png(path.encode(), C.byref(rows), C.byref(w), C.byref(h))
    if rc != 0:
        raise GlfError(ERR_IO, path)
    img = np.empty((h.value, w.value), dtype=np.uint8)
    for r in range(h.value):
        img[r] = np.ctypeslib.as_array(rows[r], shape=(w.value,))
        _lib.glf_host_free(rows[r])
    _lib.glf_host_free(rows)
    return img


def read_png_rgb(path):
    rows = C.POINTER(C.POINTER(C.c_uint8))()
    w, h = C.c_int(), C.c_int()
    rc = _lib.glf_read_png_rgb(path.encode(), C.byref(rows), C.byref(w), C.byref(h))
    if rc != 0:
        raise GlfError(ERR_IO, path)
    img = np.empty((h.value, w.value, 3), dtype=np.uint8)
    for r in range(h.value):
        img[r] = np.ctypeslib.as_array(rows[r], shape=(w.value * 3,)).reshape(w.value, 3)
        _lib.glf_host_free(rows[r])
    _lib.glf_host_free(rows)
    return img


def write_png(path, img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    rowptr = (C.POINTER(C.c_uint8) * h)()
    for r in range(h):
        rowptr[r] = C.cast(img.ctypes.data + r * w, C.POINTER(C.c_uint8))
    rc = _lib.glf_write_png(path.encode(), rowptr, C.c_uint(w), C.c_uint(h))
    if rc != 0:
        raise GlfError(ERR_IO, path)


def read_png16(path):
    """A 16-bit greyscale PNG (colour type 0, bit depth 16) as uint16 [H, W]; any other format raises GlfError."""
    rows = C.POINTER(C.POINTER(C.c_uint16))()
    w, h = C.c_int(), C.c_int()
    rc = _lib.glf_read_png16(path.encode(), C.byref(rows), C.byref(w), C.byref(h))
    if rc != 0:
        raise GlfError(ERR_IO, path)
    img = np.empty((h.value, w.value), dtype=np.uint16)
    for r in range(h.value):
        img[r] = np.ctypeslib.as_array(rows[r], shape=(w.value,))
        _lib.glf_host_free(rows[r])
    _lib.glf_host_free(rows)
    return img


def write_png16(path, img):
    """Writes uint16 [H, W] as a 16-bit greyscale PNG."""
    img = np.ascontiguousarray(img, dtype=np.uint16)
    h, w = img.shape
    rowptr = (C.POINTER(C.c_uint16) * h)()
    for r in range(h):
        rowptr[r] = C.cast(img.ctypes.data + r * w * 2, C.POINTER(C.c_uint16))
    rc = _lib.glf_write_png16(path.encode(), rowptr, C.c_uint(w), C.c_uint(h))
    if rc != 0:
        raise GlfError(ERR_IO, path)


def read_pfm(path):
    """A greyscale Portable Float Map ("Pf", either byte order) as float32 [H, W], rows top first; anything else raises GlfError."""
    rows = C.POINTER(C.POINTER(C.c_float))()
    w, h = C.c_int(), C.c_int()
    rc = _lib.glf_read_pfm(path.encode(), C.byref(rows), C.byref(w), C.byref(h))
    if rc != 0:
        raise GlfError(ERR_IO, path)
    img = np.empty((h.value, w.value), dtype=np.float32)
    for r in range(h.value):
        img[r] = np.ctypeslib.as_array(rows[r], shape=(w.value,))
        _lib.glf_host_free(rows[r])
    _lib.glf_host_free(rows)
    return img


def write_pfm(path, img):
    """Writes float32 [H, W] as a little-endian greyscale Portable Float Map (scale -1.0)."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    h, w = img.shape
    rowptr = (C.POINTER(C.c_float) * h)()
    for r in range(h):
        rowptr[r] = C.cast(img.ctypes.data + r * w * 4, C.POINTER(C.c_float))
    rc = _lib.glf_write_pfm(path.encode(), rowptr, C.c_uint(w), C.c_uint(h))
    if rc != 0:
        raise GlfError(ERR_IO, path)


def read_pfm_rgb(path):
    """A colour Portable Float Map ("PF", either byte order) as float32 [H, W, 3], rows top first; anything else raises GlfError."""
    rows = C.POINTER(C.POINTER(C.c_float))()
    w, h = C.c_int(), C.c_int()
    rc = _lib.glf_read_pfm_rgb(path.encode(), C.byref(rows), C.byref(w), C.byref(h))
    if rc != 0:
        raise GlfError(ERR_IO, path)
    img = np.empty((h.value, w.value, 3), dtype=np.float32)
    for r in range(h.value):
        img[r] = np.ctypeslib.as_array(rows[r], shape=(w.value, 3))
        _lib.glf_host_free(rows[r])
    _lib.glf_host_free(rows)
    return img


def write_pfm_rgb(path, img):
    """Writes float32 [H, W, 3] as a little-endian colour Portable Float Map (scale -1.0)."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("image must be [H, W, 3], got %s" % (img.shape,))
    h, w = img.shape[:2]
    rowptr = (C.POINTER(C.c_float) * h)()
    for r in range(h):
        rowptr[r] = C.cast(img.ctypes.data + r * w * 12, C.POINTER(C.c_float))
    rc = _lib.glf_write_pfm_rgb(path.encode(), rowptr, C.c_uint(w), C.c_uint(h))
    if rc != 0:
        raise GlfError(ERR_IO, path)


def filter_coeffs(opt, lam, c, gram=None):
    """glf_filter_coeffs (host only): (a, ident) such that ident * s + Phi a is the library's own filter of opt.filter_mode on a plane
    whose projection is c. lam [m], c [m] or [k, m] (one row per plane: a comes back in c's shape); gram [m, m] for sharpening."""
    opt = opt or default_options()
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    c2 = np.ascontiguousarray(np.atleast_2d(np.asarray(c, dtype=np.float64)))
    if lam.ndim != 1 or c2.shape[1] != lam.size:
        raise ValueError("filter_coeffs: lam %s, c %s" % (lam.shape, np.shape(c)))
    if gram is not None:
        gram = np.ascontiguousarray(gram, dtype=np.float64)
        if gram.shape != (lam.size, lam.size):
            raise ValueError("filter_coeffs: gram must be [%d, %d]" % (lam.size, lam.size))
    a = np.zeros_like(c2)
    ident = C.c_float()
    for k in range(c2.shape[0]):
        rc = _lib.glf_filter_coeffs(C.byref(opt), C.c_uint(lam.size), _ptr(lam), _ptr(gram), _ptr(c2[k]), _ptr(a[k]), C.byref(ident))
        if rc != OK:
            raise GlfError(rc, "glf_filter_coeffs(filter_mode=%d)" % opt.filter_mode)
    return a.reshape(np.shape(c)), float(ident.value)


def fit_coeffs(G, b, penalty=None):
    """glf_fit_coeffs (host only): a_k = (G + diag(penalty))^-1 b_k by an f64 Cholesky factorisation. G [m, m] symmetric, b [m] or
    [k, m] (one row per plane: a comes back in b's shape), penalty [m] >= 0 or None. A matrix that is not positive definite (NaN
    included) raises GlfError(ERR_INVALID)."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    b2 = np.ascontiguousarray(np.atleast_2d(np.asarray(b, dtype=np.float64)))
    m = G.shape[0] if G.ndim == 2 else -1
    if G.ndim != 2 or G.shape != (m, m) or b2.ndim != 2 or b2.shape[1] != m:
        raise ValueError("fit_coeffs: G %s, b %s" % (G.shape, np.shape(b)))
    if penalty is not None:
        penalty = np.ascontiguousarray(penalty, dtype=np.float64)
        if penalty.shape != (m,):
            raise ValueError("fit_coeffs: penalty must be [%d]" % m)
    a = np.zeros_like(b2)
    if b2.shape[0] == 0:
        return a.reshape(np.shape(b))
    rc = _lib.glf_fit_coeffs(C.c_uint(m), _ptr(G), _ptr(penalty), C.c_int(b2.shape[0]), _ptr(b2), _ptr(a))
    if rc != OK:
        raise GlfError(rc, "glf_fit_coeffs(m=%d): not positive definite, or an empty system" % m)
    return a.reshape(np.shape(b))


def fit_factor(G, penalty=None):
    """glf_fit_factor (host only): R [m, m] = L^-T of G + diag(penalty) = L L^T, upper triangular, so that
    phi^T (G + diag(penalty))^-1 phi = |R^T phi|^2: the R whose Graph.quadform is the leverage of the fit. G [m, m] symmetric (its
    lower triangle is read), penalty [m] or None. Raises GlfError where fit_coeffs does (not positive definite, NaN, Inf)."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    m = G.shape[0]
    if G.shape != (m, m):
        raise ValueError("G must be square, got %s" % (G.shape,))
    if penalty is not None:
        penalty = np.ascontiguousarray(penalty, dtype=np.float64)
        if penalty.shape != (m,):
            raise ValueError("penalty must be [%d], got %s" % (m, penalty.shape))
    R = np.zeros((m, m), dtype=np.float64)
    rc = _lib.glf_fit_factor(C.c_uint(m), _ptr(G), _ptr(penalty), _ptr(R))
    if rc != OK:
        raise GlfError(rc, "glf_fit_factor(m=%d): not positive definite, or an empty system" % m)
    return R


def _robust_kind(loss):
    if isinstance(loss, str):
        if loss not in ROBUST_LOSSES:
            raise ValueError("loss must be one of %s, got %r" % (sorted(ROBUST_LOSSES), loss))
        return ROBUST_LOSSES[loss]
    return int(loss)


def robust_weight(loss, q, c=None):
    """glf_robust_weight (host only): the f64 statement of the robust losses at q = r^2 >= 0 -> (u, rho), u = psi(r) / r the IRLS
    multiplier and rho the loss, in q's shape (a scalar gives two floats). loss: "huber" | "cauchy" | "tukey" (or a ROBUST_*
    constant); c: the tuning constant, None or 0 for the kind's 95 % efficiency default (1.345 / 2.385 / 4.685). An unknown kind, a c
    that is negative or not finite, a q that is negative or NaN raise GlfError(ERR_INVALID)."""
    kind, cc = _robust_kind(loss), 0.0 if c is None else float(c)
    qa = np.asarray(q, dtype=np.float64)
    u, rho = np.zeros(qa.shape), np.zeros(qa.shape)
    uo, ro = C.c_double(0.0), C.c_double(0.0)
    for i, qi in enumerate(qa.ravel()):
        rc = _lib.glf_robust_weight(C.c_int(kind), C.c_double(cc), C.c_double(qi), C.byref(uo), C.byref(ro))
        if rc != OK:
            raise GlfError(rc, "glf_robust_weight(kind=%d, c=%g, q=%g)" % (kind, cc, qi))
        u.flat[i], rho.flat[i] = uo.value, ro.value
    return (float(u), float(rho)) if qa.ndim == 0 else (u, rho)


def robust_scale(res, weight=None):
    """glf_robust_scale (host only): 1.4826 x the median of |res_i| over the entries with weight_i > 0 (None: all), the median being
    element floor((cnt - 1) / 2) of the ascending order. No entry of positive weight, an entry that is not finite or a median of 0
    raise GlfError(ERR_INVALID)."""
    res = np.ascontiguousarray(np.ravel(np.asarray(res, dtype=np.float64)))
    if weight is not None:
        weight = np.ascontiguousarray(np.ravel(np.asarray(weight, dtype=np.float64)))
        if weight.shape != res.shape:
            raise ValueError("robust_scale: weight must have res's %d entries, got %d" % (res.size, weight.size))
    sigma = C.c_double(0.0)
    rc = _lib.glf_robust_scale(_ptr(res), _ptr(weight), C.c_size_t(res.size), C.byref(sigma))
    if rc != OK:
        raise GlfError(rc, "glf_robust_scale(n=%d): no entry of positive weight, an entry that is not finite, or a median of 0" % res.size)
    return float(sigma.value)


def basis_orthonormal(G, lam=None):
    """glf_basis_orthonormal (host only): the change of basis T [m, m] that makes a basis with the Gram matrix G [m, m] orthonormal,
    T^T G T = I. lam None: T = L^-T of the Cholesky factor G = L L^T (upper triangular: Gram-Schmidt in column order) -> T.
    lam [m]: the Ritz basis of Phi diag(1 - lam) Phi^T, T = L^-T U with L^T diag(1 - lam) L = U Theta U^T -> (T, lam_new),
    lam_new = 1 - theta ascending, T diag(1 - lam_new) T^T = diag(1 - lam). Two calls give the same bits."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError("G must be [m, m], got %s" % (G.shape,))
    m = G.shape[0]
    T = np.zeros((m, m), dtype=np.float64)
    lam_new = None
    if lam is not None:
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        if lam.shape != (m,):
            raise ValueError("lam must be [%d], got %s" % (m, lam.shape))
        lam_new = np.zeros(m, dtype=np.float64)
    rc = _lib.glf_basis_orthonormal(C.c_uint(m), _ptr(G), _ptr(lam), _ptr(T), _ptr(lam_new))
    if rc != OK:
        raise GlfError(rc, "glf_basis_orthonormal(m=%d): not positive definite, not finite, or empty" % m)
    return T if lam is None else (T, lam_new)


def _scale(scale, dim):
    if scale is None:
        return None
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    if scale.shape != (dim,):
        raise ValueError("scale must be [%d], got %s" % (dim, scale.shape))
    return scale


def _update_args(name, sums, div, div_name, div_dtype, scale, cent_prev):
    """What cluster_update and cluster_update_w check and make contiguous alike -> (k, dim, scale, sums, div, cent_prev, the cent to fill)."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    div = np.ascontiguousarray(div, dtype=div_dtype)
    if sums.ndim != 2 or div.shape != (sums.shape[0],):
        raise ValueError("%s: sums %s, %s %s" % (name, sums.shape, div_name, div.shape))
    k, dim = sums.shape
    scale = _scale(scale, dim)
    if cent_prev is not None:
        cent_prev = np.ascontiguousarray(cent_prev, dtype=np.float64)
        if cent_prev.shape != (k, dim):
            raise ValueError("%s: cent_prev must be [%d, %d]" % (name, k, dim))
    return k, dim, scale, sums, div, cent_prev, np.zeros((k, dim), dtype=np.float64)


def cluster_update(sums, counts, scale=None, cent_prev=None):
    """glf_cluster_update (host only): cent_j = scale o sums_j / counts_j of one Lloyd iteration; an empty cluster keeps cent_prev_j.
    sums [k, dim] (the sums of the raw rows of Phi per label), counts [k], scale [dim] or None (= 1), cent_prev [k, dim] (may be
    None when no cluster is empty) -> cent [k, dim]."""
    k, dim, scale, sums, counts, cent_prev, cent = _update_args("cluster_update", sums, counts, "counts", np.uint64, scale, cent_prev)
    rc = _lib.glf_cluster_update(C.c_uint(k), C.c_uint(dim), _ptr(scale), _ptr(sums), _ptr(counts), _ptr(cent_prev), _ptr(cent))
    if rc != OK:
        raise GlfError(rc, "glf_cluster_update(k=%d, dim=%d): an empty cluster without cent_prev, or an empty shape" % (k, dim))
    return cent


def cluster_update_w(sums, mass, scale=None, cent_prev=None):
    """glf_cluster_update_w (host only): cent_j = scale o sums_j / mass_j, the weighted mean of one Lloyd iteration under a weight
    plane; a cluster with !(mass_j > 0) keeps cent_prev_j. sums [k, dim], mass [k] floats, scale [dim] or None (= 1), cent_prev
    [k, dim] (may be None when every mass is positive) -> cent [k, dim]."""
    k, dim, scale, sums, mass, cent_prev, cent = _update_args("cluster_update_w", sums, mass, "mass", np.float64, scale, cent_prev)
    rc = _lib.glf_cluster_update_w(C.c_uint(k), C.c_uint(dim), _ptr(scale), _ptr(sums), _ptr(mass), _ptr(cent_prev), _ptr(cent))
    if rc != OK:
        raise GlfError(rc, "glf_cluster_update_w(k=%d, dim=%d): a cluster of mass 0 without cent_prev, or an empty shape" % (k, dim))
    return cent


def _seed_args(name, rows, k, weight=None):
    """What cluster_seed and cluster_seed_w check and make contiguous alike -> (rows, weight, n, dim, the cent [k, dim] to fill)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2:
        raise ValueError("%s: rows must be [n, dim], got %s" % (name, rows.shape))
    n, dim = rows.shape
    if weight is not None:
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        if weight.shape != (n,):
            raise ValueError("%s: weight must be [%d], got %s" % (name, n, weight.shape))
    return rows, weight, n, dim, np.zeros((max(int(k), 0), dim), dtype=np.float64)


def cluster_seed_w(rows, weight, k, seed=1):
    """glf_cluster_seed_w (host only): k-means++ among rows [n, dim] with probability proportional to weight * D^2, on the uniforms of
    cluster_seed; the first centre is the first row whose running sum of the weights exceeds u_0 times their total. weight [n]
    (>= 0, finite), or None for cluster_seed itself -> cent [k, dim]."""
    rows, weight, n, dim, cent = _seed_args("cluster_seed_w", rows, k, weight)
    rc = _lib.glf_cluster_seed_w(_ptr(rows), _ptr(weight), C.c_size_t(n), C.c_uint(dim), C.c_uint(k), C.c_uint64(seed), _ptr(cent))
    if rc != OK:
        raise GlfError(rc, "glf_cluster_seed_w(n=%d, dim=%d, k=%d): fewer than k distinct rows of positive weight, a weight that is negative "
                           "or not finite, or an empty shape" % (n, dim, k))
    return cent


def cluster_seed(rows, k, seed=1):
    """glf_cluster_seed (host only): k-means++ seeding of k centres among rows [n, dim] on the uniforms random_vectors(k, 1, seed)
    exposes -> cent [k, dim]. Fewer than k distinct rows raise GlfError(ERR_INVALID)."""
    rows, _, n, dim, cent = _seed_args("cluster_seed", rows, k)
    rc = _lib.glf_cluster_seed(_ptr(rows), C.c_size_t(n), C.c_uint(dim), C.c_uint(k), C.c_uint64(seed), _ptr(cent))
    if rc != OK:
        raise GlfError(rc, "glf_cluster_seed(n=%d, dim=%d, k=%d): fewer than k distinct rows, or an empty shape" % (n, dim, k))
    return cent


def shard_rows(height, rank, size):
    """Pixel rows [row0, row1) owned by `rank` (glf_shard_rows; used by glf_image_processing)."""
    r0, r1 = C.c_int(), C.c_int()
    rc = _lib.glf_shard_rows(C.c_int(height), C.c_int(rank), C.c_int(size), C.byref(r0), C.byref(r1))
    if rc != OK:
        raise GlfError(rc, "shard_rows(%d, %d, %d)" % (height, rank, size))
    return r0.value, r1.value


BAND_WG_ROWS = 8


def band_plan(rows, cols, width, height, h_loc=40.0, row_begin=0, row_end=None, pair_stride=64):
    """glf_band_plan: the schedule of the band-form Nystroem kernel for the image rows [row_begin, row_end) and the sample
    grid rows x cols. Returns a dict: rad, tile_px, ntiles, first_row [rows], units [rows][ntiles][pair_stride] (lo | hi << 16
    in half-blocks of 8 sample columns; lo > hi: none) and ksteps. Host only."""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    row_end = height if row_end is None else row_end
    rad, tile_px, ntiles, ksteps = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
    ip, up = C.POINTER(C.c_int), C.POINTER(C.c_uint)

    def call(first_row, units):
        rc = _lib.glf_band_plan(rows.ctypes.data_as(ip), C.c_int(rows.size), cols.ctypes.data_as(ip), C.c_int(cols.size), C.c_float(h_loc),
                                C.c_int(width), C.c_int(height), C.c_int(row_begin), C.c_int(row_end), C.c_int(pair_stride),
                                C.byref(rad), C.byref(tile_px), C.byref(ntiles), first_row, units, C.byref(ksteps))
        if rc != OK:
            raise GlfError(rc, "band_plan(%d x %d, grid %d x %d)" % (width, height, rows.size, cols.size))
    call(None, None)   # (the sizes)
    n = max(row_end - row_begin, 0)
    first_row = np.empty(n, dtype=np.int32)
    units = np.empty((n, ntiles.value, pair_stride), dtype=np.uint32)
    call(first_row.ctypes.data_as(ip), units.ctypes.data_as(up))
    return {"rad": rad.value, "tile_px": tile_px.value, "ntiles": ntiles.value, "first_row": first_row, "units": units,
            "ksteps": int(ksteps.value)}


def device_tensor_from_ptr(ptr, count, dtype, device):
    """Zero-copy torch view of `count` elements at device address `ptr`."""
    iface = {"shape": (count,), "typestr": "<f8" if dtype == torch.float64 else "<f4",
             "data": (ptr, False), "version": 2, "strides": None}

    class _Holder:
        __cuda_array_interface__ = iface
    return torch.as_tensor(_Holder(), device=device)


def make_comm(rank, size, allreduce, allgather=None):
    """glf_comm whose callbacks call allreduce(ptr, count, is_f64) and, if given,
    allgather(ptr, count_per_rank) (both in place). Exceptions become a non-zero status (they cannot
    cross the C boundary). Keep the returned struct alive for as long as the context uses it."""
    def wrap(fn, *extra):
        def cb(user, ptr, count):
            try:
                fn(ptr, count, *extra)
                return 0
            except Exception as exc:  # noqa: BLE001
                print("glf collective callback failed:", repr(exc))
                return 1
        return cb
    ag = ALLGATHER_F32(wrap(allgather)) if allgather is not None else ALLGATHER_F32()
    return Comm(rank, size, ALLREDUCE_F32(wrap(allreduce, False)), ALLREDUCE_F64(wrap(allreduce, True)), ag, None)


def rccl_unique_id():
    """ncclGetUniqueId through the library (one rank calls this, every rank passes the bytes to Context.set_comm_rccl)."""
    buf = C.create_string_buffer(RCCL_ID_BYTES)
    rc = _lib.glf_rccl_unique_id(buf, C.c_size_t(RCCL_ID_BYTES))
    if rc != OK:
        raise GlfError(rc, "glf_rccl_unique_id")
    return buf.raw


class Multi:
    """glf_multi: ONE process driving n GPU ranks (one context + one host thread each), the C host's -ngpu N.
    backend MULTI_RCCL: ncclCommInitAll over distinct devices; MULTI_LOOPBACK: host-staged collectives, ranks may share a
    device (tests on a one-GPU box)."""

    def __init__(self, n, devices=None, backend=MULTI_LOOPBACK):
        self._w = C.c_void_p()
        devs = (C.c_int * n)(*devices) if devices is not None else None
        rc = _lib.glf_multi_create(C.byref(self._w), C.c_int(n), devs, C.c_int(backend))
        if rc != OK:
            raise GlfError(rc, "glf_multi_create(%d, backend %d)" % (n, backend))
        self.n = n

    def close(self):
        if self._w:
            _lib.glf_multi_destroy(self._w)
            self._w = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_contraction(self, mode):
        for r in range(self.n):
            rc = _lib.glf_ctx_set_contraction(C.c_void_p(_lib.glf_multi_ctx(self._w, C.c_int(r))), C.c_int(mode))
            if rc != OK:
                raise GlfError(rc)

    def image_processing(self, img, opt=None, want_float=False):
        """Host image in, host image out (glf_multi_image_processing): (out u8 [H, W], zf f32 [H, W] or None, per-rank infos)."""
        return self._image_processing(PIX_U8, img, None, opt, want_float)

    def image_processing_signals(self, img, signals, opt=None):
        """glf_multi_image_processing_signals: the host image plus float planes [nsig, H, W] (numpy, replicated on every
        rank) filtered through the image's graph. Returns (out u8 [H, W], zf f32 [H, W], sig_out f32 [nsig, H, W], infos)."""
        return self._image_processing(PIX_U8, img, signals, opt, True)

    def image_processing_rgb(self, img, opt=None, want_float=False):
        """glf_multi_image_processing_rgb: host uint8 [H, W, 3] in, (out u8 [H, W, 3], zf f32 [3, H, W] or None, per-rank infos)."""
        return self._image_processing(PIX_RGB8, img, None, opt, want_float)

    def image_processing_u16(self, img, opt=None, want_float=False):
        """glf_multi_image_processing_u16: host uint16 [H, W] in, (out uint16 [H, W], zf f32 [H, W] or None, per-rank infos)."""
        return self._image_processing(PIX_U16, img, None, opt, want_float)

    def image_processing_rgb_signals(self, img, signals, opt=None, want_float=False):
        """glf_multi_image_processing_rgb_signals: host uint8 [H, W, 3] plus float planes [nsig, H, W] filtered through the colour
        graph. Returns (out u8 [H, W, 3], zf f32 [3, H, W] or None, sig_out f32 [nsig, H, W], infos)."""
        return self._image_processing(PIX_RGB8, img, signals, opt, want_float)

    def image_processing_u16_signals(self, img, signals, opt=None, want_float=False):
        """glf_multi_image_processing_u16_signals: host uint16 [H, W] plus float planes [nsig, H, W] filtered through the 16-bit
        graph. Returns (out uint16 [H, W], zf f32 [H, W] or None, sig_out f32 [nsig, H, W], infos)."""
        return self._image_processing(PIX_U16, img, signals, opt, want_float)

    def image_processing_f32(self, img, opt=None):
        """glf_multi_image_processing_f32: host float32 [H, W] in (finite values), (z float32 [H, W], per-rank infos)."""
        return self._image_processing(PIX_F32, img, None, opt, False)

    def image_processing_f32_signals(self, img, signals, opt=None):
        """glf_multi_image_processing_f32_signals: host float32 [H, W] plus float planes [nsig, H, W] filtered through the float
        image's graph. Returns (z float32 [H, W], sig_out f32 [nsig, H, W], infos)."""
        return self._image_processing(PIX_F32, img, signals, opt, False)

    def image_processing_rgbf32(self, img, opt=None):
        """glf_multi_image_processing_rgbf32: host float32 [H, W, 3] in (finite values), (z float32 [H, W, 3], per-rank infos)."""
        return self._image_processing(PIX_RGBF32, img, None, opt, False)

    def image_processing_rgbf32_signals(self, img, signals, opt=None):
        """glf_multi_image_processing_rgbf32_signals: host float32 [H, W, 3] plus float planes [nsig, H, W] filtered through the
        float colour graph. Returns (z float32 [H, W, 3], sig_out f32 [nsig, H, W], infos)."""
        return self._image_processing(PIX_RGBF32, img, signals, opt, False)

    def _image_processing(self, fmt, img, signals, opt, want_float):
        """Every image_processing* method: the host image of format fmt (a PIX_*) and, with signals, float planes [nsig, H, W]
        through glf_multi_image_processing<suffix>[_signals]. Returns (out, [zf or None,] [sig_out,] per-rank infos): zf is left
        out for the float formats, whose out is the float z."""
        f = _PIX_FORMATS[fmt]
        img = np.ascontiguousarray(img, dtype=f.np_dtype)
        if fmt != PIX_U8 and not _pix_shape_ok(f, img):   # (the 8-bit calls never checked: a wrong shape fails in the unpacking below)
            raise ValueError("image must be %s, got %s" % ("[H, W, 3]" if f.channels == 3 else "[H, W]", img.shape))
        h, w = img.shape[:2] if f.channels == 3 else img.shape
        fn, sig, sig_out = "glf_multi_image_processing" + f.suffix, (), ()
        if signals is not None:
            planes, planes_out = self._planes(signals, h, w)
            fn, sig, sig_out = fn + "_signals", (C.c_int(planes.shape[0]), _ptr(planes), _ptr(planes_out)), (planes_out,)
        opt = opt or default_options()
        out = np.zeros(img.shape, dtype=f.np_dtype)
        zf = np.zeros((3, h, w) if f.channels == 3 else (h, w), dtype=np.float32) if want_float and not f.float_out else None
        infos = self._run(fn, opt, img, out, zf, sig=sig, no_zf=f.float_out)
        return (out,) + (() if f.float_out else (zf,)) + sig_out + (infos,)

    def _run(self, fn, opt, img, out, zf, sig=(), no_zf=False):
        """glf_multi_<...>(world, opt, img, width, height, [nsig, planes, planes out,] out, zf, eigvals, stats): per-rank infos.
        no_zf: the float entry points, whose out is the float z (no zf argument)."""
        h, w = img.shape[:2]
        lam = np.zeros(max(1, _realised_samples(w, h, opt)), dtype=np.float64)
        stats = (Stats * self.n)()
        outs = (_ptr(out),) if no_zf else (_ptr(out), _ptr(zf))
        rc = getattr(_lib, fn)(self._w, C.byref(opt), _ptr(img), C.c_int(w), C.c_int(h), *sig, *outs, _ptr(lam), stats)
        if rc != OK:
            raise GlfError(rc, fn + ": " + _lib.glf_multi_last_error(self._w).decode())
        return [_info(s, lam) for s in stats]

    @staticmethod
    def _planes(signals, h, w):
        sig = np.ascontiguousarray(signals, dtype=np.float32)
        if sig.ndim != 3 or sig.shape[1:] != (h, w):
            raise ValueError("signals must be [nsig, %d, %d], got %s" % (h, w, sig.shape))
        return sig, np.zeros(sig.shape, dtype=np.float32)

    def comm_counters(self, rank=0, reset=True):
        """Collectives rank `rank` issued since the last reset: dict(allreduce_calls, allreduce_bytes, allgather_calls, allgather_bytes)."""
        return _comm_counters(C.c_void_p(_lib.glf_multi_ctx(self._w, C.c_int(rank))), reset)

    def comm_info(self, rank=0):
        return _comm_info(C.c_void_p(_lib.glf_multi_ctx(self._w, C.c_int(rank))))

    def set_tuning(self, **kw):
        for r in range(self.n):
            for k, v in kw.items():
                rc = _lib.glf_ctx_set_tuning(C.c_void_p(_lib.glf_multi_ctx(self._w, C.c_int(r))), k.encode(), None if v is None else str(v).encode())
                if rc != OK:
                    raise GlfError(rc, "set_tuning(%s=%r)" % (k, v))


def _comm_counters(ctx_ptr, reset=True):
    out = (C.c_ulonglong * 4)()
    rc = _lib.glf_ctx_comm_counters(ctx_ptr, out, C.c_int(1 if reset else 0))
    if rc != OK:
        raise GlfError(rc, "glf_ctx_comm_counters")
    return dict(allreduce_calls=int(out[0]), allreduce_bytes=int(out[1]), allgather_calls=int(out[2]), allgather_bytes=int(out[3]))


def _comm_info(ctx_ptr):
    info = (C.c_int * 4)()
    rc = _lib.glf_ctx_comm_info(ctx_ptr, info)
    if rc != OK:
        raise GlfError(rc, "glf_ctx_comm_info")
    return dict(rank=int(info[0]), size=int(info[1]), backend={0: "none", 1: "rccl", 2: "loopback"}.get(int(info[2]), "?"),
                rccl_ranks=int(info[3]))


# ---- device context --------------------------------------------------------------------

class Context:
    """One glf_ctx on one GPU. The library launches on a dedicated torch stream (self.stream); the
    collective callbacks run under that stream too, so RCCL / copies are ordered with the kernels.
    (torch's default stream has handle 0, which the C-ABI reads as "create your own stream" -- a
    private stream torch knows nothing about would race with the callbacks.)"""

    def __init__(self, device=0):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.Stream(device=self.device)
        assert self.stream.cuda_stream != 0
        self._ctx = C.c_void_p()
        rc = _lib.glf_ctx_create(C.byref(self._ctx), C.c_int(device), C.c_void_p(self.stream.cuda_stream))
        if rc != OK:
            raise GlfError(rc, "glf_ctx_create(device=%d)" % device)
        self._comm_keepalive = None

    def close(self):
        if self._ctx:
            _lib.glf_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what=""):
        if rc != OK:
            raise GlfError(rc, (what + " " if what else "") + _lib.glf_ctx_last_error(self._ctx).decode())

    def set_contraction(self, mode):
        """CONTRACT_F32_MFMA or CONTRACT_F16_SPLIT (see include/glf.h)."""
        self._check(_lib.glf_ctx_set_contraction(self._ctx, C.c_int(mode)))

    def synchronize(self):
        self._check(_lib.glf_ctx_synchronize(self._ctx))

    TUNING_KEYS = ("NYS_PATH", "DEG_PATH", "MV_PATH", "ROWPASS", "ROWPASS_OP", "SWEEP_COLPASS", "COLPASS", "NYS_NO_LUT", "NO_ECR", "NO_NARROW", "NO_FUSED_FILTER", "FILTER_FORM", "BAND_NOSKIP", "PIX_BAND", "EIG_SHARD", "ZMFMA_GROUPS", "GS", "RESIDUAL", "OPERAND_MAXIMA", "VERBOSE")

    def set_tuning(self, **kw):
        """glf_ctx_set_tuning: e.g. set_tuning(NYS_PATH="grid", MV_PATH="dense"); None / "" / "auto" = the default choice."""
        for k, v in kw.items():
            rc = _lib.glf_ctx_set_tuning(self._ctx, k.encode(), None if v is None else str(v).encode())
            if rc != OK:
                raise GlfError(rc, "set_tuning(%s=%r)" % (k, v))

    def reset_tuning(self):
        self.set_tuning(**{k: None for k in self.TUNING_KEYS})

    def debug_violations(self):
        """Guard zones of work buffers found overwritten (debug pool, GLF_POOL_DEBUG=1 at creation); -1 otherwise."""
        return int(_lib.glf_ctx_debug_violations(self._ctx))

    def cached_bytes(self):
        """Bytes of work buffers the context keeps cached and unused (glf_ctx_cached_bytes)."""
        return int(_lib.glf_ctx_cached_bytes(self._ctx))

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, mem = C.c_int(), C.c_size_t()
        self._check(_lib.glf_ctx_device_info(self._ctx, name, C.c_size_t(256), C.byref(cus), C.byref(mem)))
        return dict(name=name.value.decode(), num_cus=cus.value, total_mem=mem.value)

    # -- collectives ---------------------------------------------------------------------------
    def set_comm_rccl(self, rank, size, unique_id, force=False):
        """The library's own RCCL collectives on this context's stream (glf_ctx_set_comm_rccl: ncclCommInitRank, collective
        over all `size` ranks). unique_id: the bytes of rccl_unique_id() from one rank."""
        buf = C.create_string_buffer(bytes(unique_id), RCCL_ID_BYTES)
        self._comm_keepalive = None
        self._native_rank = (rank, size)
        self._check(_lib.glf_ctx_set_comm_rccl(self._ctx, C.c_int(rank), C.c_int(size), buf, C.c_size_t(RCCL_ID_BYTES),
                                               C.c_int(1 if force else 0)), "set_comm_rccl")

    # -- the PoC's balancing steps ------------------------------------------------
    def Sinkhorn(self, phi, Pi, iterations=100, rows=None):
        """sinkhorn(phi, Pi), python/image_processing.py:90-107. phi: dense N x m Mat, Pi: diagonal Mat. Returns (r, c) as numpy
        f64 [N]; with rows = n also W_AB[:n] = diag(r) K diag(c) rows as numpy [n, N] (the PoC's [W_A W_B] for n = m)."""
        torch = self.torch
        N = int(phi.rows)
        r = torch.empty(N, dtype=torch.float64, device=self.device)
        c = torch.empty(N, dtype=torch.float64, device=self.device)
        self._check(_lib.glf_Sinkhorn(self._ctx, C.byref(phi), C.byref(Pi), C.c_int(iterations), C.c_void_p(r.data_ptr()),
                                      C.c_void_p(c.data_ptr())), "Sinkhorn")
        if rows is None:
            return r.cpu().numpy(), c.cpu().numpy()
        out = torch.empty((rows, N), dtype=torch.float64, device=self.device)
        self._check(_lib.glf_SinkhornRows(self._ctx, C.byref(phi), C.byref(Pi), C.c_void_p(r.data_ptr()), C.c_void_p(c.data_ptr()),
                                          C.c_int64(0), C.c_int(rows), C.c_void_p(out.data_ptr())), "SinkhornRows")
        return r.cpu().numpy(), c.cpu().numpy(), out.cpu().numpy()

    def Orthogonalisation(self, A, B):
        """orthogonalisation(A, B), python/image_processing.py:110-127. A: numpy n x n, B: numpy n x q -> (V [(n + q), n], Pi [n])."""
        torch = self.torch
        A = np.ascontiguousarray(A, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        n, q = A.shape[0], B.shape[1]
        dA, dB = torch.from_numpy(A).to(self.device), torch.from_numpy(B).to(self.device)
        dV = torch.empty((n + q, n), dtype=torch.float64, device=self.device)
        Pi = np.zeros(n, dtype=np.float64)
        self._check(_lib.glf_Orthogonalisation(self._ctx, C.c_void_p(dA.data_ptr()), C.c_int(n), C.c_void_p(dB.data_ptr()), C.c_int(q),
                                               C.c_void_p(dV.data_ptr()), Pi.ctypes.data_as(C.c_void_p)), "Orthogonalisation")
        return dV.cpu().numpy(), Pi

    def comm_info(self):
        """What the context's communicator reports: dict(rank, size, backend, rccl_ranks = ncclCommCount)."""
        return _comm_info(self._ctx)

    def comm_counters(self, reset=True):
        """Collectives this rank issued through the library's own communicator since the last reset."""
        return _comm_counters(self._ctx, reset)

    def set_comm_torch(self, group=None, shard_eigensolve=True, force=False):
        """Plug torch.distributed all-reduces into glf_comm: RCCL on the device buffers in place
        (backend "nccl"), or staged through host memory for a gloo group (CPU rehearsal of the
        N > 1 path, several ranks sharing one GPU in tests)."""
        import torch.distributed as dist
        torch = self.torch
        size, rank = dist.get_world_size(group), dist.get_rank(group)
        if size == 1 and not force:   # force: keep the callbacks on a one-rank group (tests the device collectives)
            self._check(_lib.glf_ctx_set_comm(self._ctx, None))
            return
        dev = self.device
        on_device = dist.get_backend(group) == "nccl"

        stream = self.stream

        def allreduce(ptr, count, is_f64):
            with torch.cuda.stream(stream):   # ordered after the library's kernels, before its next ones
                t = device_tensor_from_ptr(ptr, count, torch.float64 if is_f64 else torch.float32, dev)
                if on_device:
                    dist.all_reduce(t, group=group)
                else:
                    h = t.cpu()
                    dist.all_reduce(h, group=group)
                    t.copy_(h)
                    stream.synchronize()      # h is pageable host memory

        def allgather(ptr, count_per_rank):
            with torch.cuda.stream(stream):
                full = device_tensor_from_ptr(ptr, count_per_rank * size, torch.float32, dev)
                mine = full[rank * count_per_rank:(rank + 1) * count_per_rank]
                if on_device:
                    dist.all_gather_into_tensor(full, mine.clone(), group=group)
                else:
                    parts = [torch.empty(count_per_rank, dtype=torch.float32) for _ in range(size)]
                    dist.all_gather(parts, mine.cpu(), group=group)
                    full.copy_(torch.cat(parts))
                    stream.synchronize()

        self._comm_keepalive = make_comm(rank, size, allreduce, allgather if shard_eigensolve else None)
        self._check(_lib.glf_ctx_set_comm(self._ctx, C.byref(self._comm_keepalive)))

    # -- helpers ---------------------------------------------------------------------------
    def to_device(self, img):
        with self.torch.cuda.stream(self.stream):
            t = self.torch.from_numpy(np.ascontiguousarray(img, dtype=np.uint8)).to(self.device)
        self.stream.synchronize()
        return t

    def mat_to_numpy(self, mat, padded=False):
        """Dense / diagonal glf_mat -> numpy (rows x cols), padding stripped; padded: a dense one as stored (rows x ld)."""
        if mat.kind == MAT_DIAG:
            out = np.empty(mat.rows, dtype=np.float32)
            self._check(_lib.glf_memcpy_d2h(self._ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(mat.data),
                                            C.c_size_t(out.nbytes)))
            return out
        assert mat.kind == MAT_DENSE
        full = np.empty((mat.rows, mat.ld), dtype=np.float32)
        self._check(_lib.glf_memcpy_d2h(self._ctx, full.ctypes.data_as(C.c_void_p), C.c_void_p(mat.data),
                                        C.c_size_t(full.nbytes)))
        return full if padded else full[:, :mat.cols].copy()

    def degree_of(self, K_B):
        out = np.empty(K_B.p, dtype=np.float64)
        self._check(_lib.glf_memcpy_d2h(self._ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(K_B.degree),
                                        C.c_size_t(out.nbytes)))
        return out

    def dense_from_numpy(self, arr, ld=None, row_order=ROWS_NA):
        """numpy (rows x cols) -> dense glf_mat with ld rounded up to a power of two >= 32."""
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        rows, cols = arr.shape
        if ld is None:
            ld = 32
            while ld < min(cols, 256):
                ld *= 2
            if cols > 256:
                ld = (cols + 255) // 256 * 256     # more than 256 vectors: a multiple of 256 (panels)
        mat = Mat()
        self._check(_lib.glf_mat_create_dense(self._ctx, C.byref(mat), C.c_int64(rows), C.c_int64(cols), C.c_int64(ld)))
        full = np.zeros((rows, ld), dtype=np.float32)
        full[:, :cols] = arr
        self._check(_lib.glf_memcpy_h2d(self._ctx, C.c_void_p(mat.data), full.ctypes.data_as(C.c_void_p),
                                        C.c_size_t(full.nbytes)))
        mat.row_order = row_order
        return mat

    def diag_from_numpy(self, vec):
        vec = np.ascontiguousarray(vec, dtype=np.float32)
        mat = Mat()
        self._check(_lib.glf_mat_create_diag(self._ctx, C.byref(mat), C.c_int64(vec.size)))
        self._check(_lib.glf_memcpy_h2d(self._ctx, C.c_void_p(mat.data), vec.ctypes.data_as(C.c_void_p),
                                        C.c_size_t(vec.nbytes)))
        return mat

    def destroy(self, *mats):
        for m in mats:
            _lib.glf_mat_destroy(self._ctx, C.byref(m))

    # -- stages (names as in hpc/*.h) -------------------------------------------------------
    def ComputeAffinityMatrices(self, d_img, sample_indices, want_KA=True, kernel=KERNEL_BILATERAL,
                                h_loc=40.0, h_val=30.0):
        # (KERNEL_BILATERAL_RGB: d_img is [H, W, 3]; KERNEL_BILATERAL_U16: uint16 [H, W]; KERNEL_BILATERAL_F32: float32 [H, W];
        # KERNEL_BILATERAL_RGBF32: float32 [H, W, 3])
        dtype = {KERNEL_BILATERAL_U16: self.torch.uint16, KERNEL_BILATERAL_F32: self.torch.float32,
                 KERNEL_BILATERAL_RGBF32: self.torch.float32}.get(kernel, self.torch.uint8)
        colour = kernel in (KERNEL_BILATERAL_RGB, KERNEL_BILATERAL_RGBF32)
        assert d_img.dtype == dtype and d_img.is_cuda and d_img.is_contiguous()
        assert d_img.dim() == (3 if colour else 2) and (not colour or d_img.shape[2] == 3)
        h, w = d_img.shape[:2]
        idx = np.ascontiguousarray(sample_indices, dtype=np.uint32)
        K_A, K_B = Mat(), Mat()
        self._check(_lib.glf_ComputeAffinityMatrices(
            self._ctx, C.byref(K_A) if want_KA else None, C.byref(K_B), C.c_void_p(d_img.data_ptr()), C.c_int(w),
            C.c_int(h), C.c_uint(idx.size), idx.ctypes.data_as(C.c_void_p), C.c_int(kernel), C.c_float(h_loc),
            C.c_float(h_val)), "ComputeAffinityMatrices")
        K_B._img_keepalive = d_img
        return (K_A if want_KA else None), K_B

    def ComputeLaplacianMatrix(self, K_A, K_B):
        L_A, L_B = Mat(), Mat()
        alpha = C.c_double()
        self._check(_lib.glf_ComputeLaplacianMatrix(self._ctx, C.byref(L_A), C.byref(L_B),
                                                    C.byref(K_A) if K_A is not None else None, C.byref(K_B),
                                                    C.byref(alpha)), "ComputeLaplacianMatrix")
        return L_A, L_B, alpha.value

    def InversePowerIteration(self, A, m, optiGramSchmidt=1, epsilon=0.1, inner_rtol=1e-5, max_outer=100000,
                              X0=None, allow_noconv=False):
        vecs, vals = Mat(), Mat()
        st = EigStats()
        x0p = None
        if X0 is not None:
            X0 = np.ascontiguousarray(X0, dtype=np.float64)
            assert X0.shape == (m, A.rows)
            x0p = X0.ctypes.data_as(C.c_void_p)
        rc = _lib.glf_InversePowerIteration(self._ctx, C.byref(A), C.c_uint(m), C.byref(vecs), C.byref(vals),
                                            C.c_int(optiGramSchmidt), C.c_double(epsilon), C.c_double(inner_rtol),
                                            C.c_int(max_outer), x0p, C.byref(st))
        if not (allow_noconv and rc == ERR_NOCONV):
            self._check(rc, "InversePowerIteration")
        return vecs, vals, dict(outer_its=st.outer_its, inner_its_total=st.inner_its_total, residual=st.residual)

    def OrthonormaliseVecs(self, X):
        norms = np.empty(X.cols, dtype=np.float64)
        self._check(_lib.glf_OrthonormaliseVecs(self._ctx, C.byref(X), norms.ctypes.data_as(C.c_void_p)))
        return norms

    def NormaliseVecs(self, X):
        norms = np.empty(X.cols, dtype=np.float64)
        self._check(_lib.glf_NormaliseVecs(self._ctx, C.byref(X), norms.ctypes.data_as(C.c_void_p)))
        return norms

    def operator(self, L_B, skip_exact_zeros=0, rows=None, ld_hint=256):
        """glf_operator_create: the eigen-solve's L_A = alpha (D - K_A) of the descriptor L_B (ComputeLaplacianMatrix's) in the form the
        whole path would take under the context's contraction mode and tuning. rows = (row0, row1): the rows one rank of the
        sharded solve owns (None: all). Returns an Operator (apply, apply_numpy, stored, info, close); L_B must outlive it."""
        p = int(L_B.p)
        row0, row1 = (0, p) if rows is None else rows
        h = C.c_void_p()
        self._check(_lib.glf_operator_create(self._ctx, C.byref(L_B), C.c_int(skip_exact_zeros), C.c_uint(row0), C.c_uint(row1),
                                             C.c_uint(ld_hint), C.byref(h)), "operator")
        return Operator(self, h, p, L_B)

    def InverseDiagMat(self, x):
        inv = Mat()
        self._check(_lib.glf_InverseDiagMat(self._ctx, C.byref(x), C.byref(inv)))
        return inv

    def Nystroem(self, B, phi_A, Pi_A_Inv):
        phi = Mat()
        self._check(_lib.glf_Nystroem(self._ctx, C.byref(B), C.byref(phi_A), C.byref(Pi_A_Inv), C.byref(phi)), "Nystroem")
        return phi

    def Nystroem_ex(self, B, phi_A, Pi_A_Inv, skip_exact_zeros=0, rows=None, phi=None):
        """glf_Nystroem_ex: the Nystroem stage with the contraction's window, a range of image rows (rows = (row0, row1); None: all)
        and, with phi, an existing sample-first N x m matrix written in place. Returns (phi, info), info a dict of glf_nystroem_info."""
        row0, row1 = (0, 0) if rows is None else rows
        out = Mat() if phi is None else phi
        info = NystroemInfo()
        self._check(_lib.glf_Nystroem_ex(self._ctx, C.byref(B), C.byref(phi_A), C.byref(Pi_A_Inv), C.c_int(skip_exact_zeros), C.c_uint(row0),
                                         C.c_uint(row1), C.byref(out), C.byref(info)), "Nystroem_ex")
        return out, {k: getattr(info, k) for k, _ in NystroemInfo._fields_}

    def Degree_ex(self, d_img, sample_indices, kernel=KERNEL_BILATERAL, h_loc=40.0, h_val=30.0, skip_exact_zeros=0, rows=None,
                  plane=None, want_ysum=False, out=None):
        """glf_Degree_ex: the degree stage over the image rows `rows` = (row0, row1) (None: all) with the whole path's knobs. d_img: the
        guide as a device tensor in the kernel's format; plane: a device float32 [H, W] tensor -- the result is then the weighted sums
        U_s. out = (degree, ysum or None): host float64 [p] arrays to write into (default: new ones). Returns (degree, ysum or None,
        info dict of glf_degree_info); a refusal raises GlfError and leaves `out` untouched."""
        h, w = d_img.shape[:2]
        idx = np.ascontiguousarray(sample_indices, dtype=np.uint32)
        row0, row1 = (0, 0) if rows is None else rows
        deg, ysum = out if out is not None else (np.empty(idx.size, dtype=np.float64), np.empty(idx.size, dtype=np.float64) if want_ysum else None)
        assert deg.dtype == np.float64 and deg.size == idx.size and deg.flags.c_contiguous
        assert ysum is None or (ysum.dtype == np.float64 and ysum.size == idx.size and ysum.flags.c_contiguous)
        assert plane is None or (plane.dtype == self.torch.float32 and plane.is_cuda and plane.is_contiguous() and tuple(plane.shape) == (h, w))
        info = DegreeInfo(struct_size=C.sizeof(DegreeInfo))
        self._check(_lib.glf_Degree_ex(self._ctx, C.c_void_p(d_img.data_ptr()), C.c_int(w), C.c_int(h), C.c_uint(idx.size),
                                       idx.ctypes.data_as(C.c_void_p), C.c_int(kernel), C.c_float(h_loc), C.c_float(h_val),
                                       C.c_int(skip_exact_zeros), C.c_uint(row0), C.c_uint(row1),
                                       C.c_void_p(plane.data_ptr()) if plane is not None else None, deg.ctypes.data_as(C.c_void_p),
                                       ysum.ctypes.data_as(C.c_void_p) if ysum is not None else None, C.byref(info)), "Degree_ex")
        return deg, ysum, {k: getattr(info, k) for k, _ in DegreeInfo._fields_}

    def Filter_ex(self, pix, d_img, phi, lam, filter_mode=FILTER_REFERENCE, filter_pow=1, filter_beta=1.5, gain=3.0, rows=None, sig=None,
                  sig_out=None, c_in=None, c_out=None, gram_out=None, out=None, zf=None, corr=None):
        """glf_Filter_ex: the filter stage on the dense raster-order glf_mat phi. d_img: the guide as a device tensor in the format
        pix ([H, W] or [H, W, 3]); lam: host float64 [m]; rows = (row0, row1) (None: all); sig / sig_out: device float32 [nsig, H, W]
        planes in and out; c_in / c_out: host float64 [channels + nsig, m]; gram_out: host float64 [m, m]; out (required), zf, corr:
        device tensors the call writes into. Returns the info dict of glf_filter_info; a refusal raises GlfError and leaves every
        output untouched."""
        h, w = d_img.shape[:2]
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        row0, row1 = (0, 0) if rows is None else rows
        for a in (c_in, c_out, gram_out):
            assert a is None or (a.dtype == np.float64 and a.flags.c_contiguous)
        for t in (sig, sig_out, zf, corr):
            assert t is None or (t.dtype == self.torch.float32 and t.is_cuda and t.is_contiguous())
        assert out.is_cuda and out.is_contiguous() and d_img.is_cuda and d_img.is_contiguous()
        host = lambda a: a.ctypes.data if a is not None else None
        dev = lambda t: t.data_ptr() if t is not None else None
        rq = FilterRequest(struct_size=C.sizeof(FilterRequest), pix=pix, d_img=d_img.data_ptr(), width=w, height=h, phi=C.addressof(phi),
                           lam=lam.ctypes.data, filter_mode=filter_mode, filter_pow=filter_pow, filter_beta=filter_beta, gain=gain, row0=row0,
                           row1=row1, nsig=0 if sig is None else sig.shape[0], d_sig=dev(sig), d_sig_out=dev(sig_out), h_c_in=host(c_in),
                           h_c_out=host(c_out), h_gram_out=host(gram_out), d_out=out.data_ptr(), d_zf=dev(zf), d_corr=dev(corr))
        info = FilterInfo(struct_size=C.sizeof(FilterInfo))
        self._check(_lib.glf_Filter_ex(self._ctx, C.byref(rq), C.byref(info)), "Filter_ex")
        self.stream.synchronize()
        return {k: int(getattr(info, k)) for k, _ in FilterInfo._fields_}

    def Permutation(self, mat, sample_indices):
        idx = np.ascontiguousarray(sample_indices, dtype=np.uint32)
        out = Mat()
        self._check(_lib.glf_Permutation(self._ctx, C.byref(mat), idx.ctypes.data_as(C.c_void_p), C.c_uint(idx.size),
                                         C.byref(out)), "Permutation")
        return out

    def ComputeResultFromLaplacian(self, d_img, phi, Pi, gain=3.0, want_float=True):
        torch = self.torch
        h, w = d_img.shape
        with torch.cuda.stream(self.stream):
            out = torch.empty((h, w), dtype=torch.uint8, device=self.device)
            zf = torch.empty((h, w), dtype=torch.float32, device=self.device) if want_float else None
        self._check(_lib.glf_ComputeResultFromLaplacian(
            self._ctx, C.c_void_p(d_img.data_ptr()), C.byref(phi), C.byref(Pi), C.c_uint(w), C.c_uint(h),
            C.c_float(gain), C.c_void_p(out.data_ptr()), C.c_void_p(zf.data_ptr()) if want_float else None),
            "ComputeResultFromLaplacian")
        self.stream.synchronize()
        return out, zf

    def EntireComputation(self, d_img, kernel=KERNEL_BILATERAL, h_loc=40.0, h_val=30.0):
        """-no_approx mode (hpc/image_processing.c:155-181): z = clamp(y - L y), full N x N Laplacian."""
        torch = self.torch
        h, w = d_img.shape
        with torch.cuda.stream(self.stream):
            out = torch.empty((h, w), dtype=torch.uint8, device=self.device)
            zf = torch.empty((h, w), dtype=torch.float32, device=self.device)
        alpha = C.c_double()
        self._check(_lib.glf_EntireComputation(self._ctx, C.c_void_p(d_img.data_ptr()), C.c_int(w), C.c_int(h),
                                               C.c_int(kernel), C.c_float(h_loc), C.c_float(h_val),
                                               C.c_void_p(out.data_ptr()), C.c_void_p(zf.data_ptr()), C.byref(alpha)),
                    "EntireComputation")
        self.stream.synchronize()
        return out, zf, alpha.value

    def image_processing(self, d_img, opt=None, want_float=False, out=None, capture=False):
        """Whole approximate path (hpc/image_processing.c:183-277) on a device image tensor.
        capture=True additionally returns the run's by-products in info["capture"] (glf_capture): phi_A [p, ld] and
        phi [rows of this rank * width, ld] as device tensors, c = Phi^T y and the degree vector as numpy arrays."""
        return self._image_processing(PIX_U8, d_img, None, opt, want_float, capture, out)

    def image_processing_signals(self, d_img, signals, opt=None, want_float=False):
        """Joint filtering (glf_image_processing_signals): the guide d_img (device uint8 [H, W]) defines the graph, the
        eigenpairs and the filter; `signals` (device float32 [nsig, H, W], 1 <= nsig <= 4) go through the same operator.
        Returns (out, zf or None, sig_out float32 [nsig, H, W], info); out / zf / info are those of image_processing."""
        return self._image_processing(PIX_U8, d_img, signals, opt, want_float, False, None)

    def image_processing_rgb(self, d_rgb, opt=None, want_float=False, capture=False):
        """Colour-guided filtering (glf_image_processing_rgb): d_rgb (device uint8 [H, W, 3]) defines the graph through its RGB
        differences, and each channel goes through the graph's filter. Returns (out uint8 [H, W, 3], zf float32 [3, H, W] or None,
        info). capture=True (glf_image_processing_rgb_capture) adds info["capture"]: phi_A [p, ld] and phi [rows of this rank *
        width, ld] as device tensors, the degree vector as a numpy array."""
        return self._image_processing(PIX_RGB8, d_rgb, None, opt, want_float, capture, None)

    def image_processing_u16(self, d_img, opt=None, want_float=False, capture=False):
        """16-bit greyscale filtering (glf_image_processing_u16): d_img (device uint16 [H, W]) defines the graph through its 16-bit
        values (opt.h_val in 16-bit units) and goes through the graph's filter. Returns (out uint16 [H, W], zf float32 [H, W] or None,
        info). capture=True (glf_image_processing_u16_capture) adds info["capture"] as image_processing_rgb does."""
        return self._image_processing(PIX_U16, d_img, None, opt, want_float, capture, None)

    def image_processing_f32(self, d_img, opt=None, capture=False, out=None):
        """32-bit float greyscale filtering (glf_image_processing_f32): d_img (device float32 [H, W], finite values) defines the graph
        through its values (opt.h_val in the image's units) and goes through the graph's filter. Returns (z float32 [H, W], info):
        the output is the float z itself, not clamped. A NaN or an Inf in d_img raises GlfError(ERR_INVALID) and `out` (optional: a
        device float32 [H, W] to write into) is left as it was. capture=True adds info["capture"] as image_processing_u16 does."""
        return self._image_processing(PIX_F32, d_img, None, opt, False, capture, out)

    def image_processing_f32_signals(self, d_img, signals, opt=None):
        """Joint filtering under a float guide (glf_image_processing_f32_signals): as image_processing_u16_signals with the graph
        and the output of image_processing_f32. Returns (z float32 [H, W], sig_out float32 [nsig, H, W], info)."""
        return self._image_processing(PIX_F32, d_img, signals, opt, False, False, None)

    def image_processing_rgbf32(self, d_rgb, opt=None, capture=False, out=None):
        """Float colour filtering (glf_image_processing_rgbf32): d_rgb (device float32 [H, W, 3], finite values: HDR, [0, 1] RGB,
        Lab / YUV, a network's output) defines the graph through the differences of its three channels (opt.h_val in the image's units)
        and each channel goes through the graph's filter. Returns (z float32 [H, W, 3], info): the output is the float z itself,
        interleaved as the image, not clamped. A NaN or an Inf in d_rgb raises GlfError(ERR_INVALID) and `out` (optional: a device
        float32 [H, W, 3] to write into) is left as it was. capture=True adds info["capture"] as image_processing_rgb does."""
        return self._image_processing(PIX_RGBF32, d_rgb, None, opt, False, capture, out)

    def image_processing_rgbf32_signals(self, d_rgb, signals, opt=None):
        """Joint filtering under a float colour guide (glf_image_processing_rgbf32_signals): as image_processing_rgb_signals with the
        graph and the output of image_processing_rgbf32. Returns (z float32 [H, W, 3], sig_out float32 [nsig, H, W], info)."""
        return self._image_processing(PIX_RGBF32, d_rgb, signals, opt, False, False, None)

    def image_processing_rgb_signals(self, d_rgb, signals, opt=None, want_float=False):
        """Joint filtering under a colour guide (glf_image_processing_rgb_signals): d_rgb (device uint8 [H, W, 3]) defines the graph
        and is filtered as by image_processing_rgb; `signals` (device float32 [nsig, H, W], 1 <= nsig <= 4) go through the same
        operator. Returns (out, zf or None, sig_out float32 [nsig, H, W], info); out / zf / info are those of image_processing_rgb."""
        return self._image_processing(PIX_RGB8, d_rgb, signals, opt, want_float, False, None)

    def image_processing_u16_signals(self, d_img, signals, opt=None, want_float=False):
        """Joint filtering under a 16-bit guide (glf_image_processing_u16_signals): as image_processing_rgb_signals with the graph
        and the outputs of image_processing_u16 (d_img device uint16 [H, W])."""
        return self._image_processing(PIX_U16, d_img, signals, opt, want_float, False, None)

    def _image_processing(self, fmt, d_img, signals, opt, want_float, capture, out):
        """Every image_processing* method: the device image of format fmt (a PIX_*) and, with signals, device float planes
        [nsig, H, W] through glf_image_processing<suffix>_capture or <suffix>_signals on the context's stream. Returns (out,
        [zf or None,] [sig_out,] info): zf is left out for the float formats, whose out is the float z."""
        torch = self.torch
        f = _PIX_FORMATS[fmt]
        dtype = getattr(torch, f.torch_dtype)
        assert d_img.dtype == dtype and d_img.is_cuda and _pix_shape_ok(f, d_img) and d_img.is_contiguous()
        h, w = d_img.shape[:2]
        opt = opt or default_options()
        what, sig, sig_out = "image_processing" + f.suffix, (), ()
        if signals is not None:
            planes_out, sig = self._signal_planes(signals, h, w)   # (waits for the caller's stream)
            what, sig_out = what + "_signals", (planes_out,)
        elif f.wait_stream:
            self.stream.wait_stream(torch.cuda.current_stream(self.device))   # the image is complete before the library reads it
        with torch.cuda.stream(self.stream):   # the zero fills must be ordered before the library's writes
            if out is None:
                out = torch.zeros(tuple(d_img.shape), dtype=getattr(torch, f.zeros_dtype), device=self.device)
                if f.zeros_dtype != f.torch_dtype:
                    out = out.view(dtype)
            zf = torch.zeros((3, h, w) if f.channels == 3 else (h, w), dtype=torch.float32,
                             device=self.device) if want_float and not f.float_out else None
        if f.float_out:   # (out= of the float calls; the 8-bit call takes its out as it comes)
            assert out.dtype == dtype and out.is_cuda and tuple(out.shape) == tuple(d_img.shape) and out.is_contiguous()
        info = self._run("glf_" + what + ("" if sig else "_capture"), what, opt, d_img, out, zf, capture, grey=fmt == PIX_U8, sig=sig,
                         no_zf=f.float_out)
        return (out,) + (() if f.float_out else (zf,)) + sig_out + (info,)

    def _run(self, fn, what, opt, d_img, out, zf, capture=False, grey=False, sig=(), no_zf=False):
        """fn(ctx, opt, img, width, height, [*sig,] out, zf, eigvals, stats[, capture]) on the context's stream (sig: nsig, the
        planes and the planes out of the signals entry point, which takes no capture): the call's info dict, with info["capture"]
        when asked for (grey: also c = Phi^T y and the correction). Errors are reported as `what`. no_zf: the float entry points,
        whose out is the float z (no zf argument)."""
        h, w = d_img.shape[:2]
        p_real = _realised_samples(w, h, opt)
        lam = np.zeros(max(p_real, 1), dtype=np.float64)       # m <= p - 1 eigenvalues come back
        cap, keep = self._capture_buffers(w, h, opt, p_real, grey) if capture else (None, None)
        st = Stats()
        zfs = () if no_zf else (C.c_void_p(zf.data_ptr()) if zf is not None else None,)
        args = (C.c_void_p(d_img.data_ptr()), C.c_int(w), C.c_int(h)) + sig + (C.c_void_p(out.data_ptr()),) + zfs + (_ptr(lam), C.byref(st))
        if not sig:
            args += (C.byref(cap) if cap else None,)
        self._check(getattr(_lib, fn)(self._ctx, C.byref(opt), *args), what)
        self.stream.synchronize()
        info = _info(st, lam)
        if capture:
            phi_A, phi, deg_host, c_host, corr = keep
            assert cap.ld == phi_A.shape[1], (cap.ld, phi_A.shape)
            info["capture"] = dict(phi_A=phi_A[:st.p], phi=phi, degree=deg_host[:st.p].copy(), ld=int(cap.ld))
            if grey:
                info["capture"].update(c=c_host[:st.m].copy(), corr=corr)
        return info

    def _signal_planes(self, signals, h, w):
        """The zero-filled result planes and the (nsig, planes, planes out) arguments of a signals entry point."""
        torch = self.torch
        assert signals.dtype == torch.float32 and signals.is_cuda and signals.dim() == 3 and signals.is_contiguous()
        if tuple(signals.shape[1:]) != (h, w):
            raise ValueError("signals must be [nsig, %d, %d], got %s" % (h, w, tuple(signals.shape)))
        self.stream.wait_stream(torch.cuda.current_stream(self.device))   # the image and the planes are complete before the library reads them
        with torch.cuda.stream(self.stream):
            sig_out = torch.zeros(tuple(signals.shape), dtype=torch.float32, device=self.device)
        return sig_out, (C.c_int(signals.shape[0]), C.c_void_p(signals.data_ptr()), C.c_void_p(sig_out.data_ptr()))

    def graph(self, d_img, opt=None):
        """glf_graph_build: the graph handle of a device image -- uint8 [H, W], uint8 [H, W, 3], uint16 [H, W], float32 [H, W] or
        float32 [H, W, 3] -- as a Graph: the eigenbasis is built once (the format's capture call), then Graph.project /
        Graph.synthesize / Graph.apply run any number of spectral responses on any planes in two passes over Phi each."""
        torch = self.torch
        assert d_img.is_cuda and d_img.is_contiguous()
        pix = next((k for k, f in _PIX_FORMATS.items() if d_img.dtype == getattr(torch, f.torch_dtype) and _pix_shape_ok(f, d_img)), None)
        if pix is None:
            raise ValueError("graph: no pixel format for dtype %s, shape %s" % (d_img.dtype, tuple(d_img.shape)))
        h, w = d_img.shape[:2]
        opt = opt or default_options()
        self.stream.wait_stream(torch.cuda.current_stream(self.device))   # the image is complete before the library reads it
        handle, st = C.c_void_p(), Stats()
        self._check(_lib.glf_graph_build(self._ctx, C.byref(opt), C.c_int(pix), C.c_void_p(d_img.data_ptr()), C.c_int(w), C.c_int(h),
                                         C.byref(handle), C.byref(st)), "graph")
        return Graph(self, handle, st)

    def _capture_buffers(self, w, h, opt, p_real, grey=False):
        """glf_capture with phi_A, phi (this rank's rows) and the degree vector -- grey: also c = Phi^T y and the correction -- and
        the buffers it points to. The realised sample count and the row stride are known before the call."""
        torch = self.torch
        m_req = int(opt.num_eigvals) if 0 < opt.num_eigvals < p_real else max(1, p_real - 1)
        ld = 32
        while ld < min(m_req, 256):
            ld *= 2
        if self._comm_keepalive:
            rows = shard_rows(h, self._comm_keepalive.rank, self._comm_keepalive.size)
        elif getattr(self, "_native_rank", None):
            rows = shard_rows(h, *self._native_rank)
        else:
            rows = (0, h)
        npix = (rows[1] - rows[0]) * w
        with torch.cuda.stream(self.stream):
            phi_A = torch.zeros(((p_real + 63) // 64 * 64, ld), dtype=torch.float32, device=self.device)
            phi = torch.zeros((npix, ld), dtype=torch.float32, device=self.device)
            corr = torch.zeros(npix, dtype=torch.float32, device=self.device) if grey else None
        deg_host = np.zeros(p_real, dtype=np.float64)
        c_host = np.zeros(ld, dtype=np.float64) if grey else None
        cap = Capture(C.sizeof(Capture), 0, phi_A.data_ptr(), phi_A.numel(), phi.data_ptr(), phi.numel(),
                      c_host.ctypes.data if grey else None, deg_host.ctypes.data, corr.data_ptr() if grey else None,
                      corr.numel() if grey else 0)
        return cap, (phi_A, phi, deg_host, c_host, corr)


class Operator:
    """One glf_operator: a sweep Y = L_A X through the function the eigen-solve calls (Context.operator)."""

    def __init__(self, ctx, handle, p, desc):
        self.ctx, self._h, self.p, self._desc = ctx, handle, p, desc
        self.info = None          # dict of the last apply: path, ksplit, skipping, row0, row1

    def close(self):
        if self._h:
            _lib.glf_operator_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def apply(self, X, Y):
        """glf_operator_apply on two dense Mats of one ld -> the info dict (also kept in self.info)."""
        info = OperatorInfo()
        self.ctx._check(_lib.glf_operator_apply(self._h, C.byref(X), C.byref(Y), C.byref(info)), "operator.apply")
        self.info = {k: int(getattr(info, k)) for k, _ in OperatorInfo._fields_}
        return self.info

    def apply_numpy(self, X, fill=None):
        """X: float32 [rows >= p, ld] (the whole block, padding columns included) -> Y float32 [round_up(p, 64), ld]. The device
        blocks hold round_up(p, 64) rows, X zero from its last row on; Y starts as zeros, or as the float32 array `fill`
        [round_up(p, 64), ld] (a sentinel: rows the operator does not own, and every row after a refusal, keep it)."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        rows, ld = (self.p + 63) // 64 * 64, X.shape[1]
        if X.shape[0] > rows:
            raise ValueError("X has %d rows, more than round_up(p, 64) = %d" % (X.shape[0], rows))
        ctx = self.ctx
        full = np.zeros((rows, ld), dtype=np.float32)
        full[:X.shape[0]] = X
        y0 = np.zeros((rows, ld), dtype=np.float32) if fill is None else np.ascontiguousarray(fill, dtype=np.float32)
        assert y0.shape == (rows, ld)
        dX, dY = ctx.dense_from_numpy(full, ld=ld), ctx.dense_from_numpy(y0, ld=ld)
        dX.rows = dY.rows = max(X.shape[0], 1) if X.shape[0] < self.p else self.p
        out = np.empty((rows, ld), dtype=np.float32)
        try:
            try:
                self.apply(dX, dY)
            finally:
                ctx._check(_lib.glf_memcpy_d2h(ctx._ctx, _ptr(out), C.c_void_p(dY.data), C.c_size_t(out.nbytes)))
                self.last_Y = out
        finally:
            ctx.destroy(dX, dY)
        return out

    def solve(self, B, X, R, m, rtol=1e-5, max_it=1000, allow_noconv=False):
        """glf_operator_solve on dense Mats of one ld (R: a Mat or None) -> the info dict (iters, unconverged, matvecs, narrow_sweeps,
        path, reserved, and status: OK, or ERR_NOCONV where allow_noconv let a cut solve pass); also kept in self.solve_info."""
        info = SolveInfo()
        rc = _lib.glf_operator_solve(self._h, C.byref(B), C.byref(X), C.byref(R) if R is not None else None, C.c_uint(m), C.c_double(rtol),
                                     C.c_int(max_it), C.byref(info))
        if not (allow_noconv and rc == ERR_NOCONV):
            self.ctx._check(rc, "operator.solve")
        self.solve_info = {k: int(getattr(info, k)) for k, _ in SolveInfo._fields_}
        self.solve_info["status"] = rc
        return self.solve_info

    def solve_numpy(self, B, m, rtol=1e-5, max_it=1000, allow_noconv=False, fill=None, want_R=True):
        """B: float32 [rows <= round_up(p, 64), ld] (the whole block, padding columns included) -> (X, R, info), float32
        [round_up(p, 64), ld] each. X and R start as zeros, or as the float32 array `fill` (a sentinel: a refusal leaves it; kept
        in self.last_X, self.last_R even when the call raises)."""
        B = np.ascontiguousarray(B, dtype=np.float32)
        rows, ld = (self.p + 63) // 64 * 64, B.shape[1]
        if B.shape[0] > rows:
            raise ValueError("B has %d rows, more than round_up(p, 64) = %d" % (B.shape[0], rows))
        ctx = self.ctx
        full = np.zeros((rows, ld), dtype=np.float32)
        full[:B.shape[0]] = B
        x0 = np.zeros((rows, ld), dtype=np.float32) if fill is None else np.ascontiguousarray(fill, dtype=np.float32)
        assert x0.shape == (rows, ld)
        dB, dX = ctx.dense_from_numpy(full, ld=ld), ctx.dense_from_numpy(x0, ld=ld)
        dR = ctx.dense_from_numpy(x0, ld=ld) if want_R else None
        mats = [dB, dX] + ([dR] if want_R else [])
        for M in mats:
            M.rows = max(B.shape[0], 1) if B.shape[0] < self.p else self.p
        X, R = np.empty((rows, ld), dtype=np.float32), (np.empty((rows, ld), dtype=np.float32) if want_R else None)
        try:
            try:
                info = self.solve(dB, dX, dR, m, rtol, max_it, allow_noconv)
            finally:
                ctx._check(_lib.glf_memcpy_d2h(ctx._ctx, _ptr(X), C.c_void_p(dX.data), C.c_size_t(X.nbytes)))
                if want_R:
                    ctx._check(_lib.glf_memcpy_d2h(ctx._ctx, _ptr(R), C.c_void_p(dR.data), C.c_size_t(R.nbytes)))
                self.last_X, self.last_R = X, R
        finally:
            ctx.destroy(*mats)
        return X, R, info

    def stored(self):
        """The stored form's matrix as downloaded, float32 [p, row1 - row0] (element (k, row - row0) of the symmetric L_A);
        GlfError(ERR_UNSUPPORTED) for a factored form."""
        view = Mat()
        self.ctx._check(_lib.glf_operator_stored(self._h, C.byref(view)), "operator.stored")
        full = np.empty((view.rows, view.ld), dtype=np.float32)
        self.ctx._check(_lib.glf_memcpy_d2h(self.ctx._ctx, _ptr(full), C.c_void_p(view.data), C.c_size_t(full.nbytes)))
        return full[:, :view.cols].copy()


class Graph:
    """One glf_graph: Phi [N, ld] and the eigenvalues of one image, kept on the device until close(). It belongs to its Context and
    must be closed before it. Outputs are float planes, not clamped."""

    def __init__(self, ctx, handle, st):
        self.ctx, self._g = ctx, handle
        gi = self._refresh()
        self.stats = _info(st, self.eigenvalues)   # the build call's: a later transform does not rewrite them
        n = gi.width * gi.height
        # a view: dies with the handle, and becomes None when the handle is compacted
        self.phi = device_tensor_from_ptr(gi.d_phi, n * gi.ld, torch.float32, ctx.device).view(n, gi.ld)

    def _refresh(self):
        """info and eigenvalues from the handle: what the object caches of it (at build time and after every transform)."""
        gi = GraphInfo(struct_size=C.sizeof(GraphInfo))
        self.ctx._check(_lib.glf_graph_get_info(self._g, C.byref(gi)), "graph info")
        self.info = dict(pix=gi.pix, width=gi.width, height=gi.height, p=gi.p, m=gi.m, ld=gi.ld, phi_bytes=int(gi.phi_bytes))
        lam = np.zeros(gi.m, dtype=np.float64)
        self.ctx._check(_lib.glf_graph_eigenvalues(self._g, _ptr(lam)), "graph eigenvalues")
        self.eigenvalues = lam
        return gi

    def close(self):
        if self._g:
            self.phi = None
            handle, self._g = self._g, C.c_void_p()
            self.ctx._check(_lib.glf_graph_destroy(handle), "graph destroy")

    def __del__(self):
        # a Graph dropped without close() gives its Phi back, as long as its context is still alive (a graph is destroyed before it)
        if getattr(self, "_g", None) and self.ctx._ctx:
            _lib.glf_graph_destroy(self._g)
            self._g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def gram(self):
        """Phi^T Phi as a numpy array [m, m] (glf_graph_gram: computed on first use, cached in the handle)."""
        m = self.info["m"]
        G = np.zeros((m, m), dtype=np.float64)
        self.ctx._check(_lib.glf_graph_gram(self._g, _ptr(G)), "graph gram")
        return G

    @property
    def storage(self):
        """PHI_F32, or PHI_F16 once compact() ran (glf_graph_storage)."""
        st = C.c_int(0)
        self.ctx._check(_lib.glf_graph_storage(self._g, C.byref(st), None), "graph storage")
        return int(st.value)

    def column_exponents(self):
        """e_c as numpy int32 [ld] (glf_graph_storage): a compact handle stands for Q[px, c] = 2^e_c * half[px, c]; all 0 on an f32 one."""
        e = np.zeros(self.info["ld"], dtype=np.int32)
        self.ctx._check(_lib.glf_graph_storage(self._g, None, _ptr(e)), "graph storage")
        return e

    def compact(self, storage=PHI_F16):
        """glf_graph_compact: rewrite Phi as f16 with one power-of-two scale per column and release the f32 array (half the bytes of
        every pass and of the handle). The last step of preparing a handle: transform, orthonormalize and project refuse a compact
        handle, every other call returns bit for bit what it returns on an f32 handle whose Phi is dequantize(). phi becomes None
        (the view's memory is released: drop every reference taken from it before), info is refreshed. There is no way back."""
        t = self.ctx.torch
        self.ctx.stream.wait_stream(t.cuda.current_stream(self.ctx.device))   # the caller's own work on phi precedes the rewrite
        try:
            self.ctx._check(_lib.glf_graph_compact(self._g, C.c_int(storage)), "graph compact")   # (drained)
        finally:
            if self._refresh().d_phi is None:
                self.phi = None

    def dequantize(self):
        """Q as a new device float32 [N, ld] tensor (glf_graph_dequantize); on an f32 handle a copy of Phi."""
        t = self.ctx.torch
        n = self.info["height"] * self.info["width"]
        with t.cuda.stream(self.ctx.stream):
            out = t.empty((n, self.info["ld"]), dtype=t.float32, device=self.ctx.device)
        self.ctx._check(_lib.glf_graph_dequantize(self._g, C.c_void_p(out.data_ptr())), "graph dequantize")   # (drained)
        return out

    def _planes(self, planes):
        t = self.ctx.torch
        h, w = self.info["height"], self.info["width"]
        assert planes.dtype == t.float32 and planes.is_cuda and planes.dim() == 3 and planes.is_contiguous()
        if tuple(planes.shape[1:]) != (h, w):
            raise ValueError("planes must be [nplanes, %d, %d], got %s" % (h, w, tuple(planes.shape)))
        self.ctx.stream.wait_stream(t.cuda.current_stream(self.ctx.device))   # the planes are complete before the library reads them
        return planes

    def project(self, planes):
        """c_k = Phi^T s_k in f64 (glf_graph_project): planes device float32 [nplanes, H, W], 1 <= nplanes <= 4 -> numpy [nplanes, m].
        A compact handle raises (GLF_ERR_UNSUPPORTED): project_wide is its projection."""
        planes = self._planes(planes)
        c = np.zeros((planes.shape[0], self.info["m"]), dtype=np.float64)
        self.ctx._check(_lib.glf_graph_project(self._g, C.c_int(planes.shape[0]), C.c_void_p(planes.data_ptr()), _ptr(c)), "graph project")
        return c

    def project_wide(self, planes, weight=None):
        """c_k = Phi^T diag(w) s_k on the matrix pipe (glf_graph_project_wide: f32 chains of at most GRAPH_NORMAL_CHAIN pixel terms
        added into f64), one pass over Phi per 32 planes: planes device float32 [nplanes, H, W], any nplanes >= 1; weight device
        float32 [H, W] or None (w = 1) -> numpy [nplanes, m]. A plane's row depends neither on the planes beside it nor on its slot,
        so the grouping by 32 does not show in the bits. Neither argument is checked for NaN / Inf or sign."""
        planes = self._planes(planes)
        if planes.shape[0] < 1:
            raise ValueError("project_wide: no planes")
        if weight is not None:
            weight = self._weight(weight)
        n = self.info["height"] * self.info["width"]
        c = np.zeros((planes.shape[0], self.info["m"]), dtype=np.float64)
        for k0 in range(0, planes.shape[0], GRAPH_MAX_PLANES):
            k1 = min(k0 + GRAPH_MAX_PLANES, planes.shape[0])
            self.ctx._check(_lib.glf_graph_project_wide(self._g, C.c_void_p(weight.data_ptr()) if weight is not None else None, C.c_int(k1 - k0),
                                                        C.c_void_p(planes.data_ptr() + 4 * n * k0), _ptr(c[k0:k1])), "graph project wide")
        return c

    def _synthesize_groups(self, a, ident=None, plane=None, planes=None):
        """synthesize for any number of outputs: calls of at most GRAPH_MAX_OUTPUTS outputs, each into its rows of one tensor."""
        t = self.ctx.torch
        nout = a.shape[0]
        if nout <= GRAPH_MAX_OUTPUTS:
            return self.synthesize(a, ident, plane, planes)
        with t.cuda.stream(self.ctx.stream):
            out = t.empty((nout, self.info["height"], self.info["width"]), dtype=t.float32, device=self.ctx.device)
        for o in range(0, nout, GRAPH_MAX_OUTPUTS):
            rows = slice(o, min(o + GRAPH_MAX_OUTPUTS, nout))
            self.synthesize(a[rows], None if ident is None else ident[rows], None if plane is None else plane[rows], planes, out=out[rows])
        return out

    def _weight(self, weight):
        t = self.ctx.torch
        h, w = self.info["height"], self.info["width"]
        assert weight.dtype == t.float32 and weight.is_cuda and weight.is_contiguous()
        if tuple(weight.shape) != (h, w):
            raise ValueError("weight must be [%d, %d], got %s" % (h, w, tuple(weight.shape)))
        self.ctx.stream.wait_stream(t.cuda.current_stream(self.ctx.device))   # the weights are complete before the library reads them
        return weight

    def normal_equations(self, weight, planes=None):
        """G = Phi^T diag(w) Phi [m, m] (exactly symmetric) and b_k = Phi^T diag(w) s_k [nplanes, m] in f64, one pass over Phi
        (glf_graph_normal_equations). weight: device float32 [H, W], or None for w = 1; planes: device float32 [nplanes, H, W],
        nplanes <= 4, or None (b is then [0, m]). Neither is checked for NaN / Inf or sign."""
        m = self.info["m"]
        nplanes = 0
        if weight is not None:
            weight = self._weight(weight)
        if planes is not None:
            planes = self._planes(planes)
            nplanes = planes.shape[0]
        G, b = np.zeros((m, m), dtype=np.float64), np.zeros((nplanes, m), dtype=np.float64)
        self.ctx._check(_lib.glf_graph_normal_equations(self._g, C.c_void_p(weight.data_ptr()) if weight is not None else None, C.c_int(nplanes),
                                                        C.c_void_p(planes.data_ptr()) if nplanes else None, _ptr(G), _ptr(b) if nplanes else None),
                        "graph normal equations")
        return G, b

    def fit(self, planes, weight=None, smooth=0.0, ridge=0.0, penalty=None):
        """The weighted least-squares fit of every plane in the span of Phi: z_k = Phi a_k with a_k minimising
        sum_px w (s_k - Phi a)^2 + sum_j penalty_j a_j^2 -- hole filling (w a 0/1 mask), confidences, scribble propagation. One
        normal_equations, fit_coeffs on the host, one synthesize with no identity term -> device float32 [nplanes, H, W].
        penalty_j = (ridge + smooth * lam_j) * trace(G) / m: relative to the mean diagonal of G, so that smooth and ridge depend on
        neither the scale of w nor Phi's normalisation; penalty [m] (absolute units) overrides both. smooth * lam is the Laplacian
        energy of Phi a only to the extent that Phi is orthonormal (the extended eigenvectors are not, exactly; after orthonormalize()
        they are, to f32 rounding). With every
        penalty 0 and w = 0 on a set that leaves Phi rank deficient the system is refused (GlfError). More than 4 planes: two passes
        over Phi, normal_equations(weight) for G and project_wide(planes, weight) for b (f32 chains added into f64 instead of f64
        sums), and the synthesis in groups of 32 outputs; up to 4 planes the route and its bits are the one-pass route above."""
        if planes.shape[0] > MAX_SIGNALS:
            G = self.normal_equations(weight)[0]
            b = self.project_wide(planes, weight)
        else:
            G, b = self.normal_equations(weight, planes)
        if penalty is None:
            penalty = (float(ridge) + float(smooth) * self.eigenvalues) * (np.trace(G) / self.info["m"])
        return self._synthesize_groups(fit_coeffs(G, b, penalty))

    def quadform(self, R, centres=None, out=None, accumulate=False):
        """q_k(px) = |R^T phi_px - t_k|^2 for every pixel and centre in one pass over Phi per launch (glf_graph_quadform): R [m, r],
        centres [ncent, r] or None (one centre at the origin) -> device float32 [ncent, H, W] (out: a contiguous tensor of that shape
        to write into, or with accumulate to add to). Any r: launches of at most QUAD_MAX_COLS columns, every one after the first
        accumulating; any ncent: launches of at most QUAD_MAX_CENTRES centres. A centre's plane depends neither on the centres beside
        it nor on zero columns appended to R and the centres; up to 64 columns it is one launch and accumulate adds the plain result
        with one f32 addition, beyond that each group of columns is added in turn. Soft memberships are a softmax over -q in torch, or
        soft_assign without the distance planes."""
        t = self.ctx.torch
        R = np.asarray(R, dtype=np.float64)
        m, (h, w) = self.info["m"], (self.info["height"], self.info["width"])
        if R.ndim != 2 or R.shape[0] != m or R.shape[1] < 1:
            raise ValueError("R must be [%d, r] with r >= 1, got %s" % (m, R.shape))
        r = R.shape[1]
        cen = np.zeros((1, r)) if centres is None else np.atleast_2d(np.asarray(centres, dtype=np.float64))
        if cen.shape[1] != r or cen.shape[0] < 1:
            raise ValueError("centres must be [ncent, %d], got %s" % (r, cen.shape))
        ncent, n = cen.shape[0], h * w
        if out is None:
            if accumulate:
                raise ValueError("accumulate needs out")
            with t.cuda.stream(self.ctx.stream):
                out = t.empty((ncent, h, w), dtype=t.float32, device=self.ctx.device)   # (every element is written: no fill)
        else:
            assert out.dtype == t.float32 and out.is_cuda and out.is_contiguous()
            if tuple(out.shape) != (ncent, h, w):
                raise ValueError("out must be [%d, %d, %d], got %s" % (ncent, h, w, tuple(out.shape)))
            self.ctx.stream.wait_stream(t.cuda.current_stream(self.ctx.device))   # out is complete before the library touches it
        for c0 in range(0, r, QUAD_MAX_COLS):
            cols = slice(c0, min(c0 + QUAD_MAX_COLS, r))
            Rg = np.ascontiguousarray(R[:, cols])
            for k0 in range(0, ncent, QUAD_MAX_CENTRES):
                k1 = min(k0 + QUAD_MAX_CENTRES, ncent)
                tg = None if centres is None else np.ascontiguousarray(cen[k0:k1, cols])
                self.ctx._check(_lib.glf_graph_quadform(self._g, C.c_uint(Rg.shape[1]), _ptr(Rg), C.c_uint(k1 - k0), _ptr(tg),
                                                        C.c_int(1 if accumulate or c0 > 0 else 0), C.c_void_p(out.data_ptr() + 4 * n * k0)),
                                "graph quadform")   # (returns with the stream drained)
        return out

    def rows(self, pixels):
        """Phi[px][:m] of the given flat pixel indices as numpy float32 [len(pixels), m] (glf_graph_rows); on a compact handle the
        rows of Q = dequantize(), exact."""
        px = np.ascontiguousarray(np.atleast_1d(np.asarray(pixels)), dtype=np.int64)
        rows = np.zeros((px.size, self.info["m"]), dtype=np.float32)
        for k0 in range(0, px.size, QUAD_MAX_CENTRES):
            k1 = min(k0 + QUAD_MAX_CENTRES, px.size)
            self.ctx._check(_lib.glf_graph_rows(self._g, C.c_uint(k1 - k0), _ptr(px[k0:k1]), _ptr(rows[k0:k1])), "graph rows")
        return rows

    def _penalty(self, G, smooth, ridge, penalty):
        """fit's penalty rule: penalty_j = (ridge + smooth * lam_j) * trace(G) / m unless given in absolute units."""
        if penalty is None:
            return (float(ridge) + float(smooth) * self.eigenvalues) * (np.trace(G) / self.info["m"])
        return np.ascontiguousarray(penalty, dtype=np.float64)

    def leverage(self, weight=None, smooth=0.0, ridge=0.0, penalty=None):
        """v(px) = phi_px^T (G_w + diag(penalty))^-1 phi_px of the fit(planes, weight, smooth, ridge, penalty) of any planes: one
        normal_equations(weight), fit_factor on the host, one quadform (m > 64: in groups of 64 columns of R) -> device float32
        [H, W]. Up to the noise variance v is the posterior variance of the fitted value, where it can be trusted; with h = w v the
        fit's leave-one-out residual is e / (1 - h). The penalty rule is fit's own."""
        G = self.normal_equations(weight)[0]
        return self.quadform(fit_factor(G, self._penalty(G, smooth, ridge, penalty)))[0]

    def fit_loo(self, planes, weight, smooths, ridge=0.0):
        """Choose fit's `smooth` by exact leave-one-out cross-validation. One normal_equations in total; per candidate smooth
        fit_coeffs and fit_factor on the host, one synthesize (the fit z), one quadform (the leverage v), and in torch the score
        sum_px w (e / (1 - w v))^2 / sum_px w per plane with e = s - z. planes: device float32 [nplanes, H, W], nplanes <= 4; weight:
        device float32 [H, W] or None (= 1). -> (scores numpy [len(smooths), nplanes], the fit of the candidate with the lowest
        score summed over the planes, device float32 [nplanes, H, W], its index)."""
        t = self.ctx.torch
        G, b = self.normal_equations(weight, planes)
        smooths = [float(s) for s in smooths]
        if not smooths:
            raise ValueError("fit_loo: no candidates")
        scores = np.zeros((len(smooths), planes.shape[0]), dtype=np.float64)
        best, best_fit = -1, None
        for i, smooth in enumerate(smooths):
            pen = self._penalty(G, smooth, ridge, None)
            z = self.synthesize(fit_coeffs(G, b, pen))
            v = self.quadform(fit_factor(G, pen))[0]
            with t.cuda.stream(self.ctx.stream):
                wd = t.ones_like(v, dtype=t.float64) if weight is None else weight.double()
                loo = (planes.double() - z.double()) / (1.0 - wd * v.double())
                sc = (wd * loo * loo).sum(dim=(1, 2)) / wd.sum()
            scores[i] = sc.cpu().numpy()
            if best < 0 or scores[i].sum() < scores[best].sum():
                best, best_fit = i, z
        return scores, best_fit, best

    def distance(self, seeds, response=None, dim=None):
        """Squared diffusion distance from seed pixels, D_s(px)^2 = sum_{j < dim} g_j^2 (Phi[px][j] - Phi[seed_s][j])^2: the "magic
        wand" on a resident graph. seeds: flat pixel indices; response: g [m], default 1 - lam; dim: default m. One quadform with
        R = diag(g)[:, :dim] and the centres t_s = fl32(g) o Q[seed_s][:dim] (rows(): a compact handle uses Q), formed as the
        difference before the square, so that nothing cancels near the seed and D_s(seed_s) is 0 exactly. -> device float32
        [len(seeds), H, W]."""
        m = self.info["m"]
        dim = m if dim is None else int(dim)
        if not 1 <= dim <= m:
            raise ValueError("dim must be in 1 .. %d, got %d" % (m, dim))
        g = np.asarray(1.0 - self.eigenvalues if response is None else response, dtype=np.float64)
        if g.shape != (m,):
            raise ValueError("response must be [%d], got %s" % (m, g.shape))
        g32 = g.astype(np.float32).astype(np.float64)          # what the kernel multiplies by: the centre is then the pixel's own y
        R = np.diag(g32)[:, :dim]
        return self.quadform(R, g32[None, :dim] * self.rows(seeds)[:, :dim].astype(np.float64))

    def samples(self):
        """The sample pixels of the build call as numpy uint32 [p], ascending flat pixel indices (glf_graph_samples). Their rows of
        Phi are phi_A's own, every other row is extended, and the two differ in scale: edges() leaves them out by default."""
        idx = np.zeros(self.info["p"], dtype=np.uint32)
        self.ctx._check(_lib.glf_graph_samples(self._g, _ptr(idx)), "graph samples")
        return idx

    def _edge_args(self, dirs, response, dim, valid, exclude_samples):
        """(the bit mask of dirs, scale [dim] f64, dim, the validity mask as device uint8 [H, W] or None)."""
        t = self.ctx.torch
        m, (h, w) = self.info["m"], (self.info["height"], self.info["width"])
        dirs = (dirs,) if isinstance(dirs, str) else tuple(dirs)
        if not dirs or any(d not in EDGE_DIRS for d in dirs) or len(set(dirs)) != len(dirs):
            raise ValueError("dirs must be distinct names out of %s, got %r" % (sorted(EDGE_DIRS), dirs))
        dim = m if dim is None else int(dim)
        if not 1 <= dim <= m:
            raise ValueError("dim must be in 1 .. %d, got %d" % (m, dim))
        g = np.asarray(1.0 - self.eigenvalues if response is None else response, dtype=np.float64)
        if g.shape != (m,):
            raise ValueError("response must be [%d], got %s" % (m, g.shape))
        if valid is not None:
            if tuple(valid.shape) != (h, w) or not valid.is_cuda:
                raise ValueError("valid must be a device tensor [%d, %d], got %s" % (h, w, tuple(valid.shape)))
            self.ctx.stream.wait_stream(t.cuda.current_stream(self.ctx.device))   # the mask is complete before the library reads it
        with t.cuda.stream(self.ctx.stream):
            mask = None if valid is None else (valid != 0).to(t.uint8).contiguous()
            if exclude_samples:
                mask = t.ones((h, w), dtype=t.uint8, device=self.ctx.device) if mask is None else mask   # (a fresh tensor either way)
                mask.view(-1)[t.from_numpy(self.samples().astype(np.int64)).to(self.ctx.device)] = 0
        return sum(EDGE_DIRS[d] for d in dirs), np.ascontiguousarray(g[:dim]), dim, mask

    def edges(self, dirs=("E", "S", "SE", "SW"), response=None, dim=None, valid=None, exclude_samples=True):
        """The spectral edge map (glf_graph_edges): per direction the squared distance in the embedding between a pixel and its
        neighbour, sum_{c < dim} (g_c (Phi[nb][c] - Phi[px][c]))^2 with nb = E (row, col + 1), S (row + 1, col), SE (row + 1, col + 1),
        SW (row + 1, col - 1) -> device float32 [len(dirs), H, W], plane i for dirs[i], in one pass over Phi (m > 64: one per 64
        columns). response: g [m], default 1 - lam (distance's default); dim: default m; valid: device tensor [H, W], an edge
        with an endpoint where it is 0 is +0, as is an edge that leaves the image; exclude_samples: also drop the handle's sample
        pixels (samples()), whose rows of Phi have another scale than the extended rows and would dominate the map. The values are
        the edge weights of the 4- / 8-connected pixel graph in the spectral metric."""
        t = self.ctx.torch
        dirs = (dirs,) if isinstance(dirs, str) else tuple(dirs)
        out, order, _ = self._edges_run(dirs, response, dim, valid, exclude_samples)
        if list(dirs) == order:
            return out
        with t.cuda.stream(self.ctx.stream):
            out = out[[order.index(d) for d in dirs]]
        self.ctx.stream.synchronize()                                            # as every call here: the result is complete on return
        return out

    def _edges_run(self, dirs, response, dim, valid, exclude_samples):
        """(the planes of glf_graph_edges in the library's order, that order as a list of names, the mask the call ran with as device
        uint8 [H, W] or None). Returns with the stream drained."""
        t = self.ctx.torch
        bits, scale, dim, mask = self._edge_args(dirs, response, dim, valid, exclude_samples)
        order = sorted(dirs, key=lambda d: EDGE_DIRS[d])                         # the library's plane order: ascending bits
        h, w = self.info["height"], self.info["width"]
        with t.cuda.stream(self.ctx.stream):
            out = t.empty((len(order), h, w), dtype=t.float32, device=self.ctx.device)   # (every element is written: no fill)
        self.ctx._check(_lib.glf_graph_edges(self._g, C.c_uint(bits), C.c_uint(dim), _ptr(scale), C.c_void_p(mask.data_ptr()) if mask is not None else None,
                                             C.c_void_p(out.data_ptr())), "graph edges")   # (returns with the stream drained)
        return out, order, mask

    def boundary(self, response=None, dim=None, valid=None, exclude_samples=True):
        """The boundary strength of every pixel -> device float32 [H, W]: the sum over the pixel's up to eight incident edges (its own
        E, S, SE, SW edges and those of its W, N, NW, NE predecessors that point at it) of edges(...), divided by the number of them
        that are live (inside the image, both endpoints valid), 0 where none is. Formed in torch on the library's stream from the
        four planes of one glf_graph_edges call and the mask it ran with, in f32, the eight terms added in that order; returns with
        that stream drained."""
        t = self.ctx.torch
        e, _, mask = self._edges_run(("E", "S", "SE", "SW"), response, dim, valid, exclude_samples)
        h, w = self.info["height"], self.info["width"]
        with t.cuda.stream(self.ctx.stream):
            v = t.ones((h, w), dtype=t.bool, device=self.ctx.device) if mask is None else mask != 0
            live = t.zeros((4, h, w), dtype=t.bool, device=self.ctx.device)
            live[0, :, :-1] = v[:, :-1] & v[:, 1:]
            live[1, :-1, :] = v[:-1, :] & v[1:, :]
            live[2, :-1, :-1] = v[:-1, :-1] & v[1:, 1:]
            live[3, :-1, 1:] = v[:-1, 1:] & v[1:, :-1]
            total, count = t.zeros((h, w), dtype=t.float32, device=self.ctx.device), t.zeros((h, w), dtype=t.float32, device=self.ctx.device)
            for k in range(4):                                                   # the pixel's own forward edges
                total += e[k]
                count += live[k]
            # the forward edges of the predecessors, seen from the pixel they point at
            total[:, 1:] += e[0, :, :-1]
            count[:, 1:] += live[0, :, :-1]
            total[1:, :] += e[1, :-1, :]
            count[1:, :] += live[1, :-1, :]
            total[1:, 1:] += e[2, :-1, :-1]
            count[1:, 1:] += live[2, :-1, :-1]
            total[1:, :-1] += e[3, :-1, 1:]
            count[1:, :-1] += live[3, :-1, 1:]
            out = t.where(count > 0, total / count.clamp_min(1.0), t.zeros_like(total))
        self.ctx.stream.synchronize()                                            # as every call here: the result is complete on return
        return out

    def _robust_loss(self, loss, c, sigma, nplanes):
        rl = RobustLoss(struct_size=C.sizeof(RobustLoss), kind=_robust_kind(loss), c=0.0 if c is None else float(c))
        if sigma is not None:
            sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (nplanes,))
            for k in range(nplanes):
                rl.sigma[k] = float(sg[k])
        return rl

    def robust_step(self, planes, coeffs, loss, c=None, sigma=1.0, weight=None, want_weights=False, want_residuals=False):
        """One IRLS iteration's device work at the iterate coeffs [nplanes, m] (glf_graph_robust_step): the per-pixel weight
        w_eff = weight * u(q), q = sum_k ((s_k - Phi a_k) / sigma_k)^2, of the loss "huber" | "cauchy" | "tukey" with the tuning constant
        c (None: the kind's default), then G = Phi^T diag(w_eff) Phi and b_k = Phi^T diag(w_eff) s_k. planes: device float32
        [nplanes, H, W], nplanes <= 4; sigma: a float or [nplanes], > 0; weight: device float32 [H, W] or None (= 1).
        -> (G [m, m], b [nplanes, m], loss = sum w rho(q), mass = sum w_eff, w_eff device float32 [H, W] or None, the residual planes
        device float32 [nplanes, H, W] or None). Asking for the last two changes no bit of the rest."""
        t = self.ctx.torch
        planes = self._planes(planes)
        nplanes, h, w = planes.shape
        m = self.info["m"]
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(coeffs, dtype=np.float64)))
        if a.shape != (nplanes, m):
            raise ValueError("coeffs must be [%d, %d], got %s" % (nplanes, m, a.shape))
        if weight is not None:
            weight = self._weight(weight)
        rl = self._robust_loss(loss, c, sigma, nplanes)
        with t.cuda.stream(self.ctx.stream):
            wout = t.empty((h, w), dtype=t.float32, device=self.ctx.device) if want_weights else None   # (every element is written)
            rout = t.empty((nplanes, h, w), dtype=t.float32, device=self.ctx.device) if want_residuals else None
        G, b = np.zeros((m, m), dtype=np.float64), np.zeros((nplanes, m), dtype=np.float64)
        lo, ma = C.c_double(0.0), C.c_double(0.0)
        self.ctx._check(_lib.glf_graph_robust_step(self._g, C.byref(rl), C.c_void_p(weight.data_ptr()) if weight is not None else None,
                                                   C.c_int(nplanes), C.c_void_p(planes.data_ptr()), _ptr(a), _ptr(G), _ptr(b), C.byref(lo), C.byref(ma),
                                                   C.c_void_p(wout.data_ptr()) if want_weights else None,
                                                   C.c_void_p(rout.data_ptr()) if want_residuals else None),
                        "graph robust step")   # (returns with the stream drained)
        return G, b, float(lo.value), float(ma.value), wout, rout

    def fit_robust(self, planes, weight=None, loss="huber", c=None, sigma=None, smooth=0.0, ridge=0.0, penalty=None, max_iter=20, tol=1e-6,
                   sample_rows=4096, return_info=False):
        """The outlier-tolerant fit of the planes in the span of Phi (glf_graph_fit_robust): z_k = Phi a_k with a minimising
        sum_px w rho(q) + sum_k sum_j penalty_j a_kj^2 / (2 sigma_k^2), q = sum_k ((s_k - Phi a_k) / sigma_k)^2, by iteratively
        reweighted least squares from the plain weighted fit: robust_step + fit_coeffs(G, b, penalty) until
        max |a - a_prev| <= tol max |a| or max_iter steps ran, then one synthesize -> device float32 [nplanes, H, W]. loss, c,
        weight: as for robust_step. sigma: a float or [nplanes], or None to estimate it (robust_scale of the plain fit's residuals
        on sample_rows rows). smooth, ridge, penalty: as for fit and in its units (where every u = 1 the result is fit's), scaled by
        trace(G_0) / m of the plain system, so the penalty is fixed over the iterations. Tukey's loss is not convex: the plain fit is
        the start, nothing cleverer. return_info: -> (fit, dict(coeffs [nplanes, m], weights device float32 [H, W] = the last step's
        w_eff, the outlier map, iterations, converged, sigma [nplanes], mass, objective [min(iterations, 32)]))."""
        t = self.ctx.torch
        planes = self._planes(planes)
        nplanes, h, w = planes.shape
        m = self.info["m"]
        if weight is not None:
            weight = self._weight(weight)
        if penalty is None and (smooth or ridge):
            G0, _ = self.normal_equations(weight)
            penalty = (float(ridge) + float(smooth) * self.eigenvalues) * (np.trace(G0) / m)
        if penalty is not None:
            penalty = np.ascontiguousarray(penalty, dtype=np.float64)
            if penalty.shape != (m,):
                raise ValueError("penalty must be [%d], got %s" % (m, penalty.shape))
        opt = RobustOptions(struct_size=C.sizeof(RobustOptions), loss=self._robust_loss(loss, c, sigma, nplanes),
                            penalty=penalty.ctypes.data if penalty is not None else None, max_iter=max_iter, tol=tol, sample_rows=sample_rows,
                            estimate_sigma=1 if sigma is None else 0)
        st = RobustStats(struct_size=C.sizeof(RobustStats))
        a = np.zeros((nplanes, m), dtype=np.float64)
        with t.cuda.stream(self.ctx.stream):
            fit = t.empty((nplanes, h, w), dtype=t.float32, device=self.ctx.device)   # (every element is written)
            wout = t.empty((h, w), dtype=t.float32, device=self.ctx.device) if return_info else None
        self.ctx._check(_lib.glf_graph_fit_robust(self._g, C.byref(opt), C.c_void_p(weight.data_ptr()) if weight is not None else None,
                                                  C.c_int(nplanes), C.c_void_p(planes.data_ptr()), _ptr(a), C.c_void_p(fit.data_ptr()),
                                                  C.c_void_p(wout.data_ptr()) if return_info else None, C.byref(st)),
                        "graph fit robust")   # (returns with the stream drained)
        if not return_info:
            return fit
        its = int(st.iterations)
        return fit, dict(coeffs=a, weights=wout, iterations=its, converged=int(st.converged), sigma=np.array(st.sigma[:nplanes]),
                         mass=float(st.mass), objective=np.array(st.objective[:min(its, ROBUST_OBJECTIVES)]))

    def synthesize(self, coeffs, ident=None, plane=None, planes=None, out=None):
        """out_j = ident[j] * planes[plane[j]] + Phi coeffs[j] (glf_graph_synthesize), one pass over Phi for all outputs: coeffs
        [nout, m] (nout <= 32), ident [nout] floats, plane [nout] ints in [-1, nplanes) (-1 / None: no identity term), planes device
        float32 [nplanes, H, W] or None -> device float32 [nout, H, W] (out: a contiguous tensor of that shape to write into)."""
        t = self.ctx.torch
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(coeffs, dtype=np.float64)))
        nout, h, w = a.shape[0], self.info["height"], self.info["width"]
        if a.shape[1] != self.info["m"]:
            raise ValueError("coeffs must be [nout, %d], got %s" % (self.info["m"], a.shape))
        pl = np.full(nout, -1, dtype=np.int32) if plane is None else np.ascontiguousarray(plane, dtype=np.int32)
        idn = np.zeros(nout, dtype=np.float32) if ident is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ident, dtype=np.float32), (nout,)))
        if pl.shape != (nout,):
            raise ValueError("plane must be [%d]" % nout)
        nplanes = 0
        if planes is not None:
            planes = self._planes(planes)
            nplanes = planes.shape[0]
        if out is None:
            with t.cuda.stream(self.ctx.stream):
                out = t.empty((nout, h, w), dtype=t.float32, device=self.ctx.device)   # (every element is written: no fill)
        else:
            assert out.dtype == t.float32 and out.is_cuda and out.is_contiguous()
            if tuple(out.shape) != (nout, h, w):
                raise ValueError("out must be [%d, %d, %d], got %s" % (nout, h, w, tuple(out.shape)))
        self.ctx._check(_lib.glf_graph_synthesize(self._g, C.c_int(nout), _ptr(a), _ptr(idn), _ptr(pl), C.c_int(nplanes),
                                                  C.c_void_p(planes.data_ptr()) if planes is not None else None,
                                                  C.c_void_p(out.data_ptr())), "graph synthesize")   # (returns with the stream drained)
        return out

    def classify(self, coeffs, ident=None, plane=None, planes=None, bias=None, want=("label",)):
        """The label read-out of the k scores z_j = ident[j] * planes[plane[j]] + Phi coeffs[j] (+ bias[j]) in one pass over Phi
        (glf_graph_classify): the score planes synthesize would write are formed in registers and reduced per pixel. coeffs [k, m]
        (k <= CLASSIFY_MAX), ident / plane / planes as in synthesize, bias [k] or None; want: any of "label", "best", "margin".
        -> dict of device tensors [H, W]: label int32 (the lowest index among equal best scores; a NaN score never wins), best
        float32 (without a bias: synthesize's winning output, bit for bit), margin float32 = best - runner-up (+0 on a tie, +inf
        for k = 1)."""
        t = self.ctx.torch
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(coeffs, dtype=np.float64)))
        k, h, w = a.shape[0], self.info["height"], self.info["width"]
        if a.shape[1] != self.info["m"]:
            raise ValueError("coeffs must be [k, %d], got %s" % (self.info["m"], a.shape))
        if k > CLASSIFY_MAX:
            raise ValueError("classify takes at most %d classes (CLASSIFY_MAX), got %d" % (CLASSIFY_MAX, k))
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(key not in ("label", "best", "margin") for key in want):
            raise ValueError('want must name at least one of "label", "best", "margin", got %r' % (want,))
        pl = np.full(k, -1, dtype=np.int32) if plane is None else np.ascontiguousarray(plane, dtype=np.int32)
        idn = np.zeros(k, dtype=np.float32) if ident is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ident, dtype=np.float32), (k,)))
        if pl.shape != (k,):
            raise ValueError("plane must be [%d]" % k)
        bs = None
        if bias is not None:
            bs = np.ascontiguousarray(np.broadcast_to(np.asarray(bias, dtype=np.float64), (k,)))
        nplanes = 0
        if planes is not None:
            planes = self._planes(planes)
            nplanes = planes.shape[0]
        with t.cuda.stream(self.ctx.stream):
            out = {key: t.empty((h, w), dtype=t.int32 if key == "label" else t.float32, device=self.ctx.device) for key in want}   # (every element is written)
        ptr = {key: C.c_void_p(out[key].data_ptr()) if key in out else None for key in ("label", "best", "margin")}
        self.ctx._check(_lib.glf_graph_classify(self._g, C.c_int(k), _ptr(a), _ptr(idn), _ptr(pl), C.c_int(nplanes),
                                                C.c_void_p(planes.data_ptr()) if planes is not None else None, _ptr(bs),
                                                ptr["label"], ptr["best"], ptr["margin"]), "graph classify")   # (returns with the stream drained)
        return out

    def refine_logits(self, logits, response=None, ident=1.0, bias=None, want=("label", "margin")):
        """argmax_j (ident * logit_j + Phi diag(response) Phi^T logit_j) without writing the filtered logits: one project_wide, the
        scaling on the host, one classify with the logits as identity planes. logits: device float32 [k, H, W], k <= CLASSIFY_MAX;
        response: g [m], default 1 - lam (distance's default); ident a float or [k]. -> classify's dict."""
        k = logits.shape[0]
        if k > CLASSIFY_MAX:
            raise ValueError("refine_logits takes at most %d classes (CLASSIFY_MAX), got %d" % (CLASSIFY_MAX, k))
        m = self.info["m"]
        g = np.asarray(1.0 - self.eigenvalues if response is None else response, dtype=np.float64)
        if g.shape != (m,):
            raise ValueError("response must be [%d], got %s" % (m, g.shape))
        c = self.project_wide(logits)
        return self.classify(g[None, :] * c, ident, np.arange(k, dtype=np.int32), logits, bias, want)

    def softmax(self, coeffs, ident=None, plane=None, planes=None, bias=None, beta=1.0, want=("prob",)):
        """The softmax read-out of the k scores z_j = ident[j] * planes[plane[j]] + Phi coeffs[j] (+ bias[j]) in one pass over Phi
        (glf_graph_softmax): classify's scores, formed in registers and never written. coeffs [k, m] (k <= SOFTMAX_MAX), ident /
        plane / planes / bias as in classify, beta > 0 the inverse temperature; want: any of "prob", "lse", "entropy".
        -> dict of device float32 tensors: prob [k, H, W] = exp(beta z_j) / sum_i exp(beta z_i), lse [H, W] = log sum_j exp(beta z_j),
        entropy [H, W] = -sum_j prob_j ln prob_j. A pixel with a NaN or +inf score, or with none above -inf, is NaN in every output.
        planes must not overlap the returned prob (it cannot: prob is a fresh tensor)."""
        t = self.ctx.torch
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(coeffs, dtype=np.float64)))
        k, h, w = a.shape[0], self.info["height"], self.info["width"]
        if a.shape[1] != self.info["m"]:
            raise ValueError("coeffs must be [k, %d], got %s" % (self.info["m"], a.shape))
        if k > SOFTMAX_MAX:
            raise ValueError("softmax takes at most %d classes (SOFTMAX_MAX), got %d" % (SOFTMAX_MAX, k))
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(key not in ("prob", "lse", "entropy") for key in want):
            raise ValueError('want must name at least one of "prob", "lse", "entropy", got %r' % (want,))
        pl = np.full(k, -1, dtype=np.int32) if plane is None else np.ascontiguousarray(plane, dtype=np.int32)
        idn = np.zeros(k, dtype=np.float32) if ident is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ident, dtype=np.float32), (k,)))
        if pl.shape != (k,):
            raise ValueError("plane must be [%d]" % k)
        bs = None
        if bias is not None:
            bs = np.ascontiguousarray(np.broadcast_to(np.asarray(bias, dtype=np.float64), (k,)))
        nplanes = 0
        if planes is not None:
            planes = self._planes(planes)
            nplanes = planes.shape[0]
        with t.cuda.stream(self.ctx.stream):
            out = {key: t.empty((k, h, w) if key == "prob" else (h, w), dtype=t.float32, device=self.ctx.device) for key in want}   # (every element is written)
        ptr = {key: C.c_void_p(out[key].data_ptr()) if key in out else None for key in ("prob", "lse", "entropy")}
        self.ctx._check(_lib.glf_graph_softmax(self._g, C.c_int(k), _ptr(a), _ptr(idn), _ptr(pl), C.c_int(nplanes),
                                               C.c_void_p(planes.data_ptr()) if planes is not None else None, _ptr(bs), C.c_double(float(beta)),
                                               ptr["prob"], ptr["lse"], ptr["entropy"]), "graph softmax")   # (returns with the stream drained)
        return out

    def soft_assign(self, centres, scale=None, temperature=1.0, want=("prob",)):
        """Soft memberships of the centres t_j [k, dim] (embedding space, as in cluster_step; k <= SOFTMAX_MAX, dim <= m):
        p_j(px) proportional to exp(-|scale o Phi[px][:dim] - t_j|^2 / temperature), without forming a distance plane. The row's own
        squared length is common to the k classes and cancels, so this is one softmax with a_j = 2 scale o t_j / temperature
        (zero-padded to m) and bias_j = -|t_j|^2 / temperature. scale [dim] or None (= 1). Unit-length rows are out of scope.
        -> softmax's dict."""
        cent = np.ascontiguousarray(np.atleast_2d(np.asarray(centres, dtype=np.float64)))
        k, dim = cent.shape
        m = self.info["m"]
        if not 1 <= dim <= m:
            raise ValueError("centres must be [k, dim] with dim in 1 .. %d, got %s" % (m, cent.shape))
        if k > SOFTMAX_MAX:
            raise ValueError("soft_assign takes at most %d centres (SOFTMAX_MAX), got %d" % (SOFTMAX_MAX, k))
        temperature = float(temperature)
        if not (temperature > 0.0 and np.isfinite(temperature)):
            raise ValueError("temperature must be finite and positive, got %r" % temperature)
        scale = _scale(scale, dim)
        a = np.zeros((k, m), dtype=np.float64)
        a[:, :dim] = 2.0 * (cent if scale is None else cent * scale[None, :]) / temperature
        return self.softmax(a, bias=-(cent * cent).sum(axis=1) / temperature, want=want)

    def mean_field(self, logits, coupling=1.0, compat=None, response=None, weight=None, exclude_samples=True, beta=1.0, ident=1.0,
                   max_iter=10, tol=1e-4, init=None, want=("prob",)):
        """Mean-field iterations of a dense CRF whose pairwise kernel is Phi diag(response) Phi^T:
        Q <- softmax_j(beta (ident logit_j + sum_l' M[j][l'] (Phi diag(response) Phi_w^T Q_l'))), M = coupling I (Potts) or compat
        [k, k]. Per iteration one project_wide of Q (c = Phi^T diag(weight) Q), the mixing a = M (response o c) on the host, one
        softmax with the logits as identity planes. logits: device float32 [k, H, W], k <= SOFTMAX_MAX; response: g [m], default
        1 - lam; weight: device float32 [H, W] or None, multiplied by the mask that is 0 on samples() when exclude_samples (their rows
        of Phi differ in scale: edges()); init: Q^0 device float32 [k, H, W], default the softmax of the logits alone. Stops when
        max |a - a_prev| <= tol max |a| or after max_iter iterations. The self-message is not subtracted.
        -> softmax's dict of the last iteration (of Q^0 for max_iter = 0), plus coeffs [k, m] (the last a), changes (max |a - a_prev|
        per iteration), iterations and converged."""
        t = self.ctx.torch
        logits = self._planes(logits)
        k, (h, w), m = logits.shape[0], (self.info["height"], self.info["width"]), self.info["m"]
        if not 1 <= k <= SOFTMAX_MAX:
            raise ValueError("mean_field takes 1 .. %d classes (SOFTMAX_MAX), got %d" % (SOFTMAX_MAX, k))
        g = np.asarray(1.0 - self.eigenvalues if response is None else response, dtype=np.float64)
        if g.shape != (m,):
            raise ValueError("response must be [%d], got %s" % (m, g.shape))
        M = float(coupling) * np.eye(k) if compat is None else np.asarray(compat, dtype=np.float64)
        if M.shape != (k, k):
            raise ValueError("compat must be [%d, %d], got %s" % (k, k, M.shape))
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(key not in ("prob", "lse", "entropy") for key in want):
            raise ValueError('want must name at least one of "prob", "lse", "entropy", got %r' % (want,))
        if weight is not None:
            weight = self._weight(weight)
        if exclude_samples:
            with t.cuda.stream(self.ctx.stream):
                mask = t.ones((h, w), dtype=t.float32, device=self.ctx.device)
                mask.view(-1)[t.from_numpy(self.samples().astype(np.int64)).to(self.ctx.device)] = 0
                weight = mask if weight is None else (weight * mask).contiguous()
        slots = np.arange(k, dtype=np.int32)
        with_prob = tuple(dict.fromkeys(("prob",) + want))
        a = np.zeros((k, m), dtype=np.float64)
        if init is None:
            out = self.softmax(a, ident, slots, logits, beta=beta, want=with_prob)
        else:
            init = self._planes(init)
            if tuple(init.shape) != (k, h, w):
                raise ValueError("init must be [%d, %d, %d], got %s" % (k, h, w, tuple(init.shape)))
            out = {"prob": init}
        changes, converged = [], False
        for _ in range(int(max_iter)):
            prev = a
            a = M @ (g[None, :] * self.project_wide(out["prob"], weight))
            out = self.softmax(a, ident, slots, logits, beta=beta, want=with_prob)
            changes.append(float(np.abs(a - prev).max()))
            if changes[-1] <= float(tol) * float(np.abs(a).max()):
                converged = True
                break
        if init is not None and not changes and want != ("prob",):
            raise ValueError("mean_field: max_iter = 0 with init leaves nothing but init to return")
        res = {key: out[key] for key in want}
        res.update(coeffs=a, changes=np.array(changes), iterations=len(changes), converged=converged)
        return res

    def propagate_labels(self, seeds, k, weight=None, smooth=0.0, ridge=0.0, bias=None, want=("label", "margin")):
        """Scribbles to a label map: the weighted least-squares fit of the k one-hot seed planes in the span of Phi (fit's system,
        fit's penalty rule), read out by one classify with no identity term; the fitted planes are never written. seeds: device
        integer [H, W], -1 where unlabelled, else the class in 0 .. k - 1 (k <= CLASSIFY_MAX; every class needs a seed); weight:
        device float32 [H, W] or None (= 1), it counts on the seed pixels only. One normal_equations for G_w, one project_wide of
        the one-hot planes for b, fit_coeffs on the host. -> classify's dict plus coeffs [k, m]."""
        t = self.ctx.torch
        k = int(k)
        h, w = self.info["height"], self.info["width"]
        if not 1 <= k <= CLASSIFY_MAX:
            raise ValueError("propagate_labels takes 1 .. %d classes (CLASSIFY_MAX), got %d" % (CLASSIFY_MAX, k))
        assert seeds.is_cuda and not seeds.is_floating_point()
        if tuple(seeds.shape) != (h, w):
            raise ValueError("seeds must be [%d, %d], got %s" % (h, w, tuple(seeds.shape)))
        if weight is not None:
            weight = self._weight(weight)
        self.ctx.stream.wait_stream(t.cuda.current_stream(self.ctx.device))   # the seeds are complete before they are read here
        with t.cuda.stream(self.ctx.stream):
            sd = seeds.to(t.int64)
            lo, hi = int(sd.min()), int(sd.max())
            if lo < -1 or hi > k - 1:
                raise ValueError("seeds must lie in -1 .. %d, got %d .. %d" % (k - 1, lo, hi))
            onehot = (sd[None, :, :] == t.arange(k, device=sd.device)[:, None, None]).to(t.float32).contiguous()
            counts = onehot.sum(dim=(1, 2)).cpu().numpy()
            if (counts == 0).any():
                raise ValueError("propagate_labels: class %d has no seed" % int(np.flatnonzero(counts == 0)[0]))
            wm = (sd >= 0).to(t.float32)
            if weight is not None:
                wm = wm * weight
            wm = wm.contiguous()
        G = self.normal_equations(wm)[0]
        b = self.project_wide(onehot, wm)
        a = fit_coeffs(G, b, self._penalty(G, smooth, ridge, None))
        out = self.classify(a, bias=bias, want=want)
        out["coeffs"] = a
        return out

    def _labels(self, labels, what):
        t = self.ctx.torch
        h, w = self.info["height"], self.info["width"]
        assert labels.dtype == t.int32 and labels.is_cuda and labels.is_contiguous()
        if tuple(labels.shape) != (h, w):
            raise ValueError("%s must be [%d, %d], got %s" % (what, h, w, tuple(labels.shape)))
        self.ctx.stream.wait_stream(t.cuda.current_stream(self.ctx.device))   # the labels are complete before the library touches them
        return labels

    def _new_labels(self):
        t = self.ctx.torch
        with t.cuda.stream(self.ctx.stream):
            return t.empty((self.info["height"], self.info["width"]), dtype=t.int32, device=self.ctx.device)   # (every element is written)

    def _step_args(self, cent, scale, prev, labels):
        """What cluster_step and cluster_step_ex prepare alike -> (k, dim, cent, scale, prev's pointer or None, labels, sums, counts, changed)."""
        cent = np.ascontiguousarray(np.atleast_2d(np.asarray(cent, dtype=np.float64)))
        k, dim = cent.shape
        scale = _scale(scale, dim)
        if prev is not None:
            prev = self._labels(prev, "prev")
        labels = self._new_labels() if labels is None else self._labels(labels, "labels")
        return (k, dim, cent, scale, C.c_void_p(prev.data_ptr()) if prev is not None else None, labels, np.zeros((k, dim), dtype=np.float64),
                np.zeros(k, dtype=np.uint64), C.c_uint64(0))

    def cluster_step(self, cent, scale=None, prev=None, labels=None):
        """One Lloyd iteration of k-means over the embedded rows e(px) = scale o Phi[px][:dim] in one pass over Phi
        (glf_graph_cluster_step): every pixel takes the nearest of the centroids cent [k, dim] (embedding space; k <= 32,
        dim <= min(m, 64); the lowest index wins a tie). scale [dim] or None (= 1); prev: device int32 [H, W] labels to count the
        changes against, or None; labels: the device int32 [H, W] tensor to write (it may be prev itself), or None for a new one.
        -> (labels, sums [k, dim] of the raw rows of Phi per label, counts uint64 [k], changed)."""
        k, dim, cent, scale, prev, labels, sums, counts, changed = self._step_args(cent, scale, prev, labels)
        self.ctx._check(_lib.glf_graph_cluster_step(self._g, C.c_uint(k), C.c_uint(dim), _ptr(cent), _ptr(scale), prev, C.c_void_p(labels.data_ptr()),
                                                    _ptr(sums), _ptr(counts), C.byref(changed)), "graph cluster step")   # (returns with the stream drained)
        return labels, sums, counts, int(changed.value)

    def _embed(self, normalize, weight):
        if weight is not None:
            weight = self._weight(weight)
        return ClusterEmbed(C.sizeof(ClusterEmbed), int(bool(normalize)), weight.data_ptr() if weight is not None else None)

    def cluster_step_ex(self, cent, scale=None, prev=None, labels=None, normalize=False, weight=None):
        """cluster_step under an embedding (glf_graph_cluster_step_ex). normalize: unit-length rows, e(px) = scale o Phi[px][:dim]
        divided by its length (a row of length 0 stays at the origin); cent is then in that embedding. weight: device float32 [H, W]
        or None (= 1), not checked for sign, NaN or Inf; it enters the update only, every pixel is labelled.
        -> (labels, sums [k, dim] = sum of weight / length times the raw rows of Phi per label, counts uint64 [k] (pixels),
        mass [k] = sum of the weights per label, changed (pixels)). With neither set every output has cluster_step's bits."""
        emb = self._embed(normalize, weight)
        k, dim, cent, scale, prev, labels, sums, counts, changed = self._step_args(cent, scale, prev, labels)
        mass = np.zeros(k, dtype=np.float64)
        self.ctx._check(_lib.glf_graph_cluster_step_ex(self._g, C.byref(emb), C.c_uint(k), C.c_uint(dim), _ptr(cent), _ptr(scale), prev,
                                                       C.c_void_p(labels.data_ptr()), _ptr(sums), _ptr(counts), _ptr(mass), C.byref(changed)),
                        "graph cluster step")
        return labels, sums, counts, mass, int(changed.value)

    def segment(self, k, dim=None, scale=None, init=None, seed=1, max_iter=50, sample_rows=4096, normalize=False, weight=None):
        """Spectral segmentation (glf_graph_segment): Lloyd's k-means over the embedded rows, cluster_step + cluster_update until a
        step moves no label or max_iter steps ran. dim defaults to min(m, 64, max(k, 2)): the usual k vectors for k segments. init:
        centroids [k, dim] in embedding space, or None for k-means++ seeding (cluster_seed with `seed`) among the sample_rows rows
        floor(i N / n_s) of Phi. -> (labels device int32 [H, W], cent [k, dim], dict(iterations, converged, changed_last, counts)).
        With normalize (unit-length rows: use dim = m with it) or weight (device float32 [H, W]) set, glf_graph_segment_ex:
        cluster_step_ex + cluster_update_w, seeding by cluster_seed_w on the normalised sample; the dict then also holds mass [k]."""
        if dim is None:
            dim = min(self.info["m"], 64, max(int(k), 2))
        cent = np.zeros((max(int(k), 0), max(int(dim), 0)), dtype=np.float64)
        if init is not None:
            init = np.asarray(init, dtype=np.float64)
            if init.shape != cent.shape:
                raise ValueError("init must be [%d, %d], got %s" % (cent.shape + (init.shape,)))
            cent[...] = init
        scale = _scale(scale, int(dim))
        labels = self._new_labels()
        opt = SegmentOptions(C.sizeof(SegmentOptions), k, dim, max_iter, sample_rows, 0 if init is None else 1, seed,
                             scale.ctypes.data if scale is not None else None)
        st = SegmentStats()
        if normalize or weight is not None:
            emb = self._embed(normalize, weight)
            mass = np.zeros(max(int(k), 0), dtype=np.float64)
            self.ctx._check(_lib.glf_graph_segment_ex(self._g, C.byref(opt), C.byref(emb), C.c_void_p(labels.data_ptr()), _ptr(cent), C.byref(st),
                                                      _ptr(mass)), "graph segment")
            return labels, cent, dict(iterations=int(st.iterations), converged=int(st.converged), changed_last=int(st.changed_last),
                                      counts=np.array(st.counts[:int(k)], dtype=np.uint64), mass=mass)
        self.ctx._check(_lib.glf_graph_segment(self._g, C.byref(opt), C.c_void_p(labels.data_ptr()), _ptr(cent), C.byref(st)), "graph segment")
        return labels, cent, dict(iterations=int(st.iterations), converged=int(st.converged), changed_last=int(st.changed_last),
                                  counts=np.array(st.counts[:int(k)], dtype=np.uint64))

    def transform(self, T, lam):
        """Phi <- Phi T in place on the device (glf_graph_transform): T [m, m_new], 1 <= m_new <= m, lam [m_new] the eigenvalues of
        the new columns. The handle's m becomes m_new, columns m_new .. ld of Phi exact zeros, the cached Gram matrix is dropped;
        info and eigenvalues are refreshed (phi stays the same view; stats stay the build call's). Truncation (T = I[:, :k]), column
        reordering and rescaling, any rotation."""
        T = np.ascontiguousarray(np.asarray(T, dtype=np.float64))
        lam = np.ascontiguousarray(np.asarray(lam, dtype=np.float64))
        if T.ndim != 2 or T.shape[0] != self.info["m"] or lam.shape != (T.shape[1],):
            raise ValueError("T must be [%d, m_new] and lam [m_new], got %s and %s" % (self.info["m"], T.shape, lam.shape))
        t = self.ctx.torch
        self.ctx.stream.wait_stream(t.cuda.current_stream(self.ctx.device))   # the caller's own reads of phi precede the rewrite
        try:
            self.ctx._check(_lib.glf_graph_transform(self._g, C.c_uint(T.shape[1]), _ptr(T), _ptr(lam)), "graph transform")   # (drained)
        finally:
            self._refresh()

    def orthonormalize(self, mode="ritz", passes=1, verify=False):
        """glf_graph_orthonormalize: make Phi orthonormal in place. mode "ritz": Phi becomes the orthonormal eigenbasis of the same
        smoothing operator Phi diag(1 - lam) Phi^T, eigenvalues ascending; "cholesky": Gram-Schmidt in column order, eigenvalues
        kept. Per pass one normal_equations(None), basis_orthonormal on the host, one transform; a second pass runs in Cholesky
        mode. -> dict(passes, defect_in = max |Phi^T Phi - I| before, defect_out = the same after when verify, else NaN)."""
        modes = {"cholesky": BASIS_CHOLESKY, "ritz": BASIS_RITZ}
        st = BasisStats(struct_size=C.sizeof(BasisStats))
        try:
            self.ctx._check(_lib.glf_graph_orthonormalize(self._g, C.c_int(modes.get(mode, -1) if isinstance(mode, str) else int(mode)),
                                                          C.c_int(passes), C.c_int(bool(verify)), C.byref(st)), "graph orthonormalize")
        finally:
            self._refresh()
        return dict(passes=int(st.passes), defect_in=float(st.defect_in), defect_out=float(st.defect_out))

    def apply(self, planes, weights, ident=1.0, wide=None):
        """Diagonal responses: out[r, k] = ident[r] * s_k + Phi diag(weights[r]) Phi^T s_k for every response r and plane k -- one
        projection, the scaling on the host, the synthesis. weights [nresp, m] (e.g. gain * lam for the reference filter, 1 - lam
        for smoothing, any band-pass), ident a float or [nresp] -> device float32 [nresp, nplanes, H, W]. wide None: up to 4 planes
        and nresp * nplanes <= 32 outputs take project and one synthesize; anything larger takes project_wide (one pass over Phi
        per 32 planes) and synthesize in groups of at most 32 outputs. wide True: project_wide for any nplanes."""
        wts = np.atleast_2d(np.asarray(weights, dtype=np.float64))
        nresp, nplanes = wts.shape[0], planes.shape[0]
        if wide is None:
            wide = nplanes > MAX_SIGNALS or nresp * nplanes > GRAPH_MAX_OUTPUTS
        wide = wide or self.phi is None   # a compact handle has no project: always the wide route
        c = self.project_wide(planes) if wide else self.project(planes)
        a = (wts[:, None, :] * c[None, :, :]).reshape(nresp * nplanes, -1)
        idn = np.repeat(np.broadcast_to(np.asarray(ident, dtype=np.float32), (nresp,)), nplanes)
        out = self._synthesize_groups(a, idn, np.tile(np.arange(nplanes, dtype=np.int32), nresp), planes)
        return out.view(nresp, nplanes, self.info["height"], self.info["width"])

    def _level(self, level):
        t = self.ctx.torch
        h, w = self.info["height"], self.info["width"]
        assert level.dtype == t.float32 and level.is_cuda and level.is_contiguous()
        if tuple(level.shape) != (h, w):
            raise ValueError("level must be [%d, %d], got %s" % (h, w, tuple(level.shape)))
        self.ctx.stream.wait_stream(t.cuda.current_stream(self.ctx.device))   # the map is complete before the library reads it
        return level

    def blend(self, coeffs, level, ident=None, plane=None, planes=None, out=None):
        """The per-pixel read-out of a bank of score planes z[o, b] = ident[o, b] * planes[plane[o, b]] + Phi coeffs[o, b] in one pass
        over Phi (glf_graph_blend): the planes synthesize would write are formed in registers and never written. Output o gets
        z[o, level(px)] where the level is an integer and (1 - f) z[o, i] + f z[o, i + 1] between two levels (i its integer part, f
        the rest); a level below 0 or NaN reads level 0, one above nlevels - 1 the last. coeffs [nout, nlevels, m], or [nlevels, m]
        for one output (nlevels in 2 .. BLEND_MAX_SLOTS); level device float32 [H, W], shared by the outputs; ident floats and plane
        ints in [-1, nplanes) that broadcast to [nout, nlevels] (-1 / None: no identity term); planes device float32 [nplanes, H, W]
        or None -> device float32 [nout, H, W] (out: a contiguous tensor of that shape to write into, overlapping neither planes nor
        level). More outputs than BLEND_MAX_SLOTS // nlevels are taken in groups, each group one pass over Phi; an output's plane
        does not depend on its group."""
        t = self.ctx.torch
        a = np.asarray(coeffs, dtype=np.float64)
        if a.ndim == 2:
            a = a[None]
        m, h, w = self.info["m"], self.info["height"], self.info["width"]
        if a.ndim != 3 or a.shape[2] != m or a.shape[0] < 1:
            raise ValueError("coeffs must be [nout, nlevels, %d] or [nlevels, %d], got %s" % (m, m, a.shape))
        nout, nlevels = a.shape[:2]
        if not 2 <= nlevels <= BLEND_MAX_SLOTS:
            raise ValueError("blend takes 2 .. %d levels (BLEND_MAX_SLOTS), got %d" % (BLEND_MAX_SLOTS, nlevels))
        a = np.ascontiguousarray(a)
        try:
            pl = np.full((nout, nlevels), -1, dtype=np.int32) if plane is None else np.ascontiguousarray(
                np.broadcast_to(np.asarray(plane, dtype=np.int32), (nout, nlevels)))
            idn = np.zeros((nout, nlevels), dtype=np.float32) if ident is None else np.ascontiguousarray(
                np.broadcast_to(np.asarray(ident, dtype=np.float32), (nout, nlevels)))
        except ValueError:
            raise ValueError("ident and plane must broadcast to [%d, %d]" % (nout, nlevels))
        level = self._level(level)
        nplanes = 0
        if planes is not None:
            planes = self._planes(planes)
            nplanes = planes.shape[0]
        if out is None:
            with t.cuda.stream(self.ctx.stream):
                out = t.empty((nout, h, w), dtype=t.float32, device=self.ctx.device)   # (every element is written: no fill)
        else:
            assert out.dtype == t.float32 and out.is_cuda and out.is_contiguous()
            if tuple(out.shape) != (nout, h, w):
                raise ValueError("out must be [%d, %d, %d], got %s" % (nout, h, w, tuple(out.shape)))
        per = BLEND_MAX_SLOTS // nlevels
        for o0 in range(0, nout, per):
            o1 = min(o0 + per, nout)
            self.ctx._check(_lib.glf_graph_blend(self._g, C.c_int(o1 - o0), C.c_int(nlevels), _ptr(a[o0:o1]), _ptr(idn[o0:o1]), _ptr(pl[o0:o1]),
                                                 C.c_int(nplanes), C.c_void_p(planes.data_ptr()) if planes is not None else None,
                                                 C.c_void_p(level.data_ptr()), C.c_void_p(out.data_ptr() + 4 * h * w * o0)),
                            "graph blend")   # (returns with the stream drained)
        return out

    def apply_local(self, planes, level, weights, ident=1.0):
        """apply with a strength that varies over the image: out_k(px) = the level(px) read-out of the bank ident[b] * s_k + Phi
        diag(weights[b]) Phi^T s_k, b < B -- a sensor's noise map, a brush mask, depth-dependent blur. weights [B, m], a bank of
        responses ordered by strength (exp(-t_b lam), 1 / (1 + t_b lam), a gain ladder; B in 2 .. BLEND_MAX_SLOTS), ident a float or
        [B]; level device float32 [H, W] in units of the bank index (a strength in [0, 1] is level = strength * (B - 1)): an
        integer level b gives apply's output for response b, bit for bit, and a level between two integers their linear blend.
        One project_wide, the scaling on the host, one blend with the planes as identity planes (a pass over Phi per
        BLEND_MAX_SLOTS // B planes) -> device float32 [nplanes, H, W]."""
        wts = np.asarray(weights, dtype=np.float64)
        m = self.info["m"]
        if wts.ndim != 2 or wts.shape[1] != m or not 2 <= wts.shape[0] <= BLEND_MAX_SLOTS:
            raise ValueError("weights must be [B, %d] with B in 2 .. %d (BLEND_MAX_SLOTS), got %s" % (m, BLEND_MAX_SLOTS, wts.shape))
        nplanes = planes.shape[0]
        c = self.project_wide(planes)
        a = wts[None, :, :] * c[:, None, :]
        idn = np.broadcast_to(np.asarray(ident, dtype=np.float32), (wts.shape[0],))
        return self.blend(a, level, idn[None, :], np.arange(nplanes, dtype=np.int32)[:, None], planes)

    def gather(self, coeffs, labels, out=None):
        """The piecewise render out(px) = Phi[px] . coeffs[labels(px)] in one pass over Phi: blend with the labels as the level map.
        coeffs [k, m], 2 <= k <= BLEND_MAX_SLOTS; labels device int32 [H, W] (segment's, classify's), converted to float32; a label
        below 0 reads row 0, one above k - 1 the last -> device float32 [H, W] (out: a contiguous tensor of that shape to write into)."""
        a = np.asarray(coeffs, dtype=np.float64)
        if a.ndim != 2 or not 2 <= a.shape[0] <= BLEND_MAX_SLOTS:
            raise ValueError("coeffs must be [k, %d] with k in 2 .. %d (BLEND_MAX_SLOTS), got %s" % (self.info["m"], BLEND_MAX_SLOTS, a.shape))
        t = self.ctx.torch
        labels = self._labels(labels, "labels")
        with t.cuda.stream(self.ctx.stream):
            level = labels.to(t.float32)
        return self.blend(a, level, out=None if out is None else out[None])[0]

    def fit_piecewise(self, planes, labels, k, weight=None, smooth=0.0, ridge=0.0):
        """One fit per segment, rendered piecewise: for every label j < k, fit's system under the weight w * (labels == j) (one
        normal_equations -- beyond 4 planes normal_equations and project_wide, as in fit -- and fit_coeffs under fit's penalty rule),
        then one gather per plane. planes device float32 [nplanes, H, W], labels device int32 [H, W], 2 <= k <= BLEND_MAX_SLOTS,
        weight device float32 [H, W] or None. A label whose system is refused (an empty segment) keeps zero coefficients.
        -> (device float32 [nplanes, H, W], coefficients numpy [nplanes, k, m])."""
        t = self.ctx.torch
        k = int(k)
        if not 2 <= k <= BLEND_MAX_SLOTS:
            raise ValueError("fit_piecewise takes 2 .. %d segments (BLEND_MAX_SLOTS), got %d" % (BLEND_MAX_SLOTS, k))
        planes = self._planes(planes)
        labels = self._labels(labels, "labels")
        if weight is not None:
            weight = self._weight(weight)
        nplanes, m = planes.shape[0], self.info["m"]
        a = np.zeros((nplanes, k, m), dtype=np.float64)
        for j in range(k):
            with t.cuda.stream(self.ctx.stream):
                wj = (labels == j).to(t.float32)
                if weight is not None:
                    wj = wj * weight
            if nplanes > MAX_SIGNALS:
                G = self.normal_equations(wj)[0]
                b = self.project_wide(planes, wj)
            else:
                G, b = self.normal_equations(wj, planes)
            try:
                a[:, j, :] = fit_coeffs(G, b, (float(ridge) + float(smooth) * self.eigenvalues) * (np.trace(G) / m))
            except GlfError:
                pass
        with t.cuda.stream(self.ctx.stream):
            out = t.empty((nplanes, self.info["height"], self.info["width"]), dtype=t.float32, device=self.ctx.device)
        for p in range(nplanes):
            self.gather(a[p], labels, out=out[p])
        return out, a


@functools.lru_cache(maxsize=256)
def _realised(w, h, req, random):
    return max(req, 1) * 2 + 64 if random else int(Sampling(w, h, req).size)


def _realised_samples(w, h, opt):
    """An upper bound of the sample count a call realises (the size of its eigenvalue array): hpc/sampling.c's rule for the
    uniform sampler (which rewrites the request), the request with margin for the random one; cached per image size and request."""
    req = int(opt.num_samples) if opt.num_samples else int(h * w * opt.sample_frac)
    return _realised(w, h, req, bool(getattr(opt, "sampling", 0)))


def _pix_shape_ok(f, a):
    """a (numpy array or tensor) is [H, W] of a one-channel format f, [H, W, 3] of a three-channel one."""
    return len(a.shape) == 3 and a.shape[2] == 3 if f.channels == 3 else len(a.shape) == 2


def _info(st, lam):
    """The info dict of one call (one rank) from its glf_stats and the eigenvalue array."""
    e = st.eig
    return dict(p=st.p, m=st.m, alpha=st.alpha, outer_its=e.outer_its, inner_its_total=e.inner_its_total, residual=e.residual,
                ms_affinity=st.ms_affinity, ms_laplacian=st.ms_laplacian, ms_eigen=st.ms_eigen, ms_nystroem=st.ms_nystroem,
                ms_filter=st.ms_filter, ms_total=st.ms_total, nystroem_kernel_ms=st.nystroem_kernel_ms,
                nystroem_launches=st.nystroem_launches, row0=st.row0, row1=st.row1, contraction=st.contraction,
                skip_exact_zeros=st.skip_exact_zeros, nystroem_evaluated=st.nystroem_evaluated, degree_evaluated=st.degree_evaluated,
                nystroem_mfma_flops=st.nystroem_mfma_flops, nystroem_path=st.nystroem_path, matvec_path=st.matvec_path,
                nystroem_rowpass_launches=st.nystroem_rowpass_launches, nystroem_rowpass_ms=st.nystroem_rowpass_ms,
                nystroem_rowpass_flops=st.nystroem_rowpass_flops, nystroem_colpass_launches=st.nystroem_colpass_launches,
                nystroem_colpass_ms=st.nystroem_colpass_ms, nystroem_colpass_flops=st.nystroem_colpass_flops, rank_terms=st.rank_terms,
                filter_fused=st.filter_fused, eigen_sharded=st.eigen_sharded, matvecs=e.matvecs, matvec_ms=e.matvec_ms,
                matvec_bytes=e.matvec_bytes, narrow_sweeps=e.narrow_sweeps, eigvals=lam[:st.m].copy())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def image_processing_batch(contexts, d_imgs, opt=None):
    """Throughput mode (glf_image_processing_batch; BASELINE config 5): d_imgs is a device uint8 tensor
    [tiles, H, W]; the contexts (each on its own stream, none with a comm) filter the tiles concurrently.
    Returns (outputs [tiles, H, W] uint8, list of per-tile dicts p / m / outer_its / ms_total)."""
    ctx0 = contexts[0]
    torch = ctx0.torch
    assert d_imgs.dtype == torch.uint8 and d_imgs.is_cuda and d_imgs.dim() == 3 and d_imgs.is_contiguous()
    t, h, w = d_imgs.shape
    opt = opt or default_options()
    outs = torch.zeros((t, h, w), dtype=torch.uint8, device=ctx0.device)
    torch.cuda.synchronize(ctx0.device)      # inputs and the zero fill are complete before any context's stream starts
    stats = (Stats * max(1, t))()
    handles = (C.c_void_p * len(contexts))(*[c._ctx for c in contexts])
    rc = _lib.glf_image_processing_batch(handles, C.c_int(len(contexts)), C.byref(opt), C.c_void_p(d_imgs.data_ptr()),
                                         C.c_int(w), C.c_int(h), C.c_int(t), C.c_void_p(outs.data_ptr()), None, stats)
    ctx0._check(rc, "image_processing_batch")
    for c in contexts:
        c.stream.synchronize()
    infos = [dict(p=stats[i].p, m=stats[i].m, alpha=stats[i].alpha, outer_its=stats[i].eig.outer_its,
                  ms_total=stats[i].ms_total) for i in range(t)]
    return outs, infos

