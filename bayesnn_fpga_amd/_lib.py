"""ctypes binding of libbayesnn_fpga_amd.so (C ABI in include/bayesnn_fpga_amd.h).

There is NO CPU fallback: if the library is missing or cannot be loaded, every product entry
point raises.  Build it with ``python -m bayesnn_fpga_amd._build`` (or ``__graft_entry__.build()``).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libbayesnn_fpga_amd.so")

BMI_OK = 0
SITE_NONE, SITE_ELEMENTWISE, SITE_CHANNEL, SITE_MASKSEMBLE = 0, 1, 2, 3
SITE_POS_OUTER, SITE_POS_INNER = 0, 1
DTYPE_F16, DTYPE_BF16, DTYPE_F32, DTYPE_F16X2, DTYPE_BF16X3 = 0, 1, 2, 3, 4
DTYPES = {"f16": DTYPE_F16, "bf16": DTYPE_BF16, "f32": DTYPE_F32, "f16x2": DTYPE_F16X2, "bf16x3": DTYPE_BF16X3}
FP32_ACT_DTYPES = ("f32", "f16x2", "bf16x3")      # engines that keep fp32 activations in the workspace
OP_STEM, OP_CONV, OP_MASK, OP_HEAD, OP_MAXPOOL, OP_DENSE = 1, 2, 3, 4, 5, 6
STOP_RULES = {"sem": 0, "margin": 1}      # BMI_STOP_* of bmi_forward_mcd_adaptive
VOTE_STOP_RULES = {**STOP_RULES, "votes": 2}      # ... of bmi_forward_mcd_adaptive_votes, which alone takes BMI_STOP_VOTES
EXIT_RULES = {"confidence": 0, "margin": 1}      # BMI_EXIT_* of bmi_forward_mcd_exit_staged
STOP_ON = {"exit": 0, "ensemble": 1}      # BMI_STOP_ON_* of bmi_forward_mcd_adaptive_ensemble
NLL_VEC_SLAB, NLL_VEC_ROWS = 3456, 64       # bmi_nll_vector_scaling_grad stages min(NLL_VEC_ROWS, NLL_VEC_SLAB // (C | 1)) samples per chunk
NLL_MAT_SLAB, NLL_MAT_ROWS = 3456, 64       # bmi_nll_matrix_scaling_grad stages min(NLL_MAT_ROWS, NLL_MAT_SLAB // (C | 1)) samples per chunk
PASS_ACC_MAX_TOPS = 8                       # bmi_pass_accuracy: at most 8 top-k cut-offs per call (K), 128 classes, 32 exits
REL_MAX_BINS = 64                           # BMI_REL_MAX_BINS of bmi_reliability_table: n_bins in [1, 64], fewer than 2^22 images, 128 classes, 32 exits
KDE_MIN_GRID, KDE_MAX_GRID = 16, 65536      # BMI_KDE_* of bmi_reliability_kde: grid points; bw_scale within [2^-100, 2^100]
RANK_TILE_I, RANK_TILE_J = 512, 2048        # BMI_RANK_TILE_* of bmi_rank_quality: images a workgroup ranks / keys it stages in LDS per step
RANK_MAX_IMAGES, RANK_MAX_ROWS = 1 << 17, 1024      # BMI_RANK_MAX_*: longer rows (a radix sort) are not built
RANK_INVALID, RANK_MAX_KEY = 0xFFFFFFFF, 0x7F7FFFFF # the score key of an image that is in no count; the largest valid key (FLT_MAX's bits)
POLICY_MAX_THRESHOLDS, POLICY_MAX_RECORD_ROWS = 1024, 64       # BMI_POLICY_MAX_* of bmi_exit_policy_sweep: thresholds per call / with selected records
NLL_ENS_SLAB, NLL_ENS_ROWS = 9216, 192     # BMI_NLL_ENS_* of bmi_nll_ensemble_temperature_grid: floats / rows a workgroup stages per chunk


class ExitRule(C.Structure):
    _fields_ = [("criterion", C.c_int32), ("ensemble", C.c_int32), ("threshold", C.c_double), ("first_exit", C.c_int32)]

PROFILE_SLOTS = 8
CONV_FAMILY_KERNELS = ("conv3x3_patch_kernel", "conv_igemm_wide_kernel", "conv_igemm_kernel", "conv3x3_pw_kernel", "conv1x1_stream_kernel",
                       "conv3x3_s2_kernel", "conv_split_kernel", "conv1x1_seam_kernel")
ABI_VERSION = 600             # BMI_VERSION of include/bayesnn_fpga_amd.h this binding was written against
CONV_FAMILIES = len(CONV_FAMILY_KERNELS)     # BMI_CONV_FAMILIES
PROFILE_NAMES = {OP_STEM: "stem", OP_CONV: "conv_igemm", OP_MASK: "mask", OP_HEAD: "head", OP_MAXPOOL: "maxpool",
                 OP_DENSE: "dense", 7: "ensemble"}      # 7: BMI_PROFILE_ENSEMBLE (the row-table entry points' ensemble.hip launches)


class Site(C.Structure):
    _fields_ = [("kind", C.c_int32), ("site_id", C.c_int32), ("p", C.c_float), ("num_masks", C.c_int32),
                ("masks", C.c_void_p)]


class HeadEx(C.Structure):
    """bmi_head_ex: one exit head of bmi_head_fused_ex (unit parity tests)."""
    _fields_ = [("in_", C.c_void_p), ("in_is_f32", C.c_int32), ("in_mod", C.c_int32), ("hw", C.c_int32), ("k", C.c_int32),
                ("weight_pad", C.c_void_p), ("bias", C.c_void_p), ("out_dim", C.c_int32), ("site", C.POINTER(Site)),
                ("site_logits", C.POINTER(Site)), ("batch", C.c_int32), ("t0", C.c_int32), ("tc", C.c_int32), ("seed", C.c_uint64),
                ("mask_cnt0", C.c_int32), ("S1", C.c_void_p), ("S2", C.c_void_p), ("SL", C.c_void_p), ("SH", C.c_void_p),
                ("image_map", C.c_void_p), ("n_mapped", C.c_int32), ("image_offset", C.c_int32), ("logits", C.c_void_p),
                ("logits_tstride", C.c_size_t), ("scratch", C.c_void_p), ("inv_tau", C.c_float), ("vec_scale", C.c_void_p),
                ("vec_bias", C.c_void_p), ("mat", C.c_void_p), ("mat_bias", C.c_void_p)]


class TensorDesc(C.Structure):
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32)]


class OpDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("in_", C.c_int32), ("out", C.c_int32), ("residual", C.c_int32), ("in2", C.c_int32),
                ("ksize", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("relu", C.c_int32),
                ("weight", C.c_void_p), ("weight2", C.c_void_p), ("scale", C.c_void_p), ("bias", C.c_void_p), ("site", Site),
                ("bias_post", C.c_void_p), ("site_pos", C.c_int32)]


class ModelDesc(C.Structure):
    _fields_ = [("n_tensors", C.c_int32), ("tensors", C.POINTER(TensorDesc)), ("n_ops", C.c_int32),
                ("ops", C.POINTER(OpDesc)), ("n_exits", C.c_int32), ("out_dim", C.c_int32), ("dtype", C.c_int32)]


class BmiError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        super().__init__(f"{what} failed: {error_string(code)} ({code})")


_lib = None

_PROTOS = {
    "bmi_version": (C.c_int, []),
    "bmi_error_string": (C.c_char_p, [C.c_int]),
    "bmi_set_option": (C.c_int, [C.c_char_p, C.c_int32]),
    "bmi_engine_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "bmi_create": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(C.c_void_p)]),
    "bmi_destroy": (C.c_int, [C.c_void_p]),
    "bmi_plan": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "bmi_query": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                            C.POINTER(C.c_int32)]),
    "bmi_tensor_info": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)] + [C.POINTER(C.c_int32)] * 5),
    "bmi_image_offset_ok": (C.c_int, [C.c_void_p, C.c_int32]),
    "bmi_forward_mcd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_forward_mcd_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_forward_mcd_entropy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_ensemble_scratch_bytes": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "bmi_forward_mcd_ensemble": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32] +
                                 [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_ensemble_moments": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)] + [C.c_void_p] * 4),
    "bmi_ensemble_moments_weighted": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)] + [C.c_void_p] * 5),
    "bmi_engine_set_ensemble_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "bmi_engine_set_vector_scaling": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "bmi_ensemble_moments_vector": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "bmi_nll_vector_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bmi_nll_vector_scaling_grad": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p]),
    "bmi_engine_set_matrix_scaling": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "bmi_ensemble_moments_matrix": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "bmi_nll_matrix_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bmi_nll_matrix_scaling_grad": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p]),
    "bmi_finalize_ensemble": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 10),
    "bmi_finalize_uncertainty": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "bmi_forward_mcd_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_forward_mcd_exit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_double, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_size_t,
                                       C.c_void_p]),
    "bmi_forward_mcd_exit_staged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.POINTER(ExitRule)] +
                                    [C.c_void_p] * 5 + [C.POINTER(C.c_int32), C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_query_op_stages": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.POINTER(C.c_int32)] * 4),
    "bmi_query_exit_stages": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "bmi_forward_mcd_adaptive": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32,
                                           C.c_int32, C.c_double, C.c_int32] + [C.c_void_p] * 6 + [C.POINTER(C.c_int32), C.c_void_p,
                                                                                                   C.c_size_t, C.c_void_p]),
    "bmi_forward_mcd_adaptive_ensemble": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32,
                                                    C.c_int32, C.c_double, C.c_int32, C.c_int32] + [C.c_void_p] * 8 + [C.c_size_t] +
                                          [C.c_void_p] * 2 + [C.POINTER(C.c_int32), C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_forward_mcd_exit_staged_ensemble": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.POINTER(ExitRule)] +
                                             [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_size_t,
                                                                 C.c_void_p]),
    "bmi_finalize_ensemble_per_image": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 11),
    "bmi_finalize_per_image": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 13),
    "bmi_finalize": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p]),
    "bmi_finalize_checked": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "bmi_engine_set_temperature": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int32]),
    "bmi_engine_get_temperature": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int32]),
    "bmi_nll_temperature_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bmi_nll_temperature_grid": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_nll_ensemble_temperature_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bmi_nll_ensemble_temperature_grid": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                    C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_pass_accuracy_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bmi_pass_accuracy": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32] +
                          [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "bmi_reliability_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6),
    "bmi_reliability_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "bmi_reliability_table": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.POINTER(C.c_float)] + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]),
    "bmi_reliability_kde": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.c_double] + [C.c_void_p] * 8),
    "bmi_classwise_record": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4),
    "bmi_classwise_table": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 5 + [C.POINTER(C.c_float)] + [C.c_void_p] * 6),
    "bmi_score_record": (C.c_int, [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 3),
    "bmi_rank_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "bmi_rank_quality": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 3 + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]),
    "bmi_exit_stat_record": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 2),
    "bmi_exit_policy_scratch_bytes": (C.c_size_t, [C.c_int32] * 3),
    "bmi_exit_policy_sweep": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_int32] + [C.c_void_p] * 13 + [C.c_size_t, C.c_void_p]),
    "bmi_forward_mcd_votes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32] +
                              [C.c_void_p] * 10 + [C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_vote_counts": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)] + [C.c_void_p] * 7),
    "bmi_finalize_votes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 5),
    "bmi_vote_counts_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)] + [C.c_void_p] * 5 +
                             [C.c_int32] + [C.c_void_p] * 4),
    "bmi_vote_decide": (C.c_int, [C.c_void_p] + [C.c_int32] * 8 + [C.c_void_p, C.c_int32] + [C.c_void_p] * 4),
    "bmi_forward_mcd_adaptive_votes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32,
                                                 C.c_int32, C.c_double, C.c_int32, C.c_int32] + [C.c_void_p] * 10 + [C.c_size_t] +
                                       [C.c_void_p] * 2 + [C.POINTER(C.c_int32), C.c_void_p, C.c_size_t, C.c_void_p]),
    "bmi_forward_mcd_exit_staged_votes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.POINTER(ExitRule)] +
                                          [C.c_void_p] * 10 + [C.c_size_t, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_size_t,
                                                               C.c_void_p]),
    "bmi_profile_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "bmi_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "bmi_philox_mask": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "bmi_stem_conv_fwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 9 + [C.c_void_p]),
    "bmi_mask_bits": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Site), C.c_int32, C.c_int32, C.c_uint64,
                                C.c_void_p]),
    "bmi_conv_igemm_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 5 + [C.c_int32] * 11 + [C.POINTER(Site), C.c_int32, C.c_int32,
                                                                         C.c_uint64, C.c_int32, C.c_void_p]),
    "bmi_conv3x3_shortcut_fwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 7 + [C.c_void_p]),
    "bmi_profile_launches": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)] + [C.POINTER(C.c_int32)] * 4 + [C.POINTER(C.c_double)] * 3),
    "bmi_profile_conv_families": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double)]),
    "bmi_conv1x1_seam_fwd": (C.c_int, [C.c_void_p] * 10 + [C.c_int32] * 7 + [C.c_void_p]),
    "bmi_conv_pair_fwd": (C.c_int, [C.c_void_p] * 9 + [C.c_int32] * 11 + [C.c_void_p]),
    "bmi_mask_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Site),
                                 C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_void_p]),
    "bmi_maxpool2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "bmi_head_fused": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.POINTER(Site), C.POINTER(Site), C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bmi_head_fused_ex": (C.c_int, [C.POINTER(HeadEx), C.c_int32, C.c_void_p]),
    "bmi_dense_f32": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int32] * 5 +
                      [C.POINTER(Site), C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_void_p]),
}

EXPORTS = tuple(_PROTOS.keys())


def lib():
    """Loads the library (once).  Raises if it is absent — there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP library has not been built "
                "(run `python -m bayesnn_fpga_amd._build`).  bayesnn_fpga_amd has no CPU fallback.")
        # torch first: PyTorch-ROCm ships its own libamdhip64, and the process must end up with ONE HIP runtime.  Loaded
        # before torch, this library binds the system ROCm runtime instead; the streams and device pointers torch
        # hands over then belong to a different runtime and every launch fails (BMI_ERR_HIP).
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        if l.bmi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} reports C-ABI version {l.bmi_version()}, this binding expects {ABI_VERSION}: "
                               "rebuild the library (python -m bayesnn_fpga_amd._build)")
        _lib = l
        # BMI_OPTIONS="name=value,name=value": bmi_set_option pairs applied once at load (profiling arms: rocprofv3 wraps bench.py,
        # which has no option flag of its own)
        for kv in filter(None, os.environ.get("BMI_OPTIONS", "").split(",")):
            nm, _, val = kv.partition("=")
            if l.bmi_set_option(nm.strip().encode(), int(val)) != BMI_OK:
                raise RuntimeError(f"BMI_OPTIONS: bmi_set_option({nm.strip()}, {val}) failed")
    return _lib


def error_string(code):
    return lib().bmi_error_string(int(code)).decode()


def check(code, what):
    if code != BMI_OK:
        raise BmiError(code, what)


def set_option(name, value):
    """Process DEFAULT of a kernel-selection switch (bmi_set_option): e.g. set_option("mfma_shape_patch", 16).  Read by the single-kernel entry
    points and COPIED into every engine created afterwards; a live engine keeps its copy (``MCDEngine.set_option`` edits one engine's)."""
    check(lib().bmi_set_option(name.encode(), int(value)), f"bmi_set_option({name})")


def make_site(kind=SITE_NONE, site_id=0, p=0.0, num_masks=0, masks_ptr=None):
    return Site(int(kind), int(site_id), float(p), int(num_masks), masks_ptr)
