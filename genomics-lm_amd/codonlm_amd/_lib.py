"""ctypes binding of libcodonlm_hip.so (include/codonlm_hip.h).

The library is the product path: if it is missing or fails to load this module raises
immediately -- there is no CPU or PyTorch fallback anywhere in ``codonlm_amd``.
torch is imported first so the HIP runtime the .so binds to (libamdhip64.so.7) is the
one PyTorch already loaded (same SONAME => one runtime, shared streams and memory).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch  # noqa: F401  -- must precede the CDLL load (shared HIP runtime)

# CG_LIB_PATH: load another build of the same library (same-box A/B of two builds)
LIB_PATH = Path(os.environ.get("CG_LIB_PATH") or Path(__file__).resolve().parent / "libcodonlm_hip.so")

CG_F32, CG_BF16, CG_BF16X2 = 0, 1, 2
CG_OK, CG_EINVAL, CG_EUNSUPPORTED, CG_ELAUNCH = 0, -1, -2, -3
EPI_BIAS, EPI_GELU, EPI_DGELU, EPI_RESID, EPI_DROPOUT, EPI_ACCUM, EPI_COLSUM = 1, 2, 4, 8, 16, 32, 64
EPI_SWIGLU, EPI_DSWIGLU = 128, 256
EPI_GELU_DERIV = 512  # GELU: aux_out = gelu'(v); DGELU: aux holds gelu' (out = v * aux)
EPI_ROPE = 1024  # rotate-half RoPE of the q / k head columns after the bias (loader-wave tile only)
# cg_gemm_desc.tile: automatic, or one bf16 kernel forced (tests / A/B runs)
TILE_AUTO, TILE_VEC, TILE_WIDE, TILE_PERS, TILE_PERS_LW = range(5)
(PROBE_NONE, PROBE_GEMM_DW, PROBE_GEMM_FWD, PROBE_GEMM_DX, PROBE_ATTN_FWD, PROBE_ATTN_DQ, PROBE_ATTN_DKDV,
 PROBE_GEMM_DW_GROUPED, PROBE_GEMM_PERS, PROBE_ATTN_BWD, PROBE_DW_SLAB) = range(11)
PROBE_NAMES = {PROBE_GEMM_DW: "gemm_bf16_dW", PROBE_GEMM_FWD: "gemm_bf16_fwd", PROBE_GEMM_DX: "gemm_bf16_dX",
               PROBE_ATTN_FWD: "attn_fwd_mfma", PROBE_ATTN_DQ: "attn_bwd_dq_mfma",
               PROBE_ATTN_DKDV: "attn_bwd_dkdv_mfma", PROBE_GEMM_DW_GROUPED: "gemm_dw_grouped",
               PROBE_GEMM_PERS: "gemm_bf16_pers", PROBE_ATTN_BWD: "attn_bwd_fused_mfma",
               PROBE_DW_SLAB: "dw_slab_reduce"}
# rocprofv3 kernel-name prefixes of the probed kernel classes (every instantiation whose name
# starts with the prefix belongs to the class; bench.py / tools/kstats.py sum them)
PROBE_KERNELS = {PROBE_GEMM_DW_GROUPED: ("gemm_dw_kernel",), PROBE_ATTN_FWD: ("attn_fwd_mfma",),
                 PROBE_ATTN_DQ: ("attn_bwd_dq_mfma",), PROBE_ATTN_DKDV: ("attn_bwd_dkdv_mfma",),
                 PROBE_ATTN_BWD: ("attn_bwd_fused_mfma",),
                 # the persistent forward / dX class: the eight-wave kernel and its loader-wave
                 # variant, both launched through cg_gemm's persistent path, probed together
                 PROBE_GEMM_PERS: ("gemm_bf16_pers_kernel", "gemm_bf16_lw_kernel")}

# parameter kinds (enum in the header)
(P_TOK_EMB, P_POS_EMB, P_LN1_W, P_LN1_B, P_Q_W, P_K_W, P_V_W, P_Q_B, P_K_B, P_V_B, P_PROJ_W,
 P_PROJ_B, P_LN2_W, P_LN2_B, P_FC1_W, P_FC1_B, P_FC2_W, P_FC2_B, P_GATE_W, P_UP_W, P_DOWN_W,
 P_LNF_W, P_LNF_B, P_HEAD_W, P_TERM_W, P_TERM_B, P_OFF1_W, P_OFF1_B, P_OFF2_W, P_OFF2_B, P_NKINDS) = range(31)

vp = C.c_void_p
i32, i64, f32, u32, sz = C.c_int, C.c_longlong, C.c_float, C.c_uint32, C.c_size_t


class GemmDesc(C.Structure):
    _fields_ = [("in_dtype", i32), ("c_dtype", i32), ("M", i32), ("N", i32), ("K", i32),
                ("A", vp), ("lda", i64), ("a_kcontig", i32),
                ("B", vp), ("ldb", i64), ("b_kcontig", i32),
                ("C", vp), ("ldc", i64), ("epilogue", i32), ("alpha", f32),
                ("bias", vp), ("resid", vp), ("ldr", i64),
                ("aux", vp), ("aux_out", vp), ("ld_aux", i64),
                ("drop_seed", u32), ("drop_p", f32), ("split_k", i32), ("workspace", vp),
                ("n_valid", i32), ("ws_bytes", sz),
                ("rope_cos", vp), ("rope_sin", vp), ("rope_T", i32), ("rope_hd", i32), ("rope_heads", i32),
                ("tile", i32), ("max_wg", i32)]


DW_MAX = 32


class DwProduct(C.Structure):
    _fields_ = [("A", vp), ("lda", i64), ("B", vp), ("ldb", i64), ("C", vp), ("ldc", i64),
                ("N_out", i32), ("K_out", i32), ("alpha", f32), ("accumulate", i32), ("col_sum", vp)]


class DwGroup(C.Structure):
    _fields_ = [("n", i32), ("K", i32), ("tile_m", i32), ("p", DwProduct * DW_MAX),
                ("ksplit", i32), ("workspace", vp), ("ws_bytes", sz), ("max_wg", i32)]


REDUCE_MAX = 48


class ReduceJob(C.Structure):
    _fields_ = [("part", vp), ("ld", i64), ("nrows", i32), ("cols", i32), ("dst", vp), ("accumulate", i32),
                ("first_block", i32)]


class ReduceBatch(C.Structure):
    _fields_ = [("n", i32), ("j", ReduceJob * REDUCE_MAX)]


class AdamwSegment(C.Structure):
    _fields_ = [("begin", i64), ("end", i64), ("lr", f32), ("wd", f32)]


TRANSPOSE_MAX = 64


class TransposeItem(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("lds", i64), ("ldd", i64), ("rows", i32), ("cols", i32)]


class TransposeBatch(C.Structure):
    _fields_ = [("n", i32), ("items", TransposeItem * TRANSPOSE_MAX)]


class ModelOpts(C.Structure):
    """cg_model_opts: all zero = the measured defaults"""
    _fields_ = [("dw_group", i32), ("dw_ksplit", i32), ("dw_remainder_first", i32), ("head_dw_separate", i32),
                ("rope_tables", i32), ("attn_mask_kernel", i32), ("dw_plan_tokens", i32), ("attn_bwd_algo", i32),
                ("pers_max_wg", i32)]


class ModelCfg(C.Structure):
    _fields_ = [("vocab_size", i32), ("block_size", i32), ("n_layer", i32), ("n_head", i32),
                ("n_kv_head", i32), ("n_embd", i32), ("use_swiglu", i32), ("use_rope", i32),
                ("sep_id", i32), ("tie_embeddings", i32), ("termination_aux", i32),
                ("termination_n_classes", i32), ("n_offsets", i32), ("offsets", i32 * 8),
                ("dropout", f32), ("label_smoothing", f32), ("ln_eps", f32), ("dtype", i32), ("opts", ModelOpts)]


class ParamEntry(C.Structure):
    _fields_ = [("kind", i32), ("layer", i32), ("offset", i64), ("rows", i32), ("cols", i32), ("ld", i64)]


class Model(C.Structure):
    _fields_ = [("cfg", ModelCfg), ("params", vp), ("shadow", vp), ("grads", vp),
                ("loss_weights", vp), ("rope_cos", vp), ("rope_sin", vp),
                ("workspace", vp), ("workspace_bytes", sz),
                ("B", i32), ("T", i32), ("training", i32), ("window", i32), ("seed", u32),
                ("idx", vp), ("targets", vp), ("logits", vp),
                ("aux_ready", i32), ("head_grad_scale", f32), ("head_grad_scale_dev", vp), ("d_term_logits", vp),
                ("ld_d_term", i64),
                ("d_offset_logits", vp * 8), ("dw_done_layer", i32),
                ("head_dw_off", i64), ("head_dw_alpha", f32), ("head_dw_accumulate", i32), ("head_dw_pending", i32),
                ("reduce_pending", ReduceBatch),
                ("term_fused", i32), ("term_labels", vp), ("term_class_w", vp), ("term_scale", f32),
                ("term_scale_dev", vp)]


# cg_sample_step: token classes, sequence flags, parameters and the per-sequence state
TOK_CODON, TOK_STOP, TOK_EOS = 1, 2, 4
(GEN_DONE, GEN_TERMINAL_STOP, GEN_EARLY_STOP, GEN_EOS, GEN_TARGET, GEN_CAP, GEN_CONTEXT_FULL) = (1, 2, 4, 8, 16, 32, 64)
INT_MAX = 2 ** 31 - 1


class SampleParams(C.Structure):
    _fields_ = [("V", i32), ("tok_class", vp), ("allowed", vp), ("temperature", f32), ("topk", i32),
                ("target_codons", i32), ("max_codons", i32), ("max_tokens", i32),
                ("require_terminal_stop", i32), ("stop_on_eos", i32), ("stop_on_bio_stop", i32),
                ("stop_bias", f32), ("trigger_class_max", i32), ("bias_window", i32), ("n_term_classes", i32),
                ("seed", u32), ("Tmax", i32)]


class GenState(C.Structure):
    _fields_ = [("pos0", C.c_int32), ("pos", C.c_int32), ("n_tokens", C.c_int32), ("n_codons", C.c_int32),
                ("flags", C.c_int32), ("bias_steps", C.c_int32), ("last_term_class", C.c_int32),
                ("stream", u32)]


GEN_STATE_FIELDS = tuple(f for f, _ in GenState._fields_)  # the int32 columns of a (B, 8) state tensor

GEN_PLAN_END = 128  # cg_sample_step_plan: the sequence's plan was used up


class SamplePlan(C.Structure):
    """cg_sample_plan: per-step token sets and the drawn tokens' log-probabilities"""
    _fields_ = [("sets", vp), ("n_sets", i32), ("ld_sets", i64), ("plan", vp), ("ld_plan", i64),
                ("plan_len", vp), ("end_with_plan", i32), ("logp", vp), ("tok_logp", vp), ("ld_tok_logp", i64)]


class OffsetPrior(C.Structure):
    """cg_offset_prior: the offset heads of a step (indices into cfg.offsets) and their weights, in order"""
    _fields_ = [("n", i32), ("head", i32 * 8), ("weight", f32 * 8)]


class ScoreDesc(C.Structure):
    """cg_score_desc: every output pointer optional (None = not wanted)"""
    _fields_ = [("logits", vp), ("ldl", i64), ("rows", i32), ("V", i32), ("targets", vp), ("ignore_index", i32),
                ("smoothing", f32), ("lse", vp), ("logp", vp), ("entropy", vp), ("argmax", vp), ("rank", vp),
                ("sel", vp), ("n_sel", i32), ("delta", vp), ("ld_delta", i64), ("T", i32),
                ("seq_logp", vp), ("seq_count", vp), ("acc", vp), ("workspace", vp), ("ws_bytes", sz)]


ATTR_LOGPROB, ATTR_LOGIT = 0, 1  # cg_attr_seed / cg_attr_desc.mode


class AttrDesc(C.Structure):
    """cg_attr_desc: the seed (y None = the forward's own loss) and the optional outputs"""
    _fields_ = [("y", vp), ("w", vp), ("mode", i32), ("gxt", vp), ("gxi", vp), ("gnorm", vp),
                ("dx0", vp), ("ld_dx0", i64)]


KMEANS_CHUNK = 4096  # CG_KMEANS_CHUNK: the rows one fp32 partial of cg_kmeans_step's statistics covers


class KMeansDesc(C.Structure):
    """cg_kmeans_desc: dist2, sums (with counts) and inertia are optional (None = not wanted)"""
    _fields_ = [("x", vp), ("ldx", i64), ("n", i64), ("d", i32), ("centers", vp), ("ldc", i64), ("k", i32),
                ("labels", vp), ("dist2", vp), ("sums", vp), ("counts", vp), ("inertia", vp),
                ("workspace", vp), ("ws_bytes", sz)]


TERM_CE_MAX_CLASSES = 16  # cg_term_ce_fwd / _bwd: more classes are CG_EUNSUPPORTED


class TermCeDesc(C.Structure):
    """cg_term_ce_desc: loss, sums, dW, db and dx are optional (None = not wanted)"""
    _fields_ = [("x_dtype", i32), ("x", vp), ("ldx", i64), ("rows", i64), ("d", i32), ("C", i32),
                ("W", vp), ("ldw", i64), ("bias", vp), ("labels", vp), ("ignore_index", i32), ("class_w", vp),
                ("loss", vp), ("sums", vp), ("scale", f32), ("scale_dev", vp),
                ("dW", vp), ("lddw", i64), ("acc_dW", i32), ("db", vp), ("acc_db", i32),
                ("dx", vp), ("lddx", i64), ("acc_dx", i32), ("workspace", vp), ("ws_bytes", sz)]


NGRAM_MAX_V = 128  # CG_NGRAM_MAX_V: the dense trigram table is V^3 int64
# cg_diag_rows: the slice order of the CG_DIAG_* enumerators, under the reference's report names
DIAG_SLICES = ("all", "after_separator", "window_with_chunk_continuation", "window_without_chunk_continuation",
               "segment_position_0", "segment_position_1_3", "segment_position_4_15", "segment_position_16_63",
               "segment_position_64_plus", "target_class_special", "target_class_start_codon",
               "target_class_stop_codon", "target_class_ordinary_codon")
DIAG_CLS_SPECIAL, DIAG_CLS_START, DIAG_CLS_STOP, DIAG_CLS_ORDINARY = range(4)
DIAG_MAX_BINS = 32


class NgramNllDesc(C.Structure):
    """cg_ngram_nll_desc: tok_tri, row_sums, row_count and acc are optional (None = not wanted)"""
    _fields_ = [("x", vp), ("y", vp), ("B", i32), ("T", i32), ("V", i32), ("pad_id", i32),
                ("reset_mask", C.POINTER(u32)), ("alpha", C.c_double),
                ("uni", vp), ("bi", vp), ("tri", vp), ("uni_total", vp), ("bi_total", vp), ("tri_total", vp),
                ("tok_tri", vp), ("row_sums", vp), ("row_count", vp), ("acc", vp),
                ("workspace", vp), ("ws_bytes", sz)]


class DiagDesc(C.Structure):
    """cg_diag_desc: every output pointer optional (None = not wanted)"""
    _fields_ = [("logits", vp), ("ldl", i64), ("x", vp), ("y", vp),
                ("B", i32), ("T", i32), ("V", i32), ("pad_id", i32), ("sep_id", i32),
                ("row_flag", vp), ("tok_class", vp), ("edges", vp), ("n_bins", i32),
                ("slices", vp), ("calib", vp), ("brier_acc", vp),
                ("nll", vp), ("segpos", vp), ("conf", vp), ("row_nll", vp), ("row_count", vp),
                ("workspace", vp), ("ws_bytes", sz)]


# cg_attn_stats: the statistic order of the CG_AS_* enumerators
AS_STATS = ("entropy", "norm_entropy", "mass_special", "mass_start", "mass_stop", "mass_ordinary",
            "dist_0", "dist_1_3", "dist_4_15", "dist_16_63", "dist_64_plus", "mean_dist", "max_prob", "first")
(AS_ENTROPY, AS_NORM_ENTROPY, AS_MASS_SPECIAL, AS_MASS_START, AS_MASS_STOP, AS_MASS_ORDINARY, AS_DIST_0, AS_DIST_1_3,
 AS_DIST_4_15, AS_DIST_16_63, AS_DIST_64_PLUS, AS_MEAN_DIST, AS_MAX_PROB, AS_FIRST) = range(14)
AS_NSTAT = 14


class AttnStatsDesc(C.Structure):
    """cg_attn_stats_desc: every output pointer optional (None = not wanted)"""
    _fields_ = [("dtype", i32), ("qkv", vp), ("ldqkv", i64), ("segstart", vp),
                ("B", i32), ("T", i32), ("H", i32), ("KV", i32), ("hd", i32), ("window", i32),
                ("idx", vp), ("pad_id", i32), ("tok_class", vp), ("V", i32), ("row_keep", vp),
                ("rows", vp), ("nvis", vp), ("received", vp), ("head_acc", vp), ("n_rows", vp),
                ("workspace", vp), ("ws_bytes", sz)]


NGRAM_INDEX_MAX_N = 32  # CG_NGRAM_INDEX_MAX_N: the longest window of cg_ngram_index_build
NGRAM_INDEX_MAX_SYM = 2 ** 32 - 2  # CG_NGRAM_INDEX_MAX_SYM: 0xFFFFFFFF is the table's empty slot
NGRAM_MAX_QUERY = 16384  # CG_NGRAM_MAX_QUERY: the longest query of cg_ngram_coverage
NGRAM_INDEX_EMPTY = 0xFFFFFFFF


class NgramIndexDesc(C.Structure):
    """cg_ngram_index_desc: n_unique and n_dropped are optional (None = not wanted)"""
    _fields_ = [("sym", vp), ("n_sym", i64), ("offsets", vp), ("n_seq", i32), ("seq_lo", i32), ("seq_hi", i32),
                ("n", i32), ("table", vp), ("capacity", i64), ("n_unique", vp), ("n_dropped", vp)]


class NgramCoverageDesc(C.Structure):
    """cg_ngram_coverage_desc: hit, n_hit and covered are optional (None = not wanted)"""
    _fields_ = [("sym", vp), ("n_sym", i64), ("n", i32), ("table", vp), ("capacity", i64),
                ("qsym", vp), ("n_qsym", i64), ("qoffsets", vp), ("n_q", i32), ("max_qlen", i32),
                ("hit", vp), ("n_hit", vp), ("covered", vp)]


SHAPE_TARGETS = 14  # CG_SHAPE_TARGETS: the DNAshape columns cg_shape_targets writes per position

# header struct name -> ctypes mirror, for every `typedef struct { ... } cg_x;` of include/codonlm_hip.h
# (tests/test_binding_cpu.py compares sizes, field names, order and kinds with the header)
STRUCTS = {
    "cg_gemm_desc": GemmDesc, "cg_dw_product": DwProduct, "cg_dw_group": DwGroup, "cg_reduce_job": ReduceJob,
    "cg_reduce_batch": ReduceBatch, "cg_transpose_item": TransposeItem, "cg_transpose_batch": TransposeBatch,
    "cg_adamw_segment": AdamwSegment, "cg_model_opts": ModelOpts, "cg_model_cfg": ModelCfg,
    "cg_param_entry": ParamEntry, "cg_model": Model, "cg_offset_prior": OffsetPrior,
    "cg_sample_params": SampleParams, "cg_gen_state": GenState, "cg_sample_plan": SamplePlan,
    "cg_score_desc": ScoreDesc, "cg_attr_desc": AttrDesc, "cg_kmeans_desc": KMeansDesc,
    "cg_term_ce_desc": TermCeDesc, "cg_ngram_nll_desc": NgramNllDesc, "cg_diag_desc": DiagDesc,
    "cg_attn_stats_desc": AttnStatsDesc, "cg_ngram_index_desc": NgramIndexDesc,
    "cg_ngram_coverage_desc": NgramCoverageDesc,
}

# name -> (restype, argtypes) for every symbol include/codonlm_hip.h declares
SIGNATURES = {
    "cg_gemm": (i32, [C.POINTER(GemmDesc), vp]),
    "cg_struct_bytes": (sz, [C.c_char_p]),
    "cg_pers_cus": (i32, []),
    "cg_diag_occupy": (i32, [i32, i32, vp]),
    "cg_gemm_dw_grouped_workspace": (sz, [C.POINTER(DwGroup)]),
    "cg_gemm_dw_grouped": (i32, [C.POINTER(DwGroup), vp]),
    "cg_gemm_dw_tiles": (i32, [i32, i32, i32]),
    "cg_layernorm_fwd": (i32, [i32, vp, i64, vp, vp, vp, i64, vp, vp, i32, i32, f32, vp]),
    "cg_layernorm_fwd_mask": (i32, [i32, vp, i64, vp, vp, vp, i64, vp, vp, i32, i32, f32, i32, i32, i32, u32, f32, vp,
                                    vp]),
    "cg_layernorm_bwd_blocks": (i32, [i32]),
    "cg_layernorm_bwd_workspace": (sz, [i32, i32, i32]),
    "cg_layernorm_bwd": (i32, [i32, vp, i64, vp, i64, vp, vp, vp, vp, vp, i32, vp, u32, f32, vp, sz, vp, vp,
                               vp, i32, i32, i32, f32, vp]),
    "cg_layernorm_bwd_partials": (i32, [i32, vp, i64, vp, i64, vp, vp, vp, vp, vp, i32, vp, u32, f32, vp, sz, i32,
                                        i32, i32, vp]),
    "cg_reduce_columns": (i32, [C.POINTER(ReduceBatch), vp]),
    "cg_embed_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, u32, f32, vp]),
    "cg_embed_bwd_workspace": (sz, [i32, i32, i32, i32]),
    "cg_embed_bwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, u32, f32, i32, vp, sz, vp]),
    "cg_segment_starts": (i32, [vp, vp, i32, i32, i32, vp]),
    "cg_rope_tab": (i32, [i32, vp, i64, i32, i32, i32, i32, i32, vp, vp, i32, vp]),
    "cg_attn_fwd": (i32, [i32, vp, i64, vp, vp, i64, vp, i32, i32, i32, i32, i32, i32, u32, f32, vp, vp]),
    "cg_attn_drop_mask_bytes": (sz, [i32, i32, i32]),
    "cg_attn_drop_mask": (i32, [i32, i32, i32, u32, f32, vp, vp]),
    "cg_attn_fwd_keep": (i32, [i32, vp, i64, vp, vp, i64, vp, i32, i32, i32, i32, i32, i32, u32, f32, vp, vp]),
    "cg_attn_probs": (i32, [i32, vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "cg_attn_bwd_workspace": (sz, [i32, i32, i32]),
    "cg_attn_bwd": (i32, [i32, vp, i64, vp, vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, i32, i32, i32,
                          u32, f32, vp, vp, i64, vp, sz, vp]),
    "cg_attn_bwd_rope": (i32, [i32, vp, i64, vp, vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, i32, i32, i32,
                               u32, f32, vp, vp, i64, vp, vp, vp, sz, vp]),
    "cg_attn_bwd_algo": (i32, [i32, i32, vp, i64, vp, vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, i32, i32, i32,
                               u32, f32, vp, vp, i64, vp, vp, vp, sz, vp]),
    "cg_ce_workspace": (sz, [i32]),
    "cg_cross_entropy": (i32, [vp, i64, vp, i32, i32, f32, vp, i32, f32, i32, vp, i64, vp, vp, sz, vp]),
    "cg_swiglu_fwd": (i32, [i32, vp, i64, i32, vp, i64, i32, i32, vp]),
    "cg_swiglu_bwd": (i32, [i32, vp, i64, i32, vp, i64, vp, i64, i32, i32, vp]),
    "cg_colsum_workspace": (sz, [i32, i32]),
    "cg_colsum": (i32, [i32, vp, i64, i32, i32, vp, i32, vp, sz, vp]),
    "cg_colsum_reduce": (i32, [vp, i32, i32, vp, i32, vp]),
    "cg_colsum_partials": (i32, [i32, vp, i64, i32, i32, vp, sz, C.POINTER(i32), vp]),
    "cg_cast_f32_to_bf16": (i32, [vp, vp, i64, vp]),
    "cg_transpose16_batch": (i32, [C.POINTER(TransposeBatch), vp]),
    "cg_cast_bf16_to_f32": (i32, [vp, vp, i64, vp]),
    "cg_cast_pad_2d": (i32, [vp, i64, i32, i32, i32, vp, i64, i32, vp]),
    "cg_scale_dev": (i32, [i32, vp, i64, i32, i32, vp, vp]),
    "cg_gather_windows": (i32, [i32, vp, i64, i64, vp, i32, i32, vp, vp]),
    "cg_gather_sequences": (i32, [i32, vp, vp, vp, i64, vp, i32, i32, vp, vp, vp]),
    "cg_pool_hidden": (i32, [i32, vp, i64, vp, i32, i32, i32, i32, i32, C.POINTER(u32), vp, vp]),
    "cg_offset_targets":(i32, [vp, i32, i32, i32, C.POINTER(i32), i32, vp, vp, vp]),
    "cg_termination_labels": (i32, [vp, i32, i32, C.POINTER(i32), i32, C.POINTER(i32), i32, i32, vp, vp]),
    "cg_adamw": (i32, [vp, vp, vp, vp, vp, C.POINTER(AdamwSegment), i32, f32, f32, f32, i32, f32, vp]),
    "cg_nonfinite_flag": (i32, [vp, i64, vp, vp]),
    "cg_model_param_layout": (i32, [C.POINTER(ModelCfg), C.POINTER(ParamEntry), i32, C.POINTER(i64)]),
    "cg_model_workspace_bytes": (sz, [C.POINTER(ModelCfg), i32, i32]),
    "cg_model_dw_plan": (i32, [C.POINTER(ModelCfg), i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "cg_model_forward": (i32, [C.POINTER(Model), vp, vp, i32, i32, i32, u32, i32, vp, vp, vp]),
    "cg_model_aux_forward": (i32, [C.POINTER(Model), vp, i64, C.POINTER(vp), i64, vp]),
    "cg_model_backward": (i32, [C.POINTER(Model), i32, i32, i32, vp]),
    "cg_kv_cache_bytes": (sz, [C.POINTER(ModelCfg), i32, i32]),
    "cg_decode_workspace_bytes": (sz, [C.POINTER(ModelCfg), i32]),
    "cg_model_prefill": (i32, [C.POINTER(Model), vp, i32, i32, i32, vp, i32, vp, vp, vp]),
    "cg_model_decode": (i32, [C.POINTER(Model), vp, i32, i32, vp, i32, vp, vp, sz, vp, vp]),
    "cg_attn_decode": (i32, [i32, vp, i64, vp, i64, i32, i32, vp, i32, i32, i32, i32, i32, vp, i64, vp]),
    "cg_segstate_step": (i32, [vp, i32, i32, i32, vp, vp]),
    "cg_decode_ragged_workspace_bytes": (sz, [C.POINTER(ModelCfg), i32]),
    "cg_model_prefill_ragged": (i32, [C.POINTER(Model), vp, vp, i32, i32, i32, vp, i32, vp, vp, vp]),
    "cg_model_decode_ragged": (i32, [C.POINTER(Model), vp, vp, i32, vp, i32, vp, vp, sz, vp, vp, i64, vp]),
    "cg_attn_decode_ragged": (i32, [i32, vp, i64, vp, i64, i32, vp, vp, i32, i32, i32, i32, i32, vp, i64, vp]),
    "cg_embed_fwd_pos": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "cg_rope_pos": (i32, [i32, vp, i64, vp, i32, i32, i32, i32, vp, vp, i32, vp]),
    "cg_kv_append": (i32, [i32, vp, i64, vp, i64, i32, vp, i32, i32, vp]),
    "cg_kv_scatter": (i32, [i32, vp, i64, i32, vp, i64, i32, vp, i32, i32, vp]),
    "cg_segstate_step_ragged": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "cg_gather_rows": (i32, [vp, i64, vp, i32, i32, vp, i64, i32, vp, vp, i32, vp]),
    "cg_row_head": (i32, [i32, vp, i64, vp, vp, vp, i32, i32, i32, i32, vp, i64, vp]),
    "cg_xf_hist_bytes": (sz, [C.POINTER(ModelCfg), i32, i32]),
    "cg_model_prefill_hist": (i32, [C.POINTER(Model), vp, i32, i32, vp, i32, vp]),
    "cg_model_decode_ragged_hist": (i32, [C.POINTER(Model), vp, vp, i32, vp, i32, vp, vp, sz, vp, vp, i64, vp, vp]),
    "cg_offset_prior_workspace": (sz, [C.POINTER(ModelCfg), i32]),
    "cg_offset_prior_add": (i32, [C.POINTER(Model), C.POINTER(OffsetPrior), vp, i32, vp, i32, vp, i64, vp, sz, vp]),
    "cg_sample_step": (i32, [C.POINTER(SampleParams), vp, i64, vp, i64, vp, vp, vp, i64, vp, i32, vp]),
    "cg_sample_step_plan": (i32, [C.POINTER(SampleParams), C.POINTER(SamplePlan), vp, i64, vp, i64, vp, vp, vp, i64, vp,
                                  i32, vp]),
    "cg_score_workspace": (sz, [i32]),
    "cg_score_rows": (i32, [C.POINTER(ScoreDesc), vp]),
    "cg_attr_seed": (i32, [vp, i64, vp, vp, i32, i32, i32, i32, vp, i64, vp]),
    "cg_attr_reduce": (i32, [vp, i64, vp, vp, i64, i32, vp, i64, i32, i32, vp, vp, vp, vp]),
    "cg_model_input_grad": (i32, [C.POINTER(Model), C.POINTER(AttrDesc), vp]),
    "cg_window_keep": (i32, [vp, i32, i32, i32, i32, C.POINTER(u32), vp, vp]),
    "cg_window_pool": (i32, [i32, vp, i64, i32, i32, i32, i32, i32, vp, vp, i64, i64, vp]),
    "cg_kmeans_workspace": (sz, [i64, i32, i32]),
    "cg_kmeans_step": (i32, [C.POINTER(KMeansDesc), vp]),
    "cg_term_ce_workspace": (sz, [i64, i32, i32]),
    "cg_term_ce_fwd": (i32, [C.POINTER(TermCeDesc), vp]),
    "cg_term_ce_bwd": (i32, [C.POINTER(TermCeDesc), vp]),
    "cg_ngram_count": (i32, [vp, vp, i32, i32, i32, i32, C.POINTER(u32), vp, vp, vp, vp, vp]),
    "cg_ngram_totals": (i32, [vp, vp, vp, i32, vp, vp, vp, vp]),
    "cg_ngram_nll_workspace": (sz, [i32]),
    "cg_ngram_nll": (i32, [C.POINTER(NgramNllDesc), vp]),
    "cg_diag_workspace": (sz, [i32]),
    "cg_diag_rows": (i32, [C.POINTER(DiagDesc), vp]),
    "cg_attn_stats_workspace": (sz, [i32, i32, i32]),
    "cg_attn_stats": (i32, [C.POINTER(AttnStatsDesc), vp]),
    "cg_model_attn_stats": (i32, [C.POINTER(Model), i32, C.POINTER(AttnStatsDesc), vp]),
    "cg_ngram_index_build": (i32, [C.POINTER(NgramIndexDesc), vp]),
    "cg_ngram_coverage": (i32, [C.POINTER(NgramCoverageDesc), vp]),
    "cg_shape_targets": (i32, [vp, i32, i32, C.POINTER(i32), i32, vp, i64, vp, vp]),
    "cg_gram_workspace": (sz, [i64, i32, i32, i32]),
    "cg_gram_accum": (i32, [i32, vp, i64, i32, vp, i64, i32, vp, i64, i32, i32, vp, i64, vp, sz, vp]),
    "cg_model_forward_trunk": (i32, [C.POINTER(Model), vp, i32, i32, i32, u32, i32, vp]),
    "cg_model_term_loss": (i32, [C.POINTER(Model), vp, vp, vp, vp]),
    "cg_model_backward_heads": (i32, [C.POINTER(Model), i32, vp]),
    "cg_model_hidden": (vp, [C.POINTER(Model), i32, C.POINTER(i32), C.POINTER(i64)]),
    "cg_model_attn_probs": (i32, [C.POINTER(Model), i32, vp, vp]),
    "cg_probe_enable": (i32, [i32]),
    "cg_probe_sample": (i32, [i32]),
    "cg_probe_read": (i32, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64)]),
    "cg_probe_bytes": (i32, [C.POINTER(C.c_double)]),
    "cg_version": (C.c_char_p, []),
}


class LibraryError(RuntimeError):
    pass


def _load():
    if not LIB_PATH.exists():
        raise LibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C genomics-lm_amd/csrc). codonlm_amd has no CPU fallback.")
    lib = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(status: int, what: str) -> None:
    if status == CG_OK:
        return
    if status == CG_EINVAL:
        raise ValueError(f"{what}: invalid argument (CG_EINVAL)")
    if status == CG_EUNSUPPORTED:
        raise ValueError(f"{what}: unsupported shape/dtype (CG_EUNSUPPORTED)")
    raise RuntimeError(f"{what}: kernel launch failed (status {status})")


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor must live on the MI355X (got {t.device}); "
                           "codonlm_amd has no CPU path")
