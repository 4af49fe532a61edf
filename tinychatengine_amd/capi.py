"""ctypes binding of libtce_hip.so (include/tce_matmul.h).  Plain pointers and sizes; torch is only used by callers
to own device memory and streams.  Loading fails loudly when the HIP library has not been built: there is no fallback."""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TCE_LIB_PATH") or os.path.join(_PKG, "lib", "libtce_hip.so")  # (TCE_LIB_PATH: another build of the same library, for A/B runs)

TCE_OK = 0
TCE_ERR_BAD_ARG = -1
TCE_ERR_UNSUPPORTED_GROUP = -2
TCE_ERR_UNSUPPORTED_SHAPE = -3
TCE_ERR_HIP = -4
TCE_ERR_UNSUPPORTED_KIND = -5
TCE_W4A16_GEMV_MAX_M = 8
TCE_MAX_GROUP = 4
TCE_W4_FORCE_GEMV = 1
TCE_W4_FORCE_GEMM = 2
TCE_W4_SILU_MUL_PAIRS = 8
TCE_W4_ADD_TO_C = 16
TCE_PLAN_CHAINED = 1
TCE_PLAN_TAGGED = 2
TCE_ABI_VERSION = 113  # include/tce_matmul.h TCE_VERSION: the struct layouts mirrored below
TCE_PLAN_OVERLAPPED = 4
TCE_PLAN_TUNED = 8
TCE_PLAN_INDEPENDENT = 16
TCE_W4_ZERO_POINT_IS_8 = 4
TCE_BIAS_NONE, TCE_BIAS_INT8, TCE_BIAS_FP32 = 0, 1, 2
TCE_OUT_INT8, TCE_OUT_FP32 = 0, 1

# every symbol include/tce_matmul.h declares (tests/test_boundary.py checks the .so exports exactly these)
EXPORTS = [
    "tce_w4a16_forward", "tce_w4a16_residual_rmsnorm_workspace_bytes", "tce_w4a16_forward_residual_rmsnorm", "tce_w4a16_prepack_bytes", "tce_w4a16_prepack", "tce_w4a16_prepack_group_bytes", "tce_w4a16_prepack_group", "tce_w4a16_gemm_scratch_bytes", "tce_w4a16_gemm_scratch_faults", "tce_w4a16_describe_dispatch", "tce_w8a8_describe_dispatch", "tce_reset_last_error", "tce_bmm_f16t", "tce_rope_half", "tce_softmax_half", "tce_attention_decode_f16", "tce_attention_decode_workspace_bytes", "tce_attention_decode_describe", "tce_attention_decode_step_f16", "tce_attention_decode_step_gqa_f16", "tce_attention_decode_describe_gqa", "tce_attention_decode_step_pos_f16", "tce_attention_decode_batch_workspace_bytes", "tce_attention_decode_describe_batch", "tce_attention_decode_step_batch_f16", "tce_kv_pages_pool_bytes", "tce_attention_decode_describe_paged", "tce_attention_decode_step_paged_f16", "tce_kv_pages_scatter_f16", "tce_kv_pages_gather_f16", "tce_kv_block_table_check", "tce_attention_prefill_f16", "tce_attention_prefill_workspace_bytes", "tce_attention_prefill_paged_workspace_bytes", "tce_attention_prefill_paged_f16", "tce_attention_prefill_describe_paged", "tce_kv_pages_pool_bytes_fp8", "tce_attention_decode_step_paged_fp8", "tce_attention_prefill_paged_fp8", "tce_kv_pages_scatter_fp8", "tce_kv_pages_gather_fp8", "tce_sample_workspace_bytes", "tce_sample_f16", "tce_embed_rows_f16", "tce_attention_decode_step_paged_rows_f16", "tce_attention_decode_step_paged_rows_fp8", "tce_attention_decode_describe_paged_window", "tce_attention_decode_step_paged_window_f16", "tce_attention_decode_step_paged_window_fp8", "tce_attention_prefill_paged_window_f16", "tce_attention_prefill_paged_window_fp8", "tce_kv_block_table_check_window", "tce_attention_decode_describe_paged_sink", "tce_attention_decode_step_paged_sink_f16", "tce_attention_decode_step_paged_sink_fp8", "tce_attention_prefill_paged_sink_f16", "tce_attention_prefill_paged_sink_fp8", "tce_kv_block_table_check_sink", "tce_attention_decode_step_paged_rows_window_f16", "tce_attention_decode_step_paged_rows_window_fp8", "tce_attention_decode_step_paged_rows_sink_f16", "tce_attention_decode_step_paged_rows_sink_fp8", "tce_sample_verify_workspace_bytes", "tce_sample_verify_f16", "tce_draft_ngram", "tce_logprobs_workspace_bytes", "tce_sample_logprobs_f16", "tce_sample_verify_logprobs_f16", "tce_sample_constrained_f16", "tce_sample_verify_constrained_f16", "tce_sample_stages_f16", "tce_sample_verify_stages_f16", "tce_sample_mirostat_f16", "tce_sample_verify_mirostat_workspace_bytes", "tce_sample_verify_mirostat_f16", "tce_logprobs_f16", "tce_lora_shrink_f16", "tce_lora_expand_add_f16", "tce_lora_expand_silu_mul_f16", "tce_opt_attention_decode", "tce_prefetch", "tce_add_half", "tce_silu_mul_half", "tce_rmsnorm_half", "tce_w4a16_forward_group_rmsnorm", "tce_w4a16_forward_group", "tce_w4a16_forward_independent", "tce_w4a16_describe_independent", "tce_w4a16_forward_independent_gather", "tce_w4a16_check_zero_point_8", "tce_w4a16_awq_fp16acc", "tce_w4a16_awq_workspace_bytes",
    "tce_w4a16_gemm_awq", "tce_w4a16_shard", "tce_comm_create", "tce_comm_export", "tce_comm_connect", "tce_comm_connect_local", "tce_allgather_f16", "tce_comm_rccl_unique_id", "tce_comm_rccl_init", "tce_allgather_rows_workspace_bytes", "tce_allgather_rows_f16", "tce_comm_status", "tce_comm_set_timeout_ms", "tce_comm_reset", "tce_comm_device", "tce_comm_destroy", "tce_w8a8_matmul", "tce_opt_softmax_q", "tce_opt_kv_append", "tce_layernorm_q", "tce_layernorm_q_w8a8_group", "tce_plan_create", "tce_plan_create_ex", "tce_plan_is_chained", "tce_plan_geometry", "tce_plan_status", "tce_plan_launch_geometry", "tce_plan_launch", "tce_plan_n_launches",
    "tce_w4a16_forward_v2", "tce_w8a8_matmul_v2", "tce_w8a8_scratch_bytes", "tce_attention_decode_step_deferred_f16", "tce_w4a16_forward_deferred_attention", "tce_plan_destroy", "tce_version", "tce_last_error", "tce_build_info", "tce_w4a16_set_gemv_config", "tce_w4a16_set_gemv_i8",
    "tce_w4a16_set_gemm_config", "tce_w4a16_algorithmic_bytes", "tce_w4a16_gemv_variant", "tce_w4a16_gemm_variant",
    "tce_w4a16_set_debug_mode", "tce_attention_set_tuning", "tce_w8a8_set_tuning", "tce_w4a16_set_debug_buffer", "tce_w4a16_check_zero_point_8_async", "tce_host_alloc", "tce_host_free", "tce_malloc", "tce_free", "tce_memcpy", "tce_synchronize", "tce_device_count",
]


class W4A16Desc(C.Structure):
    """struct tce_w4a16_desc"""
    _fields_ = [
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("group_size", C.c_int32),
        ("A", C.c_void_p), ("qweight", C.c_void_p), ("scales", C.c_void_p), ("zeros", C.c_void_p), ("C", C.c_void_p),
        ("lda", C.c_int32), ("ldc", C.c_int32), ("scales_stride", C.c_int32), ("zeros_stride", C.c_int32),
        ("flags", C.c_int32), ("reserved", C.c_int32),
        ("rmsnorm_gamma", C.c_void_p), ("rmsnorm_eps", C.c_float), ("reserved2", C.c_int32),
        ("prepacked", C.c_void_p), ("scratch", C.c_void_p),
    ]


class W8A8Desc(C.Structure):
    """struct tce_w8a8_desc"""
    _fields_ = [
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("batch", C.c_int32),
        ("A", C.c_void_p), ("B", C.c_void_p), ("bias", C.c_void_p), ("C", C.c_void_p),
        ("strideA", C.c_int64), ("strideB", C.c_int64), ("strideC", C.c_int64),
        ("alpha", C.c_float), ("beta", C.c_float), ("q_min", C.c_int32), ("q_max", C.c_int32),
        ("bias_kind", C.c_int32), ("out_kind", C.c_int32), ("b_per_row", C.c_int32), ("accumulate", C.c_int32),
        ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32), ("reserved2", C.c_int32),
    ]


class AttnDeferred(C.Structure):
    """struct tce_attention_deferred: what a deferred attention step leaves for the linear that consumes it"""
    _fields_ = [("slots", C.c_int32), ("chunk", C.c_int32), ("heads", C.c_int32), ("stride", C.c_int32), ("part", C.c_void_p)]


class W4A16DescV2(C.Structure):
    """struct tce_w4a16_desc_v2: the size-prefixed form (ABI 110)"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("desc", W4A16Desc)]


class W8A8DescV2(C.Structure):
    """struct tce_w8a8_desc_v2"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("desc", W8A8Desc), ("scratch", C.c_void_p)]


def w4a16_forward_v2(desc: W4A16Desc, stream: int | None, extra_zero_bytes: int = 0) -> int:
    """tce_w4a16_forward_v2; extra_zero_bytes: pretend to be a LATER host whose descriptor has that many more (zeroed) bytes."""
    buf = (C.c_ubyte * (C.sizeof(W4A16DescV2) + extra_zero_bytes))()
    v2 = W4A16DescV2.from_buffer(buf)
    v2.struct_size = C.sizeof(W4A16DescV2) + extra_zero_bytes
    v2.desc = desc
    return lib().tce_w4a16_forward_v2(C.byref(v2), C.c_void_p(stream or 0))


_w8a8_scratch: dict = {}


def w8a8_scratch(device) -> "torch.Tensor":
    """tce_w8a8_desc_v2.scratch for `device`: one zeroed area shared by the harness's calls (ordered by its one stream)."""
    import torch
    key = str(device)
    if key not in _w8a8_scratch:
        L = lib()
        L.tce_w8a8_scratch_bytes.restype = C.c_size_t
        _w8a8_scratch[key] = torch.zeros(int(L.tce_w8a8_scratch_bytes()), dtype=torch.uint8, device=device)
    return _w8a8_scratch[key]


def w8a8_matmul_v2(desc: W8A8Desc, stream: int | None, scratch_ptr: int | None = None) -> int:
    v2 = W8A8DescV2(struct_size=C.sizeof(W8A8DescV2), reserved0=0, desc=desc, scratch=scratch_ptr)
    return lib().tce_w8a8_matmul_v2(C.byref(v2), C.c_void_p(stream or 0))


TCE_SAMPLE_MAX_K = 256
TCE_SAMPLE_RING = 64


class SampleRow(C.Structure):
    """struct tce_sample_row: one row's sampling parameters and state, on the device (304 bytes)"""
    _fields_ = [("temp", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("repeat_penalty", C.c_float), ("alpha_frequency", C.c_float), ("alpha_presence", C.c_float),
                ("repeat_last_n", C.c_int32), ("max_new", C.c_int32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("generated", C.c_uint32), ("ring_pushed", C.c_uint32),
                ("ring", C.c_int32 * 64)]


class SampleDebug(C.Structure):
    """struct tce_sample_debug: a row's sorted candidates (tests)"""
    _fields_ = [("n", C.c_int32), ("k", C.c_int32), ("u", C.c_float), ("choice", C.c_int32), ("ids", C.c_int32 * 256), ("logit", C.c_float * 256), ("p", C.c_float * 256),
                ("final_p", C.c_float * 256)]


class SampleCall(C.Structure):
    """struct tce_sample_call"""
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_int32), ("vocab", C.c_int32), ("batch", C.c_int32), ("top_k_bound", C.c_int32), ("rows", C.c_void_p), ("pos_device", C.c_void_p),
                ("pos_bound", C.c_int32), ("log_stride", C.c_int32), ("next_token", C.c_void_p), ("out_log", C.c_void_p), ("uniform_override", C.c_void_p), ("debug", C.c_void_p),
                ("workspace", C.c_void_p), ("stop_ids", C.c_int32 * 4), ("n_stop", C.c_int32), ("mirostat", C.c_int32), ("tfs_z", C.c_float), ("typical_p", C.c_float)]


def sample_f16(call: SampleCall, stream: int | None) -> int:
    return lib().tce_sample_f16(C.byref(call), C.c_void_p(stream or 0))


TCE_SPEC_MAX_ROWS = 8


class SampleVerifyCall(C.Structure):
    """struct tce_sample_verify_call"""
    _fields_ = [("s", SampleCall), ("rows_per_seq", C.c_int32), ("hist_stride", C.c_int32), ("row_token", C.c_void_p), ("row_pos", C.c_void_p), ("history", C.c_void_p),
                ("emitted", C.c_void_p)]


def sample_verify_f16(call: SampleVerifyCall, stream: int | None) -> int:
    return lib().tce_sample_verify_f16(C.byref(call), C.c_void_p(stream or 0))


class LogprobOut(C.Structure):
    """struct tce_logprob_out"""
    _fields_ = [("out_logprob", C.c_void_p), ("last_lse", C.c_void_p), ("partials", C.c_void_p)]


def sample_logprobs_f16(call: SampleCall, lp: LogprobOut, stream: int | None) -> int:
    return lib().tce_sample_logprobs_f16(C.byref(call), C.byref(lp), C.c_void_p(stream or 0))


def sample_verify_logprobs_f16(call: SampleVerifyCall, lp: LogprobOut, stream: int | None) -> int:
    return lib().tce_sample_verify_logprobs_f16(C.byref(call), C.byref(lp), C.c_void_p(stream or 0))


TCE_FSM_DONE = -1
TCE_FSM_MAX = 64
TCE_BIAS_MAX = 16
TCE_LORA_MAX_RANK = 192
TCE_LORA_MAX_ADAPTERS = 64


class Fsm(C.Structure):
    """struct tce_fsm: one token automaton's descriptor; every array on the device (56 bytes)"""
    _fields_ = [("mask", C.c_void_p), ("edge_begin", C.c_void_p), ("edge_token", C.c_void_p), ("edge_next", C.c_void_p), ("default_next", C.c_void_p), ("states", C.c_int32),
                ("mask_words", C.c_int32), ("start", C.c_int32), ("reserved0", C.c_int32)]


class ConstraintRow(C.Structure):
    """struct tce_constraint_row: a slot's automaton, state and logit bias, on the device (144 bytes)"""
    _fields_ = [("fsm", C.c_int32), ("state", C.c_int32), ("n_bias", C.c_int32), ("reserved0", C.c_int32), ("bias_id", C.c_int32 * TCE_BIAS_MAX), ("bias_val", C.c_float * TCE_BIAS_MAX)]


class Constraint(C.Structure):
    """struct tce_constraint"""
    _fields_ = [("fsms", C.c_void_p), ("n_fsm", C.c_int32), ("reserved0", C.c_int32), ("rows", C.c_void_p), ("violations", C.c_void_p)]


def sample_constrained_f16(call: SampleCall, con: Constraint | None, lp: LogprobOut | None, stream: int | None) -> int:
    return lib().tce_sample_constrained_f16(C.byref(call), C.byref(con) if con is not None else None, C.byref(lp) if lp is not None else None, C.c_void_p(stream or 0))


def sample_verify_constrained_f16(call: SampleVerifyCall, con: Constraint | None, lp: LogprobOut | None, stream: int | None) -> int:
    return lib().tce_sample_verify_constrained_f16(C.byref(call), C.byref(con) if con is not None else None, C.byref(lp) if lp is not None else None, C.c_void_p(stream or 0))


class StageRow(C.Structure):
    """struct tce_stage_row: a slot's tail-free and typical values, on the device (8 bytes; 1.0 = off)"""
    _fields_ = [("tfs_z", C.c_float), ("typical_p", C.c_float)]


class StageDebug(C.Structure):
    """struct tce_stage_debug: a row's candidates behind the two stages (tests; 2056 bytes)"""
    _fields_ = [("n_tfs", C.c_int32), ("n_typ", C.c_int32), ("order", C.c_int32 * 256), ("p_top", C.c_float * 256)]


class SampleStages(C.Structure):
    """struct tce_sample_stages"""
    _fields_ = [("rows", C.c_void_p), ("debug", C.c_void_p)]


def sample_stages_f16(call: SampleCall, st: SampleStages | None, con: Constraint | None, lp: LogprobOut | None, stream: int | None) -> int:
    return lib().tce_sample_stages_f16(C.byref(call), C.byref(st) if st is not None else None, C.byref(con) if con is not None else None,
                                       C.byref(lp) if lp is not None else None, C.c_void_p(stream or 0))


def sample_verify_stages_f16(call: SampleVerifyCall, st: SampleStages | None, con: Constraint | None, lp: LogprobOut | None, stream: int | None) -> int:
    return lib().tce_sample_verify_stages_f16(C.byref(call), C.byref(st) if st is not None else None, C.byref(con) if con is not None else None,
                                              C.byref(lp) if lp is not None else None, C.c_void_p(stream or 0))


class MirostatRow(C.Structure):
    """struct tce_mirostat_row: a slot's mirostat mode, parameters and running mu, on the device (20 bytes; mode 0 = off)"""
    _fields_ = [("mode", C.c_int32), ("m", C.c_int32), ("tau", C.c_float), ("eta", C.c_float), ("mu", C.c_float)]


class MirostatDebug(C.Structure):
    """struct tce_mirostat_debug: what the mirostat rule did with a row (tests; 40 bytes)"""
    _fields_ = [("mode", C.c_int32), ("kk", C.c_int32), ("s_hat", C.c_float), ("k_f", C.c_float), ("kept", C.c_int32), ("mu_in", C.c_float), ("mu_out", C.c_float),
                ("surprise", C.c_float), ("choice", C.c_int32), ("final_p", C.c_float)]


class SampleMirostat(C.Structure):
    """struct tce_sample_mirostat"""
    _fields_ = [("rows", C.c_void_p), ("debug", C.c_void_p)]


def sample_mirostat_f16(call: SampleCall, st: SampleStages | None, mi: SampleMirostat | None, con: Constraint | None, lp: LogprobOut | None, stream: int | None) -> int:
    return lib().tce_sample_mirostat_f16(C.byref(call), C.byref(st) if st is not None else None, C.byref(mi) if mi is not None else None,
                                         C.byref(con) if con is not None else None, C.byref(lp) if lp is not None else None, C.c_void_p(stream or 0))


def sample_verify_mirostat_f16(call: SampleVerifyCall, st: SampleStages | None, mi: SampleMirostat | None, con: Constraint | None, lp: LogprobOut | None,
                               stream: int | None) -> int:
    return lib().tce_sample_verify_mirostat_f16(C.byref(call), C.byref(st) if st is not None else None, C.byref(mi) if mi is not None else None,
                                                C.byref(con) if con is not None else None, C.byref(lp) if lp is not None else None, C.c_void_p(stream or 0))


def logprobs_f16(logits_ptr: int, ld: int, vocab: int, rows: int, target_ptr: int, out_logprob_ptr: int, out_lse_ptr: int | None, partials_ptr: int, stream: int | None) -> int:
    """tce_logprobs_f16: logprob of target[r] under logits row r (two launches)."""
    return lib().tce_logprobs_f16(C.c_void_p(logits_ptr), ld, vocab, rows, C.c_void_p(target_ptr), C.c_void_p(out_logprob_ptr), C.c_void_p(out_lse_ptr or 0),
                                  C.c_void_p(partials_ptr), C.c_void_p(stream or 0))


class TceError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libtce_hip error {code}: {msg}")
        self.code = code


_lib = None
HAS_GROUP_COPIES = False  # set by lib(): the loaded library exports tce_w4a16_prepack_group(_bytes)


def lib() -> C.CDLL:
    """The loaded library.  Raises if it has not been built (python -m tinychatengine_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m tinychatengine_amd.build` "
                "(hipcc, gfx950).  tinychatengine_amd has no CPU or PyTorch fallback."
            )
        try:
            # FIRST: the PyTorch wheel ships its own HIP runtime.  Loaded before it, this library would bring the system's copy into the process and the two
            # runtimes do not share a device (hipStreamCreate: "no ROCm-capable device" -- seen with build() and smoke() called in one process).
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.tce_version.restype = C.c_int
        # the descriptors are plain structs without a size field: a library built from another header revision would read the mirrored
        # structs below at the wrong offsets -- refuse it here, loudly, instead
        if int(L.tce_version()) != TCE_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} reports ABI version {int(L.tce_version())}, this wrapper mirrors {TCE_ABI_VERSION} (include/tce_matmul.h: TCE_VERSION): rebuild with `python -m tinychatengine_amd.build`")
        L.tce_last_error.restype = C.c_char_p
        L.tce_build_info.restype = C.c_char_p
        L.tce_w4a16_forward.argtypes = [C.POINTER(W4A16Desc), C.c_void_p]
        L.tce_w4a16_forward_group.argtypes = [C.POINTER(W4A16Desc), C.c_int, C.c_void_p]
        L.tce_w4a16_forward_independent.argtypes = [C.POINTER(W4A16Desc), C.c_int, C.POINTER(C.c_int), C.c_void_p]
        L.tce_w4a16_describe_independent.argtypes = [C.POINTER(W4A16Desc), C.c_int, C.c_char_p, C.c_int]
        L.tce_w4a16_forward_independent_gather.argtypes = [C.POINTER(W4A16Desc), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
        L.tce_w4a16_prepack_bytes.argtypes = [C.c_int] * 3
        L.tce_w4a16_prepack_bytes.restype = C.c_size_t
        L.tce_w4a16_gemm_scratch_bytes.argtypes = []
        L.tce_w4a16_gemm_scratch_bytes.restype = C.c_size_t
        L.tce_w4a16_prepack.argtypes = [C.POINTER(W4A16Desc), C.c_void_p, C.c_void_p]
        # additive within ABI 113: a TCE_LIB_PATH build from before the group copies (the parent side of an A/B run) lacks the two; HAS_GROUP_COPIES tells callers
        global HAS_GROUP_COPIES
        HAS_GROUP_COPIES = hasattr(L, "tce_w4a16_prepack_group_bytes") and hasattr(L, "tce_w4a16_prepack_group")
        if HAS_GROUP_COPIES:
            L.tce_w4a16_prepack_group_bytes.argtypes = [C.POINTER(W4A16Desc), C.c_int]
            L.tce_w4a16_prepack_group_bytes.restype = C.c_size_t
            L.tce_w4a16_prepack_group.argtypes = [C.POINTER(W4A16Desc), C.c_int, C.c_void_p, C.c_void_p]
        L.tce_prefetch.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
        L.tce_bmm_f16t.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ushort, C.c_void_p]
        L.tce_rope_half.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]
        L.tce_softmax_half.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
        L.tce_attention_decode_f16.argtypes = [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_ushort, C.c_void_p]
        L.tce_attention_decode_workspace_bytes.argtypes = [C.c_int] * 3
        L.tce_attention_decode_workspace_bytes.restype = C.c_size_t
        L.tce_attention_decode_describe.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.tce_attention_decode_step_f16.argtypes = [C.c_void_p] * 8 + [C.c_int] * 4 + [C.c_ushort, C.c_void_p]
        L.tce_attention_decode_step_gqa_f16.argtypes = [C.c_void_p] * 8 + [C.c_int] * 5 + [C.c_ushort, C.c_void_p]
        L.tce_attention_decode_step_pos_f16.argtypes = [C.c_void_p] * 8 + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_ushort, C.c_void_p]
        L.tce_attention_decode_batch_workspace_bytes.argtypes = [C.c_int] * 4
        L.tce_attention_decode_batch_workspace_bytes.restype = C.c_size_t
        L.tce_attention_decode_describe_batch.argtypes = [C.c_int] * 4 + [C.c_char_p, C.c_int]
        L.tce_attention_decode_step_batch_f16.argtypes = [C.c_void_p] * 7 + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_ushort, C.c_void_p]
        L.tce_kv_pages_pool_bytes.argtypes = [C.c_int] * 4
        L.tce_kv_pages_pool_bytes.restype = C.c_size_t
        L.tce_attention_decode_describe_paged.argtypes = [C.c_int] * 5 + [C.c_char_p, C.c_int]
        L.tce_attention_decode_step_paged_f16.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_ushort, C.c_void_p]
        L.tce_kv_pages_scatter_f16.argtypes = [C.c_void_p] * 5 + [C.c_int] * 8 + [C.c_void_p]
        L.tce_kv_pages_gather_f16.argtypes = [C.c_void_p] * 5 + [C.c_int] * 8 + [C.c_void_p]
        L.tce_kv_block_table_check.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        # the e4m3 pages (include/tce_matmul.h, "FP8 pages"): the f16 argument lists with k_scale_log2, v_scale_log2 in front of the stream
        L.tce_kv_pages_pool_bytes_fp8.argtypes = [C.c_int] * 4
        L.tce_kv_pages_pool_bytes_fp8.restype = C.c_size_t
        L.tce_attention_decode_step_paged_fp8.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_ushort, C.c_int, C.c_int, C.c_void_p]
        L.tce_kv_pages_scatter_fp8.argtypes = [C.c_void_p] * 5 + [C.c_int] * 10 + [C.c_void_p]
        L.tce_kv_pages_gather_fp8.argtypes = [C.c_void_p] * 5 + [C.c_int] * 10 + [C.c_void_p]
        L.tce_attention_decode_step_deferred_f16.argtypes = [C.c_void_p] * 8 + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_ushort, C.POINTER(AttnDeferred), C.c_void_p]
        L.tce_w4a16_forward_deferred_attention.argtypes = [C.POINTER(W4A16Desc), C.POINTER(AttnDeferred), C.c_void_p, C.c_int, C.c_void_p]
        L.tce_opt_attention_decode.argtypes = [C.c_void_p] * 7 + [C.c_int] * 6 + [C.c_float, C.c_float, C.c_void_p]
        L.tce_attention_prefill_workspace_bytes.restype = C.c_size_t
        L.tce_attention_prefill_workspace_bytes.argtypes = [C.c_int] * 3
        L.tce_attention_prefill_f16.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + \
            [C.c_int] * 6 + [C.c_ushort, C.c_void_p]
        L.tce_attention_prefill_paged_workspace_bytes.restype = C.c_size_t
        L.tce_attention_prefill_paged_workspace_bytes.argtypes = [C.c_int] * 3
        L.tce_attention_prefill_paged_f16.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + \
            [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_int, C.c_ushort, C.c_void_p]
        L.tce_attention_prefill_paged_fp8.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + \
            [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_int, C.c_ushort, C.c_int, C.c_int, C.c_void_p]
        L.tce_attention_prefill_describe_paged.restype = C.c_char_p
        L.tce_attention_prefill_describe_paged.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.tce_sample_workspace_bytes.restype = C.c_size_t
        L.tce_sample_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.tce_sample_f16.argtypes = [C.POINTER(SampleCall), C.c_void_p]
        L.tce_attention_decode_step_paged_rows_f16.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_ushort, C.c_void_p]
        L.tce_attention_decode_step_paged_rows_fp8.argtypes = [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_ushort, C.c_int, C.c_int, C.c_void_p]
        # sliding-window attention (include/tce_matmul.h): the unwindowed argument lists with `window` in front of the stream
        L.tce_attention_decode_describe_paged_window.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_int]
        L.tce_attention_decode_step_paged_window_f16.argtypes = L.tce_attention_decode_step_paged_f16.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_attention_decode_step_paged_window_fp8.argtypes = L.tce_attention_decode_step_paged_fp8.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_attention_prefill_paged_window_f16.argtypes = L.tce_attention_prefill_paged_f16.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_attention_prefill_paged_window_fp8.argtypes = L.tce_attention_prefill_paged_fp8.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_kv_block_table_check_window.argtypes = L.tce_kv_block_table_check.argtypes[:-1] + [C.c_int, C.c_void_p]
        # attention sinks beside the window (include/tce_matmul.h): the windowed argument lists with `sinks` behind `window`
        L.tce_attention_decode_describe_paged_sink.argtypes = [C.c_int] * 7 + [C.c_char_p, C.c_int]
        L.tce_attention_decode_step_paged_sink_f16.argtypes = L.tce_attention_decode_step_paged_window_f16.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_attention_decode_step_paged_sink_fp8.argtypes = L.tce_attention_decode_step_paged_window_fp8.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_attention_prefill_paged_sink_f16.argtypes = L.tce_attention_prefill_paged_window_f16.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_attention_prefill_paged_sink_fp8.argtypes = L.tce_attention_prefill_paged_window_fp8.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_kv_block_table_check_sink.argtypes = L.tce_kv_block_table_check_window.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_attention_decode_step_paged_rows_window_f16.argtypes = L.tce_attention_decode_step_paged_rows_f16.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_attention_decode_step_paged_rows_window_fp8.argtypes = L.tce_attention_decode_step_paged_rows_fp8.argtypes[:-1] + [C.c_int, C.c_void_p]
        # sinks on the multi-row step: the windowed rows argument lists with `sinks` behind `window`
        L.tce_attention_decode_step_paged_rows_sink_f16.argtypes = L.tce_attention_decode_step_paged_rows_window_f16.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_attention_decode_step_paged_rows_sink_fp8.argtypes = L.tce_attention_decode_step_paged_rows_window_fp8.argtypes[:-1] + [C.c_int, C.c_void_p]
        L.tce_sample_verify_workspace_bytes.restype = C.c_size_t
        L.tce_sample_verify_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.tce_sample_verify_f16.argtypes = [C.POINTER(SampleVerifyCall), C.c_void_p]
        L.tce_logprobs_workspace_bytes.restype = C.c_size_t
        L.tce_logprobs_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.tce_sample_logprobs_f16.argtypes = [C.POINTER(SampleCall), C.POINTER(LogprobOut), C.c_void_p]
        L.tce_sample_verify_logprobs_f16.argtypes = [C.POINTER(SampleVerifyCall), C.POINTER(LogprobOut), C.c_void_p]
        L.tce_sample_constrained_f16.argtypes = [C.POINTER(SampleCall), C.POINTER(Constraint), C.POINTER(LogprobOut), C.c_void_p]
        L.tce_sample_verify_constrained_f16.argtypes = [C.POINTER(SampleVerifyCall), C.POINTER(Constraint), C.POINTER(LogprobOut), C.c_void_p]
        L.tce_sample_stages_f16.argtypes = [C.POINTER(SampleCall), C.POINTER(SampleStages), C.POINTER(Constraint), C.POINTER(LogprobOut), C.c_void_p]
        L.tce_sample_verify_stages_f16.argtypes = [C.POINTER(SampleVerifyCall), C.POINTER(SampleStages), C.POINTER(Constraint), C.POINTER(LogprobOut), C.c_void_p]
        L.tce_sample_verify_mirostat_workspace_bytes.restype = C.c_size_t
        L.tce_sample_verify_mirostat_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.tce_sample_verify_mirostat_f16.argtypes = [C.POINTER(SampleVerifyCall), C.POINTER(SampleStages), C.POINTER(SampleMirostat), C.POINTER(Constraint), C.POINTER(LogprobOut),
                                                     C.c_void_p]
        L.tce_sample_mirostat_f16.argtypes = [C.POINTER(SampleCall), C.POINTER(SampleStages), C.POINTER(SampleMirostat), C.POINTER(Constraint), C.POINTER(LogprobOut), C.c_void_p]
        L.tce_logprobs_f16.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tce_lora_shrink_f16.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
        L.tce_lora_expand_add_f16.argtypes = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p]
        L.tce_lora_expand_silu_mul_f16.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
        L.tce_draft_ngram.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tce_embed_rows_f16.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tce_attention_decode_describe_gqa.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.tce_add_half.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        L.tce_silu_mul_half.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        L.tce_rmsnorm_half.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
        L.tce_w4a16_forward_group_rmsnorm.argtypes = [C.POINTER(W4A16Desc), C.c_int, C.c_void_p, C.c_float, C.c_void_p]
        L.tce_w4a16_check_zero_point_8.argtypes = [C.c_void_p, C.c_longlong]
        L.tce_w4a16_awq_fp16acc.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5
        L.tce_w4a16_awq_workspace_bytes.argtypes = [C.c_int] * 3
        L.tce_w4a16_awq_workspace_bytes.restype = C.c_size_t
        L.tce_w4a16_gemm_awq.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        L.tce_w8a8_matmul.argtypes = [C.POINTER(W8A8Desc), C.c_void_p]
        L.tce_opt_softmax_q.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.tce_opt_kv_append.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p]
        L.tce_w4a16_shard.argtypes = [C.POINTER(W4A16Desc), C.c_int, C.c_int, C.POINTER(W4A16Desc)]
        L.tce_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.tce_comm_export.argtypes = [C.c_void_p, C.c_void_p]
        L.tce_comm_connect.argtypes = [C.c_void_p, C.c_void_p]
        L.tce_comm_connect_local.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.tce_allgather_f16.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.tce_comm_status.argtypes = [C.c_void_p]
        L.tce_comm_set_timeout_ms.argtypes = [C.c_void_p, C.c_int]
        L.tce_comm_reset.argtypes = [C.c_void_p]
        L.tce_comm_device.argtypes = [C.c_void_p]
        L.tce_comm_destroy.argtypes = [C.c_void_p]
        L.tce_comm_destroy.restype = None
        L.tce_layernorm_q.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.tce_layernorm_q_w8a8_group.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(W8A8Desc), C.c_int, C.c_void_p, C.c_void_p]
        L.tce_plan_create.argtypes = [C.POINTER(W4A16Desc), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_void_p)]
        L.tce_plan_create_ex.argtypes = [C.POINTER(W4A16Desc), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.tce_plan_is_chained.argtypes = [C.c_void_p]
        L.tce_plan_status.argtypes = [C.c_void_p]
        L.tce_plan_geometry.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
        L.tce_plan_launch.argtypes = [C.c_void_p, C.c_void_p]
        L.tce_plan_n_launches.argtypes = [C.c_void_p]
        L.tce_plan_destroy.argtypes = [C.c_void_p]
        L.tce_plan_destroy.restype = None
        L.tce_w4a16_set_gemv_config.argtypes = [C.c_int] * 4
        L.tce_w4a16_set_gemm_config.argtypes = [C.c_int] * 2
        L.tce_w4a16_set_gemv_i8.argtypes = [C.c_int] * 2
        L.tce_w4a16_residual_rmsnorm_workspace_bytes.restype = C.c_size_t
        L.tce_w4a16_forward_residual_rmsnorm.argtypes = [C.POINTER(W4A16Desc), C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tce_comm_rccl_unique_id.argtypes = [C.c_void_p]
        L.tce_comm_rccl_init.argtypes = [C.c_void_p, C.c_void_p]
        L.tce_allgather_rows_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.tce_allgather_rows_workspace_bytes.restype = C.c_size_t
        L.tce_allgather_rows_f16.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.tce_w4a16_algorithmic_bytes.argtypes = [C.c_int] * 4
        L.tce_w4a16_algorithmic_bytes.restype = C.c_int64
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != TCE_OK:
        raise TceError(rc, lib().tce_last_error().decode())


def last_error() -> str:
    return lib().tce_last_error().decode()


def _parse_pairs(text: str) -> dict:
    """The describe entry points' "key=value key=value ..." text as a dict; a value of digits becomes an int."""
    out = {}
    for tok in text.split():
        k, v = tok.split("=")
        out[k] = int(v) if v.isdigit() else v
    return out


def describe_attention_step(heads: int, keys: int, kv_heads: int | None = None) -> dict:
    """How tce_attention_decode_step_f16 / _gqa_f16 cuts a context of `keys` keys: {"chunks", "keys-per-chunk", "waves", "workgroups", "combine"} (no GPU needed)."""
    buf = C.create_string_buffer(160)
    check(lib().tce_attention_decode_describe_gqa(heads, heads if kv_heads is None else kv_heads, keys, buf, len(buf)))
    return _parse_pairs(buf.value.decode())


def describe_attention_paged(batch: int, heads: int, kv_heads: int, pos_bound: int, page_keys: int) -> dict:
    """How tce_attention_decode_step_paged_f16 cuts the launch: describe_attention_batch's keys plus "page-keys" (no GPU needed)."""
    buf = C.create_string_buffer(192)
    check(lib().tce_attention_decode_describe_paged(batch, heads, kv_heads, pos_bound, page_keys, buf, len(buf)))
    return _parse_pairs(buf.value.decode())


def describe_attention_paged_sink(batch: int, heads: int, kv_heads: int, pos_bound: int, page_keys: int, window: int, sinks: int) -> dict:
    """How tce_attention_decode_step_paged_sink_f16 cuts the launch -- for the virtual keys a row can span (include/tce_matmul.h, "cut"): describe_attention_paged's keys
    (no GPU needed)."""
    buf = C.create_string_buffer(192)
    check(lib().tce_attention_decode_describe_paged_sink(batch, heads, kv_heads, pos_bound, page_keys, window, sinks, buf, len(buf)))
    return _parse_pairs(buf.value.decode())


def describe_attention_paged_window(batch: int, heads: int, kv_heads: int, pos_bound: int, page_keys: int, window: int) -> dict:
    """How tce_attention_decode_step_paged_window_f16 cuts the launch -- for min(pos_bound + 1, window + 3) keys: describe_attention_paged's keys (no GPU needed)."""
    buf = C.create_string_buffer(192)
    check(lib().tce_attention_decode_describe_paged_window(batch, heads, kv_heads, pos_bound, page_keys, window, buf, len(buf)))
    return _parse_pairs(buf.value.decode())


TCE_PREFILL_MAX_SEGMENTS = 16


class PrefillSegment(C.Structure):
    """tce_prefill_segment: m new rows (rows row0 .. row0 + m - 1 of qkv / out) on top of pos cached keys of table row `slot`."""
    _fields_ = [("slot", C.c_int32), ("pos", C.c_int32), ("m", C.c_int32), ("row0", C.c_int32)]


def prefill_segments(segments) -> tuple:
    """[(slot, pos, m)] -> (a tce_prefill_segment array with the rows packed in that order, the total number of rows)"""
    arr = (PrefillSegment * max(len(segments), 1))()
    row0 = 0
    for i, (slot, pos, m) in enumerate(segments):
        arr[i] = PrefillSegment(int(slot), int(pos), int(m), row0)
        row0 += int(m)
    return arr, row0


def describe_prefill_paged(heads: int, kv_heads: int, causal: bool, segments) -> dict:
    """How tce_attention_prefill_paged_f16 cuts a launch of [(slot, pos, m)]: {"form", "rows-per-block", "pair", "blocks", "workgroups", "segments"} (no GPU needed)."""
    arr, _ = prefill_segments(segments)
    text = lib().tce_attention_prefill_describe_paged(heads, kv_heads, 1 if causal else 0, C.cast(arr, C.c_void_p), len(segments))
    if text is None:
        raise TceError(TCE_ERR_BAD_ARG, last_error())
    return _parse_pairs(text.decode())


def describe_attention_batch(batch: int, heads: int, kv_heads: int, pos_bound: int) -> dict:
    """How tce_attention_decode_step_batch_f16 cuts `batch` sequences bounded by pos_bound: describe_attention_step's keys plus "batch" (no GPU needed)."""
    buf = C.create_string_buffer(160)
    check(lib().tce_attention_decode_describe_batch(batch, heads, kv_heads, pos_bound, buf, len(buf)))
    return _parse_pairs(buf.value.decode())


def describe_dispatch(desc: W4A16Desc) -> str:
    buf = C.create_string_buffer(128)
    check(lib().tce_w4a16_describe_dispatch(C.byref(desc), buf, 128))
    return buf.value.decode()


def w4a16_forward(desc: W4A16Desc, stream: int | None) -> int:
    return lib().tce_w4a16_forward(C.byref(desc), C.c_void_p(stream or 0))


def w4a16_forward_residual_rmsnorm(desc: W4A16Desc, gamma_ptr: int, eps: float, xn_ptr: int, workspace_ptr: int, stream: int | None) -> int:
    """o_proj / down_proj + residual add + the RMSNorm that follows, one launch (tce_w4a16_forward_residual_rmsnorm)."""
    return lib().tce_w4a16_forward_residual_rmsnorm(C.byref(desc), C.c_void_p(gamma_ptr), float(eps), C.c_void_p(xn_ptr), C.c_void_p(workspace_ptr), C.c_void_p(stream or 0))


def w4a16_forward_group(descs: list[W4A16Desc], stream: int | None) -> int:
    arr = (W4A16Desc * len(descs))(*descs)
    return lib().tce_w4a16_forward_group(arr, len(descs), C.c_void_p(stream or 0))


TCE_MAX_INDEPENDENT = 8


def w4a16_forward_independent(descs: list[W4A16Desc], stream: int | None) -> int:
    """tce_w4a16_forward_independent: linears that share nothing, one launch where the library has one.  Returns the number of kernel launches made (raises on error)."""
    arr = (W4A16Desc * len(descs))(*descs)
    n = C.c_int(0)
    check(lib().tce_w4a16_forward_independent(arr, len(descs), C.byref(n), C.c_void_p(stream or 0)))
    return n.value


def describe_w8a8_dispatch(desc: W8A8Desc, with_scratch: bool = False) -> str:
    """tce_w8a8_describe_dispatch: the kernel form tce_w8a8_matmul would run for this descriptor (no GPU needed)."""
    buf = C.create_string_buffer(128)
    L = lib()
    L.tce_w8a8_describe_dispatch.argtypes = [C.POINTER(W8A8Desc), C.c_int, C.c_char_p, C.c_int]
    check(L.tce_w8a8_describe_dispatch(C.byref(desc), 1 if with_scratch else 0, buf, 128))
    return buf.value.decode()


def describe_independent(descs: list[W4A16Desc]) -> str:
    """tce_w4a16_describe_independent: how the library would run these linears through tce_w4a16_forward_independent (no GPU needed)."""
    arr = (W4A16Desc * len(descs))(*descs)
    buf = C.create_string_buffer(128)
    check(lib().tce_w4a16_describe_independent(arr, len(descs), buf, len(buf)))
    return buf.value.decode()


def w8a8_matmul(desc: W8A8Desc, stream: int | None) -> int:
    return lib().tce_w8a8_matmul(C.byref(desc), C.c_void_p(stream or 0))


def algorithmic_bytes(M: int, N: int, K: int, G: int) -> int:
    return int(lib().tce_w4a16_algorithmic_bytes(M, N, K, G))


def set_gemv_config(rows: int = 0, waves_n: int = 0, waves_k: int = 0, depth: int = 0) -> None:
    check(lib().tce_w4a16_set_gemv_config(rows, waves_n, waves_k, depth))


def set_gemv_i8(mode: int = 0, tiles_per_wave: int = 0) -> None:
    """The decode kernel on pre-packed copies: mode 0 automatic, 1 off; tiles_per_wave 0 the rule, 1, 2."""
    check(lib().tce_w4a16_set_gemv_i8(mode, tiles_per_wave))


def attention_set_tuning(waves_per_workgroup: int = 0, workgroups: int = 0, heads_per_workgroup: int = 0) -> None:
    """The fast decode attention step's cut, by name (0 = the fitted rule): waves per workgroup 4 / 8 / 16, workgroups 32..8192, query heads per workgroup 1 / 2 / 4."""
    check(lib().tce_attention_set_tuning(waves_per_workgroup, workgroups, heads_per_workgroup))


def w8a8_set_tuning(quartets_per_tile: int = 0, big_tiles: int = 0, deep_pipeline: int = 0) -> None:
    """tce_w8a8_matmul's kernel choice, by name (0 = the rules): quartets per 64x64 tile 1 / 2 / 4; the 128-row tiles 1..4 forced, 9 off; the deep-pipeline 64x64 tile 1 / 2 / 4 forced, 9 off."""
    check(lib().tce_w8a8_set_tuning(quartets_per_tile, big_tiles, deep_pipeline))


def set_gemm_config(m_tiles: int = 0, n_tiles: int = 0) -> None:
    check(lib().tce_w4a16_set_gemm_config(m_tiles, n_tiles))


def gemv_variants() -> list[tuple[int, int, int, int]]:
    """(rows_per_wave, waves_n, waves_k, depth) of every compiled GEMV kernel variant."""
    out, i = [], 0
    r, n, k, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    while lib().tce_w4a16_gemv_variant(i, C.byref(r), C.byref(n), C.byref(k), C.byref(d)) == TCE_OK:
        out.append((r.value, n.value, k.value, d.value))
        i += 1
    return out


def gemm_variants() -> list[tuple[int, int]]:
    out, i = [], 0
    m, n = C.c_int(), C.c_int()
    while lib().tce_w4a16_gemm_variant(i, C.byref(m), C.byref(n)) == TCE_OK:
        out.append((m.value, n.value))
        i += 1
    return out


class Plan:
    """tce_plan: a fixed sequence of W4A16 launches captured into one hipGraph (one decode token's linears)."""

    def __init__(self, launches: list[list[W4A16Desc]], chained: bool = False, tagged: bool = False, overlapped: bool = False, tuned: bool = False, independent: bool = False):
        """tagged (chained: accepted synonym): TCE_PLAN_TAGGED -- one persistent kernel walks the list, the plan's data flow
        ordered by polling tagged output words (include/tce_matmul.h).  self.tagged tells whether that form was built.
        tuned: TCE_PLAN_TUNED -- the decode launches' geometries are timed on this device at creation (stream-ordered plans).
        independent: TCE_PLAN_INDEPENDENT -- every group is a set of linears that share nothing (up to TCE_MAX_INDEPENDENT; tce_w4a16_forward_independent)."""
        flat = [d for g in launches for d in g]
        self._descs = (W4A16Desc * len(flat))(*flat)
        self._groups = (C.c_int32 * len(launches))(*[len(g) for g in launches])
        self._h = C.c_void_p()
        check(lib().tce_plan_create_ex(self._descs, self._groups, len(launches), (TCE_PLAN_TAGGED if tagged else 0) | (TCE_PLAN_CHAINED if chained else 0) | (TCE_PLAN_OVERLAPPED if overlapped else 0) | (TCE_PLAN_TUNED if tuned else 0) | (TCE_PLAN_INDEPENDENT if independent else 0), C.byref(self._h)))
        self.n_launches = len(launches)
        self.kind = int(lib().tce_plan_is_chained(self._h))  # 0 stream-ordered, 2 token kernel (fp16 body), 3 overlapped launches, 4 token kernel on the int8-contraction body (round 6)
        self.chained = self.kind != 0
        self.tagged = self.kind in (2, 4)
        self.overlapped = self.kind == 3

    def launch(self, stream: int | None) -> None:
        check(lib().tce_plan_launch(self._h, C.c_void_p(stream or 0)))

    def geometry(self) -> dict:
        """Chained plans: what the token kernel runs with."""
        v = [C.c_int() for _ in range(4)]
        check(lib().tce_plan_geometry(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("rows", "depth", "waves", "workgroups"), (x.value for x in v)))

    def launch_geometries(self) -> list[tuple[int, int, int, int]]:
        """Per launch: the (rows, waves_n, waves_k, depth) a TCE_PLAN_TUNED plan chose, (0, 0, 0, 0) where the dispatcher's rule stayed."""
        out = []
        for i in range(self.n_launches):
            v = [C.c_int() for _ in range(4)]
            check(lib().tce_plan_launch_geometry(self._h, i, *[C.byref(x) for x in v]))
            out.append(tuple(x.value for x in v))
        return out

    def status(self) -> None:
        """Synchronise and raise if a chained launch ever gave up waiting for its predecessor."""
        check(lib().tce_plan_status(self._h))

    def close(self) -> None:
        if self._h:
            lib().tce_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """tce_comm: this rank's peer-write window + the mapped windows of the other ranks (include/tce_matmul.h, csrc/comm.hip)."""

    def __init__(self, rank: int, world: int, max_vector_elems: int, slots: int = 4):
        self.rank, self.world = rank, world
        h = C.c_void_p()
        check(lib().tce_comm_create(rank, world, max_vector_elems, slots, C.byref(h)))
        self.handle = h

    def export(self) -> bytes:
        buf = C.create_string_buffer(64)
        check(lib().tce_comm_export(self.handle, buf))
        return buf.raw

    def connect(self, handles: list[bytes]) -> None:
        table = C.create_string_buffer(b"".join(handles), 64 * self.world)
        check(lib().tce_comm_connect(self.handle, table))

    @staticmethod
    def connect_local(comms: list["Comm"]) -> None:
        arr = (C.c_void_p * len(comms))(*[c.handle for c in comms])
        for c in comms:
            check(lib().tce_comm_connect_local(c.handle, arr))

    def allgather(self, slot: int, src_ptr: int, dst_ptr: int, n_total: int, stream: int | None) -> None:
        check(lib().tce_allgather_f16(self.handle, slot, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), n_total, C.c_void_p(stream or 0)))

    def forward_independent_gather(self, descs: list, gathered: int, slot: int, dst_ptr: int, stream: int | None) -> int:
        """tce_w4a16_forward_independent_gather: the linears of `descs` as one launch, linear `gathered`'s slice exchanged with the other ranks inside it (the complete
        vector lands at dst_ptr).  Returns the number of kernel launches made."""
        arr = (W4A16Desc * len(descs))(*descs)
        n = C.c_int(0)
        check(lib().tce_w4a16_forward_independent_gather(arr, len(descs), gathered, self.handle, slot, C.c_void_p(dst_ptr), C.byref(n), C.c_void_p(stream or 0)))
        return n.value

    @staticmethod
    def rccl_unique_id() -> bytes:
        """Rank 0: the opaque blob every rank passes to rccl_init (exchanged by the host like the IPC handles)."""
        buf = C.create_string_buffer(128)
        check(lib().tce_comm_rccl_unique_id(buf))
        return buf.raw

    def rccl_init(self, unique_id: bytes) -> None:
        """Collective: the RCCL side of this communicator (exchanges beyond the peer-write kernel's 64 KiB-per-rank regime)."""
        check(lib().tce_comm_rccl_init(self.handle, C.create_string_buffer(unique_id, 128)))

    def allgather_rows(self, slot: int, src_ptr: int, dst_ptr: int, m: int, n_total: int, workspace_ptr: int | None, stream: int | None, ldd: int = 0) -> None:
        check(lib().tce_allgather_rows_f16(self.handle, slot, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), m, n_total, ldd, C.c_void_p(workspace_ptr or 0), C.c_void_p(stream or 0)))

    def status(self) -> int:
        return int(lib().tce_comm_status(self.handle))

    def set_timeout_ms(self, ms: int) -> None:
        check(lib().tce_comm_set_timeout_ms(self.handle, int(ms)))

    def reset(self) -> None:
        """Re-arm after a timed-out wait (every rank, with no exchange in flight anywhere)."""
        check(lib().tce_comm_reset(self.handle))

    @property
    def device(self) -> int:
        return int(lib().tce_comm_device(self.handle))

    def close(self) -> None:
        if self.handle:
            lib().tce_comm_destroy(self.handle)
            self.handle = None
