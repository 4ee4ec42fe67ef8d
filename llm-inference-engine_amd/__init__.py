"""llm-inference-engine_amd -- MI355X-native Llama-2 decoder hot path.

Python side = plumbing only: it loads the in-tree C-ABI library
(lib/libllmie.so, built by build.py with hipcc for gfx950; see include/llmie.h)
through ctypes and hands it device pointers of torch tensors.  There is NO CPU or
PyTorch fallback: if the library is missing or a call fails, an exception is raised.

The directory name carries a hyphen (it mirrors the reference repo's name), so import
it with importlib (tests/conftest.py, bench.py and __graft_entry__.py show how) under
the module name ``llmie_amd``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libllmie.so")

F32, F16 = 0, 1
W_F16, W_INT8, W_INT4, W_FP8, W_F32 = 0, 1, 2, 3, 4
W_MXFP4 = 5   # e2m1 codes [N, K/2] + e8m0 scale bytes [N, K/32]: linear_mxfp4 and an engine format (Decoder, wfmt=W_MXFP4)
KV_NATIVE, KV_FP8 = 0, 1
DEC_NO_PACKED_COPY, DEC_PACKED_ONLY = 1, 2
ABI_VERSION = 3  # LLMIE_ABI_VERSION of include/llmie.h this binding mirrors

_lib = None


class LlmieError(RuntimeError):
    pass


def build(force=False, jobs=4):
    """Compile every HIP source for gfx950 (hipcc) into lib/libllmie.so."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("llmie_amd_build", os.path.join(_HERE, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(force=force, jobs=jobs)


_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# name -> argtypes (restype int unless listed in _RESTYPES); mirrors include/llmie.h
_SIGS = {
    "llmie_input_embedding": [_vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "llmie_cal_padding_offset": [_vp, _vp, _vp, _i, _i, _vp],
    "llmie_build_causal_mask": [_vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "llmie_rmsnorm": [_vp, _vp, _vp, _f, _i, _i, _i, _vp],
    "llmie_fused_add_bias_residual_rmsnorm": [_vp, _vp, _vp, _vp, _f, _i, _i, _i, _vp],
    "llmie_add_residual": [_vp, _vp, _i, _i, _i, _vp],
    "llmie_linear_workspace_bytes": [_i, _i, _i, _i],
    "llmie_linear": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _sz, _vp],
    "llmie_linear_swiglu": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp],
    "llmie_linear_route": [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz],
    "llmie_gemm256_tiles": [_i, _i, _i, _i, _i],
    "llmie_batched_gemm": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "llmie_qkv_bias_transpose_rope": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp],
    "llmie_rope_decode": [_vp, _i, _i, _i, _i, _i, _vp, _i, _f, _i, _vp],
    "llmie_decoder_mha_workspace_bytes": [_i, _i, _i, _i],
    "llmie_decoder_mha": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _i, _vp],
    "llmie_decoder_mha_rope": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp, _i, _vp, _i,
                               _vp],
    "llmie_concat_kv": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "llmie_repeat_kv": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "llmie_scale_mask_softmax": [_vp, _vp, _vp, _f, _i, _i, _i, _i, _i, _vp],
    "llmie_transpose_remove_padding": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "llmie_silu_and_mul": [_vp, _vp, _i, _i, _i, _vp],
    "llmie_topk": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "llmie_sampling": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp],
    "llmie_linear_w8a16": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "llmie_linear_w4a16": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "llmie_linear_fp8": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "llmie_linear_fp8_workspace_bytes": [_i, _i, _i],
    "llmie_linear_fp8_swiglu": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp],
    "llmie_packed_weight_bytes": [_i, _i, _i, _i],
    "llmie_packed_scale_bytes": [_i, _i, _i, _i],
    "llmie_pack_weight": [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "llmie_linear_packed_workspace_bytes": [_i, _i, _i, _i],
    "llmie_linear_packed": [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _sz, _vp],
    "llmie_x32_bytes": [_i],
    "llmie_x32_convert": [_vp, _vp, _i, _i, _i, _vp],
    "llmie_quantize_w8": [_vp, _vp, _vp, _i, _i, _vp],
    "llmie_quantize_w4": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "llmie_quantize_fp8": [_vp, _vp, _vp, _i, _i, _vp],
    "llmie_quantize_mxfp4": [_vp, _vp, _vp, _i, _i, _vp],
    "llmie_dequantize_mxfp4": [_vp, _vp, _vp, _i, _i, _vp],
    "llmie_linear_mxfp4": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "llmie_decoder_workspace_bytes": [_vp],
    "llmie_decoder_create": [_vp, _vp, _vp, _sz],
    "llmie_decoder_destroy": [_vp],
    "llmie_decoder_forward": [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp],
    "llmie_decoder_forward_ragged": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp],
    "llmie_decoder_forward_paged_ragged": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    "llmie_decoder_mha_plan": [_i, _i, _i, _i, _i, _i, _i, _i, C.c_uint, _i, _i, C.c_ulonglong, C.c_longlong, _vp],
    "llmie_decoder_mha_ragged": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp, _i, _vp, _i, _i, _i, _vp],
    "llmie_decoder_mha_window": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp, _i, _vp, _i, _i, _i, _i, _vp,
                                 _i, _f, _f, _i, _vp],
    "llmie_decoder_mha_window_plan": [_i, _i, _i, _i, _i, _i, _i, _i, C.c_uint, _i, _i, C.c_ulonglong, C.c_longlong, _i, _i, _vp],
    "llmie_kv_window_advance": [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp],
    "llmie_decoder_mha_sink": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp, _i, _vp, _i, _i, _i, _i, _vp,
                               _i, _f, _f, _vp, _i, _vp],
    "llmie_decoder_mha_sink_plan": [_i, _i, _i, _i, _i, _i, _i, _i, C.c_uint, _i, _i, C.c_ulonglong, C.c_longlong, _i, _i, _vp],
    "llmie_qk_norm": [_vp, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp],
    "llmie_decoder_mha_qknorm": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp, _i, _vp, _i, _i, _i, _i, _vp,
                                 _i, _f, _f, _vp, _vp, _vp, _f, _i, _vp],
    "llmie_decoder_mha_qknorm_plan": [_i, _i, _i, _i, _i, _i, _i, _i, C.c_uint, _i, _i, C.c_ulonglong, C.c_longlong, _i, _i, _vp],
    "llmie_decoder_set_qk_norm": [_vp, _vp, _vp, _f],
    "llmie_rope_table_fill": [_vp, _i, _i, _i, _f, _vp],
    "llmie_decoder_set_head_sinks": [_vp, _vp],
    "llmie_decoder_set_rope_scaling": [_vp, _vp],
    "llmie_decoder_prefill_workspace_bytes": [_vp, _i, _i],
    "llmie_decoder_prefill": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp],
    "llmie_lm_head_sample": [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp,
                             _i, _vp],
    "llmie_lm_head_sample_next": [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp,
                                  _i, _vp],
    "llmie_advance_step": [_vp, _vp],
    "llmie_sample_logits_workspace_bytes": [_i, _i],
    "llmie_sample_logits": [_vp, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _sz, _i, _vp],
    "llmie_sample_logits_ext": [_vp, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _sz, _i, _vp, _vp],
    "llmie_score_tokens_workspace_bytes": [_i, _i, _i],
    "llmie_score_tokens": [_vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _i, _vp],
    "llmie_lm_head_sample_params": [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _vp,
                                    _vp, _i, _vp, _sz, _vp],
    "llmie_lm_head_sample_ext": [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _vp,
                                 _vp, _i, _vp, _sz, _vp, _vp],
    "llmie_decoder_forward_paged": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "llmie_decoder_prefill_paged": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp, _sz, _vp],
    "llmie_kv_pages_copy": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "llmie_beam_step_workspace_bytes": [_i, _i, _i],
    "llmie_beam_step": [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _vp, _sz, _i, _vp],
    "llmie_kv_pages_fork_workspace_bytes": [_i, _i, _i, _i, _i, _i],
    "llmie_kv_pages_fork": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp],
    "llmie_spec_verify_workspace_bytes": [_i, _i, _i],
    "llmie_spec_verify": [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _sz,
                          _i, _vp, _vp],
    "llmie_ngram_draft": [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "llmie_spec_verify_sampled_workspace_bytes": [_i, _i, _i],
    "llmie_spec_verify_sampled": [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i,
                                  _vp, _i, _vp, _sz, _i, _vp, _vp],
    "llmie_spec_tree_prepare": [_vp, _vp, _i, _i, _vp, _vp, _vp],
    "llmie_spec_verify_tree_workspace_bytes": [_i, _i, _i],
    "llmie_spec_verify_tree": [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i,
                               _vp, _i, _vp, _sz, _i, _vp, _vp],
    "llmie_kv_tree_commit": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "llmie_ngram_draft_tree": [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "llmie_decoder_set_tree": [_vp, _vp, _vp, _i],
    "llmie_lora_table_bytes": [_i, _i],
    "llmie_lora_slot_load": [_vp, _i, _i, _i, _vp, _vp],
    "llmie_lora_workspace_bytes": [_i, _i, _i],
    "llmie_lora_plan": [_vp, _vp, _i, _i, _vp, _i, _vp, _sz, _vp],
    "llmie_lora_apply": [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _i, _vp],
    "llmie_decoder_lora_workspace_bytes": [_vp, _i, _i],
    "llmie_decoder_lora_attach": [_vp, _vp, _i, _vp, _vp, _sz],
    "llmie_decoder_lora_detach": [_vp],
    "llmie_decoder_set_window": [_vp, _vp, _i],
    "llmie_moe_workspace_bytes": [_i, _i, _i, _i, _i],
    "llmie_moe_ffn_plan": [_i, _i, _i, _i, _i, C.c_uint],
    "llmie_moe_route": [_vp, _vp, _i, _i, _i, _i, C.c_uint, _vp, _vp, _i, _vp],
    "llmie_moe_ffn": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, C.c_uint, _vp, _sz, _i, _vp],
    "llmie_decoder_moe_workspace_bytes": [_vp, _i, _i, _i, _i],
    "llmie_decoder_moe_attach": [_vp, _vp, _i, _i, _i, C.c_uint, _vp, _sz],
    "llmie_decoder_moe_detach": [_vp],
    "llmie_moe_ffn_plan_ex": [_i, _i, _i, _i, _i, C.c_uint, _i, _i],
    "llmie_moe_route_ex": [_vp, _vp, _i, _i, _i, _i, C.c_uint, _vp, _vp, _i, _vp],
    "llmie_moe_ffn_ex": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, C.c_uint, _vp, _sz, _i, _vp],
    "llmie_decoder_moe_attach_ex": [_vp, _vp, _i, _i, _i, C.c_uint, _vp, _sz],
    "llmie_decoder_profile_begin": [_vp, _i],
    "llmie_decoder_profile_end": [_vp, _vp, _vp, _vp],
    "llmie_decoder_status": [_vp, _vp],
    "llmie_decoder_resident_weight_bytes": [_vp],
    "llmie_decoder_repack": [_vp, _vp, _vp],
    "llmie_decoder_plan_name": [_vp, _i, _i, C.c_uint, C.c_uint],
    "llmie_decoder_prefill_layer_plan": [_vp, _i, _i, _i, C.c_uint, C.c_uint, _vp],
    "llmie_decoder_debug_stamps": [_vp, _vp],
    "llmie_abi_version": [],
    "llmie_last_error": [],
    "llmie_target_arch": [],
}
_RESTYPES = {
    "llmie_decoder_mha_workspace_bytes": _sz,
    "llmie_decoder_resident_weight_bytes": _sz,
    "llmie_linear_fp8_workspace_bytes": _sz,
    "llmie_linear_workspace_bytes": _sz,
    "llmie_packed_weight_bytes": _sz,
    "llmie_x32_bytes": _sz,
    "llmie_packed_scale_bytes": _sz,
    "llmie_linear_packed_workspace_bytes": _sz,
    "llmie_decoder_workspace_bytes": _sz,
    "llmie_decoder_prefill_workspace_bytes": _sz,
    "llmie_sample_logits_workspace_bytes": _sz,
    "llmie_score_tokens_workspace_bytes": _sz,
    "llmie_beam_step_workspace_bytes": _sz,
    "llmie_kv_pages_fork_workspace_bytes": _sz,
    "llmie_spec_verify_workspace_bytes": _sz,
    "llmie_spec_verify_sampled_workspace_bytes": _sz,
    "llmie_spec_verify_tree_workspace_bytes": _sz,
    "llmie_lora_table_bytes": _sz,
    "llmie_lora_workspace_bytes": _sz,
    "llmie_decoder_lora_workspace_bytes": _sz,
    "llmie_moe_workspace_bytes": _sz,
    "llmie_decoder_moe_workspace_bytes": _sz,
    "llmie_moe_ffn_plan": C.c_char_p,
    "llmie_moe_ffn_plan_ex": C.c_char_p,
    "llmie_decoder_create": _vp,
    "llmie_decoder_destroy": None,
    "llmie_last_error": C.c_char_p,
    "llmie_linear_route": C.c_char_p,
    "llmie_gemm256_tiles": C.c_char_p,
    "llmie_decoder_mha_plan": C.c_char_p,
    "llmie_decoder_mha_window_plan": C.c_char_p,
    "llmie_decoder_mha_sink_plan": C.c_char_p,
    "llmie_decoder_mha_qknorm_plan": C.c_char_p,
    "llmie_decoder_plan_name": C.c_char_p,
    "llmie_decoder_prefill_layer_plan": C.c_char_p,
    "llmie_target_arch": C.c_char_p,
}

EXPORTS = tuple(sorted(_SIGS))


def lib():
    """The loaded C-ABI library.  Raises (never falls back) when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LlmieError(
                "HIP library %s is missing: run `python llm-inference-engine_amd/build.py` "
                "(or __graft_entry__.build()).  There is no CPU fallback." % LIB_PATH)
        # torch ships its own libamdhip64; load it FIRST so libllmie.so binds to the same HIP runtime
        # (two runtimes in one process = "no ROCm-capable device" on the second one).
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, args in _SIGS.items():
            fn = getattr(l, name)  # AttributeError if the ABI lost a symbol
            fn.argtypes = args
            fn.restype = _RESTYPES.get(name, C.c_int)
        if l.llmie_abi_version() != ABI_VERSION:
            raise LlmieError("libllmie.so ABI version %d, this binding was written against %d (include/llmie.h)"
                             % (l.llmie_abi_version(), ABI_VERSION))
        _lib = l
    return _lib


def _check(rc, what):
    if rc != 0:
        raise LlmieError("%s failed (%d): %s" % (what, rc, lib().llmie_last_error().decode()))


def _dt(t):
    import torch
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    raise LlmieError("unsupported dtype %s" % t.dtype)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensors only"
    return t.data_ptr()


def _st():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ per-kernel wrappers
def input_embedding(ids, table, out):
    _check(lib().llmie_input_embedding(_p(ids), _p(table), _p(out), ids.numel(), table.shape[1], table.shape[0],
                                       _dt(table), _st()), "input_embedding")
    return out


def cal_padding_offset(padding_offset, cum_seqlens, lens):
    _check(lib().llmie_cal_padding_offset(_p(padding_offset), _p(cum_seqlens), _p(lens), lens.numel(),
                                          padding_offset.shape[1], _st()), "cal_padding_offset")


def build_causal_mask(mask, q_lens, k_lens):
    _check(lib().llmie_build_causal_mask(_p(mask), _p(q_lens), _p(k_lens), mask.shape[0], mask.shape[1],
                                         mask.shape[2], _dt(mask), _st()), "build_causal_mask")
    return mask


def rmsnorm(x, resid, gamma, eps):
    _check(lib().llmie_rmsnorm(_p(x), _p(resid), _p(gamma), eps, x.shape[0], x.shape[1], _dt(x), _st()), "rmsnorm")


def fused_add_bias_residual_rmsnorm(resid, out, bias, gamma, eps):
    _check(lib().llmie_fused_add_bias_residual_rmsnorm(_p(resid), _p(out), _p(bias), _p(gamma), eps, out.shape[0],
                                                       out.shape[1], _dt(out), _st()),
           "fused_add_bias_residual_rmsnorm")


def add_residual(resid, out):
    _check(lib().llmie_add_residual(_p(resid), _p(out), out.shape[0], out.shape[1], _dt(out), _st()), "add_residual")


def linear_workspace_bytes(fmt, M, K, N):
    """bytes of caller-owned split-K slab scratch llmie_linear / _swiglu / _w8a16 / _w4a16 use for this shape (0: none)"""
    return lib().llmie_linear_workspace_bytes(fmt, M, K, N)


def linear_route(fmt, x, w, scale, y, M, K, N, swiglu=False, group=0, bias=None, residual=None, workspace=None, workspace_bytes=0):
    """name of the kernel route the projection entry points plan for this call, None where they refuse it (llmie_last_error() says
    why).  The operands are ADDRESSES (ints, never dereferenced: only their alignment counts) -- no device needed.  fmt W_FP8: the
    route of linear_fp8 ("fp8_gemv", "fp8_gemm256", "fp8_splitk"), with scale = the fp32 row scales and a workspace of
    linear_fp8_workspace_bytes(M, K, N) bytes (the activation part, which has to be there, then the slabs)."""
    r = lib().llmie_linear_route(fmt, x, w, scale, y, M, K, N, int(swiglu), group, bias, residual, workspace, workspace_bytes)
    return r.decode() if r is not None else None


G256_FORMS = {"plain": 0, "swiglu": 1, "qkv_rope": 2}
G256_OPERANDS = {"f16": 0, "e4m3": 1, "int8": 2}


def gemm256_tiles(form, operands, M, N, K):
    """tile plan of the 256-row GEMM family for a projection of the form ("plain", "swiglu": N = two_inter, "qkv_rope") and operand
    format ("f16", "e4m3", "int8"): e.g. "8p 256x32@0 128x2@8192" (include/llmie.h); None for other arguments.  No device needed."""
    r = lib().llmie_gemm256_tiles(G256_FORMS[form], G256_OPERANDS[operands], M, N, K)
    return r.decode() if r is not None else None


ATTN_FORMS = {"step_dev": 1, "ragged": 2, "bias": 4, "rope": 8, "tickets": 16, "slabs": 32, "paged": 64, "x32": 128, "bad_scales": 256,
              "head_sink": 512, "qk_norm": 1024}
ATTN_OPERANDS = ("qkv", "bias", "k", "v", "slab", "wf", "wh", "slab_stride")


def decoder_mha_plan(dtype, batch, head_num, kv_head_num, head_size, max_seq_len, step=-1, kv_e4m3=False, forms=(), max_pages=0,
                     num_pages=0, residues=None, workspace_bytes="exact"):
    """(plan text or None, status) of the decode attention launch for a call (include/llmie.h): e.g. "split f16 hs128 rep4 kv=f16 cpw1
    chunk128 grid 3x2x4 merge 8x4/128" or "generic f32 grid 6x2 lds 1028"; None where the entries refuse the call (status = their
    error code, llmie_last_error() says why).  forms: names of ATTN_FORMS; residues: {operand of ATTN_OPERANDS: address % 16};
    workspace_bytes: a size, None (no workspace) or "exact".  No device needed."""
    f = sum(ATTN_FORMS[n] for n in forms)
    r = sum((v & 15) << (4 * ATTN_OPERANDS.index(k)) for k, v in (residues or {}).items())
    if workspace_bytes == "exact":
        workspace_bytes = lib().llmie_decoder_mha_workspace_bytes(batch, head_num, head_size, max_seq_len)
    status = C.c_int(0)
    t = lib().llmie_decoder_mha_plan(dtype, int(kv_e4m3), batch, head_num, kv_head_num, head_size, max_seq_len, step, f, max_pages,
                                     num_pages, r, -1 if workspace_bytes is None else workspace_bytes, C.addressof(status))
    return (t.decode() if t is not None else None), status.value


def decoder_mha_window_plan(dtype, batch, head_num, kv_head_num, head_size, max_seq_len, window, sinks=0, step=-1, kv_e4m3=False,
                            forms=(), max_pages=0, num_pages=0, residues=None, workspace_bytes="exact"):
    """decoder_mha_plan for a sliding-window call (llmie_decoder_mha_window_plan): with window > 0 the line ends in " window W sinks
    S live N" (host step: N live chunks = grid x) or "... live <=N" (device position: the bound the grid is launched with); window =
    0 gives decoder_mha_plan's text.  No device needed."""
    f = sum(ATTN_FORMS[n] for n in forms)
    r = sum((v & 15) << (4 * ATTN_OPERANDS.index(k)) for k, v in (residues or {}).items())
    if workspace_bytes == "exact":
        workspace_bytes = lib().llmie_decoder_mha_workspace_bytes(batch, head_num, head_size, max_seq_len)
    status = C.c_int(0)
    t = lib().llmie_decoder_mha_window_plan(dtype, int(kv_e4m3), batch, head_num, kv_head_num, head_size, max_seq_len, step, f,
                                            max_pages, num_pages, r, -1 if workspace_bytes is None else workspace_bytes, window, sinks,
                                            C.addressof(status))
    return (t.decode() if t is not None else None), status.value


def decoder_mha_sink_plan(dtype, batch, head_num, kv_head_num, head_size, max_seq_len, window=0, sinks=0, step=-1, kv_e4m3=False,
                          forms=(), max_pages=0, num_pages=0, residues=None, workspace_bytes="exact"):
    """decoder_mha_window_plan plus the form "head_sink" (llmie_decoder_mha_sink_plan): with it the line ends in " head_sink" -- the
    same grid, slots and merge on the SINK instantiation of the kernels -- or the call is refused where no such form exists.  No device
    needed."""
    f = sum(ATTN_FORMS[n] for n in forms)
    r = sum((v & 15) << (4 * ATTN_OPERANDS.index(k)) for k, v in (residues or {}).items())
    if workspace_bytes == "exact":
        workspace_bytes = lib().llmie_decoder_mha_workspace_bytes(batch, head_num, head_size, max_seq_len)
    status = C.c_int(0)
    t = lib().llmie_decoder_mha_sink_plan(dtype, int(kv_e4m3), batch, head_num, kv_head_num, head_size, max_seq_len, step, f,
                                          max_pages, num_pages, r, -1 if workspace_bytes is None else workspace_bytes, window, sinks,
                                          C.addressof(status))
    return (t.decode() if t is not None else None), status.value


def decoder_mha_qknorm_plan(dtype, batch, head_num, kv_head_num, head_size, max_seq_len, window=0, sinks=0, step=-1, kv_e4m3=False,
                            forms=(), max_pages=0, num_pages=0, residues=None, workspace_bytes="exact"):
    """decoder_mha_sink_plan plus the form "qk_norm" (llmie_decoder_mha_qknorm_plan): with it the line ends in " qk_norm" -- the same
    grid, slots and merge on the QKN instantiation of the split kernel -- or the call is refused where no such form exists (a QKV bias,
    a window, a head sink, fp32, head sizes other than 64 / 128, ratio 8 over e4m3, unaligned operands).  No device needed."""
    f = sum(ATTN_FORMS[n] for n in forms)
    r = sum((v & 15) << (4 * ATTN_OPERANDS.index(k)) for k, v in (residues or {}).items())
    if workspace_bytes == "exact":
        workspace_bytes = lib().llmie_decoder_mha_workspace_bytes(batch, head_num, head_size, max_seq_len)
    status = C.c_int(0)
    t = lib().llmie_decoder_mha_qknorm_plan(dtype, int(kv_e4m3), batch, head_num, kv_head_num, head_size, max_seq_len, step, f,
                                            max_pages, num_pages, r, -1 if workspace_bytes is None else workspace_bytes, window, sinks,
                                            C.addressof(status))
    return (t.decode() if t is not None else None), status.value


ROPE_NONE, ROPE_LINEAR, ROPE_LLAMA3, ROPE_YARN = 0, 1, 2, 3
ROPE_KINDS = {"none": ROPE_NONE, "linear": ROPE_LINEAR, "llama3": ROPE_LLAMA3, "yarn": ROPE_YARN}


class RopeScaling(C.Structure):
    """llmie_rope_scaling of include/llmie.h"""
    _fields_ = [("kind", _i), ("factor", _f), ("original_max_pos", _i), ("low_freq_factor", _f), ("high_freq_factor", _f),
                ("beta_fast", _f), ("beta_slow", _f), ("attn_factor", _f), ("truncate", _i)]


def rope_scaling(scaling):
    """None, a RopeScaling, or a dict of its fields (kind: a name of ROPE_KINDS or its number) -> RopeScaling or None"""
    if scaling is None or isinstance(scaling, RopeScaling):
        return scaling
    d = dict(scaling)
    kind = d.pop("kind")
    s = RopeScaling(kind=ROPE_KINDS[kind] if isinstance(kind, str) else int(kind))
    for k, v in d.items():
        if k not in dict(RopeScaling._fields_):
            raise LlmieError("rope_scaling: unknown field %r" % k)
        setattr(s, k, v)
    return s


def rope_table(max_pos, head_size, rotary_dim, base, scaling=None):
    """llmie_rope_table_fill: the (cos, sin) table as numpy float32 [max_pos, head_size // 2, 2]; scaling: see rope_scaling().  Host only."""
    import numpy as np
    shape = (max(int(max_pos), 0), max(int(head_size), 0) // 2, 2)
    buf = np.empty(max(shape[0] * shape[1] * 2, 1), np.float32)   # (never NULL: the entry's own shape checks answer a bad shape)
    sc = rope_scaling(scaling)
    _check(lib().llmie_rope_table_fill(buf.ctypes.data, max_pos, head_size, rotary_dim, base, C.addressof(sc) if sc is not None else None),
           "rope_table_fill")
    return buf[:shape[0] * shape[1] * 2].reshape(shape)


def decoder_plan_name(cfg, prefill, rows, call_flags=0, switch_mask=0):
    """name of the launch sequence an engine of `cfg` (dict or DecoderConfig) plans for a decode step at `rows` sequences or
    (prefill=True) a prefill of `rows` tokens; None where the call is refused (llmie_last_error() says why).  No device needed."""
    c = cfg if isinstance(cfg, DecoderConfig) else DecoderConfig(**cfg)
    r = lib().llmie_decoder_plan_name(C.byref(c), int(bool(prefill)), rows, call_flags, switch_mask)
    return r.decode() if r is not None else None


def decoder_resident_weight_bytes(cfg):
    """bytes of layer-matrix storage (row-major matrices, scales and packed images) an engine of `cfg` keeps resident"""
    c = cfg if isinstance(cfg, DecoderConfig) else DecoderConfig(**cfg)
    return lib().llmie_decoder_resident_weight_bytes(C.byref(c))


def decoder_prefill_layer_plan(cfg, tokens, batch=1, max_q_len=None, call_flags=0, switch_mask=0):
    """(plan text or None, status) of what one layer of a prefill of `tokens` tokens in `batch` sequences of at most `max_q_len`
    (default: tokens) launches on an engine of `cfg` (include/llmie.h): sequence, norm / QKV / attention / gate-up forms, launches per
    op; as a dict through plan_fields().  None where the pass is refused (llmie_last_error() says why).  No device needed."""
    c = cfg if isinstance(cfg, DecoderConfig) else DecoderConfig(**cfg)
    status = C.c_int(0)
    t = lib().llmie_decoder_prefill_layer_plan(C.byref(c), tokens, batch, tokens if max_q_len is None else max_q_len, call_flags, switch_mask,
                                               C.addressof(status))
    return (t.decode() if t is not None else None), status.value


def plan_fields(text):
    """{"path": ..., "qkv": ..., ..., "launches": {op: n}} of a llmie_decoder_prefill_layer_plan text"""
    forms, launches = text.split(" launches")
    words = forms.split(" ")
    return dict([("path", words[0])] + [w.split("=") for w in words[1:]],
                launches={k: int(v) for k, v in (w.split("=") for w in launches.split())})


_scratch = {}


def _auto_ws(fmt, M, K, N, device):
    """workspace="auto": one grow-only torch buffer per device, owned by this module (the C library itself never allocates)"""
    need = linear_workspace_bytes(fmt, M, K, N)
    if need == 0:
        return None
    import torch
    buf = _scratch.get(device)
    if buf is None or buf.numel() < need:
        buf = torch.empty(need, dtype=torch.uint8, device=device)
        _scratch[device] = buf
    return buf


def _ws_args(workspace, fmt, M, K, N, device):
    if isinstance(workspace, str):
        workspace = _auto_ws(fmt, M, K, N, device)
    return _p(workspace), (workspace.numel() * workspace.element_size() if workspace is not None else 0)


def linear(x, w, y, trans_b=True, bias=None, residual=None, workspace="auto"):
    """workspace: a device tensor of linear_workspace_bytes(W_F16, M, K, N) bytes, None (non-split kernels), or the string auto"""
    M, K = x.shape[0], x.numel() // x.shape[0]
    N = y.numel() // y.shape[0]
    wp, wb = _ws_args(workspace, W_F16, M, K, N, x.device)
    _check(lib().llmie_linear(_p(x), _p(w), _p(y), M, K, N, int(trans_b), _p(bias), _p(residual), _dt(x), wp, wb, _st()),
           "linear")
    return y


def linear_swiglu(x, w_gate_up, y, workspace="auto"):
    wp, wb = _ws_args(workspace, W_F16, x.shape[0], x.shape[1], w_gate_up.shape[0], x.device)
    _check(lib().llmie_linear_swiglu(_p(x), _p(w_gate_up), _p(y), x.shape[0], x.shape[1], w_gate_up.shape[0],
                                     _dt(x), wp, wb, _st()), "linear_swiglu")
    return y


def batched_gemm(a, b, c, trans_b):
    bs, nh, m, k = a.shape
    n = c.shape[3]
    _check(lib().llmie_batched_gemm(_p(a), _p(b), _p(c), bs * nh, m, n, k, int(trans_b), _dt(a), _st()),
           "batched_gemm")
    return c


def qkv_bias_transpose_rope(q, k, v, qkv, bias, padding_offset, history_len, rotary_dim, rotary_base):
    bs, nh, S, hs = q.shape
    _check(lib().llmie_qkv_bias_transpose_rope(_p(q), _p(k), _p(v), _p(qkv), _p(bias), _p(padding_offset),
                                               _p(history_len), bs, S, qkv.shape[0], nh, k.shape[1], hs,
                                               rotary_dim, rotary_base, _dt(qkv), _st()), "qkv_bias_transpose_rope")


def rope_decode(qkv, head_num, kv_head_num, step, rotary_dim, rotary_base, step_dev=None):
    _check(lib().llmie_rope_decode(_p(qkv), qkv.shape[0], head_num, kv_head_num, qkv.shape[2], step, _p(step_dev),
                                   rotary_dim, rotary_base, _dt(qkv), _st()), "rope_decode")


def decoder_mha_workspace_bytes(batch, head_num, head_size, max_seq_len):
    return lib().llmie_decoder_mha_workspace_bytes(batch, head_num, head_size, max_seq_len)


def decoder_mha(qkv, qkv_bias, k_cache, v_cache, out, layer, head_num, kv_head_num, step, workspace,
                step_dev=None):
    bs, _, hs = qkv.shape
    max_seq = k_cache.shape[3]
    _check(lib().llmie_decoder_mha(_p(qkv), _p(qkv_bias), _p(k_cache), _p(v_cache), _p(out), layer, bs, head_num,
                                   kv_head_num, hs, max_seq, step, _p(step_dev), _p(workspace),
                                   0 if workspace is None else workspace.numel() * workspace.element_size(),
                                   _dt(qkv), _st()), "decoder_mha")
    return out


def decoder_mha_ragged(qkv, qkv_bias, k_cache, v_cache, out, layer, head_num, kv_head_num, ctx_len, workspace, rope_table,
                       rotary_dim, max_seq_len, block_table=None):
    """ragged batch: ctx_len device int32 [batch]; caches dense [L, batch, kvh, max_seq, hs] or (block_table given) page pools
    [L, num_pages, kvh, 128, hs]"""
    batch, hs = qkv.shape[0], qkv.shape[-1]
    _check(lib().llmie_decoder_mha_ragged(_p(qkv), _p(qkv_bias), _p(k_cache), _p(v_cache), _p(out), layer, batch, head_num,
                                          kv_head_num, hs, max_seq_len, _p(ctx_len), _p(workspace),
                                          workspace.numel() * workspace.element_size(), _p(rope_table), rotary_dim,
                                          _p(block_table), block_table.shape[1] if block_table is not None else 0,
                                          k_cache.shape[1] if block_table is not None else 0, _dt(qkv), _st()),
           "decoder_mha_ragged")
    return out


def decoder_mha_window(qkv, qkv_bias, k_cache, v_cache, out, layer, head_num, kv_head_num, ctx_len, workspace, rope_table,
                       rotary_dim, max_seq_len, window, sinks=0, block_table=None, tickets=None, kv_scales=None):
    """decoder_mha_ragged under a sliding window of `window` tokens plus `sinks` sink tokens (window = 0: full attention).  tickets:
    zeroed int32 [batch, kv_head_num] = in-launch merge.  kv_scales = (k_scale, v_scale): the caches are uint8 e4m3 bytes (fp16
    activations).  Block-table entries of pages without a live key are never followed and may be -1."""
    batch, hs = qkv.shape[0], qkv.shape[-1]
    ks, vs = kv_scales if kv_scales is not None else (1.0, 1.0)
    _check(lib().llmie_decoder_mha_window(_p(qkv), _p(qkv_bias), _p(k_cache), _p(v_cache), _p(out), layer, batch, head_num,
                                          kv_head_num, hs, max_seq_len, _p(ctx_len), _p(workspace),
                                          0 if workspace is None else workspace.numel() * workspace.element_size(), _p(rope_table),
                                          rotary_dim, _p(block_table), block_table.shape[1] if block_table is not None else 0,
                                          k_cache.shape[1] if block_table is not None else 0, window, sinks, _p(tickets),
                                          int(kv_scales is not None), ks, vs, _dt(qkv), _st()), "decoder_mha_window")
    return out


def decoder_mha_sink(qkv, qkv_bias, k_cache, v_cache, out, layer, head_num, kv_head_num, ctx_len, workspace, rope_table,
                     rotary_dim, max_seq_len, head_sink, window=0, sinks=0, block_table=None, tickets=None, kv_scales=None):
    """decoder_mha_window plus a learned sink logit per query head (llmie_decoder_mha_sink): head_sink = float32 device tensor
    [head_num] (-inf = no sink for that head) or None = decoder_mha_window's call.  The softmax of head h runs over the visible keys and
    one extra column with logit head_sink[h] and no value row."""
    import torch
    batch, hs = qkv.shape[0], qkv.shape[-1]
    ks, vs = kv_scales if kv_scales is not None else (1.0, 1.0)
    if head_sink is not None:
        assert head_sink.dtype == torch.float32 and head_sink.numel() == head_num, "head_sink: float32 [head_num]"
    _check(lib().llmie_decoder_mha_sink(_p(qkv), _p(qkv_bias), _p(k_cache), _p(v_cache), _p(out), layer, batch, head_num,
                                        kv_head_num, hs, max_seq_len, _p(ctx_len), _p(workspace),
                                        0 if workspace is None else workspace.numel() * workspace.element_size(), _p(rope_table),
                                        rotary_dim, _p(block_table), block_table.shape[1] if block_table is not None else 0,
                                        k_cache.shape[1] if block_table is not None else 0, window, sinks, _p(tickets),
                                        int(kv_scales is not None), ks, vs, _p(head_sink), _dt(qkv), _st()), "decoder_mha_sink")
    return out


def qk_norm(qkv, head_num, kv_head_num, q_gamma, k_gamma, eps=1e-6):
    """per-head RMSNorm of the q and k heads of packed rows, in place (llmie_qk_norm; Qwen3 q_norm / k_norm): qkv = fp16 device tensor
    [rows, head_num + 2 kv_head_num, head_size]; q_gamma / k_gamma = fp16 device tensors [head_size].  The v columns are not touched."""
    rows, hs = qkv.shape[0], qkv.shape[-1]
    _check(lib().llmie_qk_norm(_p(qkv), rows, head_num, kv_head_num, hs, _p(q_gamma), _p(k_gamma), eps, _dt(qkv), _st()), "qk_norm")
    return qkv


def decoder_mha_qknorm(qkv, qkv_bias, k_cache, v_cache, out, layer, head_num, kv_head_num, ctx_len, workspace, rope_table,
                       rotary_dim, max_seq_len, q_gamma, k_gamma, qk_eps=1e-6, head_sink=None, window=0, sinks=0, block_table=None,
                       tickets=None, kv_scales=None):
    """decoder_mha_sink plus QK-norm (llmie_decoder_mha_qknorm): q_gamma / k_gamma = device tensors [head_size] in the activation
    type, or both None = decoder_mha_sink's call.  With gammas the result is qk_norm on qkv followed by decoder_mha_sink, bit for bit."""
    batch, hs = qkv.shape[0], qkv.shape[-1]
    ks, vs = kv_scales if kv_scales is not None else (1.0, 1.0)
    for g in (q_gamma, k_gamma):
        if g is not None:
            assert g.dtype == qkv.dtype and g.numel() == hs, "q_gamma / k_gamma: [head_size] in the activation type"
    _check(lib().llmie_decoder_mha_qknorm(_p(qkv), _p(qkv_bias), _p(k_cache), _p(v_cache), _p(out), layer, batch, head_num,
                                          kv_head_num, hs, max_seq_len, _p(ctx_len), _p(workspace),
                                          0 if workspace is None else workspace.numel() * workspace.element_size(), _p(rope_table),
                                          rotary_dim, _p(block_table), block_table.shape[1] if block_table is not None else 0,
                                          k_cache.shape[1] if block_table is not None else 0, window, sinks, _p(tickets),
                                          int(kv_scales is not None), ks, vs, _p(head_sink), _p(q_gamma), _p(k_gamma), qk_eps,
                                          _dt(qkv), _st()), "decoder_mha_qknorm")
    return out


def kv_window_advance(block_table, cached_len, window, sinks=0, new_tokens=None, status=None):
    """llmie_kv_window_advance: the page ring of windowed sequences.  block_table int32 [batch, max_pages] (in/out, -1 = unmapped),
    cached_len int32 [batch], new_tokens int32 [batch] or None (1 each); returns status int32 [batch] (0 ok, 1 no dead page:
    the row is untouched, 2 positions past the table).  One launch, no host read: capturable."""
    import torch
    batch, max_pages = block_table.shape
    if status is None:
        status = torch.empty(batch, dtype=torch.int32, device=block_table.device)
    _check(lib().llmie_kv_window_advance(_p(block_table), max_pages, _p(cached_len), _p(new_tokens), batch, window, sinks, _p(status),
                                         _st()), "kv_window_advance")
    return status


def decoder_mha_rope(qkv, qkv_bias, k_cache, v_cache, out, layer, head_num, kv_head_num, step, workspace, rope_table,
                     rotary_dim, tickets, step_dev=None):
    bs, _, hs = qkv.shape
    _check(lib().llmie_decoder_mha_rope(_p(qkv), _p(qkv_bias), _p(k_cache), _p(v_cache), _p(out), layer, bs, head_num,
                                        kv_head_num, hs, k_cache.shape[3], step, _p(step_dev), _p(workspace),
                                        workspace.numel() * workspace.element_size(), _p(rope_table), rotary_dim,
                                        _p(tickets), _dt(qkv), _st()), "decoder_mha_rope")
    return out


def concat_kv(src, cache, cur_len, history_len, layer):
    bs, kvh, max_q, hs = src.shape
    _check(lib().llmie_concat_kv(_p(src), _p(cache), _p(cur_len), _p(history_len), layer, bs, kvh, max_q,
                                 cache.shape[3], hs, _dt(src), _st()), "concat_kv")


def repeat_kv(cache, dst, ctx_len, layer):
    bs, nh, max_k, hs = dst.shape
    _check(lib().llmie_repeat_kv(_p(cache), _p(dst), _p(ctx_len), layer, bs, nh, cache.shape[2], max_k,
                                 cache.shape[3], hs, _dt(dst), _st()), "repeat_kv")


def scale_mask_softmax(qk, mask, out, scale):
    bs, nh, ql, kl = qk.shape
    _check(lib().llmie_scale_mask_softmax(_p(qk), _p(mask), _p(out), scale, bs, nh, ql, kl, _dt(qk), _st()),
           "scale_mask_softmax")
    return out


def transpose_remove_padding(src, padding_offset, dst):
    bs, nh, S, hs = src.shape
    _check(lib().llmie_transpose_remove_padding(_p(src), _p(dst), _p(padding_offset), dst.shape[0], bs, S, nh, hs,
                                                _dt(src), _st()), "transpose_remove_padding")
    return dst


def silu_and_mul(x, out):
    _check(lib().llmie_silu_and_mul(_p(x), _p(out), x.shape[0], x.shape[2], _dt(x), _st()), "silu_and_mul")
    return out


def topk(probs, tmp_ids, tmp_vals, ids, vals, blocks_per_row=8):
    rows, vocab = probs.shape
    K = ids.shape[-1]
    _check(lib().llmie_topk(_p(probs), _p(tmp_ids), _p(tmp_vals), _p(ids), _p(vals), rows, vocab, K, blocks_per_row,
                            _dt(probs), _st()), "topk")


def sampling(topk_id, topk_val, seq_len, finished, out_id, step, end_id, vocab, step_dev=None):
    bs, K = topk_id.shape
    _check(lib().llmie_sampling(_p(topk_id), _p(topk_val), _p(seq_len), _p(finished), _p(out_id), bs, K, step,
                                _p(step_dev), end_id, vocab, _dt(topk_val), _st()), "sampling")


def advance_step(step_dev):
    _check(lib().llmie_advance_step(_p(step_dev), _st()), "advance_step")


# ------------------------------------------------------------------ per-request sampling
SAMPLE_MAX_HISTORY = 8192  # LLMIE_SAMPLE_MAX_HISTORY
SAMPLING_DEFAULTS = dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0,
                         frequency_penalty=0.0, seed=0)


class SamplingParams(C.Structure):
    """llmie_sampling_params (include/llmie.h)"""
    _fields_ = [("temperature", _f), ("top_k", _i), ("top_p", _f), ("min_p", _f), ("repetition_penalty", _f),
                ("presence_penalty", _f), ("frequency_penalty", _f), ("seed", C.c_uint32)]


def sampling_params(rows, out=None, device="cuda"):
    """Pack a list of per-row dicts (missing keys: SAMPLING_DEFAULTS, i.e. plain sampling at temperature 1) into the device
    array llmie_sample_logits reads: a uint8 tensor of len(rows) * sizeof(llmie_sampling_params) bytes.  out: an existing
    array to overwrite in place (a captured graph then sees the new values on replay)."""
    import torch
    arr = (SamplingParams * len(rows))()
    for i, r in enumerate(rows):
        unknown = set(r) - set(SAMPLING_DEFAULTS)
        if unknown:
            raise LlmieError("unknown sampling parameters: %s" % ", ".join(sorted(unknown)))
        v = dict(SAMPLING_DEFAULTS, **r)
        arr[i] = SamplingParams(v["temperature"], int(v["top_k"]), v["top_p"], v["min_p"], v["repetition_penalty"],
                                v["presence_penalty"], v["frequency_penalty"], int(v["seed"]) & 0xffffffff)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    if out is None:
        return host.to(device)
    if out.numel() != host.numel():
        raise LlmieError("sampling_params: out holds %d bytes, %d rows need %d" % (out.numel(), len(rows), host.numel()))
    out.copy_(host)
    return out


def sample_logits_workspace_bytes(batch, vocab):
    return lib().llmie_sample_logits_workspace_bytes(batch, vocab)


def _sample_ws(workspace, batch, vocab, device):
    import torch
    need = sample_logits_workspace_bytes(batch, vocab)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
    return workspace, workspace.numel() * workspace.element_size()


SAMPLE_MAX_BIAS, SAMPLE_MAX_STOPS, SAMPLE_MAX_TOP_N = 1024, 16, 32  # LLMIE_SAMPLE_MAX_*


class SamplingExt(C.Structure):
    """llmie_sampling_ext (include/llmie.h): a host struct of device pointers"""
    _fields_ = [("allowed_mask", _vp), ("mask_stride", _i), ("mask_rows", _i), ("mask_index", _vp), ("bias_ids", _vp),
                ("bias_vals", _vp), ("bias_len", _vp), ("bias_stride", _i), ("stop_ids", _vp), ("stop_len", _vp),
                ("stop_stride", _i), ("min_step", _vp), ("top_n", _i), ("out_top_ids", _vp), ("out_top_logprobs", _vp)]


class SamplingExtArrays:
    """What sampling_ext() returns: the device arrays of one llmie_sampling_ext (kept alive here; None where a control is off)
    and the struct that points at them.  mask (int32 words [rows, stride]), mask_index, bias_ids / bias_vals / bias_len,
    stop_ids / stop_len and min_step can be rewritten in place -- a captured graph reads them on replay.  top_ids /
    top_logprobs [batch, top_n] receive the alternatives (None when top_n == 0)."""

    def __init__(self):
        self.mask = self.mask_index = self.bias_ids = self.bias_vals = self.bias_len = None
        self.stop_ids = self.stop_len = self.min_step = self.top_ids = self.top_logprobs = None
        self.struct = SamplingExt()


def pack_token_mask(allowed, stride=None):
    """bool array-like [rows, vocab] -> numpy uint32 words [rows, stride]: bit v % 32 of word v / 32 is token v"""
    import numpy as np
    a = np.asarray(allowed, dtype=bool)
    rows, V = a.shape
    words = (V + 31) // 32
    stride = words if stride is None else stride
    if stride < words:
        raise LlmieError("pack_token_mask: stride %d below the %d words of %d tokens" % (stride, words, V))
    bits = np.zeros((rows, stride * 32), dtype=bool)
    bits[:, :V] = a
    return np.packbits(bits.reshape(rows, stride, 32), axis=-1, bitorder="little").view("<u4").reshape(rows, stride)


def _i32(x, device):
    import numpy as np
    import torch
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64).astype(np.int32))).to(device)


def sampling_ext(batch, vocab, masks=None, mask_index=None, bias=None, stops=None, min_step=None, top_n=0, device="cuda", rows=None):
    """Build the device arrays of a llmie_sampling_ext for `batch` rows over `vocab` tokens (-> SamplingExtArrays).
    masks: bool [rows, vocab] (packed here), or words [rows, stride >= ceil(vocab / 32)] as a numpy uint32 / int32 array or an
    int32 tensor.  mask_index: [batch] ints, None = row b uses mask row b.  bias: per row a list of (id, value) pairs (or a
    dict).  stops: per row a list of ids.  min_step: [batch] ints.  top_n: alternatives to return per row.  rows: the entries of
    mask_index and the rows of the top-N outputs where they differ from batch (spec_verify: batch * (k + 1), one per position)."""
    import numpy as np
    import torch
    rows_n = batch if rows is None else rows
    x = SamplingExtArrays()
    e = x.struct
    if masks is not None:
        if isinstance(masks, torch.Tensor):
            if masks.dtype == torch.bool:
                masks = masks.cpu().numpy()
            else:
                x.mask = masks.to(device=device, dtype=torch.int32).contiguous()
        if x.mask is None:
            m = np.asarray(masks)
            m = pack_token_mask(m) if m.dtype == bool else np.ascontiguousarray(m).astype(np.uint32, copy=False)
            x.mask = torch.from_numpy(m.view(np.int32).copy()).to(device)
        if x.mask.dim() != 2:
            raise LlmieError("sampling_ext: masks must be [rows, vocab] bools or [rows, stride] words")
        e.allowed_mask, e.mask_rows, e.mask_stride = x.mask.data_ptr(), x.mask.shape[0], x.mask.shape[1]
    if mask_index is not None:
        x.mask_index = _i32(mask_index, device)
        e.mask_index = x.mask_index.data_ptr()
    if bias is not None:
        rows = [list(r.items()) if isinstance(r, dict) else list(r) for r in bias]
        if len(rows) != batch:
            raise LlmieError("sampling_ext: bias has %d rows, batch is %d" % (len(rows), batch))
        stride = max(1, max(len(r) for r in rows))
        ids = np.zeros((batch, stride), np.int32)
        vals = np.zeros((batch, stride), np.float32)
        for b, r in enumerate(rows):
            for j, (t, v) in enumerate(r):
                ids[b, j], vals[b, j] = t, v
        x.bias_ids, x.bias_vals = torch.from_numpy(ids).to(device), torch.from_numpy(vals).to(device)
        x.bias_len = _i32([len(r) for r in rows], device)
        e.bias_ids, e.bias_vals, e.bias_len, e.bias_stride = x.bias_ids.data_ptr(), x.bias_vals.data_ptr(), x.bias_len.data_ptr(), stride
    if stops is not None:
        rows = [list(r) for r in stops]
        if len(rows) != batch:
            raise LlmieError("sampling_ext: stops has %d rows, batch is %d" % (len(rows), batch))
        stride = max(1, max(len(r) for r in rows))
        ids = np.full((batch, stride), -1, np.int32)
        for b, r in enumerate(rows):
            ids[b, :len(r)] = r
        x.stop_ids = torch.from_numpy(ids).to(device)
        x.stop_len = _i32([len(r) for r in rows], device)
        e.stop_ids, e.stop_len, e.stop_stride = x.stop_ids.data_ptr(), x.stop_len.data_ptr(), stride
    if min_step is not None:
        x.min_step = _i32(min_step, device)
        e.min_step = x.min_step.data_ptr()
    for name, want in (("mask_index", rows_n), ("min_step", batch)):
        t = getattr(x, name)
        if t is not None and t.numel() != want:
            raise LlmieError("sampling_ext: %s has %d entries, %d expected" % (name, t.numel(), want))
    if top_n:
        x.top_ids = torch.full((rows_n, top_n), -2, dtype=torch.int32, device=device)
        x.top_logprobs = torch.zeros((rows_n, top_n), dtype=torch.float32, device=device)
        e.top_n, e.out_top_ids, e.out_top_logprobs = top_n, x.top_ids.data_ptr(), x.top_logprobs.data_ptr()
    return x


def _ext_ref(ext):
    """ext= of sample_logits / Decoder.lm_head_sample_params: a SamplingExtArrays or a SamplingExt -> what ctypes passes"""
    return C.byref(ext.struct if isinstance(ext, SamplingExtArrays) else ext)


def sample_logits(logits, params, seq_len, finished, out_id, step, end_id, history=None, history_len=None, append=False,
                  out_logprob=None, step_dev=None, workspace=None, ext=None):
    """llmie_sample_logits on logits [batch, vocab] (fp16 / fp32, read-only).  params: sampling_params(...) of batch rows.
    history: int32 [batch, stride] with history_len int32 [batch] (device), or None.  workspace: None allocates one.
    ext: sampling_ext(...) (or a SamplingExt) -> llmie_sample_logits_ext; None calls llmie_sample_logits."""
    bs, V = logits.shape
    ws, ws_bytes = _sample_ws(workspace, bs, V, logits.device)
    stride = 0 if history is None else history.shape[1]
    args = (_p(logits), bs, V, _p(params), _p(history), stride, _p(history_len), 1 if append else 0, _p(seq_len), _p(finished),
            _p(out_id), _p(out_logprob), step, _p(step_dev), end_id, _p(ws), ws_bytes, _dt(logits), _st())
    if ext is None:
        _check(lib().llmie_sample_logits(*args), "sample_logits")
    else:
        _check(lib().llmie_sample_logits_ext(*args, _ext_ref(ext)), "sample_logits_ext")


# ------------------------------------------------------------------ token scoring
def score_tokens_workspace_bytes(rows, hidden, vocab):
    return lib().llmie_score_tokens_workspace_bytes(rows, hidden, vocab)


_score_scratch = {}


def score_tokens(hidden, lm_head, targets, gamma=None, eps=0.0, bias=None, want_lse=False, want_argmax=False, workspace="auto"):
    """llmie_score_tokens: log-probability of targets[t] (int32, device; outside [0, V): no target -> 0) under
    softmax(rmsnorm(hidden[t]) . lm_head^T + bias), the logits kept in fp32 and never written.  hidden [rows, H] fp16 is left as
    it is; gamma None: no RMSNorm.  Returns the fp32 logprob tensor, or a tuple (logprob[, lse][, argmax int32, argmax_logprob]).
    workspace: a device tensor of score_tokens_workspace_bytes(rows, H, V) bytes, or the string auto (one grow-only buffer per
    device owned by this module; inside a graph capture pass a tensor, or make a first call outside)."""
    import torch
    rows, H = hidden.shape
    V = lm_head.shape[0]
    if isinstance(workspace, str):
        need = score_tokens_workspace_bytes(rows, H, V)
        workspace = _score_scratch.get(hidden.device)
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty(need, dtype=torch.uint8, device=hidden.device)
            _score_scratch[hidden.device] = workspace
    out = torch.empty(rows, dtype=torch.float32, device=hidden.device)
    lse = torch.empty(rows, dtype=torch.float32, device=hidden.device) if want_lse else None
    amax = torch.empty(rows, dtype=torch.int32, device=hidden.device) if want_argmax else None
    amax_lp = torch.empty(rows, dtype=torch.float32, device=hidden.device) if want_argmax else None
    _check(lib().llmie_score_tokens(_p(hidden), _p(gamma), eps, _p(lm_head), _p(bias), _p(targets), _p(out), _p(lse), _p(amax),
                                    _p(amax_lp), rows, H, V, _p(workspace),
                                    0 if workspace is None else workspace.numel() * workspace.element_size(), _dt(hidden), _st()),
           "score_tokens")
    res = (out,) + ((lse,) if want_lse else ()) + ((amax, amax_lp) if want_argmax else ())
    return res[0] if len(res) == 1 else res


# ------------------------------------------------------------------ fused decoder engine
class MoeLayer(C.Structure):   # llmie_moe_layer
    _fields_ = [("router", _vp), ("gate_up", _vp), ("down", _vp)]


class MoeExpertsDesc(C.Structure):   # llmie_moe_experts
    _fields_ = [("format", _i), ("router", _vp), ("router_bias", _vp), ("gate_up", _vp), ("gate_up_scale", _vp), ("gate_up_bias", _vp),
                ("down", _vp), ("down_scale", _vp), ("down_bias", _vp), ("act", _i), ("alpha", _f), ("limit", _f)]


class Matrix(C.Structure):
    _fields_ = [("data", _vp), ("scale", _vp), ("bias", _vp)]


class LayerWeights(C.Structure):
    _fields_ = [("attn_norm_gamma", _vp), ("qkv", Matrix), ("o", Matrix), ("ffn_norm_gamma", _vp),
                ("gate_up", Matrix), ("down", Matrix)]


class DecoderConfig(C.Structure):
    _fields_ = [("head_num", _i), ("kv_head_num", _i), ("head_size", _i), ("inter_size", _i), ("num_layers", _i),
                ("vocab_size", _i), ("max_seq_len", _i), ("max_batch", _i), ("rotary_dim", _i),
                ("rotary_base", _f), ("rms_eps", _f), ("dtype", _i), ("wfmt", _i), ("int4_group", _i),
                ("kv_fmt", _i), ("k_scale", _f), ("v_scale", _f), ("flags", _i)]


def _mat(m):
    """m: tensor | (data, scale) | (data, scale, bias) | dict"""
    if isinstance(m, dict):
        return Matrix(_p(m["data"]), _p(m.get("scale")), _p(m.get("bias")))
    if isinstance(m, (tuple, list)):
        m = list(m) + [None] * (3 - len(m))
        return Matrix(_p(m[0]), _p(m[1]), _p(m[2]))
    return Matrix(_p(m), None, None)


class Decoder:
    """Thin owner of an llmie_decoder handle + its workspace (torch only allocates the bytes).

    layers: list of dicts with keys attn_norm, qkv, o, ffn_norm, gate_up, down; matrix entries are a
    tensor (fp16/fp32 [N,K]) or dict(data=, scale=, bias=).
    """

    def __init__(self, cfg, layers):
        import torch
        self.cfg = DecoderConfig(**cfg)
        self._keep = layers  # keep the weight tensors alive
        arr = (LayerWeights * len(layers))()
        for i, lw in enumerate(layers):
            arr[i] = LayerWeights(_p(lw["attn_norm"]), _mat(lw["qkv"]), _mat(lw["o"]), _p(lw["ffn_norm"]),
                                  _mat(lw["gate_up"]), _mat(lw["down"]))
        nbytes = lib().llmie_decoder_workspace_bytes(C.byref(self.cfg))
        if nbytes == 0:
            raise LlmieError("invalid decoder config")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.handle = lib().llmie_decoder_create(C.byref(self.cfg), arr, self.workspace.data_ptr(), nbytes)
        if not self.handle:
            raise LlmieError("decoder_create: " + lib().llmie_last_error().decode())

    def forward(self, hidden_in, hidden_out, k_cache, v_cache, step, step_dev=None):
        _check(lib().llmie_decoder_forward(self.handle, _p(hidden_in), _p(hidden_out), _p(k_cache), _p(v_cache),
                                           hidden_in.shape[0], step, _p(step_dev), _st()), "decoder_forward")
        return hidden_out

    def forward_ragged(self, hidden_in, hidden_out, k_cache, v_cache, ctx_len):
        """ctx_len: device int32 [batch], context length of each sequence including this step's token"""
        _check(lib().llmie_decoder_forward_ragged(self.handle, _p(hidden_in), _p(hidden_out), _p(k_cache), _p(v_cache),
                                                  hidden_in.shape[0], _p(ctx_len), _st()), "decoder_forward_ragged")
        return hidden_out

    def forward_paged_ragged(self, hidden_in, hidden_out, k_pool, v_pool, block_table, ctx_len):
        _check(lib().llmie_decoder_forward_paged_ragged(self.handle, _p(hidden_in), _p(hidden_out), _p(k_pool), _p(v_pool),
                                                        _p(block_table), block_table.shape[1], k_pool.shape[1],
                                                        hidden_in.shape[0], _p(ctx_len), _st()), "decoder_forward_paged_ragged")
        return hidden_out

    def forward_paged(self, hidden_in, hidden_out, k_pool, v_pool, block_table, step, step_dev=None):
        """pools [L, num_pages, kvh, 128, hs]; block_table int32 [batch, max_pages] (device)"""
        _check(lib().llmie_decoder_forward_paged(self.handle, _p(hidden_in), _p(hidden_out), _p(k_pool), _p(v_pool),
                                                 _p(block_table), block_table.shape[1], k_pool.shape[1], hidden_in.shape[0],
                                                 step, _p(step_dev), _st()), "decoder_forward_paged")
        return hidden_out

    def prefill(self, hidden_in, hidden_out, k_cache, v_cache, input_lengths, history_lengths, max_q_len):
        import torch
        T, bs = hidden_in.shape[0], input_lengths.numel()
        need = lib().llmie_decoder_prefill_workspace_bytes(C.byref(self.cfg), T, bs)
        if getattr(self, "_pf_ws", None) is None or self._pf_ws.numel() < need:
            self._pf_ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        _check(lib().llmie_decoder_prefill(self.handle, _p(hidden_in), _p(hidden_out), _p(k_cache), _p(v_cache),
                                           _p(input_lengths), _p(history_lengths), bs, T, max_q_len,
                                           self._pf_ws.data_ptr(), self._pf_ws.numel(), _st()), "decoder_prefill")
        return hidden_out

    def prefill_paged(self, hidden_in, hidden_out, k_pool, v_pool, block_table, input_lengths, history_lengths, max_q_len):
        """prefill on the paged cache of forward_paged (pools [L, num_pages, kvh, 128, hs])"""
        import torch
        T, bs = hidden_in.shape[0], input_lengths.numel()
        need = lib().llmie_decoder_prefill_workspace_bytes(C.byref(self.cfg), T, bs)
        if getattr(self, "_pf_ws", None) is None or self._pf_ws.numel() < need:
            self._pf_ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        _check(lib().llmie_decoder_prefill_paged(self.handle, _p(hidden_in), _p(hidden_out), _p(k_pool), _p(v_pool),
                                                 _p(block_table), block_table.shape[1], k_pool.shape[1], _p(input_lengths),
                                                 _p(history_lengths), bs, T, max_q_len, self._pf_ws.data_ptr(),
                                                 self._pf_ws.numel(), _st()), "decoder_prefill_paged")
        return hidden_out

    def lm_head_sample(self, hidden, final_gamma, lm_head, lm_fmt, logits, tmp_ids, tmp_vals, topk_ids, topk_vals,
                       seq_len, finished, out_ids, step, end_id, blocks_per_row=8, step_dev=None, embed=None, next_hidden=None,
                       advance=False, fused_tail=False):
        """fused_tail (or embed / advance): llmie_lm_head_sample_next -- top-k round 2 + sampling (+ next_hidden[b] = embed[out_ids[b]])
        (+ step_dev += 1) in one launch"""
        m = _mat(lm_head)
        if fused_tail or embed is not None or advance:
            _check(lib().llmie_lm_head_sample_next(self.handle, _p(hidden), _p(final_gamma), C.byref(m), lm_fmt, _p(logits),
                                                   _p(tmp_ids), _p(tmp_vals), _p(topk_ids), _p(topk_vals), topk_ids.shape[-1],
                                                   blocks_per_row, _p(seq_len), _p(finished), _p(out_ids), hidden.shape[0], step,
                                                   _p(step_dev), end_id, _p(embed), _p(next_hidden), 1 if advance else 0, _st()),
                   "lm_head_sample_next")
            return
        _check(lib().llmie_lm_head_sample(self.handle, _p(hidden), _p(final_gamma), C.byref(m), lm_fmt, _p(logits),
                                          _p(tmp_ids), _p(tmp_vals), _p(topk_ids), _p(topk_vals),
                                          topk_ids.shape[-1], blocks_per_row, _p(seq_len), _p(finished), _p(out_ids),
                                          hidden.shape[0], step, _p(step_dev), end_id, _st()), "lm_head_sample")

    def lm_head_sample_params(self, hidden, final_gamma, lm_head, lm_fmt, logits, params, seq_len, finished, out_ids, step,
                              end_id, history=None, history_len=None, append=False, out_logprob=None, step_dev=None, embed=None,
                              next_hidden=None, advance=False, workspace=None, ext=None):
        """llmie_lm_head_sample_params: the LM head of lm_head_sample, then sample_logits (+ next_hidden[b] = embed[out_ids[b]])
        (+ step_dev += 1).  workspace: sample_logits_workspace_bytes(batch, vocab) bytes, or None to allocate one (not
        inside a graph capture).  ext: sampling_ext(...) (or a SamplingExt) -> llmie_lm_head_sample_ext."""
        m = _mat(lm_head)
        bs = hidden.shape[0]
        ws, ws_bytes = _sample_ws(workspace, bs, self.cfg.vocab_size, hidden.device)
        stride = 0 if history is None else history.shape[1]
        args = (self.handle, _p(hidden), _p(final_gamma), C.byref(m), lm_fmt, _p(logits), _p(params), _p(history), stride,
                _p(history_len), 1 if append else 0, _p(seq_len), _p(finished), _p(out_ids), _p(out_logprob), bs, step,
                _p(step_dev), end_id, _p(embed), _p(next_hidden), 1 if advance else 0, _p(ws), ws_bytes, _st())
        if ext is None:
            _check(lib().llmie_lm_head_sample_params(*args), "lm_head_sample_params")
        else:
            _check(lib().llmie_lm_head_sample_ext(*args, _ext_ref(ext)), "lm_head_sample_ext")

    OPS = ("attn_norm", "qkv_gemm", "rope", "mha", "o_gemm", "ffn_norm", "gate_up_swiglu", "down_gemm",
           "final_norm", "lm_head", "topk", "sampling", "chain")

    def lora_workspace_bytes(self, max_tokens, slots):
        return lib().llmie_decoder_lora_workspace_bytes(C.byref(self.cfg), max_tokens, slots)

    def lora_attach(self, table, seq_slot, max_tokens=None, workspace=None):
        """While attached, every forward / prefill entry runs the lora sequence: seq_slot (device int32) holds the slot of batch
        row b (decode) or of sequence b (prefill), -1 = no adapter; it and the table are read on the device at every launch.
        max_tokens: the most rows a call will bring (default: max_batch); workspace: a uint8 tensor of lora_workspace_bytes, or None
        to allocate it."""
        import torch
        assert table.layers == self.cfg.num_layers, "the table must have the engine's layer count"
        need = self.lora_workspace_bytes(max_tokens or self.cfg.max_batch, table.slots)
        if workspace is None:
            workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=table.data.device)
        _check(lib().llmie_decoder_lora_attach(self.handle, _p(table.data), table.slots, _p(seq_slot), _p(workspace), workspace.numel()),
               "decoder_lora_attach")
        self._lora_keep = (table, seq_slot, workspace)
        return workspace

    def set_window(self, layer_window, sinks=0):
        """sliding-window attention (llmie_decoder_set_window): layer_window = one window per layer (0 = full attention on that layer),
        or one int for every layer, or None to clear; sinks = sink tokens of the windowed layers"""
        if layer_window is None:
            _check(lib().llmie_decoder_set_window(self.handle, None, sinks), "decoder_set_window")
            return
        L = self.cfg.num_layers
        w = [int(layer_window)] * L if isinstance(layer_window, int) else [int(x) for x in layer_window]
        if len(w) != L:
            raise LlmieError("set_window: %d windows for %d layers" % (len(w), L))
        arr = (C.c_int32 * L)(*w)
        _check(lib().llmie_decoder_set_window(self.handle, C.addressof(arr), sinks), "decoder_set_window")

    def set_head_sinks(self, head_sink):
        """learned per-head sink logits (llmie_decoder_set_head_sinks): a float32 device tensor [num_layers, head_num] (-inf = no
        sink for that head), kept alive by this object and read on the device at every attention launch; None clears"""
        import torch
        if head_sink is not None:
            if head_sink.dtype != torch.float32 or tuple(head_sink.shape) != (self.cfg.num_layers, self.cfg.head_num):
                raise LlmieError("set_head_sinks: needs a float32 tensor [num_layers=%d, head_num=%d]" % (self.cfg.num_layers, self.cfg.head_num))
        _check(lib().llmie_decoder_set_head_sinks(self.handle, _p(head_sink)), "decoder_set_head_sinks")
        self._head_sinks_keep = head_sink

    def set_qk_norm(self, q_gamma, k_gamma, eps=1e-6):
        """QK-norm (llmie_decoder_set_qk_norm; Qwen3 q_norm / k_norm): fp16 device tensors [num_layers, head_size] each, kept alive by
        this object and read on the device at every attention launch; both None clears"""
        import torch
        for name, g in (("q_gamma", q_gamma), ("k_gamma", k_gamma)):
            if g is not None and (g.dtype != torch.float16 or tuple(g.shape) != (self.cfg.num_layers, self.cfg.head_size)):
                raise LlmieError("set_qk_norm: %s needs a float16 tensor [num_layers=%d, head_size=%d]"
                                 % (name, self.cfg.num_layers, self.cfg.head_size))
        _check(lib().llmie_decoder_set_qk_norm(self.handle, _p(q_gamma), _p(k_gamma), eps), "decoder_set_qk_norm")
        self._qk_norm_keep = (q_gamma, k_gamma)

    def set_tree(self, depth, anc):
        """a draft tree (llmie_decoder_set_tree): depth int32 / anc int64 device tensors [batch, stride] as spec_tree_prepare leaves
        them, kept alive by this object and read on the device at every prefill launch; both None clears"""
        import torch
        if depth is None and anc is None:
            _check(lib().llmie_decoder_set_tree(self.handle, None, None, 0), "decoder_set_tree")
            self._tree_keep = None
            return
        if depth is not None and anc is not None:
            if (depth.dtype != torch.int32 or anc.dtype != torch.int64 or depth.dim() != 2 or tuple(depth.shape) != tuple(anc.shape)
                    or not depth.is_contiguous() or not anc.is_contiguous()):
                raise LlmieError("set_tree: needs contiguous int32 depth and int64 anc tensors of one shape [batch, stride]")
        stride = (depth if depth is not None else anc).shape[-1]
        _check(lib().llmie_decoder_set_tree(self.handle, _p(depth), _p(anc), stride), "decoder_set_tree")
        self._tree_keep = (depth, anc)

    def set_rope_scaling(self, scaling):
        """RoPE frequency scaling (llmie_decoder_set_rope_scaling): refills and uploads the engine's (cos, sin) table -- one synchronous
        copy, not inside a graph capture.  scaling: see rope_scaling(); None restores the create-time table"""
        sc = rope_scaling(scaling)
        _check(lib().llmie_decoder_set_rope_scaling(self.handle, C.addressof(sc) if sc is not None else None), "decoder_set_rope_scaling")

    def moe_workspace_bytes(self, max_tokens, inter, experts, top_k):
        return lib().llmie_decoder_moe_workspace_bytes(C.byref(self.cfg), max_tokens, inter, experts, top_k)

    def moe_attach(self, layers, top_k, flags=0, max_tokens=None, workspace=None):
        """While attached, every forward / prefill entry runs the moe sequence.  layers: one entry per layer, None (the layer keeps
        its dense FFN) or a dict / tuple (router [E, H], gate_up [E, 2 Ie, H], down [E, H, Ie]) of fp16 device tensors.  max_tokens:
        the most rows a call will bring (default: max_batch); workspace: a uint8 tensor of moe_workspace_bytes, or None (one is made).
        With a MoeExperts descriptor among the layers the call is llmie_decoder_moe_attach_ex; tuples / dicts beside it count as fp16
        experts."""
        if any(isinstance(lw, MoeExperts) for lw in layers):
            return self._moe_attach(layers, MoeExpertsDesc, self._moe_layer_ex, lib().llmie_decoder_moe_attach_ex, "decoder_moe_attach_ex", top_k,
                                    flags, max_tokens, workspace)
        return self._moe_attach(layers, MoeLayer, self._moe_layer, lib().llmie_decoder_moe_attach, "decoder_moe_attach", top_k, flags, max_tokens,
                                workspace)

    # one sparse layer -> ((inter, experts), or None where its tensors disagree with `shape`; the entry's struct; what keeps it alive)
    @staticmethod
    def _moe_layer(lw, shape):
        r, gu, dn = (lw["router"], lw["gate_up"], lw["down"]) if isinstance(lw, dict) else lw
        own = (gu.shape[1] // 2, gu.shape[0])
        inter, experts = shape or own
        agree = r.shape[0] == experts and tuple(dn.shape[:1]) == (experts,) and dn.shape[2] == inter
        return own if agree else None, MoeLayer(_p(r), _p(gu), _p(dn)), (r, gu, dn)

    @staticmethod
    def _moe_layer_ex(lw, shape):
        if not isinstance(lw, MoeExperts):
            lw = MoeExperts(*((lw["router"], lw["gate_up"], lw["down"]) if isinstance(lw, dict) else lw))
        return (lw.inter, lw.experts), lw.desc(), lw

    def _moe_attach(self, layers, struct, layer, attach, who, top_k, flags, max_tokens, workspace):
        """what the two attach entries share: the layer walk, the shape agreement, the workspace and what is kept alive"""
        import torch
        arr = (struct * len(layers))()
        keep, shape = [], None
        for i, lw in enumerate(layers):
            if lw is None:
                continue
            own, arr[i], alive = layer(lw, shape)
            shape = shape or own
            if own is None or own != shape:
                raise LlmieError("moe_attach: layer %d: expert shapes differ from the first sparse layer's" % i)
            keep.append(alive)
        if shape is None:
            raise LlmieError("moe_attach: no layer has experts")
        inter, experts = shape
        if workspace is None:
            need = self.moe_workspace_bytes(max_tokens or self.cfg.max_batch, inter, experts, top_k)
            workspace = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
        _check(attach(self.handle, arr, inter, experts, top_k, flags, _p(workspace), workspace.numel()), who)
        self._moe_keep = (keep, workspace)
        return workspace

    def moe_detach(self):
        _check(lib().llmie_decoder_moe_detach(self.handle), "decoder_moe_detach")
        self._moe_keep = None

    def lora_detach(self):
        _check(lib().llmie_decoder_lora_detach(self.handle), "decoder_lora_detach")
        self._lora_keep = None

    def profile_begin(self, max_events):
        _check(lib().llmie_decoder_profile_begin(self.handle, max_events), "decoder_profile_begin")

    def profile_end(self):
        """-> {op: (total_ms, launches)}; synchronises the current stream"""
        ms = (C.c_double * len(self.OPS))()
        n = (C.c_int * len(self.OPS))()
        _check(lib().llmie_decoder_profile_end(self.handle, _st(), ms, n), "decoder_profile_end")
        return {op: (ms[i], n[i]) for i, op in enumerate(self.OPS)}

    def repack(self, layers):
        """rebuild the tile-packed weight images from `layers` (same structure as at construction)"""
        arr = (LayerWeights * len(layers))()
        for i, lw in enumerate(layers):
            arr[i] = LayerWeights(_p(lw["attn_norm"]), _mat(lw["qkv"]), _mat(lw["o"]), _p(lw["ffn_norm"]), _mat(lw["gate_up"]), _mat(lw["down"]))
        _check(lib().llmie_decoder_repack(self.handle, arr, _st()), "decoder_repack")
        self._keep = layers

    def debug_stamps(self, buf):
        """diagnostic: chain launches write their phase-edge timestamps into buf (uint64 [256, 16] on the device); None disarms"""
        _check(lib().llmie_decoder_debug_stamps(self.handle, _p(buf)), "decoder_debug_stamps")

    def status(self):
        """synchronises the current stream; raises if a grid barrier of a persistent chain launch timed out"""
        _check(lib().llmie_decoder_status(self.handle, _st()), "decoder_status")

    def close(self):
        if self.handle:
            lib().llmie_decoder_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ multi-LoRA: per-request adapters
LORA_MODULES = ("qkv", "o", "gate_up", "down")   # LLMIE_LORA_QKV ... LLMIE_LORA_DOWN
LORA_RANKS = (8, 16, 32, 64)
LORA_MAX_SLOTS = 1024   # LLMIE_LORA_MAX_SLOTS
LORA_MAX_KSPLIT = 8     # LLMIE_LORA_MAX_KSPLIT
PLAN_LORA = 1024        # LLMIE_PLAN_LORA
PLAN_WINDOW = 2048      # LLMIE_PLAN_WINDOW
PLAN_HEAD_SINK = 4096   # LLMIE_PLAN_HEAD_SINK
PLAN_QK_NORM = 8192     # LLMIE_PLAN_QK_NORM
PLAN_TREE = 16384       # LLMIE_PLAN_TREE
PLAN_PAGED, PLAN_RAGGED, PLAN_HIDDEN_MISALIGNED = 1, 2, 4   # LLMIE_PLAN_* call flags of decoder_plan_name


class LoraLayer(C.Structure):
    _fields_ = [("a", _vp * 4), ("b", _vp * 4)]


class LoraAdapter(C.Structure):
    _fields_ = [("rank", _i), ("scale", _f), ("layers", _i), ("layer", C.POINTER(LoraLayer))]


class LoraTable:
    """The device slot table of llmie_lora_*: `data` (uint8, zeroed = every slot empty) plus the tensors its slots point to."""

    def __init__(self, data, slots, layers):
        self.data, self.slots, self.layers = data, slots, layers
        self.keep = [None] * slots


def lora_table(slots, layers, device="cuda"):
    import torch
    n = lib().llmie_lora_table_bytes(slots, layers)
    if n == 0:
        raise LlmieError("lora_table: bad shape slots=%d layers=%d" % (slots, layers))
    return LoraTable(torch.zeros(n, dtype=torch.uint8, device=device), slots, layers)


def _lora_stack(m, parts):
    """one module's (A, B): the fused pair, or the separate projections' pairs stacked (A rows block after block, B rows too)"""
    import torch
    if m is None:
        m = parts
    if m is None or (isinstance(m, (tuple, list)) and all(x is None for x in m)):
        return None
    if any(x is None for x in m):   # separate projections with one missing, or a pair without its A or B
        raise LlmieError("lora_slot_load: a fused module needs the adapter of every block (pass zero matrices for a missing one), "
                         "and every A its B")
    if isinstance(m[0], (tuple, list)):   # ((A_q, B_q), (A_k, B_k), (A_v, B_v))
        return torch.cat([x[0] for x in m], 0).contiguous(), torch.cat([x[1] for x in m], 0).contiguous()
    return m[0].contiguous(), m[1].contiguous()


def lora_slot_load(table, slot, adapter, scale=1.0):
    """adapter: None (empties the slot) or a list with one dict per layer.  Keys: qkv / o / gate_up / down -> (A, B) with A
    [blocks * rank, K] and B [N, rank], fp16 device tensors; or q, k, v (all three) and gate, up (both) -> (A [rank, K], B [n, rank])
    pairs of the separate projections, stacked here onto the fused matrices.  A missing key: the adapter lacks the module.  A zero
    block (no k_proj adapter, say) is a pair of zero matrices.  Enqueued on the current stream."""
    if adapter is None:
        _check(lib().llmie_lora_slot_load(_p(table.data), table.slots, table.layers, slot, None, _st()), "lora_slot_load")
        if 0 <= slot < table.slots:
            # (the tensors of the adapter that was loaded stay referenced until the next load: launches already enqueued may read them)
            table.keep[slot] = (table.keep[slot][1] or table.keep[slot][0] if table.keep[slot] else None, None)
        return
    arr = (LoraLayer * len(adapter))()
    keep, rank = [], 0
    for i, lw in enumerate(adapter):
        sep = {"qkv": ("q", "k", "v"), "gate_up": ("gate", "up")}
        for mo, name in enumerate(LORA_MODULES):
            parts = [lw.get(k) for k in sep[name]] if name in sep else None
            ab = _lora_stack(lw.get(name), parts)
            if ab is None:
                continue
            keep.append(ab)
            rank = rank or ab[1].shape[1]
            if ab[1].shape[1] != rank or ab[0].shape[0] % rank:
                raise LlmieError("lora_slot_load: layer %d module %s has rank %d (A rows %d), the adapter's first module has %d"
                                 % (i, name, ab[1].shape[1], ab[0].shape[0], rank))
            arr[i].a[mo], arr[i].b[mo] = _p(ab[0]), _p(ab[1])
    desc = LoraAdapter(rank, scale, len(adapter), arr)
    _check(lib().llmie_lora_slot_load(_p(table.data), table.slots, table.layers, slot, C.byref(desc), _st()), "lora_slot_load")
    table.keep[slot] = (table.keep[slot][1] or table.keep[slot][0] if table.keep[slot] else None, keep)


def lora_workspace_bytes(max_rows, slots, max_rank_total=192):
    return lib().llmie_lora_workspace_bytes(max_rows, slots, max_rank_total)


def lora_plan(slot, table, workspace, lengths=None, rows=None):
    """one launch per forward call: groups the rows of each slot into tiles of <= 16.  lengths (device int32 [batch]): slot holds one
    entry per sequence and is expanded over the lengths; rows: the packed token count then (default slot.numel())."""
    batch = slot.numel()
    rows = rows if rows is not None else batch
    _check(lib().llmie_lora_plan(_p(slot), _p(lengths), batch, rows, _p(table.data), table.slots, _p(workspace), workspace.numel(), _st()),
           "lora_plan")


def lora_apply(x, y, table, layer, module, workspace, block_widths=None):
    """y[m] += scale_s * B_s . (A_s . x[m]) for every row with a loaded slot (include/llmie.h), on the plan lora_plan left in
    `workspace`.  module: index or name in LORA_MODULES; block_widths: the column blocks of y (default: one block)."""
    if isinstance(module, str):
        module = LORA_MODULES.index(module)
    rows, K = x.shape
    N = y.shape[1]
    widths = list(block_widths) if block_widths is not None else [N]
    arr = (C.c_int * len(widths))(*widths)
    _check(lib().llmie_lora_apply(_p(x), _p(y), rows, K, N, len(widths), arr, _p(table.data), table.slots, table.layers, layer, module,
                                  _p(workspace), workspace.numel(), _dt(x), _st()), "lora_apply")
    return y


# ------------------------------------------------------------------ mixture-of-experts FFN
MOE_MAX_EXPERTS, MOE_MAX_TOP_K = 128, 8                           # LLMIE_MOE_MAX_EXPERTS, LLMIE_MOE_MAX_TOP_K
MOE_SOFTMAX_ALL, MOE_FORCE_GEMV, MOE_FORCE_GROUPED = 1, 2, 4      # LLMIE_MOE_* flags
MOE_FORCE_RT1, MOE_FORCE_RT4 = 8, 16


def moe_workspace(max_rows, hidden, inter, experts, top_k, device="cuda"):
    """a uint8 workspace that covers moe_ffn at every row count up to max_rows"""
    import torch
    n = lib().llmie_moe_workspace_bytes(max_rows, hidden, inter, experts, top_k)
    if n == 0:
        raise LlmieError("moe_workspace: bad shape: %s" % lib().llmie_last_error().decode())
    return torch.empty(n, dtype=torch.uint8, device=device)


def moe_ffn_plan(rows, hidden, inter, experts, top_k, flags=0):
    """the one-line plan of a moe_ffn call, space-separated key=value words; raises where the call would be refused"""
    s = lib().llmie_moe_ffn_plan(rows, hidden, inter, experts, top_k, flags)
    if s is None:
        raise LlmieError("moe_ffn_plan: %s" % lib().llmie_last_error().decode())
    return s.decode()


def moe_route(x, router, top_k, flags=0, expert=None, weight=None):
    """(expert ids int32 [rows, top_k], weights fp32 [rows, top_k]) of every row of x under the router matrix [experts, hidden]"""
    import torch
    rows, H = x.shape
    E = router.shape[0]
    if expert is None:
        expert = torch.empty((rows, top_k), dtype=torch.int32, device=x.device)
    if weight is None:
        weight = torch.empty((rows, top_k), dtype=torch.float32, device=x.device)
    _check(lib().llmie_moe_route(_p(x), _p(router), rows, H, E, top_k, flags, _p(expert), _p(weight), _dt(x), _st()), "moe_route")
    return expert, weight


def moe_ffn(x, router, gate_up, down, y, top_k, resid=None, flags=0, workspace=None, rows=None, workspace_bytes=None):
    """y = MoE FFN of x (+ resid): router [E, H], gate_up [E, 2 Ie, H], down [E, H, Ie] (include/llmie.h states the arithmetic).
    workspace: a uint8 tensor from moe_workspace (None: one is made for this call)."""
    rows = x.shape[0] if rows is None else rows
    H = x.shape[1]
    E, Ie = gate_up.shape[0], gate_up.shape[1] // 2
    if workspace is None:
        workspace = moe_workspace(rows, H, Ie, E, top_k, device=x.device)
    nbytes = workspace.numel() if workspace_bytes is None else workspace_bytes
    _check(lib().llmie_moe_ffn(_p(x), _p(router), _p(gate_up), _p(down), _p(resid), _p(y), rows, H, Ie, E, top_k, flags, _p(workspace), nbytes,
                               _dt(x), _st()), "moe_ffn")
    return y


MOE_ACT_SWIGLU, MOE_ACT_SWIGLU_CLAMPED = 0, 1                      # llmie_moe_act


class MoeExperts:
    """The expert descriptor of the _ex entries (llmie_moe_experts): device tensors, kept alive by this object.
    fp16 experts: gate_up [E, 2 Ie, H], down [E, H, Ie] fp16, no scales.  MXFP4 experts: gate_up uint8 codes [E, 2 Ie, H / 2] with
    gate_up_scale uint8 [E, 2 Ie, H / 32], down uint8 [E, H, Ie / 2] with down_scale [E, H, Ie / 32] (MoeExperts.quantize makes them).
    Optional fp16 biases: router_bias [E], gate_up_bias [E, 2 Ie], down_bias [E, H].  act: MOE_ACT_SWIGLU, or MOE_ACT_SWIGLU_CLAMPED
    with alpha and limit (gpt-oss: 1.702, 7.0)."""

    def __init__(self, router, gate_up, down, gate_up_scale=None, down_scale=None, router_bias=None, gate_up_bias=None, down_bias=None,
                 act=MOE_ACT_SWIGLU, alpha=0.0, limit=0.0, format=None):
        self.router, self.gate_up, self.down = router, gate_up, down
        self.gate_up_scale, self.down_scale = gate_up_scale, down_scale
        self.router_bias, self.gate_up_bias, self.down_bias = router_bias, gate_up_bias, down_bias
        self.act, self.alpha, self.limit = act, alpha, limit
        self.format = (W_MXFP4 if gate_up_scale is not None or down_scale is not None else W_F16) if format is None else format
        self.experts, self.inter = gate_up.shape[0], gate_up.shape[1] // 2
        self.hidden = down.shape[1]

    @classmethod
    def quantize(cls, router, gate_up, down, **kw):
        """MXFP4 experts from fp16 gate_up [E, 2 Ie, H] and down [E, H, Ie]: llmie_quantize_mxfp4 on the flattened matrices"""
        import torch
        E, two_ie, H = gate_up.shape
        Ie = down.shape[2]
        gq = torch.empty((E, two_ie, H // 2), dtype=torch.uint8, device=gate_up.device)
        gs = torch.empty((E, two_ie, H // 32), dtype=torch.uint8, device=gate_up.device)
        dq = torch.empty((E, H, Ie // 2), dtype=torch.uint8, device=down.device)
        ds = torch.empty((E, H, Ie // 32), dtype=torch.uint8, device=down.device)
        quantize_mxfp4(gate_up.reshape(E * two_ie, H), gq.view(E * two_ie, H // 2), gs.view(E * two_ie, H // 32))
        quantize_mxfp4(down.reshape(E * H, Ie), dq.view(E * H, Ie // 2), ds.view(E * H, Ie // 32))
        return cls(router, gq, dq, gate_up_scale=gs, down_scale=ds, **kw)

    def desc(self):
        d = MoeExpertsDesc()
        d.format = self.format
        for n in ("router", "router_bias", "gate_up", "gate_up_scale", "gate_up_bias", "down", "down_scale", "down_bias"):
            setattr(d, n, _p(getattr(self, n)))
        d.act, d.alpha, d.limit = self.act, self.alpha, self.limit
        return d


def moe_ffn_plan_ex(rows, hidden, inter, experts, top_k, flags=0, format=0, act=MOE_ACT_SWIGLU):
    """moe_ffn_plan for experts of a format (W_F16 / W_MXFP4) under an act: the same line + " format=.. act=.."."""
    s = lib().llmie_moe_ffn_plan_ex(rows, hidden, inter, experts, top_k, flags, format, act)
    if s is None:
        raise LlmieError("moe_ffn_plan_ex: %s" % lib().llmie_last_error().decode())
    return s.decode()


def moe_route_ex(x, ex, top_k, flags=0, expert=None, weight=None):
    """moe_route under the descriptor's router and router bias"""
    import torch
    rows, H = x.shape
    if expert is None:
        expert = torch.empty((rows, top_k), dtype=torch.int32, device=x.device)
    if weight is None:
        weight = torch.empty((rows, top_k), dtype=torch.float32, device=x.device)
    d = ex.desc()
    _check(lib().llmie_moe_route_ex(_p(x), C.byref(d), rows, H, ex.router.shape[0], top_k, flags, _p(expert), _p(weight), _dt(x), _st()), "moe_route_ex")
    return expert, weight


def moe_ffn_ex(x, ex, y, top_k, resid=None, flags=0, workspace=None, rows=None, workspace_bytes=None):
    """y = MoE FFN of x (+ resid) under a MoeExperts descriptor: MXFP4 or fp16 experts, biases, clamped SwiGLU (include/llmie.h)."""
    rows = x.shape[0] if rows is None else rows
    H = x.shape[1]
    if workspace is None:
        workspace = moe_workspace(rows, H, ex.inter, ex.experts, top_k, device=x.device)
    nbytes = workspace.numel() if workspace_bytes is None else workspace_bytes
    d = ex.desc()
    _check(lib().llmie_moe_ffn_ex(_p(x), C.byref(d), _p(resid), _p(y), rows, H, ex.inter, ex.experts, top_k, flags, _p(workspace), nbytes, _dt(x),
                                  _st()), "moe_ffn_ex")
    return y


# ------------------------------------------------------------------ weight-only quantised linears
def quantize_w8(w, wq, scale):
    _check(lib().llmie_quantize_w8(_p(w), _p(wq), _p(scale), w.shape[0], w.shape[1], _st()), "quantize_w8")


def quantize_w4(w, wq, scale, group):
    _check(lib().llmie_quantize_w4(_p(w), _p(wq), _p(scale), w.shape[0], w.shape[1], group, _st()), "quantize_w4")


def linear_w8a16(x, wq, scale, y, bias=None, residual=None, workspace="auto"):
    wp, wb = _ws_args(workspace, W_INT8, x.shape[0], x.shape[1], wq.shape[0], x.device)
    _check(lib().llmie_linear_w8a16(_p(x), _p(wq), _p(scale), _p(y), x.shape[0], x.shape[1], wq.shape[0], _p(bias),
                                    _p(residual), wp, wb, _st()), "linear_w8a16")
    return y


def linear_w4a16(x, wq, scale, y, group, bias=None, residual=None, workspace="auto"):
    wp, wb = _ws_args(workspace, W_INT4, x.shape[0], x.shape[1], wq.shape[0], x.device)
    _check(lib().llmie_linear_w4a16(_p(x), _p(wq), _p(scale), _p(y), x.shape[0], x.shape[1], wq.shape[0], group,
                                    _p(bias), _p(residual), wp, wb, _st()), "linear_w4a16")
    return y


def quantize_mxfp4(w, wq, scale):
    """w fp16 [N, K], K % 32 == 0 -> wq uint8 [N, K/2] (e2m1, low nibble = even k) + scale uint8 [N, K/32] (e8m0)"""
    _check(lib().llmie_quantize_mxfp4(_p(w), _p(wq), _p(scale), w.shape[0], w.shape[1], _st()), "quantize_mxfp4")


def dequantize_mxfp4(wq, scale, w16):
    """the fp16 image of MXFP4 weights: exact for block exponents in [-23, 13]"""
    _check(lib().llmie_dequantize_mxfp4(_p(wq), _p(scale), _p(w16), w16.shape[0], w16.shape[1], _st()), "dequantize_mxfp4")
    return w16


def linear_mxfp4(x, wq, scale, y, bias=None, residual=None, workspace="auto"):
    """workspace: a device tensor of linear_workspace_bytes(W_MXFP4, M, K, N) bytes (the fp16 image of the matrix from 192 rows on),
    None (such row counts then run as passes of 64 rows), or the string auto"""
    wp, wb = _ws_args(workspace, W_MXFP4, x.shape[0], x.shape[1], wq.shape[0], x.device)
    _check(lib().llmie_linear_mxfp4(_p(x), _p(wq), _p(scale), _p(y), x.shape[0], x.shape[1], wq.shape[0], _p(bias),
                                    _p(residual), wp, wb, _st()), "linear_mxfp4")
    return y


def quantize_fp8(w, wq, scale):
    _check(lib().llmie_quantize_fp8(_p(w), _p(wq), _p(scale), w.shape[0], w.shape[1], _st()), "quantize_fp8")


KV_PAGE_TOKENS = 128


def kv_pages_copy(dense, pool, block_table, ctx_len, to_pages):
    """dense [L, batch, kvh, max_seq, hs] <-> pool [L, num_pages, kvh, 128, hs] for the first ctx_len[b] tokens of each sequence"""
    L, batch, kvh, max_seq, hs = dense.shape
    _check(lib().llmie_kv_pages_copy(_p(dense), _p(pool), _p(block_table), _p(ctx_len), 1 if to_pages else 0, L, batch, kvh,
                                     max_seq, hs, block_table.shape[1], pool.shape[1], dense.element_size(), _st()),
           "kv_pages_copy")


# ------------------------------------------------------------------ several hypotheses per request
BEAM_MAX_WIDTH = 16  # LLMIE_BEAM_MAX_WIDTH
_beam_scratch = {}
_fork_scratch = {}


def _grow(cache, device, need):
    """workspace="auto": one grow-only torch buffer per device and entry, owned by this module"""
    import torch
    buf = cache.get(device)
    if buf is None or buf.numel() < need:
        buf = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
        cache[device] = buf
    return buf


class BeamState:
    """cum [groups, width] fp32, gen_len [groups, width] int32, finished [groups, width] uint8: what llmie_beam_step updates in
    place.  The tensors can be overwritten in place -- a captured graph reads them on replay."""

    def __init__(self, cum, gen_len, finished):
        self.cum, self.gen_len, self.finished = cum, gen_len, finished


def beam_state(groups, width, device="cuda"):
    """state of `groups` requests in front of their first step: beam 0 live at log-probability 0, the others dead (-inf), so that
    the identical rows of a first step yield no duplicates"""
    import torch
    cum = torch.full((groups, width), float("-inf"), dtype=torch.float32, device=device)
    cum[:, 0] = 0.0
    return BeamState(cum, torch.zeros((groups, width), dtype=torch.int32, device=device),
                     torch.zeros((groups, width), dtype=torch.uint8, device=device))


def beam_step_workspace_bytes(groups, width, vocab):
    return lib().llmie_beam_step_workspace_bytes(groups, width, vocab)


def beam_step(logits, state, end_id, length_penalty=0.0, workspace="auto", out=None):
    """llmie_beam_step on logits [groups * width, vocab] (fp16 / fp32, read-only): updates `state` (a BeamState) in place and
    returns (parent, token), int32 [groups, width]; parent holds ABSOLUTE rows, ready for kv_pages_fork.  out: a (parent, token)
    pair to write into.  workspace: a device tensor of beam_step_workspace_bytes(groups, width, vocab) bytes, or the string auto
    (inside a graph capture pass a tensor, or make a first call outside)."""
    import torch
    groups, width = state.cum.shape
    rows, vocab = logits.shape
    if rows != groups * width:
        raise LlmieError("beam_step: %d rows of logits for %d groups of %d beams" % (rows, groups, width))
    if isinstance(workspace, str):
        workspace = _grow(_beam_scratch, logits.device, beam_step_workspace_bytes(groups, width, vocab))
    parent, token = out if out is not None else (torch.empty((groups, width), dtype=torch.int32, device=logits.device),
                                                 torch.empty((groups, width), dtype=torch.int32, device=logits.device))
    _check(lib().llmie_beam_step(_p(logits), groups, width, vocab, _p(state.cum), _p(state.gen_len), _p(state.finished), _p(parent),
                                 _p(token), end_id, length_penalty, _p(workspace),
                                 0 if workspace is None else workspace.numel() * workspace.element_size(), _dt(logits), _st()),
           "beam_step")
    return parent, token


def kv_pages_fork_workspace_bytes(rows, layers, kv_head_num, head_size, elem_bytes, max_pages):
    return lib().llmie_kv_pages_fork_workspace_bytes(rows, layers, kv_head_num, head_size, elem_bytes, max_pages)


def kv_pages_fork(k_pool, v_pool, block_table, own_table, parent, cached_len, workspace="auto"):
    """llmie_kv_pages_fork: row j continues the sequence of row parent[j] (absolute rows, e.g. beam_step's parent).  Pools
    [L, num_pages, kvh, 128, hs]; block_table / own_table int32 [rows, max_pages]; cached_len int32 [rows].  Completed pages are
    shared through the table, only the partial tail page is copied, into own_table's page.  workspace: a device tensor of
    kv_pages_fork_workspace_bytes(...) bytes, or the string auto."""
    L, num_pages, kvh, _, hs = k_pool.shape
    rows, max_pages = block_table.shape
    if isinstance(workspace, str):
        workspace = _grow(_fork_scratch, k_pool.device, kv_pages_fork_workspace_bytes(rows, L, kvh, hs, k_pool.element_size(), max_pages))
    _check(lib().llmie_kv_pages_fork(_p(k_pool), _p(v_pool), _p(block_table), _p(own_table), _p(parent), _p(cached_len), rows, L, kvh,
                                     hs, max_pages, num_pages, k_pool.element_size(), _p(workspace),
                                     0 if workspace is None else workspace.numel() * workspace.element_size(), _st()), "kv_pages_fork")


# ------------------------------------------------------------------ speculative decoding
SPEC_MAX_DRAFT = 15  # LLMIE_SPEC_MAX_DRAFT
NGRAM_MAX_N = 8
_spec_scratch = {}


class SpecState:
    """last_token, cached_len, step_rows: int32 [batch] each, what llmie_spec_verify moves in place.  The loop's invariant:
    cached_len[b] tokens of sequence b have K / V in the cache, last_token[b] is emitted but not yet cached, step_rows[b] is the
    Philox step of the next pick.  The tensors can be overwritten in place -- a captured graph reads them on replay."""

    def __init__(self, last_token, cached_len, step_rows):
        self.last_token, self.cached_len, self.step_rows = last_token, cached_len, step_rows


def spec_state(last_token, cached_len, step_rows=None, device="cuda"):
    """state behind a prefill: last_token = the first emitted token of each sequence, cached_len = its prompt length,
    step_rows = the step of its next pick (default 0).  Lists or tensors; built on the host, moved to `device`."""
    import torch
    n = len(last_token)
    if len(cached_len) != n or (step_rows is not None and len(step_rows) != n):
        raise LlmieError("spec_state: last_token, cached_len and step_rows must have one entry per sequence")
    mk = lambda v: torch.as_tensor(v, dtype=torch.int32).clone().to(device)
    return SpecState(mk(last_token), mk(cached_len), mk([0] * n if step_rows is None else step_rows))


def spec_verify_workspace_bytes(batch, k, vocab):
    return lib().llmie_spec_verify_workspace_bytes(batch, k, vocab)


def spec_verify(logits, draft_ids, params, seq_len, finished, end_id, state=None, draft_len=None, history=None, history_len=None,
                append=False, out_logprob=None, step=0, step_dev=None, workspace="auto", ext=None, out=None):
    """llmie_spec_verify on logits [batch * (k + 1), vocab] (fp16 / fp32, read-only; row b * (k + 1) + i follows input i of
    sequence b) and draft_ids int32 [batch, k]: returns (tokens int32 [batch, k + 1], count int32 [batch]) and moves seq_len,
    finished, the history and `state` (a SpecState, or None: the Philox step is *step_dev or `step` for every sequence) as
    `count` sequential sample_logits calls would.  draft_len: int32 [batch] or None (= k).  ext: sampling_ext(...) whose
    mask_index / top-N arrays have batch * (k + 1) rows.  out: a (tokens, count) pair to write into.  workspace: a device tensor
    of spec_verify_workspace_bytes(batch, k, vocab) bytes, or the string auto (inside a graph capture pass a tensor, or make a
    first call outside)."""
    import torch
    batch, k = draft_ids.shape
    rows, vocab = logits.shape
    if rows != batch * (k + 1):
        raise LlmieError("spec_verify: %d rows of logits for %d sequences of %d + 1 positions" % (rows, batch, k))
    if isinstance(workspace, str):
        workspace = _grow(_spec_scratch, logits.device, spec_verify_workspace_bytes(batch, k, vocab))
    tokens, count = out if out is not None else (torch.empty((batch, k + 1), dtype=torch.int32, device=logits.device),
                                                 torch.empty(batch, dtype=torch.int32, device=logits.device))
    stride = 0 if history is None else history.shape[1]
    st = state if state is not None else SpecState(None, None, None)
    _check(lib().llmie_spec_verify(_p(logits), batch, k, vocab, _p(draft_ids), _p(draft_len), _p(params), _p(history), stride,
                                   _p(history_len), 1 if append else 0, _p(seq_len), _p(finished), _p(tokens), _p(count), _p(out_logprob),
                                   _p(st.last_token), _p(st.cached_len), _p(st.step_rows), step, _p(step_dev), end_id, _p(workspace),
                                   0 if workspace is None else workspace.numel() * workspace.element_size(), _dt(logits), _st(),
                                   None if ext is None else _ext_ref(ext)), "spec_verify")
    return tokens, count


def spec_verify_sampled_workspace_bytes(batch, k, vocab):
    return lib().llmie_spec_verify_sampled_workspace_bytes(batch, k, vocab)


def spec_verify_sampled(logits, draft_logits, draft_ids, params, draft_params, seq_len, finished, end_id, state=None, draft_len=None,
                        history=None, history_len=None, append=False, out_logprob=None, out_accepted=None, step=0, step_dev=None,
                        workspace="auto", ext=None, out=None):
    """llmie_spec_verify_sampled: spec_verify's operands plus draft_logits [batch, k, vocab] (the logits the drafter sampled
    draft_ids from; dtype of logits) and draft_params (sampling_params(...) of the drafter, one per sequence).  Rejection
    sampling: draft i is accepted with probability min(1, p / q), a rejection emits a draw from the residual max(0, p - q).
    Returns (tokens int32 [batch, k + 1], count int32 [batch]) and moves seq_len, finished, the history and `state` by count as
    spec_verify does; out_accepted: int32 [batch] or None, the number of drafts among the emitted tokens.  ext, out, workspace
    (spec_verify_sampled_workspace_bytes(batch, k, vocab) bytes, or the string auto; inside a graph capture pass a tensor, or
    make a first call outside): as in spec_verify."""
    import torch
    batch, k = draft_ids.shape
    rows, vocab = logits.shape
    if rows != batch * (k + 1):
        raise LlmieError("spec_verify_sampled: %d rows of logits for %d sequences of %d + 1 positions" % (rows, batch, k))
    if draft_logits.numel() != batch * k * vocab or draft_logits.dtype != logits.dtype or not draft_logits.is_contiguous():
        raise LlmieError("spec_verify_sampled: draft_logits must be contiguous [%d, %d, %d] of the logits' dtype" % (batch, k, vocab))
    if isinstance(workspace, str):
        workspace = _grow(_spec_scratch, logits.device, spec_verify_sampled_workspace_bytes(batch, k, vocab))
    tokens, count = out if out is not None else (torch.empty((batch, k + 1), dtype=torch.int32, device=logits.device),
                                                 torch.empty(batch, dtype=torch.int32, device=logits.device))
    stride = 0 if history is None else history.shape[1]
    st = state if state is not None else SpecState(None, None, None)
    _check(lib().llmie_spec_verify_sampled(_p(logits), _p(draft_logits), batch, k, vocab, _p(draft_ids), _p(draft_len), _p(params),
                                           _p(draft_params), _p(history), stride, _p(history_len), 1 if append else 0, _p(seq_len),
                                           _p(finished), _p(tokens), _p(count), _p(out_accepted), _p(out_logprob), _p(st.last_token),
                                           _p(st.cached_len), _p(st.step_rows), step, _p(step_dev), end_id, _p(workspace),
                                           0 if workspace is None else workspace.numel() * workspace.element_size(), _dt(logits), _st(),
                                           None if ext is None else _ext_ref(ext)), "spec_verify_sampled")
    return tokens, count


def ngram_draft(tokens, length, k, max_n=3, min_n=1, pad_id=0, finished=None, out=None):
    """llmie_ngram_draft on tokens int32 [batch, stride] with length int32 [batch] (the sampler's history / history_len when the
    prompt was put there): returns (ids int32 [batch, k + 1] -- the verify chunk's inputs, the last token first --, draft_ids
    int32 [batch, k], draft_len int32 [batch]).  out: such a triple to write into."""
    import torch
    batch, stride = tokens.shape
    ids, draft_ids, draft_len = out if out is not None else (torch.empty((batch, k + 1), dtype=torch.int32, device=tokens.device),
                                                             torch.empty((batch, k), dtype=torch.int32, device=tokens.device),
                                                             torch.empty(batch, dtype=torch.int32, device=tokens.device))
    _check(lib().llmie_ngram_draft(_p(tokens), stride, _p(length), _p(finished), batch, k, max_n, min_n, pad_id, _p(ids), _p(draft_ids),
                                   _p(draft_len), _st()), "ngram_draft")
    return ids, draft_ids, draft_len


# ---- draft trees: several alternatives per position, verified in one forward
SPEC_TREE_MAX_NODES = 64  # LLMIE_SPEC_TREE_MAX_NODES
NGRAM_TREE_MAX_BRANCHES = 8


class SpecTreeState:
    """What one tree step passes between its launches, all [batch, n] unless noted: ids (the token of each node; node 0 = the last
    emitted token), parent, node_count [batch], depth, anc (int64: the bits of the uint64 ancestor masks), and the verify's outputs
    tokens, count [batch], path.  The tensors are written in place, so a captured step follows a new tree on replay."""

    def __init__(self, ids, parent, node_count, depth, anc, tokens, count, path):
        self.ids, self.parent, self.node_count, self.depth, self.anc = ids, parent, node_count, depth, anc
        self.tokens, self.count, self.path = tokens, count, path
        self.n = ids.shape[1]


def spec_tree_state(batch, n, device="cuda"):
    """an empty SpecTreeState for `batch` sequences of n node slots (1 <= n <= SPEC_TREE_MAX_NODES)"""
    import torch
    if not 1 <= n <= SPEC_TREE_MAX_NODES:
        raise LlmieError("spec_tree_state: n %d outside [1,%d]" % (n, SPEC_TREE_MAX_NODES))
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)
    parent = torch.full((batch, n), -1, dtype=torch.int32, device=device)
    return SpecTreeState(z(batch, n), parent, torch.ones(batch, dtype=torch.int32, device=device), z(batch, n),
                         torch.zeros((batch, n), dtype=torch.int64, device=device), z(batch, n), z(batch), z(batch, n))


def spec_tree_prepare(parent, node_count=None, out=None):
    """llmie_spec_tree_prepare on parent int32 [batch, n] (node_count int32 [batch] or None = n): returns (depth int32 [batch, n],
    anc int64 [batch, n] -- the bits of the uint64 ancestor masks; live = bit 0).  out: such a pair to write into."""
    import torch
    batch, n = parent.shape
    depth, anc = out if out is not None else (torch.empty((batch, n), dtype=torch.int32, device=parent.device),
                                              torch.empty((batch, n), dtype=torch.int64, device=parent.device))
    _check(lib().llmie_spec_tree_prepare(_p(parent), _p(node_count), batch, n, _p(depth), _p(anc), _st()), "spec_tree_prepare")
    return depth, anc


def spec_verify_tree_workspace_bytes(batch, n, vocab):
    return lib().llmie_spec_verify_tree_workspace_bytes(batch, n, vocab)


def spec_verify_tree(logits, node_ids, parent, depth, anc, params, seq_len, finished, end_id, state=None, history=None, history_len=None,
                     append=False, out_logprob=None, step=0, step_dev=None, workspace="auto", ext=None, out=None):
    """llmie_spec_verify_tree on logits [batch * n, vocab] (row b * n + i follows node i of sequence b), node_ids / parent int32
    [batch, n] and depth / anc as spec_tree_prepare left them: returns (tokens int32 [batch, n], count int32 [batch], path int32
    [batch, n] -- the node of every emitted token, -1 behind count) and moves seq_len, finished, the history and `state` (a
    SpecState) as spec_verify does.  ext: sampling_ext(...) with batch * n rows.  out: a (tokens, count, path) triple to write
    into.  workspace: spec_verify_tree_workspace_bytes(batch, n, vocab) bytes, or the string auto (as in spec_verify)."""
    import torch
    batch, n = node_ids.shape
    rows, vocab = logits.shape
    if rows != batch * n:
        raise LlmieError("spec_verify_tree: %d rows of logits for %d sequences of %d nodes" % (rows, batch, n))
    if isinstance(workspace, str):
        workspace = _grow(_spec_scratch, logits.device, spec_verify_tree_workspace_bytes(batch, n, vocab))
    tokens, count, path = out if out is not None else (torch.empty((batch, n), dtype=torch.int32, device=logits.device),
                                                       torch.empty(batch, dtype=torch.int32, device=logits.device),
                                                       torch.empty((batch, n), dtype=torch.int32, device=logits.device))
    stride = 0 if history is None else history.shape[1]
    st = state if state is not None else SpecState(None, None, None)
    _check(lib().llmie_spec_verify_tree(_p(logits), batch, n, vocab, _p(node_ids), _p(parent), _p(depth), _p(anc), _p(params), _p(history),
                                        stride, _p(history_len), 1 if append else 0, _p(seq_len), _p(finished), _p(tokens), _p(count),
                                        _p(path), _p(out_logprob), _p(st.last_token), _p(st.cached_len), _p(st.step_rows), step,
                                        _p(step_dev), end_id, _p(workspace),
                                        0 if workspace is None else workspace.numel() * workspace.element_size(), _dt(logits), _st(),
                                        None if ext is None else _ext_ref(ext)), "spec_verify_tree")
    return tokens, count, path


def kv_tree_commit(k_cache, v_cache, base_len, path, count, block_table=None):
    """llmie_kv_tree_commit: moves the K / V rows of the accepted path into place -- node path[b, m] from slot base_len[b] +
    path[b, m] to base_len[b] + m, every layer and kv head.  Dense caches [L, batch, kvh, max_seq, hs] (block_table None) or pools
    [L, num_pages, kvh, 128, hs] with block_table int32 [batch, max_pages]; fp16 or e4m3 bytes.  base_len: the history_lengths
    the forward ran with -- NOT the array spec_verify_tree advanced."""
    batch, n = path.shape
    L, d1, kvh, d3, hs = k_cache.shape
    if block_table is None:
        max_seq, max_pages, num_pages = d3, 0, 0
    else:
        max_seq, max_pages, num_pages = 0, block_table.shape[1], d1
    _check(lib().llmie_kv_tree_commit(_p(k_cache), _p(v_cache), _p(block_table), _p(base_len), _p(path), _p(count), batch, n, L, kvh,
                                      max_seq, hs, max_pages, num_pages, k_cache.element_size(), _st()), "kv_tree_commit")


def ngram_draft_tree(tokens, length, n, k, branches=4, max_n=3, min_n=1, pad_id=0, finished=None, out=None):
    """llmie_ngram_draft_tree on tokens int32 [batch, stride] with length int32 [batch]: up to `branches` prompt-lookup
    continuations of up to k tokens each (one per matching suffix length, longest first) merged into a trie of at most n nodes.
    Returns (ids int32 [batch, n] -- node 0 the last token, unused slots pad_id --, parent int32 [batch, n] -- -1 for node 0 and
    unused slots --, node_count int32 [batch]).  out: such a triple to write into."""
    import torch
    batch, stride = tokens.shape
    ids, parent, node_count = out if out is not None else (torch.empty((batch, n), dtype=torch.int32, device=tokens.device),
                                                           torch.empty((batch, n), dtype=torch.int32, device=tokens.device),
                                                           torch.empty(batch, dtype=torch.int32, device=tokens.device))
    _check(lib().llmie_ngram_draft_tree(_p(tokens), stride, _p(length), _p(finished), batch, n, k, branches, max_n, min_n, pad_id,
                                        _p(ids), _p(parent), _p(node_count), _st()), "ngram_draft_tree")
    return ids, parent, node_count


def linear_fp8_workspace_bytes(M, K, N=0):
    """N = 0: the activation part only (linear_fp8_swiglu, prefill-sized linear_fp8)"""
    return lib().llmie_linear_fp8_workspace_bytes(M, K, N)


def linear_fp8_swiglu(x, wq, wscale, y, workspace):
    _check(lib().llmie_linear_fp8_swiglu(_p(x), _p(wq), _p(wscale), _p(y), x.shape[0], x.shape[1], wq.shape[0], _p(workspace),
                                         workspace.numel() * workspace.element_size(), _st()), "linear_fp8_swiglu")
    return y


def linear_fp8(x, wq, wscale, y, workspace, bias=None, residual=None):
    _check(lib().llmie_linear_fp8(_p(x), _p(wq), _p(wscale), _p(y), x.shape[0], x.shape[1], wq.shape[0], _p(bias),
                                  _p(residual), _p(workspace), workspace.numel() * workspace.element_size(), _st()),
           "linear_fp8")
    return y


# ---- tile-packed weight images + batch-decode linear on them (include/llmie.h section 2) ----
def pack_weight(fmt, w, scale=None, swiglu_pairs=False):
    """row-major weights (fmt's storage, [N, K] logical) -> (packed image uint8 tensor, packed int4 group scales or None)"""
    import torch
    N = w.shape[0]
    K = w.shape[1] * (2 if fmt == W_INT4 else 1)
    nbytes = lib().llmie_packed_weight_bytes(fmt, N, K, int(swiglu_pairs))
    if nbytes == 0:
        raise LlmieError("pack_weight: shape N=%d K=%d not packable in format %d" % (N, K, fmt))
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    sbytes = lib().llmie_packed_scale_bytes(fmt, N, K, int(swiglu_pairs))
    pscale = torch.empty(sbytes, dtype=torch.uint8, device=w.device) if sbytes else None
    _check(lib().llmie_pack_weight(fmt, _p(w), _p(scale), _p(packed), _p(pscale), N, K, int(swiglu_pairs), _st()), "pack_weight")
    return packed, pscale


X32_X, X32_Y, X32_RES = 1, 2, 4


def linear_packed(fmt, x, packed, scale, y, N, swiglu=False, residual=None, gamma=None, pre_bias=None, eps=0.0, M=None, K=None,
                  x32_flags=0):
    """y = [swiglu](rmsnorm(x + pre_bias) * gamma . W^T) (+ residual) on a packed image; scale = per-row (int8 / fp8) or the
    packed group scales (int4).  x32_flags: operands in the x32 activation layout (pass M, K explicitly for an x32 x)"""
    import torch
    if M is None:
        M, K = x.shape
    ws_bytes = lib().llmie_linear_packed_workspace_bytes(fmt, M, K, N)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    _check(lib().llmie_linear_packed(fmt, _p(x), _p(packed), _p(scale), _p(y), M, K, N, int(swiglu), int(x32_flags), _p(residual),
                                     _p(gamma), _p(pre_bias), float(eps), _p(ws), ws_bytes, _st()), "linear_packed")
    return y


def x32_convert(src, dst, M, C, to_x32):
    """row-major [M, C] fp16 <-> x32 image (llmie_x32_bytes(C) bytes)"""
    _check(lib().llmie_x32_convert(_p(src), _p(dst), M, C, int(to_x32), _st()), "x32_convert")
    return dst
