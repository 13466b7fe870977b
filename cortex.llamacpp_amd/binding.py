"""ctypes binding of include/mi355_llama.h (same names, same argument meaning)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .gguf_synth import (BF16, F16, F32, IQ4_NL, IQ4_XS, MXFP4, Q2_K, Q3_K, Q4_0, Q4_1, Q4_K, Q5_0, Q5_1, Q5_K, Q6_K, Q8_0, Q8_K,  # noqa: F401  (the ggml type ids)
                         TQ1_0, TQ2_0)

HERE = os.path.dirname(os.path.abspath(__file__))


class MI355Error(RuntimeError):
    pass


def lib_path() -> str:
    # MI355_LLAMA_LIB: an alternative build of the same library (tools/ experiments)
    return os.environ.get("MI355_LLAMA_LIB") or os.path.join(HERE, "lib", "libmi355_llama.so")


class ModelParams(C.Structure):
    _fields_ = [("n_gpu_layers", C.c_int32), ("main_gpu", C.c_int32), ("use_mmap", C.c_int32), ("use_mlock", C.c_int32),
                ("tp_rank", C.c_int32), ("tp_size", C.c_int32), ("prefill_planes", C.c_int32)]


class ContextParams(C.Structure):
    _fields_ = [("n_ctx", C.c_uint32), ("n_batch", C.c_uint32), ("n_ubatch", C.c_uint32), ("n_seq_max", C.c_uint32),
                ("type_k", C.c_int32), ("type_v", C.c_int32), ("flash_attn", C.c_int32), ("embeddings", C.c_int32),
                ("use_graphs", C.c_int32), ("logits_to_host", C.c_int32)]


class Batch(C.Structure):
    _fields_ = [("n_tokens", C.c_int32), ("token", C.POINTER(C.c_int32)), ("embd", C.POINTER(C.c_float)),
                ("pos", C.POINTER(C.c_int32)), ("n_seq_id", C.POINTER(C.c_int32)),
                ("seq_id", C.POINTER(C.POINTER(C.c_int32))), ("logits", C.POINTER(C.c_int8))]


class PplStats(C.Structure):           # mi355_ppl_stats
    _fields_ = [("n_chunks", C.c_int64), ("count", C.c_int64), ("top1", C.c_int64), ("dead", C.c_int64), ("same_top", C.c_int64),
                ("has_base", C.c_int32), ("stopped", C.c_int32),
                ("nll", C.c_double), ("nll2", C.c_double), ("nll_base", C.c_double), ("nll2_base", C.c_double), ("kl", C.c_double), ("kl2", C.c_double)]


PPL_CALLBACK = C.CFUNCTYPE(C.c_int32, C.POINTER(PplStats), C.c_void_p)


# every symbol include/mi355_llama.h declares: name -> (restype, argtypes)
_vp, _i32, _i64, _u32, _u64, _f32, _sz, _cp = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_size_t, C.c_char_p
ENGINE_CB = C.CFUNCTYPE(None, C.c_char_p, C.c_char_p, C.c_void_p)
SYMBOLS = {
    "mi355_backend_init": (C.c_int, []),
    "mi355_backend_free": (None, []),
    "mi355_device_count": (C.c_int, []),
    "mi355_last_error": (_cp, []),
    "mi355_time_us": (_i64, []),
    "mi355_print_system_info": (_cp, []),
    "mi355_model_default_params": (ModelParams, []),
    "mi355_model_load_from_file": (_vp, [_cp, ModelParams]),
    "mi355_model_free": (None, [_vp]),
    "mi355_model_n_vocab": (_i32, [_vp]),
    "mi355_model_n_embd": (_i32, [_vp]),
    "mi355_model_n_layer": (_i32, [_vp]),
    "mi355_model_n_head": (_i32, [_vp]),
    "mi355_model_n_head_kv": (_i32, [_vp]),
    "mi355_model_n_ctx_train": (_i32, [_vp]),
    "mi355_model_size": (_u64, [_vp]),
    "mi355_model_cpu_buffer": (_u64, [_vp]),
    "mi355_model_other_buffer": (_u64, [_vp]),
    "mi355_model_bytes_per_token": (_u64, [_vp]),
    "mi355_model_planes_bytes": (_u64, [_vp]),
    "mi355_debug_set_option": (C.c_int, [_cp, _i32]),
    "mi355_model_desc": (_cp, [_vp]),
    "mi355_model_meta_str": (C.c_int, [_vp, _cp, _cp, _sz]),
    "mi355_context_default_params": (ContextParams, []),
    "mi355_context_new": (_vp, [_vp, ContextParams]),
    "mi355_context_free": (None, [_vp]),
    "mi355_n_ctx": (_u32, [_vp]),
    "mi355_n_batch": (_u32, [_vp]),
    "mi355_n_ubatch": (_u32, [_vp]),
    "mi355_context_device_bytes": (_u64, [_vp]),
    "mi355_batch_init": (Batch, [_i32, _i32, _i32]),
    "mi355_batch_free": (None, [Batch]),
    "mi355_decode": (_i32, [_vp, Batch]),
    "mi355_greedy_steps": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp]),
    "mi355_get_logits_ith": (C.POINTER(C.c_float), [_vp, _i32]),
    "mi355_get_argmax_ith": (_i32, [_vp, _i32]),
    "mi355_get_argmax_prob_ith": (_i32, [_vp, _i32, _vp]),
    "mi355_spec_verify": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp]),
    "mi355_get_token_logprobs": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp]),
    "mi355_logits_kl": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "mi355_perplexity": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mi355_imatrix_begin": (_i32, [_vp, _i32]),
    "mi355_imatrix_end": (_i32, [_vp]),
    "mi355_imatrix_clear": (_i32, [_vp]),
    "mi355_imatrix_n_entries": (_i32, [_vp]),
    "mi355_imatrix_entry": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp]),
    "mi355_imatrix_get": (_i32, [_vp, _i32, _vp, _vp]),
    "mi355_speculative_steps": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp]),
    "mi355_get_topk_ith": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _f32, _f32, _f32, _vp, _vp]),
    "mi355_debug_mega_steps": (C.c_int64, [_vp]),
    "mi355_debug_engine_steps": (C.c_int64, [_vp]),
    "mi355_debug_fused_skipped_steps": (C.c_int64, [_vp]),
    "mi355_debug_qkv_attn_launches": (C.c_int64, [_vp]),
    "mi355_debug_qkv_attn_plan": (C.c_int64, [C.c_int32] * 10 + [C.POINTER(C.c_int32)]),
    "mi355_set_embeddings": (None, [_vp, _i32]),
    "mi355_get_embeddings_ith": (C.POINTER(C.c_float), [_vp, _i32]),
    "mi355_synchronize": (None, [_vp]),
    "mi355_adapter_lora_init": (_vp, [_vp, _cp]),
    "mi355_adapter_lora_free": (None, [_vp]),
    "mi355_adapter_lora_alpha": (_f32, [_vp]),
    "mi355_adapter_lora_n_pairs": (_i32, [_vp]),
    "mi355_set_adapter_lora": (_i32, [_vp, _vp, _f32]),
    "mi355_rm_adapter_lora": (_i32, [_vp, _vp]),
    "mi355_clear_adapter_lora": (None, [_vp]),
    "mi355_apply_adapter_cvec": (_i32, [_vp, _vp, _sz, _i32, _i32, _i32]),
    "mi355_control_vector_load": (_i64, [_vp, _vp, _i32, _vp, _sz, _vp]),
    "mi355_cvec_direction": (C.c_int, [_i32, _vp, _i64, _i32, _vp, _i32, _i32, _f32, _vp, _vp, _vp]),
    "mi355_op_add_row_vec": (C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    "mi355_op_lora_delta": (C.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "mi355_kv_cache_clear": (None, [_vp]),
    "mi355_kv_cache_seq_rm": (_i32, [_vp, _i32, _i32, _i32]),
    "mi355_kv_cache_seq_cp": (None, [_vp, _i32, _i32, _i32, _i32]),
    "mi355_kv_cache_seq_add": (None, [_vp, _i32, _i32, _i32, _i32]),
    "mi355_state_seq_get_size": (_sz, [_vp, _i32]),
    "mi355_state_seq_get_data": (_sz, [_vp, _vp, _sz, _i32]),
    "mi355_state_seq_set_data": (_sz, [_vp, _vp, _sz, _i32]),
    "mi355_state_seq_save_file": (_sz, [_vp, _cp, _i32, _vp, _sz]),
    "mi355_state_seq_load_file": (_sz, [_vp, _cp, _i32, _vp, _sz, C.POINTER(C.c_size_t)]),
    "mi355_debug_state_seq_timing": (None, [_vp, _vp]),
    "mi355_kv_cache_used_cells": (_i32, [_vp]),
    "mi355_debug_enable_taps": (None, [_vp, _i32]),
    "mi355_debug_layer_out": (_i32, [_vp, _i32, _vp, _sz]),
    "mi355_op_quantize_act": (C.c_int, [_i32, _vp, _i64, _i64, _vp]),
    "mi355_op_rms_norm_quant": (C.c_int, [_vp, _vp, _i64, _i64, _f32, _vp, _vp]),
    "mi355_op_swiglu_quant": (C.c_int, [_vp, _vp, _i64, _i64, _vp]),
    "mi355_op_mul_mat": (C.c_int, [_i32, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "mi355_op_mul_mat_add": (C.c_int, [_i32, _vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    "mi355_op_mul_mat_fused": (C.c_int, [_i32, _vp, _i64, _i64, _vp, _vp, _f32, _vp]),
    "mi355_op_mat_vec_step": (C.c_int, [_i32, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _i32, _vp, _f32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp]),
    "mi355_op_prompt_mul_mat": (C.c_int, [_i32, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _f32, _i32, _i64, _vp, _vp]),
    "mi355_op_act_q8k_planes": (C.c_int, [_i32, _vp, _vp, _vp, _f32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi355_op_f32_to_bf16": (C.c_int, [_vp, _i64, _vp]),
    "mi355_op_mul_mat_bf16": (C.c_int, [_i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "mi355_op_ffn_gate_up": (C.c_int, [_i32, _vp, _vp, _i64, _i64, _vp, _i64, _vp]),
    "mi355_op_rms_norm_mul": (C.c_int, [_vp, _vp, _i64, _i64, _f32, _vp]),
    "mi355_op_rope": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _i64, _f32, _f32, _vp, _i32]),
    "mi355_op_rope_yarn": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _i64, _f32, _f32, _vp, _i32, _f32, _f32, _f32, _f32]),
    "mi355_op_get_rows": (C.c_int, [_i32, _vp, _i64, _i64, _vp, _i64, _vp]),
    "mi355_op_repack_rows": (C.c_int, [_i32, _vp, _i64, _i64, _vp]),
    "mi355_op_swiglu": (C.c_int, [_vp, _vp, _i64, _vp]),
    "mi355_op_soft_max": (C.c_int, [_vp, _vp, _i64, _i64, _f32, _vp]),
    "mi355_op_moe_route": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "mi355_op_moe_router": (C.c_int, [_i32, _vp, _i32, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mi355_op_argmax_rows": (C.c_int, [_vp, _i64, _vp, _i32, _i32, _vp]),
    "mi355_op_argmax_prob_rows": (C.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "mi355_op_spec_verify": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "mi355_op_token_logprob_rows": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp]),
    "mi355_op_logits_kl_rows": (C.c_int, [_vp, _i32, _vp, _i32, _i64, _vp, _vp, _i32, _vp, _vp]),
    "mi355_op_imatrix_accum": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _vp, _i32, _vp, _i32, _vp, _vp]),
    "mi355_quantize_chunk": (C.c_int, [_i32, _i32, _vp, _i64, _i64, _vp, _vp]),
    "mi355_quantize_supported": (C.c_int, [_i32]),
    "mi355_quantize_last_times": (C.c_int, [_vp, _vp, _vp]),
    "mi355_op_clip_attn": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mi355_op_mul_mat_f16_xh": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _f32, _i32, _vp, _i32, _i32, _vp]),
    "mi355_op_layer_norm": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _f32, _i32, _vp, _vp]),
    "mi355_op_clip_gelu": (C.c_int, [_vp, _i64, _i32, _vp, _vp]),
    "mi355_op_clip_im2col": (C.c_int, [_vp, _i32, _i32, _i32, _vp]),
    "mi355_op_clip_embed": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "mi355_op_clip_bias": (C.c_int, [_vp, _vp, _i32, _i32, _f32, _i32]),
    "mi355_op_f32_to_f16": (C.c_int, [_vp, _i64, _vp]),
    "mi355_op_add_qkv_bias": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32]),
    "mi355_op_topk_rows": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi355_op_moe_group": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "mi355_op_moe_gather_act": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "mi355_op_moe_combine": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "mi355_op_moe_mul_mat_grouped": (C.c_int, [_i32, _i32, _vp, _vp, _i32, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "mi355_op_gather_rows_f32": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _vp]),
    "mi355_op_flash_attn": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _f32, _vp]),
    "mi355_op_attn_step": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _f32, _i32, _f32, _i32, _vp, _i64, _vp, _i32,
                                     _vp, _vp, _vp, _vp]),
    "mi355_op_attn_decode_neox": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _f32, _f32, _vp, _vp, _f32, _i32,
                                            _vp, _vp, _vp]),
    "mi355_op_flash_attn_seq": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _f32, _vp]),
    "mi355_op_flash_attn_plan": (C.c_int, [_i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "mi355_op_attn_step_seq": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _i32, _f32, _i32, _vp,
                                         _i64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "mi355_op_attn_decode_neox_seq": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp,
                                                _f32, _i32, _vp, _vp, _vp]),
    "mi355_op_attn_batch_step": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _f32, _i32, _i32, _f32,
                                           _i32, _vp, _vp]),
    "mi355_op_attn_batch_step_planes": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _f32, _i32, _i32, _f32,
                                           _i32, _vp, _vp, _vp, _vp]),
    "mi355_op_kv_store": (C.c_int, [_i32, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _f32, _vp, _vp]),
    "mi355_op_k_shift": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _vp, _f32, _f32, _vp, _f32, _f32, _f32, _f32, _vp]),
    "mi355_op_kv_state_pack": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "mi355_op_kv_state_unpack": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "mi355_bench_hbm_read": (C.c_double, [_sz, C.c_int]),
    "mi355_profile_last_decode": (_i32, [_vp, C.POINTER(_cp), C.POINTER(_f32), _i32]),
    "mi355_profile_enable": (None, [_vp, _i32]),
    "mi355_debug_force_moe_ids": (C.c_int, [_vp, _vp, _i32, _i32, _i32]),
    "mi355_bench_weight_sweep": (C.c_double, [_vp, C.c_int, C.POINTER(_u64)]),
    "mi355_bench_weight_sweep2": (C.c_double, [_vp, C.c_int, C.POINTER(_u64), C.POINTER(C.c_int32)]),
    "mi355_tokenize": (_i32, [_vp, _cp, _i32, C.POINTER(C.c_int32), _i32, _i32, _i32]),
    "mi355_token_to_piece": (_i32, [_vp, _i32, C.c_char_p, _i32, _i32]),
    "mi355_token_bos": (_i32, [_vp]),
    "mi355_token_eos": (_i32, [_vp]),
    "mi355_token_is_eog": (_i32, [_vp, _i32]),
    "mi355_engine_create": (_vp, []),
    "mi355_engine_destroy": (None, [_vp]),
    "mi355_engine_set_release_callback": (None, [_vp, _vp]),
    "mi355_engine_load_model": (None, [_vp, _cp, ENGINE_CB, _vp]),
    "mi355_engine_unload_model": (None, [_vp, _cp, ENGINE_CB, _vp]),
    "mi355_engine_get_model_status": (None, [_vp, _cp, ENGINE_CB, _vp]),
    "mi355_engine_get_models": (None, [_vp, _cp, ENGINE_CB, _vp]),
    "mi355_engine_handle_chat_completion": (None, [_vp, _cp, ENGINE_CB, _vp]),
    "mi355_engine_handle_embedding": (None, [_vp, _cp, ENGINE_CB, _vp]),
    "mi355_engine_is_supported": (_i32, [_vp, _cp]),
    "mi355_engine_stop_inferencing": (None, [_vp, _cp]),
    "mi355_engine_prompt_cache_stats": (C.c_int, [_vp, _cp, _vp]),
    "mi355_engine_spec_stats": (C.c_int, [_vp, _cp, _vp]),
    "mi355_engine_load": (None, [_vp, _cp, _cp, _i32, _cp, _i32, _i32]),
    "mi355_engine_unload": (None, [_vp]),
    "mi355_engine_set_file_logger": (None, [_vp, _i32, _cp]),
    "mi355_engine_set_log_level": (None, [_vp, _i32]),
    "mi355_engine_set_log_callback": (None, [_vp, _vp, _vp]),
    "mi355_clip_model_load": (_vp, [_cp, _i32]),
    "mi355_clip_free": (None, [_vp]),
    "mi355_clip_n_mmproj_embd": (_i32, [_vp]),
    "mi355_clip_n_patches": (_i32, [_vp]),
    "mi355_clip_image_size": (_i32, [_vp]),
    "mi355_clip_max_image_rows": (_i32, [_vp]),
    "mi355_clip_image_preprocess_grid": (_i32, [_vp, _vp, _i32, _i32, _vp, _sz, _vp, _vp]),
    "mi355_clip_image_load_from_bytes": (_i32, [_vp, _sz, C.POINTER(_i32), C.POINTER(_i32), _vp, _sz]),
    "mi355_clip_image_preprocess": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "mi355_clip_image_encode": (_i32, [_vp, _vp, _vp]),
    "mi355_llava_image_embed_from_bytes": (_i32, [_vp, _vp, _sz, _vp, _sz]),
    "mi355_tp_p2p_local_handle": (C.c_int, [_vp, _sz, _sz]),
    "mi355_tp_p2p_local_handle2": (C.c_int, [_vp, _sz, _sz, _sz]),
    "mi355_tp_p2p_prompt_exchanges": (C.c_int64, []),
    "mi355_tp_p2p_enable": (C.c_int, [_vp, _sz]),
    "mi355_tp_p2p_exchanges": (C.c_int64, []),
    "mi355_tp_unique_id": (C.c_int, [_vp, _sz]),
    "mi355_tp_init": (C.c_int, [_i32, _i32, _i32, _vp, _sz]),
    "mi355_tp_shutdown": (None, []),
    "mi355_tp_worker_main": (C.c_int, [C.c_int]),
    "mi355_tp_rank": (_i32, []),
    "mi355_tp_size": (_i32, []),
    "mi355_tp_set_host_exchange": (C.c_int, [_vp, _vp, _i32, _i32]),
}
TP_HOST_EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_int32)
TP_ID_BYTES = 128

_lib = None


def load_library(path: str | None = None):
    """dlopen the native library and type every exported entry point.  Raises if it is missing:
    there is no Python / CPU fallback for the compute path."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or lib_path()
    if not os.path.exists(p):
        raise MI355Error(f"{p} not found: build it with `python cortex.llamacpp_amd/build.py` (hipcc, gfx950)")
    lib = C.CDLL(p)
    for name, (res, args) in SYMBOLS.items():
        if name.startswith("mi355_debug_") and os.environ.get("MI355_LLAMA_LIB") and not hasattr(lib, name):
            continue                     # (tools/ab_libs.sh: an older build of the library under MI355_LLAMA_LIB may lack a diagnosis getter)
        fn = getattr(lib, name)          # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _err(lib) -> str:
    return (lib.mi355_last_error() or b"").decode("utf-8", "replace")


def control_vector_load(lib, items):
    """mi355_control_vector_load on a loaded library (host arithmetic, no device): items = [(path, scale), ...] -> (data f32, n_embd)."""
    items = [(it, 1.0) if isinstance(it, (str, os.PathLike)) else it for it in items]
    n = len(items)
    paths = (C.c_char_p * max(n, 1))(*[os.fspath(p).encode() for p, _ in items])
    scales = np.array([s for _, s in items] or [0.0], np.float32)
    ne = C.c_int32(0)
    need = int(lib.mi355_control_vector_load(C.cast(paths, C.c_void_p), _ptr(scales), n, None, 0, C.cast(C.byref(ne), C.c_void_p)))
    if need < 0:
        raise MI355Error(f"mi355_control_vector_load failed ({need}): {_err(lib)}")
    out = np.zeros(need, np.float32)
    got = int(lib.mi355_control_vector_load(C.cast(paths, C.c_void_p), _ptr(scales), n, _ptr(out), need, None))
    if got != need:
        raise MI355Error(f"mi355_control_vector_load failed ({got}): {_err(lib)}")
    return out, int(ne.value)


class Backend:
    """mi355_backend_init / per-op entry points."""

    def __init__(self):
        self.lib = load_library()
        rc = self.lib.mi355_backend_init()
        if rc != 0:
            raise MI355Error(f"mi355_backend_init failed ({rc}): {_err(self.lib)}")

    def _chk(self, rc, what):
        if rc != 0:
            raise MI355Error(f"{what} failed ({rc}): {_err(self.lib)}")

    def set_option(self, name: str, value: int) -> None:
        self._chk(self.lib.mi355_debug_set_option(name.encode(), int(value)), f"set_option({name})")

    def system_info(self) -> str:
        return self.lib.mi355_print_system_info().decode()

    def quantize_act(self, act_type: int, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        rows, n = (1, x.size) if x.ndim == 1 else x.shape
        bb = 292 * (n // 256) if act_type == Q8_K else 34 * (n // 32)
        out = np.zeros(rows * bb, np.uint8)
        self._chk(self.lib.mi355_op_quantize_act(act_type, _ptr(x), n, rows, _ptr(out)), "op_quantize_act")
        return out.reshape(rows, bb)

    def rms_norm_quant(self, x: np.ndarray, w: np.ndarray, eps: float):
        """(Q8_0 blocks [T][34 n / 32], y_f32 [T][n]) of RMSNorm(x) * w: the fused norm + quantise launch (see mi355_op_rms_norm_quant)."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        T, n = (1, x.size) if x.ndim == 1 else x.shape
        out = np.zeros((T, 34 * (n // 32)), np.uint8)
        y = np.zeros((T, n), np.float32)
        self._chk(self.lib.mi355_op_rms_norm_quant(_ptr(x), _ptr(w), n, T, eps, _ptr(y), _ptr(out)), "op_rms_norm_quant")
        return out, y

    def swiglu_quant(self, gate: np.ndarray, up: np.ndarray) -> np.ndarray:
        """Q8_0 blocks [T][34 n / 32] of silu(gate) * up (see mi355_op_swiglu_quant)."""
        gate = np.ascontiguousarray(gate, np.float32)
        up = np.ascontiguousarray(up, np.float32)
        T, n = (1, gate.size) if gate.ndim == 1 else gate.shape
        out = np.zeros((T, 34 * (n // 32)), np.uint8)
        self._chk(self.lib.mi355_op_swiglu_quant(_ptr(gate), _ptr(up), n, T, _ptr(out)), "op_swiglu_quant")
        return out

    def mul_mat_fused(self, t: int, W: np.ndarray, N: int, K: int, x: np.ndarray, norm_w=None, eps: float = 0.0) -> np.ndarray:
        """One token's W . act with the activation quantised in the launch's prologue (see mi355_op_mul_mat_fused)."""
        W = np.ascontiguousarray(W.view(np.uint8).reshape(-1))
        x = np.ascontiguousarray(x, np.float32).reshape(K)
        nw = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32).reshape(K)
        y = np.zeros(N, np.float32)
        self._chk(self.lib.mi355_op_mul_mat_fused(t, _ptr(W), N, K, _ptr(x), _ptr(nw), eps, _ptr(y)), "op_mul_mat_fused")
        return y

    MAT_VEC_KERNELS = ("base", "ring", "stream", "tiled")
    MAT_VEC_ROLES = ("stream", "qkv", "gate_up", "ffn_down", "head")

    def mat_vec_step(self, types, Ws, Ns, K: int, x: np.ndarray, epi: int = 0, resid=None, fuse: int = 0, norm_w=None, eps: float = 0.0,
                     want_host_copy: bool = False, expert_ids=None, n_expert: int = 1, ld_pad: int = 0):
        """One mat-vec launch of a decode step as the model issues it (see mi355_op_mat_vec_step).  Returns (ys, y_host, path): ys the whole out buffers
        [rows][N + ld_pad] (one for epi 2), y_host the pinned second copy or None, path one dict per launch issued: tokens, kernel, and for the weight
        stream role (moe / ternary launches: "moe" / "ternary"), kb, fast_ok, down_early."""
        n = len(Ws)
        Ws = [np.ascontiguousarray(w.view(np.uint8).reshape(-1)) for w in Ws]
        tarr = np.asarray(types, np.int32)
        Narr = np.asarray(Ns, np.int64)
        x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
        n_sel = 0 if expert_ids is None else len(expert_ids)
        ids = None if expert_ids is None else np.ascontiguousarray(expert_ids, np.int32)
        T = 1 if n_sel else x.shape[0]
        R = n_sel if n_sel else T
        ys = [np.zeros((R, int(N) + ld_pad), np.float32) for N in (Narr[:1] if epi == 2 else Narr)]
        r = None if resid is None else np.ascontiguousarray(resid, np.float32).reshape(R, int(Narr[0]) + ld_pad)
        nw = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32).reshape(K)
        yh = np.zeros(int(Narr[0]), np.float32) if want_host_copy else None
        path = np.zeros(40, np.int32)
        parr = lambda xs: (C.c_void_p * len(xs))(*[None if a is None else a.ctypes.data for a in xs])
        wp, yp = parr(Ws), parr(ys + [None] * (n - len(ys)))
        self._chk(self.lib.mi355_op_mat_vec_step(n, _ptr(tarr), wp, _ptr(Narr), K, _ptr(x), T, epi, _ptr(r), fuse, _ptr(nw), eps, int(want_host_copy), n_sel,
                                                 n_expert, _ptr(ids), ld_pad, yp, _ptr(yh), _ptr(path)), "op_mat_vec_step")
        launches = []
        for p in path.reshape(5, 8):
            if p[0] == 0:
                break
            d = {"T": int(p[0]), "kernel": self.MAT_VEC_KERNELS[p[1]]}
            if p[1] == 2:
                d.update(role="ternary" if p[7] else "moe" if p[6] else self.MAT_VEC_ROLES[p[2]], kb=int(p[3]), fast_ok=bool(p[4]), down_early=bool(p[5]))
            launches.append(d)
        return ys, yh, launches

    def prompt_mul_mat(self, types, Ws, Ns, K: int, x: np.ndarray, epi: int = 0, resid=None, in_place: bool = False, prologue: int = 0, norm_w=None,
                       eps: float = 0.0, form: int = 0, ld_pad: int = 0, check: bool = True):
        """One mat-mul launch of a dense prompt batch as the model issues it (see mi355_op_prompt_mul_mat).  x: [T][K], for prologue 2 [2][T][K] (gate, up).
        Returns (ys, path, rc): ys the whole out buffers [T][N + ld_pad] (one for epi 2), path a dict (kernel 1 K-split / 2 planes 256 x 32 / 3 planes
        128 x 128 / 4 LDS / 5 on the fly, token_tiles, n_split, mixed, swiglu, prep), rc the entry's return code (check=False: returned, not raised)."""
        n = len(Ws)
        Ws = [np.ascontiguousarray(w.view(np.uint8).reshape(-1)) for w in Ws]
        tarr = np.asarray(types, np.int32)
        Narr = np.asarray(Ns, np.int64)
        x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
        T = x.shape[0] // 2 if prologue == 2 else x.shape[0]
        ys = [np.zeros((T, int(N) + ld_pad), np.float32) for N in (Narr[:1] if epi == 2 else Narr)]
        r = None if resid is None else np.ascontiguousarray(resid, np.float32).reshape(T, int(Narr[0]) + ld_pad)
        nw = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32).reshape(K)
        path = np.zeros(8, np.int32)
        parr = lambda xs: (C.c_void_p * len(xs))(*[None if a is None else a.ctypes.data for a in xs])
        wp, yp = parr(Ws), parr(ys + [None] * (n - len(ys)))
        rc = self.lib.mi355_op_prompt_mul_mat(n, _ptr(tarr), wp, _ptr(Narr), K, _ptr(x), T, epi, _ptr(r), int(bool(in_place)), prologue, _ptr(nw), eps, form, ld_pad,
                                              yp, _ptr(path))
        if check:
            self._chk(rc, "op_prompt_mul_mat")
        keys = ("kernel", "token_tiles", "n_split", "mixed", "swiglu", "prep")
        return ys, {k: int(v) for k, v in zip(keys, path)}, int(rc)

    def act_q8k_planes(self, producer: int, x: np.ndarray, x2=None, norm_w=None, eps: float = 0.0, want_f32: bool = False):
        """One producer of the MFMA kernels' activation (mi355_op_act_q8k_planes; 0 launch_quantize, 1 launch_rmsnorm_quant, 2 launch_swiglu_quant) over the
        rows x [T][n].  Returns (blocks [T][292 * n / 256] uint8, bh, bl, prep_bh, prep_bl [T][n / 16] int8, f32 rows or None)."""
        x = np.ascontiguousarray(x, np.float32)
        T, n = x.shape
        x2 = None if x2 is None else np.ascontiguousarray(x2, np.float32).reshape(T, n)
        nw = None if norm_w is None else np.ascontiguousarray(norm_w, np.float32).reshape(n)
        blk = np.zeros((T, 292 * (n // 256)), np.uint8)
        bh, bl, ph, pl = (np.zeros((T, n // 16), np.int8) for _ in range(4))
        yf = np.zeros((T, n), np.float32) if want_f32 else None
        self._chk(self.lib.mi355_op_act_q8k_planes(producer, _ptr(x), _ptr(x2), _ptr(nw), eps, n, T, _ptr(blk), _ptr(bh), _ptr(bl), _ptr(ph), _ptr(pl), _ptr(yf)),
                  "op_act_q8k_planes")
        return blk, bh, bl, ph, pl, yf

    def mul_mat(self, t: int, W: np.ndarray, N: int, K: int, x: np.ndarray, want_ints: bool = False):
        W = np.ascontiguousarray(W.view(np.uint8).reshape(-1))
        x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
        T = x.shape[0]
        y = np.zeros((T, N), np.float32)
        isum = msum = None
        if want_ints:
            nblk = K // 32 if t in (Q8_0, Q4_0, Q5_0, IQ4_NL, Q4_1, Q5_1, MXFP4) else K // 256
            isum = np.zeros((T, N, nblk), np.int32)
            msum = np.zeros((T, N, nblk), np.int32)
        self._chk(self.lib.mi355_op_mul_mat(t, _ptr(W), N, K, _ptr(x), T, _ptr(y), _ptr(isum), _ptr(msum)), "op_mul_mat")
        return (y, isum, msum) if want_ints else y

    def mul_mat_add(self, t: int, W: np.ndarray, N: int, K: int, x: np.ndarray, resid: np.ndarray) -> np.ndarray:
        """resid + W . x on the Q8_0 prompt kernel (see mi355_op_mul_mat_add)."""
        W = np.ascontiguousarray(W.view(np.uint8).reshape(-1))
        x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
        resid = np.ascontiguousarray(resid, np.float32).reshape(x.shape[0], N)
        y = np.zeros((x.shape[0], N), np.float32)
        self._chk(self.lib.mi355_op_mul_mat_add(t, _ptr(W), N, K, _ptr(x), x.shape[0], _ptr(resid), _ptr(y)), "op_mul_mat_add")
        return y

    def f32_to_bf16(self, x: np.ndarray) -> np.ndarray:
        """bf16 bits (uint16) of the f32 values, as the bf16 kernels round their activation rows; x.size % 8 == 0."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros(x.shape, np.uint16)
        self._chk(self.lib.mi355_op_f32_to_bf16(_ptr(x), x.size, _ptr(out)), "op_f32_to_bf16")
        return out

    def mul_mat_bf16(self, Ws, K: int, x: np.ndarray, bias=None, resid=None, epi: int = 0, path: int = 0, tokens_per_launch: int = 0, graph: bool = False):
        """Ws: 1..3 bf16 tensors as uint16 arrays [N][K]; x [T][K] f32 -> list of y [T][N] (one entry for epi 2, SwiGLU).  See mi355_op_mul_mat_bf16."""
        Ws = [np.ascontiguousarray(w).view(np.uint16).reshape(-1, K) for w in Ws]
        x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
        T, n = x.shape[0], len(Ws)
        Ns = np.array([w.shape[0] for w in Ws], np.int64)
        ys = [np.zeros((T, int(N)), np.float32) for N in (Ns[:1] if epi == 2 else Ns)]
        bs = [None if bias is None or b is None else np.ascontiguousarray(b, np.float32) for b in (bias or [None] * n)]
        r = None if resid is None else np.ascontiguousarray(resid, np.float32)
        parr = lambda xs: (C.c_void_p * len(xs))(*[None if a is None else a.ctypes.data for a in xs])
        wp, bp, yp = parr(Ws), parr(bs), parr(ys + [None] * (n - len(ys)))
        self._chk(self.lib.mi355_op_mul_mat_bf16(n, wp, _ptr(Ns), K, _ptr(x), T, bp if bias is not None else None, _ptr(r), epi, path, tokens_per_launch,
                                                 int(graph), yp), "op_mul_mat_bf16")
        return ys

    def ffn_gate_up(self, t: int, Wg: np.ndarray, Wu: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
        Wg = np.ascontiguousarray(Wg.view(np.uint8).reshape(-1))
        Wu = np.ascontiguousarray(Wu.view(np.uint8).reshape(-1))
        x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
        y = np.zeros((x.shape[0], N), np.float32)
        self._chk(self.lib.mi355_op_ffn_gate_up(t, _ptr(Wg), _ptr(Wu), N, K, _ptr(x), x.shape[0], _ptr(y)), "op_ffn_gate_up")
        return y

    def rms_norm_mul(self, x: np.ndarray, w: np.ndarray, eps: float) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        T, n = (1, x.size) if x.ndim == 1 else x.shape
        y = np.zeros_like(x)
        self._chk(self.lib.mi355_op_rms_norm_mul(_ptr(x), _ptr(w), n, T, eps, _ptr(y)), "op_rms_norm_mul")
        return y

    def rope(self, x: np.ndarray, n_head: int, head_dim: int, pos, base: float, neox: bool = False, n_rot=None,
             freq_scale: float = 1.0, freq_factors=None) -> np.ndarray:
        pos = np.ascontiguousarray(pos, np.int32).reshape(-1)
        y = np.array(x, np.float32, copy=True).reshape(pos.size, n_head * head_dim)
        ff = None if freq_factors is None else np.ascontiguousarray(freq_factors, np.float32)
        self._chk(self.lib.mi355_op_rope(_ptr(y), n_head, head_dim, n_rot or head_dim, _ptr(pos), pos.size, base, freq_scale,
                                         _ptr(ff), int(neox)), "op_rope")
        return y.reshape(pos.size, n_head, head_dim)

    def rope_yarn(self, x: np.ndarray, n_head: int, head_dim: int, pos, base: float, freq_scale: float, ext_factor: float, attn_factor: float,
                  corr_lo: float, corr_hi: float, neox: bool = False, n_rot=None) -> np.ndarray:
        pos = np.ascontiguousarray(pos, np.int32).reshape(-1)
        y = np.array(x, np.float32, copy=True).reshape(pos.size, n_head * head_dim)
        self._chk(self.lib.mi355_op_rope_yarn(_ptr(y), n_head, head_dim, n_rot or head_dim, _ptr(pos), pos.size, base, freq_scale, None, int(neox),
                                              ext_factor, attn_factor, corr_lo, corr_hi), "op_rope_yarn")
        return y.reshape(pos.size, n_head, head_dim)

    def get_rows(self, t: int, table: np.ndarray, K: int, n_rows: int, ids) -> np.ndarray:
        table = np.ascontiguousarray(table.view(np.uint8).reshape(-1))
        ids = np.ascontiguousarray(ids, np.int32)
        out = np.zeros((ids.size, K), np.float32)
        self._chk(self.lib.mi355_op_get_rows(t, _ptr(table), K, n_rows, _ptr(ids), ids.size, _ptr(out)), "op_get_rows")
        return out

    def repack_rows(self, t: int, rows: np.ndarray, K: int, n_rows: int, drow: int) -> np.ndarray:
        """The device rows of n_rows ggml rows, (n_rows, drow) bytes: what the upload makes of them, padding bytes left at the guard value 0xA5."""
        rows = np.ascontiguousarray(rows.view(np.uint8).reshape(-1))
        out = np.zeros((n_rows, drow), np.uint8)
        self._chk(self.lib.mi355_op_repack_rows(t, _ptr(rows), K, n_rows, _ptr(out)), "op_repack_rows")
        return out

    def swiglu(self, g: np.ndarray, u: np.ndarray) -> np.ndarray:
        g = np.ascontiguousarray(g, np.float32)
        u = np.ascontiguousarray(u, np.float32)
        y = np.zeros_like(g)
        self._chk(self.lib.mi355_op_swiglu(_ptr(g), _ptr(u), g.size, _ptr(y)), "op_swiglu")
        return y

    def soft_max(self, x: np.ndarray, mask, scale: float) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        rows, n = (1, x.size) if x.ndim == 1 else x.shape
        m = None if mask is None else np.ascontiguousarray(mask, np.float32)
        y = np.zeros_like(x)
        self._chk(self.lib.mi355_op_soft_max(_ptr(x), _ptr(m), n, rows, scale, _ptr(y)), "op_soft_max")
        return y

    def moe_route(self, logits: np.ndarray, k: int):
        x = np.ascontiguousarray(logits, np.float32)
        T, ne = x.shape
        ids = np.zeros((T, k), np.int32); w = np.zeros((T, k), np.float32)
        self._chk(self.lib.mi355_op_moe_route(_ptr(x), T, ne, k, _ptr(ids), _ptr(w)), "op_moe_route")
        return ids, w

    def moe_router(self, t: int, gate_inp: np.ndarray, n_expert: int, K: int, x: np.ndarray, k: int, fused: bool = True, forced=None):
        """gate_inp: f32 or f16 rows [n_expert][K] (t = F32 / F16); x [T][K] -> (logits [T][n_expert], ids [T][k], w [T][k])."""
        gate_inp = np.ascontiguousarray(gate_inp).view(np.uint8).reshape(-1)
        x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
        T = x.shape[0]
        f = None if forced is None else np.ascontiguousarray(forced, np.int32).reshape(T, k)
        logits = np.zeros((T, n_expert), np.float32); ids = np.zeros((T, k), np.int32); w = np.zeros((T, k), np.float32)
        self._chk(self.lib.mi355_op_moe_router(t, _ptr(gate_inp), n_expert, K, _ptr(x), T, k, int(fused), _ptr(f), _ptr(logits), _ptr(ids), _ptr(w)),
                  "op_moe_router")
        return logits, ids, w

    def argmax_rows(self, x: np.ndarray, launches=None, cap_rows=None) -> np.ndarray:
        """Row arg-max of x [rows][n] (mi355_op_argmax_rows): `launches` splits the rows into consecutive launches on one scratch of cap_rows rows
        (default: one launch of all rows)."""
        x = np.ascontiguousarray(x, np.float32)
        x = x.reshape(1, -1) if x.ndim == 1 else x
        la = np.ascontiguousarray([x.shape[0]] if launches is None else launches, np.int32).reshape(-1)
        cap = int(la.max() if cap_rows is None else cap_rows)
        assert int(la.sum()) == x.shape[0]
        out = np.full(x.shape[0], -1, np.int32)
        self._chk(self.lib.mi355_op_argmax_rows(_ptr(x), x.shape[1], _ptr(la), la.size, cap, _ptr(out)), "op_argmax_rows")
        return out

    def argmax_prob_rows(self, x: np.ndarray):
        """(arg-max int32 [rows], its softmax probability f32 [rows]) of x [rows][n] (mi355_op_argmax_prob_rows)."""
        x = np.ascontiguousarray(x, np.float32)
        x = x.reshape(1, -1) if x.ndim == 1 else x
        idx = np.full(x.shape[0], -1, np.int32); p = np.full(x.shape[0], -1.0, np.float32)
        self._chk(self.lib.mi355_op_argmax_prob_rows(_ptr(x), x.shape[1], x.shape[0], _ptr(idx), _ptr(p)), "op_argmax_prob_rows")
        return idx, p

    def spec_verify(self, logits: np.ndarray, rows, group_start, draft):
        """Greedy acceptance (mi355_op_spec_verify): launch row r = logits[rows[r]]; group g owns launch rows group_start[g] .. group_start[g + 1] - 1; draft
        runs parallel to the launch rows.  Returns (ids int32 [R], n_accept int32 [G])."""
        logits = np.ascontiguousarray(logits, np.float32)
        rows = np.ascontiguousarray(rows, np.int32).reshape(-1)
        gs = np.ascontiguousarray(group_start, np.int32).reshape(-1)
        draft = np.ascontiguousarray(draft, np.int32).reshape(-1)
        R, G = rows.size, gs.size - 1
        assert draft.size == R
        ids = np.full(R, -1, np.int32); acc = np.full(max(G, 1), -1, np.int32)
        self._chk(self.lib.mi355_op_spec_verify(_ptr(logits), logits.shape[1], logits.shape[0], _ptr(rows), R, _ptr(gs), G, _ptr(draft), _ptr(ids), _ptr(acc)),
                  "op_spec_verify")
        return ids, acc[:G]

    def token_logprob_rows(self, base: np.ndarray, targets, rows=None):
        """(log-probability f32 [R], rank int32 [R]) of targets[r] in base[rows[r]] (rows None: row r) over the whole row (mi355_op_token_logprob_rows)."""
        base = np.ascontiguousarray(base, np.float32)
        base = base.reshape(1, -1) if base.ndim == 1 else base
        targets = np.ascontiguousarray(targets, np.int32).reshape(-1)
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32).reshape(-1)
        R = targets.size
        assert rows is None or rows.size == R
        lp = np.full(R, 7.0, np.float32); rank = np.full(R, -7, np.int32)
        self._chk(self.lib.mi355_op_token_logprob_rows(_ptr(base), base.shape[1], base.shape[0], None if rows is None else _ptr(rows), _ptr(targets), R, _ptr(lp),
                                                       _ptr(rank)), "op_token_logprob_rows")
        return lp, rank

    def logits_kl_rows(self, p: np.ndarray, q: np.ndarray, rows_p=None, rows_q=None):
        """(KL(P || Q) f32 [R], same_top int32 [R]) of the pairs (p[rows_p[r]], q[rows_q[r]]) (None: row r) (mi355_op_logits_kl_rows)."""
        p = np.ascontiguousarray(p, np.float32); q = np.ascontiguousarray(q, np.float32)
        p = p.reshape(1, -1) if p.ndim == 1 else p
        q = q.reshape(1, -1) if q.ndim == 1 else q
        assert p.shape[1] == q.shape[1]
        rows_p = None if rows_p is None else np.ascontiguousarray(rows_p, np.int32).reshape(-1)
        rows_q = None if rows_q is None else np.ascontiguousarray(rows_q, np.int32).reshape(-1)
        R = rows_p.size if rows_p is not None else rows_q.size if rows_q is not None else min(p.shape[0], q.shape[0])
        assert (rows_p is None or rows_p.size == R) and (rows_q is None or rows_q.size == R)
        kl = np.full(R, 7.0, np.float32); top = np.full(R, -7, np.int32)
        self._chk(self.lib.mi355_op_logits_kl_rows(_ptr(p), p.shape[0], _ptr(q), q.shape[0], p.shape[1], None if rows_p is None else _ptr(rows_p),
                                                   None if rows_q is None else _ptr(rows_q), R, _ptr(kl), _ptr(top)), "op_logits_kl_rows")
        return kl, top

    def imatrix_accum(self, x: np.ndarray, sum2: np.ndarray, counts: np.ndarray, x2=None, K=None, R=None, row_src=None, counts_per_mat=None):
        """The importance-matrix collector launch (mi355_op_imatrix_accum) on rows x [n_src_rows][ld] (x2: the SwiGLU producer's second operand): returns
        (sum2 [n_mat + 1][K], counts [n_mat]) = the running totals given plus this launch; the last row of sum2 is a guard row.  K defaults to ld, R to the
        rows of row_src or of x; counts_per_mat [n_mat] cuts the launch rows into one run per matrix (None: one matrix).  The inputs are not modified."""
        x = np.ascontiguousarray(x, np.float32)
        assert x.ndim == 2
        x2 = None if x2 is None else np.ascontiguousarray(x2, np.float32)
        assert x2 is None or x2.shape == x.shape
        row_src = None if row_src is None else np.ascontiguousarray(row_src, np.int32).reshape(-1)
        cpm = None if counts_per_mat is None else np.ascontiguousarray(counts_per_mat, np.int32).reshape(-1)
        ld = x.shape[1]
        K = ld if K is None else int(K)
        R = int(R) if R is not None else (row_src.size if row_src is not None else x.shape[0])
        out = np.array(sum2, np.float32, copy=True, order="C")
        cnt = np.array(counts, np.int32, copy=True, order="C").reshape(-1)
        n_mat = cnt.size
        assert out.shape == (n_mat + 1, K) and (cpm is None or cpm.size == n_mat) and (row_src is None or row_src.size >= R)
        self._chk(self.lib.mi355_op_imatrix_accum(_ptr(x), _ptr(x2), ld, K, R, _ptr(row_src), x.shape[0], _ptr(cpm), n_mat, _ptr(out), _ptr(cnt)), "op_imatrix_accum")
        return out, cnt

    # ---- the LLaVA image encoder's launches, one at a time (include/mi355_llama.h; tests/test_gpu_clip_ops.py).  f16 outputs come back as np.float16.
    def clip_attn_rc(self, q: np.ndarray, k: np.ndarray, v: np.ndarray, T: int, H: int, D: int, n_img: int = 1, want_h: bool = True):
        """The tower's attention within each of n_img images of T rows (q pre-scaled; q, k, v [n_img * T][H * D]).  Returns (rc, out, out_h or None, path):
        path 1 matrix cores, 2 LDS-tiled, 3 one wave per query, 0 refused (rc != 0, nothing launched)."""
        q, k, v = (np.ascontiguousarray(a, np.float32).reshape(n_img * T, H * D) for a in (q, k, v))
        out = np.zeros_like(q)
        out_h = np.zeros(q.shape, np.float16) if want_h else None
        path = np.full(1, -1, np.int32)
        rc = self.lib.mi355_op_clip_attn(_ptr(q), _ptr(k), _ptr(v), T, H, D, n_img, _ptr(out), _ptr(out_h), _ptr(path))
        return int(rc), out, out_h, int(path[0])

    def clip_attn(self, q, k, v, T: int, H: int, D: int, n_img: int = 1, want_h: bool = True):
        rc, out, out_h, path = self.clip_attn_rc(q, k, v, T, H, D, n_img, want_h)
        self._chk(rc, "op_clip_attn")
        return out, out_h, path

    def mul_mat_f16_xh_rc(self, W: np.ndarray, x: np.ndarray, ld_out=None, bias=None, scale=None, resid=None, in_place: bool = False, form: int = 0, y_init=None):
        """y = resid + (W . f16(x) + bias) * scale; W [N][K] float16, x [T][K].  Returns (rc, y [T][ld_out]): y starts as y_init (zeros without one; with
        in_place, as resid, which the launch then reads and writes in the one buffer), so the columns past N show whether the launch left them alone."""
        W = np.ascontiguousarray(W, np.float16)
        N, K = W.shape
        x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
        T = x.shape[0]
        ld = N if ld_out is None else int(ld_out)
        b = None if bias is None else np.ascontiguousarray(bias, np.float32).reshape(N)
        r = None if resid is None else np.ascontiguousarray(resid, np.float32).reshape(T, ld)
        y = np.array(r if in_place else (np.zeros((T, ld), np.float32) if y_init is None else y_init), np.float32, copy=True, order="C").reshape(T, ld)
        rc = self.lib.mi355_op_mul_mat_f16_xh(_ptr(W.view(np.uint16)), N, K, _ptr(x), T, ld, _ptr(b), 1.0 if scale is None else float(scale), int(scale is not None),
                                              None if in_place else _ptr(r), int(in_place), form, _ptr(y))
        return int(rc), y

    def mul_mat_f16_xh(self, W, x, **kw) -> np.ndarray:
        rc, y = self.mul_mat_f16_xh_rc(W, x, **kw)
        self._chk(rc, "op_mul_mat_f16_xh")
        return y

    def layer_norm(self, x: np.ndarray, w: np.ndarray, b: np.ndarray, eps: float, want_h: bool = True, in_place: bool = False):
        """LayerNorm with weight and bias over the rows of x [T][n] -> (y, y_h or None)."""
        x = np.ascontiguousarray(x, np.float32)
        T, n = x.shape
        w, b = np.ascontiguousarray(w, np.float32).reshape(n), np.ascontiguousarray(b, np.float32).reshape(n)
        y = np.zeros_like(x)
        y_h = np.zeros(x.shape, np.float16) if want_h else None
        self._chk(self.lib.mi355_op_layer_norm(_ptr(x), _ptr(w), _ptr(b), n, T, eps, int(in_place), _ptr(y), _ptr(y_h)), "op_layer_norm")
        return y, y_h

    def clip_gelu(self, x: np.ndarray, quick: bool, want_h: bool = True):
        """ggml's f16-table GELU / quick-GELU -> (y, y_h or None)."""
        x = np.ascontiguousarray(x, np.float32)
        y = np.zeros_like(x)
        y_h = np.zeros(x.shape, np.float16) if want_h else None
        self._chk(self.lib.mi355_op_clip_gelu(_ptr(x), x.size, int(quick), _ptr(y), _ptr(y_h)), "op_clip_gelu")
        return y, y_h

    def clip_im2col(self, img: np.ndarray, P: int, ld: int, fill: float = 0.0) -> np.ndarray:
        """img [3][S][S] -> patches [(S / P)^2][ld]; the device buffer holds `fill` everywhere before the launch."""
        img = np.ascontiguousarray(img, np.float32)
        S = img.shape[-1]
        out = np.full(((S // P) ** 2, ld), fill, np.float32)
        self._chk(self.lib.mi355_op_clip_im2col(_ptr(img), S, P, ld, _ptr(out)), "op_clip_im2col")
        return out

    def clip_embed(self, patch: np.ndarray, cls: np.ndarray, pos: np.ndarray) -> np.ndarray:
        """[class ; patches] + positions: patch [T - 1][E], cls [E], pos [T][E] -> [T][E]."""
        pos = np.ascontiguousarray(pos, np.float32)
        T, E = pos.shape
        patch, cls = np.ascontiguousarray(patch, np.float32).reshape(T - 1, E), np.ascontiguousarray(cls, np.float32).reshape(E)
        out = np.zeros_like(pos)
        self._chk(self.lib.mi355_op_clip_embed(_ptr(patch), _ptr(cls), _ptr(pos), E, T, _ptr(out)), "op_clip_embed")
        return out

    def clip_bias(self, x: np.ndarray, b: np.ndarray, scale=None) -> np.ndarray:
        """(x + b) [* scale] over the rows of x [T][n]."""
        y = np.array(x, np.float32, copy=True, order="C")
        T, n = y.shape
        b = np.ascontiguousarray(b, np.float32).reshape(n)
        self._chk(self.lib.mi355_op_clip_bias(_ptr(y), _ptr(b), n, T, 1.0 if scale is None else float(scale), int(scale is not None)), "op_clip_bias")
        return y

    def f32_to_f16(self, x: np.ndarray) -> np.ndarray:
        """f16 (round to nearest even) of the f32 values, as the f16 GEMM's activation rows are made; x.size % 4 == 0."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros(x.shape, np.float16)
        self._chk(self.lib.mi355_op_f32_to_f16(_ptr(x), x.size, _ptr(out)), "op_f32_to_f16")
        return out

    def add_qkv_bias(self, q, k, v, bq, bk, bv, nq: int, nkv: int, T: int):
        """q [T][nq] += bq, k / v [T][nkv] += bk / bv in one launch; None skips.  Returns copies (None where None went in)."""
        xs = [None if a is None else np.array(a, np.float32, copy=True, order="C") for a in (q, k, v)]
        bs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (bq, bk, bv)]
        self._chk(self.lib.mi355_op_add_qkv_bias(_ptr(xs[0]), _ptr(xs[1]), _ptr(xs[2]), _ptr(bs[0]), _ptr(bs[1]), _ptr(bs[2]), nq, nkv, T), "op_add_qkv_bias")
        return xs

    def quantize_rows(self, dst_type: int, x: np.ndarray, imatrix=None, src_type=None) -> np.ndarray:
        """The quantiser (mi355_quantize_chunk): rows x [n_rows][n_per_row] - float32, float16, or uint16 holding bf16 bits with src_type=30 - to ggml-layout
        blocks of dst_type, uint8 [n_rows][row bytes]; imatrix: None or n_per_row column weights.  A type or shape the entry refuses raises MI355Error."""
        x = np.ascontiguousarray(x)
        if src_type is None:
            src_type = {np.dtype(np.float32): 0, np.dtype(np.float16): 1}.get(x.dtype)
            if src_type is None:
                x, src_type = np.ascontiguousarray(x, np.float32), 0
        assert x.ndim == 2 and x.dtype == {0: np.float32, 1: np.float16, 30: np.uint16}.get(src_type, x.dtype)
        n_rows, n = x.shape
        im = None if imatrix is None else np.ascontiguousarray(imatrix, np.float32).reshape(-1)
        assert im is None or im.size == n
        from .gguf_synth import BLOCK_BYTES, BLOCK_ELEMS
        be, bb = BLOCK_ELEMS.get(dst_type, 1), BLOCK_BYTES.get(dst_type, 1)
        out = np.zeros((n_rows, n // be * bb if n % be == 0 else 1), np.uint8)
        self._chk(self.lib.mi355_quantize_chunk(dst_type, src_type, _ptr(x), n, n_rows, _ptr(im), _ptr(out)), "quantize_chunk")
        return out

    def add_row_vec(self, x: np.ndarray, v: np.ndarray) -> np.ndarray:
        """The control vector's add once (mi355_op_add_row_vec): x [T][E] + v [E]; returns [T + 1][E], the last row the guard row behind the rows (0xA5 bytes)."""
        x = np.ascontiguousarray(x, np.float32)
        v = np.ascontiguousarray(v, np.float32).reshape(-1)
        T, E = x.shape
        assert v.size == E
        y = np.zeros((T + 1, E), np.float32)
        self._chk(self.lib.mi355_op_add_row_vec(_ptr(x), _ptr(v), E, T, _ptr(y)), "op_add_row_vec")
        return y

    def load_control_vectors(self, items):
        """common_control_vector_load (mi355_control_vector_load): items = [(path, scale), ...] -> (data f32 [n_layers_named * n_embd], n_embd)."""
        return control_vector_load(self.lib, items)

    def cvec_direction(self, rows: np.ndarray, init=None, method: str = "pca", n_iter: int = 1000, n_batch: int = 100, tol: float = 1e-7, dir_out=None):
        """The direction of rows [R][E] (mi355_cvec_direction): (dir f32 [E], iterations, last distance).  dir_out: an array to receive it (tests)."""
        rows = np.ascontiguousarray(rows, np.float32)
        assert rows.ndim == 2
        R, E = rows.shape
        ini = None if init is None else np.ascontiguousarray(init, np.float32).reshape(-1)
        assert ini is None or ini.size == E
        out = np.zeros(E, np.float32) if dir_out is None else dir_out
        assert out.dtype == np.float32 and out.size == E and out.flags.c_contiguous
        it = np.zeros(1, np.int32); dist = np.zeros(1, np.float32)
        self._chk(self.lib.mi355_cvec_direction({"pca": 0, "mean": 1}.get(method, -1) if isinstance(method, str) else int(method), _ptr(rows), R, E, _ptr(ini),
                                                int(n_iter), int(n_batch), float(tol), _ptr(out), _ptr(it), _ptr(dist)), "cvec_direction")
        return out, int(it[0]), float(dist[0])

    def quantize_last_times(self):
        """(upload, kernel, download) milliseconds of this thread's last quantize_rows (mi355_quantize_last_times)"""
        t = np.zeros(3, np.float32)
        p = t.ctypes.data
        self._chk(self.lib.mi355_quantize_last_times(C.c_void_p(p), C.c_void_p(p + 4), C.c_void_p(p + 8)), "quantize_last_times")
        return float(t[0]), float(t[1]), float(t[2])

    @staticmethod
    def topk_decode(keys: np.ndarray):
        """(tokens int32, logits f32) of top-k keys: the inverse of the order-preserving image, as Context::topk_rows applies it."""
        keys = np.asarray(keys, np.uint64)
        u = (keys >> np.uint64(32)).astype(np.uint32)
        u = np.where(u >> np.uint32(31), u ^ np.uint32(0x80000000), u ^ np.uint32(0xffffffff)).astype(np.uint32)
        toks = (np.uint32(0xffffffff) - (keys & np.uint64(0xffffffff)).astype(np.uint32)).astype(np.uint32).view(np.int32)
        return toks, u.view(np.float32)

    def topk_rows(self, base: np.ndarray, rows, k: int, adjs=None, adj_n=None):
        """The k best of logits rows base[rows[r]] after adjustments adjs[r] = (tok [m], bias [m], cnt [m], repeat, freq, present) (None: no adjustment;
        adj_n overrides the entry counts handed over): returns (tokens [n_rows][k], logits [n_rows][k], raw keys [n_rows][k] uint64)."""
        base = np.ascontiguousarray(base, np.float32)
        base = base.reshape(1, -1) if base.ndim == 1 else base
        rows = np.ascontiguousarray(rows, np.int32).reshape(-1)
        R, A = rows.size, 192
        an = np.zeros(R, np.int32); tok = np.zeros((R, A), np.int32); bias = np.zeros((R, A), np.float32); cnt = np.zeros((R, A), np.int32)
        rep = np.ones(R, np.float32); freq = np.zeros(R, np.float32); pres = np.zeros(R, np.float32)
        for r, a in enumerate(adjs or []):
            if a is None:
                continue
            m = min(len(a[0]), A)
            an[r] = len(a[0])
            tok[r, :m] = np.asarray(a[0], np.int32)[:m]; bias[r, :m] = np.asarray(a[1], np.float32)[:m]; cnt[r, :m] = np.asarray(a[2], np.int32)[:m]
            rep[r], freq[r], pres[r] = a[3], a[4], a[5]
        if adj_n is not None:
            an = np.ascontiguousarray(adj_n, np.int32).reshape(R)
        keys = np.zeros((R, max(int(k), 1)), np.uint64)
        self._chk(self.lib.mi355_op_topk_rows(_ptr(base), base.shape[1], base.shape[0], _ptr(rows), R, int(k), _ptr(an), _ptr(tok), _ptr(bias), _ptr(cnt),
                                              _ptr(rep), _ptr(freq), _ptr(pres), _ptr(keys)), "op_topk_rows")
        toks, logits = self.topk_decode(keys)
        return toks, logits, keys

    def lora_delta(self, segs, x: np.ndarray):
        """The adapter kernels once (mi355_op_lora_delta): segs = 1 .. 3 of (A [r][K], B [N][r], scale, out [T][ld_out]) over the rows x [T][K]; A and B both
        float32 or both float16.  Returns the new out arrays (copies): out[t][n] + scale * B[n] . (A x[t]) for n < N, the rest as it was."""
        x = np.ascontiguousarray(x, np.float32)
        T, K = x.shape
        n = len(segs)
        As = [np.ascontiguousarray(sg[0]) for sg in segs]
        Bs = [np.ascontiguousarray(sg[1]) for sg in segs]
        outs = [np.array(sg[3], np.float32, order="C", copy=True).reshape(T, -1) for sg in segs]
        types = np.array([{np.dtype(np.float32): F32, np.dtype(np.float16): F16}.get(a.dtype, -1) for a in As], np.int32)
        r = np.array([a.shape[0] if a.ndim == 2 else 0 for a in As], np.int32)
        N = np.array([b.shape[0] for b in Bs], np.int64)
        scale = np.array([sg[2] for sg in segs], np.float32)
        ld = np.array([o.shape[1] for o in outs], np.int64)
        pa = (C.c_void_p * n)(*[a.ctypes.data for a in As]); pb = (C.c_void_p * n)(*[b.ctypes.data for b in Bs]); po = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        self._chk(self.lib.mi355_op_lora_delta(n, _ptr(types), pa, pb, _ptr(r), _ptr(N), _ptr(scale), _ptr(x), K, T, _ptr(ld), po), "op_lora_delta")
        return outs

    def moe_group(self, ids: np.ndarray, n_expert: int):
        """Grouping of the selections ids [T][k] by expert (mi355_op_moe_group): (meta [2 n_expert + 1], slot_of [T * k], tok_of [T * k])."""
        ids = np.ascontiguousarray(ids, np.int32)
        T, k = ids.shape
        meta = np.full(2 * max(int(n_expert), 0) + 1, -1, np.int32); slot_of = np.full(T * k, -1, np.int32); tok_of = np.full(T * k, -1, np.int32)
        self._chk(self.lib.mi355_op_moe_group(_ptr(ids), T, k, int(n_expert), _ptr(meta), _ptr(slot_of), _ptr(tok_of)), "op_moe_group")
        return meta, slot_of, tok_of

    def moe_gather_act(self, planes, tok_of, K: int, guard: int = 0xA5):
        """grouped row r = row tok_of[r] of every plane given (mi355_op_moe_gather_act).  planes: (qs, d, bsums, qs0, d0) as byte arrays [T][row bytes], the
        Q8_K triple or the Q8_0 pair may be None.  Returns the five output planes as uint8 [n_rows + 1][row bytes] (None where not given): they are filled
        with `guard` before the launch, so the last row, and every byte the kernel does not write, comes back as that."""
        tok_of = np.ascontiguousarray(tok_of, np.int32).reshape(-1)
        src = [None if p is None else np.ascontiguousarray(p).view(np.uint8).reshape(np.asarray(p).shape[0], -1) for p in planes]
        T = next(p.shape[0] for p in src if p is not None)
        out = [None if p is None else np.full((tok_of.size + 1, p.shape[1]), guard, np.uint8) for p in src]
        self._chk(self.lib.mi355_op_moe_gather_act(*[_ptr(p) for p in src], T, int(K), _ptr(tok_of), tok_of.size, *[_ptr(p) for p in out]), "op_moe_gather_act")
        return out

    def moe_combine(self, x: np.ndarray, eo: np.ndarray, w: np.ndarray, slot_of=None) -> np.ndarray:
        """x [T][E] + the weighted expert outputs in rank order (mi355_op_moe_combine): eo [k][T][E], or with slot_of [T * k] the grouped rows [T * k][E]."""
        x = np.ascontiguousarray(x, np.float32); eo = np.ascontiguousarray(eo, np.float32); w = np.ascontiguousarray(w, np.float32)
        T, E = x.shape
        k = w.shape[1]
        assert w.shape[0] == T and eo.size == T * k * E
        s = None if slot_of is None else np.ascontiguousarray(slot_of, np.int32).reshape(T * k)
        y = np.zeros_like(x)
        self._chk(self.lib.mi355_op_moe_combine(_ptr(x), _ptr(eo), _ptr(w), T, E, k, int(s is not None), _ptr(s), _ptr(y)), "op_moe_combine")
        return y

    def moe_mul_mat_grouped(self, t: int, form: int, Ws, n_expert: int, N: int, K: int, x: np.ndarray, counts, ld_out=None, guard_rows: int = 2, R=None):
        """One grouped-expert launch of a prompt batch (mi355_op_moe_mul_mat_grouped).  form 0: planes, one projection; 1: planes, gate | up with SwiGLU;
        2 / 3: the Q8_0-layout copies, one / two segments.  Ws: one or two arrays of n_expert tensors back to back (ggml rows); x [R][K] grouped rows; counts
        [n_expert].  Returns the whole out buffers [R + guard_rows][ld_out] (two for form 3): what the launch did not write holds 0xFF bytes."""
        Ws = [np.ascontiguousarray(w.view(np.uint8).reshape(-1)) for w in Ws]
        x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
        counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
        assert counts.size == n_expert and all(w.size % n_expert == 0 for w in Ws)
        R = x.shape[0] if R is None else int(R)
        ld = int(N) if ld_out is None else int(ld_out)
        ys = [np.zeros((R + guard_rows, ld), np.float32) for _ in range(2 if form == 3 else 1)]
        self._chk(self.lib.mi355_op_moe_mul_mat_grouped(t, form, _ptr(Ws[0]), _ptr(Ws[1]) if len(Ws) > 1 else None, int(n_expert), int(N), int(K), _ptr(x), _ptr(counts),
                                                        R, ld, guard_rows, _ptr(ys[0]), _ptr(ys[1]) if len(ys) > 1 else None), "op_moe_mul_mat_grouped")
        return ys

    def gather_rows_f32(self, src: np.ndarray, rows) -> np.ndarray:
        src = np.ascontiguousarray(src, np.float32)
        rows = np.ascontiguousarray(rows, np.int32).reshape(-1)
        dst = np.zeros((rows.size, src.shape[1]), np.float32)
        self._chk(self.lib.mi355_op_gather_rows_f32(_ptr(src), src.shape[0], src.shape[1], _ptr(rows), rows.size, _ptr(dst)), "op_gather_rows_f32")
        return dst

    def flash_attn(self, q: np.ndarray, n_head: int, n_head_kv: int, hd: int, type_k: int, k_rows: np.ndarray, type_v: int,
                   v_rows: np.ndarray, cell_pos, q_pos, scale: float, cell_seq=None, q_seq=None, n_kv=None) -> np.ndarray:
        """flash_attn_ext over a caller-supplied cache (mi355_op_flash_attn).  With cell_seq (uint64 [n_cells] bit masks), q_seq ([T], 0 .. 63) or n_kv (cells
        the kernels scan; the launch stays sized for all of them) it is mi355_op_flash_attn_seq; what is left out is mask 1, sequence 0, every cell."""
        q = np.ascontiguousarray(q, np.float32)
        q_pos = np.ascontiguousarray(q_pos, np.int32).reshape(-1)
        cell_pos = np.ascontiguousarray(cell_pos, np.int32)
        k_rows = np.ascontiguousarray(k_rows.view(np.uint8))
        v_rows = np.ascontiguousarray(v_rows.view(np.uint8))
        out = np.zeros((q_pos.size, n_head, hd), np.float32)
        if cell_seq is None and q_seq is None and n_kv is None:
            self._chk(self.lib.mi355_op_flash_attn(_ptr(q), q_pos.size, n_head, n_head_kv, hd, type_k, _ptr(k_rows), type_v,
                                                   _ptr(v_rows), cell_pos.size, _ptr(cell_pos), _ptr(q_pos), scale, _ptr(out)),
                      "op_flash_attn")
            return out
        cs = np.ones(cell_pos.size, np.uint64) if cell_seq is None else np.ascontiguousarray(cell_seq, np.uint64).reshape(-1)
        qs = np.zeros(q_pos.size, np.int32) if q_seq is None else np.ascontiguousarray(q_seq, np.int32).reshape(-1)
        assert cs.size == cell_pos.size and qs.size == q_pos.size
        self._chk(self.lib.mi355_op_flash_attn_seq(_ptr(q), q_pos.size, n_head, n_head_kv, hd, type_k, _ptr(k_rows), type_v, _ptr(v_rows), cell_pos.size,
                                                   _ptr(cell_pos), _ptr(cs), _ptr(q_pos), _ptr(qs), int(cell_pos.size if n_kv is None else n_kv), scale, _ptr(out)),
                  "op_flash_attn_seq")
        return out

    def flash_attn_plan(self, T: int, n_head: int, n_head_kv: int, hd: int, type_k: int, type_v: int, n_cells: int):
        """(key splits of the split kernel, key splits of the matrix-core prompt kernel, whether the prompt kernel takes the call) for a flash_attn call."""
        o = np.zeros(3, np.int32)
        self._chk(self.lib.mi355_op_flash_attn_plan(int(T), n_head, n_head_kv, hd, type_k, type_v, int(n_cells), _ptr(o)), "op_flash_attn_plan")
        return int(o[0]), int(o[1]), bool(o[2])

    def attn_step(self, q, k_new, v_new, n_head: int, n_head_kv: int, hd: int, type_k: int, k_rows, type_v: int, v_rows, cell_pos, tok_pos: int,
                  tok_cell: int, rope_base: float, n_rot: int, scale: float, type_o: int, W_o, n_embd: int, resid, fused: bool, k_row_bytes: int, v_row_bytes: int,
                  cell_seq=None, tok_seq: int = 0, use_lists: bool = False):
        """One single-token attention block (mi355_op_attn_step): returns (att [H * D], out [n_embd], k_row, v_row).  cell_seq / tok_seq / use_lists: the cells'
        sequence masks, the token's sequence and the chunk-list walk (mi355_op_attn_step_seq)."""
        q = np.ascontiguousarray(q, np.float32); k_new = np.ascontiguousarray(k_new, np.float32); v_new = np.ascontiguousarray(v_new, np.float32)
        cell_pos = np.ascontiguousarray(cell_pos, np.int32)
        k_rows = np.ascontiguousarray(k_rows.view(np.uint8)); v_rows = np.ascontiguousarray(v_rows.view(np.uint8))
        W_o = np.ascontiguousarray(W_o.view(np.uint8)); resid = np.ascontiguousarray(resid, np.float32)
        att = np.zeros(n_head * hd, np.float32); out = np.zeros(n_embd, np.float32)
        kr = np.zeros(k_row_bytes, np.uint8); vr = np.zeros(v_row_bytes, np.uint8)
        if cell_seq is None and tok_seq == 0 and not use_lists:
            self._chk(self.lib.mi355_op_attn_step(_ptr(q), _ptr(k_new), _ptr(v_new), n_head, n_head_kv, hd, type_k, _ptr(k_rows), type_v, _ptr(v_rows), cell_pos.size,
                                                  _ptr(cell_pos), int(tok_pos), int(tok_cell), float(rope_base), int(n_rot), float(scale), type_o, _ptr(W_o), n_embd,
                                                  _ptr(resid), int(bool(fused)), _ptr(att), _ptr(out), _ptr(kr), _ptr(vr)), "op_attn_step")
            return att, out, kr, vr
        cs = None if cell_seq is None else np.ascontiguousarray(cell_seq, np.uint64).reshape(-1)
        assert cs is None or cs.size == cell_pos.size
        self._chk(self.lib.mi355_op_attn_step_seq(_ptr(q), _ptr(k_new), _ptr(v_new), n_head, n_head_kv, hd, type_k, _ptr(k_rows), type_v, _ptr(v_rows), cell_pos.size,
                                                  _ptr(cell_pos), _ptr(cs), int(tok_pos), int(tok_seq), int(tok_cell), int(bool(use_lists)), float(rope_base), int(n_rot),
                                                  float(scale), type_o, _ptr(W_o), n_embd, _ptr(resid), int(bool(fused)), _ptr(att), _ptr(out), _ptr(kr), _ptr(vr)),
                  "op_attn_step_seq")
        return att, out, kr, vr

    def attn_decode_neox(self, q, k_new, v_new, n_head: int, n_head_kv: int, hd: int, type_k: int, k_rows, type_v: int, v_rows, cell_pos, tok_pos: int,
                         tok_cell: int, rope_base: float, scale: float, q_norm, k_norm, eps: float, mode: int, k_row_bytes: int, v_row_bytes: int,
                         cell_seq=None, tok_seq: int = 0, use_lists: bool = False):
        """The decode attention of one token with NEOX rope and optional per-head q / k RMSNorm weights (mi355_op_attn_decode_neox; q_norm / k_norm: [hd]
        f32 or None): returns (att [H * D], k_row, v_row).  mode 1: single-launch step, 0: store-fused batched form, 2: generic rope_kv_store path.
        cell_seq / tok_seq / use_lists as attn_step (mi355_op_attn_decode_neox_seq)."""
        q = np.ascontiguousarray(q, np.float32); k_new = np.ascontiguousarray(k_new, np.float32); v_new = np.ascontiguousarray(v_new, np.float32)
        cell_pos = np.ascontiguousarray(cell_pos, np.int32)
        k_rows = np.ascontiguousarray(k_rows.view(np.uint8)); v_rows = np.ascontiguousarray(v_rows.view(np.uint8))
        qn = None if q_norm is None else np.ascontiguousarray(q_norm, np.float32)
        kn = None if k_norm is None else np.ascontiguousarray(k_norm, np.float32)
        att = np.zeros(n_head * hd, np.float32)
        kr = np.zeros(k_row_bytes, np.uint8); vr = np.zeros(v_row_bytes, np.uint8)
        if cell_seq is None and tok_seq == 0 and not use_lists:
            self._chk(self.lib.mi355_op_attn_decode_neox(_ptr(q), _ptr(k_new), _ptr(v_new), n_head, n_head_kv, hd, type_k, _ptr(k_rows), type_v, _ptr(v_rows),
                                                         cell_pos.size, _ptr(cell_pos), int(tok_pos), int(tok_cell), float(rope_base), float(scale),
                                                         None if qn is None else _ptr(qn), None if kn is None else _ptr(kn), float(eps), int(mode),
                                                         _ptr(att), _ptr(kr), _ptr(vr)), "op_attn_decode_neox")
            return att, kr, vr
        cs = None if cell_seq is None else np.ascontiguousarray(cell_seq, np.uint64).reshape(-1)
        assert cs is None or cs.size == cell_pos.size
        self._chk(self.lib.mi355_op_attn_decode_neox_seq(_ptr(q), _ptr(k_new), _ptr(v_new), n_head, n_head_kv, hd, type_k, _ptr(k_rows), type_v, _ptr(v_rows),
                                                         cell_pos.size, _ptr(cell_pos), _ptr(cs), int(tok_pos), int(tok_seq), int(tok_cell), int(bool(use_lists)),
                                                         float(rope_base), float(scale), _ptr(qn), _ptr(kn), float(eps), int(mode), _ptr(att), _ptr(kr), _ptr(vr)),
                  "op_attn_decode_neox_seq")
        return att, kr, vr

    def attn_batch_step(self, mode: int, q, k_new, v_new, n_head: int, n_head_kv: int, hd: int, type_k: int, k_rows, type_v: int, v_rows, n_kv: int, cell_pos,
                        cell_seq, tok_pos, tok_seq, tok_cell, rope_base: float, n_rot: int, neox: bool, scale: float, want_q8k: bool = False, want_planes: bool = False):
        """The attention of one batched single-token step (mi355_op_attn_batch_step; mode 0: store inside the attention launch, 1: the same on chunk lists,
        2: small-batch store + attention on the lists, 3: generic store + attention).  k_rows / v_rows: the whole cache before the step [n_cells][row bytes];
        returns (att [T][H * D], the whole K cache after the step, the whole V cache, the Q8_K blocks [T][292 * H * D / 256] or None).  Inputs are not modified."""
        tok_pos = np.ascontiguousarray(tok_pos, np.int32).reshape(-1)
        tok_seq = np.ascontiguousarray(tok_seq, np.int32).reshape(-1); tok_cell = np.ascontiguousarray(tok_cell, np.int32).reshape(-1)
        T = tok_pos.size
        q = np.ascontiguousarray(q, np.float32).reshape(T, n_head * hd)
        k_new = np.ascontiguousarray(k_new, np.float32).reshape(T, n_head_kv * hd); v_new = np.ascontiguousarray(v_new, np.float32).reshape(T, n_head_kv * hd)
        cell_pos = np.ascontiguousarray(cell_pos, np.int32).reshape(-1); cell_seq = np.ascontiguousarray(cell_seq, np.uint64).reshape(-1)
        kc = np.array(k_rows, order="C", copy=True).view(np.uint8); vc = np.array(v_rows, order="C", copy=True).view(np.uint8)
        assert tok_seq.size == T and tok_cell.size == T and kc.ndim == 2 and vc.ndim == 2 and kc.shape[0] == vc.shape[0] == cell_pos.size == cell_seq.size
        att = np.zeros((T, n_head * hd), np.float32)
        blk = np.zeros((T, 292 * (n_head * hd // 256)), np.uint8) if want_q8k or want_planes else None
        if want_planes:          # (... and the merge's bh / bl block-sum planes [T][H * D / 16] int8 behind the four results: mi355_op_attn_batch_step_planes)
            bh, bl = np.zeros((T, n_head * hd // 16), np.int8), np.zeros((T, n_head * hd // 16), np.int8)
            self._chk(self.lib.mi355_op_attn_batch_step_planes(_ptr(q), _ptr(k_new), _ptr(v_new), T, n_head, n_head_kv, hd, type_k, _ptr(kc), type_v, _ptr(vc),
                                                               cell_pos.size, int(n_kv), _ptr(cell_pos), _ptr(cell_seq), _ptr(tok_pos), _ptr(tok_seq), _ptr(tok_cell),
                                                               float(rope_base), int(n_rot), int(bool(neox)), float(scale), int(mode), _ptr(att), _ptr(blk), _ptr(bh),
                                                               _ptr(bl)), "op_attn_batch_step_planes")
            return att, kc, vc, blk, bh, bl
        self._chk(self.lib.mi355_op_attn_batch_step(_ptr(q), _ptr(k_new), _ptr(v_new), T, n_head, n_head_kv, hd, type_k, _ptr(kc), type_v, _ptr(vc), cell_pos.size,
                                                    int(n_kv), _ptr(cell_pos), _ptr(cell_seq), _ptr(tok_pos), _ptr(tok_seq), _ptr(tok_cell), float(rope_base),
                                                    int(n_rot), int(bool(neox)), float(scale), int(mode), _ptr(att), _ptr(blk)), "op_attn_batch_step")
        return att, kc, vc, blk

    def kv_store(self, form: int, q, k, v, n_head: int, n_head_kv: int, hd: int, type_k: int, k_rows, type_v: int, v_rows, tok_pos, tok_cell, rope_base: float,
                 n_rot=None, neox: bool = False, freq_scale: float = 1.0, freq_factors=None, q_norm=None, k_norm=None, eps: float = 0.0):
        """The K / V cache write of a batch on its own (mi355_op_kv_store; form 0 / 1: the generic kernel without / with the cos / sin table, 2: the vectorised
        prompt store, 3: the small-batch decode store, q may be None).  k_rows / v_rows: the whole cache before the launch, [n_cells][row bytes]; returns
        (q rotated [T][H * D] or None, the whole K cache after the launch, the whole V cache).  The inputs are not modified."""
        tok_pos = np.ascontiguousarray(tok_pos, np.int32).reshape(-1)
        tok_cell = np.ascontiguousarray(tok_cell, np.int32).reshape(-1)
        T = tok_pos.size
        qo = None if q is None else np.array(q, np.float32, copy=True).reshape(T, n_head * hd)
        k = np.ascontiguousarray(k, np.float32).reshape(T, n_head_kv * hd); v = np.ascontiguousarray(v, np.float32).reshape(T, n_head_kv * hd)
        kc = np.array(k_rows, order="C", copy=True).view(np.uint8); vc = np.array(v_rows, order="C", copy=True).view(np.uint8)
        assert tok_cell.size == T and kc.ndim == 2 and vc.ndim == 2 and kc.shape[0] == vc.shape[0]
        ff, qn, kn = (None if a is None else np.ascontiguousarray(a, np.float32) for a in (freq_factors, q_norm, k_norm))
        self._chk(self.lib.mi355_op_kv_store(int(form), _ptr(qo), _ptr(k), _ptr(v), T, n_head, n_head_kv, hd, int(n_rot or hd), int(bool(neox)), type_k, type_v,
                                             kc.shape[0], _ptr(tok_pos), _ptr(tok_cell), float(rope_base), float(freq_scale), _ptr(ff), _ptr(qn), _ptr(kn),
                                             float(eps), _ptr(kc), _ptr(vc)), "op_kv_store")
        return qo, kc, vc

    def k_shift(self, type_k: int, n_head_kv: int, hd: int, k_rows, delta, rope_base: float, n_rot=None, neox: bool = False, freq_scale: float = 1.0,
                freq_factors=None, ext_factor: float = 0.0, attn_factor: float = 1.0, corr_lo: float = 0.0, corr_hi: float = 0.0) -> np.ndarray:
        """One K-shift launch over a whole K cache (mi355_op_k_shift): k_rows [n_cells][row bytes], delta [n_cells]; returns the cache after the launch."""
        delta = np.ascontiguousarray(delta, np.int32).reshape(-1)
        kc = np.array(k_rows, order="C", copy=True).view(np.uint8)
        assert kc.ndim == 2 and kc.shape[0] == delta.size
        ff = None if freq_factors is None else np.ascontiguousarray(freq_factors, np.float32)
        self._chk(self.lib.mi355_op_k_shift(type_k, n_head_kv, hd, int(n_rot or hd), int(bool(neox)), delta.size, _ptr(delta), float(rope_base), float(freq_scale),
                                            _ptr(ff), float(ext_factor), float(attn_factor), float(corr_lo), float(corr_hi), _ptr(kc)), "op_k_shift")
        return kc

    @staticmethod
    def _layer_ptrs(layers):
        arr = (C.c_void_p * len(layers))(*[a.ctypes.data for a in layers])
        return arr

    def kv_state_pack(self, type_k: int, type_v: int, n_head_kv: int, hd: int, k_layers, v_layers, cells) -> np.ndarray:
        """The gather kernel of a sequence's state on its own (mi355_op_kv_state_pack): k_layers / v_layers hold one [n_cells][row bytes] cache per layer;
        returns, per layer, the K rows of the listed cells in list order and then their V rows, as one uint8 array."""
        cells = np.ascontiguousarray(cells, np.int32).reshape(-1)
        kl = [np.ascontiguousarray(a).view(np.uint8) for a in k_layers]; vl = [np.ascontiguousarray(a).view(np.uint8) for a in v_layers]
        assert len(kl) == len(vl) and all(a.ndim == 2 and a.shape[0] == kl[0].shape[0] for a in kl + vl)
        out = np.zeros(sum(a.shape[1] for a in kl + vl) * cells.size, np.uint8)
        self._chk(self.lib.mi355_op_kv_state_pack(type_k, type_v, len(kl), n_head_kv, hd, kl[0].shape[0], self._layer_ptrs(kl), self._layer_ptrs(vl), _ptr(cells),
                                                  cells.size, _ptr(out)), "op_kv_state_pack")
        return out

    def kv_state_unpack(self, type_k: int, type_v: int, n_head_kv: int, hd: int, k_layers, v_layers, cells, rows):
        """The scatter kernel (mi355_op_kv_state_unpack): `rows` (the layout kv_state_pack returns) written into the listed cells of the given caches; returns
        (K caches, V caches) after the launch, one array per layer.  The inputs are not modified."""
        cells = np.ascontiguousarray(cells, np.int32).reshape(-1)
        rows = np.ascontiguousarray(rows, np.uint8).reshape(-1)
        kl = [np.array(a, order="C", copy=True).view(np.uint8) for a in k_layers]; vl = [np.array(a, order="C", copy=True).view(np.uint8) for a in v_layers]
        assert len(kl) == len(vl) and all(a.ndim == 2 and a.shape[0] == kl[0].shape[0] for a in kl + vl)
        assert rows.size == sum(a.shape[1] for a in kl + vl) * cells.size
        self._chk(self.lib.mi355_op_kv_state_unpack(type_k, type_v, len(kl), n_head_kv, hd, kl[0].shape[0], _ptr(rows), _ptr(cells), cells.size,
                                                    self._layer_ptrs(kl), self._layer_ptrs(vl)), "op_kv_state_unpack")
        return kl, vl

    def hbm_read_gbps(self, nbytes: int = 1 << 30, iters: int = 10) -> float:
        return float(self.lib.mi355_bench_hbm_read(nbytes, iters))


def gloo_exchange(group=None):
    """The host exchange of mi355_tp_set_host_exchange over a torch.distributed (gloo) group: op 0 sums the buffer in
    place over the ranks, op 1 gathers `n` floats per rank (the caller's part already at buf + rank * n)."""
    import torch
    import torch.distributed as dist

    def fn(_user, buf, n, op):
        try:
            world, rank = dist.get_world_size(group), dist.get_rank(group)
            total = n if op == 0 else n * world
            t = torch.from_numpy(np.ctypeslib.as_array(buf, shape=(total,)))
            if op == 0:
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            else:
                parts = [torch.empty(n, dtype=torch.float32) for _ in range(world)]
                dist.all_gather(parts, t[rank * n:(rank + 1) * n].clone(), group=group)
                for r in range(world):
                    t[r * n:(r + 1) * n] = parts[r]
            return 0
        except Exception:   # noqa: BLE001 - a Python exception must not unwind through the C caller
            import traceback
            traceback.print_exc()
            return 1
    return fn


_tp_keepalive = []


def tp_p2p_enable(rank: int, size: int, device: int, max_floats: int, group=None, prompt_floats: int = 0):
    """One-shot peer-to-peer all-reduce for messages of up to max_floats floats (mi355_tp_p2p_*): every rank exports its exchange buffer, the 64-byte
    IPC handles are all-gathered over torch.distributed, every rank maps its peers' buffers.  prompt_floats > max_floats: messages up to that size
    take the reduce-scatter + all-gather kernel (mi355_tp_p2p_local_handle2)."""
    import torch
    import torch.distributed as dist
    lib = load_library()
    hb = (C.c_uint8 * 64)()
    if lib.mi355_tp_p2p_local_handle2(hb, 64, max_floats, prompt_floats) != 64:
        raise MI355Error(f"mi355_tp_p2p_local_handle2 failed: {_err(lib)}")
    backend = dist.get_backend(group)
    dev = torch.device("cuda", device) if backend == "nccl" else torch.device("cpu")
    mine = torch.tensor(list(bytes(hb)), dtype=torch.uint8, device=dev)
    parts = [torch.zeros(64, dtype=torch.uint8, device=dev) for _ in range(size)]
    dist.all_gather(parts, mine, group=group)
    allh = (C.c_uint8 * (64 * size))(*[int(v) for p_ in parts for v in p_.cpu().tolist()])
    if lib.mi355_tp_p2p_enable(allh, 64 * size) != 0:
        raise MI355Error(f"mi355_tp_p2p_enable failed: {_err(lib)}")


def tp_p2p_exchanges() -> int:
    return int(load_library().mi355_tp_p2p_exchanges())


def tp_p2p_prompt_exchanges() -> int:
    return int(load_library().mi355_tp_p2p_prompt_exchanges())


def tp_init(rank: int, size: int, device: int = 0, transport: str = "rccl", group=None, p2p_floats: int = 0, p2p_prompt_floats: int = 0):
    """Forms the process's row-split group (include/mi355_llama.h, mi355_tp_*).  transport "rccl": rank 0 makes the RCCL
    id, torch.distributed (any backend) carries it to the others, every rank calls mi355_tp_init on its device.
    transport "host": the exchange goes through gloo_exchange(group) (ranks sharing one GPU; validation only).
    p2p_floats > 0: all-reduces of up to that many floats (the decode steps' exchanges) take the one-shot peer-to-peer kernel;
    p2p_prompt_floats > p2p_floats: larger ones up to that size (prompt batches) the reduce-scatter + all-gather kernel."""
    lib = load_library()
    if transport == "host":
        cb = TP_HOST_EXCHANGE(gloo_exchange(group))
        _tp_keepalive.append(cb)
        if lib.mi355_tp_set_host_exchange(C.cast(cb, C.c_void_p), None, rank, size) != 0:
            raise MI355Error(f"mi355_tp_set_host_exchange failed: {_err(lib)}")
        if p2p_floats > 0 and size > 1:
            tp_p2p_enable(rank, size, device, p2p_floats, group, p2p_prompt_floats)
        return
    buf = (C.c_uint8 * TP_ID_BYTES)()
    if size > 1:
        import torch
        import torch.distributed as dist
        if rank == 0 and lib.mi355_tp_unique_id(buf, TP_ID_BYTES) != TP_ID_BYTES:
            raise MI355Error(f"mi355_tp_unique_id failed: {_err(lib)}")
        t = torch.tensor(list(bytes(buf)), dtype=torch.uint8)
        backend = dist.get_backend(group)
        dev = torch.device("cuda", device) if backend == "nccl" else torch.device("cpu")
        t = t.to(dev)
        dist.broadcast(t, src=0, group=group)
        buf = (C.c_uint8 * TP_ID_BYTES)(*t.cpu().tolist())
    elif lib.mi355_tp_unique_id(buf, TP_ID_BYTES) != TP_ID_BYTES:
        raise MI355Error(f"mi355_tp_unique_id failed: {_err(lib)}")
    if lib.mi355_tp_init(device, rank, size, buf, TP_ID_BYTES) != 0:
        raise MI355Error(f"mi355_tp_init failed: {_err(lib)}")
    if p2p_floats > 0 and size > 1:
        tp_p2p_enable(rank, size, device, p2p_floats, group, p2p_prompt_floats)


def tp_shutdown():
    load_library().mi355_tp_shutdown()
    _tp_keepalive.clear()


class Clip:
    """The image side of a LLaVA request (clip_model_load / clip_image_load_from_bytes / clip_image_preprocess / clip_image_encode)."""

    def __init__(self, path: str, main_gpu: int = 0):
        self.lib = load_library()
        self.h = self.lib.mi355_clip_model_load(path.encode(), main_gpu)
        if not self.h:
            raise MI355Error(f"mi355_clip_model_load({path}) failed: {_err(self.lib)}")
        self.n_embd = self.lib.mi355_clip_n_mmproj_embd(self.h)
        self.n_patches = self.lib.mi355_clip_n_patches(self.h)
        self.image_size = self.lib.mi355_clip_image_size(self.h)
        self.max_image_rows = self.lib.mi355_clip_max_image_rows(self.h)

    def load_image(self, data: bytes) -> np.ndarray:
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        nx, ny = C.c_int32(0), C.c_int32(0)
        if self.lib.mi355_clip_image_load_from_bytes(buf, len(data), C.byref(nx), C.byref(ny), None, 0) != 0:
            raise MI355Error(f"image: {_err(self.lib)}")
        rgb = np.empty((ny.value, nx.value, 3), np.uint8)
        if self.lib.mi355_clip_image_load_from_bytes(buf, len(data), C.byref(nx), C.byref(ny), rgb.ctypes.data, rgb.nbytes) != 0:
            raise MI355Error(f"image: {_err(self.lib)}")
        return rgb

    def preprocess(self, rgb: np.ndarray) -> np.ndarray:
        rgb = np.ascontiguousarray(rgb, np.uint8)
        ny, nx, _ = rgb.shape
        out = np.empty((3, self.image_size, self.image_size), np.float32)
        if self.lib.mi355_clip_image_preprocess(self.h, rgb.ctypes.data, nx, ny, out.ctypes.data) != 0:
            raise MI355Error(f"preprocess: {_err(self.lib)}")
        return out

    def preprocess_grid(self, rgb: np.ndarray):
        """Every image the encoder sees for one picture (LLaVA-1.6: overview + tiles): ([n, 3, S, S], grid_w, grid_h)."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        ny, nx, _ = rgb.shape
        cap = self.max_image_rows // self.n_patches
        out = np.empty((cap, 3, self.image_size, self.image_size), np.float32)
        gw, gh = C.c_int32(0), C.c_int32(0)
        n = self.lib.mi355_clip_image_preprocess_grid(self.h, rgb.ctypes.data, nx, ny, out.ctypes.data, out.size, C.byref(gw), C.byref(gh))
        if n < 0:
            raise MI355Error(f"preprocess_grid: {_err(self.lib)}")
        return out[:n], gw.value, gh.value

    def encode(self, img: np.ndarray) -> np.ndarray:
        img = np.ascontiguousarray(img, np.float32)
        out = np.empty((self.n_patches, self.n_embd), np.float32)
        if self.lib.mi355_clip_image_encode(self.h, img.ctypes.data, out.ctypes.data) != 0:
            raise MI355Error(f"encode: {_err(self.lib)}")
        return out

    def embed_bytes(self, data: bytes) -> np.ndarray:
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        out = np.empty((self.max_image_rows, self.n_embd), np.float32)
        n = self.lib.mi355_llava_image_embed_from_bytes(self.h, buf, len(data), out.ctypes.data, out.size)
        if n < 0:
            raise MI355Error(f"llava_image_embed: {_err(self.lib)}")
        return out[:n]

    def close(self):
        if self.h:
            self.lib.mi355_clip_free(self.h)
            self.h = None


class Model:
    def __init__(self, path: str, n_gpu_layers: int = 300, main_gpu: int = 0, prefill_planes: int = -1, tp_rank: int = 0, tp_size: int = 1):
        self.lib = load_library()
        mp = self.lib.mi355_model_default_params()
        mp.n_gpu_layers = n_gpu_layers
        mp.main_gpu = main_gpu
        mp.prefill_planes = prefill_planes
        mp.tp_rank, mp.tp_size = tp_rank, tp_size
        self.h = self.lib.mi355_model_load_from_file(path.encode(), mp)
        if not self.h:
            raise MI355Error(f"mi355_model_load_from_file({path}) failed: {_err(self.lib)}")
        L = self.lib
        self.n_vocab = L.mi355_model_n_vocab(self.h)
        self.n_embd = L.mi355_model_n_embd(self.h)
        self.n_layer = L.mi355_model_n_layer(self.h)
        self.n_head = L.mi355_model_n_head(self.h)
        self.n_head_kv = L.mi355_model_n_head_kv(self.h)
        self.bytes_per_token = L.mi355_model_bytes_per_token(self.h)
        self.planes_bytes = L.mi355_model_planes_bytes(self.h)
        self.size = L.mi355_model_size(self.h)
        self.vram = L.mi355_model_other_buffer(self.h)
        self.ram = L.mi355_model_cpu_buffer(self.h)
        self.desc = L.mi355_model_desc(self.h).decode()

    def meta(self, key: str):
        buf = C.create_string_buffer(512)
        if self.lib.mi355_model_meta_str(self.h, key.encode(), buf, 512):
            return buf.value.decode()
        return None

    def tokenize(self, text: str, add_special: bool = True, parse_special: bool = False) -> list[int]:
        raw = text.encode()
        cap = len(raw) + 8
        out = (C.c_int32 * cap)()
        n = self.lib.mi355_tokenize(self.h, raw, len(raw), out, cap, int(add_special), int(parse_special))
        if n < 0:
            raise MI355Error(f"mi355_tokenize failed: {_err(self.lib)}")
        return list(out[:n])

    def token_to_piece(self, tok: int, special: bool = True) -> bytes:
        buf = C.create_string_buffer(256)
        n = self.lib.mi355_token_to_piece(self.h, tok, buf, 256, int(special))
        if n < 0:
            raise MI355Error(f"mi355_token_to_piece failed: {_err(self.lib)}")
        return buf.raw[:n]

    def close(self):
        if self.h:
            self.lib.mi355_model_free(self.h)
            self.h = None


class LoraAdapter:
    """A LoRA adapter GGUF file loaded onto a model (mi355_adapter_lora_init); set on a context with Context.set_adapter_lora."""

    def __init__(self, model: Model, path: str):
        self.lib = model.lib
        self.model = model
        self.h = self.lib.mi355_adapter_lora_init(model.h, path.encode())
        if not self.h:
            raise MI355Error(f"mi355_adapter_lora_init({path}) failed: {_err(self.lib)}")
        self.alpha = float(self.lib.mi355_adapter_lora_alpha(self.h))
        self.n_pairs = int(self.lib.mi355_adapter_lora_n_pairs(self.h))

    def close(self):
        """Free the device copy; no context may still have the adapter set."""
        if self.h:
            self.lib.mi355_adapter_lora_free(self.h)
            self.h = None


class Context:
    def __init__(self, model: Model, n_ctx: int = 512, n_batch: int = 2048, n_ubatch: int = 512, n_seq_max: int = 1,
                 type_k: int = F16, type_v: int = F16, flash_attn: bool = True, use_graphs: bool = True,
                 logits_to_host: bool = True):
        self.lib = model.lib
        self.model = model
        cp = self.lib.mi355_context_default_params()
        cp.n_ctx, cp.n_batch, cp.n_ubatch, cp.n_seq_max = n_ctx, n_batch, n_ubatch, n_seq_max
        cp.type_k, cp.type_v, cp.flash_attn, cp.use_graphs = type_k, type_v, int(flash_attn), int(use_graphs)
        cp.logits_to_host = int(logits_to_host)
        self.h = self.lib.mi355_context_new(model.h, cp)
        if not self.h:
            raise MI355Error(f"mi355_context_new failed: {_err(self.lib)}")
        self.n_ctx = n_ctx
        self._batch_cap = 0
        self._b = None

    def _batch(self, n: int) -> Batch:
        if n > self._batch_cap:
            if self._b is not None:
                self.lib.mi355_batch_free(self._b)
            self._batch_cap = max(n, 64)
            self._b = self.lib.mi355_batch_init(self._batch_cap, 0, 1)
        return self._b

    def decode(self, tokens, pos, seq=None, logits=None) -> int:
        """llama_decode on one batch; logits=None flags only the last token."""
        tokens = np.asarray(tokens, np.int32).reshape(-1)
        pos = np.asarray(pos, np.int32).reshape(-1)
        n = tokens.size
        b = self._batch(n)
        b.n_tokens = n
        C.memmove(b.token, tokens.ctypes.data, 4 * n)
        C.memmove(b.pos, pos.ctypes.data, 4 * n)
        for i in range(n):
            b.n_seq_id[i] = 1
            b.seq_id[i][0] = 0 if seq is None else int(seq[i] if np.ndim(seq) else seq)
            b.logits[i] = (1 if i == n - 1 else 0) if logits is None else int(bool(logits[i]))
        rc = self.lib.mi355_decode(self.h, b)
        if rc < 0:
            raise MI355Error(f"mi355_decode failed ({rc}): {_err(self.lib)}")
        return rc

    def decode_embd(self, embd, pos, seq=None, logits=None) -> int:
        """llama_decode on a batch of embedding rows [n][n_embd] (llama_batch.embd: how image embeddings reach the model)."""
        embd = np.ascontiguousarray(embd, np.float32)
        pos = np.asarray(pos, np.int32).reshape(-1)
        n = pos.size
        if embd.shape != (n, self.model.n_embd):
            raise ValueError(f"embd must be [{n}][{self.model.n_embd}]")
        b = self.lib.mi355_batch_init(n, self.model.n_embd, 1)
        try:
            b.n_tokens = n
            C.memmove(b.embd, embd.ctypes.data, embd.nbytes)
            C.memmove(b.pos, pos.ctypes.data, 4 * n)
            for i in range(n):
                b.n_seq_id[i] = 1
                b.seq_id[i][0] = 0 if seq is None else int(seq[i] if np.ndim(seq) else seq)
                b.logits[i] = (1 if i == n - 1 else 0) if logits is None else int(bool(logits[i]))
            rc = self.lib.mi355_decode(self.h, b)
        finally:
            self.lib.mi355_batch_free(b)
        if rc < 0:
            raise MI355Error(f"mi355_decode failed ({rc}): {_err(self.lib)}")
        return rc

    def greedy_steps(self, first: int, pos0: int, n: int, seq: int = 0) -> np.ndarray:
        """n greedy single-token steps (decode, logits row host-visible, arg-max fed back) in one C call; returns the n tokens"""
        out = np.empty(n, np.int32)
        done = self.lib.mi355_greedy_steps(self.h, int(first), int(pos0), int(seq), int(n), out.ctypes.data)
        if done != n:
            raise MI355Error(f"mi355_greedy_steps stopped after {done} of {n}: {_err(self.lib)}")
        return out

    def logits(self, i: int = -1) -> np.ndarray:
        p = self.lib.mi355_get_logits_ith(self.h, i)
        if not p:
            raise MI355Error(f"no logits for that batch row: {_err(self.lib)}")
        return np.ctypeslib.as_array(p, shape=(self.model.n_vocab,)).copy()

    def logits_ready(self, i: int = -1) -> None:
        """Block until the logits row is host-visible (no numpy copy)."""
        if not self.lib.mi355_get_logits_ith(self.h, i):
            raise MI355Error(f"no logits for that batch row: {_err(self.lib)}")

    def set_adapter_lora(self, adapter: LoraAdapter, scale: float = 1.0) -> None:
        """llama_set_adapter_lora: apply the adapter from the next step on (set again: a new scale)."""
        if self.lib.mi355_set_adapter_lora(self.h, adapter.h, float(scale)) != 0:
            raise MI355Error(f"mi355_set_adapter_lora failed: {_err(self.lib)}")

    def rm_adapter_lora(self, adapter: LoraAdapter) -> bool:
        return self.lib.mi355_rm_adapter_lora(self.h, adapter.h) == 0

    def clear_adapter_lora(self) -> None:
        self.lib.mi355_clear_adapter_lora(self.h)

    def apply_cvec(self, data, il_start: int, il_end: int, n_embd: int | None = None) -> None:
        """llama_apply_adapter_cvec: data = the vectors of layers 1, 2, ... back to back ([n][n_embd] or flat); layers il_start .. il_end take theirs from the
        next step on.  None clears."""
        if data is None:
            return self.clear_cvec()
        d = np.ascontiguousarray(data, np.float32)
        ne = int(n_embd if n_embd is not None else (d.shape[-1] if d.ndim == 2 else self.model.n_embd))
        if self.lib.mi355_apply_adapter_cvec(self.h, _ptr(d), d.size, ne, int(il_start), int(il_end)) != 0:
            raise MI355Error(f"mi355_apply_adapter_cvec failed: {_err(self.lib)}")

    def clear_cvec(self) -> None:
        if self.lib.mi355_apply_adapter_cvec(self.h, None, 0, 0, 0, 0) != 0:
            raise MI355Error(f"mi355_apply_adapter_cvec (clear) failed: {_err(self.lib)}")

    def set_embeddings(self, on: bool = True) -> None:
        self.lib.mi355_set_embeddings(self.h, int(on))

    def embeddings(self, i: int = -1) -> np.ndarray:
        p = self.lib.mi355_get_embeddings_ith(self.h, i)
        if not p:
            raise MI355Error("no embeddings for that row")
        return np.ctypeslib.as_array(p, shape=(self.model.n_embd,)).copy()

    def argmax(self, i: int = -1) -> int:
        return int(self.lib.mi355_get_argmax_ith(self.h, i))

    def argmax_prob(self, i: int = -1):
        """(arg-max token, its softmax probability over the whole vocabulary) of batch row i, from the device logits (mi355_get_argmax_prob_ith)."""
        p = C.c_float(0.0)
        t = int(self.lib.mi355_get_argmax_prob_ith(self.h, i, C.byref(p)))
        if t < 0:
            raise MI355Error(f"mi355_get_argmax_prob_ith failed: {_err(self.lib)}")
        return t, float(p.value)

    def spec_verify(self, group_start, draft):
        """Greedy acceptance over the last decode's rows (mi355_spec_verify): group g owns batch rows group_start[g] .. group_start[g + 1] - 1, all flagged; draft
        runs parallel to them (a group's last entry is ignored).  Returns (ids int32 [R], n_accept int32 [G])."""
        gs = np.ascontiguousarray(group_start, np.int32).reshape(-1)
        draft = np.ascontiguousarray(draft, np.int32).reshape(-1)
        G = gs.size - 1
        R = int(gs[-1] - gs[0]) if G >= 1 else 0
        if G < 1 or R < 1 or draft.size != R:
            raise ValueError("spec_verify: group_start [G + 1] and draft [R] with R = group_start[G] - group_start[0]")
        ids = np.full(R, -1, np.int32); acc = np.full(G, -1, np.int32)
        r = self.lib.mi355_spec_verify(self.h, G, _ptr(gs), _ptr(draft), _ptr(ids), _ptr(acc))
        if r != R:
            raise MI355Error(f"mi355_spec_verify failed: {_err(self.lib)}")
        return ids, acc

    def token_logprobs(self, batch_rows, targets):
        """(log-probability f32 [n], rank int32 [n]) of targets[r] in row batch_rows[r] of the last decode, over the whole vocabulary, from the device logits
        (mi355_get_token_logprobs).  rank 0: the target is the row's arg-max.  A dead row gives NaN and -1."""
        rows = np.ascontiguousarray(batch_rows, np.int32).reshape(-1)
        tg = np.ascontiguousarray(targets, np.int32).reshape(-1)
        if rows.size < 1 or rows.size != tg.size:
            raise ValueError("token_logprobs: batch_rows [n] and targets [n], n >= 1")
        lp = np.zeros(rows.size, np.float32); rank = np.zeros(rows.size, np.int32)
        if self.lib.mi355_get_token_logprobs(self.h, rows.size, _ptr(rows), _ptr(tg), _ptr(lp), _ptr(rank)) != rows.size:
            raise MI355Error(f"mi355_get_token_logprobs failed: {_err(self.lib)}")
        return lp, rank

    def logits_kl(self, base: "Context", rows_base, rows):
        """(KL(base || self) f32 [n], same_top int32 [n]) of row rows_base[r] of base's last decode against row rows[r] of this context's (mi355_logits_kl)."""
        rb = np.ascontiguousarray(rows_base, np.int32).reshape(-1)
        rs = np.ascontiguousarray(rows, np.int32).reshape(-1)
        if rb.size < 1 or rb.size != rs.size:
            raise ValueError("logits_kl: rows_base [n] and rows [n], n >= 1")
        kl = np.zeros(rb.size, np.float32); top = np.zeros(rb.size, np.int32)
        if self.lib.mi355_logits_kl(self.h, base.h, rb.size, _ptr(rb), _ptr(rs), _ptr(kl), _ptr(top)) != rb.size:
            raise MI355Error(f"mi355_logits_kl failed: {_err(self.lib)}")
        return kl, top

    def perplexity(self, tokens, n_chunk: int, bos: int = -1, seq: int = 0, base: "Context" = None, callback=None) -> dict:
        """The llama-perplexity procedure over `tokens` in chunks of n_chunk (mi355_perplexity): a dict of the mi355_ppl_stats fields plus "logprobs" (f32, one per
        scored position, NaN for a dead row), with a base context also "kls", and the derived "ppl" / "ppl_base" / "mean_kl".  callback(stats dict) runs after
        every chunk; a true return stops the run."""
        tk = np.ascontiguousarray(tokens, np.int32).reshape(-1)
        n_chunk = int(n_chunk)
        per = max(0, n_chunk - 1 - n_chunk // 2)
        n_out = max(1, (tk.size // max(n_chunk, 1)) * per)
        lp = np.full(n_out, np.nan, np.float32)
        kl = np.full(n_out, np.nan, np.float32) if base is not None else None
        st = PplStats()

        def as_dict(s):
            return {name: getattr(s, name) for name, _ in PplStats._fields_}

        raised = []

        def tramp(sp, _user):
            try:
                return 1 if callback(as_dict(sp.contents)) else 0
            except BaseException as ex:          # (an exception must not cross the C frames)
                raised.append(ex)
                return 1

        cb = PPL_CALLBACK(tramp) if callback is not None else None
        r = self.lib.mi355_perplexity(self.h, base.h if base is not None else None, _ptr(tk), tk.size, n_chunk, int(bos), int(seq), _ptr(lp),
                                      _ptr(kl) if kl is not None else None, C.cast(cb, C.c_void_p) if cb is not None else None, None, C.byref(st))
        if raised:
            raise raised[0]
        if r != 0:
            raise MI355Error(f"mi355_perplexity failed: {_err(self.lib)}")
        out = as_dict(st)
        n_scored = int(st.n_chunks) * per
        out["logprobs"] = lp[:n_scored]
        if kl is not None:
            out["kls"] = kl[:n_scored]
        if st.count > 0:
            out["ppl"] = float(np.exp(st.nll / st.count))
            if base is not None:
                out["ppl_base"] = float(np.exp(st.nll_base / st.count))
                out["mean_kl"] = st.kl / st.count
        return out

    def imatrix_begin(self, process_output: bool = False) -> None:
        """Start collecting the importance matrix on every decode of this context (mi355_imatrix_begin)."""
        if self.lib.mi355_imatrix_begin(self.h, int(bool(process_output))) != 0:
            raise MI355Error(f"mi355_imatrix_begin failed: {_err(self.lib)}")

    def imatrix_end(self) -> None:
        """Stop collecting and free the accumulators; the steps are again what they were before imatrix_begin."""
        if self.lib.mi355_imatrix_end(self.h) != 0:
            raise MI355Error(f"mi355_imatrix_end failed: {_err(self.lib)}")

    def imatrix_clear(self) -> None:
        """Zero the sums and counts; collection stays on."""
        if self.lib.mi355_imatrix_clear(self.h) != 0:
            raise MI355Error(f"mi355_imatrix_clear failed: {_err(self.lib)}")

    def imatrix_entries(self) -> dict:
        """{tensor name: (sum2 f32 [n_mat][ne0], counts int32 [n_mat])} of everything collected since imatrix_begin / imatrix_clear, in layer order."""
        out = {}
        buf = C.create_string_buffer(256)
        for i in range(int(self.lib.mi355_imatrix_n_entries(self.h))):
            ne0, n_mat = C.c_int32(0), C.c_int32(0)
            if self.lib.mi355_imatrix_entry(self.h, i, C.cast(buf, C.c_void_p), 256, C.cast(C.byref(ne0), C.c_void_p), C.cast(C.byref(n_mat), C.c_void_p)) < 0:
                raise MI355Error(f"mi355_imatrix_entry failed: {_err(self.lib)}")
            sum2 = np.zeros((n_mat.value, ne0.value), np.float32)
            counts = np.zeros(n_mat.value, np.int32)
            if self.lib.mi355_imatrix_get(self.h, i, _ptr(sum2), _ptr(counts)) != 0:
                raise MI355Error(f"mi355_imatrix_get failed: {_err(self.lib)}")
            out[buf.value.decode()] = (sum2, counts)
        return out

    def speculative_steps(self, draft_ctx: "Context", first: int, pos0: int, n: int, n_max: int = 16, n_min: int = 0, p_min: float = 0.75, seq: int = 0):
        """n greedy tokens with draft_ctx's model drafting up to n_max per round (mi355_speculative_steps); both contexts hold `seq` over [0, pos0).
        Returns (tokens int32 [n], stats int64 [4]: rounds, drafted, accepted, plain steps)."""
        out = np.empty(n, np.int32); stats = np.zeros(4, np.int64)
        done = self.lib.mi355_speculative_steps(self.h, draft_ctx.h, int(first), int(pos0), int(seq), int(n), int(n_max), int(n_min), float(p_min),
                                                out.ctypes.data, stats.ctypes.data)
        if done != n:
            raise MI355Error(f"mi355_speculative_steps stopped after {done} of {n}: {_err(self.lib)}")
        return out, stats

    def mega_steps(self) -> int:
        """Single-token steps that ran as one whole-step launch (diagnosis)."""
        return int(self.lib.mi355_debug_mega_steps(self.h))

    def topk(self, k: int, i: int = -1, adj_tok=(), adj_bias=(), adj_count=(), repeat: float = 1.0, freq: float = 0.0, present: float = 0.0):
        """Device-side sampling front end: (tokens [k] int32, logits [k] f32) of row i after the adjustments, best first."""
        at = np.ascontiguousarray(adj_tok, np.int32); ab = np.ascontiguousarray(adj_bias, np.float32); ac = np.ascontiguousarray(adj_count, np.int32)
        toks = np.zeros(k, np.int32); lg = np.zeros(k, np.float32)
        r = self.lib.mi355_get_topk_ith(self.h, i, k, at.size, _ptr(at), _ptr(ab), _ptr(ac), repeat, freq, present, _ptr(toks), _ptr(lg))
        if r != k:
            raise MI355Error(f"mi355_get_topk_ith failed: {_err(self.lib)}")
        return toks, lg

    def fused_skipped_steps(self) -> int:
        return int(self.lib.mi355_debug_fused_skipped_steps(self.h))

    def qkv_attn_launches(self) -> int:
        return int(self.lib.mi355_debug_qkv_attn_launches(self.h))

    def engine_steps(self) -> int:
        """Single-token steps that ran through the layer engine (one persistent launch per layer; diagnosis)."""
        return int(self.lib.mi355_debug_engine_steps(self.h))

    def synchronize(self):
        self.lib.mi355_synchronize(self.h)

    def kv_clear(self):
        self.lib.mi355_kv_cache_clear(self.h)

    def kv_seq_rm(self, seq, p0, p1) -> bool:
        return bool(self.lib.mi355_kv_cache_seq_rm(self.h, seq, p0, p1))

    def kv_seq_cp(self, s, d, p0, p1):
        self.lib.mi355_kv_cache_seq_cp(self.h, s, d, p0, p1)

    def kv_seq_add(self, seq, p0, p1, delta):
        self.lib.mi355_kv_cache_seq_add(self.h, seq, p0, p1, delta)

    def state_seq_size(self, seq: int = 0) -> int:
        return int(self.lib.mi355_state_seq_get_size(self.h, int(seq)))

    def state_seq_get(self, seq: int = 0) -> bytes:
        """llama_state_seq_get_data: the sequence's cells as a blob (header, positions, per-layer K / V rows; a pending K-shift is applied first)."""
        buf = np.zeros(self.state_seq_size(seq), np.uint8)
        n = int(self.lib.mi355_state_seq_get_data(self.h, _ptr(buf), buf.size, int(seq)))
        if n == 0:
            raise MI355Error(f"mi355_state_seq_get_data refused: {_err(self.lib)}")
        return buf[:n].tobytes()

    def state_seq_set(self, seq: int, blob) -> int:
        """llama_state_seq_set_data: replaces what `seq` holds with the blob's cells; returns the bytes consumed, raises with the library's reason on a refusal."""
        buf = np.frombuffer(bytes(blob), np.uint8)
        n = int(self.lib.mi355_state_seq_set_data(self.h, buf.ctypes.data if buf.size else None, buf.size, int(seq)))
        if n == 0:
            raise MI355Error(f"mi355_state_seq_set_data refused: {_err(self.lib)}")
        return n

    def state_seq_save_file(self, path: str, seq: int, tokens) -> int:
        tokens = np.ascontiguousarray(tokens, np.int32).reshape(-1)
        n = int(self.lib.mi355_state_seq_save_file(self.h, os.fsencode(path), int(seq), _ptr(tokens), tokens.size))
        if n == 0:
            raise MI355Error(f"mi355_state_seq_save_file refused: {_err(self.lib)}")
        return n

    def state_seq_load_file(self, path: str, seq: int, max_tokens: int = 1 << 20) -> np.ndarray:
        """llama_state_seq_load_file: restores the file's sequence into `seq`; returns the tokens stored with it."""
        toks = np.zeros(max_tokens, np.int32)
        n_tok = C.c_size_t(0)
        n = int(self.lib.mi355_state_seq_load_file(self.h, os.fsencode(path), int(seq), _ptr(toks), toks.size, C.byref(n_tok)))
        if n == 0:
            raise MI355Error(f"mi355_state_seq_load_file refused: {_err(self.lib)}")
        return toks[:n_tok.value].copy()

    def state_seq_timing(self):
        """(pack ms, device-to-host copy ms, unpack ms) of the last state_seq_get / state_seq_set; the first call switches the timing on."""
        out = np.zeros(3, np.float32)
        self.lib.mi355_debug_state_seq_timing(self.h, _ptr(out))
        return tuple(float(x) for x in out)

    def kv_used(self) -> int:
        return int(self.lib.mi355_kv_cache_used_cells(self.h))

    def enable_taps(self, on: bool = True):
        self.lib.mi355_debug_enable_taps(self.h, int(on))

    def layer_out(self, il: int, n_tokens: int) -> np.ndarray:
        out = np.zeros((n_tokens, self.model.n_embd), np.float32)
        n = self.lib.mi355_debug_layer_out(self.h, il, _ptr(out), out.size)
        if n < 0:
            raise MI355Error("debug taps not enabled")
        return out[:n]

    def profile(self, on: bool = True):
        self.lib.mi355_profile_enable(self.h, int(on))

    def last_profile(self) -> dict:
        names = (_cp * 64)()
        us = (_f32 * 64)()
        n = self.lib.mi355_profile_last_decode(self.h, names, us, 64)
        return {names[i].decode(): float(us[i]) for i in range(n)}

    def force_moe_ids(self, ids: np.ndarray) -> None:
        """ids [n_layer][T][k]: the experts the NEXT decode call takes instead of its router's selection (test hook)."""
        ids = np.ascontiguousarray(ids, np.int32)
        rc = self.lib.mi355_debug_force_moe_ids(self.h, _ptr(ids), ids.shape[0], ids.shape[1], ids.shape[2])
        if rc != 0:
            raise MI355Error(f"mi355_debug_force_moe_ids failed ({rc}): {_err(self.lib)}")

    def weight_sweep_us(self, iters: int = 5):
        b = _u64(0)
        us = self.lib.mi355_bench_weight_sweep(self.h, iters, C.byref(b))
        return float(us), int(b.value)

    def weight_sweep(self, iters: int = 5):
        """(us per sweep, weight bytes per sweep, mat-vec launches per sweep) of the step's own weight-stream launches."""
        b, n = _u64(0), C.c_int32(0)
        us = self.lib.mi355_bench_weight_sweep2(self.h, iters, C.byref(b), C.byref(n))
        return float(us), int(b.value), int(n.value)

    def close(self):
        if self._b is not None:
            self.lib.mi355_batch_free(self._b)
            self._b = None
        if self.h:
            self.lib.mi355_context_free(self.h)
            self.h = None


class Engine:
    """ctypes view of mi355_engine_* — the reference's EngineI surface (base/cortex-common/enginei.h:13-74) with JSON text
    bodies.  Every call returns the list of (status, body) pairs the callback received; a streaming chat completion
    returns one pair per SSE chunk."""

    def __init__(self):
        import json
        import threading
        self._json, self._threading = json, threading
        self.lib = load_library()
        self.h = self.lib.mi355_engine_create()
        if not self.h:
            raise MI355Error(f"mi355_engine_create failed: {_err(self.lib)}")

    def _call(self, fn, body: dict, wait_done: bool = True, timeout: float = 120.0):
        out, done = [], self._threading.Event()

        def on(status, payload, _user):
            st, bd = self._json.loads(status.decode("utf-8", "replace")), self._json.loads(payload.decode("utf-8", "replace"))
            out.append((st, bd))
            if st.get("is_done", True) or st.get("has_error", False):
                done.set()

        cb = ENGINE_CB(on)
        fn(self.h, self._json.dumps(body).encode(), cb, None)
        if wait_done and not done.wait(timeout):
            raise MI355Error("engine call timed out")
        self._keep = cb   # the callback object must outlive the native call
        return out

    def load_model(self, **body):
        return self._call(self.lib.mi355_engine_load_model, body)[-1]

    def unload_model(self, **body):
        return self._call(self.lib.mi355_engine_unload_model, body)[-1]

    def get_model_status(self, **body):
        return self._call(self.lib.mi355_engine_get_model_status, body)[-1]

    def get_models(self):
        return self._call(self.lib.mi355_engine_get_models, {})[-1]

    def chat_completion(self, **body):
        return self._call(self.lib.mi355_engine_handle_chat_completion, body)

    def embedding(self, **body):
        return self._call(self.lib.mi355_engine_handle_embedding, body)[-1]

    def is_supported(self, feature: str) -> bool:
        return bool(self.lib.mi355_engine_is_supported(self.h, feature.encode()))

    def prompt_cache_stats(self, model_id: str) -> dict:
        """The counters of the model's host-RAM prompt cache (load key "cache_ram")."""
        out = (C.c_int64 * 6)()
        rc = self.lib.mi355_engine_prompt_cache_stats(self.h, model_id.encode(), out)
        if rc < 0:
            raise MI355Error(f"mi355_engine_prompt_cache_stats failed ({rc}): {_err(self.lib)}")
        return dict(zip(("entries", "bytes", "saves", "restores", "tokens_restored", "evictions"), (int(v) for v in out)))

    def spec_stats(self, model_id: str) -> dict:
        """The speculative-decoding counters of a model loaded with "model_draft"."""
        out = (C.c_int64 * 4)()
        rc = self.lib.mi355_engine_spec_stats(self.h, model_id.encode(), out)
        if rc < 0:
            raise MI355Error(f"mi355_engine_spec_stats failed ({rc}): {_err(self.lib)}")
        return dict(zip(("rounds", "drafted", "accepted", "plain_steps"), (int(v) for v in out)))

    def stop_inferencing(self, model_id: str) -> None:
        self.lib.mi355_engine_stop_inferencing(self.h, model_id.encode())

    def close(self):
        if self.h:
            self.lib.mi355_engine_destroy(self.h)
            self.h = None
