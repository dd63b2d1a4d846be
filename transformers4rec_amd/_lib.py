"""ctypes binding of libt4r_hip.so (C ABI declared in include/t4r_hip.h).

There is NO fallback: if the shared library is missing or a call fails the product path
raises.  Build with `python -m transformers4rec_amd.build` (or __graft_entry__.build()).
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# T4R_HIP_LIB selects another build of the same ABI (A/B timing of kernel variants on one box)
LIB_PATH = os.environ.get("T4R_HIP_LIB") or os.path.join(_HERE, "lib", "libt4r_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip.h")
SAMPLING_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_sampling.h")
FILTER_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_filter.h")
OPTIM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_optim.h")
PRETRAINED_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_pretrained.h")
ATTN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_attn.h")
ROWS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_rows.h")
ROWADAM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_rowadam.h")
CONTPROJ_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_contproj.h")
ROWCLIP_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_rowclip.h")
SEQTASK_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_seqtask.h")
RTD_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "t4r_hip_rtd.h")

_P, _I, _L, _F, _Q = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_ulonglong
_C = {"p": _P, "i": _I, "l": _L, "f": _F, "Q": _Q}

# name -> (restype, argtype codes).  Must match include/t4r_hip.h (tests/test_abi.py checks the
# symbol list against the header).
_SIGS = {
    "t4r_abi_version": ("i", ""),
    "t4r_last_error": ("s", ""),
    "t4r_ragged_max_len": ("i", "ppip"),
    "t4r_ragged_to_padded": ("i", "ppppiii"),
    "t4r_ragged_gather_to_padded": ("i", "pppp" + "p" + "iii"),
    "t4r_seq_features_fwd": ("i", "pippppppiiiiiiipppp"),
    "t4r_embedding_bwd": ("i", "pppp" + "liiilii"),
    "t4r_sort_ids_ws_bytes": ("l", "l"),
    "t4r_sort_ids": ("i", "pp" + "lli" + "ppp" + "l"),
    "t4r_sort_ids_multi_ws_bytes": ("l", "li"),
    "t4r_sort_ids_multi": ("i", "ppilpp" + "ppp" + "l"),
    "t4r_embedding_bwd_sorted_ws_floats": ("l", "li"),
    "t4r_embedding_bwd_sorted": ("i", "ppppp" + "liiili" + "p"),
    "t4r_embedding_bag_fwd": ("i", "pp" + "li" + "pp" + "llii" + "p" + "li" + "p"),
    "t4r_embedding_bag_bwd_rows": ("i", "pp" + "lii" + "p" + "llii" + "p"),
    "t4r_apply_mask_fwd": ("i", "ppppiiii"),
    "t4r_apply_mask_bwd": ("i", "ppppiiii" + "p"),
    "t4r_apply_mask_bwd_ws_floats": ("l", "iii"),
    "t4r_apply_mask_bwd_to": ("i", "pppppiiii" + "p"),
    "t4r_mul": ("i", "ppppl"),
    "t4r_soft_embedding_fwd": ("i", "pppppppp" + "liif"),
    "t4r_soft_embedding_bwd": ("i", "pppppppppppp" + "liiiif" + "p"),
    "t4r_soft_embedding_bwd_ws_floats": ("l", "lii"),
    "t4r_mask_targets": ("i", "ppiiil" + "ppp" + "fQQ" + "ppp"),
    "t4r_compact_labels": ("i", "pppiil" + "pppp"),
    "t4r_gather_rows": ("i", "ppppii"),
    "t4r_scatter_rows_add": ("i", "ppppii"),
    "t4r_scatter_rows_dense": ("i", "pppippli"),
    "t4r_last_positions": ("i", "ppiiiilp"),
    "t4r_gemm_f32": ("i", "piiiiif" + "plplpl" + "pipl" + "iii" + "lll" + "fQQ"),
    "t4r_gemm_wgrad_f32": ("i", "piii" + "plpl" + "pplp"),
    "t4r_gemm_wgrad_ws_floats": ("l", "iii"),
    "t4r_mha_fwd": ("i", "pppplplp" + "iiiii" + "fQQ" + "p"),
    "t4r_mha_bwd": ("i", "pppplpplppppl" + "iiiii" + "fQQ" + "p"),
    "t4r_add_pos_fwd": ("i", "ppppp" + "iii"),
    "t4r_add_pos_bwd": ("i", "ppp" + "iii"),
    "t4r_dropout_ctr_hi": ("Q", "Qii"),
    "t4r_dropout": ("i", "pppp" + "llfQQ"),
    "t4r_set_precision": ("v", "i"),
    "t4r_get_precision": ("i", ""),
    "t4r_gemm_softmax_grad_f32": ("i", "piiiif" + "plpppf" + "plpl" + "ii"),
    "t4r_set_tok_gemm_min_rows": ("v", "i"),
    "t4r_get_tok_gemm_min_rows": ("i", ""),
    "t4r_head_split_supported": ("i", "i"),
    "t4r_head_split_fwd_products": ("i", ""),
    "t4r_head_split_ws_bytes": ("l", "iii"),
    "t4r_head_split_prepare": ("i", "ppl" + "iii" + "p"),
    "t4r_head_split_fdx_supported": ("i", "i"),
    "t4r_head_split_logits_ce_dx": ("i", "pp" + "plpl" + "pl" + "pppp" + "plp" + "iii" + "ff" + "p"),
    "t4r_head_split_logits_ce_dx_amax": ("i", "pp" + "plpl" + "pl" + "pppp" + "plp" + "iii" + "ff" + "p" + "pi"),
    "t4r_head_note_dw_form": ("i", "p"),
    "t4r_head_split_logits": ("i", "ppplpl" + "iiif" + "p"),
    "t4r_head_split_logits_ce": ("i", "ppplpl" + "pppp" + "iiiff" + "p"),
    "t4r_head_split_dw": ("i", "ppplpppf" + "pl" + "iiiii" + "fi" + "p"),
    "t4r_head_split_dx": ("i", "ppplpppf" + "plpl" + "iiiii" + "fi" + "p"),
    "t4r_head_split_recompute_supported": ("i", "i"),
    "t4r_head_split_prepare_rc": ("i", "ppl" + "iii" + "p"),
    "t4r_head_split_ce": ("i", "ppplpppp" + "iiiff" + "p"),
    "t4r_head_split_dw_rc": ("i", "ppplpppf" + "pl" + "iiifi" + "p"),
    "t4r_head_split_dx_rc": ("i", "ppplplpppf" + "pl" + "iiifi" + "p"),
    "t4r_add_layernorm_fwd": ("i", "pppppppp" + "iif" + "fQQ"),
    "t4r_add_layernorm_bwd": ("i", "pppppppppppp" + "iii" + "fQQ"),
    "t4r_colreduce_ws_floats": ("l", "li"),
    "t4r_act_bwd_bias": ("i", "pppppp" + "lii" + "fQQ"),
    "t4r_colsum": ("i", "pppp" + "lil"),
    "t4r_session_lengths": ("i", "pp" + "iiii" + "p"),
    "t4r_xlnet_attn_fwd": ("i", "ppppppppp" + "iiii" + "ifQQ" + "p"),
    "t4r_xlnet_attn_bwd_ws_floats": ("l", "iiii"),
    "t4r_xlnet_attn_bwd": ("i", "p" * 17 + "iiii" + "ifQQ" + "p"),
    "t4r_xlnet_fused_supported": ("i", "i"),
    "t4r_xlnet_fused_products": ("i", ""),
    "t4r_xlnet_ff_bwd_part_floats": ("l", "li"),
    "t4r_xlnet_layer_planes_floats": ("l", "i"),
    "t4r_xlnet_layer_prepare": ("i", "ppip"),
    "t4r_xlnet_qkv_proj": ("i", "pppp" + "li"),
    "t4r_xlnet_kr_proj": ("i", "pppp" + "li"),
    "t4r_xlnet_oproj_ln": ("i", "p" + "ppppp" + "pppp" + "liff" + "QQ"),
    "t4r_xlnet_ln1_bwd_part_floats": ("l", "li"),
    "t4r_xlnet_ln1_bwd": ("i", "p" + "ppppppp" + "pppppp" + "lif" + "QQ"),
    "t4r_xlnet_dh": ("i", "pppp" + "li"),
    "t4r_xlnet_set_cu_budget": ("v", "i"),
    "t4r_xlnet_get_cu_budget": ("i", ""),
    "t4r_device_cus": ("i", ""),
    "t4r_experimental_build": ("i", ""),
    "t4r_xlnet_attn_block_supported": ("i", "iii"),
    "t4r_xlnet_attn_block_fwd": ("i", "ppppp" + "l" + "pppp" + "ppppppp" + "iiii" + "ffQQQ" + "p"),
    "t4r_xlnet_layer_ws_offsets": ("i", "iiiii" + "pp"),
    "t4r_xlnet_stack_prepare": ("i", "ppiip" + "plp"),
    "t4r_xlnet_stack_prepare_drop": ("i", "ppiip" + "plp" + "fQQlp"),
    "t4r_xlnet_layer_bwd_join": ("i", "p"),
    "t4r_xlnet_ff_planes_floats": ("l", "i"),
    "t4r_xlnet_ff_prepare": ("i", "ppppip"),
    "t4r_xlnet_ff_fwd": ("i", "p" + "pppppp" + "pppppp" + "iiff" + "QQQ"),
    "t4r_xlnet_ff_bwd": ("i", "p" + "pppppppp" + "pppppppp" + "iif" + "QQQ"),
    "t4r_xlnet_layer_ws_floats": ("l", "iiiii"),
    "t4r_xlnet_layer_bwd_ws_floats": ("l", "iiiii"),
    "t4r_xlnet_layer_fwd": ("i", "pppppp" + "iiiif" + "fQQi" + "pp"),
    "t4r_xlnet_layer_bwd": ("i", "ppppppppp" + "iiiif" + "fQQi" + "pp"),
    "t4r_softmax_ce_fwd": ("i", "pppppp" + "iilf"),
    "t4r_softmax_ce_bwd": ("i", "pppppp" + "iilf"),
    "t4r_linear_softmax_ce_chunk_floats": ("l", "ii"),
    "t4r_linear_softmax_ce_fwd": ("i", "pplpl" + "p" + "iiiffi" + "ppppp"),
    "t4r_linear_softmax_ce_bwd": ("i", "pplpl" + "ppp" + "iiiffi" + "pplpl"),
    "t4r_sampled_logits_fwd": ("i", "ppppppp" + "iiif" + "p"),
    "t4r_log_uniform_sample": ("i", "pp" + "ill" + "QQ"),
    "t4r_sampled_logits_bwd": ("i", "ppppppppp" + "iiif"),
    "t4r_sampled_logits_bwd_rows": ("i", "ppppppppp" + "iiif"),
    "t4r_topk": ("i", "pp" + "iili" + "pp"),
    "t4r_rank_of_target_f32": ("i", "p" + "iiif" + "pl" + "pl" + "ppp"),
    "t4r_item_topk_ws_bytes": ("l", "iiii"),
    "t4r_item_topk_f32": ("i", "p" + "iiif" + "pl" + "pl" + "i" + "pp" + "pl" + "p"),
    "t4r_item_table_image_ld": ("i", "i"),
    "t4r_item_topk_h16_supported": ("i", "i"),
    "t4r_item_table_pack_h16": ("i", "p" + "pl" + "iii" + "pl"),
    "t4r_item_scores_h16": ("i", "p" + "iiif" + "pl" + "pl" + "i" + "pl" + "pl"),
    "t4r_item_topk_h16_ws_bytes": ("l", "iiii"),
    "t4r_item_topk_h16": ("i", "p" + "iiif" + "pl" + "pl" + "i" + "i" + "pp" + "pl" + "p"),
    "t4r_item_eval_h16_ws_bytes": ("l", "iii"),
    "t4r_item_eval_h16": ("i", "p" + "iiif" + "pl" + "pl" + "i" + "p" + "pppp" + "pl"),
    "t4r_swap_noise_ws_bytes": ("l", "l"),
    "t4r_swap_noise": ("i", "ppp" + "il" + "pllf" + "pp" + "QQ" + "pl"),
    "t4r_copy_cols": ("i", "pp" + "li" + "p" + "ili"),
    "t4r_seq_sum_cols": ("i", "pp" + "li" + "p" + "ili"),
    "t4r_adam_step": ("i", "ppppp" + "li" + "ffffff" + "i"),
    "t4r_adam_step_amax": ("i", "ppppp" + "li" + "ffffff" + "i" + "llp"),
}

# the second header, include/t4r_hip_sampling.h (tests/test_sampling_cpu.py checks this table against it)
_SIGS_SAMPLING = {
    "t4r_gumbel_add_f32": ("i", "pp" + "iill" + "i" + "QQ"),
    "t4r_gumbel_argmax_f32": ("i", "pp" + "iill" + "QQ" + "pp"),
    "t4r_item_sample_ws_bytes": ("l", "iiii"),
    "t4r_item_sample_f32": ("i", "p" + "iiif" + "pl" + "pl" + "i" + "pp" + "pl" + "p" + "lQQ"),
    "t4r_item_sample_h16_ws_bytes": ("l", "iiii"),
    "t4r_item_sample_h16": ("i", "p" + "iiif" + "pl" + "pl" + "i" + "i" + "pp" + "pl" + "p" + "lQQ"),
}

# the third header, include/t4r_hip_filter.h (tests/test_item_filter_cpu.py checks this table against it); the filter tail is
# allow_bits, excl, n_excl, ld_excl
_FILT = "ppil"
_SIGS_FILTER = {
    "t4r_item_allow_words": ("l", "i"),
    "t4r_item_allow_pack": ("i", "ppip"),
    "t4r_item_mask_f32": ("i", "pp" + "iili" + _FILT),
    "t4r_item_topk_filtered_f32": ("i", _SIGS["t4r_item_topk_f32"][1] + _FILT),
    "t4r_item_topk_filtered_h16": ("i", _SIGS["t4r_item_topk_h16"][1] + _FILT),
    "t4r_item_sample_filtered_f32": ("i", _SIGS_SAMPLING["t4r_item_sample_f32"][1] + _FILT),
    "t4r_item_sample_filtered_h16": ("i", _SIGS_SAMPLING["t4r_item_sample_h16"][1] + _FILT),
}

# the fourth header, include/t4r_hip_optim.h (tests/test_optim_clip_cpu.py checks this table against it)
_SIGS_OPTIM = {
    "t4r_grad_sumsq_parts": ("l", "l"),
    "t4r_grad_sumsq": ("i", "pplp"),
    "t4r_grad_clip_coef": ("i", "ppiffp"),
    "t4r_adamw_step": ("i", "ppppp" + "li" + "fffff" + "if" + "i" + "p" + "llp"),
}

# the fifth header, include/t4r_hip_pretrained.h (tests/test_pretrained_cpu.py checks this table against it); the common head is
# stream, dtype, image, ldp, rows, ids, T, ids_div
_PP = "pipllpli"
_SIGS_PRETRAINED = {
    "t4r_pretrained_proj_ws_bytes": ("l", "ii"),
    "t4r_pretrained_proj_fwd": ("i", _PP + "ppppfii" + "pli" + "pppp"),
    "t4r_pretrained_proj_bwd_ws_floats": ("l", "lii"),
    "t4r_pretrained_proj_bwd": ("i", _PP + "pli" + "ppp" + "ii" + "ppppp"),
}

# the sixth header, include/t4r_hip_attn.h (tests/test_attn_prob_cpu.py checks this table against it): the one-kernel attention
# forward and the attention core's backward with the `prob` pointer
_SIGS_ATTN = {
    "t4r_xlnet_attn_block_fwd_prob": ("i", "ppppp" + "l" + "pppp" + "pppppppp" + "iiii" + "ffQQQ" + "p"),
    "t4r_xlnet_attn_bwd_prob": ("i", "p" * 16 + "iiii" + "ifQQ"),
}

# the seventh header, include/t4r_hip_rows.h (tests/test_last_rows_cpu.py checks this table against it): the row-mapped forms
# of the layer's row-wise kernels; the tail of each is the map (rows, n)
_SIGS_ROWS = {
    "t4r_xlnet_ff_fwd_rows": ("i", _SIGS["t4r_xlnet_ff_fwd"][1] + "pi"),
    "t4r_xlnet_ff_bwd_rows": ("i", _SIGS["t4r_xlnet_ff_bwd"][1] + "pip"),
    "t4r_xlnet_ln1_bwd_rows": ("i", "p" + "ppppppp" + "ppp" + "ppp" + "lif" + "QQ" + "pi"),
    "t4r_xlnet_layer_fwd_rows": ("i", _SIGS["t4r_xlnet_layer_fwd"][1] + "pi"),
    "t4r_xlnet_layer_bwd_rows": ("i", _SIGS["t4r_xlnet_layer_bwd"][1] + "pi"),
}

# the eighth header, include/t4r_hip_rowadam.h (tests/test_row_adam_cpu.py checks this table against it): the row-sparse Adam
# step; the arguments are stream, param, exp_avg, exp_avg_sq, V, D, keys, perm, grad_rows, ld_grad, n, step, the six floats
# (lr, beta1, beta2, eps, weight_decay | decoupled | grad_scale), ws, ws_bytes
_SIGS_ROWADAM = {
    "t4r_row_adam_ws_bytes": ("l", "li"),
    "t4r_row_adam_step": ("i", "pppp" + "li" + "ppp" + "lli" + "fffff" + "if" + "pl"),
}

# the ninth header, include/t4r_hip_contproj.h (tests/test_cont_proj_cpu.py checks this table against it): the first layer of
# `continuous_projection`; the common arguments are xs (host array of C device pointers), per_session (host ints), ntok, L, C, P,
# W, b
_CP = "pp" + "liii" + "pp"
_SIGS_CONTPROJ = {
    "t4r_cont_proj_supported": ("i", "ii"),
    "t4r_cont_proj_bwd_ws_floats": ("l", "lii"),
    "t4r_cont_proj_fwd": ("i", "p" + _CP + "p"),
    "t4r_cont_proj_bwd": ("i", "p" + "pli" + _CP + "pppp"),
}

# the tenth header, include/t4r_hip_rowclip.h (tests/test_row_clip_cpu.py checks this table against it): the row-sparse Adam step
# in two halves for global-norm clipping.  reduce: stream, V, D, keys, perm, grad_rows, ld_grad, n, ws, ws_bytes, part; apply:
# stream, param, exp_avg, exp_avg_sq, V, D, n, step, the six floats (lr, beta1, beta2, eps, weight_decay | decoupled | grad_scale),
# clip_coef, ws, ws_bytes
_SIGS_ROWCLIP = {
    "t4r_row_grad_sumsq_parts": ("l", "li"),
    "t4r_row_adam_reduce": ("i", "pli" + "ppp" + "ll" + "pl" + "p"),
    "t4r_row_adam_apply": ("i", "pppp" + "li" + "li" + "fffff" + "if" + "p" + "pl"),
}

# the eleventh header, include/t4r_hip_seqtask.h (tests/test_session_task_cpu.py checks this table against it): the session-level
# prediction tasks.  fwd: stream, x, len, B, L, D, summary, w, b, act, loss_kind, target, s, pred, loss, ws; bwd: stream, g, pred,
# target, s, len, B, L, D, summary, w, act, loss_kind, dx, d_w, d_b, ws
_SIGS_SEQTASK = {
    "t4r_seq_task_supported": ("i", "ii"),
    "t4r_seq_task_ws_floats": ("l", "li"),
    "t4r_seq_task_fwd": ("i", "p" + "pp" + "lii" + "i" + "pp" + "ii" + "p" + "pppp"),
    "t4r_seq_task_bwd": ("i", "p" + "ppppp" + "lii" + "i" + "p" + "ii" + "pppp"),
}

# the twelfth header, include/t4r_hip_rtd.h (tests/test_rtd_cpu.py checks this table against it): the replaced-token-detection
# head.  fwd: stream, x, active, label, T, D, W1, b1, w2, b2, act, z, n_active, loss, ws; bwd: stream, g, x, active, label, z,
# n_active, T, D, W1, b1, w2, act, dx, d_W1, d_b1, d_w2, d_b2, ws
_SIGS_RTD = {
    "t4r_rtd_head_supported": ("i", "i"),
    "t4r_rtd_head_ws_floats": ("l", "li"),
    "t4r_rtd_head_fwd": ("i", "p" + "ppp" + "li" + "pppp" + "i" + "pppp"),
    "t4r_rtd_head_bwd": ("i", "p" + "pppppp" + "li" + "ppp" + "i" + "pppppp"),
}

_lib = None


class T4RHipError(RuntimeError):
    pass


def _declared(path):
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(t4r_\w+)\s*\(", text)))


def header_symbols():
    """Function names declared in include/t4r_hip.h."""
    return _declared(HEADER_PATH)


def sampling_header_symbols():
    """Function names declared in include/t4r_hip_sampling.h."""
    return _declared(SAMPLING_HEADER_PATH)


def filter_header_symbols():
    """Function names declared in include/t4r_hip_filter.h."""
    return _declared(FILTER_HEADER_PATH)


def optim_header_symbols():
    """Function names declared in include/t4r_hip_optim.h."""
    return _declared(OPTIM_HEADER_PATH)


def pretrained_header_symbols():
    """Function names declared in include/t4r_hip_pretrained.h."""
    return _declared(PRETRAINED_HEADER_PATH)


def attn_header_symbols():
    """Function names declared in include/t4r_hip_attn.h."""
    return _declared(ATTN_HEADER_PATH)


def rows_header_symbols():
    """Function names declared in include/t4r_hip_rows.h."""
    return _declared(ROWS_HEADER_PATH)


def rowadam_header_symbols():
    """Function names declared in include/t4r_hip_rowadam.h."""
    return _declared(ROWADAM_HEADER_PATH)


def contproj_header_symbols():
    """Function names declared in include/t4r_hip_contproj.h."""
    return _declared(CONTPROJ_HEADER_PATH)


def rowclip_header_symbols():
    """Function names declared in include/t4r_hip_rowclip.h."""
    return _declared(ROWCLIP_HEADER_PATH)


def seqtask_header_symbols():
    """Function names declared in include/t4r_hip_seqtask.h."""
    return _declared(SEQTASK_HEADER_PATH)


def rtd_header_symbols():
    """Function names declared in include/t4r_hip_rtd.h."""
    return _declared(RTD_HEADER_PATH)


def load():
    """Loads the library and sets ctypes prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise T4RHipError(
            f"{LIB_PATH} not found: the HIP extension is not built "
            "(run `python -m transformers4rec_amd.build`). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (ret, args) in (list(_SIGS.items()) + list(_SIGS_SAMPLING.items()) + list(_SIGS_FILTER.items()) + list(_SIGS_OPTIM.items())
                              + list(_SIGS_PRETRAINED.items()) + list(_SIGS_ATTN.items()) + list(_SIGS_ROWS.items()) + list(_SIGS_ROWADAM.items())
                              + list(_SIGS_CONTPROJ.items()) + list(_SIGS_ROWCLIP.items()) + list(_SIGS_SEQTASK.items())
                              + list(_SIGS_RTD.items())):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_char_p if ret == "s" else (None if ret == "v" else _C[ret])
        fn.argtypes = [_C[a] for a in args]
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().t4r_last_error()
        raise T4RHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def call(name, *args):
    rc = getattr(load(), name)(*args)
    if rc != 0:
        check(rc, name)


def ptr_array(ptrs):
    """host array of device pointers (const T* const*)"""
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def int_array(vals):
    arr = (ctypes.c_int * len(vals))(*vals)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def long_array(vals):
    arr = (ctypes.c_long * len(vals))(*vals)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def exp_env(name, default=None):
    """value of an EXPERIMENT switch: the environment variable `name` when the loaded library is an experiment build
    (-DT4R_EXPERIMENTAL, tools/experimental/build_variant.sh), else `default`.  The product build ignores these names on both
    sides of the C ABI (csrc/t4r_common.h: t4r_exp_getenv), so that the host never plans for a kernel family the library
    will not run.  The switches the product DOES read are listed in INTEGRATION.md section 5."""
    v = os.environ.get(name)
    if v is None:
        return default
    try:
        return v if load().t4r_experimental_build() else default
    except Exception:       # noqa: BLE001  (library not built yet: CPU-only import)
        return default
