"""ctypes binding of librama_hip.so (C ABI declared in include/rama_hip.h).

The product path has no fallback: if the shared library is missing or a call fails,
this raises.  Nothing here imports the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
# (RAMA_HIP_LIB: another build of the same library -- A/B runs of compile-time variants, tools/ab_lib.sh; never a fallback)
LIB_PATH = Path(os.environ["RAMA_HIP_LIB"]) if os.environ.get("RAMA_HIP_LIB") else _HERE / "librama_hip.so"

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)


class RamaError(RuntimeError):
    pass


class rama_config(C.Structure):
    """engine/src/transformer/mod.rs:128-138"""
    _fields_ = [(n, C.c_int32) for n in (
        "dim", "hidden_dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size", "seq_len", "shared_weight")]


W_FIELDS = ("token_embedding_table", "rms_att_weight", "rms_ffn_weight",
            "wq", "wk", "wv", "wo", "w1", "w2", "w3",
            "rms_final_weight", "freq_cis_real", "freq_cis_imag", "wcls")
S_FIELDS = ("x", "xb", "xb2", "hb", "hb2", "q", "k", "v", "att", "logits", "key_cache", "value_cache")


class rama_weights(C.Structure):
    """engine/src/transformer/state.rs:53-74 (device pointers)"""
    _fields_ = [(n, C.c_void_p) for n in W_FIELDS]


class rama_run_state(C.Structure):
    """engine/src/transformer/state.rs:3-17 (device pointers)"""
    _fields_ = [(n, C.c_void_p) for n in S_FIELDS]


Q8_TENSORS = ("tok", "wq", "wk", "wv", "wo", "w1", "w2", "w3", "wcls")


class rama_q8_weights(C.Structure):
    """include/rama_hip.h rama_q8_weights (device pointers; x_s = the scales of x)"""
    _fields_ = ([("group_size", C.c_int32)] +
                [(n, C.c_void_p) for n in ("token_embedding_table", "rms_att_weight", "rms_ffn_weight", "rms_final_weight",
                                           "freq_cis_real", "freq_cis_imag")] +
                [(n, C.c_void_p) for n in Q8_TENSORS] + [(n + "_s", C.c_void_p) for n in Q8_TENSORS])


class rama_stage(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("layer_begin", "layer_end", "do_embed", "do_cls")]


class rama_seq_sampling(C.Structure):
    """one sequence's sampler and forced prompt of the sampled chained batch (rama_decode_batch_begin_sampled)"""
    _fields_ = [("temperature", C.c_float), ("topp", C.c_float), ("u", C.c_float), ("forced", C.POINTER(C.c_int32)), ("n_forced", C.c_int32)]


class rama_q8_seq_plan(C.Structure):
    """one sequence's sampler, forced prompt, step budget and stop token of the chained Q8 batch (rama_q8_decode_batch_begin)"""
    _fields_ = [("temperature", C.c_float), ("topp", C.c_float), ("u", C.c_float), ("forced", C.POINTER(C.c_int32)), ("n_forced", C.c_int32),
                ("max_new", C.c_int32), ("stop_token", C.c_int32)]


class rama_q8_serve_slot(C.Structure):
    """a slot of the serving chain as rama_q8_serve_plan_step and rama_q8_serve_stats see it (state: 0 FREE, 1 PROMPT, 2 DECODE, 3 DONE)"""
    _fields_ = [(n, C.c_int32) for n in ("state", "n_context", "cursor", "n_out", "max_new")]


class rama_q8_serve_row(C.Structure):
    """a row of a serving step: its slot and position (-1, -1: idle), and whether it carries logits"""
    _fields_ = [(n, C.c_int32) for n in ("slot", "pos", "logits")]


class rama_q8_serve_plan(C.Structure):
    """an admitted sequence's sampler, budget and stop token (rama_q8_serve_admit)"""
    _fields_ = [("temperature", C.c_float), ("topp", C.c_float), ("u", C.c_float), ("max_new", C.c_int32), ("stop_token", C.c_int32)]


class rama_q8_serve_report(C.Structure):
    """what rama_q8_serve_stats fills in: the device counters, the slot table, the last step's row table"""
    _fields_ = ([(n, C.c_uint64) for n in ("steps", "graph_captures", "rows_decode", "rows_prompt", "rows_idle")] +
                [("n_slots", C.c_int32), ("max_rows", C.c_int32), ("last_rows", rama_q8_serve_row * 128),
                 ("slots", rama_q8_serve_slot * 128), ("generation", C.c_int32 * 128)])


class rama_q8_spec_plan(C.Structure):
    """the speculative chain's sampler, budget, stop token, draft sizes and hint text (rama_q8_spec_begin)"""
    _fields_ = [("temperature", C.c_float), ("topp", C.c_float), ("u", C.c_float), ("max_new", C.c_int32), ("stop_token", C.c_int32),
                ("n_draft", C.c_int32), ("ngram", C.c_int32), ("hint", C.POINTER(C.c_int32)), ("n_hint", C.c_int32)]


class rama_q8_spec_report(C.Structure):
    """what rama_q8_spec_stats fills in: the device counters, the accept histogram, the sequence's cursor"""
    _fields_ = ([(n, C.c_uint64) for n in ("steps", "graph_captures", "rows_fed", "drafts", "accepted", "emitted")] +
                [("accepted_hist", C.c_uint64 * 16), ("finished", C.c_int32), ("n_out", C.c_int32), ("cursor", C.c_int32)])


class rama_q8_spec_model_report(C.Structure):
    """what rama_q8_spec_model_stats fills in: the draft model's side of a chain begun with rama_q8_spec_begin_model"""
    _fields_ = [(n, C.c_uint64) for n in ("draft_passes", "draft_rows_fed", "catch_up_rows")] + [("draft_cursor", C.c_int32)]


class rama_q8_spec_tree_report(C.Structure):
    """what rama_q8_spec_tree_stats fills in: the tree side of a chain begun with rama_q8_spec_begin_tree"""
    _fields_ = ([(n, C.c_uint64) for n in ("off_trunk_accepted", "off_trunk_steps")] + [("nodes_hist", C.c_uint64 * 16)] +
                [("n_branch", C.c_int32), ("n_rows", C.c_int32)])


class rama_q8_serve_spec(C.Structure):
    """a slot's drafting fields on a serving chain begun with rama_q8_serve_begin_spec (rama_q8_serve_admit_spec)"""
    _fields_ = [("n_draft", C.c_int32), ("ngram", C.c_int32), ("hint", C.POINTER(C.c_int32)), ("n_hint", C.c_int32)]


class rama_q8_serve_spec_report(C.Structure):
    """what rama_q8_serve_spec_stats fills in: the row counters, the draft counters, the accept histogram, per slot the last step's drafts"""
    _fields_ = ([(n, C.c_uint64) for n in ("steps", "rows_decode", "rows_draft", "rows_prompt", "rows_idle", "drafts_wanted", "drafts_granted",
                                           "drafts_accepted", "tokens_emitted")] +
                [("accepted_hist", C.c_uint64 * 16)] + [(n, C.c_int32) for n in ("n_slots", "max_rows", "n_draft_cap", "hint_cap")] +
                [("last_want", C.c_int32 * 128), ("last_granted", C.c_int32 * 128)])


class rama_q8_serve_model_report(C.Structure):
    """what rama_q8_serve_model_stats fills in: the draft model's side of a serving chain begun with rama_q8_serve_begin_model"""
    _fields_ = ([(n, C.c_uint64) for n in ("draft_passes", "draft_rows_fed", "catch_up_rows")] +
                [("n_slots", C.c_int32), ("n_draft_cap", C.c_int32), ("draft_cursor", C.c_int32 * 128)])


class rama_pipe_plan(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("n_pos", C.c_int32), ("wrap", C.c_int32), ("prompt", C.POINTER(C.c_int32)), ("n_prompt", C.c_int32),
                ("temperature", C.c_float), ("topp", C.c_float), ("u", C.c_float), ("out_tokens_dev", C.c_void_p)]


class rama_pipe_tick(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("on", "seq", "pos", "pos_wrapped", "token_kind", "token", "samples", "send_kind", "send_seq", "send_peer",
                                         "recv_kind", "recv_seq", "recv_peer", "recv_pos")]


# name -> (restype, argtypes); every symbol include/rama_hip.h declares
_vp, _sz, _int = C.c_void_p, C.c_size_t, C.c_int
_cfgp, _wp, _sp, _stp = C.POINTER(rama_config), C.POINTER(rama_weights), C.POINTER(rama_run_state), C.POINTER(rama_stage)
SIGNATURES = {
    "rama_ctx_create": (_int, [_int, _vp, C.POINTER(_vp)]),
    "rama_ctx_destroy": (_int, [_vp]),
    "rama_sync": (_int, [_vp]),
    "rama_stream_query": (_int, [_vp]),
    "rama_last_error": (C.c_char_p, []),
    "rama_device_info": (_int, [_vp, C.c_char_p, C.POINTER(_int), C.POINTER(_sz)]),
    "rama_alloc_f32": (_int, [_vp, _sz, C.POINTER(_vp)]),
    "rama_upload_f32": (_int, [_vp, _vp, _sz, C.POINTER(_vp)]),
    "rama_copy_h2d_f32": (_int, [_vp, _vp, _vp, _sz]),
    "rama_download_f32": (_int, [_vp, _vp, _sz, _vp]),
    "rama_free": (_int, [_vp, _vp]),
    "rama_array_add": (_int, [_vp, _vp, _vp, _sz]),
    "rama_array_mult": (_int, [_vp, _vp, _vp, _sz]),
    "rama_sinu": (_int, [_vp, _vp, _sz]),
    "rama_copy_from_slice": (_int, [_vp, _vp, _vp, _sz]),
    "rama_rmsnorm": (_int, [_vp, _vp, _vp, _vp, _sz]),
    "rama_apply_position": (_int, [_vp, _vp, _vp, _vp, _vp, _sz]),
    "rama_matmul": (_int, [_vp, _vp, _vp, _vp, _sz, _sz, _sz]),
    "rama_softmax": (_int, [_vp, _vp, _sz]),
    "rama_multi_head_attention": (_int, [_vp, _vp, _vp, _vp, _vp, _vp] + [_int] * 6),
    "rama_sample_argmax": (_int, [_vp, _vp, _sz, i32p]),
    "rama_sample_topp": (_int, [_vp, _vp, _sz, C.c_float, C.c_float, C.c_float, i32p]),
    "rama_model_load": (_int, [_vp, C.c_char_p, C.POINTER(_vp)]),
    "rama_model_load_stage": (_int, [_vp, C.c_char_p, _stp, C.POINTER(_vp)]),
    "rama_model_synth": (_int, [_vp, _cfgp, C.c_uint64, _stp, _vp, _vp, C.POINTER(_vp)]),
    "rama_model_save": (_int, [_vp, _vp, C.c_char_p]),
    "rama_model_config": (_int, [_vp, _cfgp]),
    "rama_model_weights": (_int, [_vp, _wp]),
    "rama_model_bytes": (_sz, [_vp]),
    "rama_model_free": (_int, [_vp, _vp]),
    "rama_model_release_copies": (_int, [_vp, _vp, _int]),
    "rama_state_create": (_int, [_vp, _cfgp, _int, _sp]),
    "rama_state_free": (_int, [_vp, _sp]),
    "rama_fill_synth": (_int, [_vp, _vp, _sz, C.c_uint64, C.c_uint64, C.c_uint64, C.c_float, C.c_float]),
    "rama_forward": (_int, [_vp, _cfgp, _wp, _sp, _int, _int]),
    "rama_forward_stage": (_int, [_vp, _cfgp, _wp, _sp, _int, _int, _stp]),
    "rama_prefill": (_int, [_vp, _cfgp, _wp, _sp, i32p, _int, _int]),
    "rama_decode_batch": (_int, [_vp, _cfgp, _wp, _sp, i32p, i32p, _int]),
    "rama_decode_batch_begin": (_int, [_vp, _cfgp, _wp, _sp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _int, _int]),
    "rama_decode_batch_begin_sampled": (_int, [_vp, _cfgp, _wp, _sp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _int, _int,
                                                C.POINTER(rama_seq_sampling)]),
    "rama_decode_batch_steps": (_int, [_vp, _int]),
    "rama_decode_batch_tokens": (_int, [_vp, C.POINTER(C.c_int32), _int, C.POINTER(_int)]),
    "rama_forward_stage_devtok": (_int, [_vp, _cfgp, _wp, _sp, _vp, _int, _stp]),
    "rama_argmax_dev": (_int, [_vp, _vp, _sz, _vp]),
    "rama_generate_greedy": (_int, [_vp, _cfgp, _wp, _sp, i32p, _int, _int, i32p]),
    "rama_generate": (_int, [_vp, _cfgp, _wp, _sp, i32p, _int, _int, C.c_float, C.c_float, C.c_float, i32p]),
    "rama_sample_topp_dev": (_int, [_vp, _vp, _sz, C.c_float, C.c_float, C.c_float, _vp]),
    "rama_sample_topp_batch_dev": (_int, [_vp, _vp, _sz, _sz, _int, f32p, f32p, f32p, _vp]),
    "rama_decode_sampler": (_int, [_vp, C.c_float, C.c_float, C.c_float]),
    "rama_decode_begin": (_int, [_vp, _int, _int, i32p, _int]),
    "rama_decode_steps": (_int, [_vp, _cfgp, _wp, _sp, _int]),
    "rama_decode_tokens": (_int, [_vp, i32p, _int, C.POINTER(_int)]),
    "rama_decode_stream_poll": (_int, [_vp, _int, i32p, _int, C.POINTER(_int)]),
    "rama_decode_batch_stream_poll": (_int, [_vp, _int, _int, i32p, _int, C.POINTER(_int)]),
    "rama_generate_stream": (_int, [_vp, _cfgp, _wp, _sp, i32p, _int, _int, C.c_float, C.c_float, C.c_float,
                                    C.CFUNCTYPE(None, C.c_void_p, _int, C.c_int32), C.c_void_p, i32p]),
    "rama_set_graph_mode": (_int, [_vp, _int]),
    "rama_set_tuning": (_int, [_vp, C.c_char_p, _int]),
    "rama_ref_expf": (_int, [_vp, _vp, _vp, _sz]),
    "rama_pipe_unique_id": (_int, [_vp]),
    "rama_pipe_create": (_int, [_vp, _vp, _int, _int, C.POINTER(_vp)]),
    "rama_pipe_destroy": (_int, [_vp]),
    "rama_pipe_exchange": (_int, [_vp, _vp, _sz, _int, _vp, _sz, _int, _vp, _int, _vp, _int]),
    "rama_pipe_item": (_int, [_vp, _int, _int, _int, C.POINTER(_int), C.POINTER(_int)]),
    "rama_pipe_total_ticks": (_int, [_vp, _vp]),
    "rama_pipe_plan_ticks": (_int, [_vp, _int]),
    "rama_pipe_tick_plan": (_int, [_vp, _int, _int, _int, C.POINTER(rama_pipe_tick)]),
    "rama_pipe_comm_info": (_int, [_vp, C.POINTER(_int), C.POINTER(_int)]),
    "rama_pipe_run_ticks": (_int, [_vp, _cfgp, _wp, _sp, C.POINTER(_vp), _stp, _vp, _int, _int]),
    "rama_pipe_last_error": (C.c_char_p, []),
    "rama_timer_start": (_int, [_vp]),
    "rama_timer_stop": (_int, [_vp, C.POINTER(C.c_float)]),
    "rama_kprof_enable": (_int, [_vp, _int, _int]),
    "rama_kprof_read": (_int, [_vp, C.POINTER(_int), C.POINTER(C.c_double)]),
    "rama_q8_model_load": (_int, [_vp, C.c_char_p, C.POINTER(_vp)]),
    "rama_q8_model_synth": (_int, [_vp, _cfgp, _int, C.c_uint64, C.POINTER(_vp)]),
    "rama_q8_model_from_f32": (_int, [_vp, _cfgp, _wp, _int, C.POINTER(_vp)]),
    "rama_q8_model_config": (_int, [_vp, _cfgp]),
    "rama_q8_model_weights": (_int, [_vp, C.POINTER(rama_q8_weights)]),
    "rama_q8_model_bytes": (_sz, [_vp]),
    "rama_q8_model_free": (_int, [_vp, _vp]),
    "rama_q8_quantize": (_int, [_vp, _vp, _sz, _int, _vp, _vp]),
    "rama_q8_matmul": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _int]),
    "rama_q8_product_path": (_int, [_sz, _int, _int, _int]),
    "rama_q8_batch_shape_ok": (_int, [_cfgp]),
    "rama_q8_forward": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _sp, _int, _int]),
    "rama_q8_generate": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _sp, i32p, _int, _int, C.c_float, C.c_float, C.c_float, i32p]),
    "rama_q8_matmul_batch": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _int, _int]),
    "rama_q8_prefill": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _sp, i32p, _int, _int]),
    "rama_q8_decode_batch": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _sp, i32p, i32p, _int]),
    "rama_q8_decode_batch_begin": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _sp, i32p, i32p, _int, _int, C.POINTER(rama_q8_seq_plan)]),
    "rama_q8_decode_batch_steps": (_int, [_vp, _int]),
    "rama_q8_decode_batch_tokens": (_int, [_vp, i32p, _int, i32p]),
    "rama_q8_decode_batch_stream_poll": (_int, [_vp, _int, _int, i32p, _int, C.POINTER(_int), C.POINTER(_int)]),
    "rama_q8_serve_begin": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _int, _int, _int]),
    "rama_q8_serve_admit": (_int, [_vp, _int, _sp, i32p, _int, C.POINTER(rama_q8_serve_plan)]),
    "rama_q8_serve_admit_at": (_int, [_vp, _int, _sp, i32p, _int, _int, C.POINTER(rama_q8_serve_plan)]),
    "rama_q8_kv_fork": (_int, [_vp, _cfgp, _sp, _sp, _int, _int]),
    "rama_q8_serve_steps": (_int, [_vp, _int]),
    "rama_q8_serve_poll": (_int, [_vp, _int, _int, i32p, _int, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int)]),
    "rama_q8_serve_tokens": (_int, [_vp, _int, i32p, _int, C.POINTER(_int)]),
    "rama_q8_serve_stats": (_int, [_vp, C.POINTER(rama_q8_serve_report)]),
    "rama_q8_serve_plan_step": (_int, [C.POINTER(rama_q8_serve_slot), _int, _int, C.POINTER(rama_q8_serve_row), C.POINTER(rama_q8_serve_slot)]),
    "rama_q8_serve_end": (_int, [_vp]),
    # the fp32 serving chain (parity mode): the same arguments with rama_weights
    "rama_serve_begin": (_int, [_vp, _cfgp, C.POINTER(rama_weights), _int, _int, _int]),
    "rama_serve_admit": (_int, [_vp, _int, _sp, i32p, _int, C.POINTER(rama_q8_serve_plan)]),
    "rama_serve_admit_at": (_int, [_vp, _int, _sp, i32p, _int, _int, C.POINTER(rama_q8_serve_plan)]),
    "rama_serve_steps": (_int, [_vp, _int]),
    "rama_serve_poll": (_int, [_vp, _int, _int, i32p, _int, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int)]),
    "rama_serve_tokens": (_int, [_vp, _int, i32p, _int, C.POINTER(_int)]),
    "rama_serve_stats": (_int, [_vp, C.POINTER(rama_q8_serve_report)]),
    "rama_serve_end": (_int, [_vp]),
    "rama_q8_spec_begin": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _sp, i32p, _int, C.POINTER(rama_q8_spec_plan)]),
    "rama_q8_spec_steps": (_int, [_vp, _int]),
    "rama_q8_spec_poll": (_int, [_vp, _int, i32p, _int, C.POINTER(_int), C.POINTER(_int)]),
    "rama_q8_spec_tokens": (_int, [_vp, i32p, _int, C.POINTER(_int)]),
    "rama_q8_spec_stats": (_int, [_vp, C.POINTER(rama_q8_spec_report)]),
    "rama_q8_spec_end": (_int, [_vp]),
    "rama_q8_spec_begin_model": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _sp, _cfgp, C.POINTER(rama_q8_weights), _sp, i32p, _int,
                                        C.POINTER(rama_q8_spec_plan)]),
    "rama_q8_spec_model_stats": (_int, [_vp, C.POINTER(rama_q8_spec_model_report)]),
    "rama_q8_spec_draft": (_int, [i32p, _int, i32p, _int, _int, _int, _int, i32p]),
    "rama_q8_spec_accept": (_int, [i32p, _int, i32p, _int, _int, C.POINTER(_int)]),
    "rama_q8_spec_begin_tree": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _sp, i32p, _int, C.POINTER(rama_q8_spec_plan), _int, _int]),
    "rama_q8_spec_tree_stats": (_int, [_vp, C.POINTER(rama_q8_spec_tree_report)]),
    "rama_q8_spec_tree_draft": (_int, [i32p, _int, i32p, _int, _int, _int, _int, _int, _int, i32p, i32p, i32p]),
    "rama_q8_spec_tree_accept": (_int, [i32p, i32p, _int, i32p, _int, _int, i32p, C.POINTER(_int), C.POINTER(_int)]),
    "rama_q8_tree_forward": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _sp, i32p, i32p, _int, _int, _vp]),
    "rama_q8_tree_commit": (_int, [_vp, _cfgp, _sp, i32p, _int, _int]),
    "rama_q8_spec_begin_model_tree": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _sp, _cfgp, C.POINTER(rama_q8_weights), _sp, i32p, _int,
                                             C.POINTER(rama_q8_spec_plan), _int, _int]),
    "rama_q8_spec_model_tree_shape": (_int, [_int, _int, _int, i32p, i32p, i32p]),
    "rama_q8_spec_model_tree_candidates": (_int, [C.POINTER(C.c_float), _int, _int, _int, i32p]),
    "rama_q8_spec_model_tree_last": (_int, [_vp, i32p, i32p, i32p, i32p, i32p, C.POINTER(_int), C.POINTER(_int)]),
    "rama_q8_serve_begin_spec": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _int, _int, _int, _int, _int]),
    "rama_q8_serve_admit_spec": (_int, [_vp, _int, _sp, i32p, _int, _int, C.POINTER(rama_q8_serve_plan), C.POINTER(rama_q8_serve_spec)]),
    "rama_q8_serve_spec_plan_step": (_int, [C.POINTER(rama_q8_serve_slot), _int, _int, i32p, C.POINTER(rama_q8_serve_row), i32p]),
    "rama_q8_serve_spec_stats": (_int, [_vp, C.POINTER(rama_q8_serve_spec_report)]),
    "rama_q8_serve_begin_model": (_int, [_vp, _cfgp, C.POINTER(rama_q8_weights), _cfgp, C.POINTER(rama_q8_weights), _int, _int, _int, _int]),
    "rama_q8_serve_admit_model": (_int, [_vp, _int, _sp, _sp, i32p, _int, _int, C.POINTER(rama_q8_serve_plan), _int]),
    "rama_q8_serve_model_plan_step": (_int, [C.POINTER(rama_q8_serve_slot), _int, _int, _int, i32p, i32p, _int, C.POINTER(rama_q8_serve_row), i32p, i32p,
                                             C.POINTER(rama_q8_serve_row)]),
    "rama_q8_serve_model_stats": (_int, [_vp, C.POINTER(rama_q8_serve_model_report)]),
    "rama_serve_begin_spec": (_int, [_vp, _cfgp, C.POINTER(rama_weights), _int, _int, _int, _int, _int]),
    "rama_serve_admit_spec": (_int, [_vp, _int, _sp, i32p, _int, _int, C.POINTER(rama_q8_serve_plan), C.POINTER(rama_q8_serve_spec)]),
    "rama_serve_spec_stats": (_int, [_vp, C.POINTER(rama_q8_serve_spec_report)]),
    "rama_serve_begin_model": (_int, [_vp, _cfgp, C.POINTER(rama_weights), _cfgp, C.POINTER(rama_q8_weights), _int, _int, _int, _int]),
    "rama_serve_admit_model": (_int, [_vp, _int, _sp, _sp, i32p, _int, _int, C.POINTER(rama_q8_serve_plan), _int]),
    "rama_serve_model_stats": (_int, [_vp, C.POINTER(rama_q8_serve_model_report)]),
    "rama_q8_serve_cancel": (_int, [_vp, i32p, _int]),
    "rama_serve_cancel": (_int, [_vp, i32p, _int]),
}

# exported but not in the header (the rama_internal_* accessors tests read; most declare their own types where they call them): here
# because ctypes would otherwise cut a 64-bit result down to an int
INTERNAL_SIGNATURES = {
    "rama_internal_op_launches": (C.c_ulonglong, [_vp, _int]),
}

_lib = None


def load() -> C.CDLL:
    """dlopen the in-tree library.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RamaError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        f"or `make -C rama_amd/csrc`")
    L = C.CDLL(str(LIB_PATH))
    for name, (res, args) in {**SIGNATURES, **INTERNAL_SIGNATURES}.items():
        fn = getattr(L, name)          # AttributeError if the library lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().rama_last_error()
        raise RamaError(f"{what or 'rama call'} failed ({rc}): {msg.decode() if msg else ''}")
