//! Raw bindings of include/rama_hip.h: every entry point (first the ones the Device trait and the optional
//! fast path need, then the rest).
//! `*mut f32` / `*const f32` are DEVICE pointers; every function returns 0 or an error code and
//! leaves a message in `rama_last_error()` (thread-local).
#![allow(non_camel_case_types, dead_code)]
use core::ffi::{c_char, c_int, c_void};

#[repr(C)] pub struct rama_ctx { _p: [u8; 0] }
#[repr(C)] pub struct rama_model { _p: [u8; 0] }

/// transformer/mod.rs:128-138 with C ints
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct rama_config {
    pub dim: i32, pub hidden_dim: i32, pub n_layers: i32, pub n_heads: i32,
    pub n_kv_heads: i32, pub vocab_size: i32, pub seq_len: i32, pub shared_weight: i32,
}
/// transformer/state.rs:53-74 as device pointers
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_weights {
    pub token_embedding_table: *const f32, pub rms_att_weight: *const f32, pub rms_ffn_weight: *const f32,
    pub wq: *const f32, pub wk: *const f32, pub wv: *const f32, pub wo: *const f32,
    pub w1: *const f32, pub w2: *const f32, pub w3: *const f32,
    pub rms_final_weight: *const f32, pub freq_cis_real: *const f32, pub freq_cis_imag: *const f32,
    pub wcls: *const f32,
}
/// transformer/state.rs:3-17 as device pointers
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_run_state {
    pub x: *mut f32, pub xb: *mut f32, pub xb2: *mut f32, pub hb: *mut f32, pub hb2: *mut f32,
    pub q: *mut f32, pub k: *mut f32, pub v: *mut f32, pub att: *mut f32, pub logits: *mut f32,
    pub key_cache: *mut f32, pub value_cache: *mut f32,
}
/// one sequence's sampler and forced prompt of the sampled chained batch (rama_decode_batch_begin_sampled)
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_seq_sampling {
    pub temperature: f32, pub topp: f32, pub u: f32, pub forced: *const i32, pub n_forced: i32,
}
/// one sequence's sampler, forced prompt, step budget (0 = the chain's) and stop token (-1 = none) of the chained Q8 batch
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_q8_seq_plan {
    pub temperature: f32, pub topp: f32, pub u: f32, pub forced: *const i32, pub n_forced: i32, pub max_new: i32, pub stop_token: i32,
}
/// a slot of the serving chain (state: 0 FREE, 1 PROMPT, 2 DECODE, 3 DONE), a row of a step (idle: slot -1, pos -1), an admission's plan,
/// and what rama_q8_serve_stats reports
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct rama_q8_serve_slot { pub state: i32, pub n_context: i32, pub cursor: i32, pub n_out: i32, pub max_new: i32 }
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct rama_q8_serve_row { pub slot: i32, pub pos: i32, pub logits: i32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_q8_serve_plan { pub temperature: f32, pub topp: f32, pub u: f32, pub max_new: i32, pub stop_token: i32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_q8_serve_report {
    pub steps: u64, pub graph_captures: u64, pub rows_decode: u64, pub rows_prompt: u64, pub rows_idle: u64,
    pub n_slots: i32, pub max_rows: i32,
    pub last_rows: [rama_q8_serve_row; 128], pub slots: [rama_q8_serve_slot; 128], pub generation: [i32; 128],
}
/// the speculative chain's plan (hint may be null with n_hint 0) and what rama_q8_spec_stats reports
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_q8_spec_plan {
    pub temperature: f32, pub topp: f32, pub u: f32, pub max_new: i32, pub stop_token: i32, pub n_draft: i32, pub ngram: i32,
    pub hint: *const i32, pub n_hint: i32,
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct rama_q8_spec_report {
    pub steps: u64, pub graph_captures: u64, pub rows_fed: u64, pub drafts: u64, pub accepted: u64, pub emitted: u64,
    pub accepted_hist: [u64; 16],
    pub finished: i32, pub n_out: i32, pub cursor: i32,
}
/// what rama_q8_spec_model_stats reports: the draft model's side of a chain begun with rama_q8_spec_begin_model
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_q8_spec_model_report { pub draft_passes: u64, pub draft_rows_fed: u64, pub catch_up_rows: u64, pub draft_cursor: i32 }
/// what rama_q8_spec_tree_stats reports: the tree side of a chain begun with rama_q8_spec_begin_tree
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_q8_spec_tree_report { pub off_trunk_accepted: u64, pub off_trunk_steps: u64, pub nodes_hist: [u64; 16], pub n_branch: i32, pub n_rows: i32 }
/// what rama_q8_serve_model_stats reports: the draft model's side of a serving chain begun with rama_q8_serve_begin_model
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_q8_serve_model_report {
    pub draft_passes: u64, pub draft_rows_fed: u64, pub catch_up_rows: u64, pub n_slots: i32, pub n_draft_cap: i32, pub draft_cursor: [i32; 128],
}
/// a slot's drafting fields on a serving chain begun with rama_q8_serve_begin_spec (hint may be null with n_hint 0) and what
/// rama_q8_serve_spec_stats reports
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_q8_serve_spec { pub n_draft: i32, pub ngram: i32, pub hint: *const i32, pub n_hint: i32 }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_q8_serve_spec_report {
    pub steps: u64, pub rows_decode: u64, pub rows_draft: u64, pub rows_prompt: u64, pub rows_idle: u64,
    pub drafts_wanted: u64, pub drafts_granted: u64, pub drafts_accepted: u64, pub tokens_emitted: u64,
    pub accepted_hist: [u64; 16],
    pub n_slots: i32, pub max_rows: i32, pub n_draft_cap: i32, pub hint_cap: i32,
    pub last_want: [i32; 128], pub last_granted: [i32; 128],
}
#[repr(C)] pub struct rama_q8_model { _p: [u8; 0] }
/// a Q8_0 (llama2.c version-2) model as device pointers; `x_s` = the fp32 scales of the int8 tensor `x`
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_q8_weights {
    pub group_size: i32,
    pub token_embedding_table: *const f32, pub rms_att_weight: *const f32, pub rms_ffn_weight: *const f32,
    pub rms_final_weight: *const f32, pub freq_cis_real: *const f32, pub freq_cis_imag: *const f32,
    pub tok: *const i8, pub wq: *const i8, pub wk: *const i8, pub wv: *const i8, pub wo: *const i8,
    pub w1: *const i8, pub w2: *const i8, pub w3: *const i8, pub wcls: *const i8,
    pub tok_s: *const f32, pub wq_s: *const f32, pub wk_s: *const f32, pub wv_s: *const f32, pub wo_s: *const f32,
    pub w1_s: *const f32, pub w2_s: *const f32, pub w3_s: *const f32, pub wcls_s: *const f32,
}

extern "C" {
    pub fn rama_ctx_create(device: c_int, stream: *mut c_void, out: *mut *mut rama_ctx) -> c_int;
    pub fn rama_ctx_destroy(ctx: *mut rama_ctx) -> c_int;
    pub fn rama_sync(ctx: *mut rama_ctx) -> c_int;
    pub fn rama_stream_query(ctx: *mut rama_ctx) -> c_int;
    pub fn rama_last_error() -> *const c_char;

    pub fn rama_alloc_f32(ctx: *mut rama_ctx, n: usize, out: *mut *mut f32) -> c_int;
    pub fn rama_upload_f32(ctx: *mut rama_ctx, host: *const f32, n: usize, out: *mut *mut f32) -> c_int;
    pub fn rama_download_f32(ctx: *mut rama_ctx, src: *const f32, n: usize, host: *mut f32) -> c_int;
    pub fn rama_free(ctx: *mut rama_ctx, p: *mut c_void) -> c_int;

    // one per Device<T> method (device/device.rs:4-21)
    pub fn rama_array_add(ctx: *mut rama_ctx, target: *mut f32, source: *const f32, n: usize) -> c_int;
    pub fn rama_array_mult(ctx: *mut rama_ctx, target: *mut f32, source: *const f32, n: usize) -> c_int;
    pub fn rama_sinu(ctx: *mut rama_ctx, o: *mut f32, n: usize) -> c_int;
    pub fn rama_copy_from_slice(ctx: *mut rama_ctx, target: *mut f32, source: *const f32, n: usize) -> c_int;
    pub fn rama_rmsnorm(ctx: *mut rama_ctx, o: *mut f32, x: *const f32, weight: *const f32, n: usize) -> c_int;
    pub fn rama_apply_position(ctx: *mut rama_ctx, q: *mut f32, k: *mut f32, pos_real: *const f32,
                               pos_img: *const f32, head_size: usize) -> c_int;
    pub fn rama_matmul(ctx: *mut rama_ctx, o: *mut f32, a: *const f32, b: *const f32,
                       width: usize, o_rows: usize, o_cols: usize) -> c_int;
    pub fn rama_softmax(ctx: *mut rama_ctx, x: *mut f32, n: usize) -> c_int;
    pub fn rama_multi_head_attention(ctx: *mut rama_ctx, xb: *mut f32, att: *mut f32, q: *const f32,
                                     key_cache: *const f32, value_cache: *const f32, layer: c_int, dim: c_int,
                                     pos: c_int, head_size: c_int, seq_len: c_int, n_heads: c_int) -> c_int;
    pub fn rama_sample_argmax(ctx: *mut rama_ctx, logits: *const f32, n: usize, next: *mut i32) -> c_int;
    pub fn rama_sample_topp(ctx: *mut rama_ctx, logits: *const f32, n: usize, temperature: f32,
                            topp: f32, u: f32, next: *mut i32) -> c_int;

    // optional fast path: forward() / generate() as single calls, same observable state
    pub fn rama_forward(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights,
                        s: *mut rama_run_state, token: c_int, pos: c_int) -> c_int;
    pub fn rama_prefill(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights,
                        s: *mut rama_run_state, tokens_host: *const i32, n_tokens: c_int, pos0: c_int) -> c_int;
    /// one decode step for up to 64 independent sequences (states: array of n_seq run states)
    pub fn rama_decode_batch(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights,
                             states: *const rama_run_state, tokens_host: *const i32, positions_host: *const i32,
                             n_seq: c_int) -> c_int;
    pub fn rama_decode_batch_begin(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, states: *const rama_run_state,
                                   tokens_host: *const i32, positions_host: *const i32, n_seq: c_int, max_steps: c_int) -> c_int;
    pub fn rama_decode_batch_begin_sampled(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, states: *const rama_run_state,
                                           tokens_host: *const i32, positions_host: *const i32, n_seq: c_int, max_steps: c_int,
                                           per_seq: *const rama_seq_sampling) -> c_int;
    pub fn rama_decode_batch_steps(ctx: *mut rama_ctx, n_steps: c_int) -> c_int;
    pub fn rama_decode_batch_tokens(ctx: *mut rama_ctx, out_host: *mut i32, max_per_seq: c_int, n_per_seq: *mut c_int) -> c_int;
    pub fn rama_generate(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights,
                         s: *mut rama_run_state, prompt_tokens_host: *const i32, n_prompt: c_int, steps: c_int,
                         temperature: f32, topp: f32, u: f32, out_tokens_host: *mut i32) -> c_int;
    pub fn rama_set_graph_mode(ctx: *mut rama_ctx, enabled: c_int) -> c_int;

    // resident model straight from a v0 checkpoint (mmap + one H2D copy)
    pub fn rama_model_load(ctx: *mut rama_ctx, path: *const c_char, out: *mut *mut rama_model) -> c_int;
    pub fn rama_model_config(m: *const rama_model, cfg: *mut rama_config) -> c_int;
    pub fn rama_model_weights(m: *const rama_model, w: *mut rama_weights) -> c_int;
    pub fn rama_model_free(ctx: *mut rama_ctx, m: *mut rama_model) -> c_int;
    pub fn rama_model_release_copies(ctx: *mut rama_ctx, m: *mut rama_model, mask: c_int) -> c_int;
    /// one pipeline stage's tensors only (layers [layer_begin, layer_end), embedding / classifier as flagged)
    pub fn rama_model_load_stage(ctx: *mut rama_ctx, path: *const c_char, stage: *const rama_stage,
                                 out: *mut *mut rama_model) -> c_int;

    // performance / parity knobs: "ref_order" = 1 switches every op to the CPU backend's rounding order
    // (bit-identical logits, for diffing against `cargo run --release`)
    pub fn rama_set_tuning(ctx: *mut rama_ctx, key: *const c_char, value: c_int) -> c_int;

    // layer pipeline over RCCL, one process per GPU (csrc/pipe.hip)
    pub fn rama_pipe_unique_id(id_out: *mut u8) -> c_int;                       // RAMA_PIPE_ID_BYTES = 128
    pub fn rama_pipe_create(ctx: *mut rama_ctx, id: *const u8, rank: c_int, world: c_int, out: *mut *mut rama_pipe) -> c_int;
    pub fn rama_pipe_destroy(pipe: *mut rama_pipe) -> c_int;
    pub fn rama_pipe_comm_info(pipe: *const rama_pipe, n_ranks: *mut c_int, rank: *mut c_int) -> c_int;
    pub fn rama_pipe_total_ticks(pipe: *const rama_pipe, plan: *const rama_pipe_plan) -> c_int;
    pub fn rama_pipe_run_ticks(pipe: *mut rama_pipe, cfg: *const rama_config, w: *const rama_weights,
                               states: *mut rama_run_state, tok_dev: *const *mut i32, stage: *const rama_stage,
                               plan: *const rama_pipe_plan, tick_from: c_int, tick_to: c_int) -> c_int;
    pub fn rama_pipe_exchange(pipe: *mut rama_pipe, send_x: *const f32, n_send_x: usize, send_x_peer: c_int,
                              recv_x: *mut f32, n_recv_x: usize, recv_x_peer: c_int,
                              send_tok: *const i32, send_tok_peer: c_int, recv_tok: *mut i32, recv_tok_peer: c_int) -> c_int;
    pub fn rama_pipe_item(plan: *const rama_pipe_plan, world: c_int, rank: c_int, tick: c_int, seq: *mut c_int, pos: *mut c_int) -> c_int;
    pub fn rama_pipe_plan_ticks(plan: *const rama_pipe_plan, world: c_int) -> c_int;
    pub fn rama_pipe_tick_plan(plan: *const rama_pipe_plan, world: c_int, rank: c_int, tick: c_int, out: *mut rama_pipe_tick) -> c_int;
    pub fn rama_pipe_last_error() -> *const c_char;

    // the rest of include/rama_hip.h, for hosts that want more than the trait: stage-wise forwards
    // (pipeline), the chained decode loop piece by piece, device-resident sampling, model helpers,
    // measurement.  tests/test_abi_and_host.py keeps this block and the header in step.
    pub fn rama_device_info(ctx: *mut rama_ctx, name: *mut c_char /* [64] */, compute_units: *mut c_int, hbm_bytes: *mut usize) -> c_int;
    pub fn rama_copy_h2d_f32(ctx: *mut rama_ctx, dst: *mut f32, host: *const f32, n: usize) -> c_int;
    pub fn rama_fill_synth(ctx: *mut rama_ctx, dst: *mut f32, n: usize, seed: u64, tag: u64, offset: u64, scale: f32, bias: f32) -> c_int;
    pub fn rama_forward_stage(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, s: *mut rama_run_state,
                              token: c_int, pos: c_int, stage: *const rama_stage) -> c_int;
    pub fn rama_forward_stage_devtok(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, s: *mut rama_run_state,
                                     token_dev: *const i32, pos: c_int, stage: *const rama_stage) -> c_int;
    pub fn rama_argmax_dev(ctx: *mut rama_ctx, logits: *const f32, n: usize, result_dev: *mut i32) -> c_int;
    pub fn rama_sample_topp_dev(ctx: *mut rama_ctx, logits: *const f32, n: usize, temperature: f32, topp: f32, u: f32,
                                result_dev: *mut i32) -> c_int;
    pub fn rama_sample_topp_batch_dev(ctx: *mut rama_ctx, logits: *const f32, ld: usize, n: usize, n_rows: c_int, temperature_host: *const f32,
                                      topp_host: *const f32, u_host: *const f32, result_dev: *mut i32) -> c_int;
    pub fn rama_generate_greedy(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, s: *mut rama_run_state,
                                prompt_tokens_host: *const i32, n_prompt: c_int, steps: c_int, out_tokens_host: *mut i32) -> c_int;
    pub fn rama_decode_begin(ctx: *mut rama_ctx, token: c_int, pos: c_int, forced_tokens_host: *const i32, n_forced: c_int) -> c_int;
    pub fn rama_decode_sampler(ctx: *mut rama_ctx, temperature: f32, topp: f32, u: f32) -> c_int;
    pub fn rama_decode_steps(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, s: *mut rama_run_state, n_steps: c_int) -> c_int;
    pub fn rama_decode_tokens(ctx: *mut rama_ctx, out_tokens_host: *mut i32, max_tokens: c_int, n_out: *mut c_int) -> c_int;
    pub fn rama_decode_batch_stream_poll(ctx: *mut rama_ctx, seq: c_int, from: c_int, out_tokens_host: *mut i32, max_tokens: c_int, n_ready: *mut c_int) -> c_int;
    pub fn rama_decode_stream_poll(ctx: *mut rama_ctx, from: c_int, out_tokens_host: *mut i32, max_tokens: c_int, n_ready: *mut c_int) -> c_int;
    pub fn rama_generate_stream(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, s: *mut rama_run_state,
                                prompt_tokens_host: *const i32, n_prompt: c_int, steps: c_int, temperature: f32, topp: f32, u: f32,
                                on_token: Option<unsafe extern "C" fn(user: *mut c_void, index: c_int, token: i32)>, user: *mut c_void,
                                out_tokens_host: *mut i32) -> c_int;
    pub fn rama_state_create(ctx: *mut rama_ctx, cfg: *const rama_config, n_local_layers: c_int, out: *mut rama_run_state) -> c_int;
    pub fn rama_state_free(ctx: *mut rama_ctx, s: *mut rama_run_state) -> c_int;
    pub fn rama_model_synth(ctx: *mut rama_ctx, cfg: *const rama_config, seed: u64, stage: *const rama_stage,
                            rope_real_host: *const f32, rope_imag_host: *const f32, out: *mut *mut rama_model) -> c_int;
    pub fn rama_model_save(ctx: *mut rama_ctx, model: *const rama_model, path: *const c_char) -> c_int;
    pub fn rama_model_bytes(m: *const rama_model) -> usize;
    pub fn rama_ref_expf(ctx: *mut rama_ctx, o: *mut f32, x: *const f32, n: usize) -> c_int;
    pub fn rama_timer_start(ctx: *mut rama_ctx) -> c_int;
    pub fn rama_timer_stop(ctx: *mut rama_ctx, elapsed_ms: *mut f32) -> c_int;
    pub fn rama_kprof_enable(ctx: *mut rama_ctx, kernel_id: c_int, max_records: c_int) -> c_int;
    pub fn rama_kprof_read(ctx: *mut rama_ctx, n_launches: *mut c_int, total_ms: *mut f64) -> c_int;

    // Q8_0 models (llama2.c version-2 checkpoints)
    pub fn rama_q8_model_load(ctx: *mut rama_ctx, path: *const c_char, out: *mut *mut rama_q8_model) -> c_int;
    pub fn rama_q8_model_synth(ctx: *mut rama_ctx, cfg: *const rama_config, group_size: c_int, seed: u64,
                               out: *mut *mut rama_q8_model) -> c_int;
    pub fn rama_q8_model_from_f32(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, group_size: c_int,
                                  out: *mut *mut rama_q8_model) -> c_int;
    pub fn rama_q8_model_config(m: *const rama_q8_model, cfg: *mut rama_config) -> c_int;
    pub fn rama_q8_model_weights(m: *const rama_q8_model, w: *mut rama_q8_weights) -> c_int;
    pub fn rama_q8_model_bytes(m: *const rama_q8_model) -> usize;
    pub fn rama_q8_model_free(ctx: *mut rama_ctx, m: *mut rama_q8_model) -> c_int;
    pub fn rama_q8_quantize(ctx: *mut rama_ctx, x: *const f32, n: usize, group_size: c_int, q: *mut i8, s: *mut f32) -> c_int;
    pub fn rama_q8_matmul(ctx: *mut rama_ctx, o: *mut f32, wq: *const i8, ws: *const f32, xq: *const i8, xs: *const f32,
                          n: usize, d: usize, group_size: c_int) -> c_int;
    pub fn rama_q8_forward(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, s: *mut rama_run_state,
                           token: c_int, pos: c_int) -> c_int;
    pub fn rama_q8_generate(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, s: *mut rama_run_state,
                            prompt_tokens_host: *const i32, n_prompt: c_int, steps: c_int, temperature: f32, topp: f32, u: f32,
                            out_tokens_host: *mut i32) -> c_int;
    pub fn rama_q8_matmul_batch(ctx: *mut rama_ctx, o: *mut f32, wq: *const i8, ws: *const f32, xq: *const i8, xs: *const f32,
                                n: usize, d: usize, group_size: c_int, n_tok: c_int) -> c_int;
    pub fn rama_q8_product_path(n: usize, group_size: c_int, n_tok: c_int, aligned16: c_int) -> c_int;
    pub fn rama_q8_batch_shape_ok(cfg: *const rama_config) -> c_int;
    pub fn rama_q8_prefill(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, s: *mut rama_run_state,
                           tokens_host: *const i32, n_tokens: c_int, pos0: c_int) -> c_int;
    pub fn rama_q8_decode_batch(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, states: *const rama_run_state,
                                tokens_host: *const i32, positions_host: *const i32, n_seq: c_int) -> c_int;
    pub fn rama_q8_decode_batch_begin(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, states: *const rama_run_state,
                                      tokens_host: *const i32, positions_host: *const i32, n_seq: c_int, max_steps: c_int,
                                      per_seq: *const rama_q8_seq_plan) -> c_int;
    pub fn rama_q8_decode_batch_steps(ctx: *mut rama_ctx, n_steps: c_int) -> c_int;
    pub fn rama_q8_decode_batch_tokens(ctx: *mut rama_ctx, out_host: *mut i32, max_per_seq: c_int, n_per_seq: *mut i32) -> c_int;
    pub fn rama_q8_decode_batch_stream_poll(ctx: *mut rama_ctx, seq: c_int, from: c_int, out_tokens_host: *mut i32, max_tokens: c_int,
                                            n_ready: *mut c_int, finished: *mut c_int) -> c_int;
    // the serving chain (continuous batching): slots admitted and finished while the chain runs
    pub fn rama_q8_serve_begin(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, n_slots: c_int, max_rows: c_int,
                               max_new_cap: c_int) -> c_int;
    pub fn rama_q8_serve_admit(ctx: *mut rama_ctx, slot: c_int, state: *const rama_run_state, context_host: *const i32, n_context: c_int,
                               plan: *const rama_q8_serve_plan) -> c_int;
    pub fn rama_q8_serve_admit_at(ctx: *mut rama_ctx, slot: c_int, state: *const rama_run_state, context_host: *const i32, n_context: c_int,
                                  n_cached: c_int, plan: *const rama_q8_serve_plan) -> c_int;
    pub fn rama_q8_kv_fork(ctx: *mut rama_ctx, cfg: *const rama_config, src: *const rama_run_state, dsts: *const rama_run_state, n_dst: c_int,
                           n_rows: c_int) -> c_int;
    pub fn rama_q8_serve_steps(ctx: *mut rama_ctx, n_steps: c_int) -> c_int;
    pub fn rama_q8_serve_poll(ctx: *mut rama_ctx, slot: c_int, from: c_int, out_tokens_host: *mut i32, max_tokens: c_int,
                              n_ready: *mut c_int, finished: *mut c_int, generation: *mut c_int) -> c_int;
    pub fn rama_q8_serve_tokens(ctx: *mut rama_ctx, slot: c_int, out_host: *mut i32, max_tokens: c_int, n: *mut c_int) -> c_int;
    pub fn rama_q8_serve_stats(ctx: *mut rama_ctx, out: *mut rama_q8_serve_report) -> c_int;
    pub fn rama_q8_serve_plan_step(slots: *const rama_q8_serve_slot, n_slots: c_int, max_rows: c_int, rows_out: *mut rama_q8_serve_row,
                                   slots_after: *mut rama_q8_serve_slot) -> c_int;
    pub fn rama_q8_serve_end(ctx: *mut rama_ctx) -> c_int;
    // the serving chain of an fp32 model in parity mode: the same arguments and records, rama_weights for the model
    pub fn rama_serve_begin(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, n_slots: c_int, max_rows: c_int,
                            max_new_cap: c_int) -> c_int;
    pub fn rama_serve_admit(ctx: *mut rama_ctx, slot: c_int, state: *const rama_run_state, context_host: *const i32, n_context: c_int,
                            plan: *const rama_q8_serve_plan) -> c_int;
    pub fn rama_serve_admit_at(ctx: *mut rama_ctx, slot: c_int, state: *const rama_run_state, context_host: *const i32, n_context: c_int,
                               n_cached: c_int, plan: *const rama_q8_serve_plan) -> c_int;
    // ... with drafts in the rows no slot wants: the Q8 spec serving entries' arguments and records
    pub fn rama_serve_begin_spec(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, n_slots: c_int, max_rows: c_int,
                                 max_new_cap: c_int, n_draft_cap: c_int, hint_cap: c_int) -> c_int;
    pub fn rama_serve_admit_spec(ctx: *mut rama_ctx, slot: c_int, state: *const rama_run_state, context_host: *const i32, n_context: c_int,
                                 n_cached: c_int, plan: *const rama_q8_serve_plan, spec: *const rama_q8_serve_spec) -> c_int;
    pub fn rama_serve_spec_stats(ctx: *mut rama_ctx, out: *mut rama_q8_serve_spec_report) -> c_int;
    pub fn rama_serve_steps(ctx: *mut rama_ctx, n_steps: c_int) -> c_int;
    pub fn rama_serve_poll(ctx: *mut rama_ctx, slot: c_int, from: c_int, out_tokens_host: *mut i32, max_tokens: c_int,
                           n_ready: *mut c_int, finished: *mut c_int, generation: *mut c_int) -> c_int;
    pub fn rama_serve_tokens(ctx: *mut rama_ctx, slot: c_int, out_host: *mut i32, max_tokens: c_int, n: *mut c_int) -> c_int;
    pub fn rama_serve_stats(ctx: *mut rama_ctx, out: *mut rama_q8_serve_report) -> c_int;
    pub fn rama_serve_end(ctx: *mut rama_ctx) -> c_int;
    // the speculative chain: one sequence, n-gram lookup drafts verified in one pass; _draft and _accept are host-only
    pub fn rama_q8_spec_begin(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, state: *const rama_run_state,
                              context_host: *const i32, n_context: c_int, plan: *const rama_q8_spec_plan) -> c_int;
    pub fn rama_q8_spec_steps(ctx: *mut rama_ctx, n_steps: c_int) -> c_int;
    pub fn rama_q8_spec_poll(ctx: *mut rama_ctx, from: c_int, out_tokens_host: *mut i32, max_tokens: c_int, n_ready: *mut c_int,
                             finished: *mut c_int) -> c_int;
    pub fn rama_q8_spec_tokens(ctx: *mut rama_ctx, out_host: *mut i32, max_tokens: c_int, n: *mut c_int) -> c_int;
    pub fn rama_q8_spec_stats(ctx: *mut rama_ctx, out: *mut rama_q8_spec_report) -> c_int;
    pub fn rama_q8_spec_end(ctx: *mut rama_ctx) -> c_int;
    pub fn rama_q8_spec_draft(hint: *const i32, n_hint: c_int, seq: *const i32, l: c_int, n_draft: c_int, ngram: c_int, room: c_int,
                              drafts_out: *mut i32) -> c_int;
    pub fn rama_q8_spec_accept(drafts: *const i32, n_d: c_int, picks: *const i32, stop_token: c_int, remaining: c_int,
                               finished: *mut c_int) -> c_int;
    // ... with drafts from a small Q8 model over the same vocabulary instead of the lookup
    pub fn rama_q8_spec_begin_model(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, state: *const rama_run_state,
                                    dcfg: *const rama_config, dw: *const rama_q8_weights, dstate: *const rama_run_state,
                                    context_host: *const i32, n_context: c_int, plan: *const rama_q8_spec_plan) -> c_int;
    pub fn rama_q8_spec_model_stats(ctx: *mut rama_ctx, out: *mut rama_q8_spec_model_report) -> c_int;
    // ... with tree drafts: up to four continuations of the tail n-gram in one pass; _tree_draft and _tree_accept are host-only
    pub fn rama_q8_spec_begin_tree(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, state: *const rama_run_state,
                                   context_host: *const i32, n_context: c_int, plan: *const rama_q8_spec_plan, n_branch: c_int, n_rows: c_int) -> c_int;
    pub fn rama_q8_spec_tree_stats(ctx: *mut rama_ctx, out: *mut rama_q8_spec_tree_report) -> c_int;
    pub fn rama_q8_spec_tree_draft(hint: *const i32, n_hint: c_int, seq: *const i32, l: c_int, n_draft: c_int, ngram: c_int, room: c_int,
                                   n_branch: c_int, n_rows: c_int, tok_out: *mut i32, parent_out: *mut i32, depth_out: *mut i32) -> c_int;
    pub fn rama_q8_spec_tree_accept(tok: *const i32, parent: *const i32, m: c_int, picks: *const i32, stop_token: c_int, remaining: c_int,
                                    path_out: *mut i32, a_out: *mut c_int, finished: *mut c_int) -> c_int;
    pub fn rama_q8_tree_forward(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, state: *const rama_run_state,
                                tokens_host: *const i32, parent_host: *const i32, n_rows: c_int, pos0: c_int, logits_dev: *mut f32) -> c_int;
    pub fn rama_q8_tree_commit(ctx: *mut rama_ctx, cfg: *const rama_config, state: *const rama_run_state, path_host: *const i32, n_path: c_int,
                               pos0: c_int) -> c_int;
    // ... with a tree whose branches are the draft model's second and third choices; _shape and _candidates are host-only
    pub fn rama_q8_spec_begin_model_tree(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, state: *const rama_run_state,
                                         dcfg: *const rama_config, dw: *const rama_q8_weights, dstate: *const rama_run_state,
                                         context_host: *const i32, n_context: c_int, plan: *const rama_q8_spec_plan, n_branch: c_int,
                                         n_rows: c_int) -> c_int;
    pub fn rama_q8_spec_model_tree_shape(cap: c_int, n_branch: c_int, n_rows: c_int, parent_out: *mut i32, depth_out: *mut i32,
                                         rank_out: *mut i32) -> c_int;
    pub fn rama_q8_spec_model_tree_candidates(logits_host: *const f32, vocab_size: c_int, rank0_token: c_int, n: c_int, out: *mut i32) -> c_int;
    pub fn rama_q8_spec_model_tree_last(ctx: *mut rama_ctx, tok: *mut i32, parent: *mut i32, depth: *mut i32, picks: *mut i32, path: *mut i32,
                                        m: *mut c_int, a: *mut c_int) -> c_int;
    // speculation inside the serving chain: a DECODE slot's drafts in the rows no slot wants; _plan_step is host-only
    pub fn rama_q8_serve_begin_spec(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, n_slots: c_int, max_rows: c_int,
                                    max_new_cap: c_int, n_draft_cap: c_int, hint_cap: c_int) -> c_int;
    pub fn rama_q8_serve_admit_spec(ctx: *mut rama_ctx, slot: c_int, state: *const rama_run_state, context_host: *const i32, n_context: c_int,
                                    n_cached: c_int, plan: *const rama_q8_serve_plan, spec: *const rama_q8_serve_spec) -> c_int;
    pub fn rama_q8_serve_spec_plan_step(slots: *const rama_q8_serve_slot, n_slots: c_int, max_rows: c_int, want: *const i32,
                                        rows_out: *mut rama_q8_serve_row, granted_out: *mut i32) -> c_int;
    pub fn rama_q8_serve_spec_stats(ctx: *mut rama_ctx, out: *mut rama_q8_serve_spec_report) -> c_int;
    // model drafts inside the serving chain: a small Q8 model drafts for every slot in the idle rows; _plan_step is host-only
    pub fn rama_q8_serve_begin_model(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_q8_weights, dcfg: *const rama_config,
                                     dw: *const rama_q8_weights, n_slots: c_int, max_rows: c_int, max_new_cap: c_int, n_draft_cap: c_int) -> c_int;
    pub fn rama_q8_serve_admit_model(ctx: *mut rama_ctx, slot: c_int, state: *const rama_run_state, dstate: *const rama_run_state,
                                     context_host: *const i32, n_context: c_int, n_cached: c_int, plan: *const rama_q8_serve_plan,
                                     n_draft: c_int) -> c_int;
    pub fn rama_q8_serve_model_plan_step(slots: *const rama_q8_serve_slot, n_slots: c_int, max_rows: c_int, seq_len: c_int, n_draft: *const i32,
                                         draft_cursor: *const i32, n_passes: c_int, rows_out: *mut rama_q8_serve_row, want_out: *mut i32,
                                         granted_out: *mut i32, draft_rows_out: *mut rama_q8_serve_row) -> c_int;
    pub fn rama_q8_serve_model_stats(ctx: *mut rama_ctx, out: *mut rama_q8_serve_model_report) -> c_int;
    pub fn rama_serve_begin_model(ctx: *mut rama_ctx, cfg: *const rama_config, w: *const rama_weights, dcfg: *const rama_config,
                                  dw: *const rama_q8_weights, n_slots: c_int, max_rows: c_int, max_new_cap: c_int, n_draft_cap: c_int) -> c_int;
    pub fn rama_serve_admit_model(ctx: *mut rama_ctx, slot: c_int, state: *const rama_run_state, dstate: *const rama_run_state,
                                  context_host: *const i32, n_context: c_int, n_cached: c_int, plan: *const rama_q8_serve_plan,
                                  n_draft: c_int) -> c_int;
    pub fn rama_serve_model_stats(ctx: *mut rama_ctx, out: *mut rama_q8_serve_model_report) -> c_int;
    // cancel in both serving chains: the slots of the list that are still live end with the finished word RAMA_SERVE_CANCELLED (2)
    pub fn rama_q8_serve_cancel(ctx: *mut rama_ctx, slots: *const i32, n: c_int) -> c_int;
    pub fn rama_serve_cancel(ctx: *mut rama_ctx, slots: *const i32, n: c_int) -> c_int;
}

#[repr(C)] pub struct rama_pipe { _p: [u8; 0] }
#[repr(C)] #[derive(Clone, Copy)]
pub struct rama_stage { pub layer_begin: i32, pub layer_end: i32, pub do_embed: i32, pub do_cls: i32 }
#[repr(C)]
pub struct rama_pipe_plan {
    pub n_seq: i32, pub n_pos: i32, pub wrap: i32,
    pub prompt: *const i32, pub n_prompt: i32,
    pub temperature: f32, pub topp: f32, pub u: f32,
    pub out_tokens_dev: *mut i32,
}

/// one tick of one rank of the layer pipeline, decided (include/rama_hip.h rama_pipe_tick): what rama_pipe_run_ticks executes
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct rama_pipe_tick {
    pub on: i32, pub seq: i32, pub pos: i32, pub pos_wrapped: i32, pub token_kind: i32, pub token: i32,
    pub samples: i32,
    pub send_kind: i32, pub send_seq: i32, pub send_peer: i32,
    pub recv_kind: i32, pub recv_seq: i32, pub recv_peer: i32, pub recv_pos: i32,
}
