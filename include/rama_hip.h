/*
 * rama_hip.h -- C ABI of the MI355X (gfx950) backend for oliverhu/rama's decode path.
 *
 * This is the drop-in boundary: exactly what a Rust `impl Device<HipSlice> for Hip`
 * (reference trait: engine/src/device/device.rs:3-24) would bind over `extern "C"`,
 * in place of the reference's cudarc/NVRTC/cuBLAS backend (engine/src/device/gpu.rs,
 * engine/src/device/math.cu, engine/src/transformer/hbm.rs).  Plain pointers and
 * sizes only; no C++ / torch types.  See INTEGRATION.md for the Rust-side stub.
 *
 * Conventions
 *  - Every `float*` / `const float*` argument is a DEVICE pointer already offset by
 *    the caller's View.range.start (reference: `cudaview()`, gpu.rs:51-69), except
 *    where the name says `host`.
 *  - All work is enqueued on the context's HIP stream and is asynchronous unless the
 *    function copies to host memory (those synchronise, like cudarc's *_sync_* calls).
 *  - Return value: 0 = ok; > 0 = a hipError_t; < 0 = RAMA_E*.  The reference trait has
 *    no Result and unwraps every driver call (panic); a host wrapper that wants that
 *    behaviour aborts on non-zero.  rama_last_error() gives a message for the calling
 *    thread's last failure.
 *  - Thread-safety: one context = one stream; calls on one context must be serialised
 *    by the caller.  Distinct contexts / run states may be used from distinct threads
 *    over shared read-only weights (reference: one RunState per request, lib.rs:134-147).
 */
#ifndef RAMA_HIP_H
#define RAMA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAMA_OK        0
#define RAMA_EINVAL   (-1)  /* bad argument (null pointer, width % 4 != 0, pos >= seq_len ...) */
#define RAMA_EUNSUP   (-2)  /* shape the reference path does not support (n_kv_heads != n_heads) */
#define RAMA_EIO      (-3)  /* checkpoint file problem */
#define RAMA_ENOMEM   (-4)

typedef struct rama_ctx rama_ctx;
typedef struct rama_model rama_model;

/* ---------------------------------------------------------------- lifecycle
 * replaces GPU::new (gpu.rs:213-234: device 0, NVRTC compile, cuBLAS handle).
 * `hip_stream` may be NULL (the context creates its own non-blocking stream) or an
 * existing hipStream_t to adopt (e.g. a framework's current stream). */
int  rama_ctx_create(int device, void *hip_stream, rama_ctx **out);
int  rama_ctx_destroy(rama_ctx *ctx);
int  rama_sync(rama_ctx *ctx);                       /* hipStreamSynchronize; also reports an in-kernel hand-off that timed out (one-launch stage, attention+Wo) */
/* Non-blocking: 0 = everything enqueued on the context's stream has run, 1 = still running, anything else = the
 * stream has failed (what a host loop polling rama_decode_stream_poll / rama_decode_batch_stream_poll ends on). */
int  rama_stream_query(rama_ctx *ctx);
const char *rama_last_error(void);
/* name (<= 63 chars), compute units, total HBM bytes of the context's device */
int  rama_device_info(rama_ctx *ctx, char name[64], int *compute_units, size_t *hbm_bytes);

/* ---------------------------------------------------------------- memory
 * replaces hbm.rs:14-16 `allocate` (= htod_sync_copy) and dtoh_sync_copy_into
 * (gpu.rs:196-209 to_cpu, hbm.rs:38-51 into_state). */
int  rama_alloc_f32(rama_ctx *ctx, size_t n, float **out);            /* zero-filled, cf. ram.rs:10-21 */
int  rama_upload_f32(rama_ctx *ctx, const float *host, size_t n, float **out);  /* alloc + H2D */
int  rama_copy_h2d_f32(rama_ctx *ctx, float *dst, const float *host, size_t n);
int  rama_download_f32(rama_ctx *ctx, const float *src, size_t n, float *host);
int  rama_free(rama_ctx *ctx, void *device_ptr);

/* ---------------------------------------------------------------- Device<T> ops, 1:1
 * engine/src/device/device.rs:3-24; arithmetic follows the CPU backend
 * (engine/src/device/cpu.rs), never math.cu (which is buggy: SURVEY.md section 2.1). */
int  rama_array_add(rama_ctx *ctx, float *target, const float *source, size_t n);   /* device.rs:4  cpu.rs:16-21 */
int  rama_array_mult(rama_ctx *ctx, float *target, const float *source, size_t n);  /* device.rs:5  cpu.rs:59-64 */
int  rama_sinu(rama_ctx *ctx, float *o, size_t n);                                   /* device.rs:6  cpu.rs:54-57 */
int  rama_copy_from_slice(rama_ctx *ctx, float *target, const float *source, size_t n); /* device.rs:9 cpu.rs:66-72 */
int  rama_rmsnorm(rama_ctx *ctx, float *o, const float *x, const float *weight, size_t n); /* device.rs:10 cpu.rs:99-117 */
/* device.rs:12 cpu.rs:74-97: one head of q and k rotated in place by (pos_real[i], pos_img[i]) */
int  rama_apply_position(rama_ctx *ctx, float *q, float *k, const float *pos_real,
                         const float *pos_img, size_t head_size);
/* device.rs:13 cpu.rs:127-153: o[r*o_cols + c] = sum_k a[r*width + k] * b[k*o_cols + c];
 * a = weight matrix [o_rows, width] row-major, b = activations.  width % 4 != 0 ->
 * RAMA_EINVAL (the reference CPU body panics there). */
int  rama_matmul(rama_ctx *ctx, float *o, const float *a, const float *b,
                 size_t width, size_t o_rows, size_t o_cols);
int  rama_softmax(rama_ctx *ctx, float *x, size_t n);                                /* device.rs:14 cpu.rs:119-125 */
/* device.rs:7-8 cpu.rs:23-52; flat argument list as math.cu:94 calculate_attention +
 * math.cu:72 update_xb take it.  key_cache/value_cache are the full [L, seq_len, dim] buffers. */
int  rama_multi_head_attention(rama_ctx *ctx, float *xb, float *att, const float *q,
                               const float *key_cache, const float *value_cache,
                               int layer, int dim, int pos, int head_size, int seq_len, int n_heads);
/* device.rs:16 Device::sample, T == 0 leg (cpu.rs:163-167): argmax on the device, ties ->
 * last maximal index; only the 4-byte result crosses PCIe (reference GPU path clones and
 * downloads all logits per token, gpu.rs:153). */
int  rama_sample_argmax(rama_ctx *ctx, const float *logits, size_t n, int32_t *next_host);
/* T != 0 leg (cpu.rs:168-177, infer.rs:55-85): temperature scale (only if T < 1), softmax,
 * top-p.  `u` = the uniform draw; the reference re-seeds ChaCha20 every call (cpu.rs:161-162,
 * gpu.rs:151-152) so its draw is one constant.  Runs on the device (rama_sample_topp_dev below);
 * only the 4-byte result crosses PCIe.  RAMA_EINVAL when no probability exceeds the cutoff. */
int  rama_sample_topp(rama_ctx *ctx, const float *logits, size_t n, float temperature,
                      float topp, float u, int32_t *next_host);

/* ---------------------------------------------------------------- model + state
 * engine/src/transformer/mod.rs:128-138 */
typedef struct {
    int32_t dim, hidden_dim, n_layers, n_heads, n_kv_heads, vocab_size, seq_len;
    int32_t shared_weight;
} rama_config;

/* engine/src/transformer/state.rs:53-74; device pointers.  For a pipeline stage the
 * per-layer tensors hold only layers [layer_begin, layer_end) (index = layer - layer_begin);
 * tensors a stage does not own are NULL. */
typedef struct {
    const float *token_embedding_table;
    const float *rms_att_weight, *rms_ffn_weight;
    const float *wq, *wk, *wv, *wo, *w1, *w2, *w3;
    const float *rms_final_weight;
    const float *freq_cis_real, *freq_cis_imag;
    const float *wcls;            /* == token_embedding_table when shared (state.rs:111-117) */
} rama_weights;

/* engine/src/transformer/state.rs:3-17, sized as ram.rs:7-23 (caches: [n_local_layers, seq_len, dim]) */
typedef struct {
    float *x, *xb, *xb2, *hb, *hb2, *q, *k, *v, *att, *logits, *key_cache, *value_cache;
} rama_run_state;

typedef struct {
    int32_t layer_begin, layer_end;   /* this stage's layers */
    int32_t do_embed;                 /* 1: gather x from token_embedding_table (infer.rs:13) */
    int32_t do_cls;                   /* 1: final rmsnorm + classifier (infer.rs:49-51) */
} rama_stage;

/* llama2.c v0 checkpoint (header mod.rs:141-166, tensor order ram.rs:28-51): mmap the file,
 * one hipMalloc for the tensor blob, one staged H2D copy (replaces 6.7 G four-byte reads,
 * utils/read.rs:25-33, + 14 htod_sync_copy, hbm.rs:55-90). */
int  rama_model_load(rama_ctx *ctx, const char *path, rama_model **out);
/* the same for one pipeline stage: only the stage's layers (and the embedding / classifier tensors it
 * needs) are copied to this device */
int  rama_model_load_stage(rama_ctx *ctx, const char *path, const rama_stage *stage, rama_model **out);
/* Synthetic weights of a given shape, generated in HBM by an integer-hash fill kernel
 * (bit-identical to oracle_fill_synth); only layers of `stage` are materialised.
 * rope_real/rope_imag: host tables [seq_len, head_size/2] or NULL (computed here). */
int  rama_model_synth(rama_ctx *ctx, const rama_config *cfg, uint64_t seed, const rama_stage *stage,
                      const float *rope_real_host, const float *rope_imag_host, rama_model **out);
/* Write a whole model as a llama2.c v0 file -- the format engine/export/export.py:75-127
 * (legacy_export) produces and transformer/ram.rs:28-51 reads, so upstream Rama loads it too
 * (SURVEY section 8 row f2).  RAMA_EINVAL for a model that holds only a pipeline stage. */
int  rama_model_save(rama_ctx *ctx, const rama_model *model, const char *path);
/* A model also keeps W1 and W3 row-interleaved per layer (row i of W1, then row i of W3: +11.5 GB at
 * llama2-7B): the fused decode path finds that copy by the addresses of w1 / w3 in rama_weights and
 * streams ONE contiguous block per workgroup; weights uploaded tensor by tensor (rama_upload_f32) take
 * the two-tensor kernel.  rama_set_tuning "w13i" = 0 turns the lookup off.
 * And every matrix once more in MFMA tile order (+27 GB at llama2-7B; skipped when fewer than 16 GiB of
 * HBM would remain, or with RAMA_NO_TILED=1 in the environment): rama_prefill / rama_decode_batch read
 * that copy -- one contiguous 1-KiB weight read per wave -- found the same way ("tiled" = 0: off).
 * rama_model_bytes counts the checkpoint tensors only.
 * The tile-order and the chain-order copies are made on FIRST USE (rama_prefill / rama_decode_batch*; "ref_order" != 0):
 * that call allocates and synchronises the device, so it must not sit inside the caller's own stream capture --
 * a caller that captures sets RAMA_EAGER_COPIES=1 in the environment (the copies are then made by rama_model_load /
 * rama_model_synth) or makes one warm-up call first.  rama_model_release_copies gives them back. */
int  rama_model_config(const rama_model *m, rama_config *cfg);
int  rama_model_weights(const rama_model *m, rama_weights *w);
size_t rama_model_bytes(const rama_model *m);
/* Give the derived copies back (they are made again on the next call that wants them): mask 1 = the chain-order
 * copy parity mode streams, 2 = the tile-order copy of the token-batch passes, 3 = both -- llama2-7B: 92 GB -> 38 GB.
 * Synchronises the context's stream and drops its captured graphs (they hold the copies' addresses). */
int  rama_model_release_copies(rama_ctx *ctx, rama_model *m, int mask);
int  rama_model_free(rama_ctx *ctx, rama_model *m);

int  rama_state_create(rama_ctx *ctx, const rama_config *cfg, int n_local_layers, rama_run_state *out);
int  rama_state_free(rama_ctx *ctx, rama_run_state *s);

/* bit-exact device twin of oracle_fill_synth: dst[i] = bias + (float)(ih4(i+offset) - 131070) * scale */
int  rama_fill_synth(rama_ctx *ctx, float *dst, size_t n, uint64_t seed, uint64_t tag,
                     uint64_t offset, float scale, float bias);

/* ---------------------------------------------------------------- fused decode path
 * engine/src/transformer/infer.rs:8-53 forward(cfg, wv, rsv, token, pos, device): the same
 * values in logits / key_cache / value_cache / x (per-layer residual), computed with fused
 * launches (rmsnorm folded into the following matvec, RoPE + cache append into the QKV
 * epilogue, SiLU*gate into W1/W3, residual adds into Wo / W2).  Scratch buffers the fusion
 * makes dead (xb2, hb2, and x/xb after the final norm) are not written; the 1:1 ops above
 * reproduce the full choreography. */
int  rama_forward(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w,
                  rama_run_state *s, int token, int pos);
int  rama_forward_stage(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w,
                        rama_run_state *s, int token, int pos, const rama_stage *stage);

/* Batched-prompt prefill (no reference counterpart): the same state as
 * n_tokens calls rama_forward(tokens[i], pos0 + i) -- KV-cache rows pos0..pos0+n-1 of every layer,
 * residual x and logits of the LAST position -- with the weights streamed once per 128 positions (64 when the
 * weights are not a resident rama_model's: the 128-position kernels read the model's tile-order copies), as
 * dense fp32 GEMMs on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32, csrc/prefill_mfma.hpp).
 * dim or hidden_dim not a multiple of 16: falls back to one rama_forward per token.
 * Parity mode ("ref_order" = 1) on a resident model: the positions go through token-batch kernels in the reference's
 * rounding order, 32 per weight pass, the last one through rama_forward -- cache rows, logits and run state are
 * bit for bit those of one rama_forward per position ("prefill_chain" = 0 gives exactly that loop). */
int  rama_prefill(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w, rama_run_state *s,
                  const int32_t *tokens_host, int n_tokens, int pos0);

/* One decode step for up to 128 INDEPENDENT sequences (64 without a resident rama_model's tile-order copies; the
 * server's concurrent requests), every
 * weight row streamed once for all of them (no reference counterpart; same MFMA kernels as the
 * prefill).  states[i] is sequence i's run state; afterwards it holds what
 * rama_forward(token_i, pos_i) would have left in it: the appended cache rows and the logits
 * (x / xb / q ... scratch is not maintained).  Sequences may sit at different positions; two entries
 * must not share a state.  Parity mode ("ref_order" = 1) on a resident model: 32 sequences per weight pass through the
 * chain-order token-batch kernels, every sequence's logits and cache rows bit for bit those of its own rama_forward. */
int  rama_decode_batch(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w,
                       const rama_run_state *states, const int32_t *tokens_host,
                       const int32_t *positions_host, int n_seq);
/* The same pass chained on the device: rama_decode_batch_begin uploads every sequence's (token, position) once;
 * each step of rama_decode_batch_steps ends with one argmax per sequence (Device::sample at temperature 0, ties to the
 * last index) that writes the sequence's next token and advances its position in device memory, so a step needs no
 * host round trip and -- in graph mode -- is ONE hipGraph replay.  rama_decode_batch_tokens downloads what the
 * sequences produced, out_host[s * max_per_seq + k] = token k of sequence s.  position_i + max_steps <= seq_len.
 * (Fast mode only; the logits stay in the pass's scratch, states[i].logits is not written.) */
int  rama_decode_batch_begin(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w,
                             const rama_run_state *states, const int32_t *tokens_host,
                             const int32_t *positions_host, int n_seq, int max_steps);
int  rama_decode_batch_steps(rama_ctx *ctx, int n_steps);
int  rama_decode_batch_tokens(rama_ctx *ctx, int32_t *out_host, int max_per_seq, int *n_per_seq);
/* tokens `from`.. that sequence `seq` of the chained batch has produced SO FAR, without touching the stream (a host-visible
 * ring per sequence, as rama_decode_stream_poll): a server hands each request its tokens as they appear. */
int  rama_decode_batch_stream_poll(rama_ctx *ctx, int seq, int from, int32_t *out_tokens_host, int max_tokens, int *n_ready);
/* The chained batch with sampling and forced prompts (the server's requests: each samples by default and has its own prompt).
 * Sequence i runs generate()'s loop (mod.rs:169-206) from its own (token, position):
 *   next = pos < n_forced ? forced[pos] : Device::sample(logits, temperature, topp, u)
 * -- the absolute-position rule of rama_decode_begin, so sequences that all start at (1, 0) with their prompts give exactly the
 * reference's generations; temperature 0 is the argmax, a sample with no kept entry gives token 0 as in rama_decode_steps.  Every
 * step ends in the batched top-p sampler (rama_sample_topp_batch_dev); forced and temperature-0 rows skip its sorting work.
 * The records and forced lists are copied to the device here; rama_decode_batch_steps / _tokens / _stream_poll drive the chain
 * as they drive rama_decode_batch_begin's, and a step in graph mode is still one hipGraph replay.  Same restrictions as
 * rama_decode_batch_begin (fast mode: RAMA_EUNSUP otherwise; 1..128 sequences), and vocab_size <= 32768 (RAMA_EUNSUP).
 * RAMA_EINVAL, the previous chain untouched, for temperature < 0, topp outside [0, 1], u outside [0, 1), n_forced < 0 or a
 * forced token outside the vocabulary. */
typedef struct { float temperature, topp, u; const int32_t *forced; int32_t n_forced; } rama_seq_sampling;
int  rama_decode_batch_begin_sampled(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w,
                                     const rama_run_state *states, const int32_t *tokens_host,
                                     const int32_t *positions_host, int n_seq, int max_steps,
                                     const rama_seq_sampling *per_seq);

/* Layer-pipeline stage variants (no reference counterpart: the reference is single-device).
 * The token id is read from / written to DEVICE memory, so a stage boundary is one RCCL
 * send/recv of x[dim] (and of one int32 from the last stage back to the first) with no host
 * round trip.  token_dev may be NULL for a stage that does not embed. */
int  rama_forward_stage_devtok(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w,
                               rama_run_state *s, const int32_t *token_dev, int pos,
                               const rama_stage *stage);
int  rama_argmax_dev(rama_ctx *ctx, const float *logits, size_t n, int32_t *result_dev);

/* ---------------------------------------------------------------- layer pipeline over RCCL (csrc/pipe.hip)
 * One process per GPU; rank r owns a contiguous layer range -- as even as possible, the first L mod N ranks
 * one layer more -- (rama_model_load_stage / rama_model_synth with a stage), n_seq >= N sequences in flight.  Rank 0 obtains a unique id and ships its
 * RAMA_PIPE_ID_BYTES bytes to the other ranks by any side channel (a file, an environment variable,
 * a torch.distributed / MPI broadcast); every rank then creates its end.  RCCL is loaded with dlopen on
 * first use.  All exchanges are enqueued on the context's stream. */
#define RAMA_PIPE_ID_BYTES 128
typedef struct rama_pipe rama_pipe;
int  rama_pipe_unique_id(void *id_out /* RAMA_PIPE_ID_BYTES */);
int  rama_pipe_create(rama_ctx *ctx, const void *id_bytes, int rank, int world, rama_pipe **out);
int  rama_pipe_destroy(rama_pipe *pipe);
/* the communicator's own count of ranks and this end's rank in it (ncclCommCount / ncclCommUserRank) */
int  rama_pipe_comm_info(const rama_pipe *pipe, int *n_ranks, int *rank);
/* One grouped exchange (ncclGroupStart .. ncclGroupEnd): each of the four legs is skipped when its
 * buffer is NULL.  x legs carry float[n], token legs one int32; peers are ranks of the pipe. */
int  rama_pipe_exchange(rama_pipe *pipe, const float *send_x, size_t n_send_x, int send_x_peer,
                        float *recv_x, size_t n_recv_x, int recv_x_peer,
                        const int32_t *send_tok, int send_tok_peer, int32_t *recv_tok, int recv_tok_peer);
/* The schedule: item j = (slot j % S, position j / S), S = max(n_seq, world) slots per round (slots
 * beyond n_seq idle); rank r computes item tick - r at each tick (BOS at position 0, the forced
 * prompt tokens next, mod.rs:182-191, then the token the last rank sampled: argmax at temperature 0,
 * else the device top-p sampler), then exchanges: x[dim] to rank r + 1, the sampled id from the last
 * rank to rank 0.  wrap > 0: a sequence that reaches position `wrap` starts a new generation at 0 in
 * the same slot. */
typedef struct {
    int32_t n_seq, n_pos, wrap;
    const int32_t *prompt;        /* host: forced prompt tokens, the same for every sequence */
    int32_t n_prompt;
    float temperature, topp, u;   /* Device::sample on the last rank (u = the reference's constant draw) */
    int32_t *out_tokens_dev;      /* rank 0, optional: device [n_seq, n_pos], the id sampled AFTER each position */
} rama_pipe_plan;
/* the schedule alone (no GPU): 1 + (*seq, *pos) if `rank` of `world` computes an item at `tick`, 0 if idle */
int  rama_pipe_item(const rama_pipe_plan *plan, int world, int rank, int tick, int *seq, int *pos);
int  rama_pipe_total_ticks(const rama_pipe *pipe, const rama_pipe_plan *plan);   /* S * n_pos + world - 1 */
int  rama_pipe_plan_ticks(const rama_pipe_plan *plan, int world);                 /* the same without a communicator */
/* [r6] EVERYTHING one tick of one rank consists of, as pure arithmetic (no GPU, no communicator): rama_pipe_run_ticks is a loop over this function
 * and executes exactly what it says -- so a CPU test that lets gloo ranks compute and exchange by it (tests/test_pipeline_gloo.py
 * test_native_tick_plan_drives_gloo_ranks) validates the native loop's own bookkeeping; tests/test_pipe_tick_plan_host.py checks the legs, the
 * dataflow and every field for every rank and tick, also with fewer sequences than stages and with wrap.  kinds: RAMA_PIPE_NONE | RAMA_PIPE_X (float[dim]) | RAMA_PIPE_TOKEN (one int32).
 * token_kind: 0 = BOS (mod.rs:182), 1 = forced prompt token `token` (mod.rs:190-191), 2 = the sequence's device token word (rank 0: what the last
 * rank sampled; other ranks take no token).  recv_pos: the position the received token was sampled AFTER (rank 0's history row). */
enum { RAMA_PIPE_NONE = 0, RAMA_PIPE_X = 1, RAMA_PIPE_TOKEN = 2 };
typedef struct {
    int32_t on, seq, pos, pos_wrapped, token_kind, token;
    int32_t samples;                                   /* this rank runs Device::sample behind the item (the last rank) */
    int32_t send_kind, send_seq, send_peer;
    int32_t recv_kind, recv_seq, recv_peer, recv_pos;
} rama_pipe_tick;
int  rama_pipe_tick_plan(const rama_pipe_plan *plan, int world, int rank, int tick, rama_pipe_tick *out);
/* Runs ticks [tick_from, tick_to) of this rank: states[s] is sequence s's run state for this stage
 * (its x is the hand-off buffer), tok_dev[s] its device token word.  Asynchronous on the context's
 * stream; after the last tick of the last rank tok_dev[s] holds sequence s's newest token. */
int  rama_pipe_run_ticks(rama_pipe *pipe, const rama_config *cfg, const rama_weights *w, rama_run_state *states,
                         int32_t *const *tok_dev, const rama_stage *stage, const rama_pipe_plan *plan,
                         int tick_from, int tick_to);
const char *rama_pipe_last_error(void);

/* generate() loop of mod.rs:169-206 at temperature 0, chained on the device: token = 1 (BOS)
 * at pos 0; while pos < steps: forward; next = pos < n_prompt ? prompt[pos] : argmax(logits);
 * out[pos] = next.  No per-token host round trip; out_tokens_host receives `steps` ids. */
int  rama_generate_greedy(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w,
                          rama_run_state *s, const int32_t *prompt_tokens_host, int n_prompt,
                          int steps, int32_t *out_tokens_host);

/* Device::sample for temperature != 0 without the logits download (reference: cpu.rs:155-179,
 * sample_top_q infer.rs:55-85; the reference GPU path copies 128 KB to the host per token,
 * gpu.rs:149-173): logits (/ T if T < 1) -> softmax -> keep p > (1 - topp) / (n - 1) -> stable
 * descending sort -> cut where the running sum exceeds topp -> draw with r = u * sum.  `u` is the
 * uniform draw; the reference re-seeds its generator on every call, so it is the same constant
 * for every token.  temperature == 0 is the argmax.  Result in device memory;
 * -1 when no probability exceeds the cutoff (the reference's index arithmetic underflows there). */
int  rama_sample_topp_dev(rama_ctx *ctx, const float *logits, size_t n, float temperature, float topp,
                          float u, int32_t *result_dev);
/* rama_sample_topp_dev for n_rows (1..128) rows at once: row r is logits + r * ld (ld >= n floats) with its own
 * temperature_host[r], topp_host[r], u_host[r]; result_dev[r] is bit for bit what rama_sample_topp_dev gives for that row
 * (-1: nothing kept).  Rows are sampled side by side in the same launches (one workgroup per row for the running sums; n >
 * 32768: the single-row launches row by row).  Scratch is sized on the first call for the largest (rows, n) seen.
 * RAMA_EINVAL for temperature < 0, topp outside [0, 1] or u outside [0, 1). */
int  rama_sample_topp_batch_dev(rama_ctx *ctx, const float *logits, size_t ld, size_t n, int n_rows,
                                const float *temperature_host, const float *topp_host, const float *u_host,
                                int32_t *result_dev);
/* Sampler of the chained decode loop (rama_decode_steps): temperature 0 (default) = argmax. */
int  rama_decode_sampler(rama_ctx *ctx, float temperature, float topp, float u);
/* generate() (mod.rs:169-206) for any temperature, chained on the device: no per-token host round
 * trip; rama_generate_greedy is this with temperature 0. */
int  rama_generate(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w, rama_run_state *s,
                   const int32_t *prompt_tokens_host, int n_prompt, int steps, float temperature,
                   float topp, float u, int32_t *out_tokens_host);
/* The same loop in pieces, for timing: begin sets (token, pos) and the forced-token list;
 * each decode_steps call enqueues n more (forward + argmax + advance) steps. */
int  rama_decode_begin(rama_ctx *ctx, int token, int pos, const int32_t *forced_tokens_host, int n_forced);
int  rama_decode_steps(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w,
                       rama_run_state *s, int n_steps);
/* tokens produced since rama_decode_begin (synchronises) */
int  rama_decode_tokens(rama_ctx *ctx, int32_t *out_tokens_host, int max_tokens, int *n_out);
/* Tokens `from`.. that the chained loop has produced SO FAR, without touching the stream (mod.rs:209-248 generate_stream
 * sends each token as it is produced): the sampling launch writes every token also to a host-visible ring (pinned,
 * device-mapped memory, one system-scope store per token), which this call reads.  Returns at once; *n_ready may be 0.
 * What goes wrong inside the loop is reported by rama_decode_tokens at the end. */
int  rama_decode_stream_poll(rama_ctx *ctx, int from, int32_t *out_tokens_host, int max_tokens, int *n_ready);
/* generate_stream (mod.rs:209-248): rama_generate with every token handed to on_token(user, index, token) on the calling
 * thread as soon as the device has produced it; the loop itself stays chained on the device (no host round trip per
 * token).  out_tokens_host (may be NULL) receives the whole list at the end. */
int  rama_generate_stream(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w, rama_run_state *s,
                          const int32_t *prompt_tokens_host, int n_prompt, int steps, float temperature,
                          float topp, float u, void (*on_token)(void *user, int index, int32_t token), void *user,
                          int32_t *out_tokens_host);
/* 1: replay launches from hipGraphs (default 0 = eager launches): rama_decode_steps / rama_generate capture a
 * decode step (or a few, "graph_steps") once per attention variant; rama_forward and rama_forward_stage* keep one
 * graph per (run state, stage, attention variant) -- token and position travel through the device cursor, so a
 * trait-level host or a pipeline stage issues one cursor write and one graph launch per token.  Setting 0
 * synchronises and drops every captured graph; free a run state only after that (or after rama_ctx_destroy). */
int  rama_set_graph_mode(rama_ctx *ctx, int enabled);
/* Modes and performance knobs.  The MODE keys change which of the reference's admissible roundings is reproduced; every other key leaves results
 * unchanged (parity mode: the same bits; fast mode: up to fp32 summation order).  Changing a key synchronises and drops captured graphs, except
 * the switches of the recorded 1:1 ops (last line below), "chain_views", "prefill", "prefill_attn" and "prefill_chain", which only store the value.
 * Measurements and history of every key: DESIGN.md appendix A.
 *
 * MODE
 *   "ref_order" = 0|1|2|3
 *        0 (library default) FAST: fused multiply-adds, tree-shaped sums -- closer to the exact logits than the CPU path, ~1.5e-4 from it at llama2-7B depth.
 *        1 PARITY (the default of every host mirror: C++ CLI, Rust shim, bench.py's `value`): every op in the reference CPU path's own rounding order
 *          (cpu.rs: 4-lane strided matvec sums with separate multiply and add, front-to-back rmsnorm / softmax / attention sums, glibc's expf restated) on
 *          chain-order weight copies (csrc/chain.hpp; made on first use, +27 GB at llama2-7B).  Bit-identical to oracle/rama_oracle.c -- i.e. to cpu.rs with
 *          the two orders it leaves to its crates fixed: "lane_reduce" below, and rayon's softmax sum taken as ONE front-to-back sum.  Weights uploaded
 *          tensor by tensor (hbm.rs:55-90) run the same kernels: the fused entries ADOPT them, rama_matmul makes a chain-order copy of a model-less matrix
 *          on first use; rama_free, rama_copy_h2d_f32 and every entry that WRITES a tensor (an op's output, rama_fill_synth) drop what was derived from it.
 *          A resident model's own tensors (rama_model_weights) are immutable by contract.
 *        2 TOLERANCE experiment: chain-order matvecs, tree-summed norms folded in, fast attention (1.4e-4 from the CPU path: the instrument of "tol_mask").
 *        3 BAR: parity up to position "bar_pos" - 1, the fast path's attention from there on (matvecs and norms stay exact).  Not bit-identical behind the
 *          switch; measured <= 1e-4 from the oracle over the whole 2 048-position context at llama2-7B depth, +7 % tokens/s at position 1 900.
 *   "lane_reduce" = 0|1|2 : parity / bar mode: the order of cpu.rs:148 `v.reduce_add()` -- 0 pairwise (l0+l1)+(l2+l3) (default), 1 strided (l0+l2)+(l1+l3),
 *        2 sequential ((l0+l1)+l2)+l3.  wide::f32x4 leaves it to the build's target features; the Rust shim asks the crate at start-up and sets this.
 *   "bar_pos" = N : first position of bar mode's fast attention (default 128; clamped to "spread_pos" and 256)
 *   "tol_mask" = 0..127 : with "ref_order" = 2, ops swapped for A/B runs (1 / 2 / 4 / 8 / 16 = the FAST Wq|Wk|Wv / Wo / W1|W3 / W2 / classifier launch,
 *        32 = parity mode's attention, 64 = its exact norms; tools/tol_sweep.py)
 *
 * FAST MODE  (default in brackets)
 *   "geom" 0..4 [3] matvec workgroup geometry (4: 8 rows x 8 waves) | "resid_r2" 0..3 [2] geometry of Wo / W2 | "solo" -1|0|1 [-1: rows <= 2048 floats] one wave per row group
 *   "w13i" 0|1 [1] W1|W3 from the row-interleaved copy | "fused" / "fused_solo" -1|0|1 [-1: dim <= 1024 / dim > 512] a whole stage as ONE launch (layer_fused.hpp)
 *   "merge" -1|0|1 [-1: dim <= 1024] attention + Wo as one launch | "split_pos" -1|N [-1: 256 when a head's K+V cache exceeds 1 MiB] split-T attention from N
 *   "attn_nsplit" 0..32 [0], "attn_waves" 16|8|4 [8], "attn_nt" 0|1 [1], "attn_u" 8|16 [8], "combine_v" 0|1 [1] : split-T geometry
 *   "small_attn" -1|0|1 [-1], "small_attn_waves" 4|8 [8], "small_attn_pos" N [256] : fewer-wave attention at short contexts
 *   "graph_steps" -1|1..32 [-1: 4 for dim <= 1024, else 1] decode steps per captured graph | "prefill" 0|1 [1] rama_generate_greedy's prompt through rama_prefill
 *   "prefill_tok" 64|128 [128], "prefill_attn" 0|1 [1], "tiled" 0|1 [1], "norm_in_gemm" 0|1 [1] : the token-batch passes (prefill_mfma.hpp, prefill_attn.hpp)
 *   "topp_sort", "topp_pairs", "topp_dist" 0|1 [1], "topp_block" 512|1024|2048 [1024], "topp_keep_sums" 0|1 [0] : the device top-p sampler's phases
 *
 * PARITY MODE  (same bits whatever the setting)
 *   "chain" 0|1 [1] chain-order copies (0: one thread per row) | "chain_d" 0|100 W + D [0], "chain_resid_d" -1|0|100 W + D [-1], "chain_lead_w" 0|1|2 [0] : geometry
 *   "chain_norm" 0|1 [1] exact norms folded into the matvecs (dim <= 512) | "chain_lead" 0|1 [1] the norms' exact sums by a leader workgroup of the consuming launch
 *   "chain_split" 0|1 [1] remainder row groups as half groups | "chain_views" 0|1 [1] chain-order copies of model-less matrices
 *   "spread_pos" 64..2^20 [128] exact attention spread over the chip from this position | "attn_fv" 0|1 [1] its softmax + value chains as one launch
 *   "prefill_chain" 0|1 [1] prompt positions through the chain-order token-batch kernels
 *   "rope_batch", "matmul_batch", "ew_batch", "norm_fold", "resid_fold", "qkv_fold" 0|1 [1] : the 1:1 Device ops are RECORDED and issued merged (49 -> 6 launches
 *        per layer; every hazard falls back to program order) */
int  rama_set_tuning(rama_ctx *ctx, const char *key, int value);

/* glibc 2.35 expf (the exp the reference's f32::exp calls on Linux) as the reference-order kernels
 * evaluate it, elementwise: the bit-exactness test's handle on it */
int  rama_ref_expf(rama_ctx *ctx, float *o, const float *x, size_t n);

/* ---------------------------------------------------------------- Q8_0 models (llama2.c version-2 checkpoints)
 * The Q8 forward is rama's forward (parity mode's exact norms, RoPE, attention, SiLU and residual adds) with every
 * Device::matmul replaced by llama2.c runq.c's quantized product:
 *   quantize(x, GS), per group: scale = max|x| / 127.0f; q = (int8) C round(x / scale) (halves away from zero), clamped to
 *     [-127, 127]; scale == 0 gives q = 0; denormals kept.
 *   matmul, row i: val = +0.0f; for g in order: ival = sum_k xq * Wq (exact int32); val = val + ((float)ival * Ws[i][g]) * xs[g]
 *     (three separately rounded fp32 operations).
 * Activations are quantized where runq.c does it: the attention-norm output (shared by Wq, Wk, Wv), the attention output
 * (Wo), the FFN-norm output (W1, W3), SiLU * gate (W2) and the final-norm output (classifier).  The token table is
 * dequantized once at load (q * s) and embeddings are read from that fp32 copy; the KV cache stays fp32.  This is NOT
 * runq.c end to end: its rmsnorm and RoPE round differently from cpu.rs, whose order rama keeps. */
typedef struct rama_q8_model rama_q8_model;
/* device pointers; x_s = the fp32 scales of tensor x, one per group of group_size consecutive values (row-major).
 * Per-layer tensors are stacked over layers as in the file; wcls == tok when the classifier is shared. */
typedef struct {
    int32_t group_size;
    const float *token_embedding_table;            /* fp32 [vocab, dim], dequantized from tok / tok_s */
    const float *rms_att_weight, *rms_ffn_weight, *rms_final_weight;
    const float *freq_cis_real, *freq_cis_imag;    /* [seq_len, head_size / 2], computed at load */
    const int8_t *tok, *wq, *wk, *wv, *wo, *w1, *w2, *w3, *wcls;
    const float *tok_s, *wq_s, *wk_s, *wv_s, *wo_s, *w1_s, *w2_s, *w3_s, *wcls_s;
} rama_q8_weights;
/* A version-2 "ak42" file (export.py version2_export): 256-byte header (magic, version, 7 ints, shared-classifier byte,
 * group size), the fp32 norms (attention, FFN, final), then per quantized tensor its int8 values and its fp32 scales:
 * tok_embeddings, wq, wk, wv, wo, w1, w2, w3 (each over all layers), output unless shared.
 * RAMA_EIO: the size does not match the header; RAMA_EUNSUP: not version 2, a group size that does not divide dim and
 * hidden_dim, n_kv_heads != n_heads. */
int  rama_q8_model_load(rama_ctx *ctx, const char *path, rama_q8_model **out);
/* rama_model_synth's fp32 weights (same hash fill and tags), generated tensor by tensor through a bounded scratch and
 * quantized by export.py quantize_q80's rule (scale = max|w| / 127, torch.round: halves to even).  RoPE tables as
 * rama_model_synth computes them without given tables. */
int  rama_q8_model_synth(rama_ctx *ctx, const rama_config *cfg, int group_size, uint64_t seed, rama_q8_model **out);
/* A resident fp32 weight set -- rama_model_weights of a loaded or synthetic model, or tensors uploaded one by one -- quantized on the
 * device: the rama_q8_model that rama_q8_model_load gives from the version-2 file export.py writes for those weights.  tok, wq, wk,
 * wv, wo, w1, w2, w3 and (unless shared: wcls == token_embedding_table, whatever cfg->shared_weight says) wcls by quantize_q80's rule in groups
 * of group_size, every layer's matrix on its own; the fp32 norms copied; RoPE tables and the dequantized token table as
 * rama_q8_model_synth makes them.  The quantizer reads the resident tensors where they lie (no scratch); the source is only read
 * and stays valid.  Synchronises.  RAMA_EINVAL for a NULL argument, an incomplete weight set (a pipeline stage's), cfg->shared_weight
 * set over a wcls of its own, group_size <= 0
 * or one that does not divide dim and hidden_dim (the Python wrapper backs it off as version2_export does; this entry does not);
 * RAMA_EUNSUP for n_kv_heads != n_heads. */
int  rama_q8_model_from_f32(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w, int group_size, rama_q8_model **out);
int  rama_q8_model_config(const rama_q8_model *m, rama_config *cfg);
int  rama_q8_model_weights(const rama_q8_model *m, rama_q8_weights *w);
size_t rama_q8_model_bytes(const rama_q8_model *m);     /* bytes streamed per token: int8 values + scales + fp32 norms */
int  rama_q8_model_free(rama_ctx *ctx, rama_q8_model *m);
/* the op-level entries: quantize(x, n) -> q[n], s[n / group_size] (RAMA_EINVAL unless group_size divides n), and
 * o[d] = matmul(xq, wq) for wq [d, n] with scales ws [d, n / group_size] */
int  rama_q8_quantize(rama_ctx *ctx, const float *x, size_t n, int group_size, int8_t *q, float *s);
int  rama_q8_matmul(rama_ctx *ctx, float *o, const int8_t *wq, const float *ws, const int8_t *xq, const float *xs,
                    size_t n, size_t d, int group_size);
/* HOST-ONLY (no context, no GPU): the kernel a Q8 product over rows of n values takes -- the rule the launchers themselves
 * ask.  n_tok == 0: the single-token matvec (rama_q8_matmul, rama_q8_forward); n_tok >= 1: one pass of min(n_tok, 128)
 * tokens of a batch.  aligned16: activations and every matrix start on a 16-byte boundary.  MATVEC: 16-byte chunks and
 * dot4, K % 16 == 0, group size a power of two in [16, 1024], at most 2048 groups (64 KiB of LDS); GEMM_KSPLIT / GEMM_MFMA:
 * int8 matrix cores, K % 16 == 0, group size 32 or a multiple of 64 up to 4096 (KSPLIT: at most 32 tokens at 32 or 64);
 * the GENERIC kernels are bytewise and take everything else.  RAMA_EINVAL unless group_size divides n. */
enum { RAMA_Q8_PATH_MATVEC = 0, RAMA_Q8_PATH_MATVEC_GENERIC = 1, RAMA_Q8_PATH_GEMM_KSPLIT = 2, RAMA_Q8_PATH_GEMM_MFMA = 3,
       RAMA_Q8_PATH_GEMM_GENERIC = 4 };
int  rama_q8_product_path(size_t n, int group_size, int n_tok, int aligned16);
/* rama_forward for a Q8 model: the same run-state buffers (logits, the cache rows of `pos`, x).  The int8 activation
 * scratch belongs to the context and is sized on the first call (outside any capture).  Graph mode: one graph per
 * (run state, attention variant), kept apart from the fp32 graphs; rama_state_free drops the Q8 graphs of the state it frees
 * and rama_q8_model_free those of every Q8 model. */
int  rama_q8_forward(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, rama_run_state *s, int token, int pos);
/* generate() (mod.rs:169-206) over a Q8 model, chained on the device as rama_generate: BOS at 0, forced prompt, then
 * Device::sample (argmax at temperature 0, else the device top-p sampler with draw u).  Graph mode: a step is one replay. */
int  rama_q8_generate(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, rama_run_state *s,
                      const int32_t *prompt_tokens_host, int n_prompt, int steps, float temperature, float topp, float u,
                      int32_t *out_tokens_host);
/* Q8 token batches: every weight pass is shared by up to 128 tokens (int8 matrix cores at group sizes 32 and multiples of
 * 64, a bytewise kernel otherwise).  The scratch belongs to the context and is sized by the first call (outside any capture);
 * these calls run eagerly in either graph mode (the chained batch below captures its step).
 * o[t * d + i] = row i of matmul(xq[t], wq) for n_tok token rows: xq [n_tok, n], xs [n_tok, n / group_size]; bit for bit
 * n_tok calls of rama_q8_matmul */
int  rama_q8_matmul_batch(rama_ctx *ctx, float *o, const int8_t *wq, const float *ws, const int8_t *xq, const float *xs,
                          size_t n, size_t d, int group_size, int n_tok);
/* the state n_tokens calls rama_q8_forward(tokens[i], pos0 + i) leave: cache rows pos0 .. pos0 + n - 1 of every layer,
 * x and logits of the last position, bit for bit (the last position runs as rama_q8_forward) */
int  rama_q8_prefill(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, rama_run_state *s,
                     const int32_t *tokens_host, int n_tokens, int pos0);
/* one step of 1..128 independent sequences sharing every weight pass; states[i] afterwards holds what
 * rama_q8_forward(tokens[i], positions[i]) would leave in its cache rows and logits (x / xb / q ... not maintained) */
int  rama_q8_decode_batch(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, const rama_run_state *states,
                          const int32_t *tokens_host, const int32_t *positions_host, int n_seq);
/* HOST-ONLY: 1 if the token-batch pass takes this shape (chain norm, and a context that fits the chain attention's score
 * buffer), 0 if not: then rama_q8_prefill and rama_q8_decode_batch run one rama_q8_forward per token, and
 * rama_q8_decode_batch_begin and rama_q8_serve_begin answer RAMA_EUNSUP.  Negative: a bad config. */
int  rama_q8_batch_shape_ok(const rama_config *cfg);

/* rama_q8_decode_batch CHAINED ON THE DEVICE, with per-sequence sampling, forced prompts, step budgets and stop tokens.
 * rama_q8_decode_batch_begin uploads every sequence's (token, position) and plan once; each step of
 * rama_q8_decode_batch_steps is the batched pass followed by one pick per sequence on the device --
 *   next = pos < n_forced ? forced[pos] : Device::sample(logits)      (a sample that keeps nothing gives token 0)
 * -- so sequence i produces, bit for bit, the tokens rama_q8_generate / rama_q8_forward give it alone.  The logits stay in
 * the context's scratch: states[i].logits is not written.  In graph mode a step is ONE hipGraph replay, and one captured
 * graph serves the whole chain.
 * A sequence is FINISHED once it has produced max_new tokens (forced ones included), or has just recorded a sampled token
 * equal to stop_token (a forced token never stops it).  From then on it keeps its token and position, writes no more
 * tokens, and its slot only rewrites its last cache row with the same bits; the other sequences run on.  per_seq == NULL:
 * every sequence greedy, without stop token, max_steps tokens each.
 * rama_q8_decode_batch_begin checks everything before it touches a running chain: RAMA_EINVAL for a bad record
 * (temperature < 0, topp outside [0, 1], u outside [0, 1), NaN, n_forced < 0, max_new < 0, a token / forced token / stop
 * token outside the vocabulary, position_i + min(max_new_i or max_steps, max_steps) > seq_len, a shared run state, n_seq
 * outside 1..128) leaves the previous chain as it was.  RAMA_EUNSUP: a shape the Q8 token-batch pass does not take, or a
 * plan that samples or forces on vocab_size > 32768.
 * rama_q8_decode_batch_steps: RAMA_EINVAL beyond max_steps, and once the chain's model (rama_q8_model_free) or the run
 * state of one of its sequences (rama_state_free) is gone.  rama_q8_prefill / rama_q8_decode_batch / rama_q8_forward on
 * other run states between two calls are fine.
 * rama_q8_decode_batch_tokens synchronises: sequence s's tokens at out_host[s * max_per_seq ..], its count in n_per_seq[s].
 * rama_q8_decode_batch_stream_poll never touches the stream: tokens from.. of one sequence from its host-visible ring, and
 * *finished (may be NULL) = 1 once the sequence has finished -- set after its last token is visible. */
typedef struct {
    float temperature, topp, u;                 /* Device::sample; temperature 0 = argmax */
    const int32_t *forced; int32_t n_forced;    /* forced by ABSOLUTE position, as rama_decode_batch_begin_sampled */
    int32_t max_new;                            /* tokens this sequence may produce, forced ones included; 0 = max_steps */
    int32_t stop_token;                         /* -1 = none; a SAMPLED token equal to it is recorded, then the sequence is finished */
} rama_q8_seq_plan;
int  rama_q8_decode_batch_begin(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, const rama_run_state *states,
                                const int32_t *tokens_host, const int32_t *positions_host, int n_seq, int max_steps,
                                const rama_q8_seq_plan *per_seq);
int  rama_q8_decode_batch_steps(rama_ctx *ctx, int n_steps);
int  rama_q8_decode_batch_tokens(rama_ctx *ctx, int32_t *out_host, int max_per_seq, int32_t *n_per_seq);
int  rama_q8_decode_batch_stream_poll(rama_ctx *ctx, int seq, int from, int32_t *out_tokens_host, int max_tokens, int *n_ready,
                                      int *finished);

/* THE SERVING CHAIN: continuous batching over a Q8 model.  A second, open-ended chain next to the one above,
 * with a state of its own.  n_slots sequence slots (1..128) share weight passes of max_rows rows (n_slots <= max_rows <= 128).
 * A slot is FREE, PROMPT (still ingesting its context), DECODE or DONE.  An admitted sequence brings a run state, its context
 * tokens c[0..n) fed at positions 0..n-1 (the caller includes BOS), and a plan; its output is the SAMPLED tokens only.
 * One step = one weight pass over max_rows rows, then one pick per slot that has logits.  The step's rows are decided ON THE
 * DEVICE from the slot table, by the rule rama_q8_serve_plan_step states on the host:
 *   1. every DECODE slot gets one row: its current token at its position;
 *   2. every PROMPT slot gets one row: its next context position;
 *   3. the rows left over go to PROMPT slots in ascending slot index, each taking as many further consecutive context
 *      positions as it has left and as fit;
 *   4. the rest are idle (position -1): they write nothing to any run state and nothing is read through their pointers.
 * Rows are laid out by slot index, a slot's rows at consecutive positions, idle rows last.  Only a slot's last row of a step
 * may carry logits, and only if it is a DECODE row or the final context position; those rows (<= n_slots) are gathered, and
 * the final norm, the quantizer and the classifier run over n_slots rows.  After the pick a PROMPT slot that has just fed its
 * final context position records its first token and becomes DECODE; a slot that records its max_new-th token or a sampled
 * stop token becomes DONE, sets its host-visible finished word after its last ring word, and occupies no rows from then on.
 * Slot i's tokens are, bit for bit, rama_q8_generate(prompt = c[1:], steps = n - 1 + max_new, T, topp, u)[n-1:] run on that
 * sequence alone (for c[0] == 1), cut at the stop token; its cache rows 0..last are that run's, and nothing behind its last
 * position is written -- whatever the chunking, the neighbours, max_rows and the graph mode.  In graph mode a step is one
 * hipGraph replay and ONE captured graph serves the chain for its whole life, admissions included.
 *
 * rama_q8_serve_begin sizes everything outside any capture (tables, a context buffer of seq_len ints and a pinned admission
 * record per slot, out / ring rows of max_new_cap tokens) and ends a previous serving chain.  RAMA_EUNSUP where
 * rama_q8_decode_batch_begin gives it (a shape the Q8 token-batch pass does not take; vocab_size % 4 != 0 beyond 32768),
 * RAMA_EINVAL for bad sizes.
 * rama_q8_serve_admit: the slot must be FREE, or DONE as the host can already see it (the finished word; no synchronisation).
 * Stream-ordered -- an async copy of the slot's own pinned record and a small launch that installs it -- so it works between
 * any two rama_q8_serve_steps calls without draining the stream or touching the graph.  It resets the slot's ring row and
 * finished word and bumps the slot's generation number.  Everything is checked first and a refusal leaves the chain as it was:
 * RAMA_EINVAL for a busy slot, a token outside the vocabulary, temperature < 0 / topp outside [0, 1] / u outside [0, 1) / NaN,
 * a stop token outside [-1, vocab_size), n_context < 1, max_new < 1, n_context + max_new > seq_len, max_new > max_new_cap, a
 * run state that a live slot already uses; RAMA_EUNSUP for a sampled plan on vocab_size > 32768.
 * rama_q8_serve_steps: no overall limit.  RAMA_EINVAL once the model (rama_q8_model_free) or the run state of an occupied slot
 * (rama_state_free before the host could see the slot DONE) is gone.
 * rama_q8_serve_poll never touches the stream: tokens from.. of the slot's occupant, *finished, and *generation (each may be
 * NULL).  *finished is the slot's finished WORD, not a boolean: 0 while the occupant runs, 1 once it has finished by itself, and
 * RAMA_SERVE_CANCELLED (2) once a rama_q8_serve_cancel has ended it (below) -- test it against 0, not against 1.  rama_q8_serve_tokens synchronises.  rama_q8_serve_stats synchronises: the counters the scheduler launch keeps on the
 * device, the captures so far, the slot table, and the last step's row table.
 * rama_q8_serve_plan_step is HOST-ONLY (no context, no GPU): the rule above as a pure function, rows_out[max_rows] and --
 * slots_after may be NULL -- the successor states when no stop token is sampled.  The device scheduler produces exactly
 * this table. */
#define RAMA_SERVE_FREE   0
#define RAMA_SERVE_PROMPT 1
#define RAMA_SERVE_DECODE 2
#define RAMA_SERVE_DONE   3
typedef struct {
    int32_t state;                              /* RAMA_SERVE_* */
    int32_t n_context;
    int32_t cursor;                             /* PROMPT: the next context position; DECODE: the position of the next row */
    int32_t n_out;                              /* tokens produced */
    int32_t max_new;
} rama_q8_serve_slot;
typedef struct { int32_t slot, pos, logits; } rama_q8_serve_row;      /* idle: slot -1, pos -1; logits: 1 if the row carries them */
typedef struct {
    float temperature, topp, u;                 /* Device::sample; temperature 0 = argmax */
    int32_t max_new;                            /* >= 1 */
    int32_t stop_token;                         /* -1 = none; a sampled token equal to it is recorded, then the slot is DONE */
} rama_q8_serve_plan;
typedef struct {
    uint64_t steps, graph_captures, rows_decode, rows_prompt, rows_idle;
    int32_t n_slots, max_rows;
    rama_q8_serve_row last_rows[128];           /* the last step's row table (max_rows entries) */
    rama_q8_serve_slot slots[128];              /* the slot table now */
    int32_t generation[128];
} rama_q8_serve_report;
int  rama_q8_serve_begin(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, int n_slots, int max_rows, int max_new_cap);
int  rama_q8_serve_admit(rama_ctx *ctx, int slot, const rama_run_state *state, const int32_t *context_host, int n_context,
                         const rama_q8_serve_plan *plan);
int  rama_q8_serve_steps(rama_ctx *ctx, int n_steps);
int  rama_q8_serve_poll(rama_ctx *ctx, int slot, int from, int32_t *out_tokens_host, int max_tokens, int *n_ready, int *finished,
                        int *generation);
int  rama_q8_serve_tokens(rama_ctx *ctx, int slot, int32_t *out_host, int max_tokens, int *n);
int  rama_q8_serve_stats(rama_ctx *ctx, rama_q8_serve_report *out);
int  rama_q8_serve_plan_step(const rama_q8_serve_slot *slots, int n_slots, int max_rows, rama_q8_serve_row *rows_out,
                             rama_q8_serve_slot *slots_after);
int  rama_q8_serve_end(rama_ctx *ctx);

/* PROMPT CACHING for the serving chain.  Cache row t of a sequence is a function of tokens 0..t only, and its
 * bits are the same whoever computed it (chunking, neighbours, max_rows, graph mode).  So rows computed once, by any sequence
 * with the same first n tokens, are the rows this sequence would compute: copy them, start the cursor at n, and the tokens and
 * cache rows are still those of rama_q8_generate on the sequence alone, bit for bit.
 *
 * rama_q8_serve_admit_at is rama_q8_serve_admit with the first n_cached positions taken as already present in `state`'s
 * caches: rows 0..n_cached-1 of every layer are the rows of context[0..n_cached), written by work enqueued EARLIER on the
 * context's stream (the caller's contract: a rama_q8_kv_fork, a rama_q8_prefill, an earlier occupant's steps).  The slot is
 * installed PROMPT with cursor = n_cached and feeds context[n_cached..n_context).  The whole context is still passed and
 * checked, and the slot's context buffer holds all of it.  0 <= n_cached <= n_context - 1: the final context position is
 * always fed, its logits are needed.  n_cached == 0 is exactly rama_q8_serve_admit; every check of rama_q8_serve_admit
 * applies, a bad n_cached is RAMA_EINVAL, a refusal leaves the chain as it was.  Stream-ordered, no synchronisation, the graph
 * untouched, the slot's generation number goes up.
 *
 * rama_q8_kv_fork copies rows [0, n_rows) of every layer of src's key and value caches into each of dsts[0..n_dst) -- one
 * launch that reads the source once and writes every destination.  1 <= n_dst <= 16, 0 <= n_rows <= seq_len; n_rows == 0 is a
 * successful no-op.  Only cfg's dim, n_layers and seq_len and the states' key_cache / value_cache are used.  Stream-ordered on
 * the context's stream, never synchronises, legal between any two rama_q8_serve_steps calls.  The source may belong to a live
 * slot provided the copied rows lie below what earlier enqueued work has written (rows below a slot's cursor are never
 * rewritten -- on a chain begun with rama_q8_serve_begin_spec too, where rows AT AND BEHIND a speculating slot's cursor may
 * hold rejected drafts: fork only rows below the cursor, n_rows <= n_context - 1 + the tokens the host has seen).  RAMA_EINVAL for a NULL argument or cache, n_dst or n_rows out of range, a destination whose caches overlap the
 * source's or another destination's, and a destination that is in a live slot of a serving chain -- the Q8 chain's or the fp32
 * chain's (rama_serve_*, below).  Cache bases that are not 16-byte aligned take a slower path with the same result.
 * THE ONE FORK OF BOTH STACKS: the KV cache is fp32 whatever the model, and the fork reads no weight, so rows written by
 * rama_prefill, rama_generate or an fp32 serving slot are forked by this entry too (rama_serve_admit_at below). */
int  rama_q8_serve_admit_at(rama_ctx *ctx, int slot, const rama_run_state *state, const int32_t *context_host, int n_context,
                            int n_cached, const rama_q8_serve_plan *plan);
int  rama_q8_kv_fork(rama_ctx *ctx, const rama_config *cfg, const rama_run_state *src, const rama_run_state *dsts, int n_dst,
                     int n_rows);

/* THE SERVING CHAIN IN PARITY MODE: continuous batching over an fp32 model, in the reference's rounding order.
 * The rama_q8_serve_* entries above argument for argument, with rama_weights in place of rama_q8_weights and the same plan,
 * slot, row and report records; rama_q8_serve_plan_step is the host rule of both chains.  Slot i's tokens are, bit for bit,
 * parity-mode rama_generate(prompt = c[1:], steps = n - 1 + max_new, T, topp, u)[n-1:] run on that sequence alone (for
 * c[0] == 1), cut at the stop token -- the oracle's tokens; its cache rows 0..last are that run's and nothing behind its last
 * position is written, whatever the chunking, the neighbours, max_rows, the tile a row lands in and the graph mode.
 * A step's pass runs the row table in tiles of 32 rows, in ascending order; idle rows come last, and a tile whose first row is
 * idle costs its launches but streams no weight.  A state of its own: it may be live next to a Q8 serving chain on the same
 * context, and neither chain touches the other's tables or captured step.  No pipeline.  Prompt caching (rama_serve_admit_at)
 * and drafts in idle rows (rama_serve_begin_spec, declared behind the Q8 entries they mirror) are opt-in.
 *
 * rama_serve_begin: 1 <= n_slots <= max_rows <= 128 and 1 <= max_new_cap <= seq_len - 1 (RAMA_EINVAL).  PARITY MODE ONLY:
 *   RAMA_EUNSUP unless "ref_order" = 1 -- fast mode ("ref_order" = 0), tolerance mode (2) and bar mode (3) are out of scope --,
 *   and for a shape or weights the parity-mode token batch does not take: no chain-order copies ("chain" / "prefill_chain" = 0,
 *   or none can be made), dim or hidden_dim not a multiple of 16, a context too long for the attention's score buffer;
 *   vocab_size % 4 != 0 beyond 32768.  A refusal or a failed allocation leaves a running chain untouched: the new chain is made
 *   beside it, and success ends the previous fp32 chain.
 * rama_serve_admit: rama_q8_serve_admit's checks in the same order (one body), the run state checked against the fp32 model;
 *   RAMA_EUNSUP for a sampled plan on vocab_size > 32768.  Stream-ordered, the captured step untouched.
 * rama_serve_admit_at: rama_q8_serve_admit_at's contract.  0 <= n_cached <= n_context - 1 (RAMA_EINVAL); the slot is installed
 *   PROMPT with cursor = n_cached; rows 0..n_cached-1 of every layer of `state`'s caches are the caller's contract: the rows
 *   of context[0..n_cached), written by work enqueued earlier on the context's stream (a rama_prefill or rama_generate in
 *   parity mode, a rama_q8_kv_fork, an earlier occupant's steps).  rama_serve_admit is its n_cached == 0 case: one body, the
 *   same checks in the same order.  The tokens and cache rows are those of the solo run, bit for bit.
 * rama_serve_steps: no overall limit.  RAMA_EINVAL once the model (rama_model_free) or the run state of an occupied slot
 *   (rama_state_free before the host could see the slot DONE) is gone; RAMA_EUNSUP once the context has left parity mode.
 * rama_serve_poll never touches the stream: tokens from.. of the slot's occupant, *finished, *generation (each may be NULL).
 *   *finished is the finished word as rama_q8_serve_poll gives it: 0, 1, or RAMA_SERVE_CANCELLED (2) after a rama_serve_cancel.
 * rama_serve_tokens synchronises and copies the slot's tokens.
 * rama_serve_stats synchronises: the device's counters, the captures so far, the slot table, the last step's row table.
 * rama_serve_end synchronises and frees the chain; nothing to end is success. */
int  rama_serve_begin(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w, int n_slots, int max_rows, int max_new_cap);
int  rama_serve_admit(rama_ctx *ctx, int slot, const rama_run_state *state, const int32_t *context_host, int n_context,
                      const rama_q8_serve_plan *plan);
int  rama_serve_admit_at(rama_ctx *ctx, int slot, const rama_run_state *state, const int32_t *context_host, int n_context,
                         int n_cached, const rama_q8_serve_plan *plan);
int  rama_serve_steps(rama_ctx *ctx, int n_steps);
int  rama_serve_poll(rama_ctx *ctx, int slot, int from, int32_t *out_tokens_host, int max_tokens, int *n_ready, int *finished,
                     int *generation);
int  rama_serve_tokens(rama_ctx *ctx, int slot, int32_t *out_host, int max_tokens, int *n);
int  rama_serve_stats(rama_ctx *ctx, rama_q8_serve_report *out);
int  rama_serve_end(rama_ctx *ctx);

/* THE SPECULATIVE CHAIN: one-stream Q8 decode that drafts by n-gram lookup and verifies in one pass.  A third
 * chain next to the two above, with a state of its own, for ONE sequence.  A token-batch pass over rows at consecutive positions
 * of one sequence leaves every row the cache rows and logits of its own rama_q8_forward, and a pass of up to 16 rows costs about
 * what a pass of 2 costs: so K guessed tokens and the token before them are checked in one weight pass of K + 1 rows, and what
 * is accepted is exactly what rama_q8_generate would have produced.  A wrong guess costs time only.
 *
 * Notation: s[0..L) are the sequence's known tokens (the context, BOS first, and everything emitted so far); cache rows
 * 0..L-2 are valid and s[L-1] is fed next, at position P = L-1; hint[0..n_hint) is an optional text to look up in as well (a
 * document being edited or quoted, a previous answer); K = n_draft in 0..15, N = ngram in 1..4.
 * DRAFT (rama_q8_spec_draft).  For n = min(N, L) down to 1: look for the tail s[L-n..L) first in hint, then in s, and take the
 *   latest occurrence; in s it must end before L (the tail itself does not count).  The first n for which one of the two texts
 *   has an occurrence decides -- the hint's if both have one.  The drafts d[0..n_d) are the tokens that follow that occurrence in
 *   the same text, up to that text's end, with n_d <= K, n_d <= seq_len - 1 - P and n_d <= remaining - 1 (remaining = max_new
 *   minus the tokens emitted so far).  No occurrence at any n, or K = 0: n_d = 0.
 * STEP.  Rows j = 0..n_d carry s[L-1], d[0], .., d[n_d-1] at positions P..P+n_d; the other rows of the K + 1-row pass are idle
 *   (position -1: they write nothing and nothing is read through them).  All K + 1 rows go through the final norm, the quantizer
 *   and the classifier, and pick_j = Device::sample(logits_j) with the plan's temperature, topp and draw u, as rama_q8_generate
 *   applies them at that position.
 * ACCEPT (rama_q8_spec_accept).  a = the largest value <= n_d with pick_j == d[j] for all j < a.  pick_0..pick_a are emitted, cut
 *   after the first emitted token equal to stop_token and cut at the budget; either cut finishes the sequence.  L grows by the
 *   number of tokens emitted.  A finished sequence's further steps are all-idle passes.
 * The output is the sampled tokens only and is, bit for bit,
 *   rama_q8_generate(prompt = c[1:], steps = n_context - 1 + max_new, T, topp, u)[n_context-1:]  cut after the stop token
 * whatever n_draft, ngram, the hint and the graph mode.  Cache rows at or below the new P - 1 hold that run's bits.  UNLIKE the
 * other two chains, rows BEHIND that position may hold the rows of rejected drafts: the next step rewrites whatever it reads
 * before it reads it.  Nothing at or beyond position n_context - 1 + max_new is ever written.  In graph mode a step is one
 * hipGraph replay and ONE captured graph serves the chain for its whole life.
 *
 * rama_q8_spec_begin: the contract of rama_q8_serve_admit_at with n_cached = n_context - 1 -- rows 0..n_context-2 of `state`
 * were written by work enqueued earlier on the context's stream (a rama_q8_prefill of context[:-1]; nothing for n_context == 1)
 * -- and the chain feeds context[n_context-1] first.  It sizes everything outside any capture (a device token buffer of n_hint +
 * seq_len, out and a pinned host-visible ring of max_new tokens, pinned count and finished words) and ends a previous
 * speculative chain.  Everything is checked first and a refusal leaves the previous chain as it was: RAMA_EINVAL for a NULL
 * argument, temperature < 0 / topp outside [0, 1] / u outside [0, 1) / NaN, a stop token outside [-1, vocab_size), n_draft
 * outside 0..15, ngram outside 1..4, a hint or context token outside the vocabulary, n_hint < 0, n_hint > 0 with hint == NULL,
 * n_context < 1, max_new < 1, n_context + max_new > seq_len; RAMA_EUNSUP where rama_q8_decode_batch_begin gives it
 * (rama_q8_batch_shape_ok == 0; a sampled plan on vocab_size > 32768).
 * rama_q8_spec_steps: no overall limit.  RAMA_EINVAL once the model (rama_q8_model_free) or the run state (rama_state_free) is
 * gone.  rama_q8_prefill / rama_q8_decode_batch / the other chains on other run states between two calls are fine.
 * rama_q8_spec_poll never touches the stream: tokens from.. of the host-visible ring, and *finished (may be NULL) = 1 once the
 * sequence has finished -- set after its last token is visible.  rama_q8_spec_tokens and rama_q8_spec_stats synchronise.  The
 * report: steps (idle ones included), the captures so far, and over the steps before the finish rows_fed = sum (n_d + 1),
 * drafts = sum n_d, accepted = sum a, emitted, accepted_hist[a] = steps that accepted a drafts; cursor = P.
 * rama_q8_spec_draft and rama_q8_spec_accept are HOST-ONLY (no context, no GPU): the two rules above as pure functions, which
 * the device reproduces exactly.  _draft: room = min(seq_len - 1 - P, remaining - 1); returns n_d and fills drafts_out[0..n_d).
 * _accept: picks[0..n_d], remaining >= 1; returns the tokens emitted (pick_0 ..) and *finished (may be NULL).  Both answer
 * RAMA_EINVAL (negative) for a bad argument. */
typedef struct {
    float temperature, topp, u;                 /* Device::sample; temperature 0 = argmax */
    int32_t max_new;                            /* >= 1 */
    int32_t stop_token;                         /* -1 = none; an emitted token equal to it is recorded, then the sequence is finished */
    int32_t n_draft, ngram;                     /* K in 0..15, N in 1..4 */
    const int32_t *hint; int32_t n_hint;        /* a text to look up in besides the sequence's own; may be NULL / 0 */
} rama_q8_spec_plan;
typedef struct {
    uint64_t steps, graph_captures, rows_fed, drafts, accepted, emitted;
    uint64_t accepted_hist[16];
    int32_t finished, n_out, cursor;
} rama_q8_spec_report;
int  rama_q8_spec_begin(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, const rama_run_state *state,
                        const int32_t *context_host, int n_context, const rama_q8_spec_plan *plan);
int  rama_q8_spec_steps(rama_ctx *ctx, int n_steps);
int  rama_q8_spec_poll(rama_ctx *ctx, int from, int32_t *out_tokens_host, int max_tokens, int *n_ready, int *finished);
int  rama_q8_spec_tokens(rama_ctx *ctx, int32_t *out_host, int max_tokens, int *n);
int  rama_q8_spec_stats(rama_ctx *ctx, rama_q8_spec_report *out);
int  rama_q8_spec_end(rama_ctx *ctx);
int  rama_q8_spec_draft(const int32_t *hint, int n_hint, const int32_t *seq, int L, int n_draft, int ngram, int room,
                        int32_t *drafts_out);
int  rama_q8_spec_accept(const int32_t *drafts, int n_d, const int32_t *picks, int stop_token, int remaining, int *finished);

/* THE SPECULATIVE CHAIN WITH A DRAFT MODEL: the drafts come from a small Q8 model over the same vocabulary.
 * rama_q8_spec_begin_model starts the chain above -- the same sequence record, ring and finished word, one captured graph for
 * its life; rama_q8_spec_steps / _poll / _tokens / _stats / _end serve it unchanged, and it ends a previous speculative chain
 * -- with one difference: where the drafts come from.  The pick is a deterministic function of the logits, so whatever the draft
 * model proposes the output is, bit for bit, what rama_q8_spec_begin and rama_q8_generate give on the target alone.
 *
 * Notation as above, plus the DRAFT CURSOR Dc: rows 0..Dc-1 of the draft run state's cache hold the draft model's rows of
 * s[0..Dc).  P - Dc is 0 or 1 when a step opens.
 * STEP, one graph replay on one stream:
 *   OPEN.   n_d = min(K, seq_len - 1 - P, remaining - 1), 0 on a finished sequence.  The first draft pass has two rows: the rows
 *     at positions Dc..P carrying s[Dc..P] -- one live row, or two when the step before accepted all K of its drafts, whose last,
 *     d[K-1], was never fed to the draft model (the CATCH-UP row).  n_d == 0: every draft row of the step is idle (position -1:
 *     it writes nothing and nothing is read through it).
 *   DRAFT.  For j = 0..K-1 a token-batch pass of the draft model (two rows for j = 0, one after that) and
 *     d[j] = Device::sample(logits of the pass's last live row) with the plan's temperature, topp and u -- the target's own rule,
 *     so a draft model equal to the target agrees with it everywhere.  Pass j + 1 feeds d[j] at position P + j + 1; passes
 *     j >= n_d are idle.
 *   VERIFY. The target's pass of K + 1 rows over s[L-1], d[0..n_d), the picks and the accept rule, exactly as above.
 *   CLOSE.  Dc' = L + min(a, n_d - 1) for n_d >= 1 (L as the step opened; a budget or stop cut that emits fewer tokens than were
 *     accepted ends the sequence, and Dc' stops at the new L).
 * Rows of the DRAFT cache at and behind Dc' may hold the rows of rejected drafts, as rows of the target's cache behind its
 * cursor may: the next step rewrites whatever it reads before it reads it.  Nothing at or beyond position
 * n_context - 1 + max_new of either cache is ever written.
 *
 * rama_q8_spec_begin_model: the target side is rama_q8_spec_begin's contract -- rows 0..n_context-2 of `state` were written by
 * work enqueued earlier on the context's stream -- and the same holds for `dstate` under the draft model (a rama_q8_prefill of
 * context[:-1] with it).  The draft model may differ in dim, depth and group size; its passes run on a batch scratch of their
 * own, sized here outside any capture.  plan->n_draft is in 1..15, plan->ngram is ignored, plan->hint must be NULL / 0: model
 * drafts replace the n-gram lookup, they are not mixed with it.  Everything is checked first and a refusal leaves the previous
 * chain as it was: RAMA_EINVAL for a NULL argument, dcfg->vocab_size != cfg->vocab_size, n_context + max_new > dcfg->seq_len,
 * dstate sharing a cache with state, a hint, n_draft outside 1..15 and everything else rama_q8_spec_begin refuses; RAMA_EUNSUP
 * where rama_q8_spec_begin gives it, and for rama_q8_batch_shape_ok(dcfg) == 0.
 * rama_q8_spec_steps answers RAMA_EINVAL once either model (rama_q8_model_free) or either run state (rama_state_free) is gone.
 * rama_q8_spec_stats keeps its meaning: drafts = sum n_d, accepted, accepted_hist, rows_fed = sum (n_d + 1), cursor = P.
 * rama_q8_spec_model_stats synchronises; RAMA_EINVAL on a chain begun with rama_q8_spec_begin.  Over the steps before the
 * finish: draft_passes = the live draft passes (sum n_d), draft_rows_fed = the live rows of those passes (catch-up rows
 * included), catch_up_rows; draft_cursor = Dc. */
typedef struct {
    uint64_t draft_passes, draft_rows_fed, catch_up_rows;
    int32_t draft_cursor;
} rama_q8_spec_model_report;
int  rama_q8_spec_begin_model(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, const rama_run_state *state,
                              const rama_config *dcfg, const rama_q8_weights *dw, const rama_run_state *dstate,
                              const int32_t *context_host, int n_context, const rama_q8_spec_plan *plan);
int  rama_q8_spec_model_stats(rama_ctx *ctx, rama_q8_spec_model_report *out);

/* THE SPECULATIVE CHAIN WITH TREE DRAFTS: several continuations of the tail n-gram, verified in one weight pass.
 * rama_q8_spec_begin_tree starts the speculative chain above -- the same sequence record, ring and finished word, one captured
 * graph for its life; rama_q8_spec_steps / _poll / _tokens / _stats / _end serve it unchanged, and it ends a previous speculative
 * chain.  Notation as rama_q8_spec_begin's, plus B = n_branch in 1..4 and R = n_rows in 2..16.
 * DRAFT (rama_q8_spec_tree_draft).  cap = min(K, room); cap <= 0: only the root.  n as above.  The occurrences of the tail at that
 *   n, ordered hint before sequence and larger end first; the first B are the branches (there may be fewer), branch b the
 *   min(cap, text_end - e_b) tokens behind occurrence b in its own text.  The branches are inserted in order into a trie whose root
 *   (node 0) carries s[L-1]: walk from the root, follow a child with the same token, else create node m + 1 with parent = the
 *   current node and depth = depth(parent) + 1; once R - 1 nodes exist everything stops.  Children of a node have distinct tokens,
 *   parent < index, and branch 0 is rama_q8_spec_draft's draft: its nodes have index == depth.  A node with index != depth is OFF
 *   THE TRUNK.
 * STEP.  Row j carries tok[j] at position P + depth[j]; rows m+1..R-1 are idle.  All R rows are classified and
 *   pick_j = Device::sample(logits_j).  Only the root writes its cache row (at P) during the pass: two nodes of one depth share a
 *   position.  A row's attention reads timestep t <= P from the cache and timestep P + k from its ancestor of depth k in the pass.
 * ACCEPT (rama_q8_spec_tree_accept).  cur = 0, emit pick_0; while the token just emitted is not the stop token, the budget is not
 *   used up and cur has a child c with tok[c] == that token: cur = c, emit pick_c.  a = depth(cur); the path is the rows visited.
 *   The sequence finishes at the budget or on an emitted stop token.  (a counts the rows walked: a stop token ends the walk, where
 *   rama_q8_spec_accept's a goes on counting the drafts its picks reproduce behind it.)
 * COMMIT.  The path's rows 1..a are copied to cache positions P+1..P+a in every layer.  UNLIKE rama_q8_spec_begin's chain, nothing
 *   at or behind the new P is ever written.
 * The output is rama_q8_generate's, bit for bit, whatever B, R, K, N, the hint and the graph mode; with B = 1 and R = K + 1 the
 * drafts, the steps and the tokens are rama_q8_spec_begin's.
 * rama_q8_spec_begin_tree: rama_q8_spec_begin's contract and refusals, plus RAMA_EINVAL for n_branch outside 1..4, n_rows
 * outside 2..16 and n_draft < 1.  It also sizes the tree store, [n_layers][R-1][dim] floats twice, outside any capture.
 * rama_q8_spec_stats keeps its meanings: drafts = sum m, rows_fed = sum (m + 1), accepted = sum a, accepted_hist[a].
 * rama_q8_spec_tree_stats synchronises; RAMA_EINVAL on a chain begun any other way.  off_trunk_accepted = accepted nodes with
 * index != depth, off_trunk_steps = steps that accepted one, nodes_hist[m] = steps whose tree had m nodes besides the root.
 * rama_q8_spec_tree_draft and rama_q8_spec_tree_accept are HOST-ONLY.  _draft returns m and fills tok_out / parent_out /
 * depth_out[0..m) with nodes 1..m.  _accept takes nodes 1..m the same way (tok[j-1], parent[j-1]) and picks[0..m]; it returns the
 * tokens emitted and fills path_out[0..a] (>= 16 entries; may be NULL), *a_out and *finished (may be NULL).  Both answer
 * RAMA_EINVAL (negative) for a bad argument.
 *
 * THE BUILDING BLOCKS, for host-driven speculators.  rama_q8_tree_forward: an eager pass over a caller's tree -- parent[0] = -1,
 * parent[j] in [0, j), depth at most 15, n_rows in 1..16, pos0 + the deepest depth < seq_len; rows 0..pos0-1 of `state` were
 * written by work enqueued earlier on the context's stream.  It writes logits_dev [n_rows, vocab_size] (device memory), the root's
 * cache row at pos0 and nothing else of the cache.  rama_q8_tree_commit copies a root-to-node path (path[0] = 0, each row a child
 * of the one before) of the LAST tree pass on that state to cache positions pos0+1..pos0+n_path-1.  Stream-ordered.  RAMA_EINVAL
 * for every bad argument (a path that is none, another state, model or pos0 than the last pass's, a state freed since);
 * RAMA_EUNSUP where rama_q8_batch_shape_ok == 0. */
typedef struct {
    uint64_t off_trunk_accepted, off_trunk_steps;
    uint64_t nodes_hist[16];
    int32_t n_branch, n_rows;
} rama_q8_spec_tree_report;
int  rama_q8_spec_begin_tree(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, const rama_run_state *state,
                             const int32_t *context_host, int n_context, const rama_q8_spec_plan *plan, int n_branch, int n_rows);
int  rama_q8_spec_tree_stats(rama_ctx *ctx, rama_q8_spec_tree_report *out);
int  rama_q8_spec_tree_draft(const int32_t *hint, int n_hint, const int32_t *seq, int L, int n_draft, int ngram, int room,
                             int n_branch, int n_rows, int32_t *tok_out, int32_t *parent_out, int32_t *depth_out);
int  rama_q8_spec_tree_accept(const int32_t *tok, const int32_t *parent, int m, const int32_t *picks, int stop_token, int remaining,
                              int32_t *path_out, int *a_out, int *finished);
int  rama_q8_tree_forward(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, const rama_run_state *state,
                          const int32_t *tokens_host, const int32_t *parent_host, int n_rows, int pos0, float *logits_dev);
int  rama_q8_tree_commit(rama_ctx *ctx, const rama_config *cfg, const rama_run_state *state, const int32_t *path_host, int n_path,
                         int pos0);

/* THE SPECULATIVE CHAIN WITH TREE DRAFTS FROM A DRAFT MODEL: the draft model's second and third choices as branches.
 * rama_q8_spec_begin_model_tree starts the speculative chain above with rama_q8_spec_begin_model's drafter and
 * rama_q8_spec_begin_tree's verification; rama_q8_spec_steps / _poll / _tokens / _stats / _end serve it unchanged, and it ends a
 * previous speculative chain.  Notation as above: K = plan->n_draft, B = n_branch in 1..4, R = n_rows in 2..16, P = L - 1, Dc the
 * draft cursor, cap = min(K, seq_len - 1 - P, remaining - 1), at least 0, and 0 on a finished sequence.
 * SHAPE (rama_q8_spec_model_tree_shape).  Static: a pure function of (cap, B, R), no data in it.  Node 0 is the root and carries
 *   s[L-1].  Trunk first: nodes 1..min(cap, R-1), node d with parent d - 1, depth d, rank 0.  Then the sides, level by level: for
 *   depth d = 1..cap and every node p of depth d - 1 in ascending index, each new node taking the next free index -- p on the trunk
 *   (index == depth, the root included): side children of ranks 1..B-1; otherwise one child of rank 0.  Everything stops once R - 1
 *   nodes exist; m = the nodes besides the root.  parent < index, and OFF THE TRUNK is index != depth as above.  B = 1: the line
 *   1..cap.  B = 2, K = 4, R = 16: 14 nodes.
 * CANDIDATES (rama_q8_spec_model_tree_candidates).  A node's token comes from the draft model's logits after the prefix and the
 *   path to the node's PARENT.  Rank 0 is Device::sample of that row under the plan's (temperature, topp, u): rama_q8_spec_begin_model's
 *   draft.  Ranks 1..B-1: order all tokens by a 64-bit key, descending -- high word the logit's bits mapped monotonically to
 *   unsigned (bits ^ 0x80000000 for a clear sign bit, ~bits for a set one; a NaN lands where its bits put it), low word the token
 *   index: the larger logit first, on ties the higher index, the argmax's own rule --, drop rank 0's token, take the first B - 1.
 *   Children of one node have distinct tokens.
 * STEP.  One graph replay on one stream.  OPEN: cap, the shape, the target's row table.  K DRAFT LEVELS: pass d feeds every node of
 *   depth d - 1 at position P + d - 1 (pass 1: the root, behind rama_q8_spec_begin_model's catch-up row at P - 1 when P - Dc == 1);
 *   only the root and the catch-up row write the draft cache, every other fed node leaves its rotated k and its v in row node - 1
 *   of a draft tree store, and a fed row's attention takes timestep t <= P from the draft cache and timestep P + k from the store
 *   row of its ancestor of depth k.  Each pass ends with its rows' picks: every child's token.  Passes d > cap are idle: position
 *   -1, nothing written, nothing read.  VERIFY: the target's tree pass over rows 0..m, the picks, ACCEPT and COMMIT as
 *   rama_q8_spec_begin_tree runs them.  CLOSE: the accepted path's fed nodes, depths 1..min(a, cap - 1), go from the draft store to
 *   draft cache positions P+1..; Dc' = L + min(a, cap - 1) for cap >= 1 (L as the step opened; a budget or stop cut stops it at
 *   the new L).  P - Dc stays in {0, 1}.  Nothing at or behind Dc', or behind the new P, is written in either cache.
 * The output is rama_q8_generate's, bit for bit, whatever the drafter proposes.  Draft cache rows below Dc are those of a fresh
 * rama_q8_prefill of the draft model, and every node's draft logits those of rama_q8_forward after the prefix and the node's path.
 * rama_q8_spec_begin_model_tree: rama_q8_spec_begin_model's contract and refusals, plus RAMA_EINVAL for n_branch outside 1..4,
 * n_rows outside 2..16 and n_branch > vocab_size.  Checks come first: a refusal leaves a running chain as it was.  It also sizes
 * the tree store and the draft tree store, [dn_layers][R-1][ddim] floats twice, outside any capture.  rama_q8_spec_steps answers
 * RAMA_EINVAL once either model or either run state is freed.
 * rama_q8_spec_model_stats and rama_q8_spec_tree_stats both answer on this chain: draft_passes = sum cap, draft_rows_fed = the live
 * draft rows (catch-up rows included), drafts = sum m, rows_fed = sum (m + 1), accepted = sum a; off_trunk_* and nodes_hist as above.
 * rama_q8_spec_model_tree_shape and _candidates are HOST-ONLY pure functions, RAMA_EINVAL (negative) on a bad argument.  _shape
 * (cap in 0..15) returns m and fills parent_out / depth_out / rank_out[0..m) with nodes 1..m.  _candidates (n in 0..3, n <
 * vocab_size, rank0_token in the vocabulary) fills out[0..n) with ranks 1..n and returns n.
 * rama_q8_spec_model_tree_last synchronises and reports the last step's tree as the device built it: tok / parent / depth / picks
 * [0..m] (>= 16 entries each; node 0 the root), path[0..a] (>= 16 entries), *m and *a.  RAMA_EINVAL on a chain begun any other way. */
int  rama_q8_spec_begin_model_tree(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, const rama_run_state *state,
                                   const rama_config *dcfg, const rama_q8_weights *dw, const rama_run_state *dstate,
                                   const int32_t *context_host, int n_context, const rama_q8_spec_plan *plan, int n_branch, int n_rows);
int  rama_q8_spec_model_tree_shape(int cap, int n_branch, int n_rows, int32_t *parent_out, int32_t *depth_out, int32_t *rank_out);
int  rama_q8_spec_model_tree_candidates(const float *logits_host, int vocab_size, int rank0_token, int n, int32_t *out);
int  rama_q8_spec_model_tree_last(rama_ctx *ctx, int32_t *tok, int32_t *parent, int32_t *depth, int32_t *picks, int32_t *path,
                                  int *m, int *a);

/* SPECULATION INSIDE THE SERVING CHAIN: a DECODE slot's drafts fill the rows no slot wants.  A step of the
 * serving chain costs its weight pass of max_rows rows whatever they hold, and rows at consecutive positions of one sequence
 * are exact (the speculative chain above); so a slot may put drafted tokens into rows that would otherwise be idle, and take
 * several tokens out of one step.  Opt-in per chain and per slot: a chain begun with rama_q8_serve_begin is untouched.
 *
 * TEXT.  A slot's text is s = context ++ outputs, L = n_context + n_out tokens; on such a chain the slot's context buffer holds
 *   s contiguously (n_context + max_new <= seq_len, so it fits) and every emitted token is appended to it on the device.
 * DRAFT, per DECODE slot with n_draft > 0, at every step: exactly
 *   rama_q8_spec_draft(hint, n_hint, s, L, n_draft, ngram, room),  room = min(seq_len - 1 - P, max_new - n_out - 1),  P = L - 1
 *   (P is the slot's cursor) -> want[i] drafts d[i][0..want).  PROMPT, FREE and DONE slots, and slots with n_draft == 0, want 0.
 * SCHEDULE (rama_q8_serve_spec_plan_step).  First rules 1-3 of the serving chain, unchanged: one row per DECODE slot, one per
 *   PROMPT slot, the rows left over to PROMPT slots in ascending slot index.  Then
 *   3a. the rows still left go to the DECODE slots' drafts in ascending slot index, slot i being granted min(want[i], left);
 *   4.  the rest are idle.
 *   Ingestion is certain work and a draft is a bet, so prompts go first.  Rows are laid out by slot index as before; a DECODE
 *   slot's rows are tok, d[0..granted) at positions cursor .. cursor + granted; idle rows last.  With every want == 0 the table
 *   is rama_q8_serve_plan_step's, except that the logits flag below is per row.
 * LOGITS.  Every row of a DECODE slot and the final context row of a PROMPT slot are classified and picked: the final norm, the
 *   quantizer and the classifier run over all max_rows rows in place (no gather), the sampler's records are per row, and
 *   pick_r = Device::sample(logits_r) with the slot's temperature, topp and u.  A row's `logits` flag (rama_q8_serve_stats,
 *   rama_q8_serve_spec_plan_step) is 1 for exactly those rows.
 * ACCEPT, per slot.  A PROMPT slot inside its context moves its cursor on; at its final context position it records its one
 *   pick and becomes DECODE (or DONE), as on any serving chain.  A DECODE slot takes
 *   rama_q8_spec_accept(d, granted, picks of its rows, stop_token, max_new - n_out): the emitted tokens go to its output, to its
 *   ring words in order and to its text; its token becomes the last one emitted, its cursor advances by the number emitted, and
 *   it becomes DONE -- the finished word stored after the ring words -- when the rule says finished.
 * Slot i's tokens are still, bit for bit, those of rama_q8_generate on that sequence alone, cut at the stop token, whatever
 * the drafts, the hints, the neighbours, max_rows and the graph mode: row j of a slot gets the bits of its own rama_q8_forward
 * provided the rows before it carry the right tokens (8.5), rows of different slots do not interact (8.1-8.3), and only picks
 * behind verified drafts are emitted.  Cache rows below a slot's cursor hold that run's bits and are never rewritten, so
 * rama_q8_kv_fork from a live speculating slot (rows below what earlier enqueued work has written as accepted, i.e. below its
 * cursor) and prompt caching stay exact.  UNLIKE a plain serving chain, rows AT AND BEHIND the cursor, up to
 * n_context - 2 + max_new, may hold the rows of rejected drafts: each is rewritten by the step that feeds its position before
 * any attention reads it.  Nothing at or beyond row n_context - 1 + max_new is ever written.
 *
 * rama_q8_serve_begin_spec: rama_q8_serve_begin with its checks, plus 0 <= n_draft_cap <= 15 and 0 <= hint_cap < 2^30 (RAMA_EINVAL).
 * Everything is sized here, outside any capture: the serving chain's tables, a hint buffer of hint_cap tokens and draft / pick
 * arrays per slot, logits flags, sampler records and sampler slices for max_rows rows.  One serving chain per context, of
 * either kind; rama_q8_serve_end, _steps, _poll, _tokens, _stats, the `live` rules and the graph rules are the same entries.
 * rama_q8_serve_admit_spec: rama_q8_serve_admit_at (n_cached may be 0) with the slot's drafting fields; its checks in its
 * order, then RAMA_EINVAL on a chain not begun with rama_q8_serve_begin_spec, for spec == NULL, n_draft outside
 * [0, n_draft_cap], ngram outside 1..4, n_hint outside [0, hint_cap], n_hint > 0 with hint == NULL, a hint token outside the
 * vocabulary.  rama_q8_serve_admit and rama_q8_serve_admit_at on such a chain admit with n_draft = 0.
 * rama_q8_serve_spec_plan_step is HOST-ONLY (no context, no GPU): the schedule above as a pure function of the slot table and
 * want[n_slots] (0..15 each; non-zero only for a DECODE slot, and then <= max_new - n_out - 1) -> rows_out[max_rows] and
 * granted_out[n_slots].  The device scheduler produces exactly this table.
 * rama_q8_serve_spec_stats synchronises.  steps and rows_decode / rows_prompt / rows_idle as rama_q8_serve_stats (rows_decode
 * counts a DECODE slot's first row only), rows_draft and drafts_wanted as the scheduler counted them, drafts_granted,
 * drafts_accepted and accepted_hist[a] (DECODE slot-steps that accepted a drafts) as the accept launch summed them --
 * rows_draft == drafts_granted --, tokens_emitted (every token recorded, a PROMPT slot's first one included), and per slot the
 * last step's wanted and granted drafts (0 for a slot admitted since).  RAMA_EINVAL on a chain begun without drafts. */
typedef struct {
    int32_t n_draft, ngram;                     /* K in 0..n_draft_cap, N in 1..4 */
    const int32_t *hint; int32_t n_hint;        /* a text to look up in besides the slot's own; may be NULL / 0 */
} rama_q8_serve_spec;
typedef struct {
    uint64_t steps, rows_decode, rows_draft, rows_prompt, rows_idle;
    uint64_t drafts_wanted, drafts_granted, drafts_accepted, tokens_emitted;
    uint64_t accepted_hist[16];
    int32_t n_slots, max_rows, n_draft_cap, hint_cap;
    int32_t last_want[128], last_granted[128];
} rama_q8_serve_spec_report;
int  rama_q8_serve_begin_spec(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, int n_slots, int max_rows,
                              int max_new_cap, int n_draft_cap, int hint_cap);
int  rama_q8_serve_admit_spec(rama_ctx *ctx, int slot, const rama_run_state *state, const int32_t *context_host, int n_context,
                              int n_cached, const rama_q8_serve_plan *plan, const rama_q8_serve_spec *spec);
int  rama_q8_serve_spec_plan_step(const rama_q8_serve_slot *slots, int n_slots, int max_rows, const int32_t *want,
                                  rama_q8_serve_row *rows_out, int32_t *granted_out);
int  rama_q8_serve_spec_stats(rama_ctx *ctx, rama_q8_serve_spec_report *out);

/* MODEL DRAFTS INSIDE THE SERVING CHAIN: the chain above with the n-gram lookup replaced, per slot, by the next
 * tokens of a SMALL Q8 MODEL over the same vocabulary -- the drafting of rama_q8_spec_begin_model, for many sequences at once.  A
 * third, opt-in kind of Q8 serving chain: chains begun with rama_q8_serve_begin or rama_q8_serve_begin_spec are untouched.
 * Every slot that drafts has a draft run state of its own and a draft cursor Dc: rows 0..Dc-1 of the draft cache belong to the
 * slot's text s.  A step, one graph replay on one stream:
 *   OPEN.  A DECODE slot with n_draft > 0 wants min(n_draft, seq_len - 1 - P, max_new - n_out - 1) drafts, every other slot 0.
 *     No draft exists yet; the count is all the scheduler needs.  Such a slot feeds s[Dc..P] to the draft model in the first
 *     draft pass -- one row, or two when the step before accepted all it was granted (the catch-up row) -- WHATEVER it is then
 *     granted: the pass is in the graph anyway, and feeding keeps P - Dc in {0, 1} on steps where the prompts take every row.
 *   SCHEDULE.  rama_q8_serve_spec_plan_step's rule over those wants, unchanged: prompts first, then g[i] = min(want, left) in
 *     ascending slot index.  The draft rows' tokens are filled in by the passes below.
 *   DRAFT.  n_draft_cap passes of the draft model, all drafting slots at once: 2 n_slots rows (slot i's rows 2i, 2i + 1), then
 *     n_slots rows (slot i's row i).  After pass j, for j < g[i]: d[i][j] = Device::sample of slot i's last live row with the
 *     slot's own temperature, topp and u -- the target's rule --, which becomes the token of the slot's target row j + 1, the
 *     draft the accept rule compares, and the slot's row (d[j], P + j + 1) of pass j + 1, live only while j + 1 < g[i].  Idle
 *     draft rows have position -1: they write nothing and nothing is read through them.
 *   VERIFY.  The target's pass over max_rows rows, the picks per row and the accept rule per slot, as on a chain begun with
 *     rama_q8_serve_begin_spec.
 *   CLOSE.  Dc' = L + min(a, max(g - 1, 0)), L as the step opened; on a finishing step it stops at the new L.
 * Slot i's tokens are still, bit for bit, rama_q8_generate's on that sequence alone: the drafts only choose which rows are
 * verified.  The cache contract of the target's run states is rama_q8_serve_begin_spec's; the draft run states follow the same
 * one under the draft model (rows below Dc are those of a rama_q8_prefill of the same tokens with it; nothing at or beyond row
 * n_context - 1 + max_new is written).
 *
 * rama_q8_serve_begin_model: rama_q8_serve_begin_spec with hint_cap = 0, plus the draft model.  RAMA_EINVAL for
 * dcfg->vocab_size != cfg->vocab_size, n_draft_cap outside 1..15 and 2 * n_slots > 128 (the first draft pass carries up to two
 * rows per slot, and the token-batch pass takes 128); RAMA_EUNSUP where rama_q8_batch_shape_ok(dcfg) == 0 and wherever
 * rama_q8_serve_begin_spec gives it.  Everything is sized here, outside any capture: a draft batch scratch of 2 * n_slots rows in
 * the draft model's shape, separate from the context's own, and the context's scratches for the larger of the two shapes, so
 * that a rama_q8_prefill with either model between two steps regrows nothing the captured step holds.
 * rama_q8_serve_admit_model: rama_q8_serve_admit_at plus the slot's draft run state and its n_draft in 0..n_draft_cap.  THE
 * CALLER'S CONTRACT: rows 0..n_context-1 of `dstate` hold the draft model's rows of the WHOLE context, written by work enqueued
 * earlier on the context's stream (a rama_q8_prefill with the draft model).  RAMA_EINVAL, besides rama_q8_serve_admit_at's, for
 * n_context + max_new > dcfg->seq_len, a dstate that shares a cache with `state`, and a dstate (or state) that a live slot
 * already uses, as draft or as target state.  rama_q8_serve_admit and _admit_at on such a chain admit with n_draft = 0;
 * rama_q8_serve_admit_spec is RAMA_EINVAL: model drafts replace the lookup.
 * rama_q8_serve_model_plan_step is HOST-ONLY: the rule above as a pure function of the slot table, per slot n_draft (0..n_passes)
 * and Dc, seq_len and n_passes = n_draft_cap -> rows_out[max_rows] (the target's table), want_out and granted_out [n_slots], and
 * draft_rows_out[(n_passes + 1) * n_slots]: pass 0's 2 n_slots rows, then n_slots rows per later pass (`logits`: the row is
 * picked from).
 * rama_q8_serve_model_stats synchronises: the live draft passes (slot-steps that fed the draft model count max(g, 1) passes), the
 * live draft rows fed (catch-up rows included), the catch-up rows, and every slot's draft cursor.  rama_q8_serve_spec_stats keeps
 * its meaning on such a chain.  _steps, _poll, _tokens, _stats and _end are the existing entries; rama_q8_serve_steps answers
 * RAMA_EINVAL once either model (rama_q8_model_free), or the target or draft run state of an occupied slot (rama_state_free), is
 * gone. */
typedef struct {
    uint64_t draft_passes, draft_rows_fed, catch_up_rows;
    int32_t n_slots, n_draft_cap;
    int32_t draft_cursor[128];
} rama_q8_serve_model_report;
int  rama_q8_serve_begin_model(rama_ctx *ctx, const rama_config *cfg, const rama_q8_weights *w, const rama_config *dcfg,
                               const rama_q8_weights *dw, int n_slots, int max_rows, int max_new_cap, int n_draft_cap);
int  rama_q8_serve_admit_model(rama_ctx *ctx, int slot, const rama_run_state *state, const rama_run_state *dstate,
                               const int32_t *context_host, int n_context, int n_cached, const rama_q8_serve_plan *plan, int n_draft);
int  rama_q8_serve_model_plan_step(const rama_q8_serve_slot *slots, int n_slots, int max_rows, int seq_len, const int32_t *n_draft,
                                   const int32_t *draft_cursor, int n_passes, rama_q8_serve_row *rows_out, int32_t *want_out,
                                   int32_t *granted_out, rama_q8_serve_row *draft_rows_out);
int  rama_q8_serve_model_stats(rama_ctx *ctx, rama_q8_serve_model_report *out);

/* DRAFTS IN THE IDLE ROWS OF THE PARITY-MODE SERVING CHAIN: the three entries above for an fp32 model, argument
 * for argument, with rama_weights and the same plan, spec and report records.  A parity pass runs in tiles of 32 rows and a tile
 * costs its whole weight pass whatever its rows hold, so the rows of a live tile that no slot wants are paid for: a DECODE
 * slot's n-gram drafts take them.  THE SCHEDULE, LOGITS flags and ACCEPT rule are those above (the same kernels); a DECODE
 * slot's rows tok, d[0..granted) sit at consecutive positions like a prompt chunk and may straddle a tile boundary.  The final
 * norm and the classifier run over the pass's rows where they sit, tile by tile: a tile none of whose rows carries logits --
 * wholly idle, or holding only rows inside a context -- is skipped before its first load.  Slot i's tokens are still, bit for
 * bit, parity-mode rama_generate's on that sequence alone, cut at the stop token, whatever the drafts, the hints, the
 * neighbours, max_rows, the tile a row lands in and the graph mode.
 * THE CACHE CONTRACT OF SUCH A CHAIN.  Rows below a slot's cursor hold the solo run's bits and are never rewritten.  UNLIKE the
 * plain chain (nothing behind a slot's last position is written), rows AT AND BEHIND a speculating slot's cursor, up to
 * n_context - 2 + max_new, may hold the rows of rejected drafts: each is rewritten by the step that feeds its position before
 * any attention reads it.  Nothing at or beyond row n_context - 1 + max_new is ever written.  Fork from a live speculating
 * slot only rows below its cursor.
 * rama_serve_begin_spec: rama_serve_begin's checks, then 0 <= n_draft_cap <= 15 and 0 <= hint_cap < 2^30 (RAMA_EINVAL).
 *   Everything is sized here, outside any capture: the drafting tables, per-row sampler records, sampler slices and logits for
 *   max_rows rows.  One fp32 serving chain per context, of either kind; rama_serve_end, _steps, _poll, _tokens, _stats, the
 *   `live` rules, the re-capture when the chain-order copies move and the parity-mode rule are the same entries'.
 * rama_serve_admit_spec: rama_serve_admit_at (n_cached may be 0) with the slot's drafting fields; its checks in its order --
 *   n_context + max_new <= seq_len among them --, then RAMA_EINVAL as rama_q8_serve_admit_spec.  rama_serve_admit and
 *   rama_serve_admit_at on such a chain admit with n_draft = 0.
 * rama_serve_spec_stats: as rama_q8_serve_spec_stats; RAMA_EINVAL on a chain begun with rama_serve_begin. */
int  rama_serve_begin_spec(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w, int n_slots, int max_rows,
                           int max_new_cap, int n_draft_cap, int hint_cap);
int  rama_serve_admit_spec(rama_ctx *ctx, int slot, const rama_run_state *state, const int32_t *context_host, int n_context,
                           int n_cached, const rama_q8_serve_plan *plan, const rama_q8_serve_spec *spec);
int  rama_serve_spec_stats(rama_ctx *ctx, rama_q8_serve_spec_report *out);

/* MODEL DRAFTS IN THE IDLE ROWS OF THE PARITY-MODE SERVING CHAIN: rama_q8_serve_begin_model / _admit_model /
 * _model_stats argument for argument, for an fp32 TARGET in parity mode (rama_weights) and a Q8 DRAFT model (dcfg, dw) over the
 * same vocabulary -- rama_q8_model_from_f32 makes one from an fp32 model.  The same plan and report records;
 * rama_q8_serve_model_plan_step is the host plan of both stacks.  A step is the Q8 chain's OPEN, SCHEDULE and DRAFT PASSES (the
 * same kernels, the draft passes on the chain's own batch scratch), then the verify half of rama_serve_begin_spec's step -- the
 * tiles' guard entries, the pass tile by tile, the final norm and classifier where the rows sit, the picks, the accept rule --,
 * then CLOSE.  One graph replay on one stream, one captured graph for the chain's life.  Slot i's tokens and target cache rows
 * are, bit for bit, parity-mode rama_generate's on that sequence alone; the draft cache contract is rama_q8_serve_begin_model's.
 * rama_serve_begin_model: rama_serve_begin_spec's checks with hint_cap = 0 (parity mode only: RAMA_EUNSUP otherwise, at _steps
 *   too), and rama_q8_serve_begin_model's of the draft model, n_draft_cap in 1..15 and 2 * n_slots <= 128.  Sized here, outside
 *   any capture: the drafting tables, logits for max_rows rows, sampler slices for max(max_rows, 2 * n_slots) rows, the draft
 *   batch scratch for 2 * n_slots rows, and the context's Q8 scratches for the draft's shape (what a rama_q8_prefill of the draft
 *   cache runs on).  THE CAPTURED STEP HOLDS NONE OF THE CONTEXT'S Q8 SCRATCHES: a Q8 chain or a prefill with a larger Q8 model
 *   on the same context may regrow them between two steps.  (The sampler's slices are shared: whoever regrows them drops every
 *   captured step, this one included, and it is captured again.)
 * rama_serve_admit_model: rama_q8_serve_admit_model's contract and refusals in this entry's words; `state` is an fp32 run state
 *   of the target, `dstate` a run state of the draft model.  rama_serve_admit and _admit_at on such a chain admit with
 *   n_draft = 0; rama_serve_admit_spec is RAMA_EINVAL.
 * rama_serve_steps answers RAMA_EINVAL once the target (rama_model_free), the draft model (rama_q8_model_free), or the target or
 *   draft run state of an occupied slot (rama_state_free) is gone.  rama_q8_kv_fork refuses a destination that is a live slot's
 *   draft run state, on either chain.
 * rama_serve_model_stats: as rama_q8_serve_model_stats; RAMA_EINVAL on a chain not begun with rama_serve_begin_model. */
int  rama_serve_begin_model(rama_ctx *ctx, const rama_config *cfg, const rama_weights *w, const rama_config *dcfg,
                            const rama_q8_weights *dw, int n_slots, int max_rows, int max_new_cap, int n_draft_cap);
int  rama_serve_admit_model(rama_ctx *ctx, int slot, const rama_run_state *state, const rama_run_state *dstate,
                            const int32_t *context_host, int n_context, int n_cached, const rama_q8_serve_plan *plan, int n_draft);
int  rama_serve_model_stats(rama_ctx *ctx, rama_q8_serve_model_report *out);

/* CANCEL in both serving chains: end requests from outside.  One entry per stack, one body; chains begun with
 * _begin, _begin_spec and _begin_model alike.  A slot of the list that is PROMPT or DECODE when the launch runs becomes DONE
 * with the finished word RAMA_SERVE_CANCELLED; to every kernel of a step it is a slot that ran out of budget at that point.  Its
 * cursor, n_out, tokens, ring row and cache rows stay as they are, so the tokens polled until the word shows are the request's,
 * and the sequence can be continued later on the same run state with the bits of an uninterrupted run: _admit_at with the old
 * context plus the tokens produced, n_cached = the slot's cursor (rama_*_serve_stats; at most n_context - 1) and the budget that
 * is left.  A slot whose occupant finishes by itself before the launch runs keeps the word 1 and all its tokens.
 * Like an admission: stream-ordered on the context's stream, never synchronises, leaves the captured step alone, legal between
 * any two _steps calls.  The set travels as launch arguments: no copy is staged.  Everything is checked first and a refusal
 * leaves the chain as it was: RAMA_EINVAL for no chain, a NULL list with n > 0, n < 0 or n > 128, a slot index outside the
 * table.  Duplicates are fine.  A slot the host can already see is not live -- never admitted, or its finished word set -- is
 * skipped without error; if nothing is left, nothing is launched.  The host's books do not change at the cancel: the slot is
 * admissible once the host sees the word (_poll reports it as it is: 0, 1 or RAMA_SERVE_CANCELLED), and rama_state_free on the
 * occupant's run state before that still ends the chain. */
#define RAMA_SERVE_CANCELLED 2      /* the finished word of a slot ended by a cancel */
int  rama_q8_serve_cancel(rama_ctx *ctx, const int32_t *slots, int n);
int  rama_serve_cancel(rama_ctx *ctx, const int32_t *slots, int n);

/* ---------------------------------------------------------------- measurement
 * HIP events on the context's stream (the stream the kernels are launched on). */
int  rama_timer_start(rama_ctx *ctx);
int  rama_timer_stop(rama_ctx *ctx, float *elapsed_ms);      /* synchronises */
/* Per-kernel timing: while enabled, every launch of kernel class `kernel_id` on the fused
 * path is bracketed by an event pair (eager mode only).  Classes: */
#define RAMA_K_QKV   0   /* rmsnorm + Wq|Wk|Wv matvec + RoPE + cache append */
#define RAMA_K_ATTN  1   /* multi-head attention */
#define RAMA_K_WO    2   /* Wo matvec + residual */
#define RAMA_K_W13   3   /* rmsnorm + W1|W3 matvec + SiLU*gate */
#define RAMA_K_W2    4   /* W2 matvec + residual */
#define RAMA_K_CLS   5   /* final rmsnorm + classifier matvec */
#define RAMA_K_NORM  6   /* an rmsnorm launch of its own (parity mode: the exact sequential sum of squares) */
#define RAMA_K_SAMPLE 7  /* Device::sample on the device: argmax, or the top-p sampler's launches (event records around them) */
#define RAMA_K_COUNT 8
int  rama_kprof_enable(rama_ctx *ctx, int kernel_id, int max_records);
int  rama_kprof_read(rama_ctx *ctx, int *n_launches, double *total_ms);  /* synchronises, disables */

#ifdef __cplusplus
}
#endif
#endif /* RAMA_HIP_H */
