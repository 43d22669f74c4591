// ctx.hpp -- what the library's C-ABI translation units (rama_api.hip, batch_api.hip, chain_api.hip, q8_api.hip, q8_serve_api.hip, q8_spec_api.hip) share: the context, the error plumbing, graph
// capture, the launch macros, and declarations of what each defines for the others.  Internal: not installed, not part of the C ABI.
//
// The library is built WITHOUT relocatable device code, so a kernel or a __device__ global lives in the code object of the translation
// unit that instantiates / defines it (DESIGN.md "Translation units").  Hence the launchers below: whoever needs attention_chain_kernel,
// rmsnorm_chain_kernel or the sampler's kernels calls chain_api.hip, the one translation unit that owns them.
#pragma once
#include "../../include/rama_hip.h"
#include "kernels.hpp"
#include "topp_sort.hpp"        // ToppRow, ToppStats, ToppBatchParams
#include "ref_order.hpp"        // RefAttnParams
#include "chain_params.hpp"     // ChainParams, GemmChainParams, CEPI_* / CNORM_*
#include "q8_serve_tables.hpp"  // ServeTables
#include "q8_spec_tables.hpp"   // SpecTables
#include "q8_tree_tables.hpp"   // TreeTables, TreeAttnParams
#include "q8_serve_spec_tables.hpp"     // ServeSpecTables
#include "q8_serve_model_tables.hpp"    // ServeModelTables

#include <hip/hip_ext.h>   // hipExtLaunchKernelGGL: start/stop events carried by the dispatch itself

#include <algorithm>
#include <cstdint>
#include <vector>

using namespace rama;

extern "C" int rama_internal_note_write(rama_ctx* ctx, const float* dst, size_t n);                    // model.hip: an entry is about to write [dst, dst + n) on the device
// every entry that writes device memory the caller names says so first: a chain-order copy DERIVED from a tensor uploaded by the caller (an adopted model's, a
// view's) must not outlive a device-side write into that tensor (rama_fill_synth re-seeding it, an op's output landing in it).  Two atomic loads when the
// range lies outside everything copies were derived from.
#define RAMA_WRITES(c, p, n) do { if ((p) && (n)) { const int rw_ = rama_internal_note_write((c), (p), (size_t)(n)); if (rw_) return rw_; } } while (0)

// ---------------------------------------------------------------- error plumbing

#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail((int)e_, #expr, __FILE__, __LINE__); } while (0)
#define REQUIRE(cond, code, msg) do { if (!(cond)) return fail((code), msg, __FILE__, __LINE__); } while (0)
#define LAUNCHCHK() HIPCHK(hipGetLastError())

// ---------------------------------------------------------------- context

constexpr int kSmallAttnPosDefault = 256;
constexpr size_t kAttnChainMaxLds = 136 * 1024;      // dynamic LDS attention_chain_kernel may ask for (allowed once per device in rama_ctx_create)
constexpr int kSpreadAttnPos = 128;        // parity mode: from this position on the attention is two launches spread over the chip (chain.hpp; "spread_pos": 187 against 184 tok/s at positions 124..179, 178 against 152 at 800)
constexpr int kLongAttnPos = 256;          // parity mode: attention_chain_kernel runs 16 waves per head from this position on

struct KProf {
    int kernel_id = -1;
    int max_records = 0;
    int used = 0;
    std::vector<hipEvent_t> ev;   // 2 per record
};

// a captured, instantiated graph: made by capture_graph, launched by replay_graph
struct CapturedGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool handoff = false;              // [r6] the captured launches hand data over inside a kernel (a leader norm, attention+Wo, the one-launch stage): a REPLAY must mark
                                       // the error word as worth reading too (rama_ctx::handoff_dirty is otherwise only set where such a launch is enqueued)
};
struct GraphCache {
    CapturedGraph cg;
    // identity of what was captured
    rama_config cfg{};
    rama_weights w{};
    rama_run_state s{};
    bool valid = false;
    int steps = 1;                     // decode steps in the captured graph
    unsigned long long copies_gen = 0; // model.hip's generation of derived weight copies at capture: a graph holds their addresses, and ANOTHER context may free them
};

// The peephole recorder of the 1:1 Device<T> ops (rama_api.hip "the 1:1 op recorder"): an op entry may RECORD its call instead of launching it, and
// the next entry either folds its own call into what is recorded or issues what is recorded first.  Whatever else enters the library issues it too
// (RAMA_ENTER, flush_pending).  Only on a stream the context owns; every record has its switch among rama_ctx's tune_* ("rope_batch" = 0: every
// call a launch, ...).
//
//   rope  [r5] a run of Device::apply_position calls on consecutive heads (infer.rs:25-29: n_heads calls per layer, 1 024 per llama2-7B token, each a
//         launch of its own) is ISSUED AS ONE LAUNCH: a call only records (q, k, table rows, head size), the next call extends the run when it
//         continues it ("rope_batch")
//   mm    a run of up to three parity-mode Device::matmul calls with the same activations and shape on chain-order copies (infer.rs:20-23: Wq, Wk,
//         Wv; :41-42: W1, W3): one launch over all their row groups ("matmul_batch").  A Device::array_add of a recorded matmul's output becomes
//         that launch's residual epilogue ("resid_fold")
//   nrm   a parity-mode Device::rmsnorm waits for the run of matmuls on its output (infer.rs:19-23, :40-42): the run's launch then carries the norm
//         as its leader workgroup (chain.hpp CNORM_LEAD: the exact sum of squares while the row groups' weights are already on their way), and
//         the leader also stores the normalised vector the call was asked for; mm.norm says that the pending run takes it.  No run on its output:
//         the norm is a launch of its own ("norm_fold").  The leader's tagged words rotate through a range of their own (lead_next, the second
//         half of rama_ctx::lead_slots); the epoch advances when the range wraps
//   ew    Device::sinu waits for the Device::array_mult on the same vector (infer.rs:44-45), one Device::copy_from_slice for the next (:32-33): one
//         launch per pair ("ew_batch")
//
// THE INVARIANT.  Pending together may be: a norm and the run of matmuls on its output; a run of three matmuls, the rotations of its first two
// outputs over their heads and the copy of its second output into a cache row (infer.rs:20-33, which the second copy turns into ONE launch with the
// Wq|Wk|Wv epilogue: "qkv_fold").  Otherwise at most ONE record is pending: whoever records issues the others first.  Records are issued in the
// order they can have been made: the norm and the run, the rotations, the elementwise op (flush_pending).
struct PendingOps {
    struct { float* q = nullptr; float* k = nullptr; const float* pr = nullptr; const float* pi = nullptr; int hs = 0, count = 0; } rope;
    struct { const float* w[3]; float* o[3]; const float* x = nullptr; int K = 0, rows = 0, count = 0; bool norm = false; } mm;
    struct { float* o = nullptr; const float* x = nullptr; const float* w = nullptr; int n = 0; bool on = false; } nrm;
    struct { int kind = 0; float* t = nullptr; const float* s = nullptr; size_t n = 0; } ew;      // 1: sinu(t, n); 2: copy(t, s, n)
    int lead_next = 0;                     // the leader word the next recorded norm takes
    unsigned long long op_launches = 0;    // launches made for the 1:1 op entries and by flush_pending (rama_internal_op_launches): a fold that stops happening shows here
    int any() const { return rope.count | mm.count | ew.kind | (int)nrm.on; }
};

struct rama_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    Ctl* ctl = nullptr;          // device cursor
    int* forced = nullptr;       // device forced-token list
    int forced_cap = 0;
    int* out = nullptr;          // device produced-token list
    int out_cap = 0;
    int* ring = nullptr;                    // host-pinned, device-mapped: ring[i] = token i of the chained loop + 1 (0: not produced yet)
    int* ring_dev = nullptr;
    int ring_hi = 0;                        // entries that may be non-zero
    int* argmax_result = nullptr;   // device int for rama_sample_argmax
    int* pinned_int = nullptr;      // host pinned
    int* pinned_tok = nullptr;      // host pinned staging: token ids + a SeqSlot table of a token-batch pass
    bool graph_mode = false;
    struct StageGraph { GraphCache g; rama_stage st{}; int variant = 0; unsigned long long used = 0; };
    std::vector<StageGraph> sg;        // rama_forward / rama_forward_stage* in graph mode: one graph per (state, stage, attention variant)
    unsigned long long sg_clock = 0;
    GraphCache gc[8];                  // [0..3] one step per graph, [4..7] tune_graph_steps steps per graph; by attention variant (attn_variant)
    KProf kp;
    int cu_count = 0;
    hipEvent_t cur_start = nullptr, cur_stop = nullptr;   // events the next profiled launch carries
    int tune_geom = 3;
    int tune_w13i = 1;                     // 1: the fused W1|W3 launch streams the model's row-interleaved copy when there is one
    int tune_solo = -1;                    // small-K matvecs, one wave per row group: 1 on, 0 off, -1 = rows of <= 2048 floats
    int tune_ref_order = 0;                // 1: every op in the reference's own rounding order: bit-comparable with the CPU path ("parity mode")
    int tune_tol = 0;                      // "ref_order" = 2, the tolerance-mode experiment: the chain-order matvecs (the reference's rounding sequence) with the layer
                                           // norms folded into them as tree-shaped sums and the fast attention -- 0.72 of the roofline, but 1.4e-4 from the CPU path at
                                           // llama2-7B x 200 positions, no closer than the fast path; kept as the per-op A/B instrument
    int tune_bar = 0;                      // [r6] "ref_order" = 3, BAR mode: parity mode's launches (chain-order matvecs, exact norms, the exact attention) up to position
                                           // "bar_pos", the FAST path's attention from there on -- not bit-identical, but measured <= 1e-4 from the CPU path over the WHOLE
                                           // 2 048-position context at llama2-7B depth (profiles/r06_tolerance_sweep_7b_2048pos.jsonl: fast attention at every position 9.75e-5;
                                           // every other single swap >= 1.3e-4 already at 200 positions), where the exact attention costs 25 us a layer at position 1 900
    int tune_bar_pos = kSpreadAttnPos;     // ... the first position that takes the fast attention (clamped to the spread attention's switch and to 256: below it one exact variant)
    bool bar_fast = false;                 // ... the steps being enqueued / captured are at or behind it
    int tune_lane_reduce = 0;              // [r6] parity mode: the order of the final 4-lane sum of cpu.rs:148 `v.reduce_add()` (wide::f32x4 leaves it to the build's target
                                           // features): 0 pairwise (l0+l1)+(l2+l3), 1 strided (l0+l2)+(l1+l3), 2 sequential ((l0+l1)+l2)+l3 -- the oracle's switch of the same name
    int tune_tol_mask = 0;                 // tolerance mode, A/B: ops swapped for the fast path's (1 qkv, 2 wo, 4 w13, 8 w2, 16 cls) or parity mode's (32 attention, 64 norms)
    int tune_chain = 1;                    // parity mode streams the model's chain-order weight copy (chain.hpp); 0: ref_order.hpp's one-thread-per-row kernels
    int tune_chain_d = 0;                  // chain-order matvec geometry: 0 = by row groups per CU, else 100 W + D (waves per group, blocks per wave in flight)
    // device top-p sampler (Device::sample for temperature != 0); temperature 0 = argmax
    float samp_T = 0.0f, samp_topp = 0.9f, samp_u = 0.0f;
    float* topp_keys[2] = {nullptr, nullptr}; int* topp_vals[2] = {nullptr, nullptr};
    float* topp_prefix = nullptr; int* topp_m = nullptr; unsigned* topp_err = nullptr;
    int topp_cap = 0;
    float* topp_bp = nullptr; int* topp_bi = nullptr; int* topp_bcount = nullptr;       // topp_sort.hpp
    int* topp_racc = nullptr;               // pair-wise ranking: the accumulators, one per block slot
    unsigned long long* topp_rk = nullptr;  // small-block path: count << 48 | mass accumulators, one per block slot
    unsigned long long* topp_bm = nullptr;  // ... the blocks' running masses
    float* topp_approx = nullptr;           // ... the mass in front of every entry of the whole order
    void* topp_dist = nullptr;              // topp_pick_dist_kernel's hand-off words: items | hdr | cross | epoch | bad
    bool topp_dist_dirty = false;           // ... a distributed pick has been enqueued since its error word was last read (else a synchronising exit need not read it)
    int tune_spread_pos = kSpreadAttnPos;   // parity mode: from this position on the attention is spread over the chip (scores | softmax + values)
    int tune_attn_fv = 1;                   // parity mode, long contexts: softmax + value chains as one launch (0: two launches)
    int tune_topp_dist = 1;                 // 1: the running sums by up to 32 workgroups in one launch (topp_pick.hpp); 0: one workgroup's scan rounds
    ToppStats* topp_stats = nullptr;        // small-block path: partial softmax statistics, one per 1024 logits
    int tune_topp_block = 1024;             // entries per sorted block on the pair-ranking path: 1024 or 512 (statistics once + 8- / 4-wave sorts) or 2048 (round 3's block sort)
    int tune_topp_pairs = 1;                // 1: the ranking as (block, block) pairs spread over the chip + a scatter launch; 0: one workgroup searches all blocks in its LDS
    int tune_norm_in_gemm = 1;              // token-batch passes: the rmsnorm's per-token scale is applied by the consuming GEMM (one launch per norm instead of two)
    int tune_tiled = 1;                     // token-batch GEMMs read the model's tile-order weight copy when it exists
    int tune_prefill_tok = kMfMaxTok;       // prompt positions per weight pass of rama_prefill: 128 (needs the tile-order copies) or 64
    int tune_prefill_attn = 1;              // 1: prefill passes run attention as MFMA tiles, 16 queries per workgroup (prefill_attn.hpp)
    int tune_graph_steps = -1;              // decode steps captured per hipGraph (the cursor lives on the device, so steps are identical); -1: 4 for dim <= 1024, else 1
    int tune_attn_u = 8;                    // cache rows per lane and round in the split-T attention (8 | 16; 16 measured no faster)
    int tune_topp_sort = 1;                 // 0: ranks through global memory (topp_rank_global_kernel) for every vocabulary size
    int tune_topp_keep_sums = 0;            // 1: the scan sampler also writes its running sums to global memory (tests)
    // the batched top-p sampler (rama_sample_topp_batch_dev, the sampled chained batch; topp_sort.hpp ROWS kernels): one scratch slice
    // per row, sized by the op's first call or by rama_decode_batch_begin_sampled -- never inside a step, which may be captured
    struct ToppBatchScratch {
        int rows = 0; size_t rstride = 0;  // rows x rstride entries per slice array
        float* keys = nullptr; int* vals = nullptr; float* bp = nullptr; int* bi = nullptr;
        unsigned long long* rk = nullptr; unsigned long long* bm = nullptr;
        int* bcount = nullptr; ToppStats* stats = nullptr; int* m = nullptr;     // rows x kToppRowBlocks, rows x kToppRowBlocks, rows
        ToppRow* rows_dev = nullptr;       // [kMfMaxTok] rama_sample_topp_batch_dev's (T, topp, u) per row, written by a launch
    } tb;
    // Q8 models (rama_q8_forward / rama_q8_generate): the int8 activations and their scales, sized by the first call; graphs of their own
    int8_t* q8_xq = nullptr; float* q8_xs = nullptr; size_t q8_cap = 0;
    struct Q8Graph { CapturedGraph cg; rama_config cfg{}; rama_q8_weights w{}; rama_run_state s{}; int variant = 0; int chained = 0; };
    std::vector<Q8Graph> q8g;
    // Q8 token batches (rama_q8_prefill / rama_q8_decode_batch / the chained batch): row-major scratch for kQ8bMaxTok tokens, sized by
    // the first call (never inside a capture; only the chained batch's step q8c.cg holds it, and goes when it moves), see Q8BatchScratch
    char* q8b_blob = nullptr; size_t q8b_cap = 0;
    int tune_split_pos = -1;               // attention runs split-T (+ combine launch) from this position on; -1 = by model size
    int tune_resid_r2 = 2;                 // Wo / W2 under geometry 3: 0 = 4-row workgroups, 1 = 2 rows x 8 waves (+0.45 %),
                                           // 2 = additionally 16 waves for rows wider than 8192 floats (W2: +1.15 % more), 3 = 16 waves x 4 chunks
    int tune_prefill = 1;                  // 1: rama_generate_greedy runs the forced prompt positions through rama_prefill
    int tune_merge = -1;                   // attention + Wo in one launch: 1 on, 0 off, -1 by model size (on for dim <= 1024:
                                           // +4..8 % at the stories shapes; at llama2-7B +0.9 % short / -2.5 % long contexts)
    int tune_fused = -1;                   // a stage's layers (+ classifier) as one launch (layer_fused.hpp): 1 on, 0 off, -1 on for dim <= 1024
                                           // (stories15M +4 %, stories110M +25 % tokens/s over the separate launches)
    int tune_fused_solo = -1;              // its workgroups alone on their CU (LDS request padded): 1, 0, -1 = for dim > 512 (stories110M: 216 -> 200 us
                                           // per token, a consumer's polls do not queue behind a neighbour's weight requests; stories15M: 89 -> 92)
    tagged_t* fused_hand = nullptr;        // device: its hand-off vectors (tagged words), room for the largest shape it takes
    unsigned* fused_epoch = nullptr;       // device: the tag of the current token, advanced after every launch of the stage kernel
    bool fused_chained = false;            // the step being enqueued ends in a sampler launch, which advances the epoch
    bool fused_epoch_owed = false;         // ... and the stage launch just enqueued relies on that
    int merge_blocks_per_cu[3] = {-1, -1, -1};   // occupancy of attn_wo_kernel<16|32|64> at the LDS size below
    size_t merge_lds[3] = {0, 0, 0};
    unsigned* attn_counter = nullptr;      // device: arrivals of the attention workgroups
    float* attn_part = nullptr;            // split-T partials [n_heads, nsplit, head_size + 4]
    size_t attn_part_floats = 0;
    float* attn_scores = nullptr;          // parity mode, spread attention: the raw scores [n_heads, seq_len] (the softmax+values launch reads them here and
    size_t attn_scores_floats = 0;         // writes the probabilities to the caller's att: no workgroup reads a buffer another one of the launch writes)
    float* pf_blob = nullptr;              // token-batch scratch (tile layout): see BatchScratch
    float* pc_blob = nullptr;              // parity-mode prefill scratch (row-major token batches): see prefill_chain
    size_t pc_floats = 0;
    int tune_chain_lead = 1;               // parity mode, dim > 512: the layer norms' exact sums by a leader workgroup INSIDE the consuming matvec's launch (chain.hpp CNORM_LEAD)
    unsigned long long* lead_slots = nullptr;   // device: one tagged word per (layer, norm), 256 bytes apart
    int tune_chain_norm = 1;               // parity mode, dim <= 512: the layer norms folded into the matvecs that consume them
    int tune_chain_split = 1;              // parity mode: the row groups that do not divide by the compute units walked as half groups (chain.hpp half_from)
    int tune_chain_lead_w = 0;             // parity mode: waves per row group of the launches with a leader norm (0: by the number of row groups)
    int tune_chain_resid_d = -1;           // parity mode: 100 W + D for the residual products (Wo, W2) only; 0: by the number of row groups like the others; -1: W = 1, D = 32 when a CU holds one group
    PendingOps rec;                        // the recorded 1:1 ops (above); the switches of what it may record and fold:
    int tune_rope_batch = 1;               // runs of apply_position calls are recorded
    int tune_matmul_batch = 1;             // runs of parity-mode matmuls are recorded
    int tune_norm_fold = 1;                // a parity-mode rmsnorm waits for the run on its output
    int tune_qkv_fold = 1;                 // Wq|Wk|Wv, the rotations over all heads and the two cache copies as one launch
    int tune_resid_fold = 1;               // an array_add of a recorded matmul's output becomes that launch's residual epilogue
    int tune_ew_batch = 1;                 // sinu and copy_from_slice are recorded
    int tune_chain_views = 1;              // parity mode, Device::matmul on a matrix of no model: a chain-order copy of the tensor is made on first use
    int tune_prefill_chain = 1;            // parity mode: prompt positions go through the chain-order token-batch kernels (32 per weight pass); 0: one forward() each
    size_t pf_floats = 0;
    int host_pos = -1;                     // position of the next chained decode step (mirrors the device cursor)
    bool split_attn = false;               // variant the steps being enqueued / captured use
    bool long_attn = false;                // parity mode: the position is >= 256 (16 waves per head in attention_chain_kernel)
    bool spread_attn = false;              // parity mode: the position is >= tune_spread_pos (the exact attention as launches spread over the whole chip)
    int variant = 0;                       // attn_variant() of the steps being enqueued / captured
    bool small_attn = false;               // 4-wave attention workgroups (contexts of <= kSmallAttnPos timesteps)
    int tune_small_waves = 8, tune_small_pos = kSmallAttnPosDefault;   // waves per head and position limit of the small-attention variant
    int tune_combine_v = 1;                // split-T combine: 1 = all slice loads up front, 0 = round 1's loop
    int tune_attn_nsplit = 0;              // split-T slices per head: 0 = #CUs / n_heads (<= 16), else 1..32
    int tune_attn_waves = 8;               // waves per split-T workgroup (16, 8 or 4); 8 measured best at llama2-7B, 1000-1900 tokens
    int tune_attn_nt = 1;                  // 1: split-T attention reads the cache rows non-temporally (+2.7 % tokens/s at 1900 tokens)
    int tune_small_attn = -1;              // fewer-wave attention in the decode step: -1 (default) below tune_small_pos where attention
                                           // is not merged with Wo, 0 never, 1 always (below the split threshold)
    unsigned long long* pbar = nullptr;    // device: [1] = error word of the merged attention+Wo launch's bounded spin
    bool handoff_dirty = false;            // a launch with an in-kernel hand-off (attention+Wo, the one-launch stage) has been enqueued since the error word was last read
    const float* embedded_x = nullptr;   // run-state x that already holds emb[ctl.token] (chained decode)
    // rama_decode_batch_begin / _steps: the sequences' cursors live on the device
    struct BatchChain {
        int n_seq = 0, pos_max = 0, out_cap = 0, steps_done = 0;
        int* toks = nullptr;               // [kMfMaxTok] the token each sequence feeds next
        SeqSlot* seqs = nullptr;           // [kMfMaxTok] cache bases + position of every sequence
        int* out = nullptr;                // [kMfMaxTok, out_cap] the tokens produced
        int* ring = nullptr;               // the same, host-pinned and device-mapped: token + 1, 0 = not produced yet (rama_decode_batch_stream_poll)
        int* ring_dev = nullptr;
        rama_config cfg{}; rama_weights w{};
        CapturedGraph cg; int graph_bucket = -1;        // the step captured for contexts of up to 256 * graph_bucket timesteps
        // rama_decode_batch_begin_sampled: a step ends in the batched top-p sampler instead of argmax_batch_kernel
        bool sampled = false;
        ToppRow* rows = nullptr;           // [kMfMaxTok] every sequence's (T, topp, u, forced list)
        int* forced = nullptr; size_t forced_cap = 0;      // the forced lists, one after the other
    } bc;
    // what the three Q8 chains below share, and all that drop_q8_graphs, rama_internal_drop_q8_graphs and the _steps entries need of one (q8_api.hip
    // q8_chains, q8_host.hpp q8_chain_steps): the model it was begun on, whether it may still run, its one captured step.  The chains share procedures, not state.
    struct Q8ChainBase {
        bool live = false;                 // false once the model or a run state the chain still uses has been freed: its _steps entry refuses
        rama_config cfg{}; rama_q8_weights w{};
        CapturedGraph cg;                  // one step, for the chain's whole life: the tables' addresses, nothing of a sequence or a position
        unsigned long long captures = 0;
    };
    // rama_q8_decode_batch_begin / _steps: the same for a Q8 model, with per-sequence ends (a step budget, a stop token).  A state of
    // its own: the fp32 chain above neither sees nor shares any of it.
    struct Q8Chain : Q8ChainBase {
        int n_seq = 0, max_steps = 0, out_cap = 0, steps_done = 0;      // out_cap: row stride of out / ring, >= every sequence's budget
        int* toks = nullptr;               // [kMfMaxTok] the token each sequence feeds next
        SeqSlot* seqs = nullptr;           // [kMfMaxTok] cache bases, position and tokens produced of every sequence
        int* out = nullptr;                // [kMfMaxTok, out_cap] the tokens produced
        int* ring = nullptr;               // the same, host-pinned and device-mapped: token + 1, 0 = not produced yet
        int* ring_dev = nullptr;
        BatchEnds* ends = nullptr;         // device: every sequence's budget (a stop lowers it) and stop token, and where `done` is
        int* done = nullptr;               // [kMfMaxTok] host-pinned and device-mapped: 1 = the sequence has finished
        int* done_dev = nullptr;
        bool sampled = false;              // a step ends in the batched top-p sampler (a row samples, or is forced) instead of argmax_batch_kernel
        ToppRow* rows = nullptr;           // [kMfMaxTok] every sequence's (T, topp, u, forced list)
        int* forced = nullptr; size_t forced_cap = 0;
        std::vector<rama_run_state> states;
    } q8c;
    // What a serving chain keeps whatever its model (q8_serve_api.hip serve_state_* / serve_admit_*): the geometry, the device tables, the admission records,
    // the host-visible rings and the host's view of the slots.  The Q8 chain and the fp32 chain below each have one; they share procedures, not state.
    struct ServeState {
        int n_slots = 0, max_rows = 0, out_cap = 0;       // n_slots 0: no serving chain
        bool sampler = false;              // a step runs the batched sampler's ordering launches (vocab_size <= 32768)
        ServeTables t{};                   // the device tables (ring / done: the device addresses of the two below)
        char* blob = nullptr;              // ... all of them, one allocation
        char* stage = nullptr;             // device: one admission record per slot (a ServeSlot + seq_len tokens)
        char* pinned = nullptr;            // host-pinned: the same, what an _admit entry fills and copies from
        size_t rec_bytes = 0;
        int* ring = nullptr;               // [n_slots, out_cap] host-pinned and device-mapped: token + 1, 0 = not produced yet
        int* done = nullptr;               // [n_slots] host-pinned and device-mapped: 1 = the slot's occupant has finished
        std::vector<rama_run_state> states;   // per slot, the occupant's
        std::vector<char> occupied;        // per slot: admitted, and not yet seen DONE by a call that frees the slot
        std::vector<int> gen;
        unsigned long long steps = 0;
        // a chain begun with rama_q8_serve_begin_spec / rama_serve_begin_spec (q8_serve_spec.hpp): drafts in the rows no slot wants; all of it unused on
        // a chain begun without it
        unsigned long long cancel_launches = 0;   // serve_cancel_kernel launches since the chain began (rama_internal_serve_cancel_launches)
        bool spec = false;
        int n_draft_cap = 0, hint_cap = 0;
        ServeSpecTables st{};              // the device tables (inside blob)
        char* sstage = nullptr;            // device: one spec admission record per slot (a ServeSpecSlot + hint_cap tokens)
        char* spinned = nullptr;           // host-pinned: the same
        size_t srec_bytes = 0;
        // a chain begun with rama_q8_serve_begin_model (q8_serve_model.hpp): a slot's drafts are a second Q8 model's; all of it unused otherwise
        bool model = false;
        rama_config dcfg{}; rama_q8_weights dw{};      // the draft model: the chain dies with it
        std::vector<rama_run_state> dstates;  // per slot, the occupant's draft run state (all NULL: admitted without drafts)
        ServeModelTables mt{};             // the device tables (inside mblob)
        char* mblob = nullptr;
        char* dblob = nullptr;             // the draft passes' batch scratch, a Q8BatchScratch of draft_rows rows of the draft model's shape
        int draft_rows = 0;                // 2 n_slots: the rows of the first draft pass
    };
    // rama_q8_serve_begin / _admit / _steps: the serving chain (q8_serve.hpp), a state of its own next to the chain above
    struct Q8Serve : Q8ChainBase, ServeState {} q8s;
    // rama_q8_spec_begin / _steps: the speculative chain (q8_spec.hpp), a third state next to the two above
    struct Q8Spec : Q8ChainBase {
        bool active = false;               // false: no speculative chain
        bool sampled = false;              // a step runs the batched sampler's ordering launches
        int n_rows = 0, out_cap = 0;       // n_draft + 1 rows per pass; max_new
        SpecTables t{};                    // the device tables (ring / count / done: the device addresses of the two below)
        char* blob = nullptr;              // ... all of them, one allocation
        int* ring = nullptr;               // [max_new] host-pinned and device-mapped: token + 1, 0 = not emitted yet
        int* words = nullptr;              // host-pinned and device-mapped: [0] tokens emitted, [1] 1 = the sequence has finished
        rama_run_state state{};
        // a chain begun with rama_q8_spec_begin_model (q8_spec_model.hpp): the drafts are a second Q8 model's; all of it unused otherwise
        bool model = false;
        rama_config dcfg{}; rama_q8_weights dw{}; rama_run_state dstate{};      // the draft model and its run state: the chain dies with either
        SpecModelTables mt{};              // the device tables (inside blob)
        char* dblob = nullptr;             // the draft passes' batch scratch, a Q8BatchScratch of kSpecRows rows of the draft model's shape
        // a chain begun with rama_q8_spec_begin_tree (q8_tree.hpp): the drafts form a tree; all of it unused otherwise
        bool tree = false;
        TreeTables tt{};                   // the tree record and the ancestor records (inside blob), the tree store (tblob)
        char* tblob = nullptr;
        // a chain begun with rama_q8_spec_begin_model_tree (q8_spec_model_tree.hpp): model and tree both set, and the draft model runs over the
        // tree level by level; all of it unused otherwise
        SpecModelTreeTables xt{};          // the levels' row tables (inside blob), the draft tree store (xblob)
        char* xblob = nullptr;
        int n_levels = 0;                  // n_draft: the draft passes of a step
        int level_rows[kSpecMaxDraft] = {};   // the rows of draft pass d at [d - 1]: the widest that level gets at any cap
    } q8p;
    // rama_q8_tree_forward / _commit (q8_tree.hpp): the tables of an eager tree pass and what its commit checks a path against
    struct Q8Tree {
        char* blob = nullptr; char* store = nullptr; size_t store_cap = 0;
        SeqSlot* rows = nullptr; int* row_tok = nullptr;
        TreeTables tt{};
        float* kc = nullptr;               // the run state of the last pass (NULL: none, or its state is gone)
        int n_rows = 0, pos0 = 0, n_layers = 0, dim = 0, seq_len = 0;
        int parent[kSpecRows] = {};
    } q8t;
    // rama_serve_begin / _admit / _steps: the serving chain of an fp32 model in parity mode (batch_api.hip).  A state of its own: it
    // may be live next to q8s on the same context, and neither touches the other's graph or tables.
    struct Serve : ServeState {
        bool live = false;                 // false once the model or the run state of an occupied slot has been freed: _admit and _steps refuse
        rama_config cfg{}; rama_weights w{};
        CapturedGraph cg;                  // one step, for the chain's whole life
        unsigned long long captures = 0;
        const float* copies[7] = {};       // the chain-order copies the captured step streams (they may be released and made again: the step is then captured again)
        float* scratch = nullptr;          // the pass's rows, one allocation: X | XN | Q | XB | HB [max_rows], ATT [kGcMaxTok], XG | XGN [n_slots], LG [n_slots, vocab]
                                           // (a chain with drafts classifies the rows where they sit: no XG | XGN, LG [max_rows, vocab])
        SeqSlot* tguard = nullptr;         // a chain with drafts: one guard entry per tile of kGcMaxTok rows, pos -1 when no row of the tile carries logits
                                           // (serve_tile_guard.hpp) -- what that tile's classifier launches get as their row table
    } sv;
};

// everything declared from here on is shared inside the library and kept out of its exported symbols
#pragma GCC visibility push(hidden)

// ---------------------------------------------------------------- defined in rama_api.hip

int fail(int code, const char* what, const char* file, int line);      // records the text for rama_last_error, returns code
void destroy_graph(CapturedGraph& g);
int set_device(rama_ctx* c);
int flush_pending(rama_ctx* c);
int check_cfg(const rama_config* cfg);
int handoff_check(rama_ctx* c);
int replay_graph(rama_ctx* c, const CapturedGraph& g);
void drop_graph(rama_ctx* c);      // every captured graph of the context (scratch a graph holds is about to move); exported as rama_internal_drop_graphs

int launch_rmsnorm_ref(rama_ctx* c, float* o, const float* x, const float* w, int n);
int launch_attention_ref(rama_ctx* c, float* xb, float* att, const float* q, const float* kc_layer, const float* vc_layer,
                         const Ctl* ctl, int pos, int dim, int head_size, int seq_len, int n_heads);

// what batch_api.hip needs of the one-token forward: the check of (weights, run state, stage), parity mode's chain-order copy made on first use
// (st == NULL: the whole model), and the final norm + classifier of one token through this translation unit's gemv_rows
int check_stage(const rama_config* cfg, const rama_weights* w, const rama_run_state* s, const rama_stage* st);
int ensure_chain_copy(rama_ctx* c, const rama_config* cfg, const rama_weights* w, const rama_stage* st);
int launch_classifier(rama_ctx* c, float* logits, const float* wcls, const float* x, const float* gain, int dim, int vocab);

// ---------------------------------------------------------------- defined in batch_api.hip: the token batches, the chained batch, the fp32 serving chain

int stage_tokens(rama_ctx* c, int* toks_dev, const int32_t* tokens_host, int n, SeqSlot* seqs_dev = nullptr,
                 const rama_run_state* states = nullptr, const int32_t* pos_host = nullptr);
int copy_out_logits(rama_ctx* c, const rama_run_state* states, const float* lg, int n, int V);
void drop_batch_graphs(rama_ctx* c);                                 // drop_graph: the chained batch's step and the serving chain's
void release_batch(rama_ctx* c);                                     // rama_ctx_destroy: the scratch blobs, the chained batch's and the serving chain's allocations; the stream is idle
void serve_state_gone(rama_ctx* c, const rama_run_state* s);         // rama_state_free: a serving chain whose live slot uses s ends

// ---------------------------------------------------------------- defined in chain_api.hip: parity mode's launches (chain.hpp) and the samplers

int chain_api_init(rama_ctx* c);      // rama_ctx_create: the dynamic-LDS attributes of attention_chain_kernel and gemm_chain_kernel

// epi: CEPI_*; norm: CNORM_*.  A pair no caller uses has no kernel: RAMA_EINVAL
int launch_chain(rama_ctx* c, ChainParams& p, int epi, int norm = CNORM_NONE);
int launch_gemm_chain(rama_ctx* c, GemmChainParams& p, int epi);

bool rmsnorm_chain_ok(size_t n);      // (softmax_chain_kernel's limit too)
int launch_rmsnorm_chain(rama_ctx* c, float* o, const float* x, const float* w, int n, float* copy_to, int batch = 1, int stride = 0, const SeqSlot* tile = nullptr);
int launch_softmax_chain(rama_ctx* c, float* x, int n);

int attn_chain_waves(int head_size, bool long_ctx);
bool attn_chain_ok(int head_size, int seq_len);
size_t attn_chain_lds_bytes(int head_size, int seq_len, int nw);      // dynamic LDS of attention_chain_kernel<nw>
int ensure_attn_scores(rama_ctx* c, int n_heads, int seq_len);
int launch_attention_chain(rama_ctx* c, float* xb, float* att, const float* q, const float* kc_layer, const float* vc_layer,
                           const Ctl* ctl, int pos, int dim, int head_size, int seq_len, int n_heads, bool long_ctx = false, bool spread_wanted = false);
int launch_attention_chain_tokens(rama_ctx* c, const RefAttnParams& a, int n_heads, int nt, int nw, size_t lds);
int launch_attention_tree(rama_ctx* c, const TreeAttnParams& a, int n_heads, int nt, int nw, size_t lds, bool by_node = false);      // q8_tree.hpp's attention_tree_kernel / attention_draft_tree_kernel

int topp_dist_check(rama_ctx* c);     // handoff_check: the distributed pick's error word
int enqueue_sample(rama_ctx* c, ArgmaxParams fin, float temperature, float topp, float u);
int ensure_topp_scratch(rama_ctx* c, int n);
int ensure_topp_batch(rama_ctx* c, int rows, int n);
bool topp_params_ok(float temperature, float topp, float u);
int enqueue_topp_batch(rama_ctx* c, const ToppRow* rows, int n_rows, const float* logits, size_t ld, int n, ToppBatchParams fin);
int enqueue_topp_batch_order(rama_ctx* c, const ToppRow* rows, int n_rows, const float* logits, size_t ld, int n, const SeqSlot* seqs);

// ---------------------------------------------------------------- defined in q8_api.hip: all that rama_api.hip needs of the Q8 stack

void drop_q8_graphs(rama_ctx* c, const rama_run_state* s);      // drop_graph, rama_state_free: the captured Q8 steps, all of them (s == NULL) or those over one run state
void release_q8(rama_ctx* c);                                   // rama_ctx_destroy: the Q8 stack's allocations; the stream is idle

// ---------------------------------------------------------------- defined in q8_serve_api.hip (check_slots_rows .. launch_serve_model_close)

// the serving chains' shared host layer: what rama_q8_serve_* and rama_serve_* do alike is written once in q8_serve_api.hip, which also
// owns q8_serve.hpp's kernels -- batch_api.hip reaches them through the launchers
// The tables of one allocation in order, each rounded up to 256 bytes.  The same code lays a blob out twice: over no base for its size
// (`used`), then over the allocation for the typed pointers.
struct BlobCarver {
    char* base = nullptr;
    size_t used = 0;
    template <class T> void take(T*& table, size_t count) {
        table = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += (count * sizeof(T) + 255) / 256 * 256;
    }
};
int check_slots_rows(const char* entry, int n_slots, int max_rows);
void serve_state_free(rama_ctx::ServeState& sv);            // the allocations, the drafting records included; the stream is idle.  The caller resets its state
// the tables, admission records and rings of a chain of this geometry; `more` carves further tables out of the same blob
int serve_state_alloc(rama_ctx* c, rama_ctx::ServeState& sv, int seq_len, int n_slots, int max_rows, int max_new_cap, void (*more)(BlobCarver&, void*), void* arg);
// the same for a chain that may draft: with `spec` the drafting tables come out of the same blob, and the spec admission records are made
int check_spec_caps(const char* entry, int n_draft_cap, int hint_cap);
int serve_state_alloc_spec(rama_ctx* c, rama_ctx::ServeState& sv, int seq_len, int n_slots, int max_rows, int max_new_cap, bool spec, int n_draft_cap, int hint_cap);
bool serve_slot_live(const rama_ctx::ServeState& sv, int slot);
// an admission's refusals in their order, in the calling entry's words: the head up to the slot index, then -- behind the caller's own check of
// the run state against its model -- the tail; then the install (the record's copy and serve_install_kernel, stream-ordered)
struct ServeNames { const char* admit; const char* admit_at; const char* begin; const char* admit_spec; const char* begin_spec; };      // a chain's entries as its refusals name them
int serve_admit_head(const ServeNames& names, const rama_ctx::ServeState& sv, bool live, int slot, const rama_run_state* state, const int32_t* context_host, const rama_q8_serve_plan* plan);
int serve_admit_tail(const ServeNames& names, const rama_ctx::ServeState& sv, const rama_config& cfg, int slot, const rama_run_state* state, const int32_t* context_host, int n_context,
                     int n_cached, const rama_q8_serve_plan* plan);
int serve_admit_install(rama_ctx* c, rama_ctx::ServeState& sv, int slot, const rama_run_state* state, const int32_t* context_host, int n_context, int n_cached,
                        const rama_q8_serve_plan* plan);
// a cancel, for either chain of any kind: the refusals in the calling entry's words, then serve_cancel_kernel for the slots of the list still live
int serve_cancel(rama_ctx* c, const char* entry, rama_ctx::ServeState& sv, const int32_t* slots, int n);
// the drafting half of an admission, behind the tail: spec != NULL is an _admit_spec entry's record -- refused on a chain begun without drafts --, and
// the install puts the slot's drafting fields and hint in (spec == NULL: n_draft = 0); nothing to do on a chain begun without drafts
int serve_admit_spec_check(const ServeNames& names, const rama_ctx::ServeState& sv, int vocab_size, const rama_q8_serve_spec* spec);
int serve_admit_spec_install(rama_ctx* c, rama_ctx::ServeState& sv, int slot, const rama_q8_serve_spec* spec);
// the run state s is about to be freed: true when a slot whose occupant the host cannot yet see DONE still uses it (a finished occupant's is its owner's again)
bool serve_state_uses(rama_ctx::ServeState& sv, const rama_run_state* s);
int serve_poll_ring(const char* entry, const rama_ctx::ServeState& sv, int slot, int from, int32_t* out_host, int max_tokens, int* n_ready, int* finished, int* generation);
int serve_tokens_back(rama_ctx* c, const char* entry, const rama_ctx::ServeState& sv, int slot, int32_t* out_host, int max_tokens, int* n_out);
int serve_report(rama_ctx* c, const rama_ctx::ServeState& sv, unsigned long long captures, const int* lflag_dev, rama_q8_serve_report* out);
int launch_serve_schedule(rama_ctx* c, const ServeTables& t);
int launch_serve_embed(rama_ctx* c, float* X, const float* emb, const ServeTables& t, int dim);      // rows at position -1 keep what they hold
int launch_serve_gather(rama_ctx* c, float* XG, const float* X, const ServeTables& t, int dim);
int launch_serve_pick(rama_ctx* c, const ServeTables& t, const float* logits, int V, bool sampled);
// ... and q8_serve_spec.hpp's, for the step of a chain with drafts: the drafts, the scheduler, the pick over one logits row per ROW (`sampled`: the
// ordering launches over the rows' sampler records go first), the accept rule
int launch_serve_draft(rama_ctx* c, const ServeTables& t, const ServeSpecTables& st);
int launch_serve_spec_schedule(rama_ctx* c, const ServeTables& t, const ServeSpecTables& st);
int launch_serve_spec_pick(rama_ctx* c, const ServeTables& t, const ServeSpecTables& st, const float* logits, int V, bool sampled);
int launch_serve_spec_accept(rama_ctx* c, const ServeTables& t, const ServeSpecTables& st);
int serve_spec_report(rama_ctx* c, const rama_ctx::ServeState& sv, rama_q8_serve_spec_report* out);
// ... and what a chain with a DRAFT MODEL (rama_q8_serve_begin_model, rama_serve_begin_model; q8_serve_model.hpp) does alike whatever its target: the
// begin's refusals in the entry's words, the draft side's allocations behind serve_state_alloc_spec (the chain's own draft batch scratch and tables; the
// context's Q8 scratches sized for the draft's shape), an _admit_model entry's checks (names.admit_spec: the entry, names.begin_spec: its begin) and
// install, the report, and the two halves of the step around the verify pass -- the draft passes hold the chain's own buffers and the sampler's slices only
int serve_model_begin_check(const char* entry, const rama_config* cfg, const rama_config* dcfg, const rama_q8_weights* dw, int n_slots, int max_rows, int n_draft_cap);
int serve_model_alloc(rama_ctx* c, rama_ctx::ServeState& sv, const rama_config* dcfg, const rama_q8_weights* dw);
bool serve_model_state_clash(const rama_ctx::ServeState& sv, int slot, const rama_run_state* s);
int serve_admit_model_dstate(rama_ctx* c, const rama_ctx::ServeState& sv, const rama_run_state* dstate);
int serve_admit_model_check(const ServeNames& names, const rama_ctx::ServeState& sv, int slot, const rama_run_state* state, const rama_run_state* dstate,
                            int n_context, const rama_q8_serve_plan* plan, int n_draft);
int serve_admit_model_install(rama_ctx* c, rama_ctx::ServeState& sv, int slot, const rama_run_state* dstate, int n_context, int n_draft);
int serve_model_report(rama_ctx* c, const rama_ctx::ServeState& sv, rama_q8_serve_model_report* out);
int launch_serve_model_drafts(rama_ctx* c, const rama_ctx::ServeState& sv);
int launch_serve_model_close(rama_ctx* c, const rama_ctx::ServeState& sv);

// the pending run of recorded 1:1 ops is issued by whatever enters the library next: first statement of every entry point
// that enqueues, synchronises or changes a setting
#define RAMA_PENDING(c) ((c)->rec.any())
#define RAMA_ENTER(c) do { if ((c) && RAMA_PENDING(c)) { const int rf_ = flush_pending(c); if (rf_) return rf_; } } while (0)

// g = the launches `enqueue` puts on the stream, captured and instantiated (whatever g held goes first).  The capture always ends -- a stream
// must never be left capturing --, and an error of `enqueue` comes before the capture's own status.  rama_ctx::handoff_dirty is saved and
// cleared around the capture: what the enqueue sets is a property of the GRAPH (g.handoff), which replay_graph re-arms at every launch.
template <class Enqueue>
int capture_graph(rama_ctx* c, CapturedGraph& g, Enqueue&& enqueue) {
    destroy_graph(g);
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    const bool dirty_before = c->handoff_dirty;
    c->handoff_dirty = false;
    const int rc = enqueue();
    hipError_t err = hipStreamEndCapture(c->stream, &g.graph);
    g.handoff = c->handoff_dirty;
    c->handoff_dirty = dirty_before;
    if (rc) { destroy_graph(g); return rc; }
    if (err == hipSuccess) err = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
    if (err != hipSuccess) { destroy_graph(g); return fail((int)err, "graph capture", __FILE__, __LINE__); }
    return 0;
}

// ---------------------------------------------------------------- launch helpers

inline int ew_grid(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 2048); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool ranges_overlap(const float* p0, size_t n0, const float* p1, size_t n1) { return p0 < p1 + n1 && p1 < p0 + n0; }

// Per-kernel timing: while a kernel class is being profiled, its next launch carries a start and
// a stop event ON THE DISPATCH ITSELF (hipExtLaunchKernelGGL), so the interval is the kernel's own
// begin..end as rocprofv3 sees it -- separate event records around the launch add ~3 us.
struct KTimer {
    rama_ctx* c; bool on;
    KTimer(rama_ctx* c_, int kid) : c(c_), on(false) {
        KProf& k = c->kp;
        if (k.kernel_id == kid && k.used < k.max_records) {
            on = true;
            c->cur_start = k.ev[2 * k.used]; c->cur_stop = k.ev[2 * k.used + 1];
        }
    }
    ~KTimer() {
        if (on) { c->kp.used++; c->cur_start = c->cur_stop = nullptr; }
    }
};
// launch on the context's stream; the first launch inside an armed KTimer scope takes the events
#define RAMA_LAUNCH(c, kernel, grid, block, shm, ...)                                                          \
    do {                                                                                                        \
        if ((c)->cur_start) {                                                                                   \
            hipExtLaunchKernelGGL(kernel, grid, block, shm, (c)->stream, (c)->cur_start, (c)->cur_stop, 0, __VA_ARGS__); \
            (c)->cur_start = nullptr;                                                                           \
        } else {                                                                                                \
            hipLaunchKernelGGL(kernel, grid, block, shm, (c)->stream, __VA_ARGS__);                             \
        }                                                                                                       \
    } while (0)

// Up to max_tokens tokens from entry `from` of a host-mapped ring row of `cap` entries (an entry is token + 1, 0 = not produced yet; the
// device stores them in order): acquire loads, stops at the first entry not there yet.  Returns the count.  Touches no stream.
inline int read_ring(const int* row, int cap, int from, int32_t* out_host, int max_tokens) {
    int n = 0;
    while (n < max_tokens && from + n < cap) {
        const int v = __atomic_load_n(row + from + n, __ATOMIC_ACQUIRE);
        if (v == 0) break;
        out_host[n++] = v - 1;
    }
    return n;
}

#pragma GCC visibility pop
