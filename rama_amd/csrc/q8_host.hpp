// q8_host.hpp -- what the three Q8 translation units (q8_api.hip, q8_serve_api.hip, q8_spec_api.hip) share ON THE HOST, on the model of ctx.hpp's
// cross-unit declarations: the types the shared procedures take, hidden-visibility declarations of what one unit defines for the others, the refusal
// macros, and the two procedures that are templates.  No kernel: q8_api.hip alone includes q8.hpp and q8_batch.hpp, and the other two reach the
// token-batch pass through enqueue_q8_row_layers / enqueue_q8_batch_pass / enqueue_q8_pick_rows (DESIGN.md "Translation units").  Internal: not installed.
#pragma once
#include "ctx.hpp"

#include <cstdio>

constexpr int kQ8bMaxTok = 128;    // token rows per launch of the token-batch pass (8 tiles of 16)

// the batch path's scratch, row-major per token (T = kQ8bMaxTok): X residual rows, XN their norms, Q / Kr / V, XB attention
// output, HB, ATT score rows [T][n_heads][seq_len], LG logits [T][vocab]; the int8 activations [T][max(dim, hidden)] and their
// scales; token ids; the sequence table
struct Q8BatchScratch { float *X, *XN, *Q, *Kr, *V, *XB, *HB, *ATT, *LG; int8_t* xq; float* xs; int* toks; SeqSlot* seqs; int nw; size_t att_lds; };

#pragma GCC visibility push(hidden)

// ---------------------------------------------------------------- defined in q8_api.hip: the checks, the scratches, the pass, the drain

bool q8_weights_complete(const rama_q8_weights* w);
int q8_check(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* s);

// ---- The refusals several entries share, each in the calling entry's words: "<entry>: <what>" is the text that entry has always given.  An
// entry calls them where its own REQUIREs of the same matter stood, so which error a bad call gets does not change.
int refuse(const char* entry, const char* what, const char* file, int line, int code = RAMA_EINVAL);
#define REFUSE_UNLESS(cond, entry, what) do { if (!(cond)) return refuse((entry), (what), __FILE__, __LINE__); } while (0)
#define UNSUPPORTED_UNLESS(cond, entry, what) do { if (!(cond)) return refuse((entry), (what), __FILE__, __LINE__, RAMA_EUNSUP); } while (0)
#define CHECKED(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// every token of a list is in the vocabulary
int check_tokens(const char* entry, const char* what, const int32_t* toks, int n, int V);
// a sampling plan's two halves (rama_q8_decode_batch_begin has refusals of its own between them): Device::sample's (temperature, topp, u) ...
int check_sampler(const char* entry, float temperature, float topp, float u);
// ... and the stop token (-1: none) against the vocabulary
int check_stop_token(const char* entry, int stop_token, int V);
// the drafting fields of a plan (rama_q8_serve_spec, rama_q8_spec_plan): n_draft and the hint's length against the caller's caps -- those two
// refusals name the cap in the caller's words --, ngram, the hint's tokens against the vocabulary
template <class Plan>
static int check_drafting(const char* entry, const Plan& p, int n_draft_cap, const char* n_draft_what, int n_hint_cap, const char* hint_what, int V) {
    REFUSE_UNLESS(p.n_draft >= 0 && p.n_draft <= n_draft_cap, entry, n_draft_what);
    REFUSE_UNLESS(p.ngram >= 1 && p.ngram <= kSpecMaxNgram, entry, "ngram outside 1..4");
    REFUSE_UNLESS(p.n_hint >= 0 && (p.n_hint == 0 || p.hint) && p.n_hint <= n_hint_cap, entry, hint_what);
    return check_tokens(entry, "hint token outside the vocabulary", p.hint, p.n_hint, V);
}

int ensure_q8_scratch(rama_ctx* c, const rama_config* cfg);      // the int8 activations of one token, sized outside any capture
bool q8_batch_ok(const rama_config* cfg);                        // the shapes the batch path takes
// a scratch of T rows over `base` (NULL: its size only), and the attention's geometry; the context's own for kQ8bMaxTok rows
size_t q8_batch_scratch_lay(const rama_config* cfg, int gs, size_t T, char* base, Q8BatchScratch* b);
int ensure_q8_batch_scratch(rama_ctx* c, const rama_config* cfg, int gs, Q8BatchScratch* b);
// what a chain's step runs on: both scratches and -- sampler_rows > 0 -- the batched sampler's slices for so many rows
int q8_chain_scratch(rama_ctx* c, const rama_config* cfg, int group_size, int sampler_rows, Q8BatchScratch* b);

// a pass over a device row table: the embedding rows and every layer; the same with the classifier tail over every row; the classifier over
// n_rows rows of src_rows into b.LG; what a sampled step does behind the classifier
// (tree_by_node: `tree` is a level of a draft model's tree, q8_spec_model_tree.hpp -- its store holds row node - 1 of every node fed so far)
int enqueue_q8_row_layers(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const Q8BatchScratch& b, const int* row_tok,
                          const SeqSlot* rows, int n_rows, const TreeTables* tree = nullptr, bool tree_by_node = false);
int enqueue_q8_batch_pass(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const Q8BatchScratch& b, const int* row_tok,
                          const SeqSlot* rows, int n_rows, const TreeTables* tree = nullptr, bool tree_by_node = false);
int enqueue_q8_classifier(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const Q8BatchScratch& b, const float* src_rows, int n_rows);
int enqueue_q8_pick_rows(rama_ctx* c, const Q8BatchScratch& b, int V, bool sampled, const ToppRow* trow, int n_rows, PickRows* r);

// what the _tokens and _stats entries of the chains open with, and what a _tokens entry ends with
int q8_drain(rama_ctx* c);
int q8_tokens_back(int32_t* out_host, const int* row_dev, int produced, int cap, int max_tokens, int* n);

// ---------------------------------------------------------------- defined in q8_serve_api.hip / q8_spec_api.hip, for release_q8

void serve_release(rama_ctx* c);      // the serving chain's graph and allocations, its state reset; the stream is idle
void spec_release(rama_ctx* c);       // ... and the speculative chain's

// What every _steps entry does behind its own checks: the scratch, then n_steps times `step(b)` -- eager, or (graph mode, no kernel class being
// timed) captured into the chain's graph on first use and replayed.  *n_done: the steps enqueued, also when one fails.
template <class Step>
static int q8_chain_steps(rama_ctx* c, rama_ctx::Q8ChainBase& ch, int sampler_rows, int n_steps, Step&& step, int* n_done) {
    *n_done = 0;
    Q8BatchScratch b{};
    int rc = q8_chain_scratch(c, &ch.cfg, ch.w.group_size, sampler_rows, &b); if (rc) return rc;
    c->embedded_x = nullptr; c->host_pos = -1;
    auto enqueue = [&] { return step(b); };
    const bool graphs = c->graph_mode && c->kp.kernel_id < 0;
    for (; *n_done < n_steps; ++*n_done) {
        if (!graphs) {
            rc = enqueue(); if (rc) return rc;
            continue;
        }
        if (!ch.cg.exec) {
            rc = capture_graph(c, ch.cg, enqueue); if (rc) return rc;
            ch.captures++;
        }
        rc = replay_graph(c, ch.cg); if (rc) return rc;
    }
    return 0;
}

#pragma GCC visibility pop
