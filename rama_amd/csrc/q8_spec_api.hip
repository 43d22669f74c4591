// q8_spec_api.hip -- THE SPECULATIVE CHAIN of a Q8 model (rama_q8_spec_*) and the tree drafts (rama_q8_spec_begin_tree,
// rama_q8_tree_forward / _commit, 8.13), with the host-only statements of their rules.  The kernels are q8_spec.hpp, q8_spec_model.hpp and the
// drafting / accept / commit kernels of q8_tree.hpp, which this translation unit alone includes; the token-batch pass (its tree launches included)
// and the checks every Q8 chain shares are q8_api.hip's, reached through q8_host.hpp (DESIGN.md "Translation units").
//
// One sequence, up to 15 drafted tokens per step by n-gram lookup in its own text
// and a caller's hint, drafts and the token before them verified in ONE weight pass of n_draft + 1 rows.  A token-batch pass over rows at
// consecutive positions of one sequence gives every row the bits of its own rama_q8_forward, so whatever is accepted is what
// rama_q8_generate produces: a wrong draft costs time only.  A third chain next to the chained batch and the serving chain, with a state of its own.
#include "q8_host.hpp"
#include "q8_spec.hpp"
#include "q8_spec_model.hpp"
#include "q8_tree.hpp"
#include "q8_spec_model_tree.hpp"

#if defined(RAMA_CHAIN_HPP) || defined(RAMA_Q8_HPP) || defined(RAMA_Q8_SERVE_HPP)
#error "q8_spec_api.hip must not include chain.hpp, q8.hpp / q8_batch.hpp or q8_serve.hpp: their kernels belong to other code objects"
#endif

#include <algorithm>
#include <cstring>
#include <vector>

// the speculative chain's allocations (rama_q8_spec_begin / _end, release_q8); the stream is idle
void spec_release(rama_ctx* c) {
    auto& sp = c->q8p;
    destroy_graph(sp.cg);
    hipFree(sp.blob); hipFree(sp.dblob); hipFree(sp.tblob); hipFree(sp.xblob);
    if (sp.ring) hipHostFree(sp.ring);
    if (sp.words) hipHostFree(sp.words);
    sp = rama_ctx::Q8Spec();
}

// the drafting rule on the host (spec_draft_kernel finds the same occurrence by a max reduction over candidate ends)
int rama_q8_spec_draft(const int32_t* hint, int n_hint, const int32_t* seq, int L, int n_draft, int ngram, int room, int32_t* drafts_out) {
    REQUIRE(seq && L >= 1 && n_hint >= 0 && (n_hint == 0 || hint), RAMA_EINVAL, "q8_spec_draft: bad text");
    REQUIRE(n_draft >= 0 && n_draft <= kSpecMaxDraft && ngram >= 1 && ngram <= kSpecMaxNgram, RAMA_EINVAL, "q8_spec_draft: n_draft in 0..15, ngram in 1..4");
    REQUIRE(n_draft == 0 || drafts_out, RAMA_EINVAL, "q8_spec_draft: NULL argument");
    const int cap = std::min(n_draft, room);
    if (cap <= 0) return 0;
    for (int n = std::min(ngram, L); n >= 1; n--) {
        const int32_t* tail = seq + (L - n);
        // the latest occurrence: its exclusive end e, in the hint first; in the sequence it ends before L
        const int32_t* text = hint; int len = n_hint, e = -1;
        for (int k = n_hint; k >= n && e < 0; k--) if (!memcmp(hint + (k - n), tail, sizeof(int32_t) * n)) e = k;
        if (e < 0) {
            text = seq; len = L;
            for (int k = L - 1; k >= n && e < 0; k--) if (!memcmp(seq + (k - n), tail, sizeof(int32_t) * n)) e = k;
        }
        if (e < 0) continue;
        const int n_d = std::min(cap, len - e);
        for (int j = 0; j < n_d; j++) drafts_out[j] = text[e + j];
        return n_d;
    }
    return 0;
}

int rama_q8_spec_accept(const int32_t* drafts, int n_d, const int32_t* picks, int stop_token, int remaining, int* finished) {
    REQUIRE(picks && n_d >= 0 && n_d <= kSpecMaxDraft && (n_d == 0 || drafts) && remaining >= 1, RAMA_EINVAL,
            "q8_spec_accept: n_d in 0..15 drafts, n_d + 1 picks, remaining >= 1");
    int a = 0, fin = 0;
    const int emit = spec_accept_rule(drafts, n_d, picks, stop_token, remaining, &a, &fin);
    if (finished) *finished = fin;
    return emit;
}

int rama_q8_spec_end(rama_ctx* c) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "q8_spec_end: ctx is NULL");
    if (!c->q8p.active && !c->q8p.blob) return 0;
    if (set_device(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    spec_release(c);
    return 0;
}

// the draft model of rama_q8_spec_begin_model and its run state (NULL: rama_q8_spec_begin, the n-gram lookup)
struct SpecDrafter { const rama_config* cfg; const rama_q8_weights* w; const rama_run_state* state; };

// rama_q8_spec_begin (dm NULL) and rama_q8_spec_begin_model: one chain, begun the same way; the latter also sizes the draft passes' scratch and tables
// n_rows > 0: rama_q8_spec_begin_tree -- the lookup's drafts form a tree of n_branch continuations in a pass of n_rows rows (q8_tree.hpp)
static int spec_begin(rama_ctx* c, const char* entry, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* state,
                      const SpecDrafter* dm, const int32_t* context_host, int n_context, const rama_q8_spec_plan* plan, int n_branch = 0,
                      int n_rows = 0, bool tree = false) {
    // everything is checked before anything of a running chain is touched
    REFUSE_UNLESS(c && state && context_host && plan && (!dm || dm->state), entry, "NULL argument");
    int rc = q8_check(c, cfg, w, state); if (rc) return rc;
    if (dm) { rc = q8_check(c, dm->cfg, dm->w, dm->state); if (rc) return rc; }
    const int V = cfg->vocab_size;
    CHECKED(check_sampler(entry, plan->temperature, plan->topp, plan->u));
    CHECKED(check_stop_token(entry, plan->stop_token, V));
    if (!dm) CHECKED(check_drafting(entry, *plan, kSpecMaxDraft, "n_draft outside 0..15", kSpecHintBit - 1, "bad hint", V));
    else {      // (ngram is ignored)
        REFUSE_UNLESS(plan->n_draft >= 1 && plan->n_draft <= kSpecMaxDraft, entry, "n_draft outside 1..15");
        REFUSE_UNLESS(!plan->hint && plan->n_hint == 0, entry, "a hint: model drafts replace the n-gram lookup");
        REFUSE_UNLESS(dm->cfg->vocab_size == V, entry, "the draft model's vocabulary is not the target's");
        REFUSE_UNLESS(dm->state->key_cache != state->key_cache && dm->state->value_cache != state->value_cache, entry,
                      "the draft run state is the target's");
    }
    if (tree) {
        REFUSE_UNLESS(plan->n_draft >= 1, entry, "n_draft outside 1..15");
        REFUSE_UNLESS(n_branch >= 1 && n_branch <= kTreeMaxBranch, entry, "n_branch outside 1..4");
        REFUSE_UNLESS(n_rows >= 2 && n_rows <= kSpecRows, entry, "n_rows outside 2..16");
        if (dm) REFUSE_UNLESS(n_branch <= V, entry, "n_branch beyond vocab_size");
    }
    REFUSE_UNLESS(n_context >= 1, entry, "n_context < 1");
    REFUSE_UNLESS(plan->max_new >= 1, entry, "max_new < 1");
    REFUSE_UNLESS(plan->max_new <= cfg->seq_len && n_context <= cfg->seq_len - plan->max_new, entry, "n_context + max_new beyond seq_len");
    if (dm) REFUSE_UNLESS(plan->max_new <= dm->cfg->seq_len && n_context <= dm->cfg->seq_len - plan->max_new, entry,
                          "n_context + max_new beyond the draft model's seq_len");
    CHECKED(check_tokens(entry, "token outside the vocabulary", context_host, n_context, V));
    UNSUPPORTED_UNLESS(q8_batch_ok(cfg), entry, "a shape the Q8 token-batch pass does not take");
    if (dm) UNSUPPORTED_UNLESS(q8_batch_ok(dm->cfg), entry, "a draft model of a shape the Q8 token-batch pass does not take");
    const bool sampled = plan->temperature != 0.0f;
    UNSUPPORTED_UNLESS(!sampled || (V > 1 && V <= kToppBlock * kToppMaxBlocks), entry, "a sampled plan needs vocab_size <= 32768");
    if (set_device(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    spec_release(c);
    // the scratch and the chain's tables: sized here, outside any capture
    const int R = tree ? n_rows : plan->n_draft + 1;       // (a chain with a draft model has n_draft >= 1: its two-row draft pass fits the sampler's R slices)
    Q8BatchScratch b{};
    // (a draft model's tree: a draft level has up to 15 rows -- two at least --, whatever R is)
    rc = q8_chain_scratch(c, cfg, w->group_size, sampled ? (dm && tree ? kSpecRows : R) : 0, &b); if (rc) return rc;
    auto& sp = c->q8p;
    SpecModelTreeTables& xt = sp.xt;
    SpecTables& t = sp.t;
    SpecModelTables& mt = sp.mt;
    TreeTables& tt = sp.tt;
    const size_t S = (size_t)cfg->seq_len, H = (size_t)plan->n_hint, cap = (size_t)plan->max_new;
    auto lay = [&](char* base) {
        BlobCarver bc{base};
        bc.take(t.st, 1); bc.take(t.text, H + S); bc.take(t.rows, kSpecRows); bc.take(t.row_tok, kSpecRows); bc.take(t.trow, kSpecRows);
        bc.take(t.out, cap);
        if (dm) { bc.take(mt.ms, 1); bc.take(mt.rows, kSpecModelRows); bc.take(mt.row_tok, kSpecModelRows); bc.take(mt.trow, kSpecModelRows); }
        if (tree) { bc.take(tt.ts, 1); bc.take(tt.anc, kSpecRows); }
        if (dm && tree) {
            constexpr size_t n = (size_t)kSpecMaxDraft * kSpecRows;
            bc.take(xt.xs, 1); bc.take(xt.dts, 1); bc.take(xt.rows, n); bc.take(xt.row_tok, n); bc.take(xt.trow, n); bc.take(xt.anc, n);
        }
        return bc.used;
    };
    const size_t need = lay(nullptr);
    HIPCHK(hipMalloc(&sp.blob, need));
    HIPCHK(hipMemset(sp.blob, 0, need));
    lay(sp.blob);
    if (dm) {      // the draft passes' rows: a scratch of its own, in the draft model's shape -- one 16-token tile of the products
        Q8BatchScratch db{};
        const size_t dneed = q8_batch_scratch_lay(dm->cfg, dm->w->group_size, kSpecRows, nullptr, &db);
        HIPCHK(hipMalloc(&sp.dblob, dneed));
        HIPCHK(hipMemset(sp.dblob, 0, dneed));
        SpecModelState mh{};
        mh.kc = dm->state->key_cache; mh.vc = dm->state->value_cache;
        mh.Dc = n_context - 1; mh.pick_row = -1;
        HIPCHK(hipMemcpy(mt.ms, &mh, sizeof mh, hipMemcpyHostToDevice));
    }
    if (tree) {      // the tree store: every layer's k and v rows of the pass but the root's, for the commit
        const size_t n = (size_t)cfg->n_layers * (size_t)(R - 1) * (size_t)cfg->dim;
        HIPCHK(hipMalloc(&sp.tblob, 2 * n * sizeof(float)));
        HIPCHK(hipMemset(sp.tblob, 0, 2 * n * sizeof(float)));
        tt.ks = reinterpret_cast<float*>(sp.tblob); tt.vs = tt.ks + n; tt.store_rows = R - 1;
        TreeState th{};
        th.n_branch = n_branch; th.n_rows = R;
        HIPCHK(hipMemcpy(tt.ts, &th, sizeof th, hipMemcpyHostToDevice));
    }
    if (dm && tree) {      // the draft tree store, and every level's row count: the widest that depth gets at any cap
        const size_t n = (size_t)dm->cfg->n_layers * (size_t)(R - 1) * (size_t)dm->cfg->dim;
        HIPCHK(hipMalloc(&sp.xblob, 2 * n * sizeof(float)));
        HIPCHK(hipMemset(sp.xblob, 0, 2 * n * sizeof(float)));
        xt.ks = reinterpret_cast<float*>(sp.xblob); xt.vs = xt.ks + n; xt.store_rows = R - 1;
        for (int d = 0; d < kSpecMaxDraft; d++) sp.level_rows[d] = d == 0 ? kSpecModelRows : 1;
        for (int k = 1; k <= plan->n_draft; k++) {
            int par[kSpecRows], dep[kSpecRows], rank[kSpecRows], width[kSpecRows] = {0};
            const int m = spec_model_tree_shape(k, n_branch, R, par, dep, rank);
            for (int j = 1; j <= m; j++) if (dep[j] < k) sp.level_rows[dep[j]] = std::max(sp.level_rows[dep[j]], ++width[dep[j]]);
        }
    }
    HIPCHK(hipHostMalloc(&sp.ring, sizeof(int) * cap, hipHostMallocMapped));
    HIPCHK(hipHostMalloc(&sp.words, sizeof(int) * 2, hipHostMallocMapped));
    memset(sp.ring, 0, sizeof(int) * cap);
    memset(sp.words, 0, sizeof(int) * 2);
    int* words_dev = nullptr;
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&t.ring), sp.ring, 0));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&words_dev), sp.words, 0));
    t.count = words_dev; t.done = words_dev + 1;
    SpecState h{};
    h.kc = state->key_cache; h.vc = state->value_cache;
    h.L = n_context; h.max_new = plan->max_new; h.stop = plan->stop_token;
    h.n_draft = plan->n_draft; h.ngram = plan->ngram; h.n_hint = plan->n_hint; h.seq_len = cfg->seq_len;
    h.temperature = plan->temperature; h.topp = plan->topp; h.u = plan->u;
    HIPCHK(hipMemcpy(t.st, &h, sizeof h, hipMemcpyHostToDevice));
    if (plan->n_hint) HIPCHK(hipMemcpy(t.text, plan->hint, sizeof(int) * H, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.text + H, context_host, sizeof(int) * (size_t)n_context, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(c->stream));
    sp.cfg = *cfg; sp.w = *w; sp.state = *state; sp.sampled = sampled;
    sp.n_rows = R; sp.out_cap = plan->max_new; sp.captures = 0; sp.active = true; sp.live = true;
    if (dm) { sp.model = true; sp.dcfg = *dm->cfg; sp.dw = *dm->w; sp.dstate = *dm->state; }
    sp.tree = tree;
    sp.n_levels = dm && tree ? plan->n_draft : 0;
    return 0;
}

int rama_q8_spec_begin(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* state, const int32_t* context_host,
                       int n_context, const rama_q8_spec_plan* plan) {
    RAMA_ENTER(c);
    return spec_begin(c, "q8_spec_begin", cfg, w, state, nullptr, context_host, n_context, plan);
}

int rama_q8_spec_begin_model(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* state, const rama_config* dcfg,
                             const rama_q8_weights* dw, const rama_run_state* dstate, const int32_t* context_host, int n_context,
                             const rama_q8_spec_plan* plan) {
    RAMA_ENTER(c);
    const SpecDrafter dm{dcfg, dw, dstate};
    return spec_begin(c, "q8_spec_begin_model", cfg, w, state, &dm, context_host, n_context, plan);
}

int rama_q8_spec_begin_tree(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* state, const int32_t* context_host,
                            int n_context, const rama_q8_spec_plan* plan, int n_branch, int n_rows) {
    RAMA_ENTER(c);
    return spec_begin(c, "q8_spec_begin_tree", cfg, w, state, nullptr, context_host, n_context, plan, n_branch, n_rows, true);
}

int rama_q8_spec_begin_model_tree(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* state, const rama_config* dcfg,
                                  const rama_q8_weights* dw, const rama_run_state* dstate, const int32_t* context_host, int n_context,
                                  const rama_q8_spec_plan* plan, int n_branch, int n_rows) {
    RAMA_ENTER(c);
    const SpecDrafter dm{dcfg, dw, dstate};
    return spec_begin(c, "q8_spec_begin_model_tree", cfg, w, state, &dm, context_host, n_context, plan, n_branch, n_rows, true);
}

// the commit of a tree pass: the path recorded in tt.ts, from the tree store into the caches at kc / vc (q8_tree.hpp tree_commit_kernel)
static int launch_tree_commit(rama_ctx* c, const TreeTables& tt, float* kc, float* vc, int n_layers, int dim, int seq_len) {
    TreeCommitParams p{tt.ts, kc, vc, tt.ks, tt.vs, dim, seq_len, tt.store_rows};
    hipLaunchKernelGGL(tree_commit_kernel, dim3(n_layers, kSpecMaxDraft), dim3(256), 0, c->stream, p);
    LAUNCHCHK();
    return 0;
}

// one step of a chain begun with rama_q8_spec_begin_tree: the tree and its row table, the pass over it, every row's pick, the accept rule
// over the tree, the accepted path's rows into the cache
static int enqueue_q8_spec_model_tree_drafts(rama_ctx* c);
static int enqueue_q8_spec_tree_step(rama_ctx* c, const Q8BatchScratch& b) {
    auto& sp = c->q8p;
    const int R = sp.n_rows;
    int rc = 0;
    if (sp.model) { rc = enqueue_q8_spec_model_tree_drafts(c); if (rc) return rc; }      // (rama_q8_spec_begin_model_tree: the tree is the draft model's)
    else {
        hipLaunchKernelGGL(spec_tree_draft_kernel, dim3(1), dim3(1024), 0, c->stream, sp.t, sp.tt);
        LAUNCHCHK();
    }
    rc = enqueue_q8_batch_pass(c, &sp.cfg, &sp.w, b, sp.t.row_tok, sp.t.rows, R, &sp.tt); if (rc) return rc;
    SpecPickParams fin{};
    fin.t = sp.t;
    rc = enqueue_q8_pick_rows(c, b, sp.cfg.vocab_size, sp.sampled, sp.t.trow, R, &fin.r); if (rc) return rc;
    hipLaunchKernelGGL(spec_pick_kernel, dim3(R), dim3(1024), 0, c->stream, fin);
    LAUNCHCHK();
    hipLaunchKernelGGL(spec_tree_accept_kernel, dim3(1), dim3(64), 0, c->stream, sp.t, sp.tt);
    LAUNCHCHK();
    rc = launch_tree_commit(c, sp.tt, sp.state.key_cache, sp.state.value_cache, sp.cfg.n_layers, sp.cfg.dim, sp.cfg.seq_len); if (rc) return rc;
    if (!sp.model) return 0;
    // the draft cursor and the draft commit's record from what the accept rule took; then the same commit over the draft's caches and store
    hipLaunchKernelGGL(spec_model_tree_close_kernel, dim3(1), dim3(64), 0, c->stream, sp.t, sp.mt, sp.tt, sp.xt);
    LAUNCHCHK();
    const TreeTables dt{sp.xt.dts, nullptr, sp.xt.ks, sp.xt.vs, sp.xt.store_rows};
    return launch_tree_commit(c, dt, sp.dstate.key_cache, sp.dstate.value_cache, sp.dcfg.n_layers, sp.dcfg.dim, sp.dcfg.seq_len);
}

// the drafts of a chain begun with rama_q8_spec_begin_model_tree (q8_spec_model_tree.hpp): the step's opening launch, then n_draft passes of the draft
// model over its own scratch, one per level of the tree, each ended by the pick that gives the level's children their tokens
static int enqueue_q8_spec_model_tree_drafts(rama_ctx* c) {
    auto& sp = c->q8p;
    Q8BatchScratch db{};
    q8_batch_scratch_lay(&sp.dcfg, sp.dw.group_size, kSpecRows, sp.dblob, &db);
    hipLaunchKernelGGL(spec_model_tree_open_kernel, dim3(1), dim3(256), 0, c->stream, sp.t, sp.mt, sp.tt, sp.xt);
    LAUNCHCHK();
    for (int d = 1; d <= sp.n_levels; d++) {
        const int n = sp.level_rows[d - 1], at = (d - 1) * kSpecRows;
        const TreeTables lt{nullptr, sp.xt.anc + at, sp.xt.ks, sp.xt.vs, sp.xt.store_rows};
        int rc = enqueue_q8_batch_pass(c, &sp.dcfg, &sp.dw, db, sp.xt.row_tok + at, sp.xt.rows + at, n, &lt, true); if (rc) return rc;
        SpecModelTreePickParams pk{};
        pk.t = sp.t; pk.tt = sp.tt; pk.x = sp.xt; pk.d = d;
        rc = enqueue_q8_pick_rows(c, db, sp.dcfg.vocab_size, sp.sampled, sp.xt.trow + at, n, &pk.r); if (rc) return rc;
        hipLaunchKernelGGL(spec_model_tree_pick_kernel, dim3(n), dim3(1024), 0, c->stream, pk);
        LAUNCHCHK();
    }
    return 0;
}

// the drafts of a chain begun with rama_q8_spec_begin_model (q8_spec_model.hpp): the step's opening launch, then n_draft passes of the draft model
// over its own scratch -- two rows, then one -- each ended by the pick that stores d[j] and sets the next pass's row
static int enqueue_q8_spec_model_drafts(rama_ctx* c) {
    auto& sp = c->q8p;
    Q8BatchScratch db{};
    q8_batch_scratch_lay(&sp.dcfg, sp.dw.group_size, kSpecRows, sp.dblob, &db);
    hipLaunchKernelGGL(spec_model_open_kernel, dim3(1), dim3(64), 0, c->stream, sp.t, sp.mt);
    LAUNCHCHK();
    for (int j = 0; j < sp.n_rows - 1; j++) {
        const int n = j == 0 ? kSpecModelRows : 1;
        int rc = enqueue_q8_batch_pass(c, &sp.dcfg, &sp.dw, db, sp.mt.row_tok, sp.mt.rows, n); if (rc) return rc;
        SpecModelPickParams pk{};
        pk.t = sp.t; pk.m = sp.mt; pk.j = j;
        rc = enqueue_q8_pick_rows(c, db, sp.dcfg.vocab_size, sp.sampled, sp.mt.trow, n, &pk.r); if (rc) return rc;
        hipLaunchKernelGGL(spec_model_pick_kernel, dim3(1), dim3(1024), 0, c->stream, pk);
        LAUNCHCHK();
    }
    return 0;
}

// one step: the drafts and the row table, the pass over it, every row's logits, every row's pick, the accept rule
static int enqueue_q8_spec_step(rama_ctx* c, const Q8BatchScratch& b) {
    auto& sp = c->q8p;
    if (sp.tree) return enqueue_q8_spec_tree_step(c, b);
    const int R = sp.n_rows;
    int rc = 0;
    if (sp.model) { rc = enqueue_q8_spec_model_drafts(c); if (rc) return rc; }
    else {
        hipLaunchKernelGGL(spec_draft_kernel, dim3(1), dim3(1024), 0, c->stream, sp.t);
        LAUNCHCHK();
    }
    rc = enqueue_q8_batch_pass(c, &sp.cfg, &sp.w, b, sp.t.row_tok, sp.t.rows, R); if (rc) return rc;
    SpecPickParams fin{};
    fin.t = sp.t;
    rc = enqueue_q8_pick_rows(c, b, sp.cfg.vocab_size, sp.sampled, sp.t.trow, R, &fin.r); if (rc) return rc;
    hipLaunchKernelGGL(spec_pick_kernel, dim3(R), dim3(1024), 0, c->stream, fin);
    LAUNCHCHK();
    hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(64), 0, c->stream, sp.t);
    LAUNCHCHK();
    if (sp.model) {      // the draft cursor, from what the accept rule took
        hipLaunchKernelGGL(spec_model_close_kernel, dim3(1), dim3(64), 0, c->stream, sp.t, sp.mt);
        LAUNCHCHK();
    }
    return 0;
}

int rama_q8_spec_steps(rama_ctx* c, int n_steps) {
    RAMA_ENTER(c);
    REQUIRE(c && c->q8p.active, RAMA_EINVAL, "q8_spec_steps: call rama_q8_spec_begin first");
    auto& sp = c->q8p;
    REQUIRE(sp.live, RAMA_EINVAL, "q8_spec_steps: the chain's model or its run state has been freed");      // (the target's or the draft's)
    REQUIRE(n_steps >= 0, RAMA_EINVAL, "q8_spec_steps: n_steps < 0");
    if (set_device(c)) return 1;
    int n_done = 0;
    const int sampler_rows = sp.model && sp.tree ? kSpecRows : sp.n_rows;
    return q8_chain_steps(c, sp, sp.sampled ? sampler_rows : 0, n_steps, [&](const Q8BatchScratch& b) { return enqueue_q8_spec_step(c, b); }, &n_done);
}

int rama_q8_spec_poll(rama_ctx* c, int from, int32_t* out_host, int max_tokens, int* n_ready, int* finished) {
    RAMA_ENTER(c);
    REQUIRE(c && n_ready && c->q8p.active && from >= 0 && max_tokens >= 0 && (max_tokens == 0 || out_host), RAMA_EINVAL, "q8_spec_poll: bad argument");
    const auto& sp = c->q8p;
    // the finished word first, then the count: each is stored after what it vouches for
    const int fin = __atomic_load_n(sp.words + 1, __ATOMIC_ACQUIRE);
    const int cnt = std::min(__atomic_load_n(sp.words, __ATOMIC_ACQUIRE), sp.out_cap);
    *n_ready = read_ring(sp.ring, cnt, from, out_host, max_tokens);
    if (finished) *finished = fin != 0;
    return 0;
}

int rama_q8_spec_tokens(rama_ctx* c, int32_t* out_host, int max_tokens, int* n) {
    RAMA_ENTER(c);
    REQUIRE(c && n && c->q8p.active && max_tokens >= 0 && (max_tokens == 0 || out_host), RAMA_EINVAL, "q8_spec_tokens: bad argument");
    auto& sp = c->q8p;
    { const int rh = q8_drain(c); if (rh) return rh; }
    SpecState s{};
    HIPCHK(hipMemcpy(&s, sp.t.st, sizeof s, hipMemcpyDeviceToHost));
    return q8_tokens_back(out_host, sp.t.out, s.n_out, sp.out_cap, max_tokens, n);
}

int rama_q8_spec_stats(rama_ctx* c, rama_q8_spec_report* out) {
    RAMA_ENTER(c);
    REQUIRE(c && out && c->q8p.active, RAMA_EINVAL, "q8_spec_stats: bad argument");
    auto& sp = c->q8p;
    { const int rh = q8_drain(c); if (rh) return rh; }
    SpecState s{};
    HIPCHK(hipMemcpy(&s, sp.t.st, sizeof s, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->steps = s.steps; out->graph_captures = sp.captures; out->rows_fed = s.rows_fed; out->drafts = s.drafts;
    out->accepted = s.accepted; out->emitted = s.emitted;
    static_assert(sizeof out->accepted_hist == sizeof s.hist, "one histogram entry per accept count 0..15");
    memcpy(out->accepted_hist, s.hist, sizeof s.hist);
    out->finished = s.finished; out->n_out = s.n_out; out->cursor = s.L - 1;
    return 0;
}

int rama_q8_spec_model_stats(rama_ctx* c, rama_q8_spec_model_report* out) {
    RAMA_ENTER(c);
    REQUIRE(c && out && c->q8p.active && c->q8p.model, RAMA_EINVAL, "q8_spec_model_stats: no chain begun with rama_q8_spec_begin_model");
    { const int rh = q8_drain(c); if (rh) return rh; }
    SpecModelState s{};
    HIPCHK(hipMemcpy(&s, c->q8p.mt.ms, sizeof s, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->draft_passes = s.draft_passes; out->draft_rows_fed = s.draft_rows_fed; out->catch_up_rows = s.catch_up_rows;
    out->draft_cursor = s.Dc;
    return 0;
}

int rama_q8_spec_tree_stats(rama_ctx* c, rama_q8_spec_tree_report* out) {
    RAMA_ENTER(c);
    REQUIRE(c && out && c->q8p.active && c->q8p.tree, RAMA_EINVAL, "q8_spec_tree_stats: no chain begun with rama_q8_spec_begin_tree");
    { const int rh = q8_drain(c); if (rh) return rh; }
    TreeState s{};
    HIPCHK(hipMemcpy(&s, c->q8p.tt.ts, sizeof s, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->off_trunk_accepted = s.off_trunk_accepted; out->off_trunk_steps = s.off_trunk_steps;
    static_assert(sizeof out->nodes_hist == sizeof s.nodes_hist, "one histogram entry per node count 0..15");
    memcpy(out->nodes_hist, s.nodes_hist, sizeof s.nodes_hist);
    out->n_branch = s.n_branch; out->n_rows = s.n_rows;
    return 0;
}

// ---- TREE DRAFTS (q8_tree.hpp): the two rules as host-only pure functions, and the eager building blocks

// the drafting rule over a tree on the host (spec_tree_draft_kernel finds the same occurrences by n_branch max reductions)
int rama_q8_spec_tree_draft(const int32_t* hint, int n_hint, const int32_t* seq, int L, int n_draft, int ngram, int room, int n_branch, int n_rows,
                            int32_t* tok_out, int32_t* parent_out, int32_t* depth_out) {
    REQUIRE(seq && L >= 1 && n_hint >= 0 && n_hint < kSpecHintBit && L < kSpecHintBit && (n_hint == 0 || hint), RAMA_EINVAL, "q8_spec_tree_draft: bad text");
    REQUIRE(n_draft >= 0 && n_draft <= kSpecMaxDraft && ngram >= 1 && ngram <= kSpecMaxNgram, RAMA_EINVAL,
            "q8_spec_tree_draft: n_draft in 0..15, ngram in 1..4");
    REQUIRE(n_branch >= 1 && n_branch <= kTreeMaxBranch && n_rows >= 2 && n_rows <= kSpecRows, RAMA_EINVAL,
            "q8_spec_tree_draft: n_branch in 1..4, n_rows in 2..16");
    REQUIRE(tok_out && parent_out && depth_out, RAMA_EINVAL, "q8_spec_tree_draft: NULL argument");
    const int cap = std::min(n_draft, room);
    int tok[kSpecRows], parent[kSpecRows], depth[kSpecRows], m = 0;
    tok[0] = seq[L - 1]; parent[0] = -1; depth[0] = 0;
    for (int n = std::min(ngram, L); cap > 0 && n >= 1; n--) {
        const int32_t* tail = seq + (L - n);
        // the occurrences by descending key: the hint's before the sequence's, a later end first; in the sequence they end before L
        std::vector<int> keys;
        for (int k = n_hint; k >= n && (int)keys.size() < n_branch; k--) if (!memcmp(hint + (k - n), tail, sizeof(int32_t) * n)) keys.push_back(kSpecHintBit | k);
        for (int k = L - 1; k >= n && (int)keys.size() < n_branch; k--) if (!memcmp(seq + (k - n), tail, sizeof(int32_t) * n)) keys.push_back(k);
        if (keys.empty()) continue;
        for (int key : keys) {
            const bool in_hint = (key & kSpecHintBit) != 0;
            const int e = key & (kSpecHintBit - 1), len = std::min(cap, (in_hint ? n_hint : L) - e);
            if (!spec_tree_insert(tok, parent, depth, &m, (in_hint ? hint : seq) + e, len, n_rows)) break;
        }
        break;
    }
    for (int j = 1; j <= m; j++) { tok_out[j - 1] = tok[j]; parent_out[j - 1] = parent[j]; depth_out[j - 1] = depth[j]; }
    return m;
}

// ---- TREES FROM A DRAFT MODEL (q8_spec_model_tree.hpp): the shape and the candidate order as host-only pure functions

int rama_q8_spec_model_tree_shape(int cap, int n_branch, int n_rows, int32_t* parent_out, int32_t* depth_out, int32_t* rank_out) {
    REQUIRE(cap >= 0 && cap <= kSpecMaxDraft && n_branch >= 1 && n_branch <= kTreeMaxBranch && n_rows >= 2 && n_rows <= kSpecRows, RAMA_EINVAL,
            "q8_spec_model_tree_shape: cap in 0..15, n_branch in 1..4, n_rows in 2..16");
    REQUIRE(parent_out && depth_out && rank_out, RAMA_EINVAL, "q8_spec_model_tree_shape: NULL argument");
    int parent[kSpecRows], depth[kSpecRows], rank[kSpecRows];
    const int m = spec_model_tree_shape(cap, n_branch, n_rows, parent, depth, rank);
    for (int j = 1; j <= m; j++) { parent_out[j - 1] = parent[j]; depth_out[j - 1] = depth[j]; rank_out[j - 1] = rank[j]; }
    return m;
}

// (spec_model_tree_pick_kernel finds the same tokens by n rounds of a workgroup-wide maximum below the round before's)
int rama_q8_spec_model_tree_candidates(const float* logits_host, int vocab_size, int rank0_token, int n, int32_t* out) {
    REQUIRE(logits_host && vocab_size >= 1 && rank0_token >= 0 && rank0_token < vocab_size, RAMA_EINVAL,
            "q8_spec_model_tree_candidates: a logits row and a rank-0 token inside it");
    REQUIRE(n >= 0 && n < kTreeMaxBranch && n < vocab_size && (n == 0 || out), RAMA_EINVAL,
            "q8_spec_model_tree_candidates: n in 0..3, below vocab_size");
    unsigned long long limit = ~0ull;
    for (int r = 0; r < n; r++) {
        unsigned long long best = 0ull;
        for (int i = 0; i < vocab_size; i++) {
            unsigned bits;
            memcpy(&bits, logits_host + i, sizeof bits);
            const unsigned long long k1 = spec_model_tree_key1(bits, i);
            if (i != rank0_token && k1 < limit && k1 > best) best = k1;
        }
        out[r] = (int32_t)(unsigned)((best - 1ull) & 0xffffffffull);
        limit = best;
    }
    return n;
}

int rama_q8_spec_model_tree_last(rama_ctx* c, int32_t* tok, int32_t* parent, int32_t* depth, int32_t* picks, int32_t* path, int* m, int* a) {
    RAMA_ENTER(c);
    REQUIRE(c && tok && parent && depth && picks && path && m && a && c->q8p.active && c->q8p.model && c->q8p.tree, RAMA_EINVAL,
            "q8_spec_model_tree_last: no chain begun with rama_q8_spec_begin_model_tree");
    { const int rh = q8_drain(c); if (rh) return rh; }
    TreeState ts{};
    SpecState s{};
    HIPCHK(hipMemcpy(&ts, c->q8p.tt.ts, sizeof ts, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&s, c->q8p.t.st, sizeof s, hipMemcpyDeviceToHost));
    REQUIRE(ts.m >= 0 && ts.m < kSpecRows && ts.a >= 0 && ts.a <= ts.m, RAMA_EINVAL, "q8_spec_model_tree_last: no step has run");
    for (int j = 0; j <= ts.m; j++) { tok[j] = ts.tok[j]; parent[j] = ts.parent[j]; depth[j] = ts.depth[j]; picks[j] = s.picks[j]; }
    for (int k = 0; k <= ts.a; k++) path[k] = ts.path[k];
    *m = ts.m; *a = ts.a;
    return 0;
}

// a caller's tree: parent[0] = -1, parent[j] in [0, j), depth at most 15 -> its depths; false for anything else
static bool tree_depths(const int32_t* parent, int n, int* depth) {
    if (n < 1 || n > kSpecRows || parent[0] != -1) return false;
    depth[0] = 0;
    for (int j = 1; j < n; j++) {
        if (parent[j] < 0 || parent[j] >= j) return false;
        depth[j] = depth[parent[j]] + 1;
        if (depth[j] > kSpecMaxDraft) return false;
    }
    return true;
}

int rama_q8_spec_tree_accept(const int32_t* tok, const int32_t* parent, int m, const int32_t* picks, int stop_token, int remaining, int32_t* path_out,
                             int* a_out, int* finished) {
    REQUIRE(picks && m >= 0 && m <= kSpecMaxDraft && (m == 0 || (tok && parent)) && remaining >= 1, RAMA_EINVAL,
            "q8_spec_tree_accept: m in 0..15 nodes, m + 1 picks, remaining >= 1");
    int t[kSpecRows] = {0}, p[kSpecRows] = {-1}, depth[kSpecRows];
    for (int j = 1; j <= m; j++) { t[j] = tok[j - 1]; p[j] = parent[j - 1]; }
    REQUIRE(tree_depths(p, m + 1, depth), RAMA_EINVAL, "q8_spec_tree_accept: parent[j] must lie in [0, j]");
    int a = 0, fin = 0, path[kSpecRows], emitted[kSpecRows];
    const int emit = spec_tree_accept_rule(t, p, m, picks, stop_token, remaining, path, emitted, &a, &fin);
    if (path_out) for (int k = 0; k <= a; k++) path_out[k] = path[k];
    if (a_out) *a_out = a;
    if (finished) *finished = fin;
    return emit;
}

// the eager pass's tables: one small blob for the context's life, and a tree store that grows with the model (never inside a capture)
static int ensure_q8_tree(rama_ctx* c, const rama_config* cfg) {
    auto& q = c->q8t;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    REQUIRE(hipStreamIsCapturing(c->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone, RAMA_EINVAL, "q8_tree_forward: not inside a capture");
    auto lay = [&](char* base) {
        BlobCarver bc{base};
        bc.take(q.rows, kSpecRows); bc.take(q.row_tok, kSpecRows); bc.take(q.tt.ts, 1); bc.take(q.tt.anc, kSpecRows);
        return bc.used;
    };
    if (!q.blob) {
        const size_t need = lay(nullptr);
        HIPCHK(hipMalloc(&q.blob, need));
        HIPCHK(hipMemset(q.blob, 0, need));
    }
    lay(q.blob);
    const size_t n = (size_t)cfg->n_layers * (size_t)kSpecMaxDraft * (size_t)cfg->dim;
    if (2 * n * sizeof(float) > q.store_cap) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (q.store) { HIPCHK(hipFree(q.store)); q.store = nullptr; }
        q.store_cap = 0; q.kc = nullptr;
        HIPCHK(hipMalloc(&q.store, 2 * n * sizeof(float)));
        q.store_cap = 2 * n * sizeof(float);
    }
    q.tt.ks = reinterpret_cast<float*>(q.store); q.tt.vs = q.tt.ks + n; q.tt.store_rows = kSpecMaxDraft;
    return 0;
}

int rama_q8_tree_forward(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* state, const int32_t* tokens_host,
                         const int32_t* parent_host, int n_rows, int pos0, float* logits_dev) {
    RAMA_ENTER(c);
    REQUIRE(c && state && tokens_host && parent_host && logits_dev, RAMA_EINVAL, "q8_tree_forward: NULL argument");
    int rc = q8_check(c, cfg, w, state); if (rc) return rc;
    int depth[kSpecRows];
    REQUIRE(n_rows >= 1 && n_rows <= kSpecRows && tree_depths(parent_host, n_rows, depth), RAMA_EINVAL,
            "q8_tree_forward: 1..16 rows, parent[0] = -1, parent[j] in [0, j), depth at most 15");
    int deepest = 0;
    for (int j = 0; j < n_rows; j++) deepest = std::max(deepest, depth[j]);
    REQUIRE(pos0 >= 0 && pos0 < cfg->seq_len - deepest, RAMA_EINVAL, "q8_tree_forward: positions outside [0, seq_len)");
    CHECKED(check_tokens("q8_tree_forward", "token outside the vocabulary", tokens_host, n_rows, cfg->vocab_size));
    UNSUPPORTED_UNLESS(q8_batch_ok(cfg), "q8_tree_forward", "a shape the Q8 token-batch pass does not take");
    if (set_device(c)) return 1;
    Q8BatchScratch b{};
    rc = q8_chain_scratch(c, cfg, w->group_size, 0, &b); if (rc) return rc;
    rc = ensure_q8_tree(c, cfg); if (rc) return rc;
    auto& q = c->q8t;
    c->embedded_x = nullptr; c->host_pos = -1;
    struct { SeqSlot rows[kSpecRows]; int tok[kSpecRows]; TreeAnc anc[kSpecRows]; } h{};
    for (int j = 0; j < kSpecRows; j++) {
        const bool on = j < n_rows;
        h.rows[j] = on ? SeqSlot{state->key_cache, state->value_cache, pos0 + depth[j], 0} : SeqSlot{nullptr, nullptr, -1, -1};
        h.tok[j] = on ? tokens_host[j] : 0;
        unsigned long long path = 0ull;
        for (int cur = on ? j : 0, k = on ? depth[j] : 0; k >= 0; k--) { path |= (unsigned long long)cur << (4 * k); cur = std::max(parent_host[cur], 0); }
        h.anc[j] = TreeAnc{path, on ? depth[j] : 0, 0};
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(q.rows, h.rows, sizeof h.rows, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(q.row_tok, h.tok, sizeof h.tok, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(q.tt.anc, h.anc, sizeof h.anc, hipMemcpyHostToDevice));
    q.kc = nullptr;
    rc = enqueue_q8_batch_pass(c, cfg, w, b, q.row_tok, q.rows, n_rows, &q.tt); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(logits_dev, b.LG, sizeof(float) * (size_t)n_rows * (size_t)cfg->vocab_size, hipMemcpyDeviceToDevice, c->stream));
    q.kc = state->key_cache; q.n_rows = n_rows; q.pos0 = pos0; q.n_layers = cfg->n_layers; q.dim = cfg->dim; q.seq_len = cfg->seq_len;
    for (int j = 0; j < n_rows; j++) q.parent[j] = parent_host[j];
    return 0;
}

int rama_q8_tree_commit(rama_ctx* c, const rama_config* cfg, const rama_run_state* state, const int32_t* path_host, int n_path, int pos0) {
    RAMA_ENTER(c);
    REQUIRE(c && cfg && state && path_host, RAMA_EINVAL, "q8_tree_commit: NULL argument");
    { const int rc = check_cfg(cfg); if (rc) return rc; }
    const auto& q = c->q8t;
    REQUIRE(state->key_cache && state->value_cache && q.kc == state->key_cache, RAMA_EINVAL, "q8_tree_commit: no tree pass on this run state to commit");
    REQUIRE(cfg->n_layers == q.n_layers && cfg->dim == q.dim && cfg->seq_len == q.seq_len && pos0 == q.pos0, RAMA_EINVAL,
            "q8_tree_commit: not the last tree pass's model and position");
    REQUIRE(n_path >= 1 && n_path <= q.n_rows && path_host[0] == 0, RAMA_EINVAL, "q8_tree_commit: a path starts at the root, row 0");
    for (int k = 1; k < n_path; k++)
        REQUIRE(path_host[k] >= 1 && path_host[k] < q.n_rows && q.parent[path_host[k]] == path_host[k - 1], RAMA_EINVAL,
                "q8_tree_commit: every row of the path must be a child of the row before it");
    if (set_device(c)) return 1;
    TreeState h{};
    h.a = n_path - 1; h.pos0 = pos0;
    for (int k = 0; k < n_path; k++) h.path[k] = path_host[k];
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(q.tt.ts, &h, sizeof h, hipMemcpyHostToDevice));
    return launch_tree_commit(c, q.tt, state->key_cache, state->value_cache, q.n_layers, q.dim, q.seq_len);
}
