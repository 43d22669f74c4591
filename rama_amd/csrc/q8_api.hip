// q8_api.hip -- the Q8 part of the C ABI of include/rama_hip.h: rama_q8_quantize / _matmul, the Q8 forward and generate, the token
// batches (prefill, decode batch), the chained batch, the serving chain (with and without drafts) and the speculative chain.  The kernels are q8.hpp,
// q8_batch.hpp, q8_serve.hpp, q8_fork.hpp, q8_spec.hpp, q8_spec_model.hpp, q8_serve_spec.hpp and q8_serve_model.hpp; parity mode's norms and attention and the samplers are reached through the launchers of ctx.hpp, which chain_api.hip
// defines -- this translation unit instantiates none of their kernels (DESIGN.md "Translation units").
// The three device-chained loops are states of their own (rama_ctx::Q8Chain / Q8Serve / Q8Spec over Q8ChainBase) that share PROCEDURES, each
// written once here (DESIGN.md "Q8 chains: shared pass, layout, pick and lookup"): q8_chains (graph and lifetime handling), q8_product (a layer's five
// products, for the forward and the batch), BlobCarver (a blob's tables), enqueue_q8_row_layers / enqueue_q8_batch_pass (a pass over a device row
// table), enqueue_q8_pick_rows (what a sampled step does behind the classifier), q8_chain_scratch / q8_chain_steps (the begin and _steps
// preambles, the step loop), q8_drain / q8_tokens_back (the _tokens and _stats entries) and the check_* refusals in the calling entry's words.
#include "ctx.hpp"
#include "q8.hpp"
#include "q8_batch.hpp"
#include "q8_serve.hpp"
#include "q8_fork.hpp"
#include "q8_spec.hpp"
#include "q8_spec_model.hpp"
#include "q8_tree.hpp"
#include "q8_serve_spec.hpp"
#include "q8_serve_model.hpp"

#ifdef RAMA_CHAIN_HPP
#error "q8_api.hip must not include chain.hpp: its kernels and g_pred_stats belong to chain_api.hip's code object"
#endif

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <vector>

// the three device-chained loops, as what their graph and lifetime handling needs of them: the chained batch, the serving chain, the speculative chain
static std::array<rama_ctx::Q8ChainBase*, 3> q8_chains(rama_ctx* c) { return {&c->q8c, &c->q8s, &c->q8p}; }

// the captured Q8 steps: all of them (s == NULL) or those over one run state (drop_graph and rama_state_free of rama_api.hip call this too)
void drop_q8_graphs(rama_ctx* c, const rama_run_state* s) {
    // a chain's step goes with all Q8 graphs (its next _steps call captures again), and with a run state the chain still uses -- after which the
    // chain is dead.  Which run states those are is each chain's own: a member's, a live slot's, the one sequence's.
    auto& sv = c->q8s;
    if (s && c->q8t.kc == s->key_cache) c->q8t.kc = nullptr;      // the last eager tree pass was this run state's: nothing of it to commit any more
    const auto& sp = c->q8p;         // (a chain with a draft model uses two run states)
    bool uses[3] = {false, false, s && sp.active && (sp.state.key_cache == s->key_cache || (sp.model && sp.dstate.key_cache == s->key_cache))};
    for (const auto& m : c->q8c.states) uses[0] = uses[0] || (s && m.key_cache == s->key_cache);
    // the serving chain's per-slot rule: the run state of a slot whose occupant the host cannot yet see DONE ends the chain -- a finished
    // occupant's is its owner's again
    uses[1] = s && serve_state_uses(sv, s);
    const auto chains = q8_chains(c);
    for (int k = 0; k < 3; k++) {
        if (uses[k] || (!s && chains[k]->cg.exec)) (void)hipStreamSynchronize(c->stream);
        if (uses[k] || !s) destroy_graph(chains[k]->cg);
        if (uses[k]) chains[k]->live = false;
    }
    bool any = false;
    for (auto& e : c->q8g) any = any || !s || !memcmp(&e.s, s, sizeof *s);
    if (!any) return;
    (void)hipStreamSynchronize(c->stream);
    for (size_t i = 0; i < c->q8g.size();) {
        auto& e = c->q8g[i];
        if (s && memcmp(&e.s, s, sizeof *s)) { i++; continue; }
        destroy_graph(e.cg);
        c->q8g.erase(c->q8g.begin() + (long)i);
    }
}
// q8_model.hip: a Q8 model (weights *freed) is about to go: the captured Q8 steps, and a chain over it is dead (one never begun, or ended, is
// not live in the first place)
extern "C" void rama_internal_drop_q8_graphs(rama_ctx* c, const rama_q8_weights* freed) {
    if (!c) return;
    drop_q8_graphs(c, nullptr);
    for (auto* ch : q8_chains(c))
        if (freed && ch->w.wq == freed->wq) ch->live = false;
    if (freed && c->q8p.model && c->q8p.dw.wq == freed->wq) c->q8p.live = false;      // the speculative chain's draft model
    if (freed && c->q8s.model && c->q8s.dw.wq == freed->wq) c->q8s.live = false;      // ... and the serving chain's
    // ... and the fp32 serving chain's (rama_serve_begin_model): its captured step is no Q8 graph, and goes only with its own draft model
    if (freed && c->sv.model && c->sv.dw.wq == freed->wq) { destroy_graph(c->sv.cg); c->sv.live = false; }
}

// the serving chain's allocations (rama_q8_serve_begin / _end, release_q8); the stream is idle
void serve_state_free(rama_ctx::ServeState& sv) {
    hipFree(sv.blob); hipFree(sv.stage);
    if (sv.pinned) hipHostFree(sv.pinned);
    if (sv.ring) hipHostFree(sv.ring);
    if (sv.done) hipHostFree(sv.done);
    hipFree(sv.sstage);
    if (sv.spinned) hipHostFree(sv.spinned);
    hipFree(sv.mblob); hipFree(sv.dblob);
}
static void serve_release(rama_ctx* c) {
    auto& sv = c->q8s;
    destroy_graph(sv.cg);
    serve_state_free(sv);
    sv = rama_ctx::Q8Serve();
}
// ... and the chained batch's
static void q8_chain_release(rama_ctx* c) {
    auto& qc = c->q8c;
    destroy_graph(qc.cg);
    hipFree(qc.toks); hipFree(qc.seqs); hipFree(qc.out); hipFree(qc.ends); hipFree(qc.rows); hipFree(qc.forced);
    if (qc.ring) hipHostFree(qc.ring);
    if (qc.done) hipHostFree(qc.done);
    qc = rama_ctx::Q8Chain();
}
// ... and the speculative chain's
static void spec_release(rama_ctx* c) {
    auto& sp = c->q8p;
    destroy_graph(sp.cg);
    hipFree(sp.blob); hipFree(sp.dblob); hipFree(sp.tblob);
    if (sp.ring) hipHostFree(sp.ring);
    if (sp.words) hipHostFree(sp.words);
    sp = rama_ctx::Q8Spec();
}
// rama_ctx_destroy: everything of the Q8 stack the context holds (the captured steps have gone with drop_q8_graphs)
void release_q8(rama_ctx* c) {
    q8_chain_release(c);
    serve_release(c);
    spec_release(c);
    hipFree(c->q8_xq); hipFree(c->q8_xs); hipFree(c->q8b_blob);
    hipFree(c->q8t.blob); hipFree(c->q8t.store);
    c->q8t = rama_ctx::Q8Tree();
}

// ---------------------------------------------------------------- Q8_0 models (q8.hpp, q8_model.hip)
// The forward of a version-2 checkpoint: parity mode's exact norms, RoPE + cache append, attention, SiLU and residual adds,
// with every matmul replaced by runq.c's quantized product (rama_hip.h).  Per layer: norm, quantize,
// Wq|Wk|Wv, RoPE + cache rows, attention, quantize, Wo (+ residual), norm, quantize, W1|W3 (+ SiLU * gate), quantize, W2 (+ residual).

static int launch_q8_quantize(rama_ctx* c, const float* x, int n, int gs, int8_t* q, float* s) {
    const int groups = n / gs;
    RAMA_LAUNCH(c, q8_quantize_kernel, dim3((groups + 3) / 4), dim3(256), 0, x, n, gs, q, s);
    LAUNCHCHK();
    return 0;
}

// The kernel a Q8 product takes: the one statement of the dispatch rule (launch_q8_matvec and launch_q8_gemm ask it; so can a caller).
// n_tok == 0 is the single-token matvec; a batch answers for one pass of min(n_tok, kQ8bMaxTok) tokens.  aligned16: the activations and
// every matrix of the product start on a 16-byte boundary.  The fast matvec keeps kQ8Waves x 2 rows of group terms in 64 KiB of LDS.
int rama_q8_product_path(size_t n, int group_size, int n_tok, int aligned16) {
    REQUIRE(group_size > 0 && n > 0 && n % (size_t)group_size == 0 && n < ((size_t)1 << 31) && n_tok >= 0, RAMA_EINVAL,
            "q8_product_path: group_size must divide n, n_tok >= 0");
    const int K = (int)n, gs = group_size;
    if (n_tok == 0) {
        const size_t lds = (size_t)kQ8Waves * 2 * (K / gs) * sizeof(float);
        return aligned16 && q8_matvec_fast_ok(K, gs) && lds <= 64 * 1024 ? RAMA_Q8_PATH_MATVEC : RAMA_Q8_PATH_MATVEC_GENERIC;
    }
    if (!aligned16 || !q8_gemm_mfma_ok(K, gs)) return RAMA_Q8_PATH_GEMM_GENERIC;
    // few tokens: K split over the waves of a workgroup
    return std::min(n_tok, kQ8bMaxTok) <= 32 && (gs == 32 || gs == 64) ? RAMA_Q8_PATH_GEMM_KSPLIT : RAMA_Q8_PATH_GEMM_MFMA;
}

template <int EPI>
static int launch_q8_matvec(rama_ctx* c, Q8MatParams& p) {
    const int G = p.K / p.gs, nm = EPI == Q8EPI_SWIGLU ? 2 : p.nmat;
    bool al = aligned16(p.xq);
    for (int m = 0; m < nm; m++) al = al && aligned16(p.w[m]);
    if (rama_q8_product_path((size_t)p.K, p.gs, 0, al) == RAMA_Q8_PATH_MATVEC) {
        const int tasks = EPI == Q8EPI_SWIGLU ? p.rows : (p.nmat * p.rows + 1) / 2;
        const size_t lds = (size_t)kQ8Waves * 2 * G * sizeof(float);
        RAMA_LAUNCH(c, (q8_matvec_kernel<2, EPI>), dim3((tasks + kQ8Waves - 1) / kQ8Waves), dim3(kQ8Waves * 64), lds, p);
    } else {
        const int total = EPI == Q8EPI_SWIGLU ? p.rows : p.nmat * p.rows;
        RAMA_LAUNCH(c, (q8_matvec_generic_kernel<EPI>), dim3((total + 255) / 256), dim3(256), 0, p);
    }
    LAUNCHCHK();
    return 0;
}

int rama_q8_quantize(rama_ctx* c, const float* x, size_t n, int group_size, int8_t* q, float* s) {
    RAMA_ENTER(c);
    REQUIRE(c && x && q && s, RAMA_EINVAL, "q8_quantize: NULL argument");
    REQUIRE(group_size > 0 && n > 0 && n % (size_t)group_size == 0 && n < ((size_t)1 << 31), RAMA_EINVAL, "q8_quantize: group_size must divide n");
    if (set_device(c)) return 1;
    RAMA_WRITES(c, s, n / group_size);
    return launch_q8_quantize(c, x, (int)n, group_size, q, s);
}

int rama_q8_matmul(rama_ctx* c, float* o, const int8_t* wq, const float* ws, const int8_t* xq, const float* xs, size_t n, size_t d, int group_size) {
    RAMA_ENTER(c);
    REQUIRE(c && o && wq && ws && xq && xs, RAMA_EINVAL, "q8_matmul: NULL argument");
    REQUIRE(group_size > 0 && n > 0 && d > 0 && n % (size_t)group_size == 0 && n < ((size_t)1 << 31) && d < ((size_t)1 << 31), RAMA_EINVAL,
            "q8_matmul: group_size must divide n");
    if (set_device(c)) return 1;
    RAMA_WRITES(c, o, d);
    Q8MatParams p{};
    p.w[0] = wq; p.ws[0] = ws; p.o[0] = o; p.xq = xq; p.xs = xs; p.K = (int)n; p.rows = (int)d; p.gs = group_size; p.nmat = 1;
    return launch_q8_matvec<Q8EPI_STORE>(c, p);
}

static bool q8_weights_complete(const rama_q8_weights* w) {
    return w->token_embedding_table && w->rms_att_weight && w->rms_ffn_weight && w->rms_final_weight && w->freq_cis_real && w->freq_cis_imag &&
           w->wq && w->wk && w->wv && w->wo && w->w1 && w->w2 && w->w3 && w->wcls && w->wq_s && w->wk_s && w->wv_s && w->wo_s && w->w1_s &&
           w->w2_s && w->w3_s && w->wcls_s;
}

static int q8_check(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* s) {
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    int rc = check_cfg(cfg); if (rc) return rc;
    REQUIRE(w && s, RAMA_EINVAL, "q8 forward: NULL argument");
    const int gs = w->group_size;
    REQUIRE(gs > 0 && cfg->dim % gs == 0 && cfg->hidden_dim % gs == 0, RAMA_EINVAL, "q8 forward: group_size must divide dim and hidden_dim");
    REQUIRE(q8_weights_complete(w), RAMA_EINVAL, "q8 forward: missing weights");
    REQUIRE(s->x && s->xb && s->hb && s->q && s->k && s->v && s->att && s->logits && s->key_cache && s->value_cache, RAMA_EINVAL,
            "q8 forward: missing state buffer");
    return 0;
}

// ---- The refusals several entries share, each in the calling entry's words: "<entry>: <what>" is the text that entry has always given.  An
// entry calls them where its own REQUIREs of the same matter stood, so which error a bad call gets does not change.
static int refuse(const char* entry, const char* what, int line, int code = RAMA_EINVAL) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", entry, what);
    return fail(code, msg, __FILE__, line);
}
#define REFUSE_UNLESS(cond, entry, what) do { if (!(cond)) return refuse((entry), (what), __LINE__); } while (0)
#define UNSUPPORTED_UNLESS(cond, entry, what) do { if (!(cond)) return refuse((entry), (what), __LINE__, RAMA_EUNSUP); } while (0)

// every token of a list is in the vocabulary
static int check_tokens(const char* entry, const char* what, const int32_t* toks, int n, int V) {
    for (int i = 0; i < n; i++) REFUSE_UNLESS(toks[i] >= 0 && toks[i] < V, entry, what);
    return 0;
}
// a sampling plan's two halves (rama_q8_decode_batch_begin has refusals of its own between them): Device::sample's (temperature, topp, u) ...
static int check_sampler(const char* entry, float temperature, float topp, float u) {
    REFUSE_UNLESS(topp_params_ok(temperature, topp, u), entry, "temperature >= 0, topp in [0,1], u in [0,1)");
    return 0;
}
// ... and the stop token (-1: none) against the vocabulary
static int check_stop_token(const char* entry, int stop_token, int V) {
    REFUSE_UNLESS(stop_token >= -1 && stop_token < V, entry, "stop token outside the vocabulary");
    return 0;
}
// the drafting fields of a plan (rama_q8_serve_spec, rama_q8_spec_plan): n_draft and the hint's length against the caller's caps -- those two
// refusals name the cap in the caller's words --, ngram, the hint's tokens against the vocabulary
template <class Plan>
static int check_drafting(const char* entry, const Plan& p, int n_draft_cap, const char* n_draft_what, int n_hint_cap, const char* hint_what, int V) {
    REFUSE_UNLESS(p.n_draft >= 0 && p.n_draft <= n_draft_cap, entry, n_draft_what);
    REFUSE_UNLESS(p.ngram >= 1 && p.ngram <= kSpecMaxNgram, entry, "ngram outside 1..4");
    REFUSE_UNLESS(p.n_hint >= 0 && (p.n_hint == 0 || p.hint) && p.n_hint <= n_hint_cap, entry, hint_what);
    return check_tokens(entry, "hint token outside the vocabulary", p.hint, p.n_hint, V);
}
// the serving chain's geometry, and a slot of a slot table handed to one of the two plan functions
int check_slots_rows(const char* entry, int n_slots, int max_rows) {
    REFUSE_UNLESS(n_slots >= 1 && n_slots <= kServeMaxSlots && max_rows >= n_slots && max_rows <= kQ8bMaxTok, entry, "1 <= n_slots <= max_rows <= 128");
    return 0;
}
static int check_plan_slot(const char* entry, const rama_q8_serve_slot& s) {
    REFUSE_UNLESS(s.state >= RAMA_SERVE_FREE && s.state <= RAMA_SERVE_DONE, entry, "bad slot state");
    if (s.state == RAMA_SERVE_PROMPT) REFUSE_UNLESS(s.n_context >= 1 && s.cursor >= 0 && s.cursor < s.n_context && s.max_new >= 1, entry, "bad PROMPT slot");
    if (s.state == RAMA_SERVE_DECODE) REFUSE_UNLESS(s.cursor >= 0 && s.n_out >= 1 && s.n_out < s.max_new, entry, "bad DECODE slot");
    return 0;
}
#define CHECKED(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// the int8 activations: one buffer of max(dim, hidden) values and as many scales (sized here, never inside a capture)
static int ensure_q8_scratch(rama_ctx* c, const rama_config* cfg) {
    const size_t need = (size_t)std::max(cfg->dim, cfg->hidden_dim);
    if (need <= c->q8_cap) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    REQUIRE(hipStreamIsCapturing(c->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone, RAMA_EINVAL,
            "q8: the activation scratch is sized by the first call, which must not be captured");
    HIPCHK(hipStreamSynchronize(c->stream));
    drop_q8_graphs(c, nullptr);        // (they hold the scratch's addresses; nothing else reads it)
    if (c->q8_xq) { HIPCHK(hipFree(c->q8_xq)); c->q8_xq = nullptr; }
    if (c->q8_xs) { HIPCHK(hipFree(c->q8_xs)); c->q8_xs = nullptr; }
    c->q8_cap = 0;
    HIPCHK(hipMalloc(&c->q8_xq, (need + 15) / 16 * 16));
    HIPCHK(hipMalloc(&c->q8_xs, need * sizeof(float)));
    c->q8_cap = need;
    return 0;
}

// the attention variant of a Q8 step: parity mode's exact attention, 16 waves per head from position 256, spread over the chip from "spread_pos"
static int q8_variant(rama_ctx* c, int pos) {
    c->long_attn = pos >= kLongAttnPos;
    c->spread_attn = pos >= c->tune_spread_pos;
    return c->spread_attn ? 2 : (c->long_attn ? 1 : 0);
}

static int q8_norm(rama_ctx* c, float* o, float* x, const float* gain, int n, float* copy_to) {
    KTimer kt(c, RAMA_K_NORM);
    if (rmsnorm_chain_ok(n)) return launch_rmsnorm_chain(c, o, x, gain, n, copy_to);
    if (copy_to) {      // xb = x; x = rmsnorm(xb) (infer.rs:49-50)
        hipLaunchKernelGGL(copy_kernel, dim3(ew_grid(n)), dim3(256), 0, c->stream, copy_to, (const float*)x, (size_t)n);
        LAUNCHCHK();
        return launch_rmsnorm_ref(c, o, copy_to, gain, n);
    }
    return launch_rmsnorm_ref(c, o, x, gain, n);
}

// The products of a model, stated once for the forward (P = Q8MatParams) and the token batch (Q8BatchParams): layer l's Wq|Wk|Wv, Wo, W1|W3 and
// W2, and the classifier (l ignored) -- the matrices and their scales, K, rows and nmat over the activations xq / xs, into o0 (.. o2).
enum Q8Product { Q8P_QKV, Q8P_WO, Q8P_W13, Q8P_W2, Q8P_CLS };
template <class P>
static P q8_product(const rama_config* cfg, const rama_q8_weights* w, int l, Q8Product kind, const int8_t* xq, const float* xs, float* o0, float* o1 = nullptr,
                    float* o2 = nullptr) {
    const int dim = cfg->dim, hidden = cfg->hidden_dim, gs = w->group_size;
    const size_t dd = (size_t)l * dim * dim, hd = (size_t)l * hidden * dim;      // layer l's offset in the square matrices and in the FFN's
    P p{};
    p.xq = xq; p.xs = xs; p.gs = gs; p.K = dim; p.rows = dim; p.nmat = 1;
    p.o[0] = o0; p.o[1] = o1; p.o[2] = o2;
    auto mat = [&](int m, const int8_t* q, const float* s, size_t off) { p.w[m] = q + off; p.ws[m] = s + off / gs; };
    switch (kind) {
    case Q8P_QKV: mat(0, w->wq, w->wq_s, dd); mat(1, w->wk, w->wk_s, dd); mat(2, w->wv, w->wv_s, dd); p.nmat = 3; break;
    case Q8P_WO:  mat(0, w->wo, w->wo_s, dd); break;
    case Q8P_W13: mat(0, w->w1, w->w1_s, hd); mat(1, w->w3, w->w3_s, hd); p.rows = hidden; p.nmat = 2; break;
    case Q8P_W2:  mat(0, w->w2, w->w2_s, hd); p.K = hidden; break;
    case Q8P_CLS: mat(0, w->wcls, w->wcls_s, 0); p.rows = cfg->vocab_size; break;
    }
    return p;
}

// one forward (token and position in the device cursor); embed = 0: x already holds the token's embedding (chained decode)
static int enqueue_q8_stage(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, rama_run_state* s, bool embed) {
    const int dim = cfg->dim, hidden = cfg->hidden_dim, hs = dim / cfg->n_heads, gs = w->group_size;
    int8_t* xq = c->q8_xq; float* xs = c->q8_xs;
    int rc;
    if (embed) {
        hipLaunchKernelGGL(embed_kernel, dim3((dim + 255) / 256), dim3(256), 0, c->stream, s->x, w->token_embedding_table, (const Ctl*)c->ctl, 0, dim);
        LAUNCHCHK();
    }
    for (int l = 0; l < cfg->n_layers; l++) {
        float* kc = s->key_cache + (size_t)l * cfg->seq_len * dim;
        float* vc = s->value_cache + (size_t)l * cfg->seq_len * dim;
        rc = q8_norm(c, s->xb, s->x, w->rms_att_weight + (size_t)l * dim, dim, nullptr); if (rc) return rc;          // infer.rs:19
        rc = launch_q8_quantize(c, s->xb, dim, gs, xq, xs); if (rc) return rc;
        {   // :20-23
            KTimer kt(c, RAMA_K_QKV);
            Q8MatParams p = q8_product<Q8MatParams>(cfg, w, l, Q8P_QKV, xq, xs, s->q, s->k, s->v);
            rc = launch_q8_matvec<Q8EPI_STORE>(c, p); if (rc) return rc;
        }
        hipLaunchKernelGGL(rope_ref_cursor_kernel, dim3((dim / 2 + 255) / 256), dim3(256), 0, c->stream, s->q, s->k, (const float*)s->v,
                           w->freq_cis_real, w->freq_cis_imag, dim, hs, kc, vc, (const Ctl*)c->ctl);                  // :25-33
        LAUNCHCHK();
        {   // :34
            KTimer kt(c, RAMA_K_ATTN);
            if (attn_chain_ok(hs, cfg->seq_len))
                rc = launch_attention_chain(c, s->xb, s->att, s->q, kc, vc, c->ctl, 0, dim, hs, cfg->seq_len, cfg->n_heads, c->long_attn, c->spread_attn);
            else rc = launch_attention_ref(c, s->xb, s->att, s->q, kc, vc, c->ctl, 0, dim, hs, cfg->seq_len, cfg->n_heads);
            if (rc) return rc;
        }
        rc = launch_q8_quantize(c, s->xb, dim, gs, xq, xs); if (rc) return rc;
        {   // :35-37: x = x + Wo . xb
            KTimer kt(c, RAMA_K_WO);
            Q8MatParams p = q8_product<Q8MatParams>(cfg, w, l, Q8P_WO, xq, xs, s->x);
            rc = launch_q8_matvec<Q8EPI_RESID>(c, p); if (rc) return rc;
        }
        rc = q8_norm(c, s->xb, s->x, w->rms_ffn_weight + (size_t)l * dim, dim, nullptr); if (rc) return rc;          // :39
        rc = launch_q8_quantize(c, s->xb, dim, gs, xq, xs); if (rc) return rc;
        {   // :41-45: hb = sinu(W1 . xb) * (W3 . xb)
            KTimer kt(c, RAMA_K_W13);
            Q8MatParams p = q8_product<Q8MatParams>(cfg, w, l, Q8P_W13, xq, xs, s->hb);
            rc = launch_q8_matvec<Q8EPI_SWIGLU>(c, p); if (rc) return rc;
        }
        rc = launch_q8_quantize(c, s->hb, hidden, gs, xq, xs); if (rc) return rc;
        {   // :46-47: x = x + W2 . hb
            KTimer kt(c, RAMA_K_W2);
            Q8MatParams p = q8_product<Q8MatParams>(cfg, w, l, Q8P_W2, xq, xs, s->x);
            rc = launch_q8_matvec<Q8EPI_RESID>(c, p); if (rc) return rc;
        }
    }
    // :49-51: xb = x; x = rmsnorm(xb); logits = Wcls . x
    rc = q8_norm(c, s->x, s->x, w->rms_final_weight, dim, s->xb); if (rc) return rc;
    rc = launch_q8_quantize(c, s->x, dim, gs, xq, xs); if (rc) return rc;
    KTimer kt(c, RAMA_K_CLS);
    Q8MatParams p = q8_product<Q8MatParams>(cfg, w, 0, Q8P_CLS, xq, xs, s->logits);
    return launch_q8_matvec<Q8EPI_STORE>(c, p);
}

// a chained step: the layers, then Device::sample (cursor advance, next token's embedding gather from the fp32 table)
static int enqueue_q8_step(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, rama_run_state* s) {
    int rc = enqueue_q8_stage(c, cfg, w, s, false);
    if (rc) return rc;
    ArgmaxParams ap{};
    ap.logits = s->logits; ap.n = cfg->vocab_size;
    ap.ctl = c->ctl; ap.forced = c->forced; ap.out = c->out; ap.out_cap = c->out_cap; ap.ring = c->ring_dev;
    ap.emb = w->token_embedding_table; ap.x = s->x; ap.dim = cfg->dim;
    return enqueue_sample(c, ap, c->samp_T, c->samp_topp, c->samp_u);
}

// eager, or replayed from the context's Q8 graph for (config, weights, state, attention variant, kind)
static int run_q8(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, rama_run_state* s, int variant, int chained) {
    auto enqueue = [&]() { return chained ? enqueue_q8_step(c, cfg, w, s) : enqueue_q8_stage(c, cfg, w, s, true); };
    if (!c->graph_mode || c->kp.kernel_id >= 0) return enqueue();
    rama_ctx::Q8Graph* hit = nullptr;
    for (auto& e : c->q8g)
        if (e.variant == variant && e.chained == chained && !memcmp(&e.cfg, cfg, sizeof *cfg) && !memcmp(&e.w, w, sizeof *w) && !memcmp(&e.s, s, sizeof *s)) { hit = &e; break; }
    if (!hit) {
        if (c->q8g.size() >= 16) {
            HIPCHK(hipStreamSynchronize(c->stream));
            for (auto& e : c->q8g) destroy_graph(e.cg);
            c->q8g.clear();
        }
        rama_ctx::Q8Graph e;
        const int rc = capture_graph(c, e.cg, enqueue);
        if (rc) return rc;
        e.cfg = *cfg; e.w = *w; e.s = *s; e.variant = variant; e.chained = chained;
        c->q8g.push_back(e);
        hit = &c->q8g.back();
    }
    return replay_graph(c, hit->cg);
}

int rama_q8_forward(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, rama_run_state* s, int token, int pos) {
    RAMA_ENTER(c);
    int rc = q8_check(c, cfg, w, s); if (rc) return rc;
    if (set_device(c)) return 1;
    REQUIRE(pos >= 0 && pos < cfg->seq_len, RAMA_EINVAL, "q8_forward: pos outside [0, seq_len)");
    REQUIRE(token >= 0 && token < cfg->vocab_size, RAMA_EINVAL, "q8_forward: token outside the vocabulary");
    rc = ensure_q8_scratch(c, cfg); if (rc) return rc;
    hipLaunchKernelGGL(set_ctl_kernel, dim3(1), dim3(1), 0, c->stream, c->ctl, token, pos, 0, 0);
    LAUNCHCHK();
    c->embedded_x = nullptr;
    c->host_pos = -1;
    return run_q8(c, cfg, w, s, q8_variant(c, pos), 0);
}

int rama_q8_generate(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, rama_run_state* s, const int32_t* prompt_host, int n_prompt,
                     int steps, float temperature, float topp, float u, int32_t* out_host) {
    RAMA_ENTER(c);
    int rc = q8_check(c, cfg, w, s); if (rc) return rc;
    REQUIRE(out_host, RAMA_EINVAL, "q8_generate: NULL argument");
    if (set_device(c)) return 1;
    rc = rama_decode_sampler(c, temperature, topp, u); if (rc) return rc;
    REQUIRE(steps >= 0 && steps <= cfg->seq_len && steps <= c->out_cap, RAMA_EINVAL, "q8_generate: steps outside [0, seq_len]");
    REQUIRE(n_prompt >= 0 && (n_prompt == 0 || prompt_host) && n_prompt <= c->forced_cap, RAMA_EINVAL, "q8_generate: bad prompt");
    CHECKED(check_tokens("q8_generate", "prompt token outside the vocabulary", prompt_host, n_prompt, cfg->vocab_size));
    rc = ensure_q8_scratch(c, cfg); if (rc) return rc;
    if (c->samp_T != 0.0f) { rc = ensure_topp_scratch(c, cfg->vocab_size); if (rc) return rc; c->topp_dist_dirty = true; }
    rc = rama_decode_begin(c, /*BOS*/ 1, 0, prompt_host, n_prompt); if (rc) return rc;
    if (steps == 0) { int n = 0; return rama_decode_tokens(c, out_host, 0, &n); }
    hipLaunchKernelGGL(embed_kernel, dim3((cfg->dim + 255) / 256), dim3(256), 0, c->stream, s->x, w->token_embedding_table, (const Ctl*)c->ctl, 0, cfg->dim);
    LAUNCHCHK();
    for (int i = 0; i < steps; i++) {
        rc = run_q8(c, cfg, w, s, q8_variant(c, c->host_pos), 1);
        if (rc) return rc;
        c->host_pos++;
    }
    c->embedded_x = nullptr;
    c->ring_hi = std::min(c->out_cap, c->ring_hi + steps);
    int n = 0;
    return rama_decode_tokens(c, out_host, steps, &n);
}

// ---------------------------------------------------------------- Q8_0 token batches (q8_batch.hpp)
// rama_q8_prefill and rama_q8_decode_batch: enqueue_q8_stage over up to kQ8bMaxTok tokens per weight pass.  The batched exact
// norm, the quantizer over T rows (a group never straddles a row), the batched product, RoPE + cache rows per token and parity
// mode's attention on a (heads, tokens) grid: every token's bits are those of its own rama_q8_forward.

template <int EPI>
static int launch_q8_gemm(rama_ctx* c, const Q8BatchParams& p) {
    const int nm = EPI == Q8EPI_SWIGLU ? 2 : p.nmat;
    bool al = aligned16(p.xq);
    for (int m = 0; m < nm; m++) al = al && aligned16(p.w[m]);
    const int G = p.K / p.gs;
    const int total = EPI == Q8EPI_SWIGLU ? p.rows : p.nmat * p.rows;
    const int tiles = (p.rows + 15) / 16, tasks = EPI == Q8EPI_SWIGLU ? tiles : p.nmat * tiles;
    for (int t0 = 0; t0 < p.n_tok; t0 += kQ8bMaxTok) {
        Q8BatchParams q = p;
        q.n_tok = std::min(kQ8bMaxTok, p.n_tok - t0);
        q.xq = p.xq + (size_t)t0 * p.K; q.xs = p.xs + (size_t)t0 * G;
        for (int m = 0; m < 3; m++) if (q.o[m]) q.o[m] = p.o[m] + (size_t)t0 * p.ostride;
        const int path = rama_q8_product_path((size_t)q.K, q.gs, q.n_tok, al);
        if (path == RAMA_Q8_PATH_GEMM_KSPLIT) {
            constexpr int RT = EPI == Q8EPI_SWIGLU ? 2 : 1;
#define RAMA_Q8S(NT_, G32_) RAMA_LAUNCH(c, (q8_gemm_ksplit_kernel<NT_, EPI, G32_>), dim3(tasks), dim3(kQ8sWaves * 64), q8s_lds_bytes(NT_, RT, G32_), q)
            if (q.n_tok <= 16) { if (q.gs == 32) RAMA_Q8S(1, true); else RAMA_Q8S(1, false); }
            else { if (q.gs == 32) RAMA_Q8S(2, true); else RAMA_Q8S(2, false); }
#undef RAMA_Q8S
        } else if (path == RAMA_Q8_PATH_GEMM_MFMA) {
            const dim3 grid((tasks + kQ8bWaves - 1) / kQ8bWaves), block(kQ8bWaves * 64);
#define RAMA_Q8G(NT_) do { if (q.gs == 32) RAMA_LAUNCH(c, (q8_gemm_mfma_kernel<NT_, EPI, true>), grid, block, 0, q); \
                           else RAMA_LAUNCH(c, (q8_gemm_mfma_kernel<NT_, EPI, false>), grid, block, 0, q); } while (0)
            if (q.n_tok <= 16) RAMA_Q8G(1);
            else if (q.n_tok <= 32) RAMA_Q8G(2);
            else if (q.n_tok <= 64) RAMA_Q8G(4);
            else RAMA_Q8G(8);
#undef RAMA_Q8G
        } else {
            RAMA_LAUNCH(c, (q8_gemm_generic_kernel<EPI>), dim3((total + 255) / 256, q.n_tok), dim3(256), 0, q);
        }
        LAUNCHCHK();
    }
    return 0;
}

int rama_q8_matmul_batch(rama_ctx* c, float* o, const int8_t* wq, const float* ws, const int8_t* xq, const float* xs, size_t n, size_t d,
                         int group_size, int n_tok) {
    RAMA_ENTER(c);
    REQUIRE(c && o && wq && ws && xq && xs, RAMA_EINVAL, "q8_matmul_batch: NULL argument");
    REQUIRE(group_size > 0 && n > 0 && d > 0 && n % (size_t)group_size == 0 && n < ((size_t)1 << 31) && d < ((size_t)1 << 31), RAMA_EINVAL,
            "q8_matmul_batch: group_size must divide n");
    REQUIRE(n_tok >= 1, RAMA_EINVAL, "q8_matmul_batch: n_tok < 1");
    if (set_device(c)) return 1;
    RAMA_WRITES(c, o, d * (size_t)n_tok);
    Q8BatchParams p{};
    p.w[0] = wq; p.ws[0] = ws; p.o[0] = o; p.xq = xq; p.xs = xs;
    p.K = (int)n; p.rows = (int)d; p.gs = group_size; p.nmat = 1; p.n_tok = n_tok; p.ostride = (int)d;
    return launch_q8_gemm<Q8EPI_STORE>(c, p);
}

// the batch path's scratch, row-major per token (T = kQ8bMaxTok): X residual rows, XN their norms, Q / Kr / V, XB attention
// output, HB, ATT score rows [T][n_heads][seq_len], LG logits [T][vocab]; the int8 activations [T][max(dim, hidden)] and their
// scales; token ids; the sequence table
struct Q8BatchScratch { float *X, *XN, *Q, *Kr, *V, *XB, *HB, *ATT, *LG; int8_t* xq; float* xs; int* toks; SeqSlot* seqs; int nw; size_t att_lds; };

// the shapes the batch path takes: those whose single-token forward runs parity mode's chain norm and chain attention
static bool q8_batch_ok(const rama_config* cfg) {
    const int hs = cfg->dim / cfg->n_heads;
    if (!rmsnorm_chain_ok((size_t)cfg->dim) || !attn_chain_ok(hs, cfg->seq_len) || cfg->dim % 4) return false;
    return attn_chain_lds_bytes(hs, cfg->seq_len, attn_chain_waves(hs, false)) <= kAttnChainMaxLds;
}

int rama_q8_batch_shape_ok(const rama_config* cfg) {
    REQUIRE(cfg, RAMA_EINVAL, "q8_batch_shape_ok: NULL argument");
    const int rc = check_cfg(cfg); if (rc) return rc;
    return q8_batch_ok(cfg) ? 1 : 0;
}

// (BlobCarver, ctx.hpp: the tables of one allocation in order)  A scratch of T rows over `base` (NULL: its size only), and the attention's geometry
static size_t q8_batch_scratch_lay(const rama_config* cfg, int gs, size_t T, char* base, Q8BatchScratch* b) {
    const size_t dim = (size_t)cfg->dim, hidden = (size_t)cfg->hidden_dim, mx = std::max(dim, hidden);
    BlobCarver bc{base};
    for (float** f : {&b->X, &b->XN, &b->Q, &b->Kr, &b->V, &b->XB}) bc.take(*f, T * dim);
    bc.take(b->HB, T * hidden); bc.take(b->ATT, T * (size_t)cfg->n_heads * cfg->seq_len); bc.take(b->LG, T * (size_t)cfg->vocab_size);
    bc.take(b->xq, T * mx); bc.take(b->xs, T * (mx / gs)); bc.take(b->toks, T); bc.take(b->seqs, T);
    const int hs = cfg->dim / cfg->n_heads;
    b->nw = attn_chain_waves(hs, false);
    b->att_lds = attn_chain_lds_bytes(hs, cfg->seq_len, b->nw);
    return bc.used;
}
static int ensure_q8_batch_scratch(rama_ctx* c, const rama_config* cfg, int gs, Q8BatchScratch* b) {
    auto lay = [&](char* base) { return q8_batch_scratch_lay(cfg, gs, kQ8bMaxTok, base, b); };
    const size_t need = lay(nullptr);
    if (need > c->q8b_cap) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        REQUIRE(hipStreamIsCapturing(c->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone, RAMA_EINVAL,
                "q8 batch: the scratch is sized by the first call, which must not be captured");
        HIPCHK(hipStreamSynchronize(c->stream));
        for (auto* ch : q8_chains(c)) destroy_graph(ch->cg);      // (every chain's step holds the old scratch's addresses)
        if (c->q8b_blob) { HIPCHK(hipFree(c->q8b_blob)); c->q8b_blob = nullptr; }
        c->q8b_cap = 0;
        HIPCHK(hipMalloc(&c->q8b_blob, need));
        c->q8b_cap = need;
    }
    lay(c->q8b_blob);
    return 0;
}

// the layers for nt tokens whose embeddings sit in b.X: consecutive positions p0.. of one sequence (key_cache / value_cache
// its caches), or -- seqs != NULL -- token t of independent sequence t (device table).  tree != NULL (q8_tree.hpp; seqs is then the tree's
// row table): the two launches that touch the cache are swapped for the tree's -- only row 0 writes its cache row, the others' k and v go to
// the tree store, and a row's attention reads the timesteps behind row 0's position from its ancestors' rows of this pass
static int q8_batch_layers(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const Q8BatchScratch& b, int nt, int p0,
                           float* key_cache, float* value_cache, const SeqSlot* seqs, const TreeTables* tree = nullptr) {
    const int dim = cfg->dim, hidden = cfg->hidden_dim, hs = dim / cfg->n_heads, H = cfg->n_heads, seq = cfg->seq_len, gs = w->group_size;
    int rc;
    for (int l = 0; l < cfg->n_layers; l++) {
        // a product of this layer over the nt rows of b.xq, into rows `ostride` floats apart
        auto product = [&](Q8Product kind, int ostride, float* o0, float* o1 = nullptr, float* o2 = nullptr) {
            Q8BatchParams p = q8_product<Q8BatchParams>(cfg, w, l, kind, b.xq, b.xs, o0, o1, o2);
            p.n_tok = nt; p.ostride = ostride;
            return p;
        };
        const size_t layer_off = (size_t)l * seq * dim;
        float* kc = key_cache ? key_cache + layer_off : nullptr;
        float* vc = value_cache ? value_cache + layer_off : nullptr;
        rc = launch_rmsnorm_chain(c, b.XN, b.X, w->rms_att_weight + (size_t)l * dim, dim, nullptr, nt, dim); if (rc) return rc;    // infer.rs:19
        rc = launch_q8_quantize(c, b.XN, nt * dim, gs, b.xq, b.xs); if (rc) return rc;
        rc = launch_q8_gemm<Q8EPI_STORE>(c, product(Q8P_QKV, dim, b.Q, b.Kr, b.V)); if (rc) return rc;                             // :20-23
        if (tree) {
            const size_t store_off = (size_t)l * tree->store_rows * dim;
            hipLaunchKernelGGL(q8_rope_tree_kernel, dim3((dim / 2 + 255) / 256, nt), dim3(256), 0, c->stream, b.Q, b.Kr, (const float*)b.V,
                               w->freq_cis_real, w->freq_cis_imag, dim, hs, seqs, layer_off, tree->ks + store_off, tree->vs + store_off);
            LAUNCHCHK();
            TreeAttnParams ta{};
            RefAttnParams& a = ta.a;
            a.q = b.Q; a.att = b.ATT; a.xb = b.XB; a.dim = dim; a.head_size = hs; a.seq_len = seq; a.tok_stride = dim; a.att_stride = H * seq;
            a.seqs = seqs; a.layer_off = layer_off;
            ta.anc = tree->anc; ta.kr = b.Kr; ta.v = b.V;
            rc = launch_attention_tree(c, ta, H, nt, b.nw, b.att_lds); if (rc) return rc;
        } else {
            hipLaunchKernelGGL(q8_rope_batch_kernel, dim3((dim / 2 + 255) / 256, nt), dim3(256), 0, c->stream, b.Q, b.Kr, (const float*)b.V,
                               w->freq_cis_real, w->freq_cis_imag, dim, hs, kc, vc, p0, seqs, layer_off);                    // :25-33
            LAUNCHCHK();
            // :34, one workgroup per (head, token)
            RefAttnParams a{};
            a.q = b.Q; a.kc = kc; a.vc = vc; a.att = b.ATT; a.xb = b.XB; a.ctl = nullptr; a.pos_val = p0;
            a.dim = dim; a.head_size = hs; a.seq_len = seq; a.tok_stride = dim; a.att_stride = H * seq;
            a.seqs = seqs; a.layer_off = layer_off;
            rc = launch_attention_chain_tokens(c, a, H, nt, b.nw, b.att_lds); if (rc) return rc;
        }
        rc = launch_q8_quantize(c, b.XB, nt * dim, gs, b.xq, b.xs); if (rc) return rc;
        rc = launch_q8_gemm<Q8EPI_RESID>(c, product(Q8P_WO, dim, b.X)); if (rc) return rc;                // :35-37: x = x + Wo . xb
        rc = launch_rmsnorm_chain(c, b.XN, b.X, w->rms_ffn_weight + (size_t)l * dim, dim, nullptr, nt, dim); if (rc) return rc;    // :39
        rc = launch_q8_quantize(c, b.XN, nt * dim, gs, b.xq, b.xs); if (rc) return rc;
        rc = launch_q8_gemm<Q8EPI_SWIGLU>(c, product(Q8P_W13, hidden, b.HB)); if (rc) return rc;          // :41-45: hb = sinu(W1 . xb) * (W3 . xb)
        rc = launch_q8_quantize(c, b.HB, nt * hidden, gs, b.xq, b.xs); if (rc) return rc;
        rc = launch_q8_gemm<Q8EPI_RESID>(c, product(Q8P_W2, dim, b.X)); if (rc) return rc;                // :46-47: x = x + W2 . hb
    }
    return 0;
}

int rama_q8_prefill(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, rama_run_state* s, const int32_t* tokens_host, int n_tokens, int pos0) {
    RAMA_ENTER(c);
    REQUIRE(c && tokens_host, RAMA_EINVAL, "q8_prefill: NULL argument");
    int rc = q8_check(c, cfg, w, s); if (rc) return rc;
    REQUIRE(n_tokens >= 1 && pos0 >= 0 && pos0 <= cfg->seq_len - n_tokens, RAMA_EINVAL, "q8_prefill: positions outside [0, seq_len)");
    CHECKED(check_tokens("q8_prefill", "token outside the vocabulary", tokens_host, n_tokens, cfg->vocab_size));
    if (set_device(c)) return 1;
    rc = ensure_q8_scratch(c, cfg); if (rc) return rc;
    // the last position runs as rama_q8_forward (x and logits); a batched pass of one token costs more than a forward (4.7 against
    // 3.8 ms at llama2-7B), so batches start at two tokens
    const int n_batch = q8_batch_ok(cfg) && n_tokens >= 3 ? n_tokens - 1 : 0;
    if (n_batch > 0) {
        Q8BatchScratch b{};
        rc = ensure_q8_batch_scratch(c, cfg, w->group_size, &b); if (rc) return rc;
        c->embedded_x = nullptr; c->host_pos = -1;
        for (int c0 = 0; c0 < n_batch; c0 += kQ8bMaxTok) {
            const int nt = std::min(kQ8bMaxTok, n_batch - c0);
            rc = stage_tokens(c, b.toks, tokens_host + c0, nt); if (rc) return rc;
            hipLaunchKernelGGL(embed_rows_kernel, dim3((cfg->dim + 255) / 256, nt), dim3(256), 0, c->stream, b.X, w->token_embedding_table,
                               (const int*)b.toks, nt, cfg->dim);
            LAUNCHCHK();
            rc = q8_batch_layers(c, cfg, w, b, nt, pos0 + c0, s->key_cache, s->value_cache, nullptr); if (rc) return rc;
        }
    }
    for (int i = n_batch; i < n_tokens; i++) { rc = rama_q8_forward(c, cfg, w, s, tokens_host[i], pos0 + i); if (rc) return rc; }
    return 0;
}

// infer.rs:49-51 for n_rows rows of src_rows [n_rows, dim]: x = rmsnorm(x), logits = Wcls . x -- the batched final norm, the quantizer
// and the classifier as one more product into b.LG [n_rows, vocab]
static int enqueue_q8_classifier(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const Q8BatchScratch& b, const float* src_rows, int n_rows) {
    const int dim = cfg->dim, V = cfg->vocab_size;
    int rc = launch_rmsnorm_chain(c, b.XN, src_rows, w->rms_final_weight, dim, nullptr, n_rows, dim); if (rc) return rc;
    rc = launch_q8_quantize(c, b.XN, n_rows * dim, w->group_size, b.xq, b.xs); if (rc) return rc;
    Q8BatchParams p = q8_product<Q8BatchParams>(cfg, w, 0, Q8P_CLS, b.xq, b.xs, b.LG);
    p.n_tok = n_rows; p.ostride = V;
    return launch_q8_gemm<Q8EPI_STORE>(c, p);
}

// A pass over a device row table: the embedding rows of row_tok and every layer over `rows` (n_rows of them; an idle row has position -1) ...
static int enqueue_q8_row_layers(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const Q8BatchScratch& b, const int* row_tok,
                                 const SeqSlot* rows, int n_rows, const TreeTables* tree = nullptr) {
    const int dim = cfg->dim;
    hipLaunchKernelGGL(embed_rows_kernel, dim3((dim + 255) / 256, n_rows), dim3(256), 0, c->stream, b.X, w->token_embedding_table, row_tok, n_rows, dim);
    LAUNCHCHK();
    return q8_batch_layers(c, cfg, w, b, n_rows, 0, nullptr, nullptr, rows, tree);
}
// ... and the classifier tail over every row: rama_q8_decode_batch's pass, and that of every chain's step but the serving chain's without
// drafts, which classifies the rows it has gathered
static int enqueue_q8_batch_pass(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const Q8BatchScratch& b, const int* row_tok,
                                 const SeqSlot* rows, int n_rows, const TreeTables* tree = nullptr) {
    const int rc = enqueue_q8_row_layers(c, cfg, w, b, row_tok, rows, n_rows, tree); if (rc) return rc;
    return enqueue_q8_classifier(c, cfg, w, b, b.X, n_rows);
}

// What every sampled chain's step does behind the classifier: the pick kernel's rows are b.LG's, and -- `sampled` -- the batched sampler's
// ordering launches over the rows' sampler records leave their slices in the context's scratch
static int enqueue_q8_pick_rows(rama_ctx* c, const Q8BatchScratch& b, int V, bool sampled, const ToppRow* trow, int n_rows, PickRows* r) {
    *r = PickRows{b.LG, (size_t)V, V, nullptr, nullptr, nullptr, 0};
    if (!sampled) return 0;
    const int rc = enqueue_topp_batch_order(c, trow, n_rows, b.LG, (size_t)V, V, nullptr); if (rc) return rc;
    r->keys = c->tb.keys; r->vals = c->tb.vals; r->m = c->tb.m; r->rstride = c->tb.rstride;
    return 0;
}

int rama_q8_decode_batch(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* states,
                         const int32_t* tokens_host, const int32_t* positions_host, int n_seq) {
    RAMA_ENTER(c);
    REQUIRE(c && states && tokens_host && positions_host, RAMA_EINVAL, "q8_decode_batch: NULL argument");
    REQUIRE(n_seq >= 1 && n_seq <= kQ8bMaxTok, RAMA_EINVAL, "q8_decode_batch: 1..128 sequences per call");
    for (int i = 0; i < n_seq; i++) {
        int rc = q8_check(c, cfg, w, &states[i]); if (rc) return rc;
        REQUIRE(tokens_host[i] >= 0 && tokens_host[i] < cfg->vocab_size, RAMA_EINVAL, "q8_decode_batch: token outside the vocabulary");
        REQUIRE(positions_host[i] >= 0 && positions_host[i] < cfg->seq_len, RAMA_EINVAL, "q8_decode_batch: position outside [0, seq_len)");
        for (int j = 0; j < i; j++)
            REQUIRE(states[j].key_cache != states[i].key_cache && states[j].value_cache != states[i].value_cache && states[j].logits != states[i].logits,
                    RAMA_EINVAL, "q8_decode_batch: two sequences share a run state");
    }
    if (set_device(c)) return 1;
    int rc = ensure_q8_scratch(c, cfg); if (rc) return rc;
    if (!q8_batch_ok(cfg) || n_seq == 1) {      // see rama_q8_prefill: one rama_q8_forward per sequence (and for a single one)
        for (int i = 0; i < n_seq; i++) {
            rama_run_state si = states[i];
            rc = rama_q8_forward(c, cfg, w, &si, tokens_host[i], positions_host[i]); if (rc) return rc;
        }
        return 0;
    }
    Q8BatchScratch b{};
    rc = ensure_q8_batch_scratch(c, cfg, w->group_size, &b); if (rc) return rc;
    c->embedded_x = nullptr; c->host_pos = -1;
    rc = stage_tokens(c, b.toks, tokens_host, n_seq, b.seqs, states, positions_host); if (rc) return rc;
    rc = enqueue_q8_batch_pass(c, cfg, w, b, b.toks, b.seqs, n_seq); if (rc) return rc;
    return copy_out_logits(c, states, b.LG, n_seq, cfg->vocab_size);
}

// ---- the same pass CHAINED ON THE DEVICE (the Q8 counterpart of rama_decode_batch_begin / _steps): every sequence's (token, position)
// lives in device memory, a step ends with argmax_batch_kernel or the batched top-p sampler, and -- new here -- a sequence ENDS on its
// own: after `max_new` tokens or on a sampled stop token (kernels.hpp batch_seq_advance).  A finished slot repeats its last forward,
// which rewrites one cache row with the same bits, so the pass needs no mask and one captured graph serves the whole chain: nothing in
// the pass's launch geometry depends on the positions (score rows and attention LDS are sized by seq_len).

// What a chain's step runs on: both scratches and -- sampler_rows > 0 -- the batched sampler's slices for so many rows.  A chain's begin sizes
// them here, outside any capture; at its _steps entry neither grows: whoever grew them since for another shape dropped the step's graph.
static int q8_chain_scratch(rama_ctx* c, const rama_config* cfg, int group_size, int sampler_rows, Q8BatchScratch* b) {
    int rc = ensure_q8_scratch(c, cfg); if (rc) return rc;
    rc = ensure_q8_batch_scratch(c, cfg, group_size, b); if (rc) return rc;
    return sampler_rows > 0 ? ensure_topp_batch(c, sampler_rows, cfg->vocab_size) : 0;
}

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

// a sequence's budget: its own max_new (0: none) within the chain's max_steps
static int q8_chain_limit(const rama_q8_seq_plan* per_seq, int i, int max_steps) {
    return per_seq && per_seq[i].max_new > 0 ? std::min(per_seq[i].max_new, max_steps) : max_steps;
}

int rama_q8_decode_batch_begin(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* states,
                               const int32_t* tokens_host, const int32_t* positions_host, int n_seq, int max_steps,
                               const rama_q8_seq_plan* per_seq) {
    RAMA_ENTER(c);
    // everything is checked before anything of a running chain is touched
    REQUIRE(c && states && tokens_host && positions_host, RAMA_EINVAL, "q8_decode_batch_begin: NULL argument");
    REQUIRE(n_seq >= 1 && n_seq <= kQ8bMaxTok, RAMA_EINVAL, "q8_decode_batch_begin: 1..128 sequences");
    REQUIRE(max_steps >= 1 && max_steps <= (1 << 20), RAMA_EINVAL, "q8_decode_batch_begin: bad max_steps");
    bool sampled = false;
    size_t n_forced_all = 0;
    int cap = 1;
    for (int i = 0; i < n_seq; i++) {
        int rc = q8_check(c, cfg, w, &states[i]); if (rc) return rc;
        REQUIRE(tokens_host[i] >= 0 && tokens_host[i] < cfg->vocab_size, RAMA_EINVAL, "q8_decode_batch_begin: token outside the vocabulary");
        for (int j = 0; j < i; j++)
            REQUIRE(states[j].key_cache != states[i].key_cache && states[j].value_cache != states[i].value_cache, RAMA_EINVAL,
                    "q8_decode_batch_begin: two sequences share a run state");
        if (per_seq) {
            const rama_q8_seq_plan& q = per_seq[i];
            CHECKED(check_sampler("q8_decode_batch_begin", q.temperature, q.topp, q.u));
            REQUIRE(q.n_forced >= 0 && (q.n_forced == 0 || q.forced), RAMA_EINVAL, "q8_decode_batch_begin: bad forced list");
            CHECKED(check_tokens("q8_decode_batch_begin", "forced token outside the vocabulary", q.forced, q.n_forced, cfg->vocab_size));
            REQUIRE(q.max_new >= 0, RAMA_EINVAL, "q8_decode_batch_begin: max_new < 0");
            CHECKED(check_stop_token("q8_decode_batch_begin", q.stop_token, cfg->vocab_size));
            sampled = sampled || q.temperature != 0.0f || q.n_forced > 0;
            n_forced_all += (size_t)q.n_forced;
        }
        const int limit = q8_chain_limit(per_seq, i, max_steps);
        REQUIRE(positions_host[i] >= 0 && positions_host[i] <= cfg->seq_len - limit, RAMA_EINVAL,
                "q8_decode_batch_begin: position + step budget beyond seq_len");
        cap = std::max(cap, limit);
    }
    REQUIRE(q8_batch_ok(cfg), RAMA_EUNSUP, "q8_decode_batch_begin: a shape the Q8 token-batch pass does not take");
    // argmax_batch_kernel reads 16-byte pieces of the logits rows: other vocabulary sizes end their steps in the sampler's launch
    const bool use_sampler = sampled || cfg->vocab_size % 4 != 0;
    REQUIRE(!use_sampler || (cfg->vocab_size > 1 && cfg->vocab_size <= kToppBlock * kToppMaxBlocks), RAMA_EUNSUP,
            sampled ? "q8_decode_batch_begin: a sampled plan needs vocab_size <= 32768" : "q8_decode_batch_begin: vocab_size % 4 != 0 needs vocab_size <= 32768");
    if (set_device(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    auto& qc = c->q8c;
    destroy_graph(qc.cg);
    qc.n_seq = 0; qc.live = false; qc.states.clear();
    // the scratch and the chain's tables: sized here, outside any capture
    Q8BatchScratch b{};
    int rc = q8_chain_scratch(c, cfg, w->group_size, use_sampler ? n_seq : 0, &b); if (rc) return rc;
    if (!qc.toks) {
        HIPCHK(hipMalloc(&qc.toks, sizeof(int) * kQ8bMaxTok)); HIPCHK(hipMalloc(&qc.seqs, sizeof(SeqSlot) * kQ8bMaxTok));
        HIPCHK(hipMalloc(&qc.ends, sizeof(BatchEnds)));
        HIPCHK(hipMalloc(&qc.rows, sizeof(ToppRow) * kQ8bMaxTok));
        HIPCHK(hipHostMalloc(&qc.done, sizeof(int) * kQ8bMaxTok, hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&qc.done_dev), qc.done, 0));
    }
    if (qc.out_cap < cap) {
        hipFree(qc.out); qc.out = nullptr; qc.out_cap = 0;
        if (qc.ring) { hipHostFree(qc.ring); qc.ring = nullptr; }
        HIPCHK(hipMalloc(&qc.out, sizeof(int) * (size_t)kQ8bMaxTok * cap));
        HIPCHK(hipHostMalloc(&qc.ring, sizeof(int) * (size_t)kQ8bMaxTok * cap, hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&qc.ring_dev), qc.ring, 0));
        qc.out_cap = cap;
    }
    memset(qc.ring, 0, sizeof(int) * (size_t)kQ8bMaxTok * qc.out_cap);      // (the stream was drained above: nothing is on its way)
    memset(qc.done, 0, sizeof(int) * kQ8bMaxTok);
    if (qc.forced_cap < n_forced_all) {
        hipFree(qc.forced); qc.forced = nullptr; qc.forced_cap = 0;
        HIPCHK(hipMalloc(&qc.forced, sizeof(int) * n_forced_all));
        qc.forced_cap = n_forced_all;
    }
    rc = stage_tokens(c, qc.toks, tokens_host, n_seq, qc.seqs, states, positions_host); if (rc) return rc;
    static_assert(kQ8bMaxTok <= 128, "BatchEnds holds 128 sequences");
    BatchEnds ends{};
    ends.done = qc.done_dev;
    ToppRow rows[kQ8bMaxTok];
    size_t at = 0;
    for (int i = 0; i < n_seq; i++) {
        ends.limit[i] = q8_chain_limit(per_seq, i, max_steps);
        ends.stop[i] = per_seq ? per_seq[i].stop_token : -1;
        rows[i] = ToppRow{0.0f, 0.9f, 0.0f, 0, nullptr};
        if (!per_seq) continue;
        const rama_q8_seq_plan& q = per_seq[i];
        rows[i] = ToppRow{q.temperature, q.topp, q.u, q.n_forced, q.n_forced ? qc.forced + at : nullptr};
        if (q.n_forced) HIPCHK(hipMemcpy(qc.forced + at, q.forced, sizeof(int) * q.n_forced, hipMemcpyHostToDevice));
        at += (size_t)q.n_forced;
    }
    HIPCHK(hipMemcpy(qc.ends, &ends, sizeof ends, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(qc.rows, rows, sizeof(ToppRow) * n_seq, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(c->stream));
    qc.sampled = use_sampler; qc.cfg = *cfg; qc.w = *w; qc.states.assign(states, states + n_seq);
    qc.max_steps = max_steps; qc.steps_done = 0; qc.n_seq = n_seq; qc.live = true;
    return 0;
}

// one step: the pass over the chain's own tables, then what ends it
static int enqueue_q8_chain_step(rama_ctx* c, const Q8BatchScratch& b) {
    auto& qc = c->q8c;
    const int V = qc.cfg.vocab_size;
    int rc = enqueue_q8_batch_pass(c, &qc.cfg, &qc.w, b, qc.toks, qc.seqs, qc.n_seq); if (rc) return rc;
    if (!qc.sampled) {
        BatchArgmaxParams ap{b.LG, V, qc.toks, qc.seqs, qc.out, qc.out_cap, qc.ring_dev, qc.ends};
        hipLaunchKernelGGL(argmax_batch_kernel, dim3(qc.n_seq), dim3(1024), 0, c->stream, ap);
        LAUNCHCHK();
        return 0;
    }
    ToppBatchParams fin{};
    fin.toks = qc.toks; fin.seqs = qc.seqs; fin.out = qc.out; fin.out_cap = qc.out_cap; fin.ring = qc.ring_dev;
    fin.ends = qc.ends;
    return enqueue_topp_batch(c, qc.rows, qc.n_seq, b.LG, (size_t)V, V, fin);
}

int rama_q8_decode_batch_steps(rama_ctx* c, int n_steps) {
    RAMA_ENTER(c);
    REQUIRE(c && c->q8c.n_seq > 0, RAMA_EINVAL, "q8_decode_batch_steps: call rama_q8_decode_batch_begin first");
    auto& qc = c->q8c;
    REQUIRE(qc.live, RAMA_EINVAL, "q8_decode_batch_steps: the chain's model or one of its run states has been freed");
    REQUIRE(n_steps >= 0 && n_steps <= qc.max_steps - qc.steps_done, RAMA_EINVAL, "q8_decode_batch_steps: more steps than rama_q8_decode_batch_begin allowed for");
    if (set_device(c)) return 1;
    int n_done = 0;
    const int rc = q8_chain_steps(c, qc, qc.sampled ? qc.n_seq : 0, n_steps, [&](const Q8BatchScratch& b) { return enqueue_q8_chain_step(c, b); }, &n_done);
    qc.steps_done += n_done;
    return rc;
}

// What the _tokens and _stats entries of the chains open with: the stream drained, the hand-off words read
static int q8_drain(rama_ctx* c) {
    if (set_device(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return handoff_check(c);
}
// ... and what a _tokens entry ends with: the first min(produced, cap, max_tokens) tokens of a device row, and their number
static int q8_tokens_back(int32_t* out_host, const int* row_dev, int produced, int cap, int max_tokens, int* n) {
    *n = std::min(std::min(produced, cap), max_tokens);
    if (*n > 0) HIPCHK(hipMemcpy(out_host, row_dev, sizeof(int) * *n, hipMemcpyDeviceToHost));
    return 0;
}

int rama_q8_decode_batch_tokens(rama_ctx* c, int32_t* out_host, int max_per_seq, int32_t* n_per_seq) {
    RAMA_ENTER(c);
    REQUIRE(c && out_host && n_per_seq && c->q8c.n_seq > 0 && max_per_seq >= 0, RAMA_EINVAL, "q8_decode_batch_tokens: bad argument");
    auto& qc = c->q8c;
    int rc = q8_drain(c); if (rc) return rc;
    SeqSlot slots[kQ8bMaxTok];
    HIPCHK(hipMemcpy(slots, qc.seqs, sizeof(SeqSlot) * qc.n_seq, hipMemcpyDeviceToHost));
    for (int s_ = 0; s_ < qc.n_seq; s_++) {      // pad: the tokens the sequence has produced
        rc = q8_tokens_back(out_host + (size_t)s_ * max_per_seq, qc.out + (size_t)s_ * qc.out_cap, slots[s_].pad, qc.out_cap, max_per_seq, n_per_seq + s_);
        if (rc) return rc;
    }
    return 0;
}

int rama_q8_decode_batch_stream_poll(rama_ctx* c, int seq, int from, int32_t* out_host, int max_tokens, int* n_ready, int* finished) {
    RAMA_ENTER(c);
    REQUIRE(c && n_ready && c->q8c.n_seq > 0 && c->q8c.ring && seq >= 0 && seq < c->q8c.n_seq && from >= 0 && max_tokens >= 0 && (max_tokens == 0 || out_host),
            RAMA_EINVAL, "q8_decode_batch_stream_poll: bad argument");
    const auto& qc = c->q8c;
    // the finished word first: it is stored after the sequence's last ring word, so a set word means every token is there to be read
    const int fin = __atomic_load_n(qc.done + seq, __ATOMIC_ACQUIRE);
    *n_ready = read_ring(qc.ring + (size_t)seq * qc.out_cap, qc.out_cap, from, out_host, max_tokens);
    if (finished) *finished = fin != 0;
    return 0;
}

// ---- THE SERVING CHAIN (q8_serve.hpp): continuous batching.  n_slots slots share passes of max_rows rows; a scheduler
// launch builds every step's row table from the slot table on the device, a pick launch runs the slots' state machine, and an admission
// is a stream-ordered copy + launch between two steps.  Nothing in a step's launch geometry depends on a sequence, so one captured graph
// serves the chain for its whole life.

// the scheduling rule on the host: the rows every slot gets in the next step (serve_schedule_kernel computes the same numbers by scans)
static void serve_plan_counts(const rama_q8_serve_slot* slots, int n_slots, int max_rows, int* nrows) {
    int left = max_rows;
    for (int i = 0; i < n_slots; i++) {
        nrows[i] = slots[i].state == RAMA_SERVE_DECODE || slots[i].state == RAMA_SERVE_PROMPT ? 1 : 0;
        left -= nrows[i];
    }
    for (int i = 0; i < n_slots && left > 0; i++) {
        if (slots[i].state != RAMA_SERVE_PROMPT) continue;
        const int extra = std::min(slots[i].n_context - slots[i].cursor - 1, left);
        nrows[i] += extra;
        left -= extra;
    }
}

int rama_q8_serve_plan_step(const rama_q8_serve_slot* slots, int n_slots, int max_rows, rama_q8_serve_row* rows_out, rama_q8_serve_slot* slots_after) {
    REQUIRE(slots && rows_out, RAMA_EINVAL, "q8_serve_plan_step: NULL argument");
    CHECKED(check_slots_rows("q8_serve_plan_step", n_slots, max_rows));
    for (int i = 0; i < n_slots; i++) CHECKED(check_plan_slot("q8_serve_plan_step", slots[i]));
    int nrows[kServeMaxSlots];
    serve_plan_counts(slots, n_slots, max_rows, nrows);
    int r = 0;
    for (int i = 0; i < n_slots; i++) {
        const rama_q8_serve_slot& s = slots[i];
        const bool lg = s.state == RAMA_SERVE_DECODE || (s.state == RAMA_SERVE_PROMPT && s.cursor + nrows[i] == s.n_context);
        for (int k = 0; k < nrows[i]; k++) rows_out[r++] = rama_q8_serve_row{i, s.cursor + k, lg && k == nrows[i] - 1 ? 1 : 0};
        if (!slots_after) continue;
        rama_q8_serve_slot a = s;
        if (nrows[i]) {
            a.cursor = s.cursor + nrows[i];
            if (lg) {
                a.n_out = s.n_out + 1;
                a.state = a.n_out >= s.max_new ? RAMA_SERVE_DONE : RAMA_SERVE_DECODE;
            }
        }
        slots_after[i] = a;
    }
    for (; r < max_rows; r++) rows_out[r] = rama_q8_serve_row{-1, -1, 0};
    return 0;
}

// the same rule with the third class (serve_spec_schedule_kernel computes the same numbers by scans): what the prompts leave goes to the
// DECODE slots' drafts, in ascending slot index
int rama_q8_serve_spec_plan_step(const rama_q8_serve_slot* slots, int n_slots, int max_rows, const int32_t* want, rama_q8_serve_row* rows_out,
                                 int32_t* granted_out) {
    REQUIRE(slots && want && rows_out && granted_out, RAMA_EINVAL, "q8_serve_spec_plan_step: NULL argument");
    CHECKED(check_slots_rows("q8_serve_spec_plan_step", n_slots, max_rows));
    for (int i = 0; i < n_slots; i++) {
        const rama_q8_serve_slot& s = slots[i];
        CHECKED(check_plan_slot("q8_serve_spec_plan_step", s));
        REQUIRE(want[i] >= 0 && want[i] <= kSpecMaxDraft, RAMA_EINVAL, "q8_serve_spec_plan_step: a slot wants 0..15 drafts");
        REQUIRE(want[i] == 0 || (s.state == RAMA_SERVE_DECODE && want[i] <= s.max_new - s.n_out - 1), RAMA_EINVAL,
                "q8_serve_spec_plan_step: only a DECODE slot drafts, and at most max_new - n_out - 1 tokens");
    }
    int nrows[kServeMaxSlots];
    serve_plan_counts(slots, n_slots, max_rows, nrows);
    int left = max_rows;
    for (int i = 0; i < n_slots; i++) left -= nrows[i];
    for (int i = 0; i < n_slots; i++) {
        granted_out[i] = std::min(want[i], left);
        left -= granted_out[i];
    }
    int r = 0;
    for (int i = 0; i < n_slots; i++) {
        const rama_q8_serve_slot& s = slots[i];
        const bool dec = s.state == RAMA_SERVE_DECODE;
        for (int k = 0; k < nrows[i] + granted_out[i]; k++)
            rows_out[r++] = rama_q8_serve_row{i, s.cursor + k, dec || s.cursor + k == s.n_context - 1 ? 1 : 0};
    }
    for (; r < max_rows; r++) rows_out[r] = rama_q8_serve_row{-1, -1, 0};
    return 0;
}

int rama_q8_serve_end(rama_ctx* c) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "q8_serve_end: ctx is NULL");
    if (!c->q8s.n_slots && !c->q8s.blob) return 0;
    if (set_device(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    serve_release(c);
    return 0;
}

// rama_q8_serve_begin (spec false) and rama_q8_serve_begin_spec: the latter sizes the drafting tables as well, and its sampler for max_rows rows
// draft_rows > 0 (rama_q8_serve_begin_model): the sampler is sized for the first draft pass's rows as well
static int serve_begin(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, int n_slots, int max_rows, int max_new_cap, bool spec,
                       int n_draft_cap, int hint_cap, int draft_rows = 0) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    int rc = check_cfg(cfg); if (rc) return rc;
    REQUIRE(w && w->group_size > 0 && cfg->dim % w->group_size == 0 && cfg->hidden_dim % w->group_size == 0, RAMA_EINVAL,
            "q8_serve_begin: group_size must divide dim and hidden_dim");
    REQUIRE(q8_weights_complete(w), RAMA_EINVAL, "q8_serve_begin: missing weights");
    CHECKED(check_slots_rows("q8_serve_begin", n_slots, max_rows));
    REQUIRE(max_new_cap >= 1 && max_new_cap <= cfg->seq_len - 1, RAMA_EINVAL, "q8_serve_begin: max_new_cap outside [1, seq_len - 1]");
    REQUIRE(q8_batch_ok(cfg), RAMA_EUNSUP, "q8_serve_begin: a shape the Q8 token-batch pass does not take");
    const int V = cfg->vocab_size;
    const bool sampler = V > 1 && V <= kToppBlock * kToppMaxBlocks;
    REQUIRE(sampler || V % 4 == 0, RAMA_EUNSUP, "q8_serve_begin: vocab_size % 4 != 0 needs vocab_size <= 32768");
    CHECKED(check_spec_caps("q8_serve_begin_spec", n_draft_cap, hint_cap));
    if (set_device(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    serve_release(c);
    // the scratch (a spec chain picks per row) and the chain's tables: sized here, outside any capture
    Q8BatchScratch b{};
    rc = q8_chain_scratch(c, cfg, w->group_size, sampler ? std::max(spec ? max_rows : n_slots, draft_rows) : 0, &b); if (rc) return rc;
    auto& sv = c->q8s;
    rc = serve_state_alloc_spec(c, sv, cfg->seq_len, n_slots, max_rows, max_new_cap, spec, n_draft_cap, hint_cap); if (rc) return rc;
    sv.cfg = *cfg; sv.w = *w; sv.sampler = sampler;
    sv.captures = 0;
    sv.live = true;
    return 0;
}

// a drafting chain's two caps, in the calling entry's words
int check_spec_caps(const char* entry, int n_draft_cap, int hint_cap) {
    REFUSE_UNLESS(n_draft_cap >= 0 && n_draft_cap <= kSpecMaxDraft, entry, "n_draft_cap outside 0..15");
    REFUSE_UNLESS(hint_cap >= 0 && hint_cap < kSpecHintBit, entry, "hint_cap outside [0, 2^30)");
    return 0;
}

int serve_state_alloc_spec(rama_ctx* c, rama_ctx::ServeState& sv, int seq_len, int n_slots, int max_rows, int max_new_cap, bool spec, int n_draft_cap, int hint_cap) {
    ServeSpecTables& st = sv.st;
    const size_t N = (size_t)n_slots, H = (size_t)hint_cap;
    struct More { ServeSpecTables* st; size_t N, R, H; bool spec; } more{&st, N, (size_t)max_rows, H, spec};
    const int rc = serve_state_alloc(c, sv, seq_len, n_slots, max_rows, max_new_cap, [](BlobCarver& bc, void* arg) {
        const More& m = *static_cast<const More*>(arg);
        if (!m.spec) return;      // the drafting tables: nothing of them on a chain begun without drafts
        ServeSpecTables& st = *m.st;
        bc.take(st.ss, m.N); bc.take(st.hint, m.N * m.H); bc.take(st.picks, m.R); bc.take(st.lflag, m.R); bc.take(st.rrow, m.R); bc.take(st.sums, m.N);
        bc.take(st.sched, 2);
    }, &more);
    if (rc) return rc;
    if (spec) {
        sv.srec_bytes = (sizeof(ServeSpecSlot) + H * sizeof(int) + 255) / 256 * 256;
        HIPCHK(hipMalloc(&sv.sstage, N * sv.srec_bytes));
        HIPCHK(hipHostMalloc(&sv.spinned, N * sv.srec_bytes, hipHostMallocDefault));
        st.hint_cap = hint_cap;
    }
    sv.spec = spec; sv.n_draft_cap = n_draft_cap; sv.hint_cap = hint_cap;
    return 0;
}

int serve_state_alloc(rama_ctx* c, rama_ctx::ServeState& sv, int seq_len, int n_slots, int max_rows, int max_new_cap, void (*more)(BlobCarver&, void*), void* arg) {
    ServeTables& t = sv.t;
    const size_t S = (size_t)seq_len, N = (size_t)n_slots, R = (size_t)max_rows, cap = (size_t)max_new_cap;
    auto lay = [&](char* base) {
        BlobCarver bc{base};
        bc.take(t.slots, N); bc.take(t.ctx, N * S); bc.take(t.rows, R); bc.take(t.row_tok, R); bc.take(t.nrows, N); bc.take(t.lrow, N);
        bc.take(t.trow, N); bc.take(t.counters, 4); bc.take(t.out, N * cap);
        if (more) more(bc, arg);
        return bc.used;
    };
    const size_t need = lay(nullptr);
    HIPCHK(hipMalloc(&sv.blob, need));
    HIPCHK(hipMemsetAsync(sv.blob, 0, need, c->stream));          // every slot FREE, the counters 0
    lay(sv.blob);
    sv.rec_bytes = (sizeof(ServeSlot) + S * sizeof(int) + 255) / 256 * 256;
    HIPCHK(hipMalloc(&sv.stage, N * sv.rec_bytes));
    HIPCHK(hipHostMalloc(&sv.pinned, N * sv.rec_bytes, hipHostMallocDefault));
    HIPCHK(hipHostMalloc(&sv.ring, sizeof(int) * N * cap, hipHostMallocMapped));
    HIPCHK(hipHostMalloc(&sv.done, sizeof(int) * N, hipHostMallocMapped));
    memset(sv.ring, 0, sizeof(int) * N * cap);
    memset(sv.done, 0, sizeof(int) * N);
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&t.ring), sv.ring, 0));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&t.done), sv.done, 0));
    t.seq_len = seq_len; t.n_slots = n_slots; t.max_rows = max_rows; t.out_cap = max_new_cap;
    HIPCHK(hipStreamSynchronize(c->stream));
    sv.states.assign(N, rama_run_state{}); sv.occupied.assign(N, 0); sv.gen.assign(N, 0);
    sv.steps = 0;
    sv.max_rows = max_rows; sv.out_cap = max_new_cap; sv.n_slots = n_slots;
    return 0;
}

int rama_q8_serve_begin(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, int n_slots, int max_rows, int max_new_cap) {
    return serve_begin(c, cfg, w, n_slots, max_rows, max_new_cap, false, 0, 0);
}

int rama_q8_serve_begin_spec(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, int n_slots, int max_rows, int max_new_cap,
                             int n_draft_cap, int hint_cap) {
    return serve_begin(c, cfg, w, n_slots, max_rows, max_new_cap, true, n_draft_cap, hint_cap);
}

// the slot's occupant is still on the device's hands: admitted, and its finished word not yet set
bool serve_slot_live(const rama_ctx::ServeState& sv, int slot) {
    return sv.occupied[slot] && !__atomic_load_n(sv.done + slot, __ATOMIC_ACQUIRE);
}
bool serve_state_uses(rama_ctx::ServeState& sv, const rama_run_state* s) {
    bool uses = false;
    for (int i = 0; i < sv.n_slots; i++) {
        const bool drafts_on = sv.model && sv.dstates[i].key_cache && sv.dstates[i].key_cache == s->key_cache;      // (a slot's draft run state counts as its own)
        if (!sv.occupied[i] || (sv.states[i].key_cache != s->key_cache && !drafts_on)) continue;
        if (__atomic_load_n(sv.done + i, __ATOMIC_ACQUIRE)) { sv.occupied[i] = 0; continue; }
        uses = true;
    }
    return uses;
}

// ---- an admission, for either serving chain (ctx.hpp): the refusals in the calling entry's words, then the install
static int refuse_as(int code, const char* entry, const char* what, int line) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", entry, what);
    return fail(code, msg, __FILE__, line);
}
#define ADMIT_UNLESS(cond, what) do { if (!(cond)) return refuse_as(RAMA_EINVAL, names.admit, (what), __LINE__); } while (0)
static const ServeNames kQ8ServeNames{"q8_serve_admit", "q8_serve_admit_at", "rama_q8_serve_begin", "q8_serve_admit_spec", "rama_q8_serve_begin_spec"};
int serve_admit_head(const ServeNames& names, const rama_ctx::ServeState& sv, bool live, int slot, const rama_run_state* state, const int32_t* context_host,
                     const rama_q8_serve_plan* plan) {
    // everything is checked before anything of the running chain is touched
    ADMIT_UNLESS(live, "the chain's model or the run state of an occupied slot has been freed");
    ADMIT_UNLESS(state && context_host && plan, "NULL argument");
    ADMIT_UNLESS(slot >= 0 && slot < sv.n_slots, "no such slot");
    return 0;
}
int serve_admit_tail(const ServeNames& names, const rama_ctx::ServeState& sv, const rama_config& cfg, int slot, const rama_run_state* state, const int32_t* context_host,
                     int n_context, int n_cached, const rama_q8_serve_plan* plan) {
    ADMIT_UNLESS(!serve_slot_live(sv, slot), "the slot is busy");
    const int V = cfg.vocab_size;
    ADMIT_UNLESS(n_context >= 1, "n_context < 1");
    if (!(n_cached >= 0 && n_cached <= n_context - 1))
        return refuse_as(RAMA_EINVAL, names.admit_at, "n_cached outside [0, n_context - 1] (the final context position is always fed)", __LINE__);
    ADMIT_UNLESS(plan->max_new >= 1, "max_new < 1");
    if (plan->max_new > sv.out_cap) {
        char what[96];
        snprintf(what, sizeof what, "max_new beyond %s's max_new_cap", names.begin);
        return refuse_as(RAMA_EINVAL, names.admit, what, __LINE__);
    }
    ADMIT_UNLESS(n_context <= cfg.seq_len - plan->max_new, "n_context + max_new beyond seq_len");
    CHECKED(check_tokens(names.admit, "token outside the vocabulary", context_host, n_context, V));
    CHECKED(check_sampler(names.admit, plan->temperature, plan->topp, plan->u));
    CHECKED(check_stop_token(names.admit, plan->stop_token, V));
    for (int j = 0; j < sv.n_slots; j++)
        ADMIT_UNLESS(j == slot || !serve_slot_live(sv, j) || (sv.states[j].key_cache != state->key_cache && sv.states[j].value_cache != state->value_cache),
                     "the run state is already in a live slot");
    if (!(plan->temperature == 0.0f || sv.sampler)) return refuse_as(RAMA_EUNSUP, names.admit, "a sampled plan needs vocab_size <= 32768", __LINE__);
    return 0;
}
int serve_admit_install(rama_ctx* c, rama_ctx::ServeState& sv, int slot, const rama_run_state* state, const int32_t* context_host, int n_context, int n_cached,
                        const rama_q8_serve_plan* plan) {
    // the slot's own pinned record: its previous copy has run (the occupant it installed has finished, or there was none)
    char* rec = sv.pinned + (size_t)slot * sv.rec_bytes;
    ServeSlot h{};
    h.kc = state->key_cache; h.vc = state->value_cache;
    h.state = kServePrompt; h.n_ctx = n_context; h.cursor = n_cached; h.tok = 0; h.n_out = 0;
    h.max_new = plan->max_new; h.stop = plan->stop_token; h.gen = sv.gen[slot] + 1;
    h.temperature = plan->temperature; h.topp = plan->topp; h.u = plan->u;
    memcpy(rec, &h, sizeof h);
    memcpy(rec + sizeof h, context_host, sizeof(int) * (size_t)n_context);
    // (the device writes neither again for the previous occupant: it is DONE)
    memset(sv.ring + (size_t)slot * sv.out_cap, 0, sizeof(int) * (size_t)sv.out_cap);
    __atomic_store_n(sv.done + slot, 0, __ATOMIC_RELEASE);
    char* dst = sv.stage + (size_t)slot * sv.rec_bytes;
    HIPCHK(hipMemcpyAsync(dst, rec, sizeof h + sizeof(int) * (size_t)n_context, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(serve_install_kernel, dim3(1), dim3(256), 0, c->stream, sv.t, slot, reinterpret_cast<const ServeSlot*>(dst));
    LAUNCHCHK();
    return 0;
}
// rama_q8_serve_cancel and rama_serve_cancel behind RAMA_ENTER: everything is checked first, then one launch of serve_cancel_kernel for the slots
// still on the device's hands -- stream-ordered, no synchronisation, no staging copy (the set travels as launch arguments), the captured step
// untouched.  A slot never admitted, or one whose finished word the host can see, is skipped; nothing left: nothing launched.  The host's books
// (occupied, gen) do not change: as with any finish, the slot is admissible once the host sees the word.  A drafting chain needs no more than this:
// the draft, open, schedule, accept and close kernels key on the slot's state.
int serve_cancel(rama_ctx* c, const char* entry, rama_ctx::ServeState& sv, const int32_t* slots, int n) {
    REFUSE_UNLESS(sv.n_slots > 0, entry, "no serving chain");
    REFUSE_UNLESS(n >= 0 && n <= kServeMaxSlots, entry, "n outside [0, 128]");
    REFUSE_UNLESS(n == 0 || slots, entry, "NULL argument");
    for (int k = 0; k < n; k++) REFUSE_UNLESS(slots[k] >= 0 && slots[k] < sv.n_slots, entry, "no such slot");
    unsigned long long mask[2] = {0ull, 0ull};
    for (int k = 0; k < n; k++)
        if (serve_slot_live(sv, slots[k])) mask[slots[k] >> 6] |= 1ull << (slots[k] & 63);
    if (!(mask[0] | mask[1])) return 0;
    if (set_device(c)) return 1;
    hipLaunchKernelGGL(serve_cancel_kernel, dim3(1), dim3(kServeMaxSlots), 0, c->stream, sv.t, mask[0], mask[1]);
    LAUNCHCHK();
    sv.cancel_launches++;
    return 0;
}
// A hook for the tests, exported like the other rama_internal_* accessors and not in the header: the serve_cancel_kernel launches since the chain began, of the
// context's Q8 chain (fp32 == 0) or fp32 chain -- tests/test_hip_serve_cancel.py sees that a cancel with nothing left to cancel launches nothing
extern "C" long long rama_internal_serve_cancel_launches(rama_ctx* c, int fp32) {
    if (!c) return -1;
    return (long long)(fp32 ? static_cast<const rama_ctx::ServeState&>(c->sv) : static_cast<const rama_ctx::ServeState&>(c->q8s)).cancel_launches;
}
int rama_q8_serve_cancel(rama_ctx* c, const int32_t* slots, int n) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "q8_serve_cancel: ctx is NULL");
    return serve_cancel(c, "q8_serve_cancel", c->q8s, slots, n);
}

int serve_admit_spec_check(const ServeNames& names, const rama_ctx::ServeState& sv, int vocab_size, const rama_q8_serve_spec* spec) {
    if (!spec) return 0;
    char what[3][112];
    snprintf(what[0], sizeof what[0], "the chain was not begun with %s", names.begin_spec);
    snprintf(what[1], sizeof what[1], "n_draft beyond %s's n_draft_cap", names.begin_spec);
    snprintf(what[2], sizeof what[2], "bad hint, or one beyond %s's hint_cap", names.begin_spec);
    REFUSE_UNLESS(sv.spec, names.admit_spec, what[0]);
    return check_drafting(names.admit_spec, *spec, sv.n_draft_cap, what[1], sv.hint_cap, what[2], vocab_size);
}
int serve_admit_spec_install(rama_ctx* c, rama_ctx::ServeState& sv, int slot, const rama_q8_serve_spec* spec) {
    if (!sv.spec) return 0;
    // the same way as serve_admit_install, the slot's own pinned spec record
    char* srec = sv.spinned + (size_t)slot * sv.srec_bytes;
    ServeSpecSlot g{};
    g.n_draft = spec ? spec->n_draft : 0; g.ngram = spec ? spec->ngram : 1; g.n_hint = spec ? spec->n_hint : 0;
    memcpy(srec, &g, sizeof g);
    if (g.n_hint) memcpy(srec + sizeof g, spec->hint, sizeof(int) * (size_t)g.n_hint);
    char* sdst = sv.sstage + (size_t)slot * sv.srec_bytes;
    HIPCHK(hipMemcpyAsync(sdst, srec, sizeof g + sizeof(int) * (size_t)g.n_hint, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(serve_spec_install_kernel, dim3(1), dim3(256), 0, c->stream, sv.st, slot, reinterpret_cast<const ServeSpecSlot*>(sdst));
    LAUNCHCHK();
    return 0;
}

// a chain begun with an _begin_model entry: `s` shares a cache with the draft run state of a live slot other than `slot`
bool serve_model_state_clash(const rama_ctx::ServeState& sv, int slot, const rama_run_state* s) {
    for (int j = 0; j < sv.n_slots; j++) {
        const rama_run_state& d = sv.dstates[j];
        if (j == slot || !serve_slot_live(sv, j) || !d.key_cache) continue;
        if (d.key_cache == s->key_cache || d.value_cache == s->value_cache) return true;
    }
    return false;
}

// rama_q8_serve_admit (n_cached 0) and rama_q8_serve_admit_at: the slot starts PROMPT at cursor = n_cached, over rows 0 .. n_cached - 1 that
// earlier work on the stream has put into the run state's caches
// spec (rama_q8_serve_admit_spec; a chain begun with rama_q8_serve_begin_spec only): the slot's drafting fields and hint; without it a slot of
// such a chain is admitted with n_draft = 0
static int serve_admit(rama_ctx* c, int slot, const rama_run_state* state, const int32_t* context_host, int n_context, int n_cached,
                       const rama_q8_serve_plan* plan, const rama_q8_serve_spec* spec = nullptr) {
    RAMA_ENTER(c);
    REQUIRE(c && c->q8s.n_slots > 0, RAMA_EINVAL, "q8_serve_admit: call rama_q8_serve_begin first");
    auto& sv = c->q8s;
    CHECKED(serve_admit_head(kQ8ServeNames, sv, sv.live, slot, state, context_host, plan));
    int rc = q8_check(c, &sv.cfg, &sv.w, state); if (rc) return rc;
    CHECKED(serve_admit_tail(kQ8ServeNames, sv, sv.cfg, slot, state, context_host, n_context, n_cached, plan));
    CHECKED(serve_admit_spec_check(kQ8ServeNames, sv, sv.cfg.vocab_size, spec));
    if (sv.model) {      // a chain begun with rama_q8_serve_begin_model: no lookup drafts, and no run state that a live slot drafts on
        REFUSE_UNLESS(!spec, "q8_serve_admit_spec", "the chain was begun with rama_q8_serve_begin_model: model drafts replace the lookup");
        REFUSE_UNLESS(!serve_model_state_clash(sv, slot, state), "q8_serve_admit", "the run state is already in a live slot");
    }
    if (set_device(c)) return 1;
    rc = serve_admit_install(c, sv, slot, state, context_host, n_context, n_cached, plan); if (rc) return rc;
    rc = serve_admit_spec_install(c, sv, slot, spec); if (rc) return rc;
    sv.states[slot] = *state; sv.occupied[slot] = 1; sv.gen[slot]++;
    if (sv.model) sv.dstates[slot] = rama_run_state{};
    return 0;
}

int rama_q8_serve_admit(rama_ctx* c, int slot, const rama_run_state* state, const int32_t* context_host, int n_context, const rama_q8_serve_plan* plan) {
    return serve_admit(c, slot, state, context_host, n_context, 0, plan);
}

int rama_q8_serve_admit_at(rama_ctx* c, int slot, const rama_run_state* state, const int32_t* context_host, int n_context, int n_cached,
                           const rama_q8_serve_plan* plan) {
    return serve_admit(c, slot, state, context_host, n_context, n_cached, plan);
}

int rama_q8_serve_admit_spec(rama_ctx* c, int slot, const rama_run_state* state, const int32_t* context_host, int n_context, int n_cached,
                             const rama_q8_serve_plan* plan, const rama_q8_serve_spec* spec) {
    REQUIRE(spec, RAMA_EINVAL, "q8_serve_admit_spec: NULL argument");
    return serve_admit(c, slot, state, context_host, n_context, n_cached, plan, spec);
}

// ---- MODEL DRAFTS INSIDE THE SERVING CHAIN (q8_serve_model.hpp): rama_q8_serve_begin_spec with hint_cap 0, plus a draft model
// whose passes run on a batch scratch of their own; a slot is admitted with a draft run state and drafts with that model instead of the lookup

// what an _begin_model entry refuses of the draft model and the geometry, in the entry's words (before anything is allocated)
int serve_model_begin_check(const char* entry, const rama_config* cfg, const rama_config* dcfg, const rama_q8_weights* dw, int n_slots, int max_rows, int n_draft_cap) {
    REFUSE_UNLESS(dw && dw->group_size > 0 && dcfg->dim % dw->group_size == 0 && dcfg->hidden_dim % dw->group_size == 0, entry,
                  "the draft model's group_size must divide its dim and hidden_dim");
    REFUSE_UNLESS(q8_weights_complete(dw), entry, "missing draft weights");
    REFUSE_UNLESS(dcfg->vocab_size == cfg->vocab_size, entry, "the draft model's vocabulary is not the target's");
    REFUSE_UNLESS(n_draft_cap >= 1 && n_draft_cap <= kSpecMaxDraft, entry, "n_draft_cap outside 1..15");
    CHECKED(check_slots_rows(entry, n_slots, max_rows));
    REFUSE_UNLESS(2 * n_slots <= kQ8bMaxTok, entry, "2 n_slots > 128 (the first draft pass carries up to two rows per slot)");
    UNSUPPORTED_UNLESS(q8_batch_ok(dcfg), entry, "a draft model of a shape the Q8 token-batch pass does not take");
    return 0;
}

// The draft side of a chain whose tables serve_state_alloc_spec has made: the context's two Q8 scratches for the draft's shape (what a draft-model
// prefill between two steps runs on: sized here, outside any capture), then what the draft passes themselves run on -- a batch scratch of 2 n_slots rows
// and the draft tables, both the chain's own.  The caller frees a half-made state (serve_state_free).
int serve_model_alloc(rama_ctx* c, rama_ctx::ServeState& sv, const rama_config* dcfg, const rama_q8_weights* dw) {
    const int n_slots = sv.n_slots, draft_rows = 2 * n_slots;
    Q8BatchScratch b{};
    int r = ensure_q8_scratch(c, dcfg); if (r) return r;
    r = ensure_q8_batch_scratch(c, dcfg, dw->group_size, &b); if (r) return r;
    Q8BatchScratch db{};
    const size_t dneed = q8_batch_scratch_lay(dcfg, dw->group_size, (size_t)draft_rows, nullptr, &db);
    HIPCHK(hipMalloc(&sv.dblob, dneed));
    HIPCHK(hipMemset(sv.dblob, 0, dneed));
    ServeModelTables& m = sv.mt;
    const size_t N = (size_t)n_slots;
    auto lay = [&](char* base) {
        BlobCarver bc{base};
        bc.take(m.ms, N); bc.take(m.rows0, 2 * N); bc.take(m.row_tok0, 2 * N); bc.take(m.trow0, 2 * N);
        bc.take(m.rows, N); bc.take(m.row_tok, N); bc.take(m.trow, N);
        return bc.used;
    };
    const size_t need = lay(nullptr);
    HIPCHK(hipMalloc(&sv.mblob, need));
    HIPCHK(hipMemset(sv.mblob, 0, need));
    lay(sv.mblob);
    sv.model = true; sv.dcfg = *dcfg; sv.dw = *dw; sv.draft_rows = draft_rows;
    sv.dstates.assign(N, rama_run_state{});
    return 0;
}

int rama_q8_serve_begin_model(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_config* dcfg, const rama_q8_weights* dw,
                              int n_slots, int max_rows, int max_new_cap, int n_draft_cap) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "ctx is NULL");
    int rc = check_cfg(cfg); if (rc) return rc;
    rc = check_cfg(dcfg); if (rc) return rc;
    CHECKED(serve_model_begin_check("q8_serve_begin_model", cfg, dcfg, dw, n_slots, max_rows, n_draft_cap));
    rc = serve_begin(c, cfg, w, n_slots, max_rows, max_new_cap, true, n_draft_cap, 0, 2 * n_slots); if (rc) return rc;
    // everything a draft pass, and a draft-model prefill between two steps, runs on: sized here, outside any capture, so that neither regrows a
    // buffer the captured step holds -- both scratches of the context for the larger of the two shapes, the draft passes' own for 2 n_slots rows
    rc = serve_model_alloc(c, c->q8s, dcfg, dw);
    Q8BatchScratch b{};
    if (!rc) rc = q8_chain_scratch(c, cfg, w->group_size, 0, &b);
    if (rc) { serve_release(c); return rc; }
    return 0;
}

static const ServeNames kQ8ServeModelNames{"q8_serve_admit_model", "q8_serve_admit_model", "rama_q8_serve_begin_model", "q8_serve_admit_model",
                                           "rama_q8_serve_begin_model"};

// an _admit_model entry's refusals behind serve_admit_tail, in its words (names.admit_spec; names.begin_spec is its _begin_model entry) ...
int serve_admit_model_check(const ServeNames& names, const rama_ctx::ServeState& sv, int slot, const rama_run_state* state, const rama_run_state* dstate,
                            int n_context, const rama_q8_serve_plan* plan, int n_draft) {
    const char* entry = names.admit_spec;
    char what[2][112];
    snprintf(what[0], sizeof what[0], "n_draft beyond %s's n_draft_cap", names.begin_spec);
    REFUSE_UNLESS(n_draft >= 0 && n_draft <= sv.n_draft_cap, entry, what[0]);
    REFUSE_UNLESS(n_context <= sv.dcfg.seq_len - plan->max_new, entry, "n_context + max_new beyond the draft model's seq_len");
    REFUSE_UNLESS(dstate->key_cache != state->key_cache && dstate->value_cache != state->value_cache, entry, "the draft run state is the target's");
    for (int j = 0; j < sv.n_slots; j++)
        REFUSE_UNLESS(j == slot || !serve_slot_live(sv, j) || (sv.states[j].key_cache != dstate->key_cache && sv.states[j].value_cache != dstate->value_cache),
                      entry, "the draft run state is already in a live slot");
    REFUSE_UNLESS(!serve_model_state_clash(sv, slot, dstate) && !serve_model_state_clash(sv, slot, state), entry, "a run state is already a live slot's draft state");
    return 0;
}
// ... the draft run state against the draft model (where the entry checks the target's against its own) ...
int serve_admit_model_dstate(rama_ctx* c, const rama_ctx::ServeState& sv, const rama_run_state* dstate) { return q8_check(c, &sv.dcfg, &sv.dw, dstate); }
// ... and the drafting half of the install, behind serve_admit_install: the slot's n_draft, and its draft cursor -- rows 0 .. n_context - 1 of the draft
// cache hold the whole context (the caller's contract)
int serve_admit_model_install(rama_ctx* c, rama_ctx::ServeState& sv, int slot, const rama_run_state* dstate, int n_context, int n_draft) {
    const rama_q8_serve_spec spec{n_draft, 1, nullptr, 0};
    const int rc = serve_admit_spec_install(c, sv, slot, &spec); if (rc) return rc;
    hipLaunchKernelGGL(serve_model_install_kernel, dim3(1), dim3(64), 0, c->stream, sv.mt, slot, dstate->key_cache, dstate->value_cache, n_context);
    LAUNCHCHK();
    return 0;
}

int rama_q8_serve_admit_model(rama_ctx* c, int slot, const rama_run_state* state, const rama_run_state* dstate, const int32_t* context_host,
                              int n_context, int n_cached, const rama_q8_serve_plan* plan, int n_draft) {
    RAMA_ENTER(c);
    const char* entry = "q8_serve_admit_model";
    REQUIRE(c && c->q8s.n_slots > 0 && c->q8s.model, RAMA_EINVAL, "q8_serve_admit_model: call rama_q8_serve_begin_model first");
    auto& sv = c->q8s;
    CHECKED(serve_admit_head(kQ8ServeModelNames, sv, sv.live, slot, state, context_host, plan));
    REFUSE_UNLESS(dstate, entry, "NULL argument");
    int rc = q8_check(c, &sv.cfg, &sv.w, state); if (rc) return rc;
    rc = serve_admit_model_dstate(c, sv, dstate); if (rc) return rc;
    CHECKED(serve_admit_tail(kQ8ServeModelNames, sv, sv.cfg, slot, state, context_host, n_context, n_cached, plan));
    CHECKED(serve_admit_model_check(kQ8ServeModelNames, sv, slot, state, dstate, n_context, plan, n_draft));
    if (set_device(c)) return 1;
    rc = serve_admit_install(c, sv, slot, state, context_host, n_context, n_cached, plan); if (rc) return rc;
    rc = serve_admit_model_install(c, sv, slot, dstate, n_context, n_draft); if (rc) return rc;
    sv.states[slot] = *state; sv.dstates[slot] = *dstate; sv.occupied[slot] = 1; sv.gen[slot]++;
    return 0;
}

// the step's schedule on the host: the wants, rama_q8_serve_spec_plan_step's rule over them, and every draft pass's row table
int rama_q8_serve_model_plan_step(const rama_q8_serve_slot* slots, int n_slots, int max_rows, int seq_len, const int32_t* n_draft,
                                  const int32_t* draft_cursor, int n_passes, rama_q8_serve_row* rows_out, int32_t* want_out, int32_t* granted_out,
                                  rama_q8_serve_row* draft_rows_out) {
    REQUIRE(slots && n_draft && draft_cursor && rows_out && want_out && granted_out && draft_rows_out, RAMA_EINVAL, "q8_serve_model_plan_step: NULL argument");
    CHECKED(check_slots_rows("q8_serve_model_plan_step", n_slots, max_rows));
    REQUIRE(2 * n_slots <= kQ8bMaxTok && n_passes >= 1 && n_passes <= kSpecMaxDraft && seq_len >= 1, RAMA_EINVAL,
            "q8_serve_model_plan_step: 2 n_slots <= 128, 1..15 passes");
    for (int i = 0; i < n_slots; i++) {
        const rama_q8_serve_slot& s = slots[i];
        CHECKED(check_plan_slot("q8_serve_model_plan_step", s));
        REQUIRE(n_draft[i] >= 0 && n_draft[i] <= n_passes, RAMA_EINVAL, "q8_serve_model_plan_step: a slot's n_draft outside 0..n_passes");
        const bool dec = s.state == RAMA_SERVE_DECODE && n_draft[i] > 0;
        REQUIRE(!dec || (s.cursor < seq_len && s.cursor - draft_cursor[i] >= 0 && s.cursor - draft_cursor[i] <= 1), RAMA_EINVAL,
                "q8_serve_model_plan_step: a drafting slot's draft cursor is its cursor, or one row behind");
        want_out[i] = dec ? std::max(std::min(n_draft[i], std::min(seq_len - 1 - s.cursor, s.max_new - s.n_out - 1)), 0) : 0;
    }
    CHECKED(rama_q8_serve_spec_plan_step(slots, n_slots, max_rows, want_out, rows_out, granted_out));
    const rama_q8_serve_row idle{-1, -1, 0};
    for (int i = 0; i < n_slots; i++) {
        const rama_q8_serve_slot& s = slots[i];
        const bool dec = s.state == RAMA_SERVE_DECODE && n_draft[i] > 0;
        const int gap = dec ? s.cursor - draft_cursor[i] : -1, g = granted_out[i];
        for (int k = 0; k < 2; k++)      // the first pass: s[Dc..P], fed whatever the grant; the last live row is picked from when g > 0
            draft_rows_out[2 * i + k] = k <= gap ? rama_q8_serve_row{i, draft_cursor[i] + k, k == gap && g > 0 ? 1 : 0} : idle;
        for (int j = 1; j < n_passes; j++)
            draft_rows_out[(size_t)(j + 1) * n_slots + i] = j < g ? rama_q8_serve_row{i, s.cursor + j, 1} : idle;
    }
    return 0;
}

int serve_model_report(rama_ctx* c, const rama_ctx::ServeState& sv, rama_q8_serve_model_report* out) {
    { const int rh = q8_drain(c); if (rh) return rh; }
    std::vector<ServeModelSlot> ms(sv.n_slots);
    HIPCHK(hipMemcpy(ms.data(), sv.mt.ms, sizeof(ServeModelSlot) * sv.n_slots, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->n_slots = sv.n_slots; out->n_draft_cap = sv.n_draft_cap;
    for (int i = 0; i < sv.n_slots; i++) {
        out->draft_passes += ms[i].draft_passes; out->draft_rows_fed += ms[i].draft_rows_fed; out->catch_up_rows += ms[i].catch_up_rows;
        out->draft_cursor[i] = ms[i].Dc;
    }
    return 0;
}

int rama_q8_serve_model_stats(rama_ctx* c, rama_q8_serve_model_report* out) {
    RAMA_ENTER(c);
    REQUIRE(c && out && c->q8s.n_slots > 0 && c->q8s.model, RAMA_EINVAL, "q8_serve_model_stats: no chain begun with rama_q8_serve_begin_model");
    return serve_model_report(c, c->q8s, out);
}

// slot j's occupant runs on a cache of `s`: its target run state, or -- a chain with a draft model -- its draft run state
static bool serve_slot_holds(const rama_ctx::ServeState& sv, int j, const rama_run_state& s) {
    const rama_run_state& t = sv.states[j];
    if (t.key_cache == s.key_cache || t.value_cache == s.value_cache) return true;
    if (!sv.model || !sv.dstates[j].key_cache) return false;
    return sv.dstates[j].key_cache == s.key_cache || sv.dstates[j].value_cache == s.value_cache;
}

// rows [0, n_rows) of every layer of src's caches into every destination's: one launch (q8_fork.hpp), stream-ordered
int rama_q8_kv_fork(rama_ctx* c, const rama_config* cfg, const rama_run_state* src, const rama_run_state* dsts, int n_dst, int n_rows) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "q8_kv_fork: ctx is NULL");
    int rc = check_cfg(cfg); if (rc) return rc;
    REQUIRE(src && dsts, RAMA_EINVAL, "q8_kv_fork: NULL argument");
    REQUIRE(n_dst >= 1 && n_dst <= kForkMaxDst, RAMA_EINVAL, "q8_kv_fork: 1 <= n_dst <= 16");
    REQUIRE(n_rows >= 0 && n_rows <= cfg->seq_len, RAMA_EINVAL, "q8_kv_fork: n_rows outside [0, seq_len]");
    REQUIRE(src->key_cache && src->value_cache, RAMA_EINVAL, "q8_kv_fork: the source has no caches");
    const size_t layer = (size_t)cfg->seq_len * (size_t)cfg->dim, total = layer * (size_t)cfg->n_layers;
    // every cache written must lie clear of the source's and of every other one written
    std::vector<const float*> caches = {src->key_cache, src->value_cache};
    for (int d = 0; d < n_dst; d++) {
        REQUIRE(dsts[d].key_cache && dsts[d].value_cache, RAMA_EINVAL, "q8_kv_fork: a destination has no caches");
        caches.push_back(dsts[d].key_cache); caches.push_back(dsts[d].value_cache);
    }
    for (size_t i = 2; i < caches.size(); i++)
        for (size_t j = 0; j < i; j++)
            REQUIRE(!ranges_overlap(caches[i], total, caches[j], total), RAMA_EINVAL,
                    "q8_kv_fork: a destination shares a cache with the source or with another destination");
    // the Q8 serving chain's slots and the fp32 one's: the fork serves both stacks
    const struct { const rama_ctx::ServeState* sv; const char* what; } chains[2] = {
        {&c->q8s, "q8_kv_fork: a destination is in a live slot of the serving chain"},
        {&c->sv, "q8_kv_fork: a destination is in a live slot of the fp32 serving chain (rama_serve_*)"}};
    for (const auto& ch : chains)
        for (int d = 0; d < n_dst; d++)
            for (int j = 0; j < ch.sv->n_slots; j++)
                REQUIRE(!serve_slot_live(*ch.sv, j) || !serve_slot_holds(*ch.sv, j, dsts[d]), RAMA_EINVAL, ch.what);
    if (n_rows == 0) return 0;
    const size_t span = (size_t)n_rows * (size_t)cfg->dim, reach = layer * (size_t)(cfg->n_layers - 1) + span;
    for (int d = 0; d < n_dst; d++) { RAMA_WRITES(c, dsts[d].key_cache, reach); RAMA_WRITES(c, dsts[d].value_cache, reach); }
    if (set_device(c)) return 1;
    ForkParams p{};
    p.src[0] = src->key_cache; p.src[1] = src->value_cache;
    bool vec = aligned16(p.src[0]) && aligned16(p.src[1]);       // (dim % 4 == 0: a layer and a span are whole 16-byte words)
    for (int d = 0; d < n_dst; d++) {
        p.dst[0][d] = dsts[d].key_cache; p.dst[1][d] = dsts[d].value_cache;
        vec = vec && aligned16(p.dst[0][d]) && aligned16(p.dst[1][d]);
    }
    p.n_dst = n_dst; p.layer_floats = layer; p.n_words = vec ? span / 4 : span;
    const dim3 grid((unsigned)((p.n_words + kForkPiece - 1) / kForkPiece), (unsigned)(2 * cfg->n_layers));
    if (vec) hipLaunchKernelGGL(kv_fork_kernel<true>, grid, dim3(kForkThreads), 0, c->stream, p);
    else hipLaunchKernelGGL(kv_fork_kernel<false>, grid, dim3(kForkThreads), 0, c->stream, p);
    LAUNCHCHK();
    return 0;
}

// q8_serve.hpp's kernels for whoever runs a serving chain's step (ctx.hpp): this translation unit instantiates them
int launch_serve_schedule(rama_ctx* c, const ServeTables& t) {
    hipLaunchKernelGGL(serve_schedule_kernel, dim3(1), dim3(kServeMaxSlots), 0, c->stream, t);
    LAUNCHCHK();
    return 0;
}
int launch_serve_embed(rama_ctx* c, float* X, const float* emb, const ServeTables& t, int dim) {
    hipLaunchKernelGGL(serve_embed_rows_kernel, dim3((dim + 255) / 256, t.max_rows), dim3(256), 0, c->stream, X, emb, (const int*)t.row_tok, (const SeqSlot*)t.rows, dim);
    LAUNCHCHK();
    return 0;
}
int launch_serve_gather(rama_ctx* c, float* XG, const float* X, const ServeTables& t, int dim) {
    hipLaunchKernelGGL(serve_gather_kernel, dim3((dim + 255) / 256, t.n_slots), dim3(256), 0, c->stream, XG, X, (const int*)t.lrow, dim);
    LAUNCHCHK();
    return 0;
}
// the pick over one logits row per slot; `sampled`: the batched sampler's ordering launches over the slots' sampler records go first
int launch_serve_pick(rama_ctx* c, const ServeTables& t, const float* logits, int V, bool sampled) {
    ServePickParams fin{};
    fin.t = t;
    fin.r = PickRows{logits, (size_t)V, V, nullptr, nullptr, nullptr, 0};
    if (sampled) {
        const int rc = enqueue_topp_batch_order(c, t.trow, t.n_slots, logits, (size_t)V, V, nullptr); if (rc) return rc;
        fin.r.keys = c->tb.keys; fin.r.vals = c->tb.vals; fin.r.m = c->tb.m; fin.r.rstride = c->tb.rstride;
    }
    hipLaunchKernelGGL(serve_pick_kernel, dim3(t.n_slots), dim3(1024), 0, c->stream, fin);
    LAUNCHCHK();
    return 0;
}
// ... and q8_serve_spec.hpp's, for the step of either chain with drafts
int launch_serve_draft(rama_ctx* c, const ServeTables& t, const ServeSpecTables& st) {
    hipLaunchKernelGGL(serve_draft_kernel, dim3(t.n_slots), dim3(kServeDraftThreads), 0, c->stream, t, st);
    LAUNCHCHK();
    return 0;
}
int launch_serve_spec_schedule(rama_ctx* c, const ServeTables& t, const ServeSpecTables& st) {
    hipLaunchKernelGGL(serve_spec_schedule_kernel, dim3(1), dim3(kServeMaxSlots), 0, c->stream, t, st);
    LAUNCHCHK();
    return 0;
}
// the pick over one logits row per ROW of the step's table, logits [max_rows, V]; `sampled`: the ordering launches over the rows' sampler records go first
int launch_serve_spec_pick(rama_ctx* c, const ServeTables& t, const ServeSpecTables& st, const float* logits, int V, bool sampled) {
    ServeSpecPickParams fin{};
    fin.t = t; fin.st = st;
    fin.r = PickRows{logits, (size_t)V, V, nullptr, nullptr, nullptr, 0};
    if (sampled) {
        const int rc = enqueue_topp_batch_order(c, st.rrow, t.max_rows, logits, (size_t)V, V, nullptr); if (rc) return rc;
        fin.r.keys = c->tb.keys; fin.r.vals = c->tb.vals; fin.r.m = c->tb.m; fin.r.rstride = c->tb.rstride;
    }
    hipLaunchKernelGGL(serve_spec_pick_kernel, dim3(t.max_rows), dim3(1024), 0, c->stream, fin);
    LAUNCHCHK();
    return 0;
}
int launch_serve_spec_accept(rama_ctx* c, const ServeTables& t, const ServeSpecTables& st) {
    hipLaunchKernelGGL(serve_spec_accept_kernel, dim3(t.n_slots), dim3(64), 0, c->stream, t, st);
    LAUNCHCHK();
    return 0;
}

// one step: the scheduler, the pass over its row table, the logits of the rows that carry them, the pick and the slots' state machine
static int enqueue_q8_serve_step(rama_ctx* c, const Q8BatchScratch& b) {
    auto& sv = c->q8s;
    const rama_config* cfg = &sv.cfg;
    const rama_q8_weights* w = &sv.w;
    int rc = launch_serve_schedule(c, sv.t); if (rc) return rc;
    rc = enqueue_q8_row_layers(c, cfg, w, b, sv.t.row_tok, sv.t.rows, sv.max_rows); if (rc) return rc;
    // the classifier tail for the slots' logits rows only (b.Q is free here)
    rc = launch_serve_gather(c, b.Q, b.X, sv.t, cfg->dim); if (rc) return rc;
    rc = enqueue_q8_classifier(c, cfg, w, b, b.Q, sv.n_slots); if (rc) return rc;
    return launch_serve_pick(c, sv.t, b.LG, cfg->vocab_size, sv.sampler);
}

// one step of a chain begun with rama_q8_serve_begin_spec: the drafts, the scheduler, the pass over its row table, every row's logits, every
// flagged row's pick, the accept rule per slot
static int enqueue_q8_serve_spec_step(rama_ctx* c, const Q8BatchScratch& b) {
    auto& sv = c->q8s;
    int rc = launch_serve_draft(c, sv.t, sv.st); if (rc) return rc;
    rc = launch_serve_spec_schedule(c, sv.t, sv.st); if (rc) return rc;
    rc = enqueue_q8_batch_pass(c, &sv.cfg, &sv.w, b, sv.t.row_tok, sv.t.rows, sv.max_rows); if (rc) return rc;
    rc = launch_serve_spec_pick(c, sv.t, sv.st, b.LG, sv.cfg.vocab_size, sv.sampler); if (rc) return rc;
    return launch_serve_spec_accept(c, sv.t, sv.st);
}

// one step of a chain begun with rama_q8_serve_begin_model (q8_serve_model.hpp): the wants and the first draft pass's rows, the scheduler, n_draft_cap
// passes of the draft model over its own scratch -- 2 n_slots rows, then n_slots -- each ended by the pick that stores every slot's d[j] and sets its
// row of the next pass; then the spec step's pass, picks and accept rule, and the draft cursors
static int enqueue_q8_serve_model_step(rama_ctx* c, const Q8BatchScratch& b) {
    auto& sv = c->q8s;
    int rc = launch_serve_model_drafts(c, sv); if (rc) return rc;
    rc = enqueue_q8_batch_pass(c, &sv.cfg, &sv.w, b, sv.t.row_tok, sv.t.rows, sv.max_rows); if (rc) return rc;
    rc = launch_serve_spec_pick(c, sv.t, sv.st, b.LG, sv.cfg.vocab_size, sv.sampler); if (rc) return rc;
    rc = launch_serve_spec_accept(c, sv.t, sv.st); if (rc) return rc;
    return launch_serve_model_close(c, sv);
}
// q8_serve_model.hpp's kernels and the draft passes for either chain with a draft model (ctx.hpp).  The drafting half of a step: the wants and the first
// draft pass's rows, the scheduler, then n_draft_cap token-batch passes of the draft model over the chain's own scratch (sv.dblob: nothing of the
// context's Q8 scratches, so whoever regrows those moves nothing a captured step holds) -- 2 n_slots rows, then n_slots -- each ended by the sampler's
// ordering launches and the pick that stores every slot's d[j] and sets its row of the next pass
int launch_serve_model_drafts(rama_ctx* c, const rama_ctx::ServeState& sv) {
    Q8BatchScratch db{};
    q8_batch_scratch_lay(&sv.dcfg, sv.dw.group_size, (size_t)sv.draft_rows, sv.dblob, &db);
    hipLaunchKernelGGL(serve_model_open_kernel, dim3(1), dim3(kServeMaxSlots), 0, c->stream, sv.t, sv.st, sv.mt);
    LAUNCHCHK();
    int rc = launch_serve_spec_schedule(c, sv.t, sv.st); if (rc) return rc;
    for (int j = 0; j < sv.n_draft_cap; j++) {
        const int n = j == 0 ? sv.draft_rows : sv.n_slots;
        const int* toks = j == 0 ? sv.mt.row_tok0 : sv.mt.row_tok;
        const SeqSlot* rows = j == 0 ? sv.mt.rows0 : sv.mt.rows;
        rc = enqueue_q8_batch_pass(c, &sv.dcfg, &sv.dw, db, toks, rows, n); if (rc) return rc;
        ServeModelPickParams pk{};
        pk.t = sv.t; pk.st = sv.st; pk.m = sv.mt; pk.j = j;
        rc = enqueue_q8_pick_rows(c, db, sv.dcfg.vocab_size, sv.sampler, j == 0 ? sv.mt.trow0 : sv.mt.trow, n, &pk.r); if (rc) return rc;
        hipLaunchKernelGGL(serve_model_pick_kernel, dim3(sv.n_slots), dim3(1024), 0, c->stream, pk);
        LAUNCHCHK();
    }
    return 0;
}
// ... and what ends the step, behind the accept rule: the draft cursors
int launch_serve_model_close(rama_ctx* c, const rama_ctx::ServeState& sv) {
    hipLaunchKernelGGL(serve_model_close_kernel, dim3(1), dim3(kServeMaxSlots), 0, c->stream, sv.t, sv.st, sv.mt);
    LAUNCHCHK();
    return 0;
}

int rama_q8_serve_steps(rama_ctx* c, int n_steps) {
    RAMA_ENTER(c);
    REQUIRE(c && c->q8s.n_slots > 0, RAMA_EINVAL, "q8_serve_steps: call rama_q8_serve_begin first");
    auto& sv = c->q8s;
    REQUIRE(sv.live, RAMA_EINVAL, "q8_serve_steps: the chain's model or the run state of an occupied slot has been freed");
    REQUIRE(n_steps >= 0, RAMA_EINVAL, "q8_serve_steps: n_steps < 0");
    if (set_device(c)) return 1;
    int n_done = 0;
    const int rc = q8_chain_steps(c, sv, sv.sampler ? std::max(sv.spec ? sv.max_rows : sv.n_slots, sv.draft_rows) : 0, n_steps, [&](const Q8BatchScratch& b) {
        return sv.model ? enqueue_q8_serve_model_step(c, b) : sv.spec ? enqueue_q8_serve_spec_step(c, b) : enqueue_q8_serve_step(c, b);
    }, &n_done);
    sv.steps += (unsigned long long)n_done;
    return rc;
}

// ---- what either serving chain's _poll / _tokens / _stats entry does behind RAMA_ENTER (ctx.hpp)
int serve_poll_ring(const char* entry, const rama_ctx::ServeState& sv, int slot, int from, int32_t* out_host, int max_tokens, int* n_ready, int* finished, int* generation) {
    if (!(n_ready && sv.n_slots > 0 && slot >= 0 && slot < sv.n_slots && from >= 0 && max_tokens >= 0 && (max_tokens == 0 || out_host)))
        return refuse_as(RAMA_EINVAL, entry, "bad argument", __LINE__);
    // the finished word first: it is stored after the occupant's last ring word, so a set word means every token is there to be read
    const int fin = __atomic_load_n(sv.done + slot, __ATOMIC_ACQUIRE);
    *n_ready = read_ring(sv.ring + (size_t)slot * sv.out_cap, sv.out_cap, from, out_host, max_tokens);
    if (finished) *finished = fin;                                 // 0, 1, or RAMA_SERVE_CANCELLED
    if (generation) *generation = sv.gen[slot];
    return 0;
}
int serve_tokens_back(rama_ctx* c, const char* entry, const rama_ctx::ServeState& sv, int slot, int32_t* out_host, int max_tokens, int* n_out) {
    if (!(n_out && sv.n_slots > 0 && slot >= 0 && slot < sv.n_slots && max_tokens >= 0 && (max_tokens == 0 || out_host)))
        return refuse_as(RAMA_EINVAL, entry, "bad argument", __LINE__);
    const int rc = q8_drain(c); if (rc) return rc;
    ServeSlot s{};
    HIPCHK(hipMemcpy(&s, sv.t.slots + slot, sizeof s, hipMemcpyDeviceToHost));
    return q8_tokens_back(out_host, sv.t.out + (size_t)slot * sv.out_cap, s.n_out, sv.out_cap, max_tokens, n_out);
}
// lflag_dev: a chain with drafts flags its logits rows per row; NULL: a slot's logits row is lrow[slot]
int serve_report(rama_ctx* c, const rama_ctx::ServeState& sv, unsigned long long captures, const int* lflag_dev, rama_q8_serve_report* out) {
    { const int rh = q8_drain(c); if (rh) return rh; }
    memset(out, 0, sizeof *out);
    unsigned long long cnt[4];
    ServeSlot slots[kServeMaxSlots];
    SeqSlot rows[kQ8bMaxTok];
    int lrow[kServeMaxSlots], lflag[kQ8bMaxTok];
    if (lflag_dev) HIPCHK(hipMemcpy(lflag, lflag_dev, sizeof(int) * sv.max_rows, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cnt, sv.t.counters, sizeof cnt, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(slots, sv.t.slots, sizeof(ServeSlot) * sv.n_slots, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rows, sv.t.rows, sizeof(SeqSlot) * sv.max_rows, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lrow, sv.t.lrow, sizeof(int) * sv.n_slots, hipMemcpyDeviceToHost));
    out->steps = cnt[0]; out->graph_captures = captures; out->rows_decode = cnt[1]; out->rows_prompt = cnt[2]; out->rows_idle = cnt[3];
    out->n_slots = sv.n_slots; out->max_rows = sv.max_rows;
    for (int r = 0; r < sv.max_rows; r++) {
        const bool on = cnt[0] > 0 && rows[r].pos >= 0;            // (before the first step the table holds nothing)
        const bool lg = on && (lflag_dev ? lflag[r] != 0 : lrow[rows[r].pad] == r);
        out->last_rows[r] = rama_q8_serve_row{on ? rows[r].pad : -1, on ? rows[r].pos : -1, lg ? 1 : 0};
    }
    for (int i = 0; i < sv.n_slots; i++) {
        out->slots[i] = rama_q8_serve_slot{slots[i].state, slots[i].n_ctx, slots[i].cursor, slots[i].n_out, slots[i].max_new};
        out->generation[i] = sv.gen[i];
    }
    return 0;
}

int rama_q8_serve_poll(rama_ctx* c, int slot, int from, int32_t* out_host, int max_tokens, int* n_ready, int* finished, int* generation) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "q8_serve_poll: bad argument");
    return serve_poll_ring("q8_serve_poll", c->q8s, slot, from, out_host, max_tokens, n_ready, finished, generation);
}

int rama_q8_serve_tokens(rama_ctx* c, int slot, int32_t* out_host, int max_tokens, int* n_out) {
    RAMA_ENTER(c);
    REQUIRE(c, RAMA_EINVAL, "q8_serve_tokens: bad argument");
    return serve_tokens_back(c, "q8_serve_tokens", c->q8s, slot, out_host, max_tokens, n_out);
}

int rama_q8_serve_stats(rama_ctx* c, rama_q8_serve_report* out) {
    RAMA_ENTER(c);
    REQUIRE(c && out && c->q8s.n_slots > 0, RAMA_EINVAL, "q8_serve_stats: bad argument");
    return serve_report(c, c->q8s, c->q8s.captures, c->q8s.spec ? c->q8s.st.lflag : nullptr, out);
}

int rama_q8_serve_spec_stats(rama_ctx* c, rama_q8_serve_spec_report* out) {
    RAMA_ENTER(c);
    REQUIRE(c && out && c->q8s.n_slots > 0 && c->q8s.spec, RAMA_EINVAL, "q8_serve_spec_stats: no chain begun with rama_q8_serve_begin_spec");
    return serve_spec_report(c, c->q8s, out);
}
// what either chain's _spec_stats entry does behind its refusal
int serve_spec_report(rama_ctx* c, const rama_ctx::ServeState& sv, rama_q8_serve_spec_report* out) {
    { const int rh = q8_drain(c); if (rh) return rh; }
    memset(out, 0, sizeof *out);
    unsigned long long cnt[4], sched[2];
    std::vector<ServeSpecSlot> ss(sv.n_slots);
    std::vector<ServeSpecSums> sums(sv.n_slots);
    HIPCHK(hipMemcpy(cnt, sv.t.counters, sizeof cnt, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sched, sv.st.sched, sizeof sched, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ss.data(), sv.st.ss, sizeof(ServeSpecSlot) * sv.n_slots, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sums.data(), sv.st.sums, sizeof(ServeSpecSums) * sv.n_slots, hipMemcpyDeviceToHost));
    out->steps = cnt[0]; out->rows_decode = cnt[1]; out->rows_prompt = cnt[2]; out->rows_idle = cnt[3];
    out->rows_draft = sched[0]; out->drafts_wanted = sched[1];
    out->n_slots = sv.n_slots; out->max_rows = sv.max_rows; out->n_draft_cap = sv.n_draft_cap; out->hint_cap = sv.hint_cap;
    static_assert(sizeof out->accepted_hist == sizeof sums[0].hist, "one histogram entry per accept count 0..15");
    for (int i = 0; i < sv.n_slots; i++) {
        out->drafts_granted += sums[i].granted; out->drafts_accepted += sums[i].accepted; out->tokens_emitted += sums[i].emitted;
        for (int a = 0; a < kSpecRows; a++) out->accepted_hist[a] += sums[i].hist[a];
        out->last_want[i] = cnt[0] ? ss[i].want : 0;
        out->last_granted[i] = cnt[0] ? ss[i].granted : 0;
    }
    return 0;
}

// ---- THE SPECULATIVE CHAIN (q8_spec.hpp): one sequence, up to 15 drafted tokens per step by n-gram lookup in its own text
// and a caller's hint, drafts and the token before them verified in ONE weight pass of n_draft + 1 rows.  A token-batch pass over rows at
// consecutive positions of one sequence gives every row the bits of its own rama_q8_forward, so whatever is accepted is what
// rama_q8_generate produces: a wrong draft costs time only.  A third chain next to the two above, with a state of its own.

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
    rc = q8_chain_scratch(c, cfg, w->group_size, sampled ? R : 0, &b); if (rc) return rc;
    auto& sp = c->q8p;
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

// the commit of a tree pass: the path recorded in tt.ts, from the tree store into the caches at kc / vc (q8_tree.hpp tree_commit_kernel)
static int launch_tree_commit(rama_ctx* c, const TreeTables& tt, float* kc, float* vc, int n_layers, int dim, int seq_len) {
    TreeCommitParams p{tt.ts, kc, vc, tt.ks, tt.vs, dim, seq_len, tt.store_rows};
    hipLaunchKernelGGL(tree_commit_kernel, dim3(n_layers, kSpecMaxDraft), dim3(256), 0, c->stream, p);
    LAUNCHCHK();
    return 0;
}

// one step of a chain begun with rama_q8_spec_begin_tree: the tree and its row table, the pass over it, every row's pick, the accept rule
// over the tree, the accepted path's rows into the cache
static int enqueue_q8_spec_tree_step(rama_ctx* c, const Q8BatchScratch& b) {
    auto& sp = c->q8p;
    const int R = sp.n_rows;
    hipLaunchKernelGGL(spec_tree_draft_kernel, dim3(1), dim3(1024), 0, c->stream, sp.t, sp.tt);
    LAUNCHCHK();
    int rc = enqueue_q8_batch_pass(c, &sp.cfg, &sp.w, b, sp.t.row_tok, sp.t.rows, R, &sp.tt); if (rc) return rc;
    SpecPickParams fin{};
    fin.t = sp.t;
    rc = enqueue_q8_pick_rows(c, b, sp.cfg.vocab_size, sp.sampled, sp.t.trow, R, &fin.r); if (rc) return rc;
    hipLaunchKernelGGL(spec_pick_kernel, dim3(R), dim3(1024), 0, c->stream, fin);
    LAUNCHCHK();
    hipLaunchKernelGGL(spec_tree_accept_kernel, dim3(1), dim3(64), 0, c->stream, sp.t, sp.tt);
    LAUNCHCHK();
    return launch_tree_commit(c, sp.tt, sp.state.key_cache, sp.state.value_cache, sp.cfg.n_layers, sp.cfg.dim, sp.cfg.seq_len);
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
    return q8_chain_steps(c, sp, sp.sampled ? sp.n_rows : 0, n_steps, [&](const Q8BatchScratch& b) { return enqueue_q8_spec_step(c, b); }, &n_done);
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
