// q8_api.hip -- the Q8 part of the C ABI of include/rama_hip.h but for the serving chain (q8_serve_api.hip) and the speculative chain
// (q8_spec_api.hip): rama_q8_quantize / _matmul, the Q8 forward and generate, the token batches (prefill, decode batch) and the chained batch.  The
// kernels are q8.hpp and q8_batch.hpp, which this translation unit alone includes; parity mode's norms and attention and the samplers are reached
// through the launchers of ctx.hpp, which chain_api.hip defines -- this translation unit instantiates none of their kernels (DESIGN.md "Translation units").
// The three device-chained loops are states of their own (rama_ctx::Q8Chain / Q8Serve / Q8Spec over Q8ChainBase) that share PROCEDURES, each
// written once (DESIGN.md "Q8 chains: shared pass, layout, pick and lookup"), here unless marked: q8_chains (graph and lifetime handling), q8_product
// (a layer's five products, for the forward and the batch), BlobCarver (a blob's tables: ctx.hpp), enqueue_q8_row_layers / enqueue_q8_batch_pass (a
// pass over a device row table), enqueue_q8_pick_rows (what a sampled step does behind the classifier), q8_chain_scratch / q8_chain_steps (the begin
// and _steps preambles; the step loop: q8_host.hpp), q8_drain / q8_tokens_back (the _tokens and _stats entries) and the check_* refusals in the
// calling entry's words.  q8_host.hpp declares those of them that the other two Q8 translation units call.
#include "q8_host.hpp"
#include "q8.hpp"
#include "q8_batch.hpp"

#ifdef RAMA_CHAIN_HPP
#error "q8_api.hip must not include chain.hpp: its kernels and g_pred_stats belong to chain_api.hip's code object"
#endif
#if defined(RAMA_Q8_SERVE_HPP) || defined(RAMA_Q8_SPEC_HPP) || defined(RAMA_Q8_TREE_HPP)
#error "q8_api.hip must not include q8_serve.hpp, q8_spec.hpp or q8_tree.hpp: their kernels belong to q8_serve_api.hip's and q8_spec_api.hip's code objects"
#endif

#include <algorithm>
#include <array>
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

// the chained batch's allocations (release_q8); the stream is idle
static void q8_chain_release(rama_ctx* c) {
    auto& qc = c->q8c;
    destroy_graph(qc.cg);
    hipFree(qc.toks); hipFree(qc.seqs); hipFree(qc.out); hipFree(qc.ends); hipFree(qc.rows); hipFree(qc.forced);
    if (qc.ring) hipHostFree(qc.ring);
    if (qc.done) hipHostFree(qc.done);
    qc = rama_ctx::Q8Chain();
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

bool q8_weights_complete(const rama_q8_weights* w) {
    return w->token_embedding_table && w->rms_att_weight && w->rms_ffn_weight && w->rms_final_weight && w->freq_cis_real && w->freq_cis_imag &&
           w->wq && w->wk && w->wv && w->wo && w->w1 && w->w2 && w->w3 && w->wcls && w->wq_s && w->wk_s && w->wv_s && w->wo_s && w->w1_s &&
           w->w2_s && w->w3_s && w->wcls_s;
}

int q8_check(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const rama_run_state* s) {
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

// ---- The refusals several entries share (q8_host.hpp), each in the calling entry's words: the macros pass the refusing line's own file and line
int refuse(const char* entry, const char* what, const char* file, int line, int code) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", entry, what);
    return fail(code, msg, file, line);
}
int check_tokens(const char* entry, const char* what, const int32_t* toks, int n, int V) {
    for (int i = 0; i < n; i++) REFUSE_UNLESS(toks[i] >= 0 && toks[i] < V, entry, what);
    return 0;
}
int check_sampler(const char* entry, float temperature, float topp, float u) {
    REFUSE_UNLESS(topp_params_ok(temperature, topp, u), entry, "temperature >= 0, topp in [0,1], u in [0,1)");
    return 0;
}
int check_stop_token(const char* entry, int stop_token, int V) {
    REFUSE_UNLESS(stop_token >= -1 && stop_token < V, entry, "stop token outside the vocabulary");
    return 0;
}

// the int8 activations: one buffer of max(dim, hidden) values and as many scales (sized here, never inside a capture)
int ensure_q8_scratch(rama_ctx* c, const rama_config* cfg) {
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

// (Q8BatchScratch, q8_host.hpp: the batch path's scratch)
// the shapes the batch path takes: those whose single-token forward runs parity mode's chain norm and chain attention
bool q8_batch_ok(const rama_config* cfg) {
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
size_t q8_batch_scratch_lay(const rama_config* cfg, int gs, size_t T, char* base, Q8BatchScratch* b) {
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
int ensure_q8_batch_scratch(rama_ctx* c, const rama_config* cfg, int gs, Q8BatchScratch* b) {
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
                           float* key_cache, float* value_cache, const SeqSlot* seqs, const TreeTables* tree = nullptr, bool tree_by_node = false) {
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
        if (tree && tree_by_node) {      // a level of a draft model's tree: a fed node's k and v go to the store row of the NODE
            const size_t store_off = (size_t)l * tree->store_rows * dim;
            hipLaunchKernelGGL(q8_rope_tree_node_kernel, dim3((dim / 2 + 255) / 256, nt), dim3(256), 0, c->stream, b.Q, b.Kr, (const float*)b.V,
                               w->freq_cis_real, w->freq_cis_imag, dim, hs, seqs, layer_off, tree->ks + store_off, tree->vs + store_off,
                               (const TreeAnc*)tree->anc);
            LAUNCHCHK();
            TreeAttnParams ta{};
            RefAttnParams& a = ta.a;
            a.q = b.Q; a.att = b.ATT; a.xb = b.XB; a.dim = dim; a.head_size = hs; a.seq_len = seq; a.tok_stride = dim; a.att_stride = H * seq;
            a.seqs = seqs; a.layer_off = layer_off;
            ta.anc = tree->anc; ta.kr = tree->ks + store_off; ta.v = tree->vs + store_off;
            rc = launch_attention_tree(c, ta, H, nt, b.nw, b.att_lds, true); if (rc) return rc;
        } else if (tree) {
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
int enqueue_q8_classifier(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const Q8BatchScratch& b, const float* src_rows, int n_rows) {
    const int dim = cfg->dim, V = cfg->vocab_size;
    int rc = launch_rmsnorm_chain(c, b.XN, src_rows, w->rms_final_weight, dim, nullptr, n_rows, dim); if (rc) return rc;
    rc = launch_q8_quantize(c, b.XN, n_rows * dim, w->group_size, b.xq, b.xs); if (rc) return rc;
    Q8BatchParams p = q8_product<Q8BatchParams>(cfg, w, 0, Q8P_CLS, b.xq, b.xs, b.LG);
    p.n_tok = n_rows; p.ostride = V;
    return launch_q8_gemm<Q8EPI_STORE>(c, p);
}

// A pass over a device row table: the embedding rows of row_tok and every layer over `rows` (n_rows of them; an idle row has position -1) ...
int enqueue_q8_row_layers(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const Q8BatchScratch& b, const int* row_tok,
                          const SeqSlot* rows, int n_rows, const TreeTables* tree, bool tree_by_node) {
    const int dim = cfg->dim;
    hipLaunchKernelGGL(embed_rows_kernel, dim3((dim + 255) / 256, n_rows), dim3(256), 0, c->stream, b.X, w->token_embedding_table, row_tok, n_rows, dim);
    LAUNCHCHK();
    return q8_batch_layers(c, cfg, w, b, n_rows, 0, nullptr, nullptr, rows, tree, tree_by_node);
}
// ... and the classifier tail over every row: rama_q8_decode_batch's pass, and that of every chain's step but the serving chain's without
// drafts, which classifies the rows it has gathered
int enqueue_q8_batch_pass(rama_ctx* c, const rama_config* cfg, const rama_q8_weights* w, const Q8BatchScratch& b, const int* row_tok,
                          const SeqSlot* rows, int n_rows, const TreeTables* tree, bool tree_by_node) {
    const int rc = enqueue_q8_row_layers(c, cfg, w, b, row_tok, rows, n_rows, tree, tree_by_node); if (rc) return rc;
    return enqueue_q8_classifier(c, cfg, w, b, b.X, n_rows);
}

// What every sampled chain's step does behind the classifier: the pick kernel's rows are b.LG's, and -- `sampled` -- the batched sampler's
// ordering launches over the rows' sampler records leave their slices in the context's scratch
int enqueue_q8_pick_rows(rama_ctx* c, const Q8BatchScratch& b, int V, bool sampled, const ToppRow* trow, int n_rows, PickRows* r) {
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
int q8_chain_scratch(rama_ctx* c, const rama_config* cfg, int group_size, int sampler_rows, Q8BatchScratch* b) {
    int rc = ensure_q8_scratch(c, cfg); if (rc) return rc;
    rc = ensure_q8_batch_scratch(c, cfg, group_size, b); if (rc) return rc;
    return sampler_rows > 0 ? ensure_topp_batch(c, sampler_rows, cfg->vocab_size) : 0;
}
// (q8_chain_steps, q8_host.hpp: what every _steps entry does behind its own checks)

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
int q8_drain(rama_ctx* c) {
    if (set_device(c)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    return handoff_check(c);
}
// ... and what a _tokens entry ends with: the first min(produced, cap, max_tokens) tokens of a device row, and their number
int q8_tokens_back(int32_t* out_host, const int* row_dev, int produced, int cap, int max_tokens, int* n) {
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
