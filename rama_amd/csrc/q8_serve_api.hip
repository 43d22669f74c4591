// q8_serve_api.hip -- THE SERVING CHAIN of a Q8 model (rama_q8_serve_*) and rama_q8_kv_fork, with the host layer
// that the fp32 serving chain of batch_api.hip shares through ctx.hpp: the serve_state_* / serve_admit_* / serve_cancel / serve_*_report procedures and
// the launch_serve_* launchers.  The kernels are q8_serve.hpp, q8_serve_spec.hpp, q8_serve_model.hpp and q8_fork.hpp, which this translation unit alone
// includes; the token-batch pass and the checks every Q8 chain shares are q8_api.hip's, reached through q8_host.hpp (DESIGN.md "Translation units").
//
// Continuous batching: n_slots slots share passes of max_rows rows; a scheduler
// launch builds every step's row table from the slot table on the device, a pick launch runs the slots' state machine, and an admission
// is a stream-ordered copy + launch between two steps.  Nothing in a step's launch geometry depends on a sequence, so one captured graph
// serves the chain for its whole life.
#include "q8_host.hpp"
#include "q8_serve.hpp"
#include "q8_fork.hpp"
#include "q8_serve_spec.hpp"
#include "q8_serve_model.hpp"

#if defined(RAMA_CHAIN_HPP) || defined(RAMA_Q8_HPP) || defined(RAMA_Q8_SPEC_HPP) || defined(RAMA_Q8_TREE_HPP)
#error "q8_serve_api.hip must not include chain.hpp, q8.hpp / q8_batch.hpp, q8_spec.hpp or q8_tree.hpp: their kernels belong to other code objects"
#endif

#include <algorithm>
#include <cstring>
#include <vector>

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
void serve_release(rama_ctx* c) {
    auto& sv = c->q8s;
    destroy_graph(sv.cg);
    serve_state_free(sv);
    sv = rama_ctx::Q8Serve();
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
#define ADMIT_UNLESS(cond, what) REFUSE_UNLESS(cond, names.admit, what)
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
    REFUSE_UNLESS(n_cached >= 0 && n_cached <= n_context - 1, names.admit_at, "n_cached outside [0, n_context - 1] (the final context position is always fed)");
    ADMIT_UNLESS(plan->max_new >= 1, "max_new < 1");
    if (plan->max_new > sv.out_cap) {
        char what[96];
        snprintf(what, sizeof what, "max_new beyond %s's max_new_cap", names.begin);
        return refuse(names.admit, what, __FILE__, __LINE__);
    }
    ADMIT_UNLESS(n_context <= cfg.seq_len - plan->max_new, "n_context + max_new beyond seq_len");
    CHECKED(check_tokens(names.admit, "token outside the vocabulary", context_host, n_context, V));
    CHECKED(check_sampler(names.admit, plan->temperature, plan->topp, plan->u));
    CHECKED(check_stop_token(names.admit, plan->stop_token, V));
    for (int j = 0; j < sv.n_slots; j++)
        ADMIT_UNLESS(j == slot || !serve_slot_live(sv, j) || (sv.states[j].key_cache != state->key_cache && sv.states[j].value_cache != state->value_cache),
                     "the run state is already in a live slot");
    UNSUPPORTED_UNLESS(plan->temperature == 0.0f || sv.sampler, names.admit, "a sampled plan needs vocab_size <= 32768");
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
    REFUSE_UNLESS(n_ready && sv.n_slots > 0 && slot >= 0 && slot < sv.n_slots && from >= 0 && max_tokens >= 0 && (max_tokens == 0 || out_host), entry, "bad argument");
    // the finished word first: it is stored after the occupant's last ring word, so a set word means every token is there to be read
    const int fin = __atomic_load_n(sv.done + slot, __ATOMIC_ACQUIRE);
    *n_ready = read_ring(sv.ring + (size_t)slot * sv.out_cap, sv.out_cap, from, out_host, max_tokens);
    if (finished) *finished = fin;                                 // 0, 1, or RAMA_SERVE_CANCELLED
    if (generation) *generation = sv.gen[slot];
    return 0;
}
int serve_tokens_back(rama_ctx* c, const char* entry, const rama_ctx::ServeState& sv, int slot, int32_t* out_host, int max_tokens, int* n_out) {
    REFUSE_UNLESS(n_out && sv.n_slots > 0 && slot >= 0 && slot < sv.n_slots && max_tokens >= 0 && (max_tokens == 0 || out_host), entry, "bad argument");
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

