// q8_serve_spec.hpp -- SPECULATION INSIDE THE SERVING CHAIN (rama_q8_serve_begin_spec / _admit_spec): a DECODE
// slot's n-gram drafts ride on the rows of the step that no slot wants.  The slot table, the row table and the admission are q8_serve.hpp's;
// the drafting rule and the accept rule are q8_spec.hpp's, per slot.  Every step of such a chain
//   serve_draft_kernel           one workgroup per slot: a DECODE slot with n_draft > 0 looks the tail of its text (its row of t.ctx:
//                                context ++ outputs) up in its hint and in the text -> want, d[0..want)
//   serve_spec_schedule_kernel   serve_schedule_kernel's rule, then the rows still left to the DECODE slots' drafts in ascending slot index:
//                                the row table, the row tokens, per ROW the logits flag and the sampler record, per slot nrows / granted / row0
//   the batched pass             embed_rows_kernel, q8_batch_layers, the final norm, the quantizer and the classifier over all max_rows rows
//   the batched sampler's ordering launches (topp_sort.hpp; a row without the flag or at temperature 0 leaves them at once)
//   serve_spec_pick_kernel       one workgroup per row: Device::sample of a flagged row's logits, nothing else
//   serve_spec_accept_kernel     one workgroup per slot: the cursor of a slot inside its context, the one token of a final context row,
//                                spec_accept_rule for a DECODE slot; the tokens go to out, the ring and the text, then the finished word
// The rules are rama_q8_spec_draft's and rama_q8_spec_accept's (q8_spec_api.hip) and rama_q8_serve_spec_plan_step's (q8_serve_api.hip), which the
// kernels must reproduce exactly.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "q8_serve.hpp"         // the chain it extends
#include "q8_serve_spec_tables.hpp"     // (and q8_spec_tables.hpp: spec_scan_text, spec_accept_rule -- not q8_spec.hpp, whose kernels are q8_spec_api.hip's)

namespace rama {

constexpr int kServeDraftThreads = 256;

// serve_scan128 (q8_serve.hpp), word for word: a copy of its own, because a second kernel that calls the same inline function changes the
// order in which the compiler inlines it into serve_schedule_kernel, and with it that kernel's listing (the listing comparison)
__device__ __forceinline__ unsigned long long serve_spec_scan128(unsigned long long v, unsigned long long* buf, unsigned long long* total) {
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int d = 1; d < kServeMaxSlots; d <<= 1) {
        const unsigned long long x = tid >= d ? buf[tid - d] : 0ull;
        __syncthreads();
        buf[tid] += x;
        __syncthreads();
    }
    const unsigned long long inc = buf[tid];
    *total = buf[kServeMaxSlots - 1];
    __syncthreads();
    return inc - v;
}

// an admission's drafting fields and hint: the record (a ServeSpecSlot, then n_hint tokens) that an async copy has brought to `rec`
__global__ void serve_spec_install_kernel(ServeSpecTables st, int slot, const ServeSpecSlot* rec) {
    const int* toks = reinterpret_cast<const int*>(rec + 1);
    const int n = rec->n_hint;
    for (int k = threadIdx.x; k < n; k += blockDim.x) st.hint[(size_t)slot * st.hint_cap + k] = toks[k];
    if (threadIdx.x == 0) st.ss[slot] = *rec;
}

__global__ __launch_bounds__(kServeDraftThreads) void serve_draft_kernel(ServeTables t, ServeSpecTables st) {
    __shared__ int s_best[kServeDraftThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ServeSlot sl = t.slots[b];
    ServeSpecSlot* ss = st.ss + b;
    const int K = ss->n_draft, n_hint = ss->n_hint;
    const int L = sl.n_ctx + sl.n_out, P = L - 1;                   // a DECODE slot: cursor == P, s[P] == tok
    const int room = min(t.seq_len - 1 - P, sl.max_new - sl.n_out - 1);
    const int cap = sl.state == kServeDecode ? max(min(K, room), 0) : 0;
    if (cap == 0) {                                                // wants nothing (uniform: the whole workgroup, before any barrier)
        if (tid == 0) ss->want = 0;
        return;
    }
    const int* hint = st.hint + (size_t)b * st.hint_cap;
    const int* s = t.ctx + (size_t)b * t.seq_len;
    int key = -1;
    for (int n = min(ss->ngram, L); n >= 1 && key < 0; n--) {
        int tail[kSpecMaxNgram];
#pragma unroll
        for (int i = 0; i < kSpecMaxNgram; i++) tail[i] = s[min(L - n + i, L - 1)];
        int best = spec_scan_text(hint, n_hint, n, tail, kSpecHintBit, -1);
        best = spec_scan_text(s, L - 1, n, tail, 0, best);         // the occurrence ends before L: the tail itself does not count
        best = wave_max_i(best);
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        key = s_best[0];
        for (int w = 1; w < kServeDraftThreads / 64; w++) key = max(key, s_best[w]);
        __syncthreads();
    }
    const bool in_hint = key >= 0 && (key & kSpecHintBit);
    const int e = key & (kSpecHintBit - 1);
    const int n_d = key < 0 ? 0 : min(cap, (in_hint ? n_hint : L) - e);
    if (tid < kSpecMaxDraft) {
        const bool on = tid < n_d;
        const int at = on ? e + tid : L - 1;                       // (a valid index of the text it is taken from whatever the thread)
        const int tok = (on && in_hint ? hint : s)[at];
        ss->d[tid] = on ? tok : -1;
    }
    if (tid == 0) ss->want = n_d;
}

__global__ __launch_bounds__(kServeMaxSlots) void serve_spec_schedule_kernel(ServeTables t, ServeSpecTables st) {
    __shared__ unsigned long long s_buf[kServeMaxSlots];
    __shared__ int s_off[kServeMaxSlots + 1];
    const int i = threadIdx.x;
    ServeSlot s{};
    int dwant = 0;
    if (i < t.n_slots) { s = t.slots[i]; dwant = st.ss[i].want; }
    const bool dec = s.state == kServeDecode, pro = s.state == kServePrompt;
    const int base = dec || pro ? 1 : 0;
    const int want = pro ? s.n_ctx - s.cursor - 1 : 0;            // context positions beyond the slot's first row
    dwant = dec ? dwant : 0;
    // serve_schedule_kernel's scan: slots with a row (bits 52..), DECODE slots (bits 40..51), further positions wanted (bits 0..39)
    unsigned long long tot;
    const unsigned long long before = serve_spec_scan128(((unsigned long long)base << 52) | ((unsigned long long)(dec ? 1 : 0) << 40) | (unsigned long long)want, s_buf, &tot);
    const int n_base = (int)(tot >> 52), n_dec = (int)((tot >> 40) & 0xFFFull);
    const long long want_before = (long long)(before & ((1ull << 40) - 1ull)), want_all = (long long)(tot & ((1ull << 40) - 1ull));
    const long long spare = (long long)(t.max_rows - n_base);
    const long long left = spare - want_before;                    // rows left over when this slot's turn comes
    const int extra = left <= 0 ? 0 : (int)((long long)want < left ? (long long)want : left);
    // the third class: what the prompts leave goes to the drafts, again in ascending slot index
    const long long spare_d = spare - (want_all < spare ? want_all : spare);
    unsigned long long dtot;
    const long long d_before = (long long)serve_spec_scan128((unsigned long long)dwant, s_buf, &dtot);
    const long long d_left = spare_d - d_before;
    const int granted = d_left <= 0 ? 0 : (int)((long long)dwant < d_left ? (long long)dwant : d_left);
    const int n = base + extra + granted;
    const int off = (int)serve_spec_scan128((unsigned long long)n, s_buf, &tot);
    const int used = (int)tot;
    if (i < t.n_slots) {
        const bool lg = dec || (pro && s.cursor + n == s.n_ctx);  // DECODE rows, or the final context position
        t.nrows[i] = n;
        t.lrow[i] = lg ? off + n - 1 : -1;
        st.ss[i].granted = granted;
        st.ss[i].row0 = off;
    }
    s_off[i] = off;
    if (i == kServeMaxSlots - 1) s_off[kServeMaxSlots] = used;
    __syncthreads();
    if (i < t.max_rows) {
        if (i < used) {
            int lo = 0, hi = kServeMaxSlots - 1;                  // the first slot whose rows end behind row i
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_off[mid + 1] > i) hi = mid; else lo = mid + 1; }
            const ServeSlot o = t.slots[lo];
            const int k = i - s_off[lo], pos = o.cursor + k;
            const bool od = o.state == kServeDecode;
            // both loads are made, at an index inside their arrays, and the token selected afterwards
            const int dtok = st.ss[lo].d[min(max(k - 1, 0), kSpecMaxDraft - 1)];
            const int ctok = t.ctx[(size_t)lo * t.seq_len + min(pos, t.seq_len - 1)];
            const bool flag = od || pos == o.n_ctx - 1;
            t.rows[i] = SeqSlot{o.kc, o.vc, pos, lo};
            t.row_tok[i] = od ? (k == 0 ? o.tok : dtok) : ctok;
            st.lflag[i] = flag ? 1 : 0;
            st.rrow[i] = ToppRow{flag ? o.temperature : 0.0f, o.topp, o.u, 0, nullptr};
        } else {
            t.rows[i] = SeqSlot{nullptr, nullptr, -1, -1};
            t.row_tok[i] = 0;
            st.lflag[i] = 0;
            st.rrow[i] = ToppRow{0.0f, 0.0f, 0.0f, 0, nullptr};
        }
    }
    if (i == 0) {
        const long long g_all = (long long)dtot < spare_d ? (long long)dtot : spare_d;
        t.counters[0] += 1ull;
        t.counters[1] += (unsigned long long)n_dec;
        t.counters[2] += (unsigned long long)(used - n_dec - (int)g_all);
        t.counters[3] += (unsigned long long)(t.max_rows - used);
        st.sched[0] += (unsigned long long)g_all;
        st.sched[1] += dtot;
    }
}

// Device::sample of row b's logits -- spec_pick_kernel's body, keyed by the row's flag, with the sampler of the row's slot -- into picks[b].
// It advances nothing: serve_spec_accept_kernel decides what the picks mean.
struct ServeSpecPickParams {
    ServeTables t; ServeSpecTables st;
    PickRows r;
};
__global__ __launch_bounds__(1024) void serve_spec_pick_kernel(ServeSpecPickParams p) {
    __shared__ ScanShared sh;
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!p.st.lflag[b]) return;                                    // idle, or inside a context (uniform: the whole workgroup)
    const ServeSlot* sl = p.t.slots + p.t.rows[b].pad;
    const int tok = topp_row_pick(p.r, b, sl->temperature, sl->topp, sl->u, sh, s_v, s_i);
    if (tid == 0) p.st.picks[b] = tok;
}

// What ends a step, one workgroup per slot and one thread of it: at most 16 tokens, and the host-visible words must go out in order.
__global__ void serve_spec_accept_kernel(ServeTables t, ServeSpecTables st) {
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x;
    ServeSlot* d = t.slots + b;
    const ServeSlot s = *d;
    const int n = t.nrows[b];
    if (n == 0) return;                                            // FREE or DONE
    const int row0 = st.ss[b].row0;
    if (s.state == kServePrompt && s.cursor + n < s.n_ctx) {       // inside its context: no logits yet
        d->cursor = s.cursor + n;
        return;
    }
    int a = 0, fin, emit;
    const int* picks = st.picks + row0;
    if (s.state == kServePrompt) {                                 // the final context position: one pick, one token
        picks += n - 1;
        emit = 1;
        fin = s.max_new <= 1 || picks[0] == s.stop;
    } else {
        const int granted = st.ss[b].granted;
        emit = spec_accept_rule(st.ss[b].d, granted, picks, s.stop, s.max_new - s.n_out, &a, &fin);
        st.sums[b].granted += (unsigned long long)granted;
        st.sums[b].accepted += (unsigned long long)a;
        st.sums[b].hist[a] += 1ull;
    }
    st.sums[b].emitted += (unsigned long long)emit;
    int* text = t.ctx + (size_t)b * t.seq_len + s.n_ctx;           // n_ctx + max_new <= seq_len; n_out + emit <= max_new <= out_cap
    const size_t o = (size_t)b * t.out_cap;
    for (int i = 0; i < emit; i++) {
        const int tok = picks[i];
        text[s.n_out + i] = tok;
        t.out[o + s.n_out + i] = tok;
        // the host may be polling these words while the chain runs on: system-scope stores
        __hip_atomic_store(t.ring + o + s.n_out + i, tok + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    d->n_out = s.n_out + emit;
    d->tok = picks[emit - 1];
    d->cursor = s.state == kServePrompt ? s.n_ctx : s.cursor + emit;       // the position `tok` is fed at
    if (fin) {
        d->state = kServeDone;
        __hip_atomic_store(t.done + b, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);          // (after the ring words: who sees it set finds every token)
    } else {
        d->state = kServeDecode;
    }
}

}  // namespace rama
