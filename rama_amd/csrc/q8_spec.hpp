// q8_spec.hpp -- the SPECULATIVE CHAIN of a Q8 model (rama_q8_spec_begin / _steps): one sequence, drafts by
// n-gram lookup in its own text and a caller's hint, all of them verified in one weight pass.  Every step
//   spec_draft_kernel    the tail n-gram's latest occurrence (hint first, longest n first) -> the drafts; the row table
//                        (SeqSlot[n_draft + 1]: row j = token s[L-1], d[0], ... at positions P, P + 1, ...; the rest idle, position -1),
//                        the row tokens and the sampler records
//   the batched pass     embed_rows_kernel, q8_batch_layers, the final norm, the quantizer and the classifier over n_draft + 1 rows
//   the batched sampler's ordering launches (topp_sort.hpp; an idle row or temperature 0 leaves them at once)
//   spec_pick_kernel     one workgroup per row: Device::sample of the row's logits, nothing else
//   spec_accept_kernel   the accept rule (q8_spec_tables.hpp), the emitted tokens appended to s, to `out` and to the host-visible ring,
//                        the count and the finished word, the counters
// Nothing in a step's launch geometry depends on the sequence, so one captured graph serves the chain for its whole life.
// The drafting rule is rama_q8_spec_draft's (q8_spec_api.hip), which the kernel must reproduce exactly.
#pragma once
#define RAMA_Q8_SPEC_HPP 1      // (q8_api.hip and q8_serve_api.hip refuse to be compiled with this header: its kernels are q8_spec_api.hip's)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "topp_sort.hpp"
#include "q8_spec_tables.hpp"   // the tables, spec_scan_text, spec_accept_rule

namespace rama {

__global__ __launch_bounds__(1024) void spec_draft_kernel(SpecTables t) {
    __shared__ int s_best[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SpecState* st = t.st;
    const int L = st->L, n_hint = st->n_hint, K = st->n_draft, fin = st->finished;
    const int P = L - 1;
    const int* hint = t.text;
    const int* s = t.text + n_hint;
    const int room = min(st->seq_len - 1 - P, st->max_new - st->n_out - 1);
    const int cap = fin ? 0 : max(min(K, room), 0);
    int key = -1;
    if (cap > 0) {                                                 // (uniform, as everything that decides a barrier below)
        for (int n = min(st->ngram, L); n >= 1 && key < 0; n--) {
            int tail[kSpecMaxNgram];
#pragma unroll
            for (int i = 0; i < kSpecMaxNgram; i++) tail[i] = s[min(L - n + i, L - 1)];
            int best = spec_scan_text(hint, n_hint, n, tail, kSpecHintBit, -1);
            best = spec_scan_text(s, L - 1, n, tail, 0, best);     // the occurrence ends before L: the tail itself does not count
            best = wave_max_i(best);
            if (lane == 0) s_best[wave] = best;
            __syncthreads();
            key = s_best[0];
            for (int w = 1; w < (int)(blockDim.x >> 6); w++) key = max(key, s_best[w]);
            __syncthreads();
        }
    }
    const bool in_hint = key >= 0 && (key & kSpecHintBit);
    const int e = key & (kSpecHintBit - 1);
    const int* src = in_hint ? hint : s;
    const int n_d = key < 0 ? 0 : min(cap, (in_hint ? n_hint : L) - e);
    if (tid <= K) {                                                // K + 1 <= kSpecRows rows
        const bool on = !fin && tid <= n_d;
        const int at = tid == 0 || !on ? L - 1 : e + tid - 1;       // (a valid index of either text whatever the row)
        const int tok = (tid == 0 || !on ? s : src)[at];
        t.rows[tid] = on ? SeqSlot{st->kc, st->vc, P + tid, 0} : SeqSlot{nullptr, nullptr, -1, -1};
        t.row_tok[tid] = on ? tok : 0;
        t.trow[tid] = ToppRow{on ? st->temperature : 0.0f, st->topp, st->u, 0, nullptr};
        if (tid >= 1) st->d[tid - 1] = on ? tok : -1;
    }
    if (tid == 0) {
        st->n_d = n_d;
        st->steps += 1ull;
        if (!fin) { st->rows_fed += (unsigned long long)(n_d + 1); st->drafts += (unsigned long long)n_d; }
    }
}

// Device::sample of row b's logits -- the argmax (cpu.rs:163-167: the LAST maximal index) or topp_pick_scan_kernel's pick on the slices
// the ordering launches left -- into picks[b].  It advances nothing: spec_accept_kernel decides what the picks mean.
struct SpecPickParams {
    SpecTables t;
    PickRows r;
};
__global__ __launch_bounds__(1024) void spec_pick_kernel(SpecPickParams p) {
    __shared__ ScanShared sh;
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    SpecState* st = p.t.st;
    if (st->finished || b > st->n_d) return;                       // an idle row (uniform: the whole workgroup)
    const int tok = topp_row_pick(p.r, b, st->temperature, st->topp, st->u, sh, s_v, s_i);
    if (tid == 0) st->picks[b] = tok;
}

// What ends a step: one workgroup, one thread of it -- at most 16 tokens, and the host-visible words must go out in order.
__global__ void spec_accept_kernel(SpecTables t) {
    if (threadIdx.x != 0) return;
    SpecState* st = t.st;
    if (st->finished) return;
    const int n_out = st->n_out, L = st->L;
    int a, fin;
    const int emit = spec_accept_rule(st->d, st->n_d, st->picks, st->stop, st->max_new - n_out, &a, &fin);
    int* s = t.text + st->n_hint;
    for (int i = 0; i < emit; i++) {                               // L + emit <= n_context + max_new <= seq_len; n_out + emit <= max_new
        const int tok = st->picks[i];
        s[L + i] = tok;
        t.out[n_out + i] = tok;
        // the host may be polling these words while the chain runs on: system-scope stores
        __hip_atomic_store(t.ring + n_out + i, tok + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    st->L = L + emit;
    st->n_out = n_out + emit;
    __hip_atomic_store(t.count, n_out + emit, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);      // (after the ring words)
    if (fin) {
        st->finished = 1;
        __hip_atomic_store(t.done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);              // (after the count: who sees it set finds every token)
    }
    st->accepted += (unsigned long long)a;
    st->emitted += (unsigned long long)emit;
    st->hist[a] += 1ull;
}

}  // namespace rama
