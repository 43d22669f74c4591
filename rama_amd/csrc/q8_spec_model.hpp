// q8_spec_model.hpp -- the speculative chain with drafts from a SMALL Q8 MODEL (rama_q8_spec_begin_model): the chain of
// q8_spec.hpp -- its SpecState, ring, finished word, pick and accept kernels, all unchanged -- with the n-gram lookup replaced by K greedy-or-sampled
// passes of a draft model over the same vocabulary.  Every step
//   spec_model_open_kernel    n_d = min(K, seq_len - 1 - P, remaining - 1); the TARGET's row table (SeqSlot[K + 1]: positions P, P + 1, ...; the rows
//                             behind n_d idle), its sampler records and row 0's token s[L - 1]; the first DRAFT pass's row table: the rows at
//                             positions Dc..P carrying s[Dc..P] -- one row, or two when the step before accepted all of its drafts (d[K - 1] was
//                             never fed to the draft model: the catch-up row)
//   K times                   a token-batch pass of the draft model (2 rows, then 1) and spec_model_pick_kernel: Device::sample -- the plan's (T, topp, u),
//                             the target's own rule -- of the last live row's logits -> d[j], the target's row j + 1 token, and the next draft pass's
//                             row (d[j], P + j + 1), idle once j + 1 >= n_d
//   the target's pass, the ordering launches, spec_pick_kernel and spec_accept_kernel of q8_spec.hpp
//   spec_model_close_kernel   the draft cursor Dc' = L + min(a, n_d - 1): the draft rows whose tokens the accept rule made part of s
// An idle draft row (n_d == 0, a finished sequence, passes j >= n_d) has position -1: it writes nothing and nothing is read through it.  Rows of the
// draft cache at and behind Dc' may hold the rows of rejected drafts, as the target's cache may behind its cursor: the next step rewrites whatever it
// reads before it reads it.  Nothing in a step's launch geometry depends on the sequence: one captured graph for the chain's life.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "topp_sort.hpp"
#include "q8_spec_tables.hpp"

namespace rama {

// What opens a step: one workgroup of 64 threads; thread i writes the target's row i and, below kSpecModelRows, the draft pass's row i.
__global__ void spec_model_open_kernel(SpecTables t, SpecModelTables m) {
    const int tid = threadIdx.x;
    SpecState* st = t.st;
    SpecModelState* ms = m.ms;
    const int L = st->L, K = st->n_draft, fin = st->finished, Dc = ms->Dc;
    const int P = L - 1;
    const int* s = t.text + st->n_hint;
    const float T = st->temperature, topp = st->topp, u = st->u;
    const int room = min(st->seq_len - 1 - P, st->max_new - st->n_out - 1);
    const int n_d = fin ? 0 : max(min(K, room), 0);
    const int gap = P - Dc;                                        // 0, or 1 after a step that accepted all of its drafts
    const int n_live = n_d > 0 && gap >= 0 ? min(gap, kSpecModelRows - 1) + 1 : 0;
    if (tid <= K) {                                                // K + 1 <= kSpecRows rows of the target's pass
        const bool on = !fin && tid <= n_d;
        t.rows[tid] = on ? SeqSlot{st->kc, st->vc, P + tid, 0} : SeqSlot{nullptr, nullptr, -1, -1};
        t.row_tok[tid] = on && tid == 0 ? s[P] : 0;                // (rows 1..n_d: spec_model_pick_kernel)
        t.trow[tid] = ToppRow{on ? T : 0.0f, topp, u, 0, nullptr};
        if (tid >= 1) st->d[tid - 1] = -1;
    }
    if (tid < kSpecModelRows) {
        const bool on = tid < n_live;
        const int at = min(max(Dc + tid, 0), P);                   // (a valid index of s whatever the row)
        m.rows[tid] = on ? SeqSlot{ms->kc, ms->vc, at, 0} : SeqSlot{nullptr, nullptr, -1, -1};
        m.row_tok[tid] = on ? s[at] : 0;
        m.trow[tid] = ToppRow{on && tid == n_live - 1 ? T : 0.0f, topp, u, 0, nullptr};
    }
    if (tid == 0) {
        st->n_d = n_d;
        st->steps += 1ull;
        if (!fin) { st->rows_fed += (unsigned long long)(n_d + 1); st->drafts += (unsigned long long)n_d; }
        ms->pick_row = n_live - 1;
        ms->L0 = L;
        ms->open = !fin;
        if (n_live > 0) {
            ms->draft_passes += (unsigned long long)n_d;
            ms->draft_rows_fed += (unsigned long long)(n_d + n_live - 1);
            ms->catch_up_rows += (unsigned long long)(n_live - 1);
        }
    }
}

// What ends draft pass j, one workgroup: d[j] = Device::sample of the pass's last live row -- the argmax or topp_pick_scan_kernel's pick on the slices
// the ordering launches left, exactly spec_pick_kernel's rule --, stored where the accept rule and the target's row j + 1 read it; and the next
// pass's one row.
struct SpecModelPickParams {
    SpecTables t;
    SpecModelTables m;
    PickRows r;
    int j;
};
__global__ __launch_bounds__(1024) void spec_model_pick_kernel(SpecModelPickParams p) {
    __shared__ ScanShared sh;
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    const int tid = threadIdx.x, j = p.j;
    SpecState* st = p.t.st;
    SpecModelState* ms = p.m.ms;
    const int n_d = st->n_d, L0 = ms->L0;
    const int b = j == 0 ? ms->pick_row : 0;
    const bool on = ms->open && j < n_d && b >= 0;                 // (uniform: the whole workgroup)
    const float T = st->temperature, topp = st->topp, u = st->u;
    int tok = 0;
    if (on) tok = topp_row_pick(p.r, b, T, topp, u, sh, s_v, s_i);
    if (tid != 0) return;
    const bool next = on && j + 1 < n_d;                           // pass j + 1 feeds d[j] at position P + j + 1 = L0 + j <= P + n_d - 1
    st->d[j] = on ? tok : -1;
    p.t.row_tok[j + 1] = on ? tok : 0;                             // j + 1 <= K
    p.m.rows[0] = next ? SeqSlot{ms->kc, ms->vc, L0 + j, 0} : SeqSlot{nullptr, nullptr, -1, -1};
    p.m.row_tok[0] = next ? tok : 0;
    p.m.trow[0] = ToppRow{next ? T : 0.0f, topp, u, 0, nullptr};
}

// What closes a step, behind spec_accept_kernel: the draft rows at positions P..P + n_d - 1 carry s[P], d[0], .., d[n_d - 2], and the accept rule made
// d[0..a) part of s -- so the rows up to position P + min(a, n_d - 1) belong to s.  On the finishing step a budget or stop cut may emit fewer tokens
// than were accepted: the cursor stops at the new L.
__global__ void spec_model_close_kernel(SpecTables t, SpecModelTables m) {
    if (threadIdx.x != 0) return;
    SpecState* st = t.st;
    SpecModelState* ms = m.ms;
    const int n_d = st->n_d;
    if (!ms->open || n_d < 1 || ms->pick_row < 0) return;
    int a = 0;
    while (a < n_d && st->picks[a] == st->d[a]) a++;
    ms->Dc = min(ms->L0 + min(a, n_d - 1), st->L);
}

}  // namespace rama
