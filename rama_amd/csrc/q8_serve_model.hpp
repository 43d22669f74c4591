// q8_serve_model.hpp -- MODEL DRAFTS INSIDE THE SERVING CHAIN (rama_q8_serve_begin_model / _admit_model): a DECODE slot's
// drafts ride on the rows of the step that no slot wants, as in q8_serve_spec.hpp, but they are the next tokens of a SMALL Q8 MODEL over the same
// vocabulary, as in q8_spec_model.hpp -- per slot, with a draft run state and a draft cursor of its own.  The slot table, the row table and the
// admission are q8_serve.hpp's; the scheduler, the pick per row and the accept rule per slot are q8_serve_spec.hpp's kernels, unchanged.  Every step
//   serve_model_open_kernel      per slot: want = min(n_draft, seq_len - 1 - P, max_new - n_out - 1) for a DECODE slot with n_draft > 0 (no draft
//                                exists yet: the scheduler needs the count only); the FIRST draft pass's row table -- such a slot feeds s[Dc..P] to the
//                                draft model, one row, or two when the step before accepted all it was granted (the catch-up row) -- whatever it
//                                will be granted: the pass is in the graph anyway, and feeding keeps P - Dc in {0, 1} while prompts take every row
//   serve_spec_schedule_kernel   the rows and the grants g[i] (q8_serve_spec.hpp); the draft rows' tokens are filled in below
//   n_draft_cap times            a token-batch pass of the draft model over its own scratch (2 n_slots rows, then n_slots), the ordering launches and
//                                serve_model_pick_kernel, one workgroup per slot: d[i][j] = Device::sample of the slot's last live row with the slot's
//                                (T, topp, u) -- the target's rule -- for j < g[i]: the token of the slot's target row j + 1, the draft the accept rule
//                                compares, and the slot's row (d[j], P + j + 1) of pass j + 1, live while j + 1 < g[i]
//   the target's pass over max_rows rows, serve_spec_pick_kernel and serve_spec_accept_kernel (q8_serve_spec.hpp)
//   serve_model_close_kernel     per slot: Dc' = L + min(a, max(g - 1, 0)), L as the step opened, stopped at the new L on a finishing step
// An idle draft row has position -1: it writes nothing and nothing is read through it.  Nothing in a step's launch geometry depends on a
// sequence: one captured graph for the chain's life.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "q8_serve_spec.hpp"        // the chain it extends
#include "q8_serve_model_tables.hpp"

namespace rama {

// an admission's draft side (the values travel as launch arguments: no record to stage)
__global__ void serve_model_install_kernel(ServeModelTables m, int slot, float* kc, float* vc, int Dc) {
    if (threadIdx.x != 0) return;
    ServeModelSlot* ms = m.ms + slot;
    ms->kc = kc; ms->vc = vc; ms->Dc = Dc;
    ms->L0 = 0; ms->open = 0; ms->pick_row = -1; ms->n_live = 0;
}

// What opens a step, one workgroup of kServeMaxSlots threads: thread i is slot i.
__global__ __launch_bounds__(kServeMaxSlots) void serve_model_open_kernel(ServeTables t, ServeSpecTables st, ServeModelTables m) {
    const int i = threadIdx.x;
    if (i >= t.n_slots) return;
    const ServeSlot sl = t.slots[i];
    ServeSpecSlot* ss = st.ss + i;
    ServeModelSlot* ms = m.ms + i;
    const int K = ss->n_draft;
    const int L = sl.n_ctx + sl.n_out, P = L - 1;                   // a DECODE slot: cursor == P, s[P] == tok
    const bool dec = sl.state == kServeDecode && K > 0;
    const int room = min(t.seq_len - 1 - P, sl.max_new - sl.n_out - 1);
    const int want = dec ? max(min(K, room), 0) : 0;
    const int Dc = ms->Dc, gap = P - Dc;                            // 0, or 1 after a step that accepted all it was granted
    const bool feed = dec && gap >= 0 && gap <= 1;
    const int n_live = feed ? gap + 1 : 0;
    const int* s = t.ctx + (size_t)i * t.seq_len;
    ss->want = want;
#pragma unroll
    for (int j = 0; j < kSpecRows; j++) ss->d[j] = 0;              // (a token of the vocabulary: the scheduler copies d into the draft rows)
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const bool on = k < n_live;
        const int at = min(max(Dc + k, 0), t.seq_len - 1);          // (a valid index of s whatever the row)
        const int tok = s[at];
        m.rows0[2 * i + k] = on ? SeqSlot{ms->kc, ms->vc, at, i} : SeqSlot{nullptr, nullptr, -1, -1};
        m.row_tok0[2 * i + k] = on ? tok : 0;
        m.trow0[2 * i + k] = ToppRow{on && k == n_live - 1 && want > 0 ? sl.temperature : 0.0f, sl.topp, sl.u, 0, nullptr};
    }
    ms->L0 = L;
    ms->open = feed ? 1 : 0;
    ms->pick_row = feed ? 2 * i + gap : -1;
    ms->n_live = n_live;
}

// What ends draft pass j, one workgroup per slot: d[j] = Device::sample of the slot's last live row -- the argmax or topp_pick_scan_kernel's pick on
// the slices the ordering launches left, exactly serve_spec_pick_kernel's rule --, stored where the accept rule and the target's row j + 1 read it;
// and the slot's row of the next pass.
struct ServeModelPickParams {
    ServeTables t; ServeSpecTables st; ServeModelTables m;
    PickRows r;
    int j;
};
__global__ __launch_bounds__(1024) void serve_model_pick_kernel(ServeModelPickParams p) {
    __shared__ ScanShared sh;
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    const int b = blockIdx.x, tid = threadIdx.x, j = p.j;
    const ServeModelSlot* ms = p.m.ms + b;
    ServeSpecSlot* ss = p.st.ss + b;
    const ServeSlot* sl = p.t.slots + b;
    const int g = ss->granted, L0 = ms->L0;
    const int row = j == 0 ? ms->pick_row : b;
    const bool on = ms->open && j < g && row >= 0;                 // (uniform: the whole workgroup)
    const float T = sl->temperature, topp = sl->topp, u = sl->u;
    int tok = 0;
    if (on) tok = topp_row_pick(p.r, row, T, topp, u, sh, s_v, s_i);
    if (tid != 0) return;
    const bool next = on && j + 1 < g;                             // pass j + 1 feeds d[j] at position P + j + 1 = L0 + j <= P + g - 1
    if (on) {
        ss->d[j] = tok;
        p.t.row_tok[ss->row0 + j + 1] = tok;                       // row0 + g < max_rows: the scheduler granted the row
    }
    p.m.rows[b] = next ? SeqSlot{ms->kc, ms->vc, L0 + j, b} : SeqSlot{nullptr, nullptr, -1, -1};
    p.m.row_tok[b] = next ? tok : 0;
    p.m.trow[b] = ToppRow{next ? T : 0.0f, topp, u, 0, nullptr};
}

// What closes a step, behind serve_spec_accept_kernel, thread i for slot i: the draft rows at positions Dc..P + max(g - 1, 0) carry s[Dc..P], d[0], ..,
// d[g - 2], and the accept rule made d[0..a) part of s -- so the rows up to position P + min(a, g - 1) belong to s.  On a finishing step a budget or
// stop cut may emit fewer tokens than were accepted: the cursor stops at the new L.
__global__ __launch_bounds__(kServeMaxSlots) void serve_model_close_kernel(ServeTables t, ServeSpecTables st, ServeModelTables m) {
    const int i = threadIdx.x;
    if (i >= t.n_slots) return;
    ServeModelSlot* ms = m.ms + i;
    if (!ms->open) return;
    const ServeSpecSlot* ss = st.ss + i;
    const int g = ss->granted;
    const int* picks = st.picks + ss->row0;
    int a = 0;
    while (a < g && picks[a] == ss->d[a]) a++;
    const int L = t.slots[i].n_ctx + t.slots[i].n_out;             // after the accept rule
    ms->Dc = min(ms->L0 + min(a, max(g - 1, 0)), L);
    ms->open = 0;
    ms->draft_passes += (unsigned long long)max(g, 1);
    ms->draft_rows_fed += (unsigned long long)(ms->n_live + max(g, 1) - 1);
    ms->catch_up_rows += (unsigned long long)(ms->n_live - 1);
}

}  // namespace rama
