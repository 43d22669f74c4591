// q8_spec_model_tree.hpp -- TREE DRAFTS FROM A DRAFT MODEL for the speculative chain of a Q8 model (rama_q8_spec_begin_model_tree, DESIGN.md
// section 8.14): section 8.9's draft model proposes section 8.13's tree.  The tree's SHAPE is static -- spec_model_tree_shape(cap, B, R),
// q8_tree_tables.hpp --; its tokens are the draft model's first choice below every node and its next B - 1 choices below the trunk's.  Every step
//   spec_model_tree_open_kernel   cap, the shape, the TARGET's row table / ancestor records / sampler records as spec_tree_draft_kernel leaves
//                                 them, and every DRAFT level's row table: level d feeds the nodes of depth d - 1 at position P + d - 1 (level 1:
//                                 the root, behind section 8.9's catch-up row when P - Dc == 1); levels behind cap are idle
//   K times                       a token-batch pass of the draft model over the level (q8_rope_tree_node_kernel and attention_draft_tree_kernel
//                                 in place of the launches that touch the cache: only rows of depth 0 write the draft cache, a fed node's k and v
//                                 go to row node - 1 of the draft tree store, and a row's timestep P + k is its depth-k ancestor's store row), the
//                                 ordering launches, and spec_model_tree_pick_kernel: every child's token
//   the target's tree pass, spec_pick_kernel, spec_tree_accept_kernel and tree_commit_kernel of q8_spec.hpp / q8_tree.hpp, unchanged
//   spec_model_tree_close_kernel  the draft cursor Dc' = L + min(a, cap - 1) and the draft commit's record; tree_commit_kernel once more, over the
//                                 draft's caches and store: the accepted path's fed nodes to draft cache positions P + 1 .. Dc' - 1
// An idle draft row has position -1: it writes nothing and nothing is read through it.  Nothing at or behind Dc', or behind the new P, is written in
// either cache.  Nothing in a step's launch geometry depends on the sequence: one captured graph for the chain's life.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "topp_sort.hpp"
#include "q8_spec_tables.hpp"
#include "q8_tree_tables.hpp"

namespace rama {

// What opens a step: one workgroup of 256 threads.  Thread 0 states the shape in LDS; thread i < 16 writes the target's row i; thread
// (d - 1) 16 + r writes row r of draft level d.
__global__ __launch_bounds__(256) void spec_model_tree_open_kernel(SpecTables t, SpecModelTables m, TreeTables tt, SpecModelTreeTables x) {
    __shared__ int s_par[kSpecRows], s_dep[kSpecRows], s_rank[kSpecRows], s_rowof[kSpecRows], s_lvl[kSpecMaxDraft][kSpecRows], s_m, s_fed;
    const int tid = threadIdx.x;
    SpecState* st = t.st;
    SpecModelState* ms = m.ms;
    TreeState* ts = tt.ts;
    SpecModelTreeState* xs = x.xs;
    const int L = st->L, K = st->n_draft, fin = st->finished, Dc = ms->Dc;
    const int B = ts->n_branch, R = ts->n_rows;
    const int P = L - 1;
    const int* s = t.text + st->n_hint;
    const float T = st->temperature, topp = st->topp, u = st->u;
    const int room = min(st->seq_len - 1 - P, st->max_new - st->n_out - 1);
    const int gap = P - Dc;                                        // 0, or 1 after a step that accepted a leaf of depth cap
    const int cap = fin || gap < 0 || gap > 1 ? 0 : max(min(K, room), 0);
    if (tid == 0) {
        const int mm = spec_model_tree_shape(cap, B, R, s_par, s_dep, s_rank);
        for (int j = mm + 1; j < kSpecRows; j++) { s_par[j] = 0; s_dep[j] = 0; s_rank[j] = 0; }
        for (int d = 0; d < kSpecMaxDraft; d++)
            for (int r = 0; r < kSpecRows; r++) s_lvl[d][r] = -1;
        for (int j = 0; j < kSpecRows; j++) {
            s_rowof[j] = -1;
            for (int r = 0; r < kTreeMaxBranch; r++) xs->child[j][r] = -1;
        }
        int width[kSpecMaxDraft] = {0}, fed = 0;
        for (int j = 0; j <= mm; j++) {
            const int d = s_dep[j];                                // fed by level d + 1, when there is one
            if (j > 0) xs->child[s_par[j]][s_rank[j]] = j;
            if (cap < 1 || d > cap - 1) continue;
            const int r = d == 0 ? gap : width[d]++;               // level 1: the root sits behind the catch-up row
            s_lvl[d][r] = j; s_rowof[j] = r; fed++;
        }
        for (int j = 0; j < kSpecRows; j++) xs->row_of[j] = s_rowof[j];
        xs->cap = cap;
        s_m = mm; s_fed = fed;
        ts->m = mm;
        ts->a = 0;                                                 // an idle step commits nothing
        ts->pos0 = P;
        st->n_d = mm;                                              // spec_pick_kernel picks rows 0..n_d
        st->steps += 1ull;
        if (!fin) { st->rows_fed += (unsigned long long)(mm + 1); st->drafts += (unsigned long long)mm; }
        ms->pick_row = cap > 0 ? gap : -1;
        ms->L0 = L;
        ms->open = !fin;
        if (cap > 0) {
            ms->draft_passes += (unsigned long long)cap;
            ms->draft_rows_fed += (unsigned long long)(fed + gap);
            ms->catch_up_rows += (unsigned long long)gap;
        }
        x.dts->a = 0; x.dts->pos0 = P;
    }
    __syncthreads();
    const int mm = s_m;
    if (tid < kSpecRows) {                                         // the target's pass: rows are nodes
        const bool on = !fin && tid <= mm;
        const int d = on ? s_dep[tid] : 0;
        unsigned long long path = 0ull;
        for (int c = on ? tid : 0, k = d; k >= 0; k--) {           // from the node up to the root: nibble k = the ancestor at depth k
            path |= (unsigned long long)c << (4 * k);
            c = max(s_par[c], 0);
        }
        if (on) { ts->tok[tid] = tid == 0 ? s[P] : -1; ts->parent[tid] = s_par[tid]; ts->depth[tid] = d; }      // (tokens 1..m: the pick kernels)
        if (tid < R) {
            t.rows[tid] = on ? SeqSlot{st->kc, st->vc, P + d, 0} : SeqSlot{nullptr, nullptr, -1, -1};
            tt.anc[tid] = TreeAnc{path, d, 0};
            t.row_tok[tid] = on && tid == 0 ? s[P] : 0;
            t.trow[tid] = ToppRow{on ? T : 0.0f, topp, u, 0, nullptr};
        }
        if (tid >= 1) st->d[tid - 1] = -1;
    }
    if (tid < kSpecMaxDraft * kSpecRows) {                         // the draft levels
        const int lv = tid / kSpecRows, r = tid - lv * kSpecRows;  // level lv + 1 feeds depth lv at position P + lv
        const int node = s_lvl[lv][r];
        const bool catch_up = lv == 0 && r == 0 && gap == 1 && cap > 0;
        const bool on = node >= 0 || catch_up;
        const int d = node >= 0 ? s_dep[node] : 0;
        unsigned long long path = 0ull;
        for (int c = max(node, 0), k = d; k >= 0; k--) {
            path |= (unsigned long long)c << (4 * k);
            c = max(s_par[c], 0);
        }
        const int at = max(catch_up ? P - 1 : P + lv, 0);
        x.rows[tid] = on ? SeqSlot{ms->kc, ms->vc, at, 0} : SeqSlot{nullptr, nullptr, -1, -1};
        x.anc[tid] = TreeAnc{path, d, on && !catch_up ? node : -1};
        x.row_tok[tid] = on && lv == 0 ? s[min(at, P)] : 0;        // (levels 2..: the pick kernels)
        x.trow[tid] = ToppRow{on && !catch_up ? T : 0.0f, topp, u, 0, nullptr};
    }
}

// What ends draft level d, one workgroup per row of the pass: the tokens of the fed node's children.  Rank 0 is Device::sample of the row --
// topp_row_pick, exactly section 8.9's draft --; below a trunk node ranks 1..B - 1 are the first B - 1 tokens by descending key
// (spec_model_tree_key1) with rank 0's token dropped: B - 1 rounds of a workgroup-wide maximum below the round before's.  Each child's token goes
// to TreeState.tok, the target's row token and the row of the next level that feeds the child.
struct SpecModelTreePickParams {
    SpecTables t;
    TreeTables tt;
    SpecModelTreeTables x;
    PickRows r;
    int d;                              // the level, 1..K
};
__global__ __launch_bounds__(1024) void spec_model_tree_pick_kernel(SpecModelTreePickParams p) {
    __shared__ ScanShared sh;
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    __shared__ unsigned long long s_k[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x, d = p.d, at = (d - 1) * kSpecRows + row;
    const int node = p.x.anc[at].pad;
    if (p.x.rows[at].pos < 0 || node < 0) return;                  // an idle row, the catch-up row (uniform: the whole workgroup)
    SpecState* st = p.t.st;
    TreeState* ts = p.tt.ts;
    const SpecModelTreeState* xs = p.x.xs;
    const int B = ts->n_branch;
    const int tok0 = topp_row_pick(p.r, row, st->temperature, st->topp, st->u, sh, s_v, s_i);
    int cand[kTreeMaxBranch] = {tok0, 0, 0, 0};
    if (node == d - 1) {                                           // a trunk node (uniform)
        const float* lg = p.r.logits + (size_t)row * p.r.ld;
        unsigned long long limit = ~0ull;
        for (int rk = 1; rk < B; rk++) {                           // (uniform)
            unsigned long long best = 0ull;
            for (int i = tid; i < p.r.n; i += 1024) {
                const unsigned long long k1 = spec_model_tree_key1(__float_as_uint(lg[i]), i);
                best = i != tok0 && k1 < limit && k1 > best ? k1 : best;
            }
#pragma unroll
            for (int mk = 1; mk < 64; mk <<= 1) {
                const unsigned long long o = __shfl_xor(best, mk);
                best = o > best ? o : best;
            }
            __syncthreads();                                       // (the round before's s_k has been read)
            if (lane == 0) s_k[wave] = best;
            __syncthreads();
            best = s_k[0];
            for (int w = 1; w < 16; w++) best = s_k[w] > best ? s_k[w] : best;
            cand[rk] = best ? (int)(unsigned)((best - 1ull) & 0xffffffffull) : 0;      // (B <= vocab_size: there is one)
            limit = best;
        }
    }
    if (tid != 0) return;
    for (int rk = 0; rk < kTreeMaxBranch; rk++) {
        const int c = xs->child[node][rk];
        if (c < 0) continue;
        const int tok = cand[rk];
        ts->tok[c] = tok;
        p.t.row_tok[c] = tok;                                      // c <= m <= n_rows - 1
        st->d[c - 1] = tok;
        const int rr = xs->row_of[c];                              // fed by level d + 1 <= cap <= 15
        if (rr >= 0 && d < kSpecMaxDraft) p.x.row_tok[d * kSpecRows + rr] = tok;
    }
}

// What closes a step, behind spec_tree_accept_kernel: the fed nodes of the accepted path, depths 1..min(a, cap - 1), carry tokens the accept
// rule made part of s -- the draft commit takes their rows to draft cache positions P + 1 .. and the cursor goes behind them.  A budget or stop
// cut stops the cursor at the new L.
__global__ void spec_model_tree_close_kernel(SpecTables t, SpecModelTables m, TreeTables tt, SpecModelTreeTables x) {
    if (threadIdx.x != 0) return;
    SpecState* st = t.st;
    SpecModelState* ms = m.ms;
    const TreeState* ts = tt.ts;
    TreeState* dts = x.dts;
    const int cap = x.xs->cap;
    dts->a = 0;
    if (!ms->open || cap < 1) return;
    const int keep = max(min(min(ts->a, cap - 1), st->L - ms->L0), 0);
    for (int k = 0; k <= keep; k++) dts->path[k] = ts->path[k];
    dts->a = keep;
    dts->pos0 = ms->L0 - 1;
    ms->Dc = ms->L0 + keep;
}

}  // namespace rama
