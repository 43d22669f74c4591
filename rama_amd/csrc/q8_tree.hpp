// q8_tree.hpp -- TREE DRAFTS for the speculative chain of a Q8 model (rama_q8_spec_begin_tree, rama_q8_tree_forward / _commit, DESIGN.md
// section 8.13): up to four continuations of the tail n-gram share their common prefix in one pass of up to 16 rows.  Two nodes at one depth
// sit at one position, so only the root writes its cache row during the pass; every other row's k and v stay in the pass's own rows, and a row's
// attention takes each timestep behind the root from the ancestor of that depth.  Every step
//   spec_tree_draft_kernel   spec_draft_kernel's scan n_branch times (round b: the largest key below round b - 1's), the trie, the row table,
//                            the ancestor records, the row tokens, the sampler records
//   the batched pass         q8_batch_layers with q8_rope_tree_kernel (q8_batch.hpp) and attention_tree_kernel in place of the two launches that touch the cache
//   spec_pick_kernel         (q8_spec.hpp, unchanged: rows 0..m)
//   spec_tree_accept_kernel  the accept rule over the tree, the ring / count / finished words as spec_accept_kernel stores them, the path
//   tree_commit_kernel       the path's rows from the tree store to cache positions P + 1 .. P + a, every layer
// This header serves two translation units (DESIGN.md "Translation units"): attention_tree_kernel is built from chain.hpp's pieces and lives
// with them in chain_api.hip (the half under RAMA_CHAIN_HPP); the drafts, the accept rule and the commit live in q8_spec_api.hip, which must not see chain.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "q8_tree_tables.hpp"

namespace rama {

#ifdef RAMA_CHAIN_HPP
// ---------------------------------------------------------------- cpu.rs:23-52 multi_head_attention over a tree row
// attention_chain_body's operations in its order per output -- the score chains in index order, / sqrtf(hs); max, expf_glibc_tab,
// seq_sum_cascade over pos + 1 terms, divide; the products a * v rounded, added in ascending t -- with one difference: where a timestep's
// row comes from.  t <= P (the root's position) is cache row t; t = P + k is row path[k] of the pass.  Both addresses are formed, one is
// selected, the load is issued: no branch around a load, and both bases are global address space.
#define RAMA_TREE_ROW(nib) (nib)
template <int NW>
__global__ __launch_bounds__(NW * 64) void attention_tree_kernel(TreeAttnParams tp) {
#include "q8_tree_attn_body.hpp"
}
#undef RAMA_TREE_ROW

// The same over one level of a DRAFT MODEL's tree (q8_spec_model_tree.hpp): tp.kr / tp.v are the layer's slice of the draft tree
// store, the path's nibbles are NODES, and node n sits in store row n - 1 (the root's nibble is never selected: t <= P is the cache's).
#define RAMA_TREE_ROW(nib) max((nib) - 1, 0)
template <int NW>
__global__ __launch_bounds__(NW * 64) void attention_draft_tree_kernel(TreeAttnParams tp) {
#include "q8_tree_attn_body.hpp"
}
#undef RAMA_TREE_ROW

#else  // ---------------------------------------------------------------- the drafts, the accept rule and the commit: q8_spec_api.hip's half
#define RAMA_Q8_TREE_HPP 1      // (q8_api.hip and q8_serve_api.hip refuse to be compiled with this half: its kernels are q8_spec_api.hip's)

// (q8_rope_tree_kernel is the pass's kernel, launched from q8_batch_layers: q8_batch.hpp, beside q8_rope_batch_kernel)

// The commit: row path[k] of the store -> cache position pos0 + k for k = 1..a, every layer.  Grid (n_layers, 15): the path and a are read from
// the chain state, so the launch is the same whatever was accepted.
struct TreeCommitParams {
    const TreeState* ts;
    float* kc; float* vc;               // the sequence's cache bases
    const float* ks; const float* vs;
    int dim, seq_len, store_rows;
};
__global__ __launch_bounds__(256) void tree_commit_kernel(TreeCommitParams p) {
    const int l = blockIdx.x, k = blockIdx.y + 1;
    const TreeState* ts = p.ts;
    if (k > ts->a) return;                                        // (uniform: the whole workgroup)
    const int r = ts->path[k];                                    // 1..store_rows
    const size_t src = ((size_t)l * p.store_rows + (size_t)(r - 1)) * p.dim;
    const size_t dst = ((size_t)l * p.seq_len + (size_t)(ts->pos0 + k)) * p.dim;
    for (int i = threadIdx.x; i < p.dim / 4; i += blockDim.x) {
        reinterpret_cast<f4*>(p.kc + dst)[i] = reinterpret_cast<const f4*>(p.ks + src)[i];
        reinterpret_cast<f4*>(p.vc + dst)[i] = reinterpret_cast<const f4*>(p.vs + src)[i];
    }
}

// spec_scan_text (q8_spec_tables.hpp) with a ceiling: the largest key below `limit` among this thread's candidates
__device__ __forceinline__ int spec_tree_scan_text(const int* text, int hi, int n, const int (&tail)[kSpecMaxNgram], int key_bit, int limit, int best) {
    for (int e = n + (int)threadIdx.x; e <= hi; e += (int)blockDim.x) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < kSpecMaxNgram; i++) {
            const int v = text[min(e - n + i, e - 1)];            // e >= n >= 1: [e - n, e - 1] is inside the text
            ok = ok && (i >= n || v == tail[i]);
        }
        const int key = key_bit | e;
        best = ok && key < limit ? max(best, key) : best;
    }
    return best;
}

__global__ __launch_bounds__(1024) void spec_tree_draft_kernel(SpecTables t, TreeTables tt) {
    __shared__ int s_best[16];
    __shared__ int s_keys[kTreeMaxBranch], s_br[kTreeMaxBranch][kSpecMaxDraft], s_tok[kSpecRows], s_par[kSpecRows], s_dep[kSpecRows], s_m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SpecState* st = t.st;
    TreeState* ts = tt.ts;
    const int L = st->L, n_hint = st->n_hint, K = st->n_draft, fin = st->finished;
    const int B = ts->n_branch, R = ts->n_rows;
    const int P = L - 1;
    const int* hint = t.text;
    const int* s = t.text + n_hint;
    const int room = min(st->seq_len - 1 - P, st->max_new - st->n_out - 1);
    const int cap = fin ? 0 : max(min(K, room), 0);
    int nb = 0;
    if (cap > 0) {                                                 // (uniform, as everything that decides a barrier below)
        for (int n = min(st->ngram, L); n >= 1 && nb == 0; n--) {
            int tail[kSpecMaxNgram];
#pragma unroll
            for (int i = 0; i < kSpecMaxNgram; i++) tail[i] = s[min(L - n + i, L - 1)];
            int limit = 0x7fffffff;
            for (int b = 0; b < B; b++) {                          // round b: the largest key strictly below round b - 1's
                int best = spec_tree_scan_text(hint, n_hint, n, tail, kSpecHintBit, limit, -1);
                best = spec_tree_scan_text(s, L - 1, n, tail, 0, limit, best);
                best = wave_max_i(best);
                if (lane == 0) s_best[wave] = best;
                __syncthreads();
                int key = s_best[0];
                for (int w = 1; w < (int)(blockDim.x >> 6); w++) key = max(key, s_best[w]);
                __syncthreads();
                if (key < 0) break;                                // (uniform) fewer occurrences than branches
                if (tid == 0) s_keys[nb] = key;
                nb++; limit = key;
            }
        }
    }
    __syncthreads();
    // the branches' tokens, one per thread (index clamped into the text, the value selected afterwards), then the trie in LDS by one thread:
    // at most 4 x 15 insertions, one statement with the host's
    if (tid < kTreeMaxBranch * kSpecMaxDraft) {
        const int b = tid / kSpecMaxDraft, i = tid - b * kSpecMaxDraft;
        const int key = s_keys[min(b, max(nb - 1, 0))];
        const bool in_hint = (key & kSpecHintBit) != 0;
        const int e = key & (kSpecHintBit - 1), len_text = in_hint ? n_hint : L;
        const bool on = b < nb && i < min(cap, len_text - e);
        const int v = (in_hint ? hint : s)[on ? e + i : 0];       // (s[0] exists: L >= 1)
        s_br[b][i] = on ? v : -1;
    }
    if (tid == 0) { s_tok[0] = s[L - 1]; s_par[0] = -1; s_dep[0] = 0; }
    __syncthreads();
    if (tid == 0) {
        int m = 0;
        for (int b = 0; b < nb; b++) {
            int len = 0;
            while (len < kSpecMaxDraft && s_br[b][len] >= 0) len++;
            if (!spec_tree_insert(s_tok, s_par, s_dep, &m, s_br[b], len, R)) break;
        }
        s_m = m;
        ts->m = m;
        ts->a = 0;                                                 // an idle step commits nothing
        ts->pos0 = P;
        st->n_d = m;                                               // spec_pick_kernel picks rows 0..n_d
        st->steps += 1ull;
        if (!fin) { st->rows_fed += (unsigned long long)(m + 1); st->drafts += (unsigned long long)m; }
    }
    __syncthreads();
    if (tid < kSpecRows) {
        const int m = s_m;
        const bool on = !fin && tid <= m;
        const int d = on ? s_dep[tid] : 0;
        unsigned long long path = 0ull;
        for (int c = on ? tid : 0, k = d; k >= 0; k--) {           // from the node up to the root: nibble k = the ancestor at depth k
            path |= (unsigned long long)c << (4 * k);
            c = max(s_par[c], 0);
        }
        const int tok = on ? s_tok[tid] : 0;
        if (on) { ts->tok[tid] = tok; ts->parent[tid] = s_par[tid]; ts->depth[tid] = d; }
        if (tid < R) {                                             // R <= kSpecRows rows
            t.rows[tid] = on ? SeqSlot{st->kc, st->vc, P + d, 0} : SeqSlot{nullptr, nullptr, -1, -1};
            tt.anc[tid] = TreeAnc{path, d, 0};
            t.row_tok[tid] = tok;
            t.trow[tid] = ToppRow{on ? st->temperature : 0.0f, st->topp, st->u, 0, nullptr};
        }
        if (tid >= 1) st->d[tid - 1] = on ? tok : -1;
    }
}

// What ends a step: spec_accept_kernel's stores in its order and at its scopes, over the tree rule; the path stays behind for the commit.
__global__ void spec_tree_accept_kernel(SpecTables t, TreeTables tt) {
    if (threadIdx.x != 0) return;
    SpecState* st = t.st;
    TreeState* ts = tt.ts;
    if (st->finished) return;
    const int n_out = st->n_out, L = st->L, m = ts->m;
    int a, fin, toks[kSpecRows], path[kSpecRows];
    const int emit = spec_tree_accept_rule(ts->tok, ts->parent, m, st->picks, st->stop, st->max_new - n_out, path, toks, &a, &fin);
    int* s = t.text + st->n_hint;
    for (int i = 0; i < emit; i++) {                               // L + emit <= n_context + max_new <= seq_len; n_out + emit <= max_new
        const int tok = toks[i];
        s[L + i] = tok;
        t.out[n_out + i] = tok;
        __hip_atomic_store(t.ring + n_out + i, tok + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    st->L = L + emit;
    st->n_out = n_out + emit;
    __hip_atomic_store(t.count, n_out + emit, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);      // (after the ring words)
    if (fin) {
        st->finished = 1;
        __hip_atomic_store(t.done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);              // (after the count)
    }
    st->accepted += (unsigned long long)a;
    st->emitted += (unsigned long long)emit;
    st->hist[a] += 1ull;
    int off = 0;
    for (int k = 0; k <= a; k++) { ts->path[k] = path[k]; off += path[k] != k; }      // a node with index != depth is off the trunk
    ts->a = a;
    ts->off_trunk_accepted += (unsigned long long)off;
    ts->off_trunk_steps += off ? 1ull : 0ull;
    ts->nodes_hist[m] += 1ull;
}

#endif  // RAMA_CHAIN_HPP

}  // namespace rama
