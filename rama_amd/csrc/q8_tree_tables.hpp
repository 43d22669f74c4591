// q8_tree_tables.hpp -- the tree chain's device tables and its two rules (q8_tree.hpp has the kernels that work on them): what the host's
// context (ctx.hpp) keeps a copy of, so it holds no kernel.  DESIGN.md section 8.13.
#pragma once

#include "q8_spec_tables.hpp"
#include "ref_order.hpp"       // RefAttnParams

namespace rama {

constexpr int kTreeMaxBranch = 4;       // continuations merged into one tree

// a row's ancestors, beside its SeqSlot: nibble k of `path` is the row that sits k levels below the root on the way to this row (nibble 0 is
// the root, row 0; nibble `depth` the row itself).  The row's timestep P + k, 1 <= k <= depth, is read from that row of the pass.
struct TreeAnc { unsigned long long path; int depth; int pad; };

// the tree of the step under way, the accepted path for the commit, and what rama_q8_spec_tree_stats reports
struct TreeState {
    int m;                              // nodes besides the root
    int a;                              // the accepted path's depth (0 on an idle step: nothing to commit)
    int pos0;                           // the root's position when the step opened
    int n_branch, n_rows;
    int pad_;
    int tok[kSpecRows], parent[kSpecRows], depth[kSpecRows];      // node 0 is the root
    int path[kSpecRows];                // path[k]: the accepted row at depth k (path[0] = 0)
    unsigned long long off_trunk_accepted, off_trunk_steps, nodes_hist[kSpecRows];
};

struct TreeTables {
    TreeState* ts;
    TreeAnc* anc;                       // [kSpecRows]
    float* ks; float* vs;               // the tree store [n_layers][n_rows - 1][dim]: rows 1.. of every layer's rotated k, and v
    int store_rows;                     // n_rows - 1
};

// what attention_tree_kernel needs besides attention_chain_kernel's block: the ancestor records and this layer's rows of the pass
struct TreeAttnParams {
    RefAttnParams a;                    // a.seqs is the row table; a.kc / a.vc are unused
    const TreeAnc* anc;
    const float* kr; const float* v;    // [n_rows, dim] the layer's rotated k and v rows of the pass
};

// THE TRIE (rama_q8_spec_tree_draft on the host, spec_tree_draft_kernel on the device: one statement for both).  Inserts one branch; false once
// n_rows - 1 nodes exist and the branch needs one more: the caller stops everything.
__host__ __device__ inline bool spec_tree_insert(int* tok, int* parent, int* depth, int* m, const int* branch, int len, int n_rows) {
    int cur = 0;
    for (int i = 0; i < len; i++) {
        int c = -1;
        for (int j = 1; j <= *m && c < 0; j++)
            if (parent[j] == cur && tok[j] == branch[i]) c = j;
        if (c < 0) {
            if (*m >= n_rows - 1) return false;
            c = ++*m;
            tok[c] = branch[i]; parent[c] = cur; depth[c] = depth[cur] + 1;
        }
        cur = c;
    }
    return true;
}

// THE ACCEPT RULE over a tree (rama_q8_spec_tree_accept on the host, spec_tree_accept_kernel on the device).  tok / parent: nodes 0..m (node 0 the
// root); picks[0..m].  Walks from the root along the children the picks reproduce; emitted[] gets the picks of the rows visited, cut at the
// budget (`remaining` >= 1) and after the first token equal to `stop`; path[k] = the row visited at depth k, *a = the depth reached.
// Returns the tokens emitted (>= 1).
__host__ __device__ inline int spec_tree_accept_rule(const int* tok, const int* parent, int m, const int* picks, int stop, int remaining, int* path,
                                                     int* emitted, int* a, int* finished) {
    int cur = 0, emit = 0, k = 0;
    path[0] = 0;
    emitted[emit++] = picks[0];
    while (emitted[emit - 1] != stop && emit < remaining) {
        int c = -1;
        for (int j = 1; j <= m && c < 0; j++)
            if (parent[j] == cur && tok[j] == emitted[emit - 1]) c = j;
        if (c < 0) break;
        cur = c;
        path[++k] = c;
        emitted[emit++] = picks[c];
    }
    *a = k;
    *finished = emit >= remaining || emitted[emit - 1] == stop;
    return emit;
}

// ---------------------------------------------------------------- trees from a draft model (q8_spec_model_tree.hpp)

// THE SHAPE (rama_q8_spec_model_tree_shape on the host, spec_model_tree_open_kernel on the device: one statement for both), a pure function of
// (cap, n_branch, n_rows): the trunk 1..min(cap, n_rows - 1) first, then level by level every node of the level above in ascending index -- a
// trunk node (index == depth, the root included) gets side children of ranks 1..n_branch - 1, any other node one child of rank 0 -- until
// n_rows - 1 nodes exist.  parent / depth / rank: nodes 0..m (node 0 the root).  Returns m.
__host__ __device__ inline int spec_model_tree_shape(int cap, int n_branch, int n_rows, int* parent, int* depth, int* rank) {
    int m = 0;
    parent[0] = -1; depth[0] = 0; rank[0] = 0;
    for (int d = 1; d <= cap && m < n_rows - 1; d++) { m = d; parent[d] = d - 1; depth[d] = d; rank[d] = 0; }
    for (int d = 1; d <= cap && m < n_rows - 1; d++) {
        const int have = m;                                       // (the nodes of depth d - 1 all exist: the trunk's, or made one level up)
        for (int p = 0; p <= have && m < n_rows - 1; p++) {
            if (depth[p] != d - 1) continue;
            if (p == depth[p]) {
                for (int r = 1; r < n_branch && m < n_rows - 1; r++) { ++m; parent[m] = p; depth[m] = d; rank[m] = r; }
            } else { ++m; parent[m] = p; depth[m] = d; rank[m] = 0; }
        }
    }
    return m;
}

// THE CANDIDATE ORDER of ranks 1..: a token's 64-bit key -- the logit's bits mapped monotonically to unsigned (the sign-flip map; a NaN lands
// where its bits put it) above the token index --, PLUS ONE so that 0 means "none".  Descending: the larger logit first, on ties the higher
// index, the argmax's own tie rule.
__host__ __device__ inline unsigned long long spec_model_tree_key1(unsigned bits, int index) {
    const unsigned hi = bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
    return (((unsigned long long)hi << 32) | (unsigned long long)(unsigned)index) + 1ull;
}

// the step under way on the draft model's side, next to SpecModelState (Dc, L0, open and the counters are that record's)
struct SpecModelTreeState {
    int cap;                            // the step's depth bound (0: every draft row idle)
    int pad_;
    int child[kSpecRows][kTreeMaxBranch];      // node p's child of rank r (-1: none)
    int row_of[kSpecRows];              // the row of the draft pass that feeds the node (-1: a node that is not fed)
};

struct SpecModelTreeTables {
    SpecModelTreeState* xs;
    SeqSlot* rows;                      // [kSpecMaxDraft][kSpecRows] level d's row table at (d - 1) kSpecRows (idle: position -1)
    int* row_tok;                       // [kSpecMaxDraft][kSpecRows]
    ToppRow* trow;                      // [kSpecMaxDraft][kSpecRows] temperature 0 but for a row that feeds a node
    TreeAnc* anc;                       // [kSpecMaxDraft][kSpecRows] nibbles are NODES; pad = the node the row feeds (-1: the catch-up row, an idle row)
    TreeState* dts;                     // the draft commit's record: a = min(a, cap - 1), the path, pos0
    float* ks; float* vs;               // the draft tree store [dn_layers][n_rows - 1][ddim]: row node - 1
    int store_rows;
};

}  // namespace rama
