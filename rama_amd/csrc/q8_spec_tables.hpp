// q8_spec_tables.hpp -- the speculative chain's device tables, its accept rule and the lookup's scan (q8_spec.hpp has the kernels that work on
// them; the serving chain's drafting kernel of q8_serve_spec.hpp scans the same way): what the host's context (ctx.hpp) keeps a copy of, so it holds no kernel
#pragma once

#include "kernels.hpp"          // SeqSlot
#include "topp_sort.hpp"        // ToppRow

namespace rama {

constexpr int kSpecMaxDraft = 15;       // drafts per step: a pass of up to 16 rows is one 16-token tile of the K-split product
constexpr int kSpecRows = kSpecMaxDraft + 1;
constexpr int kSpecMaxNgram = 4;
constexpr int kSpecHintBit = 1 << 30;   // spec_draft_kernel's match key: an occurrence in the hint beats every one in the sequence

// the sequence on the device (one record; the counters are what rama_q8_spec_stats reports)
struct SpecState {
    float* kc; float* vc;               // the sequence's cache bases
    int L;                              // known tokens s[0..L): s[L - 1] is fed next, at position L - 1
    int n_out;                          // tokens emitted
    int finished;
    int n_d;                            // drafts of the step under way
    int max_new, stop;                  // the budget; the token whose sampling ends the sequence (-1: none)
    int n_draft, ngram, n_hint, seq_len;
    float temperature, topp, u;
    int pad_;
    unsigned long long steps, rows_fed, drafts, accepted, emitted, hist[kSpecRows];
    int d[kSpecRows];                   // the step's drafts (-1 behind n_d)
    int picks[kSpecRows];               // Device::sample of rows 0..n_d
};

struct SpecTables {
    SpecState* st;
    int* text;                          // [n_hint + seq_len] the hint, then the sequence s
    SeqSlot* rows;                      // [kSpecRows] the step's row table (n_draft + 1 entries used; idle: position -1)
    int* row_tok;                       // [kSpecRows]
    ToppRow* trow;                      // [kSpecRows] the sampler's record of the step: temperature 0 for an idle row
    int* out;                           // [max_new] the tokens emitted
    int* ring;                          // the same host-visible (token + 1)
    int* count; int* done;              // host-visible: tokens emitted, stored after their ring words; the finished word, stored after both
};

// a chain begun with rama_q8_spec_begin_model (q8_spec_model.hpp): the draft model's side of the sequence, next to the record above
struct SpecModelState {
    float* kc; float* vc;               // the draft run state's cache bases
    int Dc;                             // the draft cursor: rows 0..Dc-1 of the draft cache belong to s
    int pick_row;                       // the step under way: the row of the first draft pass whose logits give d[0] (-1: every draft row is idle)
    int L0;                             // ... L when it opened
    int open;                           // ... 1: it opened on an unfinished sequence
    unsigned long long draft_passes, draft_rows_fed, catch_up_rows;
};

constexpr int kSpecModelRows = 2;       // rows of the first draft pass: the catch-up row and s[L - 1]; every later pass has one

struct SpecModelTables {
    SpecModelState* ms;
    SeqSlot* rows;                      // [kSpecModelRows] the row table of the draft pass under way (idle: position -1)
    int* row_tok;                       // [kSpecModelRows]
    ToppRow* trow;                      // [kSpecModelRows] temperature 0 but for the row whose logits are picked from
};

// THE ACCEPT RULE (rama_q8_spec_accept on the host, spec_accept_kernel on the device: one statement for both).  *a: the drafts the picks
// reproduce, from the front; pick_0 .. pick_a are emitted, cut at the budget (`remaining` >= 1 tokens) and after the first emitted token
// equal to `stop`; either cut finishes the sequence.  Returns the tokens emitted (>= 1).
__host__ __device__ inline int spec_accept_rule(const int* drafts, int n_d, const int* picks, int stop, int remaining, int* a, int* finished) {
    int k = 0;
    while (k < n_d && picks[k] == drafts[k]) k++;
    *a = k;
    int emit = k + 1 < remaining ? k + 1 : remaining;
    int fin = emit >= remaining;
    for (int j = 0; j < emit; j++)
        if (picks[j] == stop) { emit = j + 1; fin = 1; break; }
    *finished = fin;
    return emit;
}

// THE LOOKUP'S SCAN (spec_draft_kernel, serve_draft_kernel): the latest end e in [n, hi] (exclusive end: text[e - n .. e) equals the tail) among
// this thread's candidates, as a key; -1: none.
// Every load is made -- index clamped into the text -- and the comparison selected afterwards: no branch around a load.
__device__ __forceinline__ int spec_scan_text(const int* text, int hi, int n, const int (&tail)[kSpecMaxNgram], int key_bit, int best) {
    for (int e = n + (int)threadIdx.x; e <= hi; e += (int)blockDim.x) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < kSpecMaxNgram; i++) {
            const int v = text[min(e - n + i, e - 1)];            // e >= n >= 1: [e - n, e - 1] is inside the text
            ok = ok && (i >= n || v == tail[i]);
        }
        best = ok ? max(best, key_bit | e) : best;
    }
    return best;
}

}  // namespace rama
