// q8_serve_tables.hpp -- the serving chain's device tables (q8_serve.hpp has the kernels that work on them): what the host's context
// (ctx.hpp) keeps a copy of, so it holds no kernel
#pragma once

#include "kernels.hpp"          // SeqSlot
#include "topp_sort.hpp"        // ToppRow

namespace rama {

constexpr int kServeMaxSlots = 128;
constexpr int kServeFree = 0, kServePrompt = 1, kServeDecode = 2, kServeDone = 3;

// a slot of the device table (64 bytes; also the head of an admission record, followed by the context tokens)
struct ServeSlot {
    float* kc; float* vc;              // the sequence's cache bases
    int state;
    int n_ctx;                         // context tokens, fed at positions 0 .. n_ctx - 1
    int cursor;                        // PROMPT: the next context position to feed; DECODE: the position `tok` is fed at
    int tok;                           // DECODE: the token to feed
    int n_out;                         // tokens produced
    int max_new, stop;                 // the budget; the token whose sampling ends the sequence (-1: none)
    int gen;                           // the admission's generation number
    float temperature, topp, u;
    int pad_;
};
static_assert(sizeof(ServeSlot) == 64, "an admission record is a ServeSlot followed by the context tokens");

struct ServeTables {
    ServeSlot* slots;                  // [n_slots]
    int* ctx;                          // [n_slots][seq_len] every slot's context tokens
    int seq_len, n_slots, max_rows;
    SeqSlot* rows;                     // [max_rows] the step's row table; pad = the slot (-1: idle)
    int* row_tok;                      // [max_rows]
    int* nrows;                        // [n_slots] rows the slot has in this step
    int* lrow;                         // [n_slots] its row that carries logits (-1: none this step)
    ToppRow* trow;                     // [n_slots] the sampler's record of the step: temperature 0 unless the slot samples now
    unsigned long long* counters;      // steps, decode rows, prompt rows, idle rows
    int* out; int* ring; int* done;    // [n_slots][out_cap] tokens; the same host-visible (token + 1); [n_slots] finished words
    int out_cap;
};

}  // namespace rama
