// q8_serve_model_tables.hpp -- what a serving chain begun with rama_q8_serve_begin_model keeps next to ServeTables and ServeSpecTables
// (q8_serve_model.hpp has the kernels that work on them): what the host's context (ctx.hpp) keeps a copy of, so it holds no kernel
#pragma once

#include "q8_serve_spec_tables.hpp"

namespace rama {

// a slot's draft side: parallel to ServeSlot and ServeSpecSlot, which stay as they are
struct ServeModelSlot {
    float* kc; float* vc;               // the draft run state's cache bases
    int Dc;                             // the draft cursor: rows 0..Dc-1 of the draft cache belong to the slot's text
    int L0;                             // the step under way: L when it opened
    int open;                           // ... 1: the slot was DECODE with n_draft > 0, and the first draft pass feeds s[Dc..P]
    int pick_row;                       // ... the row of the first draft pass whose logits give d[0]
    int n_live;                         // ... the live rows of the first draft pass: 1, or 2 with a catch-up row
    int pad_;
    unsigned long long draft_passes, draft_rows_fed, catch_up_rows;      // summed over the chain's life (the host adds the slots up)
};

struct ServeModelTables {
    ServeModelSlot* ms;                 // [n_slots]
    SeqSlot* rows0;                     // [2 n_slots] the first draft pass's row table: slot i's rows 2i, 2i + 1 (idle: position -1)
    int* row_tok0;                      // [2 n_slots]
    ToppRow* trow0;                     // [2 n_slots] temperature 0 but for a row whose logits are picked from
    SeqSlot* rows;                      // [n_slots] the row table of every later draft pass: slot i's row i
    int* row_tok;                       // [n_slots]
    ToppRow* trow;                      // [n_slots]
};

}  // namespace rama
