// q8_serve_spec_tables.hpp -- what a serving chain begun with rama_q8_serve_begin_spec keeps next to ServeTables (q8_serve_spec.hpp has the
// kernels that work on them): what the host's context (ctx.hpp) keeps a copy of, so it holds no kernel
#pragma once

#include "q8_serve_tables.hpp"
#include "q8_spec_tables.hpp"   // kSpecMaxDraft, kSpecRows, spec_accept_rule

namespace rama {

// a slot's drafting fields: parallel to ServeSlot, which stays as it is (also the head of a spec admission record, followed by the hint)
struct ServeSpecSlot {
    int n_draft, ngram, n_hint;         // the admission's: drafts per step at most (0: none), the longest tail looked up, hint tokens
    int want;                           // serve_draft_kernel: the drafts the slot has for this step
    int granted;                        // serve_spec_schedule_kernel: those that got a row
    int row0;                           // ... and the slot's first row
    int pad_[2];
    int d[kSpecRows];                   // the step's drafts d[0..want)
};
static_assert(sizeof(ServeSpecSlot) == 96, "a spec admission record is a ServeSpecSlot followed by the hint tokens");

// what serve_spec_accept_kernel sums per slot over the chain's life (an admission does not reset it; the host adds the slots up)
struct ServeSpecSums {
    unsigned long long granted, accepted, emitted;      // drafts judged, drafts the picks reproduced, tokens recorded
    unsigned long long hist[kSpecRows];                 // DECODE slot-steps by the number of drafts accepted
};

struct ServeSpecTables {
    ServeSpecSlot* ss;                  // [n_slots]
    int* hint;                          // [n_slots][hint_cap] every slot's hint text
    int hint_cap;
    int* picks;                         // [max_rows] Device::sample of every row that carries logits
    int* lflag;                         // [max_rows] 1: the row is classified and picked
    ToppRow* rrow;                      // [max_rows] the sampler's record of the step, per ROW: temperature 0 unless the row samples
    ServeSpecSums* sums;                // [n_slots]
    unsigned long long* sched;          // the scheduler's: draft rows, drafts wanted
};

}  // namespace rama
