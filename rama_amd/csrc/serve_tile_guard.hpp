// serve_tile_guard.hpp -- the one kernel the fp32 serving chain adds for a step with drafts (rama_serve_begin_spec).  In parity
// mode every classifier tile is a full pass over wcls, so a tile of kGcMaxTok rows none of which carries logits -- wholly idle, or holding only
// rows inside a context -- must not be classified at all.  One workgroup behind the scheduler reads the step's per-row logits flags and writes one
// guard entry per tile: a SeqSlot whose pos is -1 when no row of the tile is flagged, else 0.  The tile's final-norm and classifier launches get
// that entry as their row table, and the guard they already have (chain.hpp: a scalar test on the argument before the first load) skips the tile.
// batch_api.hip instantiates it; nothing else does.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.hpp"          // SeqSlot
#include "chain_params.hpp"     // kGcMaxTok
#include "q8_serve_tables.hpp"  // kServeMaxSlots: a step has at most as many rows

namespace rama {

constexpr int kTileGuardThreads = kServeMaxSlots;      // one thread per row of the longest table
static_assert(kGcMaxTok == 32 && kTileGuardThreads % 64 == 0, "a wave of 64 rows holds exactly two tiles of 32");

__global__ __launch_bounds__(kTileGuardThreads) void serve_tile_guard_kernel(const int* lflag, int max_rows, SeqSlot* guard) {
    const int r = threadIdx.x;
    const int f = lflag[min(r, max_rows - 1)];                     // the load is made, at an index inside the table, and the flag selected afterwards
    const bool on = r < max_rows && f != 0;
    const unsigned long long wave_rows = __ballot(on);            // bit l: row (r & ~63) + l carries logits
    const unsigned tile_rows = (unsigned)(wave_rows >> (r & 32));  // the 32 rows of this thread's tile
    if ((r & (kGcMaxTok - 1)) == 0 && r < max_rows) guard[r / kGcMaxTok] = SeqSlot{nullptr, nullptr, tile_rows ? 0 : -1, 0};
}

}  // namespace rama
