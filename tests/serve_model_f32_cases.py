"""The cases of tests/test_hip_serve_model.py and tests/test_serve_model_f32_host.py: the parity-mode serving chain with a Q8 draft model
(rama_serve_begin_model).  The one-tile workloads are tests/serve_model_cases.py's; here are the draft shapes and the workloads that need
the second tile of a parity pass.  No GPU, nothing of rama_amd imported."""
from tests.serve_model_cases import ARRIVALS, GREEDY, HOLE, ONE, SAMPLED  # noqa: F401  (the one-tile workloads: re-exported)

TILE = 32

# the small unrelated draft of a target: a synthetic Q8 model of another shape over the target's vocabulary (seq_len: the target's)
SMALL_DRAFT = dict(dim=32, hidden_dim=64, n_layers=1, n_heads=2, n_kv_heads=2, shared_weight=True)
SMALL_GS, SMALL_SEED = 32, 41

# A workload: (n_slots, max_rows, use_slots, requests); a request: (n_context, max_new, n_draft, sampler, stop_at), as in serve_model_cases.
# TWO_TILES: 4 slots x 40 rows.  Step 0 feeds the three contexts (7 rows); from step 1 on the slots want 7, 15 and 15 drafts: rows 0..7, 8..23
# and 24..39 -- exactly the 40 rows, and slot 2's straddle row 32.  Slot 3 stays FREE.
TWO_TILES = (4, 40, [0, 1, 2], [(2, 30, 7, GREEDY, None), (3, 30, 15, SAMPLED, None), (2, 30, 15, GREEDY, None)])
# WIDE16: 16 slots x 32 rows, every slot drafting from step 1 on: the first draft pass carries a row (or two) of every slot, and the 16 rows the
# slots leave are shared out in slot order
WIDE16 = (16, 32, None, [(1 + i % 3, 5 + i % 4, (1, 2, 7, 15)[i % 4], (GREEDY, SAMPLED)[i % 2], None) for i in range(16)])
# GUARD: 2 slots x 40 rows: slot 0 decodes without drafts while slot 1 feeds a context of 50 tokens -- in step 0 tile 1 holds only rows inside
# that context (a live tile without a logits row); from step 1 on it is wholly idle
GUARD = (2, 40, None, [(1, 6, 0, GREEDY, None), (50, 3, 2, GREEDY, None)])


# the seeds of the workloads' contexts (BOS, then default_rng(seed) tokens in [2, vocab)): the GPU tests and the host replay use the same
SEEDS = dict(ONE=3, HOLE=3, ARRIVALS=3, TWO_TILES=3, WIDE16=3, GUARD=5)
TARGET_SEED = 23                 # the synthetic TINY target's (tests/test_hip_serve.py SEED)


def contexts(workload, vocab, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    return [[1] + [int(t) for t in rng.integers(2, vocab, n_ctx - 1)] for n_ctx, _, _, _, _ in workload[3]]


def conditions(rp):
    """which of the eight coverage conditions a replay shows: the five outcomes of a drafting slot-step, and the three of the second tile"""
    seen = set()
    for st in rp["steps"]:
        for slot, (g, a, emit, catch_up) in st["drafting"].items():
            if g > 0 and a == 0:
                seen.add("a == 0")
            if a == g > 0:
                seen.add("a == g > 0")
            if 0 < a < g:
                seen.add("0 < a < g")
            if 0 < g < st["want"][slot]:
                seen.add("0 < g < want")
            if g == 0 and catch_up:
                seen.add("g == 0 with a live catch-up row")
        rows = st["rows"]
        if len(rows) > TILE:
            if straddles(rows):
                seen.add("a DECODE slot across row 32")
            tail = rows[TILE:]
            if any(s >= 0 for s, _, _ in tail) and not any(lg for _, _, lg in tail):
                seen.add("a live second tile without a logits row")
            if all(s < 0 for s, _, _ in tail):
                seen.add("a wholly idle second tile")
    return seen


ALL_CONDITIONS = {"a == 0", "a == g > 0", "0 < a < g", "0 < g < want", "g == 0 with a live catch-up row", "a DECODE slot across row 32",
                  "a live second tile without a logits row", "a wholly idle second tile"}


def straddles(rows):
    """a DECODE slot with drafts (two rows or more, every one carrying logits) has rows on both sides of row 32 of this step's table"""
    flags = {}
    for s, _, lg in rows:
        if s >= 0:
            flags.setdefault(s, []).append(lg)
    drafting = {s for s, f in flags.items() if len(f) >= 2 and all(f)}
    return bool({s for s, _, _ in rows[:TILE]} & {s for s, _, _ in rows[TILE:]} & drafting)
