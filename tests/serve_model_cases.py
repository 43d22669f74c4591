"""The cases of tests/test_q8_serve_model_host.py and tests/test_hip_q8_serve_model.py: the serving chain with a draft model
(rama_q8_serve_begin_model).  The (target <- draft) pairs are tests/spec_model_cases.py's; here are the geometries, the workloads and
a row-by-row restatement of the step's schedule.  No GPU, nothing of rama_amd imported."""
from tests.spec_model_cases import PAIRS  # noqa: F401  (the pairs: re-exported)

FREE, PROMPT, DECODE, DONE = 0, 1, 2, 3

# (n_slots, max_rows) of the host plan's random tables
PLAN_SHAPES = [(1, 1), (4, 8), (16, 16), (64, 128)]

GREEDY, SAMPLED, COOL = (0.0, 0.9, 0.0), (1.0, 0.9, 0.4), (0.7, 1.0, 0.3)      # (temperature, topp, u)

# A workload: (n_slots, max_rows, use_slots, requests); a request: (n_context, max_new, n_draft, sampler, stop_at) -- stop_at = the index of
# the solo run's token that becomes the stop token (None: no stop).  Requests are admitted in order into the usable slots that are FREE or
# DONE before every step, so a request behind the n_slots-th arrives while the others decode.
#
# ONE: 1 slot x 1 row.  There is never an idle row: g == 0 on every step, the pure catch-up path -- and the draft cache still follows.
ONE = (1, 1, None, [(3, 6, 7, GREEDY, None), (1, 4, 2, SAMPLED, None)])
# HOLE: 3 slots x 8 rows around a FREE hole (slot 1 is never used).
HOLE = (3, 8, [0, 2], [(2, 9, 7, GREEDY, None), (4, 7, 2, SAMPLED, None), (1, 5, 15, COOL, None)])
# ARRIVALS: 4 slots x 16 rows, prompts arriving while others decode so that grants are cut.  On a pair of one model with itself: request 0
# accepts all 7 drafts of step 1 (its draft cursor falls one behind); request 1 finishes in step 1, request 4 -- a context of 21 tokens --
# takes its slot in step 2 and, with the other first rows, every row of that step: request 0 is granted nothing and feeds its catch-up row
# (g == 0 with a live catch-up row); in step 3 the prompt leaves rows for some of what the decoding slots want (0 < g < want).  Request 3 stops
# on the third token of its solo run, inside an accepted run; request 2's budget ends inside an accepted run.
ARRIVALS = (4, 16, None, [(2, 25, 7, GREEDY, None), (1, 2, 0, GREEDY, None), (3, 11, 15, SAMPLED, None), (2, 9, 7, COOL, 2),
                          (21, 2, 1, GREEDY, None), (5, 6, 2, SAMPLED, None)])
# the same geometry at the sizes of the draft model of untied <- tied (seq_len 16): n_context + max_new <= 16
ARRIVALS_SHORT = (4, 16, None, [(2, 13, 7, GREEDY, None), (1, 2, 0, GREEDY, None), (3, 9, 15, SAMPLED, None), (2, 8, 7, COOL, 2),
                                (13, 2, 1, GREEDY, None), (5, 6, 2, SAMPLED, None)])
# WIDE: 64 slots x 128 rows on the smallest fixture: the first draft pass is full (2 x 64 rows)
WIDE = (64, 128, None, [(1 + i % 3, 4 + i % 4, (1, 2, 7, 15)[i % 4], (GREEDY, SAMPLED)[i % 2], None) for i in range(64)])

# the near-copy pair's request (spec_model_cases: the context seed chosen for a sampled run in which the draft is right once and wrong next)
NEAR_CONTEXT_SEED, NEAR_REQUEST = 7, (9, 24, 7, SAMPLED, None)


def plan_py(slots, n_draft, draft_cursor, max_rows, seq_len, n_passes):
    """the step's schedule, row by row: -> (rows, want, granted, passes) as rama_amd.q8.serve_model_plan_step gives them"""
    n = len(slots)
    drafting = [s[0] == DECODE and n_draft[i] > 0 for i, s in enumerate(slots)]
    want = [max(min(n_draft[i], seq_len - 1 - s[2], s[4] - s[3] - 1), 0) if drafting[i] else 0 for i, s in enumerate(slots)]
    # rule 1-2: a row per DECODE and per PROMPT slot; rule 3: the rows left to the prompts, in slot order; rule 3a: then to the drafts
    nrows = [1 if s[0] in (PROMPT, DECODE) else 0 for s in slots]
    left = max_rows - sum(nrows)
    for i, s in enumerate(slots):
        if s[0] == PROMPT:
            take = 0
            while take < s[1] - s[2] - 1 and left > 0:
                take, left = take + 1, left - 1
            nrows[i] += take
    granted = [0] * n
    for i in range(n):
        while granted[i] < want[i] and left > 0:
            granted[i], left = granted[i] + 1, left - 1
    rows = []
    for i, s in enumerate(slots):
        for k in range(nrows[i] + granted[i]):
            rows.append((i, s[2] + k, 1 if s[0] == DECODE or s[2] + k == s[1] - 1 else 0))
    rows += [(-1, -1, 0)] * (max_rows - len(rows))
    idle = (-1, -1, 0)
    first = [idle] * (2 * n)
    later = [[idle] * n for _ in range(n_passes - 1)]
    for i, s in enumerate(slots):
        if not drafting[i]:
            continue
        pos = draft_cursor[i]
        while pos <= s[2]:                                        # s[Dc..P]: one row, or two
            first[2 * i + pos - draft_cursor[i]] = (i, pos, 1 if pos == s[2] and granted[i] > 0 else 0)
            pos += 1
        for j in range(1, granted[i]):
            later[j - 1][i] = (i, s[2] + j, 1)
    return rows, want, granted, [first] + later


def random_table(rng, n_slots, seq_len, n_passes):
    """a slot table with every state, per slot n_draft and a draft cursor at the cursor or one row behind"""
    slots, n_draft, cursors = [], [], []
    for _ in range(n_slots):
        state = int(rng.integers(0, 4))
        n_ctx = int(rng.integers(1, seq_len // 2))
        max_new = int(rng.integers(1, seq_len - n_ctx + 1))
        if state == PROMPT:
            s = (PROMPT, n_ctx, int(rng.integers(0, n_ctx)), 0, max_new)
        elif state == DECODE and max_new >= 2:
            n_out = int(rng.integers(1, max_new))
            s = (DECODE, n_ctx, n_ctx + n_out - 1, n_out, max_new)
        elif state == DONE:
            s = (DONE, n_ctx, n_ctx + max_new - 1, max_new, max_new)
        else:
            s = (FREE, 0, 0, 0, 0)
        slots.append(s)
        n_draft.append(int(rng.integers(0, n_passes + 1)) if rng.integers(0, 4) else 0)
        cursors.append(max(s[2] - int(rng.integers(0, 2)), 0) if s[0] == DECODE else int(rng.integers(0, seq_len)))
    return slots, n_draft, cursors
