"""The workloads of the fp32 serving chain's tests, as data: tests/test_serve_host.py asserts from the host plan that each reaches what it is
there for (a wholly idle second tile, one slot's rows on both sides of row 32), tests/test_hip_serve.py runs them on the GPU."""
from oracle import oracle as O

FREE, PROMPT, DECODE, DONE = 0, 1, 2, 3
TILE = 32                      # rows per weight pass of the parity-mode token batch (kGcMaxTok)

# the smallest configuration the parity-mode token batch takes, the stories15M shape, one layer of llama2-7B's
TINY = O.Config(64, 176, 2, 4, 4, 320, 96, False)
STORIES15M = O.Config(288, 768, 6, 6, 6, 32000, 256, True)
L1_7B = O.Config(4096, 11008, 1, 32, 32, 320, 1152, False)

# (context length, max_new) per request
IDLE_TILE = dict(n_slots=4, max_rows=64, narrow_rows=32, sizes=[(3, 5), (1, 6), (2, 4), (2, 3)])       # <= 8 wanted rows in every step: 8 context positions in all, then 4 decode rows
STRADDLE = dict(n_slots=2, sizes=[(30, 3), (40, 4)])      # at max_rows 64: slot 0 takes rows 0..29, slot 1 rows 30..63 -- both sides of row 32
HOLES = dict(n_slots=33, max_rows=64, holes=(0, 31, 32), sizes=[(1 + i % 4, 2 + i % 3) for i in range(30)])
REUSE = dict(n_slots=4, sizes=[(1, 6), (3, 1), (9, 5), (2, 7), (12, 3), (1, 4), (6, 6), (4, 2), (17, 5), (2, 1), (5, 4), (3, 3), (8, 2), (1, 5)])
SERVER = dict(n_slots=4, sizes=REUSE["sizes"][:12])
LONG_7B = dict(n_slots=3, max_rows=32, sizes=[(3, 48), (2, 48), (1100, 2)])


def replay(slots, max_rows, plan_step):
    """the host plan step by step until nobody is live -> [(rows, slots after)]"""
    out = []
    while any(s[0] in (PROMPT, DECODE) for s in slots):
        rows, slots = plan_step(slots, max_rows)
        out.append((rows, slots))
    return out


def admitted(sizes, n_slots, holes=()):
    """the slot table right after the first n_slots - len(holes) requests have been admitted"""
    it = iter(sizes)
    table = []
    for i in range(n_slots):
        if i in holes:
            table.append((FREE, 0, 0, 0, 0))
        else:
            n, new = next(it)
            table.append((PROMPT, n, 0, 0, new))
    return table
