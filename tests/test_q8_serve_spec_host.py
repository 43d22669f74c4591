"""Speculation inside the serving chain, host side (no GPU): the new symbols are declared everywhere; rama_q8_serve_spec_plan_step --
the scheduling rule with drafts as a pure function -- equals a restatement that hands rows out one at a time, on random slot tables
and random want vectors and on its named edges, and with every want == 0 it is rama_q8_serve_plan_step; serve_spec_replay reproduces
a hand-written trajectory of three slots that reaches every accept outcome; every refusal that needs no GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
SYMBOLS = ["rama_q8_serve_begin_spec", "rama_q8_serve_admit_spec", "rama_q8_serve_spec_plan_step", "rama_q8_serve_spec_stats"]
FREE, PROMPT, DECODE, DONE = 0, 1, 2, 3
EINVAL = -1
SIZES = [(1, 1), (4, 8), (16, 16), (65, 96), (128, 128)]


def test_serve_spec_symbols_are_declared_everywhere():
    import rama_amd
    from rama_amd import _lib
    L = rama_amd.load()
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "rama_hip.h").read_text(), flags=re.S)
    rust = (REPO / "integration" / "rust" / "hip_sys.rs").read_text()
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), f"include/rama_hip.h lacks {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES lacks {s}"
        assert hasattr(L, s), f"librama_hip.so lacks {s}"
        decl = re.findall(rf"pub fn {s}\s*\((.*?)\)\s*->", rust, flags=re.S)
        assert len(decl) == 1, f"hip_sys.rs must declare {s} once"
        assert decl[0].count(",") + 1 == len(_lib.SIGNATURES[s][1]), f"{s}: hip_sys.rs and _lib.py disagree on the argument count"
    for name in ("rama_q8_serve_spec", "rama_q8_serve_spec_report"):
        assert re.search(rf"\}}\s*{name};", header) and f"pub struct {name}" in rust and hasattr(_lib, name), name
    # the structs as the header lays them out (LP64): two ints, a pointer, an int and padding; 25 uint64, 4 ints and 2 x 128 ints
    assert C.sizeof(_lib.rama_q8_serve_spec) == 24 and _lib.rama_q8_serve_spec.hint.offset == 8
    assert C.sizeof(_lib.rama_q8_serve_spec_report) == 25 * 8 + 16 + 2 * 512 and _lib.rama_q8_serve_spec_report.accepted_hist.offset == 72


# ------------------------------------------------------------------ the scheduling rule, restated row by row

def rule_plan(slots, want, max_rows):
    """rows handed out one at a time: a first row per DECODE and PROMPT slot, then further context positions to the PROMPT slots in
    ascending slot index, then drafts to the DECODE slots in ascending slot index"""
    n = [1 if s[0] in (PROMPT, DECODE) else 0 for s in slots]
    left = max_rows - sum(n)
    assert left >= 0
    for i, s in enumerate(slots):
        while s[0] == PROMPT and left > 0 and s[2] + n[i] < s[1]:
            n[i] += 1
            left -= 1
    granted = [0] * len(slots)
    for i, s in enumerate(slots):
        while s[0] == DECODE and left > 0 and granted[i] < want[i]:
            granted[i] += 1
            left -= 1
    rows = []
    for i, s in enumerate(slots):
        for k in range(n[i] + granted[i]):
            pos = s[2] + k
            rows.append((i, pos, int(s[0] == DECODE or pos == s[1] - 1)))
    return rows + [(-1, -1, 0)] * left, granted


def random_table(rng, n_slots, p_decode=0.4):
    slots, want = [], []
    for _ in range(n_slots):
        x = rng.random()
        if x < p_decode:
            max_new = int(rng.integers(2, 40))
            n_out = int(rng.integers(1, max_new))
            n_ctx = int(rng.integers(1, 30))
            slots.append((DECODE, n_ctx, n_ctx + n_out - 1, n_out, max_new))
            want.append(int(rng.integers(0, min(15, max_new - n_out - 1) + 1)) if rng.random() < 0.8 else 0)
        elif x < 0.7:
            n_ctx = int(rng.integers(1, 60))
            slots.append((PROMPT, n_ctx, int(rng.integers(0, n_ctx)), 0, int(rng.integers(1, 9))))
            want.append(0)
        else:
            slots.append((FREE if rng.random() < 0.5 else DONE, 3, 2, 0, 4))
            want.append(0)
    return slots, want


@pytest.mark.parametrize("n_slots,max_rows", SIZES)
def test_plan_equals_the_restated_rule_on_random_tables(n_slots, max_rows):
    from rama_amd.q8 import _spec_plan_py, serve_plan_step, serve_spec_plan_step
    rng = np.random.default_rng(100 * n_slots + max_rows)
    cut = partial = 0
    for trial in range(60):
        slots, want = random_table(rng, n_slots, p_decode=(0.2, 0.4, 0.9)[trial % 3])
        rows, granted = serve_spec_plan_step(slots, want, max_rows)
        assert (rows, granted) == rule_plan(slots, want, max_rows), (slots, want)
        assert (rows, granted) == _spec_plan_py(slots, want, max_rows), (slots, want)          # serve_spec_replay's own statement
        assert len(rows) == max_rows
        cut += any(g < w for g, w in zip(granted, want))
        partial += any(0 < g < w for g, w in zip(granted, want))
        # with every want == 0: the plain chain's table
        rows0, granted0 = serve_spec_plan_step(slots, [0] * n_slots, max_rows)
        assert granted0 == [0] * n_slots and rows0 == serve_plan_step(slots, max_rows)[0], slots
    if max_rows > 1:
        assert cut, "no table of this size ran out of rows"
    if (n_slots, max_rows) in ((4, 8), (65, 96)):
        assert partial, "no table of this size cut a grant in the middle"


def test_plan_named_edges():
    from rama_amd.q8 import serve_plan_step, serve_spec_plan_step
    dec = lambda n_ctx, n_out, max_new=32: (DECODE, n_ctx, n_ctx + n_out - 1, n_out, max_new)
    # no rows left for any draft: the two first rows and the prompt's 2 extras fill max_rows = 4
    slots = [dec(3, 1), (PROMPT, 9, 2, 0, 4), (FREE, 0, 0, 0, 0)]
    rows, granted = serve_spec_plan_step(slots, [5, 0, 0], 4)
    assert granted == [0, 0, 0] and rows == [(0, 3, 1), (1, 2, 0), (1, 3, 0), (1, 4, 0)]
    # rows run out in the middle of one slot's drafts: 3 first rows, 5 left, slot 0 takes 3, slot 1 gets 2 of its 4, slot 2 nothing
    slots = [dec(3, 1), dec(5, 2), dec(2, 4)]
    rows, granted = serve_spec_plan_step(slots, [3, 4, 2], 8)
    assert granted == [3, 2, 0]
    assert rows == [(0, 3, 1), (0, 4, 1), (0, 5, 1), (0, 6, 1), (1, 6, 1), (1, 7, 1), (1, 8, 1), (2, 5, 1)]
    # a PROMPT slot's extras consume what a LOWER-index DECODE slot wanted: ingestion goes first whatever the index
    slots = [dec(3, 1), (PROMPT, 6, 0, 0, 4)]
    rows, granted = serve_spec_plan_step(slots, [4, 0], 7)
    assert granted == [0, 0] and rows == [(0, 3, 1)] + [(1, p, int(p == 5)) for p in range(6)]
    rows, granted = serve_spec_plan_step(slots, [4, 0], 9)           # two rows more: the drafts get exactly those
    assert granted == [2, 0] and rows == [(0, 3, 1), (0, 4, 1), (0, 5, 1)] + [(1, p, int(p == 5)) for p in range(6)]
    # max_rows == n_slots, all DECODE: never a draft row
    slots = [dec(2 + i, 1 + i) for i in range(5)]
    rows, granted = serve_spec_plan_step(slots, [15, 1, 7, 3, 2], 5)
    assert granted == [0] * 5 and rows == serve_plan_step(slots, 5)[0] == [(i, 2 * i + 2, 1) for i in range(5)]
    # a DONE and a FREE slot between them take nothing; the idle rows come last
    slots = [(DONE, 3, 5, 3, 3), dec(4, 2), (FREE, 0, 0, 0, 0), dec(1, 1)]
    rows, granted = serve_spec_plan_step(slots, [0, 2, 0, 1], 8)
    assert granted == [0, 2, 0, 1] and rows == [(1, 5, 1), (1, 6, 1), (1, 7, 1), (3, 1, 1), (3, 2, 1)] + [(-1, -1, 0)] * 3


def test_plan_refusals():
    import rama_amd
    from rama_amd._lib import rama_q8_serve_row, rama_q8_serve_slot
    L = rama_amd.load()

    def call(slots, want, max_rows, null=()):
        n = len(slots)
        arr = (rama_q8_serve_slot * max(n, 1))(*[rama_q8_serve_slot(*s) for s in slots])
        w = (C.c_int32 * max(n, 1))(*want)
        rows, g = (rama_q8_serve_row * 128)(), (C.c_int32 * 128)()
        return L.rama_q8_serve_spec_plan_step(None if "slots" in null else arr, n, max_rows, None if "want" in null else w,
                                              None if "rows" in null else rows, None if "granted" in null else g)

    ok = [(DECODE, 3, 4, 2, 9), (PROMPT, 4, 1, 0, 3)]
    assert call(ok, [2, 0], 4) == 0
    for null in ("slots", "want", "rows", "granted"):
        assert call(ok, [2, 0], 4, null=(null,)) == EINVAL
    assert call(ok, [2, 0], 1) == EINVAL                          # max_rows < n_slots
    assert call(ok, [2, 0], 129) == EINVAL
    assert call([], [], 4) == EINVAL
    assert call(ok, [16, 0], 4) == EINVAL                         # more than 15 drafts
    assert call(ok, [-1, 0], 4) == EINVAL
    assert call(ok, [0, 1], 4) == EINVAL                          # a PROMPT slot drafts nothing
    assert call([(FREE, 0, 0, 0, 0)], [1], 4) == EINVAL
    assert call([(DONE, 3, 5, 3, 3)], [1], 4) == EINVAL
    assert call([(DECODE, 3, 4, 2, 9)], [6], 4) == 0              # max_new - n_out - 1 = 6
    assert call([(DECODE, 3, 4, 2, 9)], [7], 4) == EINVAL         # ... and one more would emit beyond the budget
    assert call([(5, 0, 0, 0, 0)], [0], 4) == EINVAL              # the plain rule's own refusals
    assert call([(DECODE, 3, 4, 0, 9)], [0], 4) == EINVAL
    assert call([(PROMPT, 4, 4, 0, 3)], [0], 4) == EINVAL


def test_entries_refuse_without_a_context_or_a_chain():
    import rama_amd
    from rama_amd import _lib
    L = rama_amd.load()
    cfg = _lib.rama_config(64, 128, 2, 4, 4, 64, 32, 1)
    w, st = _lib.rama_q8_weights(), _lib.rama_run_state()
    plan = _lib.rama_q8_serve_plan(0.0, 0.9, 0.0, 3, -1)
    spec = _lib.rama_q8_serve_spec(2, 3, None, 0)
    ctx = (C.c_int32 * 2)(1, 2)
    assert L.rama_q8_serve_begin_spec(None, C.byref(cfg), C.byref(w), 2, 4, 8, 3, 0) == EINVAL
    assert L.rama_q8_serve_admit_spec(None, 0, C.byref(st), ctx, 2, 0, C.byref(plan), C.byref(spec)) == EINVAL
    assert L.rama_q8_serve_admit_spec(None, 0, C.byref(st), ctx, 2, 0, C.byref(plan), None) == EINVAL
    assert L.rama_q8_serve_spec_stats(None, C.byref(_lib.rama_q8_serve_spec_report())) == EINVAL


def test_server_checks_before_any_library_call():
    from rama_amd.q8 import serve_spec_request, serve_spec_sizes
    from rama_amd.transformer import Config
    cfg = Config(64, 128, 2, 4, 4, 50, 32, True)
    assert serve_spec_sizes(0, 3, 0) == (0, 3, 0) and serve_spec_sizes(15, 4, 100) == (15, 4, 100)
    for bad in [(-1, 3, 0), (16, 3, 0), (3, 0, 0), (3, 5, 0), (3, 3, -1), (0, 3, 8)]:
        with pytest.raises(ValueError):
            serve_spec_sizes(*bad)
    assert serve_spec_request(cfg, 7, 3, 4) == (7, 3, [])         # the server's default
    assert serve_spec_request(cfg, 7, 3, 4, 0, [1, 2]) == (0, 3, [1, 2])
    assert serve_spec_request(cfg, 0, 3, 0) == (0, 3, [])         # a plain server: nothing to ask for
    for bad in [dict(n_draft=8), dict(n_draft=-1), dict(hint=[1, 2, 3, 4, 5]), dict(hint=[50]), dict(hint=[-1])]:
        with pytest.raises(ValueError):
            serve_spec_request(cfg, 7, 3, 4, **bad)
    with pytest.raises(ValueError):
        serve_spec_request(cfg, 0, 3, 0, n_draft=1)               # drafts on a server made without them
    with pytest.raises(ValueError):
        serve_spec_request(cfg, 0, 3, 0, hint=[1])


# ------------------------------------------------------------------ serve_spec_replay against a trajectory written by hand

def test_replay_of_a_hand_written_trajectory():
    """three slots, max_rows 8, five requests on synthetic reference streams.  Worked by hand from the rules in rama_hip.h:
    step 1  slot 0 wants [5,6,7] behind the tail (6,7); slot 2's context takes 3 extra rows first, so 2 are granted (a grant cut by
            lack of rows) and both are accepted (all of its granted drafts);
    step 2  slot 0's last two tokens in one step: its one draft is right and the budget ends with it; slot 1's draft 31 (from its
            hint) meets the pick 40 (the first draft rejected); slot 2's drafts 21, 22 are both right and 22 is its stop token;
    step 3  requests 3 and 4 enter slots 0 and 2; slot 1 emits its last token while slot 0 ingests a 12-token context;
    step 6  request 4: one right draft, and the budget ends with it."""
    from rama_amd.q8 import serve_spec_replay
    reqs = [dict(context=[1, 5, 6, 7, 5, 6], max_new=6, n_draft=3, ngram=2),
            dict(context=[1, 2], max_new=3, n_draft=2, ngram=1, hint=[2, 30, 31, 32]),
            dict(context=[1, 3, 4, 14, 15], max_new=4, n_draft=3, ngram=3, hint=[20, 21, 22, 23], stop_token=22),
            dict(context=[1] + list(range(60, 71)), max_new=2),
            dict(context=[1, 8, 9, 8, 9], max_new=3, n_draft=3, ngram=2)]
    refs = [[7, 5, 6, 7, 5, 6], [30, 40, 41], [20, 21, 22, 23], [70, 71], [8, 9, 8]]
    out = serve_spec_replay(reqs, refs, 3, 8)
    idle = (-1, -1, 0)
    want_steps = [
        dict(admitted=[(0, 0), (1, 1), (2, 2)], rows=[(0, p, int(p == 5)) for p in range(6)] + [(1, 0, 0), (2, 0, 0)],
             want=[0, 0, 0], granted=[0, 0, 0], accepted={}, emitted={0: 1}, finished=[],
             slots=[(DECODE, 6, 6, 1, 6), (PROMPT, 2, 1, 0, 3), (PROMPT, 5, 1, 0, 4)]),
        dict(admitted=[], rows=[(0, 6, 1), (0, 7, 1), (0, 8, 1), (1, 1, 1), (2, 1, 0), (2, 2, 0), (2, 3, 0), (2, 4, 1)],
             want=[3, 0, 0], granted=[2, 0, 0], accepted={0: 2}, emitted={0: 3, 1: 1, 2: 1}, finished=[],
             slots=[(DECODE, 6, 9, 4, 6), (DECODE, 2, 2, 1, 3), (DECODE, 5, 5, 1, 4)]),
        dict(admitted=[], rows=[(0, 9, 1), (0, 10, 1), (1, 2, 1), (1, 3, 1), (2, 5, 1), (2, 6, 1), (2, 7, 1), idle],
             want=[1, 1, 2], granted=[1, 1, 2], accepted={0: 1, 1: 0, 2: 2}, emitted={0: 2, 1: 1, 2: 2}, finished=[0, 2],
             slots=[(DONE, 6, 11, 6, 6), (DECODE, 2, 3, 2, 3), (DONE, 5, 7, 3, 4)]),
        dict(admitted=[(0, 3), (2, 4)], rows=[(0, p, 0) for p in range(6)] + [(1, 3, 1), (2, 0, 0)],
             want=[0, 0, 0], granted=[0, 0, 0], accepted={1: 0}, emitted={1: 1}, finished=[1],
             slots=[(PROMPT, 12, 6, 0, 2), (DONE, 2, 4, 3, 3), (PROMPT, 5, 1, 0, 3)]),
        dict(admitted=[], rows=[(0, p, int(p == 11)) for p in range(6, 12)] + [(2, 1, 0), (2, 2, 0)],
             want=[0, 0, 0], granted=[0, 0, 0], accepted={}, emitted={0: 1}, finished=[],
             slots=[(DECODE, 12, 12, 1, 2), (DONE, 2, 4, 3, 3), (PROMPT, 5, 3, 0, 3)]),
        dict(admitted=[], rows=[(0, 12, 1), (2, 3, 0), (2, 4, 1)] + [idle] * 5,
             want=[0, 0, 0], granted=[0, 0, 0], accepted={0: 0}, emitted={0: 1, 2: 1}, finished=[0],
             slots=[(DONE, 12, 13, 2, 2), (DONE, 2, 4, 3, 3), (DECODE, 5, 5, 1, 3)]),
        dict(admitted=[], rows=[(2, 5, 1), (2, 6, 1)] + [idle] * 6,
             want=[0, 0, 1], granted=[0, 0, 1], accepted={2: 1}, emitted={2: 2}, finished=[2],
             slots=[(DONE, 12, 13, 2, 2), (DONE, 2, 4, 3, 3), (DONE, 5, 7, 3, 3)]),
    ]
    assert len(out["steps"]) == len(want_steps)
    for k, (got, want) in enumerate(zip(out["steps"], want_steps)):
        assert got == want, k
    assert out["counters"] == dict(steps=7, rows_decode=7, rows_draft=7, rows_prompt=30, rows_idle=12, drafts_wanted=8, drafts_granted=7,
                                   drafts_accepted=6, tokens_emitted=17, accepted_hist=[3, 2, 2] + [0] * 13)
    assert out["finish_step"] == [2, 3, 2, 5, 6] and out["slot"] == [0, 1, 2, 0, 2]
    assert out["outputs"] == [[7, 5, 6, 7, 5, 6], [30, 40, 41], [20, 21, 22], [70, 71], [8, 9, 8]]
    # the six outcomes, found in the replay itself
    steps = out["steps"]
    assert any(s["granted"][i] > 0 and s["accepted"].get(i) == s["granted"][i] for s in steps for i in range(3))       # all granted accepted
    assert any(s["granted"][i] > 0 and s["accepted"].get(i) == 0 for s in steps for i in range(3))                      # the first rejected
    assert any(0 < s["granted"][i] < s["want"][i] for s in steps for i in range(3))                                     # a grant cut
    assert steps[2]["accepted"][0] == 1 and 0 in steps[2]["finished"] and len(out["outputs"][0]) == 6                   # the budget ends in a run
    assert steps[2]["accepted"][2] == 2 and steps[2]["emitted"][2] == 2 and out["outputs"][2][-1] == 22                 # a stop among the accepted
    assert 1 in steps[3]["finished"] and steps[3]["slots"][0][0] == PROMPT                                              # a finish next to an ingestion


def test_replay_with_a_hole_and_without_drafts():
    """use_slots leaves slot 1 FREE; with n_draft 0 everywhere every step is the plain rule's and one token per DECODE slot"""
    from rama_amd.q8 import serve_plan_step, serve_spec_replay
    reqs = [dict(context=[1, 4, 5], max_new=3), dict(context=[1], max_new=2), dict(context=[1, 9, 9, 9, 9, 9, 9], max_new=2)]
    refs = [[7, 8, 9], [3, 3], [5, 5]]
    out = serve_spec_replay(reqs, refs, 4, 4, use_slots=[0, 2, 3])
    assert out["slot"] == [0, 2, 3] and out["outputs"] == refs
    table = [(FREE, 0, 0, 0, 0)] * 4
    for s in out["steps"]:
        for i, q in s["admitted"]:
            table[i] = (PROMPT, len(reqs[q]["context"]), 0, 0, reqs[q]["max_new"])
        rows, after = serve_plan_step(table, 4)
        assert s["rows"] == rows and s["want"] == s["granted"] == [0] * 4
        assert s["slots"] == after
        table = after
        assert all(r[0] != 1 for r in rows)
    assert out["counters"]["rows_draft"] == 0 and out["counters"]["accepted_hist"][0] == out["counters"]["rows_decode"]
    with pytest.raises(ValueError):
        serve_spec_replay(reqs, [[7, 8], [3, 3], [5, 5]], 4, 4)
