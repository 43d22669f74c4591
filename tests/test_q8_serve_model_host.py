"""The serving chain with a draft model, without a GPU: rama_q8_serve_model_plan_step against a row-by-row restatement, the whole
workload's replay (rama_amd.q8_replay.serve_model_replay) under always-right, always-wrong and right-for-m-tokens drafters, and the
refusals that need no device.  The cases: tests/serve_model_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests.serve_model_cases import DECODE, DONE, FREE, PLAN_SHAPES, PROMPT, plan_py, random_table

EINVAL = -1


def plan(slots, n_draft, cursors, max_rows, seq_len, n_passes):
    from rama_amd.q8 import serve_model_plan_step
    rows, want, granted, passes = serve_model_plan_step(slots, n_draft, cursors, max_rows, seq_len, n_passes)
    return rows, list(want), list(granted), passes


# ------------------------------------------------------------------ 1. the plan

@pytest.mark.parametrize("n_slots,max_rows", PLAN_SHAPES)
def test_plan_equals_the_row_by_row_restatement_on_random_tables(n_slots, max_rows):
    rng = np.random.default_rng(100 * n_slots + max_rows)
    seen = set()
    for _ in range(60):
        n_passes = int(rng.integers(1, 16))
        slots, n_draft, cursors = random_table(rng, n_slots, 48, n_passes)
        got = plan(slots, n_draft, cursors, max_rows, 48, n_passes)
        assert got == plan_py(slots, n_draft, cursors, max_rows, 48, n_passes), (slots, n_draft, cursors, n_passes)
        rows, want, granted, passes = got
        assert len(passes) == n_passes and len(passes[0]) == 2 * n_slots and all(len(p) == n_slots for p in passes[1:])
        for i in range(n_slots):
            seen.add("cut" if 0 < granted[i] < want[i] else "none" if want[i] and not granted[i] else "all" if want[i] else "-")
            if want[i] and passes[0][2 * i + 1][0] == i:
                seen.add("catch-up" if granted[i] else "catch-up without a grant")
    if (n_slots, max_rows) == (4, 8):
        assert {"cut", "none", "all", "catch-up", "catch-up without a grant"} <= seen, seen


def test_plan_named_edges():
    # one slot, one row: the slot's own row takes it; it wants 7, is granted nothing and still feeds s[Dc..P] -- two rows here
    rows, want, granted, passes = plan([(DECODE, 3, 5, 3, 12)], [7], [4], 1, 32, 7)
    assert (rows, want, granted) == ([(0, 5, 1)], [7], [0])
    assert passes[0] == [(0, 4, 0), (0, 5, 0)] and all(p == [(-1, -1, 0)] for p in passes[1:])
    # the budget, then the context window, bind the want: max_new - n_out - 1, seq_len - 1 - P
    assert plan([(DECODE, 3, 5, 3, 5)], [7], [5], 16, 32, 7)[1] == [1]
    assert plan([(DECODE, 3, 5, 3, 4)], [7], [5], 16, 32, 7)[1] == [0]
    assert plan([(DECODE, 3, 5, 3, 30)], [7], [5], 16, 8, 7)[1] == [2]
    # a slot that wants nothing (its last token) still feeds its row: the draft cache follows to the end
    assert plan([(DECODE, 3, 5, 3, 4)], [7], [5], 16, 32, 7)[3][0] == [(0, 5, 0), (-1, -1, 0)]
    # granted 3 of 7: the first pass picks from the last live row, passes 1 and 2 carry d[0], d[1] at P + 1, P + 2, pass 3 is idle
    rows, want, granted, passes = plan([(DECODE, 3, 5, 3, 12), (PROMPT, 9, 0, 0, 2)], [7, 0], [5, 0], 13, 32, 7)
    assert (want, granted) == ([7, 0], [3, 0])
    assert rows[:4] == [(0, 5, 1), (0, 6, 1), (0, 7, 1), (0, 8, 1)] and rows[4] == (1, 0, 0) and rows[12] == (1, 8, 1)
    assert passes[0] == [(0, 5, 1), (-1, -1, 0), (-1, -1, 0), (-1, -1, 0)]
    assert [p[0] for p in passes[1:]] == [(0, 6, 1), (0, 7, 1)] + [(-1, -1, 0)] * 4
    # FREE, DONE and PROMPT slots, and a DECODE slot with n_draft 0, neither want nor feed
    slots = [(FREE, 0, 0, 0, 0), (DONE, 2, 5, 4, 4), (PROMPT, 4, 1, 0, 3), (DECODE, 2, 3, 2, 9)]
    rows, want, granted, passes = plan(slots, [7, 7, 7, 0], [0, 5, 1, 3], 8, 32, 7)
    assert want == [0] * 4 and all(r == (-1, -1, 0) for p in passes for r in p)


@pytest.mark.parametrize("n_slots,max_rows", PLAN_SHAPES)
def test_with_no_drafts_the_target_table_is_the_spec_plans_with_zero_wants(n_slots, max_rows):
    from rama_amd.q8 import serve_spec_plan_step
    rng = np.random.default_rng(7 * n_slots + max_rows)
    for _ in range(30):
        slots, _, cursors = random_table(rng, n_slots, 48, 7)
        rows, want, granted, passes = plan(slots, [0] * n_slots, cursors, max_rows, 48, 7)
        ref_rows, ref_granted = serve_spec_plan_step(slots, [0] * n_slots, max_rows)
        assert rows == ref_rows and granted == list(ref_granted) == [0] * n_slots and want == [0] * n_slots
        assert all(r == (-1, -1, 0) for p in passes for r in p)


# ------------------------------------------------------------------ 2. the replay

def workload(rng, n_req, seq_len=64):
    reqs, refs = [], []
    for q in range(n_req):
        n_ctx = int(rng.integers(1, 20))
        new = int(rng.integers(1, 24))
        ref = [int(t) for t in rng.integers(2, 50, new)]
        stop = ref[new // 2] if q % 3 == 1 else None
        reqs.append(dict(context=[1] + [int(t) for t in rng.integers(2, 50, n_ctx - 1)], max_new=new, stop_token=stop,
                         n_draft=int(rng.choice([0, 1, 2, 7, 15]))))
        refs.append(ref)
    return reqs, refs


def drafter(reqs, refs, q, right_for):
    """request q's draft function: right for the first `right_for` tokens of every call (None: always), then a token the run never has"""
    n_ctx, ref = len(reqs[q]["context"]), refs[q]

    def fn(prefix, n):
        e = len(prefix) - n_ctx
        assert prefix[n_ctx:] == ref[:e]                          # the text is the context and the reference tokens so far
        return [ref[e + j] if right_for is None or j < right_for else 1 for j in range(n)]
    return fn


@pytest.mark.parametrize("right_for", [None, 0, 1, 3])
@pytest.mark.parametrize("n_slots,max_rows", [(1, 1), (3, 8), (4, 16), (16, 16)])
def test_replay_keeps_the_gap_and_cuts_by_the_accept_rule(n_slots, max_rows, right_for):
    from rama_amd.q8 import _accept_py, serve_model_replay
    rng = np.random.default_rng(1000 * n_slots + max_rows)
    reqs, refs = workload(rng, 3 * n_slots)
    rp = serve_model_replay(reqs, refs, [drafter(reqs, refs, q, right_for) for q in range(len(reqs))], n_slots, max_rows)
    who, n_out, Dc = {}, {}, {}
    for st in rp["steps"]:
        for slot, q in st["admitted"]:
            who[slot], n_out[slot], Dc[slot] = q, 0, len(reqs[q]["context"])
        for slot, (g, a, emit, catch_up) in st["drafting"].items():
            q = who[slot]
            P = len(reqs[q]["context"]) + n_out[slot] - 1
            assert P - Dc[slot] == catch_up and catch_up in (0, 1)              # the gap when the step opened
            assert g == st["granted"][slot] <= st["want"][slot] == max(min(reqs[q]["n_draft"], reqs[q]["max_new"] - n_out[slot] - 1), 0)
            d = drafter(reqs, refs, q, right_for)(reqs[q]["context"] + refs[q][:n_out[slot]], g)
            stop = reqs[q]["stop_token"]
            want = _accept_py(d, refs[q][n_out[slot]:n_out[slot] + g + 1], reqs[q]["max_new"] - n_out[slot], -1 if stop is None else stop)
            assert (a, emit) == want[:2] and (slot in st["finished"]) == want[2]
            if right_for is None:
                assert a == g
            elif g:
                assert a == min(right_for, g)
        for slot, e in st["emitted"].items():
            n_out[slot] += e
        for slot in who:
            Dc[slot] = st["cursors"][slot]
            q = who[slot]
            P = len(reqs[q]["context"]) + n_out[slot] - 1
            if st["slots"][slot][0] == DECODE and reqs[q]["n_draft"]:
                assert P - Dc[slot] in (0, 1), (slot, st)
    for q, r in enumerate(reqs):
        out = rp["outputs"][q]
        cut = refs[q][:refs[q].index(r["stop_token"]) + 1] if r["stop_token"] in refs[q] else refs[q]
        assert out == cut
        if r["n_draft"] and len(out) > 1:                         # the draft cache holds the rows of every token fed but, at most, the last
            assert len(r["context"]) + len(out) - 2 <= rp["cursor"][q] <= len(r["context"]) + len(out)
    c = rp["counters"]
    assert c["rows_draft"] == c["drafts_granted"] and c["draft_passes"] <= c["draft_rows_fed"] == c["draft_passes"] + c["catch_up_rows"]
    if (n_slots, max_rows) == (1, 1):
        assert c["drafts_granted"] == 0 and c["catch_up_rows"] == 0


def test_replay_without_drafts_is_the_spec_replay_without_drafts():
    from rama_amd.q8 import serve_model_replay, serve_spec_replay
    rng = np.random.default_rng(5)
    reqs, refs = workload(rng, 9)
    for r in reqs:
        r["n_draft"] = 0
    a = serve_model_replay(reqs, refs, lambda prefix, n: [], 3, 8)
    b = serve_spec_replay(reqs, refs, 3, 8)
    assert a["outputs"] == b["outputs"] and a["finish_step"] == b["finish_step"]
    assert [s["rows"] for s in a["steps"]] == [s["rows"] for s in b["steps"]]
    assert {k: a["counters"][k] for k in b["counters"]} == b["counters"] and a["counters"]["draft_passes"] == 0


# ------------------------------------------------------------------ 3. the refusals that need no device

def test_plan_step_refusals():
    import rama_amd
    from rama_amd._lib import rama_q8_serve_row, rama_q8_serve_slot
    L = rama_amd.load()

    def call(slots, n_draft, cursors, max_rows, seq_len=32, n_passes=7, null=None):
        n = len(slots)
        table = (rama_q8_serve_slot * max(n, 1))(*[rama_q8_serve_slot(*s) for s in slots])
        rows, drows = (rama_q8_serve_row * 128)(), (rama_q8_serve_row * (16 * 128))()
        want, granted = (C.c_int32 * 128)(), (C.c_int32 * 128)()
        args = [table, n, max_rows, seq_len, (C.c_int32 * max(n, 1))(*n_draft), (C.c_int32 * max(n, 1))(*cursors), n_passes, rows, want, granted, drows]
        if null is not None:
            args[null] = None
        return L.rama_q8_serve_model_plan_step(*args)
    ok = [(DECODE, 3, 5, 3, 12)]
    assert call(ok, [7], [5], 4) == 0
    for null in (0, 4, 5, 7, 8, 9, 10):
        assert call(ok, [7], [5], 4, null=null) == EINVAL
    assert call(ok, [8], [5], 4) == EINVAL                        # n_draft beyond the passes
    assert call(ok, [-1], [5], 4) == EINVAL
    assert call(ok, [7], [3], 4) == EINVAL                        # a draft cursor two rows behind
    assert call(ok, [7], [6], 4) == EINVAL                        # ... or ahead
    assert call(ok, [0], [0], 4) == 0                             # (a slot that does not draft: its cursor is not looked at)
    assert call(ok, [7], [5], 4, n_passes=0) == EINVAL
    assert call(ok, [7], [5], 4, n_passes=16) == EINVAL
    assert call(ok, [7], [5], 0) == EINVAL
    assert call(ok * 65, [0] * 65, [0] * 65, 128) == EINVAL       # 2 n_slots > 128
    assert call(ok * 64, [0] * 64, [0] * 64, 128) == 0
    assert call([(DECODE, 3, 5, 0, 12)], [7], [5], 4) == EINVAL   # a DECODE slot has produced a token
    assert call([(7, 3, 5, 3, 12)], [0], [0], 4) == EINVAL


def test_server_refuses_bad_draft_sizes_before_any_library_call():
    from rama_amd.q8 import serve_model_sizes
    from rama_amd.transformer import Config

    class M:
        def __init__(self, V):
            self.cfg = Config(32, 64, 2, 4, 4, V, 32, True)
    cfg = M(64).cfg
    serve_model_sizes(cfg, M(64), 64, 15, 0)
    for args in [(M(64), 4, 7, 8), (M(64), 4, 0, 0), (M(64), 4, 16, 0), (M(65), 4, 7, 0), (M(64), 65, 7, 0)]:
        with pytest.raises(ValueError):
            serve_model_sizes(cfg, *args)
