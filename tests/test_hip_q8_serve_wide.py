"""The serving chain at the slot and row counts it is sold for (up to 128 slots, up to 128 rows).  Each case is the first to
reach some code on the device: the scheduler's second wave (the scan across the wave boundary, the rows of threads 64..127,
PROMPT slots from index 64 on taking rows left over), the classifier over 17..32 gathered rows (ksplit<2>) and over 33 or more
(the one-wave MFMA form), the sampler's ordering launches and the pick over dozens of mixed slots, the layer pass at 17..64
rows with idle rows in its last tile, the chain's own vocabulary rules, the budget and cache edges.  The promise is the one of
tests/test_hip_q8_serve.py: every slot's tokens and cache rows are bit for bit those of Q8Engine.generate on it alone, and the
device's row table is the host plan's.  Every comparison is exact.  tests/test_q8_serve_wide_host.py shows without a GPU that
the workloads of tests/serve_wide_cases.py reach what they are for; the first test here holds the device's own run to the same
conditions."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.serve_wide_cases import WORKLOADS, case_id, occupied
from tests.test_hip_q8 import same_bits
from tests.test_hip_q8_prefix import admit_at, fork_eng
from tests.test_hip_q8_serve import (DECODE, DONE, EINVAL, EUNSUP, FREE, PROMPT, SENTINEL, Req, admit, begin, cache, dev,  # noqa: F401
                                     fill_all, mixed_requests, open_model, plan_steps_to_first_finish, poll, run_until_done, set_graph,
                                     stats, steps, tokens)
from tests.test_q8_serve_wide_host import reached, required

pytestmark = pytest.mark.gpu

IDLE = (-1, -1, 0)


def live(st):
    return any(s[0] in (PROMPT, DECODE) for s in st["slots"])


def step_and_compare(dev, before, max_rows, by_slot, totals, trace=None):
    """one step; the device's row table is the host rule applied to the device's own previous slot table, the successors are the
    plan's for every slot without a stop token, the four counters are the running totals -> the report after the step"""
    from rama_amd.q8 import serve_plan_step
    assert steps(dev, 1) == 0
    now = stats(dev)
    rows, after = serve_plan_step(before["slots"], max_rows)
    assert now["rows"] == rows, totals["steps"]
    for i, r in by_slot.items():
        if r.stop < 0:
            assert now["slots"][i] == after[i], (totals["steps"], i)
    used = [r for r in rows if r[0] >= 0]
    dec = sum(1 for r in used if before["slots"][r[0]][0] == DECODE)
    totals["steps"] += 1; totals["decode"] += dec; totals["prompt"] += len(used) - dec; totals["idle"] += max_rows - len(used)
    assert {k: now[k] for k in totals} == totals
    if trace is not None:
        trace.append((before["slots"], rows))
    return now


def counters(st):
    return dict(steps=st["steps"], decode=st["decode"], prompt=st["prompt"], idle=st["idle"])


# ------------------------------------------------------------------ a. the table of wide workloads

@pytest.mark.parametrize("w,graph", [(w, g) for w in WORKLOADS for g in w.graphs], ids=lambda v: case_id(v) if isinstance(v, tuple) else f"graph{v}")
def test_wide_chain_equals_solo_runs(dev, golden_dir, w, graph):
    import rama_amd
    m = open_model(dev, golden_dir, w.model)
    reqs = mixed_requests(dev, m, np.random.default_rng(w.seed + graph), [(n_ctx, new) for n_ctx, new, _ in w.sizes])
    by_slot = dict(zip(occupied(w), reqs))
    spare = [rama_amd.Q8Engine(dev, m) for _ in w.holes]          # run states nobody admits: nothing may write them
    try:
        for e in spare:
            fill_all(e)
        for r, (_, _, kind) in zip(reqs, w.sizes):
            assert kind == ("sampled" if r.T > 0.0 else "greedy") + ("+stop" if r.stop >= 0 else "")
            r.solo()
        set_graph(dev, graph)
        assert begin(dev, m, w.n_slots, w.max_rows, max(r.max_new for r in reqs)) == 0
        for i, r in by_slot.items():
            assert admit(dev, i, r) == 0
        before = stats(dev)
        assert before["slots"] == [(PROMPT, len(by_slot[i].ctx), 0, 0, by_slot[i].max_new) if i in by_slot else (FREE, 0, 0, 0, 0)
                                   for i in range(w.n_slots)]
        totals, trace = counters(before), []
        assert totals == dict(steps=0, decode=0, prompt=0, idle=0)
        while live(before):
            before = step_and_compare(dev, before, w.max_rows, by_slot, totals, trace)
            assert totals["steps"] < 400
        # the device's own run got to what the workload is for (stop tokens fell where they fell)
        got = reached(trace, w.n_slots, w.max_rows)
        assert not [c for c in required(w.n_slots, w.max_rows) if not got[c]], got
        assert [s[0] for s in before["slots"]] == [DONE if i in by_slot else FREE for i in range(w.n_slots)]
        assert before["captures"] == (1 if graph else 0)
        assert before["prompt"] == sum(len(r.ctx) for r in reqs)
        toks = {}
        for i, r in by_slot.items():
            toks[i] = tokens(dev, i)
            assert poll(dev, i) == (toks[i], True, 1)
            r.check(toks[i], (case_id(w), graph, i))
        for h in w.holes:
            assert poll(dev, h) == ([], False, 0) and tokens(dev, h) == []
        # two more steps with every slot DONE or FREE: idle rows only, and nothing else moves
        snap = {i: cache(r.eng) for i, r in by_slot.items()}
        assert steps(dev, 2) == 0
        after = stats(dev)
        assert after["rows"] == [IDLE] * w.max_rows
        totals["steps"] += 2; totals["idle"] += 2 * w.max_rows
        assert counters(after) == totals
        assert after["slots"] == before["slots"] and after["generation"] == before["generation"] and after["captures"] == before["captures"]
        for i, r in by_slot.items():
            assert tokens(dev, i) == toks[i]
            for a, b in zip(cache(r.eng), snap[i]):
                assert same_bits(a, b), (case_id(w), graph, i)
        for e in spare:
            assert all((a == SENTINEL).all() for a in cache(e))
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs:
            r.free()
        for e in spare:
            e.free()
        m.free()


# ------------------------------------------------------------------ b. Q8Server over dozens of reused slots

@pytest.mark.parametrize("which,n_slots,max_rows", [("ckpt_v2_q80_untied", 48, 64), ("synth15m", 33, 33)])
@pytest.mark.parametrize("graph", [0, 1])
def test_wide_server_refills_slots(dev, golden_dir, which, n_slots, max_rows, graph):
    import rama_amd
    from rama_amd.q8 import Q8Server
    m = open_model(dev, golden_dir, which)
    c = m.cfg
    rng = np.random.default_rng(500 + n_slots + graph)
    small = c.seq_len < 64
    twin = rama_amd.Q8Engine(dev, m)
    srv = None
    try:
        reqs = []
        for i in range(3 * n_slots):
            n_ctx = int(rng.integers(1, 14 if small else 40))
            new = int(rng.integers(1, (c.seq_len - n_ctx if small else 8) + 1))
            T, P, U = [(0.0, 0.9, 0.0), (1.0, 0.9, 0.21), (0.8, 0.6, 0.7)][i % 3]
            ctx = [1] + [int(t) for t in rng.integers(2, c.vocab_size, n_ctx - 1)]
            want = twin.generate(ctx[1:], n_ctx - 1 + new, T, P, U)[n_ctx - 1:]
            reqs.append((ctx, new, T, P, U, want))
        set_graph(dev, graph)
        srv = Q8Server(m, n_slots, max_rows, max(r[1] for r in reqs))
        hs = [srv.submit(ctx, new, T, P, U) for ctx, new, T, P, U, _ in reqs]
        srv.run()
        for h, r in zip(hs, reqs):
            assert srv.finished(h)
            assert srv.result(h) == r[5], (which, graph, h)
        st = srv.stats()
        assert st["graph_captures"] == (1 if graph else 0)
        # no stop tokens here, so the host plan is exact for the admission order the server used: the device's sums are the plan's
        for k in ("steps", "rows_decode", "rows_prompt", "rows_idle"):
            assert st[k] == srv.planned[k], (k, st[k], srv.planned[k])
        assert st["rows_prompt"] == sum(len(r[0]) for r in reqs) and st["rows_decode"] == sum(r[1] - 1 for r in reqs)
        assert max(st["generation"]) >= 3 and min(st["generation"]) >= 1
    finally:
        if srv is not None:
            srv.close()
        set_graph(dev, 0)
        twin.free()
        m.free()


# ------------------------------------------------------------------ c. admissions into a table of 65 slots

def test_wide_admission_next_to_running_slots(dev, golden_dir):
    """65 slots at 96 rows, graph mode.  A block of steps that runs past the first foreseen finish is enqueued at once; a newcomer
    with a run state of its own goes into the first slot whose finished word is set, behind whatever of the block still runs; a
    second one goes into slot 64 over rows forked from its finished neighbour, slot 63, with which it shares a prefix"""
    import time
    n_slots, max_rows = 65, 96
    m = open_model(dev, golden_dir, "ckpt_v2_q80_untied")
    rng = np.random.default_rng(65096)
    sizes = [(int(rng.integers(1, 17)), int(rng.integers(5, 13))) for _ in range(n_slots)]
    sizes[2] = (1, 1)                                              # the first to finish, whatever the others do
    sizes[63], sizes[64] = (7, 2), (3, 2)                          # early too; too short a budget for mixed_requests to give them a stop
    reqs = mixed_requests(dev, m, rng, sizes)
    late = Req(dev, m, rng, 14, 6, 1.0, 0.9, 0.37)
    over = Req(dev, m, rng, 19, 5, 0.7, 0.5, 0.6)                  # its first 8 tokens become those slot 63 was fed
    try:
        for r in reqs + [late]:
            r.solo()
        donor = reqs[63]
        n = len(donor.ctx) + 1                                     # slot 63 is fed its context and its first token: rows 0..7
        over.ctx = (donor.ctx + donor.want())[:n] + over.ctx[n:]
        assert len(donor.want()) == 2 and len(over.ctx) == 19
        over.solo()
        set_graph(dev, 1)
        assert begin(dev, m, n_slots, max_rows, 12) == 0
        for i, r in enumerate(reqs):
            assert admit(dev, i, r) == 0
        assert admit(dev, 64, late) == EINVAL                       # every slot is busy
        assert steps(dev, plan_steps_to_first_finish(reqs, n_slots, max_rows) + 6) == 0      # one block, asynchronous
        first, deadline = None, time.time() + 60
        while first is None and time.time() < deadline:
            for i in range(n_slots):
                if poll(dev, i, 0, 1)[1]:
                    first = i
                    break
        assert first is not None and first <= 2
        old_first = poll(dev, first)
        assert admit(dev, first, late) == 0                         # behind whatever of the block is still running
        run_until_done(dev, [63, 64])
        old_64 = poll(dev, 64)
        assert fork_eng(dev, m, donor.eng, [over.eng], n) == 0
        assert admit_at(dev, 64, over, n) == 0
        by_slot = dict(enumerate(reqs))
        by_slot[first], by_slot[64] = late, over
        before = stats(dev)
        assert before["slots"][64] == (PROMPT, 19, n, 0, 5) and before["generation"][64] == 2 == before["generation"][first]
        totals = counters(before)
        while live(before):
            before = step_and_compare(dev, before, max_rows, by_slot, totals)
            assert totals["steps"] < 400
        assert all(s[0] == DONE for s in before["slots"]) and before["captures"] == 1
        assert before["prompt"] == sum(len(r.ctx) for r in reqs) + len(late.ctx) + len(over.ctx) - n
        for i, r in by_slot.items():
            got = tokens(dev, i)
            assert poll(dev, i)[:2] == (got, True)
            r.check(got, i)
        # the old occupants' run states, downloaded only now
        reqs[first].check(old_first[0], "old occupant of the first finished slot")
        reqs[64].check(old_64[0], "old occupant of slot 64")
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs + [late, over]:
            r.free()
        m.free()


# ------------------------------------------------------------------ d. the chain's own vocabulary rules

def vocab_model(dev, vocab_size):
    import rama_amd
    cfg = dict(dim=64, hidden_dim=192, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=vocab_size, seq_len=32, shared_weight=True)
    return rama_amd.Q8Model.synth(dev, O.Config(**cfg), 32, 3)


@pytest.mark.parametrize("vocab_size", [4099, 32772, 40001])
def test_serve_vocabulary_rules(dev, golden_dir, vocab_size):
    """4 099: not a multiple of 4, within the sampler's 32 768 -- sampled and greedy plans run.  32 772: greedy only (the argmax
    over a long row); a sampled plan is refused and the running chain is as it was.  40 001: begin refuses"""
    m = vocab_model(dev, vocab_size)
    rng = np.random.default_rng(vocab_size)
    reqs = []
    try:
        if vocab_size == 40001:
            assert begin(dev, m, 3, 8, 8) == EUNSUP
            assert steps(dev, 1) == EINVAL                         # no chain
            legal = open_model(dev, golden_dir, "ckpt_v2_q80_tied")
            r = Req(dev, legal, rng, 3, 4)
            try:
                assert begin(dev, legal, 3, 8, 8) == 0
                assert admit(dev, 1, r) == 0
                run_until_done(dev, [1])
                r.check(tokens(dev, 1), "a legal model after the refusal")
            finally:
                dev.lib.rama_q8_serve_end(dev.ctx)
                r.free()
                legal.free()
            return
        reqs += [Req(dev, m, rng, 11, 7), Req(dev, m, rng, 4, 8, 1.0 if vocab_size == 4099 else 0.0, 0.9, 0.42)]
        sampled = Req(dev, m, rng, 5, 6, 0.8, 0.7, 0.15)
        reqs.append(sampled)
        for r in reqs[:2] + ([sampled] if vocab_size == 4099 else []):
            r.solo()
        assert begin(dev, m, 3, 8, 8) == 0
        for i, r in enumerate(reqs[:2]):
            assert admit(dev, i, r) == 0
        assert steps(dev, 2) == 0
        st, toks = stats(dev), [tokens(dev, 0), tokens(dev, 1)]
        if vocab_size == 4099:
            assert admit(dev, 2, sampled) == 0
            run_until_done(dev, [0, 1, 2])
            for i, r in enumerate(reqs):
                r.check(tokens(dev, i), (vocab_size, i))
        else:
            assert admit(dev, 2, sampled) == EUNSUP
            assert stats(dev) == st and [tokens(dev, 0), tokens(dev, 1)] == toks and poll(dev, 2) == ([], False, 0)
            run_until_done(dev, [0, 1])
            for i, r in enumerate(reqs[:2]):
                r.check(tokens(dev, i), (vocab_size, i))
            assert stats(dev)["slots"][2] == (FREE, 0, 0, 0, 0)
            assert all((a == SENTINEL).all() for a in cache(sampled.eng))
    finally:
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs:
            r.free()
        m.free()


# ------------------------------------------------------------------ e. budget and cache edges

@pytest.mark.parametrize("graph", [0, 1])
def test_serve_budget_edges(dev, golden_dir, graph):
    """seq_len 16.  A: a one-token context and max_new = max_new_cap = seq_len - 1: 15 tokens, cache rows 0..14, row 15 never
    written.  B: 15 context tokens and max_new 1 at max_rows 4: PROMPT for four steps, then DONE with its one token, never
    DECODE.  C: n_context + max_new = 17 is refused and changes nothing"""
    m = open_model(dev, golden_dir, "ckpt_v2_q80_tied")
    assert m.cfg.seq_len == 16
    rng = np.random.default_rng(16 + graph)
    a, b, c = Req(dev, m, rng, 1, 15), Req(dev, m, rng, 15, 1, 1.0, 0.9, 0.64), Req(dev, m, rng, 9, 8)
    try:
        a.solo(); b.solo()
        assert a.ctx == [1]
        set_graph(dev, graph)
        assert begin(dev, m, 3, 4, 16) == EINVAL                  # max_new_cap beyond seq_len - 1
        assert begin(dev, m, 3, 4, 15) == 0
        assert admit(dev, 0, a) == 0 and admit(dev, 1, b) == 0
        by_slot = {0: a, 1: b}
        before = stats(dev)
        totals = counters(before)
        seen_b = []
        while live(before):
            if totals["steps"] == 2:
                assert admit(dev, 2, c) == EINVAL                 # 9 + 8 = 17 > seq_len
                assert stats(dev) == before
            before = step_and_compare(dev, before, 4, by_slot, totals)
            seen_b.append(before["slots"][1])
            assert totals["steps"] < 40
        # B shares steps of 4 rows with A's one row: 3 context positions a step; its fifth step feeds the last three and picks
        assert seen_b[:5] == [(PROMPT, 15, 3, 0, 1), (PROMPT, 15, 6, 0, 1), (PROMPT, 15, 9, 0, 1), (PROMPT, 15, 12, 0, 1), (DONE, 15, 15, 1, 1)]
        assert all(s == seen_b[4] for s in seen_b[4:])
        assert totals["steps"] == 15 and before["slots"] == [(DONE, 1, 15, 15, 15), (DONE, 15, 15, 1, 1), (FREE, 0, 0, 0, 0)]
        got_a, got_b = tokens(dev, 0), tokens(dev, 1)
        assert len(got_a) == 15 and len(got_b) == 1
        a.check(got_a, (graph, "A"))
        b.check(got_b, (graph, "B"))
        for kv in cache(a.eng):                                   # (check's own last clause, spelled out: row 15 of every layer)
            assert (kv[:, 15] == SENTINEL).all()
        assert all((kv == SENTINEL).all() for kv in cache(c.eng))
        assert before["captures"] == (1 if graph else 0) and before["generation"] == [1, 1, 0]
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in (a, b, c):
            r.free()
        m.free()
