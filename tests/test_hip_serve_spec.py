"""Prompt caching and drafts on the serving chain in parity mode, on the GPU (rama_serve_admit_at / _begin_spec / _admit_spec / _spec_stats,
rama_amd.Server(n_draft=, prefix_cache=)).  Every comparison is exact, against parity-mode Engine.generate on each sequence alone, on a twin
engine: tokens, cache rows, the device's tables against the host rules and the pure-Python replay after every step.  The workloads are
tests/serve_spec_cases.py's; tests/test_serve_spec_host.py shows on the host that they reach what they are there for."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import serve_spec_cases as W
from tests.serve_cases import DECODE, DONE, FREE, PROMPT, TILE
from tests.test_hip_serve import (EINVAL, EUNSUP, SENTINEL, Req, admit, begin, cache, dev, models, plan_step, poll, same_bits,  # noqa: F401
                                  stats, steps, tokens)

pytestmark = pytest.mark.gpu


def set_graph(dev, on):
    dev.lib.rama_set_graph_mode(dev.ctx, int(on))


class SReq(Req):
    """a Case of the workloads on engines of its own: the solo run is the twin's"""

    def __init__(self, dev, cfg, m, case):
        super().__init__(dev, cfg, m, np.random.default_rng(0), len(case.ctx), case.max_new, case.T, case.topp, case.u, case.stop)
        self.ctx, self.case = list(case.ctx), case

    K = property(lambda self: self.case.K)
    N = property(lambda self: self.case.N)
    hint = property(lambda self: self.case.hint)
    n_cached = property(lambda self: self.case.n_cached)

    def spec(self):
        self.case.stop = self.stop
        return self.case.spec()

    def check_spec(self, got, what):
        """tokens, every cache row below the final cursor, and the sentinel from row n_context - 1 + max_new on"""
        assert got == self.want(), what
        valid, untouched = len(self.ctx) + len(got) - 1, len(self.ctx) - 1 + self.max_new
        for a, b in zip(cache(self.eng, self.cfg), cache(self.twin, self.cfg)):
            assert same_bits(a[:, :valid], b[:, :valid]), what
            assert (a[:, untouched:] == SENTINEL).all(), what


def build(dev, cfg, m, workload, *args):
    """a workload of serve_spec_cases over solo runs on the GPU -> (the workload, its SReqs)"""
    made = {}

    def solo(case):
        r = SReq(dev, cfg, m, case)
        made[id(case)] = r
        return r.solo()
    w = workload(solo, cfg.vocab_size, *args)
    reqs = [made.pop(id(c)) for c in w["cases"]]
    for r in made.values():                                       # (cases the builder tried and dropped)
        r.free()
    for r in reqs:
        r.stop = r.case.stop
    return w, reqs


def one(dev, cfg, m, rng, n_ctx, max_new, T=0.0, topp=0.9, u=0.0, stop=-1, **kw):
    case = W.Case(rng, cfg.vocab_size, n_ctx, max_new, T, topp, u, stop, **kw)
    r = SReq(dev, cfg, m, case)
    case.resolve(r.solo())
    return r


def begin_spec(dev, m, n_slots, max_rows, cap, n_draft_cap=15, hint_cap=W.HINT_CAP):
    return dev.lib.rama_serve_begin_spec(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), n_slots, max_rows, cap, n_draft_cap, hint_cap)


def i32(v):
    return (C.c_int32 * max(len(v), 1))(*v)


def admit_at(dev, slot, r, n_cached, ctx=None, eng=None):
    ctx, p = r.ctx if ctx is None else ctx, r.plan()
    return dev.lib.rama_serve_admit_at(dev.ctx, slot, C.byref((eng or r.eng).state), i32(ctx), len(ctx), n_cached, C.byref(p))


def admit_spec(dev, slot, r, K=None, N=None, hint=None, n_cached=None, ctx=None, eng=None, null=False):
    from rama_amd._lib import rama_q8_serve_spec
    ctx = r.ctx if ctx is None else ctx
    hint = r.hint if hint is None else hint
    p = r.plan()
    s = rama_q8_serve_spec(r.K if K is None else K, r.N if N is None else N, i32(hint) if hint else None, len(hint))
    return dev.lib.rama_serve_admit_spec(dev.ctx, slot, C.byref((eng or r.eng).state), i32(ctx), len(ctx),
                                         r.n_cached if n_cached is None else n_cached, C.byref(p), None if null else C.byref(s))


def spec_stats(dev):
    from rama_amd._lib import rama_q8_serve_spec_report
    from rama_amd.q8 import serve_spec_report
    r = rama_q8_serve_spec_report()
    assert dev.lib.rama_serve_spec_stats(dev.ctx, C.byref(r)) == 0
    return serve_spec_report(r)


def prefill(dev, m, eng, toks):
    assert dev.lib.rama_prefill(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state), i32(toks), len(toks), 0) == 0


def fork(dev, m, src, dst, n):
    return dev.lib.rama_q8_kv_fork(dev.ctx, C.byref(m.ccfg), C.byref(src.state), C.byref(dst.state), 1, n)


def finish(dev, reqs, bound=200):
    for _ in range(bound):
        if all(poll(dev, i)[1] for i in range(len(reqs))):
            return
        assert steps(dev, 1) == 0 and dev.lib.rama_sync(dev.ctx) == 0
    raise AssertionError("the chain did not finish")


@pytest.fixture
def tiny(dev, models):
    cfg, m = models("TINY")
    made = []
    yield cfg, m, made
    set_graph(dev, 0)
    dev.lib.rama_serve_end(dev.ctx)
    for r in made:
        r.free()


# ------------------------------------------------------------------ 1. admission over cached rows

@pytest.mark.parametrize("graph", [0, 1])
def test_admit_at_over_prefilled_and_forked_rows(dev, tiny, graph):
    """n_cached 1, the middle and n_context - 1; rows written by rama_prefill on the slot's own engine or forked from a donor's; tails longer than
    max_rows; greedy and sampled; a stop token.  After every step the device's row and slot tables are rama_q8_serve_plan_step's"""
    cfg, m, made = tiny
    rng = np.random.default_rng(71)
    sizes = [(40, 5, 1), (40, 6, 20), (40, 4, 39), (13, 7, 6)]
    reqs = [one(dev, cfg, m, rng, n, new, *W.PLANS[1 + i % 3]) for i, (n, new, _) in enumerate(sizes)]
    made += reqs
    reqs[1].stop = reqs[1].solo()[3]
    donor = one(dev, cfg, m, rng, 2, 1)
    made.append(donor)
    set_graph(dev, graph)
    assert begin(dev, m, 4, 8, 8) == 0
    table = []
    for i, (r, (_, _, n_cached)) in enumerate(zip(reqs, sizes)):
        if i % 2:                                                 # the rows come from a donor that ingested the whole context
            prefill(dev, m, donor.eng, r.ctx)
            assert fork(dev, m, donor.eng, r.eng, n_cached) == 0
        else:
            prefill(dev, m, r.eng, r.ctx[:n_cached])
        assert admit_at(dev, i, r, n_cached) == 0
        table.append((PROMPT, len(r.ctx), n_cached, 0, r.max_new))
    assert len(reqs[0].ctx) - 1 > 8                               # a tail longer than max_rows
    for k in range(60):
        if all(s[0] == DONE for s in table):
            break
        rows, after = plan_step(table, 8)
        assert steps(dev, 1) == 0
        s = stats(dev)
        assert s["rows"] == rows, k
        stopped = [i for i, (a, b) in enumerate(zip(s["slots"], after)) if a != b]
        assert all(s["slots"][i][0] == DONE and reqs[i].stop >= 0 for i in stopped), k      # (the plan does not see a stop token)
        table = s["slots"]
    for i, r in enumerate(reqs):
        r.check(tokens(dev, i), (graph, i))
    assert len(tokens(dev, 1)) < reqs[1].max_new                  # (the stop token fell)
    assert stats(dev)["captures"] == (1 if graph else 0)


def test_a_next_chat_turn_on_the_same_run_state(dev, tiny):
    cfg, m, made = tiny
    rng = np.random.default_rng(72)
    first = one(dev, cfg, m, rng, 9, 6, 1.0, 0.9, 0.4)
    made.append(first)
    assert begin(dev, m, 2, 8, 8) == 0 and admit(dev, 0, first) == 0
    finish(dev, [first])
    out = tokens(dev, 0)
    first.check(out, "the first turn")
    turn = one(dev, cfg, m, rng, 5, 5, 0.7, 1.0, 0.2)            # the user's next words, behind the conversation so far
    made.append(turn)
    turn.ctx = first.ctx + out + turn.ctx[1:]
    turn._solo = None
    n_cached = len(first.ctx) + len(out) - 1                      # every token but the last one recorded has been fed
    assert admit_at(dev, 1, turn, n_cached, eng=first.eng) == 0
    for _ in range(12):
        assert steps(dev, 1) == 0
    got = tokens(dev, 1)
    assert got == turn.want() and stats(dev)["slots"][1][0] == DONE
    last = len(turn.ctx) + len(got) - 2
    for a, b in zip(cache(first.eng, cfg), cache(turn.twin, cfg)):
        assert same_bits(a[:, :last + 1], b[:, :last + 1]) and (a[:, last + 1:] == SENTINEL).all()


def test_the_fork_refuses_a_destination_in_a_live_fp32_slot(dev, tiny):
    cfg, m, made = tiny
    rng = np.random.default_rng(73)
    a, b = one(dev, cfg, m, rng, 5, 6), one(dev, cfg, m, rng, 3, 1)
    made += [a, b]
    assert begin(dev, m, 2, 8, 8) == 0 and admit(dev, 0, a) == 0 and admit(dev, 1, b) == 0
    assert steps(dev, 2) == 0 and dev.lib.rama_sync(dev.ctx) == 0
    assert poll(dev, 1)[1] and not poll(dev, 0)[1]
    assert fork(dev, m, b.eng, a.eng, 2) == EINVAL                # a is live
    assert fork(dev, m, a.eng, b.eng, 2) == 0                     # b has finished; a live source is fine below its cursor
    finish(dev, [a])
    a.check(tokens(dev, 0), "after the refused fork")


def test_server_with_a_prefix_cache_against_the_cache_off_run(dev, models):
    """8 requests over 2 shared prefixes and a third that evicts one: Server(prefix_cache=2) against Server() and the solo runs"""
    import rama_amd
    cfg, m = models("TINY")
    rng = np.random.default_rng(74)
    prefixes = [[1] + [int(t) for t in rng.integers(2, cfg.vocab_size, n)] for n in (17, 11, 9)]
    order = [0, 1, 0, 1, 2, 0, 1, 2]
    reqs = []
    for i, p in enumerate(order):
        r = one(dev, cfg, m, rng, 1 + i % 4, 3 + i % 3, *W.PLANS[i % 5])
        r.ctx = prefixes[p] + r.ctx[1:] + [2 + i]
        r._solo = None
        reqs.append(r)
    try:
        results = {}
        for k in (2, 0):
            srv = rama_amd.Server(m, 2, max_rows=8, max_new_cap=8, prefix_cache=k)
            hs = []
            for i, r in enumerate(reqs):                          # one at a time: a request finds the donors its predecessors left
                hs.append(srv.submit(r.ctx, r.max_new, r.T, r.topp, r.u, retain=i in (0, 1, 4)))      # each prefix's first request stays as its donor
                srv.run()
            results[k] = [srv.result(h) for h in hs]
            st = srv.stats()
            if k:
                assert st["rows_cached"] > 0 and len(srv.pool) == 2
                assert srv.cached(hs[0]) == 0 and srv.cached(hs[2]) >= len(prefixes[0]) and srv.cached(hs[3]) >= len(prefixes[1])
                assert srv.cached(hs[5]) == 0                     # prefix 0's donor went when prefix 2's came: the eviction
                assert srv.cached(hs[7]) >= len(prefixes[2])
            else:
                assert st["rows_cached"] == 0
            srv.close()
        assert results[2] == results[0] == [r.want() for r in reqs]
    finally:
        for r in reqs:
            r.free()


# ------------------------------------------------------------------ 2. drafts

COUNTERS = ("steps", "rows_decode", "rows_draft", "rows_prompt", "rows_idle", "drafts_wanted", "drafts_granted", "drafts_accepted",
            "tokens_emitted", "accepted_hist")


def drive(dev, m, reqs, n_slots, max_rows, use_slots=None, what=None):
    """the workload under serve_spec_replay's admission rule, one step at a time: after every step the device's row table, slot table and wanted /
    granted drafts against the replay's; at the end the counters, every request's tokens and cache rows -> (the replay, the device's trace)"""
    from rama_amd.q8_replay import serve_spec_replay
    rp = serve_spec_replay([r.spec() for r in reqs], [r.solo() for r in reqs], n_slots, max_rows, use_slots)
    assert begin_spec(dev, m, n_slots, max_rows, max(r.max_new for r in reqs)) == 0
    who, got, trace = {}, {}, []
    before = [(FREE, 0, 0, 0, 0)] * n_slots
    for k, st in enumerate(rp["steps"]):
        for slot, q in st["admitted"]:
            assert admit_spec(dev, slot, reqs[q]) == 0, (what, k, slot)
            who[slot] = q
            before[slot] = (PROMPT, len(reqs[q].ctx), reqs[q].n_cached, 0, reqs[q].max_new)
        assert steps(dev, 1) == 0
        s, ss = stats(dev), spec_stats(dev)
        assert s["rows"] == st["rows"], (what, k)
        assert s["slots"] == st["slots"], (what, k)
        assert (ss["last_want"], ss["last_granted"]) == (st["want"], st["granted"]), (what, k)
        trace.append((list(before), s["slots"], ss["last_want"], ss["last_granted"]))
        before = list(s["slots"])
        for slot in st["finished"]:
            got[who[slot]] = tokens(dev, slot)
            assert poll(dev, slot)[:2] == (got[who[slot]], True), (what, k, slot)
    s, ss = stats(dev), spec_stats(dev)
    assert {c: ss[c] for c in COUNTERS} == rp["counters"], what
    assert (s["steps"], s["decode"], s["prompt"], s["idle"]) == tuple(rp["counters"][c] for c in ("steps", "rows_decode", "rows_prompt", "rows_idle"))
    assert ss["rows_draft"] == ss["drafts_granted"] and sum(ss["accepted_hist"]) == ss["rows_decode"]
    assert sorted(got) == list(range(len(reqs))), what
    for q, r in enumerate(reqs):
        assert got[q] == rp["outputs"][q], (what, q)
        r.check_spec(got[q], (what, q))
    return rp, trace


@pytest.mark.parametrize("graph", [0, 1])
def test_mixed_workload_equals_the_replay_and_reaches_every_outcome(dev, tiny, graph):
    cfg, m, made = tiny
    w, reqs = build(dev, cfg, m, W.mixed)
    made += reqs
    set_graph(dev, graph)
    rp, trace = drive(dev, m, reqs, w["n_slots"], w["max_rows"], what=graph)
    assert W.outcomes(trace) == W.SIX, W.SIX - W.outcomes(trace)
    assert stats(dev)["captures"] == (1 if graph else 0)


@pytest.mark.parametrize("kind", ["own", "corrupt", None])
def test_hint_kinds_at_8_16_and_40_rows_and_around_a_free_hole(dev, tiny, kind):
    cfg, m, made = tiny
    w, reqs = build(dev, cfg, m, W.hints, kind)
    made += reqs
    set_graph(dev, 1)
    for max_rows, use in W.LAYOUTS:
        for r in reqs:
            for name in ("key_cache", "value_cache"):
                r.eng.set_buffer(name, np.full(cfg.n_layers * cfg.seq_len * cfg.dim, SENTINEL))
        rp, trace = drive(dev, m, reqs, w["n_slots"], max_rows, use, what=(kind, max_rows, use))
        c = rp["counters"]
        assert c["drafts_granted"] > 0
        if kind == "own":
            assert c["drafts_accepted"] == c["drafts_granted"]
        if kind == "corrupt":
            assert c["drafts_accepted"] < c["drafts_granted"]
        if use:
            assert all(t[1][1][0] == FREE for t in trace)
        assert stats(dev)["captures"] == 1


@pytest.mark.parametrize("graph", [0, 1])
def test_a_decode_slot_across_row_32_then_an_idle_second_tile(dev, tiny, graph):
    cfg, m, made = tiny
    w, reqs = build(dev, cfg, m, W.straddle)
    made += reqs
    set_graph(dev, graph)
    rp, trace = drive(dev, m, reqs, w["n_slots"], w["max_rows"], what=graph)
    assert any(st["rows"][TILE - 1][0] == st["rows"][TILE][0] and st["rows"][TILE][0] in st["accepted"] for st in rp["steps"])
    assert any(all(x == (-1, -1, 0) for x in st["rows"][TILE:]) for st in rp["steps"])


def test_a_spec_chain_without_drafts_is_the_plain_chain(dev, tiny):
    cfg, m, made = tiny
    rng = np.random.default_rng(75)
    sizes = [(1, 6), (3, 4), (11, 5), (2, 7)]
    reqs = [one(dev, cfg, m, rng, n, new, *((1.0, 0.9, 0.4) if i % 2 else (0.0, 0.9, 0.0))) for i, (n, new) in enumerate(sizes)]
    twins = [one(dev, cfg, m, rng, n, new) for n, new in sizes]
    made += reqs + twins
    tables = {}
    for kind in ("plain", "spec"):
        assert (begin(dev, m, 4, 6, 8) if kind == "plain" else begin_spec(dev, m, 4, 6, 8, 7, 0)) == 0
        for i, r in enumerate(reqs):
            eng = r.eng if kind == "spec" else twins[i].eng
            if kind == "plain" or i == 1:                         # (rama_serve_admit and _admit_at on a spec chain admit with n_draft = 0)
                assert admit_at(dev, i, r, 0, eng=eng) == 0
            elif i == 3:
                assert dev.lib.rama_serve_admit(dev.ctx, i, C.byref(eng.state), i32(r.ctx), len(r.ctx), C.byref(r.plan())) == 0
            else:
                assert admit_spec(dev, i, r, K=0) == 0
        tables[kind] = []
        for _ in range(14):
            assert steps(dev, 1) == 0
            s = stats(dev)
            tables[kind].append((s["rows"], s["slots"]))
        tables[kind].append([tokens(dev, i) for i in range(4)])
        if kind == "spec":
            ss = spec_stats(dev)
            assert ss["rows_draft"] == ss["drafts_wanted"] == ss["drafts_granted"] == 0 and ss["accepted_hist"][0] == ss["rows_decode"]
    assert tables["plain"] == tables["spec"]
    for i, r in enumerate(reqs):
        r.check(tables["spec"][-1][i], i)


def test_admit_spec_over_rows_forked_from_a_live_speculating_donor(dev, tiny):
    cfg, m, made = tiny
    rng = np.random.default_rng(76)
    donor = one(dev, cfg, m, rng, 6, 40, 1.0, 0.9, 0.35, K=7, N=2, hint="corrupt")
    heir = one(dev, cfg, m, rng, 2, 9, 1.0, 0.9, 0.7, K=7, N=3)
    made += [donor, heir]
    set_graph(dev, 1)
    assert begin_spec(dev, m, 2, 12, 40) == 0
    assert admit_spec(dev, 0, donor) == 0
    assert steps(dev, 6) == 0 and dev.lib.rama_sync(dev.ctx) == 0
    seen = poll(dev, 0)[0]
    assert 6 <= len(seen) < 40 and not poll(dev, 0)[1]
    heir.ctx = donor.ctx + seen                                   # the rows of all of it but the last token lie below the donor's cursor
    heir._solo = None
    heir.case.ctx, heir.case.n_cached = heir.ctx, len(heir.ctx) - 1
    heir.case.kind = "own"
    heir.case.resolve(heir.solo())
    assert fork(dev, m, donor.eng, heir.eng, heir.n_cached) == 0
    assert admit_spec(dev, 1, heir) == 0
    assert steps(dev, 40) == 0 and dev.lib.rama_sync(dev.ctx) == 0
    for i, r in enumerate([donor, heir]):
        assert poll(dev, i)[1]
        r.check_spec(tokens(dev, i), i)
    ss = spec_stats(dev)
    assert 0 < ss["drafts_accepted"] and ss["rows_prompt"] == len(donor.ctx) + 1


@pytest.mark.parametrize("graph", [0, 1])
def test_admission_and_polling_while_a_block_is_in_flight(dev, tiny, graph):
    cfg, m, made = tiny
    rng = np.random.default_rng(77 + graph)
    reqs = [one(dev, cfg, m, rng, 3, 6, K=7, hint="own"), one(dev, cfg, m, rng, 5, 30, 1.0, 0.9, 0.2, K=7, hint="corrupt"),
            one(dev, cfg, m, rng, 9, 30, 0.7, 1.0, 0.5, K=4, N=2, periodic=3)]
    late = one(dev, cfg, m, rng, 12, 8, 0.7, 1.0, 0.45, K=7, hint="own")
    made += reqs + [late]
    set_graph(dev, graph)
    assert begin_spec(dev, m, 3, 8, 30) == 0
    for i, r in enumerate(reqs):
        assert admit_spec(dev, i, r) == 0
    assert steps(dev, 24) == 0
    deadline = time.monotonic() + 60
    while True:                                                   # no stream query, no synchronising call
        for i, r in enumerate(reqs):
            got, fin, _ = poll(dev, i)
            assert got == r.want()[:len(got)] and (not fin or got == r.want()), i
        if poll(dev, 0)[1]:
            break
        assert time.monotonic() < deadline, "slot 0 never finished"
    assert admit_spec(dev, 0, late) == 0
    assert steps(dev, 30) == 0 and dev.lib.rama_sync(dev.ctx) == 0
    for i, r in enumerate([late] + reqs[1:]):
        assert poll(dev, i)[1]
        r.check_spec(tokens(dev, i), (graph, i))
    assert stats(dev)["captures"] == (1 if graph else 0)


def test_server_with_drafts_against_the_plain_server_and_the_solo_runs(dev, models):
    import rama_amd
    cfg, m = models("TINY")
    rng = np.random.default_rng(78)
    reqs = [one(dev, cfg, m, rng, int(rng.integers(1, 20)), int(rng.integers(3, 14)), *W.PLANS[i % 5], hint="own" if i % 2 else None,
                periodic=i % 2 == 0 and 2) for i in range(8)]
    try:
        reqs[4].stop = reqs[4].solo()[len(reqs[4].solo()) // 2]
        results = {}
        for K in (7, 0):
            set_graph(dev, 1)
            srv = rama_amd.Server(m, 3, max_rows=40, max_new_cap=16, n_draft=K, ngram=3, hint_cap=W.HINT_CAP if K else 0)
            hs = [srv.submit(r.ctx, r.max_new, r.T, r.topp, r.u, None if r.stop < 0 else r.stop,
                             **(dict(hint=r.hint, n_draft=None if i % 3 else 3) if K else {})) for i, r in enumerate(reqs)]
            srv.run()
            st = srv.stats()
            results[K] = [srv.result(h) for h in hs]
            assert all(srv.finished(h) for h in hs) and ("spec" in st) == bool(K)
            if K:
                assert st["spec"]["drafts_accepted"] > 0 and st["spec"]["tokens_emitted"] == sum(len(r) for r in results[K])
            srv.close()
        assert results[7] == results[0] == [r.want() for r in reqs]
    finally:
        set_graph(dev, 0)
        for r in reqs:
            r.free()


# ------------------------------------------------------------------ 3. the classifier guard

def logits_rows(dev):
    lg, rows, V = C.POINTER(C.c_float)(), C.c_int(), C.c_int()
    dev.lib.rama_internal_serve_logits.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert dev.lib.rama_internal_serve_logits(dev.ctx, C.byref(lg), C.byref(rows), C.byref(V)) == 0
    return C.cast(lg, C.c_void_p).value, rows.value, V.value


@pytest.mark.parametrize("graph", [0, 1])
def test_a_tile_without_a_logits_row_is_not_classified(dev, tiny, graph):
    """tile 1's logits rows hold a sentinel: a step in which the tile has only rows inside a context leaves it; the next step, in which the tile
    holds slot 1's final context row, picks that row's token as the solo run does"""
    cfg, m, made = tiny
    w, reqs = build(dev, cfg, m, W.guard)
    made += reqs
    set_graph(dev, graph)
    assert begin_spec(dev, m, 2, 40, 8, 0, 0) == 0
    for i, r in enumerate(reqs):
        assert admit_spec(dev, i, r) == 0
    base, rows, V = logits_rows(dev)
    assert (rows, V) == (40, cfg.vocab_size)
    n = (rows - TILE) * V
    fill = np.full(n, SENTINEL)
    assert dev.lib.rama_copy_h2d_f32(dev.ctx, C.c_void_p(base + 4 * TILE * V), fill.ctypes.data, n) == 0
    assert steps(dev, 1) == 0
    s = stats(dev)
    assert all(x[0] == 1 and x[2] == 0 for x in s["rows"][TILE:]) and s["rows"][29] == (0, 29, 1)
    back = np.empty(n, np.float32)
    assert dev.lib.rama_download_f32(dev.ctx, C.c_void_p(base + 4 * TILE * V), n, back.ctypes.data) == 0
    assert (back == SENTINEL).all(), "a tile without a logits row was classified"
    assert poll(dev, 0)[0] == reqs[0].want()[:1]
    assert steps(dev, 1) == 0
    s = stats(dev)
    assert s["rows"][36] == (1, 45, 1)
    assert dev.lib.rama_download_f32(dev.ctx, C.c_void_p(base + 4 * TILE * V), n, back.ctypes.data) == 0
    assert not (back.reshape(-1, V)[36 - TILE] == SENTINEL).any()
    assert poll(dev, 1)[0] == reqs[1].want()[:1]
    finish(dev, reqs)
    for i, r in enumerate(reqs):
        r.check_spec(tokens(dev, i), (graph, i))


# ------------------------------------------------------------------ 4. refusals and lifetimes

def test_refusals_leave_the_running_chain_as_it_was(dev, tiny):
    from rama_amd._lib import check, rama_q8_serve_spec_report
    cfg, m, made = tiny
    V = cfg.vocab_size
    rng = np.random.default_rng(79)
    reqs = [one(dev, cfg, m, rng, 3, 9, 1.0, 0.9, 0.3, K=5, hint="own"), one(dev, cfg, m, rng, 11, 7, K=3, N=2, periodic=2)]
    extra = one(dev, cfg, m, rng, 4, 6, K=5, hint="own")
    made += reqs + [extra]
    L, ctx = dev.lib, dev.ctx
    for bad in [(16, 8), (-1, 8), (3, -1)]:                       # n_draft_cap in 0..15, hint_cap >= 0; and rama_serve_begin's own checks
        assert begin_spec(dev, m, 3, 8, 12, *bad) == EINVAL
    assert begin_spec(dev, m, 4, 3, 12) == EINVAL and begin_spec(dev, m, 3, 8, 0) == EINVAL and begin_spec(dev, m, 0, 8, 12) == EINVAL
    assert begin(dev, m, 3, 8, 12) == 0                           # a plain chain takes no drafting admission and has no spec report
    assert admit_spec(dev, 0, extra) == EINVAL
    assert L.rama_serve_spec_stats(ctx, C.byref(rama_q8_serve_spec_report())) == EINVAL
    assert admit_at(dev, 0, extra, len(extra.ctx)) == EINVAL and admit_at(dev, 0, extra, -1) == EINVAL
    assert admit(dev, 0, extra) == 0 and steps(dev, 1) == 0       # ... and is intact
    set_graph(dev, 1)
    assert begin_spec(dev, m, 3, 8, 12, 5, 20) == 0
    for i, r in enumerate(reqs):
        assert admit_spec(dev, i, r) == 0
    assert steps(dev, 2) == 0
    check(L.rama_set_tuning(ctx, b"ref_order", 0))               # leaving parity mode: neither a new chain nor a step
    try:
        assert begin_spec(dev, m, 3, 8, 12, 5, 20) == EUNSUP and steps(dev, 1) == EUNSUP
    finally:
        check(L.rama_set_tuning(ctx, b"ref_order", 1))
    refused = [
        admit_spec(dev, 2, extra, K=6),                           # beyond n_draft_cap
        admit_spec(dev, 2, extra, K=-1),
        admit_spec(dev, 2, extra, N=0), admit_spec(dev, 2, extra, N=5),
        admit_spec(dev, 2, extra, hint=[1] * 21),                 # beyond hint_cap
        admit_spec(dev, 2, extra, hint=[1, V]), admit_spec(dev, 2, extra, hint=[-1]),
        admit_spec(dev, 2, extra, null=True),
        admit_spec(dev, 0, extra),                                # serve_admit's own: a busy slot, a live run state, sizes
        admit_spec(dev, 2, extra, eng=reqs[1].eng),
        admit_spec(dev, 2, extra, n_cached=len(extra.ctx)),
        admit_spec(dev, 2, extra, ctx=[1] * (cfg.seq_len - 5)),   # n_context + max_new beyond seq_len
        admit_spec(dev, 2, extra, ctx=[1, V]),
        admit_spec(dev, 3, extra), admit_spec(dev, -1, extra),
    ]
    assert refused == [EINVAL] * len(refused)
    assert L.rama_serve_spec_stats(ctx, None) == EINVAL and steps(dev, -1) == EINVAL
    assert admit_spec(dev, 2, extra) == 0                         # ... and a good one still goes in
    assert steps(dev, 16) == 0 and L.rama_sync(ctx) == 0
    for i, r in enumerate(reqs + [extra]):
        assert poll(dev, i)[1]
        r.check_spec(tokens(dev, i), i)
    assert stats(dev)["captures"] == 2                            # (a change of "ref_order" drops every captured graph: the step was captured again)


def test_released_copies_are_made_again_and_the_step_is_captured_again(dev, tiny):
    cfg, m, made = tiny
    rng = np.random.default_rng(80)
    r = one(dev, cfg, m, rng, 5, 12, 1.0, 0.9, 0.6, K=7, hint="own")
    made.append(r)
    set_graph(dev, 1)
    assert begin_spec(dev, m, 2, 8, 12) == 0 and admit_spec(dev, 0, r) == 0
    assert steps(dev, 2) == 0 and dev.lib.rama_sync(dev.ctx) == 0
    assert stats(dev)["captures"] == 1
    m.release_copies(1)
    import rama_amd
    other = rama_amd.Engine(dev, m)                               # (takes freed memory: the copies made again land elsewhere)
    assert steps(dev, 1) == 0 and dev.lib.rama_sync(dev.ctx) == 0
    other.free()
    assert stats(dev)["captures"] == 2
    finish(dev, [r])
    r.check_spec(tokens(dev, 0), "across the release")


def test_state_free_of_a_live_slot_ends_a_chain_with_drafts(dev, tiny):
    cfg, m, made = tiny
    rng = np.random.default_rng(81)
    a, b = one(dev, cfg, m, rng, 3, 2, K=3, hint="own"), one(dev, cfg, m, rng, 4, 20, K=0)
    set_graph(dev, 1)
    assert begin_spec(dev, m, 2, 6, 20) == 0
    assert admit_spec(dev, 0, a) == 0 and admit_spec(dev, 1, b) == 0
    assert steps(dev, 3) == 0 and dev.lib.rama_sync(dev.ctx) == 0
    assert poll(dev, 0)[1] and not poll(dev, 1)[1]
    a.eng.free()                                                  # DONE as the host can see it
    assert steps(dev, 1) == 0
    b.eng.free()
    assert steps(dev, 1) == EINVAL and admit_spec(dev, 0, b, eng=b.twin) == EINVAL
    assert dev.lib.rama_serve_end(dev.ctx) == 0
    a.twin.free(); b.twin.free()


def test_a_q8_chain_with_drafts_and_the_fp32_one_on_one_context(dev, tiny, golden_dir):
    import rama_amd
    from rama_amd._lib import rama_q8_serve_plan, rama_q8_serve_spec
    cfg, m, made = tiny
    rng = np.random.default_rng(82)
    reqs = [one(dev, cfg, m, rng, 5, 10, 1.0, 0.9, 0.3, K=7, hint="own"), one(dev, cfg, m, rng, 11, 6, K=3, N=2, periodic=2)]
    made += reqs
    qm = rama_amd.Q8Model.load(dev, golden_dir / "ckpt_v2_q80_tied.bin")
    qe, qt = rama_amd.Q8Engine(dev, qm), rama_amd.Q8Engine(dev, qm)
    qctx = [1] + [int(t) for t in rng.integers(2, qm.cfg.vocab_size, 4)]
    qwant = [int(t) for t in qt.generate(qctx[1:], len(qctx) - 1 + 8, 0.0, 0.9, 0.0)][len(qctx) - 1:]
    L, ctx = dev.lib, dev.ctx
    set_graph(dev, 1)
    try:
        assert L.rama_q8_serve_begin_spec(ctx, C.byref(qm.ccfg), C.byref(qm.weights), 1, 8, 8, 7, 32) == 0
        assert begin_spec(dev, m, 2, 8, 10) == 0
        plan, hint = rama_q8_serve_plan(0.0, 0.9, 0.0, 8, -1), i32(qctx + qwant)
        qs = rama_q8_serve_spec(7, 3, hint, len(qctx) + 8)
        assert L.rama_q8_serve_admit_spec(ctx, 0, C.byref(qe.state), i32(qctx), len(qctx), 0, C.byref(plan), C.byref(qs)) == 0
        for i, r in enumerate(reqs):
            assert admit_spec(dev, i, r) == 0
        for _ in range(14):                                       # stepping in turn
            assert steps(dev, 1) == 0
            assert L.rama_q8_serve_steps(ctx, 1) == 0
        assert L.rama_sync(ctx) == 0
        for i, r in enumerate(reqs):
            r.check_spec(tokens(dev, i), f"fp32 slot {i}")
        buf, k = (C.c_int32 * 16)(), C.c_int()
        assert L.rama_q8_serve_tokens(ctx, 0, buf, 16, C.byref(k)) == 0
        assert [int(buf[i]) for i in range(k.value)] == qwant
        assert stats(dev)["captures"] == 1 and spec_stats(dev)["drafts_accepted"] > 0
    finally:
        set_graph(dev, 0)
        L.rama_q8_serve_end(ctx)
        qe.free(); qt.free(); qm.free()
