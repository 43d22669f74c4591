"""The serving chain with a draft model on the GPU (rama_q8_serve_begin_model / _admit_model / _model_stats, Q8Server(draft=...)): a
DECODE slot's drafts are the next tokens of a small Q8 model and ride on the rows no slot wants.  Whatever the draft model, n_draft,
the samplers, the neighbours, max_rows and the graph mode, every request's tokens are bit for bit those of Q8Engine.generate on a twin
engine and its cache rows below its final cursor are the twin's; the draft cache's rows below the final draft cursor are those of a
fresh draft engine prefilled with the same tokens; nothing from row n_context - 1 + max_new on is written in either cache; the device's
row table, slot table, wants, grants and draft cursors equal serve_model_replay's after every step -- the draft engine's own generate
is the draft function -- and both reports equal its counters at the end.  Every comparison is exact.  The cases: tests/serve_model_cases.py."""
import ctypes as C
import time

import numpy as np
import pytest

from tests.serve_model_cases import (ARRIVALS, ARRIVALS_SHORT, DECODE, FREE, GREEDY, HOLE, NEAR_CONTEXT_SEED, NEAR_REQUEST, ONE, PAIRS, PROMPT,
                                     SAMPLED, WIDE)
from tests.test_hip_q8 import same_bits
from tests.test_hip_q8_serve import EINVAL, EUNSUP, SENTINEL, cache, fill_all, poll, set_graph, stats, steps, tokens
from tests.test_hip_q8_serve_spec import COUNTERS, spec_stats
from tests.test_hip_q8_spec_model import open_model

pytestmark = pytest.mark.gpu

MODEL_COUNTERS = ("draft_passes", "draft_rows_fed", "catch_up_rows")


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


class Models:
    """a target model and a draft model (one model twice for a pair with itself)"""

    def __init__(self, dev, golden_dir, target, draft):
        self.dev = dev
        self.m = open_model(dev, golden_dir, target)
        self.dm = self.m if draft == target else open_model(dev, golden_dir, draft)

    def free(self):
        if self.dm is not self.m:
            self.dm.free()
        self.m.free()


@pytest.fixture(scope="module")
def models(dev, golden_dir):
    made = {}

    def get(name):
        if name not in made:
            target, draft = PAIRS[name][:2] if name in PAIRS else (name, name)
            made[name] = Models(dev, golden_dir, target, draft)
        return made[name]
    yield get
    dev.lib.rama_q8_serve_end(dev.ctx)
    for p in made.values():
        p.free()


class MReq:
    """a request: its context (BOS first), its plan, the target and draft engines of its slot and a twin of each for the solo runs"""

    def __init__(self, mm, ctx, max_new, K, sampler=GREEDY, stop_at=None, n_cached=0):
        import rama_amd
        self.mm, self.ctx, self.max_new, self.K, self.n_cached = mm, list(ctx), max_new, K, n_cached
        self.T, self.topp, self.u = sampler
        d = mm.dev
        self.eng, self.twin = rama_amd.Q8Engine(d, mm.m), rama_amd.Q8Engine(d, mm.m)
        self.deng, self.dtwin = rama_amd.Q8Engine(d, mm.dm), rama_amd.Q8Engine(d, mm.dm)
        fill_all(self.eng); fill_all(self.deng)
        n = len(self.ctx)
        self.solo = self.twin.generate(self.ctx[1:], n - 1 + max_new, self.T, self.topp, self.u)[n - 1:]
        self.stop = -1 if stop_at is None else self.solo[stop_at]
        self._drafts = {}

    def want(self):
        return self.solo[:self.solo.index(self.stop) + 1] if self.stop in self.solo else list(self.solo)

    def draft_fn(self, prefix, n):
        """the draft model's own solo run behind a prefix, under the request's sampler"""
        key = (tuple(prefix), n)
        if key not in self._drafts:
            self._drafts[key] = self.dtwin.generate(prefix[1:], len(prefix) - 1 + n, self.T, self.topp, self.u)[len(prefix) - 1:]
        return self._drafts[key]

    def spec(self):
        return dict(context=self.ctx, max_new=self.max_new, stop_token=None if self.stop < 0 else self.stop, n_draft=self.K, n_cached=self.n_cached)

    def plan(self):
        from rama_amd._lib import rama_q8_serve_plan
        return rama_q8_serve_plan(self.T, self.topp, self.u, self.max_new, self.stop)

    def check(self, got, cursor, what):
        """the tokens; the target's rows below its final cursor; the draft's rows below the final draft cursor against a fresh prefill of the
        same tokens; the sentinel from row n_context - 1 + max_new on in both caches"""
        assert got == self.want(), what
        valid, untouched = len(self.ctx) + len(got) - 1, len(self.ctx) - 1 + self.max_new
        for a, b in zip(cache(self.eng), cache(self.twin)):
            assert same_bits(a[:, :valid], b[:, :valid]), what
            assert (a[:, untouched:] == SENTINEL).all(), what
        text = self.ctx + got
        assert len(self.ctx) <= cursor <= len(text), what
        self.dtwin.prefill(text[:cursor])
        for a, b in zip(cache(self.deng), cache(self.dtwin)):
            assert same_bits(a[:, :cursor], b[:, :cursor]), what
            assert (a[:, untouched:] == SENTINEL).all(), what

    def free(self):
        for e in (self.eng, self.twin, self.deng, self.dtwin):
            e.free()


def requests(mm, workload, seed=3):
    rng = np.random.default_rng(seed)
    V = mm.m.cfg.vocab_size
    return [MReq(mm, [1] + [int(t) for t in rng.integers(2, V, n_ctx - 1)], new, K, samp, stop_at) for n_ctx, new, K, samp, stop_at in workload[3]]


def arr(v):
    return (C.c_int32 * max(len(v), 1))(*v)


def begin_model(dev, mm, n_slots, max_rows, cap, n_draft_cap=15, m=None, dm=None):
    m, dm = m or mm.m, dm or mm.dm
    return dev.lib.rama_q8_serve_begin_model(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(dm.ccfg), C.byref(dm.weights), n_slots, max_rows,
                                             cap, n_draft_cap)


def admit_model(dev, slot, r, K=None, prefill=True, eng=None, deng=None, ctx=None, n_cached=None, plan=None):
    """the draft model's rows of the whole context (and the target's cached rows) enqueued first, then rama_q8_serve_admit_model"""
    ctx = r.ctx if ctx is None else ctx
    n_cached = r.n_cached if n_cached is None else n_cached
    eng, deng = eng or r.eng, deng or r.deng
    if prefill:
        deng.prefill(ctx)
        if n_cached:
            eng.prefill(ctx[:n_cached])
    p = r.plan() if plan is None else plan
    return dev.lib.rama_q8_serve_admit_model(dev.ctx, slot, C.byref(eng.state), C.byref(deng.state), arr(ctx), len(ctx), n_cached, C.byref(p),
                                             r.K if K is None else K)


def model_stats(dev):
    from rama_amd._lib import rama_q8_serve_model_report
    from rama_amd.q8 import serve_model_report
    r = rama_q8_serve_model_report()
    assert dev.lib.rama_q8_serve_model_stats(dev.ctx, C.byref(r)) == 0
    return serve_model_report(r)


def drive(dev, mm, reqs, workload, graph, what=None):
    """the workload under serve_model_replay's admission rule, one step at a time: after every step the device's row table, slot table, wanted and
    granted drafts and draft cursors against the replay's; at the end both reports, every request's tokens and both caches -> the replay"""
    from rama_amd.q8 import serve_model_replay
    n_slots, max_rows, use_slots = workload[:3]
    rp = serve_model_replay([r.spec() for r in reqs], [r.solo for r in reqs], [r.draft_fn for r in reqs], n_slots, max_rows, use_slots)
    set_graph(dev, graph)
    try:
        assert begin_model(dev, mm, n_slots, max_rows, max(r.max_new for r in reqs)) == 0
        who, got, cursor = {}, {}, {}
        for k, st in enumerate(rp["steps"]):
            for slot, q in st["admitted"]:
                assert admit_model(dev, slot, reqs[q]) == 0, (what, k, slot)
                who[slot] = q
            assert steps(dev, 1) == 0
            s, ss, ms = stats(dev), spec_stats(dev), model_stats(dev)
            assert s["rows"] == st["rows"], (what, k)
            assert s["slots"] == st["slots"], (what, k)
            assert (ss["last_want"], ss["last_granted"]) == (st["want"], st["granted"]), (what, k)
            assert [ms["draft_cursor"][i] for i in who] == [st["cursors"][i] for i in who], (what, k)
            for slot in st["finished"]:
                got[who[slot]], cursor[who[slot]] = tokens(dev, slot), ms["draft_cursor"][slot]
                assert poll(dev, slot)[:2] == (got[who[slot]], True), (what, k, slot)
        s, ss, ms = stats(dev), spec_stats(dev), model_stats(dev)
        assert {c: ss[c] for c in COUNTERS} == {c: rp["counters"][c] for c in COUNTERS}, what
        assert {c: ms[c] for c in MODEL_COUNTERS} == {c: rp["counters"][c] for c in MODEL_COUNTERS}, what
        assert s["captures"] == (1 if graph else 0), what
    finally:
        set_graph(dev, 0)
    assert sorted(got) == list(range(len(reqs))), what
    for q, r in enumerate(reqs):
        assert got[q] == rp["outputs"][q] and cursor[q] == rp["cursor"][q], (what, q)
        r.check(got[q], cursor[q], (what, q))
    return rp


def conditions(rp):
    """which of the five coverage conditions a run shows"""
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
    return seen


def arrivals(mm):
    return ARRIVALS if min(mm.m.cfg.seq_len, mm.dm.cfg.seq_len) >= 32 else ARRIVALS_SHORT


def run(dev, mm, workload, graph, what, seed=3):
    reqs = requests(mm, workload, seed)
    try:
        return drive(dev, mm, reqs, workload, graph, what)
    finally:
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs:
            r.free()


# ------------------------------------------------------------------ 1. the shapes, smallest first; the models; the settings

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("pair", ["untied<-untied", "untied<-tied"])
def test_one_slot_one_row_the_draft_cache_follows_without_a_grant(dev, models, pair, graph):
    """1 slot x 1 row: never an idle row, so g == 0 on every step -- the pure catch-up path"""
    rp = run(dev, models(pair), ONE, graph, (pair, graph))
    assert rp["counters"]["drafts_granted"] == 0 and rp["counters"]["draft_passes"] > 0 and rp["counters"]["drafts_wanted"] > 0
    assert all(g == 0 for st in rp["steps"] for g, _, _, _ in st["drafting"].values())


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("pair", ["gs8<-gs8", "untied<-tied"])
def test_three_slots_around_a_free_hole(dev, models, pair, graph):
    rp = run(dev, models(pair), HOLE, graph, (pair, graph))
    assert all(st["slots"][1][0] == FREE for st in rp["steps"]) and rp["counters"]["drafts_granted"] > 0


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_prompts_arrive_while_others_decode(dev, models, pair, graph):
    """4 x 16, n_draft 0, 1, 2, 7 and 15, greedy and sampled plans, a stop and a budget cut inside accepted runs, grants cut by an arriving prompt"""
    mm = models(pair)
    rp = run(dev, mm, arrivals(mm), graph, (pair, graph))
    assert {"0 < g < want", "g == 0 with a live catch-up row"} <= conditions(rp) or pair not in ("untied<-untied", "gs8<-gs8")
    if mm.dm is mm.m:                                             # a model drafting for itself: every granted draft is accepted
        assert rp["counters"]["drafts_accepted"] == rp["counters"]["drafts_granted"] > 0


@pytest.mark.parametrize("graph", [0, 1])
def test_sixty_four_slots_fill_the_first_draft_pass(dev, models, graph):
    rp = run(dev, models("ckpt_v2_q80_tied"), WIDE, graph, ("wide", graph))
    assert max(len(st["drafting"]) for st in rp["steps"]) == 64
    assert rp["counters"]["catch_up_rows"] > 0 and rp["counters"]["drafts_granted"] > 0


def test_every_coverage_condition_occurs(dev, models):
    """conditions, not measurements: the recorded cases must show every outcome of a drafting slot-step"""
    seen = conditions(run(dev, models("untied<-untied"), ARRIVALS, 1, "self"))
    seen |= conditions(run(dev, models("untied<-tied"), ARRIVALS_SHORT, 1, "unrelated"))
    mm = models("synth15m<-near")
    n_ctx, new, K, samp, _ = NEAR_REQUEST
    rng = np.random.default_rng(NEAR_CONTEXT_SEED)
    r = MReq(mm, [1] + [int(t) for t in rng.integers(0, mm.m.cfg.vocab_size, n_ctx - 1)], new, K, samp)
    try:
        seen |= conditions(drive(dev, mm, [r], (1, 8, None), 1, "near"))
    finally:
        dev.lib.rama_q8_serve_end(dev.ctx)
        r.free()
    assert seen == {"a == 0", "a == g > 0", "0 < a < g", "0 < g < want", "g == 0 with a live catch-up row"}, seen


# ------------------------------------------------------------------ 2. admissions

def test_admission_over_forked_rows_and_readmission_with_a_shorter_context(dev, models):
    mm = models("untied<-untied")
    d = dev
    rng = np.random.default_rng(11)
    V = mm.m.cfg.vocab_size
    long_ctx = [1] + [int(t) for t in rng.integers(2, V, 11)]
    a = MReq(mm, long_ctx, 9, 7, SAMPLED, n_cached=8)
    b = MReq(mm, long_ctx[:3], 12, 15, GREEDY)
    donor = MReq(mm, long_ctx[:9], 1, 0)
    try:
        assert begin_model(d, mm, 2, 8, 12) == 0
        # rows 0..7 of a's target cache come from a donor by rama_q8_kv_fork; the draft cache is prefilled whole
        donor.eng.prefill(long_ctx[:8])
        assert d.lib.rama_q8_kv_fork(d.ctx, C.byref(mm.m.ccfg), C.byref(donor.eng.state), C.byref(a.eng.state), 1, 8) == 0
        a.deng.prefill(a.ctx)
        assert admit_model(d, 0, a, prefill=False) == 0
        for _ in range(40):
            if poll(d, 0, 0, 1)[1]:
                break
            assert steps(d, 1) == 0 and d.lib.rama_sync(d.ctx) == 0
        got = tokens(d, 0)
        a.check(got, model_stats(d)["draft_cursor"][0], "forked")
        assert stats(d)["prompt"] == len(long_ctx) - 8
        # the same slot and the same two run states again, with a shorter context: the draft cursor starts over
        fill_all(a.eng); fill_all(a.deng)
        b.eng.free(); b.deng.free()
        b.eng, b.deng = a.eng, a.deng
        assert admit_model(d, 0, b) == 0
        for _ in range(40):
            if poll(d, 0, 0, 1)[1]:
                break
            assert steps(d, 1) == 0 and d.lib.rama_sync(d.ctx) == 0
        b.check(tokens(d, 0), model_stats(d)["draft_cursor"][0], "readmitted")
        assert poll(d, 0)[2] == 2
        b.eng, b.deng = None, None
    finally:
        d.lib.rama_q8_serve_end(d.ctx)
        for r in (a, donor):
            r.free()
        b.twin.free(); b.dtwin.free()


def test_admission_and_polling_while_a_block_is_in_flight(dev, models):
    mm = models("untied<-untied")
    reqs = requests(mm, (2, 8, None, [(3, 20, 7, GREEDY, None), (5, 14, 2, SAMPLED, None)]), 5)
    try:
        set_graph(dev, 1)
        assert begin_model(dev, mm, 2, 8, 20) == 0
        assert admit_model(dev, 0, reqs[0]) == 0
        assert steps(dev, 6) == 0
        assert admit_model(dev, 1, reqs[1]) == 0                  # behind the block in flight, with its draft prefill
        seen = []
        while dev.lib.rama_stream_query(dev.ctx) == 1:
            seen.append(len(poll(dev, 0)[0]))
        assert seen == sorted(seen)
        for _ in range(40):
            if poll(dev, 0, 0, 1)[1] and poll(dev, 1, 0, 1)[1]:
                break
            assert steps(dev, 2) == 0
            while dev.lib.rama_stream_query(dev.ctx) == 1:
                time.sleep(0.0002)
        ms = model_stats(dev)
        for slot, r in enumerate(reqs):
            r.check(tokens(dev, slot), ms["draft_cursor"][slot], ("in flight", slot))
        assert stats(dev)["captures"] == 1
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs:
            r.free()


# ------------------------------------------------------------------ 3. refusals and lifetimes

def test_every_refusal_leaves_the_chain_stepping(dev, models, golden_dir):
    from rama_amd._lib import rama_q8_serve_plan, rama_q8_serve_spec
    mm, other = models("untied<-tied"), models("gs8<-gs8")
    d = dev
    reqs = requests(mm, (3, 8, None, [(3, 13, 7, GREEDY, None), (2, 6, 2, SAMPLED, None), (2, 5, 1, GREEDY, None)]), 9)
    r0, r1, r2 = reqs
    try:
        assert begin_model(d, mm, 3, 8, 13, 7) == 0
        assert admit_model(d, 0, r0) == 0 and steps(d, 2) == 0
        # begin: the vocabulary, n_draft_cap, the slots of the first draft pass -- the running chain is untouched
        assert begin_model(d, mm, 3, 8, 13, 7, dm=other.m) == EINVAL
        assert begin_model(d, mm, 3, 8, 13, 0) == EINVAL and begin_model(d, mm, 3, 8, 13, 16) == EINVAL
        assert begin_model(d, mm, 65, 128, 9, 7) == EINVAL
        assert d.lib.rama_q8_serve_begin_model(d.ctx, C.byref(mm.m.ccfg), C.byref(mm.m.weights), None, C.byref(mm.dm.weights), 3, 8, 9, 7) == EINVAL
        # admit
        assert admit_model(d, 0, r1) == EINVAL                                        # busy
        assert admit_model(d, 1, r1, K=8) == EINVAL and admit_model(d, 1, r1, K=-1) == EINVAL
        assert admit_model(d, 1, r1, deng=r1.eng, prefill=False) == EINVAL            # dstate shares a cache with state (and is no draft-model state)
        assert admit_model(d, 1, r1, deng=r0.deng, prefill=False) == EINVAL           # a live slot's draft state
        assert admit_model(d, 1, r1, eng=r0.eng, prefill=False) == EINVAL             # a live slot's target state
        long_plan = rama_q8_serve_plan(0.0, 0.9, 0.0, 9, -1)
        assert admit_model(d, 1, r1, ctx=[1] + [5] * 8, plan=long_plan, prefill=False) == EINVAL      # 9 + 9 > the draft model's seq_len 16
        assert admit_model(d, 1, r1, n_cached=2, prefill=False) == EINVAL             # n_cached > n_context - 1
        p = r1.plan()
        assert d.lib.rama_q8_serve_admit_model(d.ctx, 1, C.byref(r1.eng.state), None, arr(r1.ctx), len(r1.ctx), 0, C.byref(p), 2) == EINVAL
        spec = rama_q8_serve_spec(2, 3, None, 0)
        assert d.lib.rama_q8_serve_admit_spec(d.ctx, 1, C.byref(r1.eng.state), arr(r1.ctx), len(r1.ctx), 0, C.byref(p), C.byref(spec)) == EINVAL
        # the plain admission on such a chain: n_draft = 0
        assert d.lib.rama_q8_serve_admit(d.ctx, 2, C.byref(r2.eng.state), arr(r2.ctx), len(r2.ctx), C.byref(r2.plan())) == 0
        assert admit_model(d, 1, r1) == 0
        for _ in range(40):
            if all(poll(d, s, 0, 1)[1] for s in range(3)):
                break
            assert steps(d, 1) == 0 and d.lib.rama_sync(d.ctx) == 0
        ms = model_stats(d)
        for slot in (0, 1):
            reqs[slot].check(tokens(d, slot), ms["draft_cursor"][slot], ("after the refusals", slot))
        assert tokens(d, 2) == r2.want() and spec_stats(d)["last_want"][2] == 0
        # the model entries on chains of the other kinds
        assert d.lib.rama_q8_serve_begin_spec(d.ctx, C.byref(mm.m.ccfg), C.byref(mm.m.weights), 3, 8, 9, 7, 0) == 0
        assert admit_model(d, 0, r0, prefill=False) == EINVAL
        from rama_amd._lib import rama_q8_serve_model_report
        assert d.lib.rama_q8_serve_model_stats(d.ctx, C.byref(rama_q8_serve_model_report())) == EINVAL
    finally:
        d.lib.rama_q8_serve_end(d.ctx)
        for r in reqs:
            r.free()


def test_an_unsupported_draft_shape_is_refused(dev, models):
    from oracle import oracle as O
    import rama_amd
    mm = models("untied<-untied")
    c = mm.m.cfg
    odd = rama_amd.Q8Model.synth(dev, O.Config(dim=64, hidden_dim=192, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=c.vocab_size, seq_len=8192,
                                               shared_weight=True), 32, 9)
    try:
        assert dev.lib.rama_q8_batch_shape_ok(C.byref(odd.ccfg)) == 0
        assert begin_model(dev, mm, 2, 4, 4, 7, dm=odd) == EUNSUP
        assert begin_model(dev, mm, 2, 4, 4, 7, m=odd) == EUNSUP
    finally:
        dev.lib.rama_q8_serve_end(dev.ctx)
        odd.free()


@pytest.mark.parametrize("gone", ["draft model", "draft state", "target state"])
def test_steps_refuse_once_a_model_or_a_live_run_state_is_freed(dev, golden_dir, gone):
    mm = Models(dev, golden_dir, "ckpt_v2_q80_untied", "ckpt_v2_q80_tied")
    r = MReq(mm, [1, 5, 9], 9, 7)
    try:
        assert begin_model(dev, mm, 2, 8, 9) == 0
        assert admit_model(dev, 0, r) == 0 and steps(dev, 2) == 0
        if gone == "draft model":
            mm.dm.free()
            mm.dm = mm.m
        elif gone == "draft state":
            r.deng.free()
        else:
            r.eng.free()
        assert steps(dev, 1) == EINVAL
        assert admit_model(dev, 1, r, prefill=False) == EINVAL
    finally:
        dev.lib.rama_q8_serve_end(dev.ctx)
        r.free()
        mm.free()


# ------------------------------------------------------------------ 4. the server

@pytest.mark.parametrize("pair", ["untied<-untied", "untied<-tied"])
def test_server_with_a_draft_model_gives_the_plain_servers_tokens(dev, models, pair):
    import rama_amd
    mm = models(pair)
    rng = np.random.default_rng(21)
    V = mm.m.cfg.vocab_size
    jobs = [([1] + [int(t) for t in rng.integers(2, V, n - 1)], new, samp) for n, new, samp in
            [(3, 9, GREEDY), (1, 6, SAMPLED), (6, 8, GREEDY), (2, 10, SAMPLED), (4, 5, GREEDY)]]
    twin = rama_amd.Q8Engine(dev, mm.m)
    solo = [twin.generate(c[1:], len(c) - 1 + new, *s)[len(c) - 1:] for c, new, s in jobs]
    twin.free()
    out = {}
    for kind in ("plain", "draft"):
        srv = rama_amd.Q8Server(mm.m, 3, 12, 10, **(dict(draft=mm.dm, n_draft=7) if kind == "draft" else {}))
        try:
            hs = [srv.submit(c, new, *s, n_draft=None if kind == "plain" else (7, 2, 0, 1, 7)[i]) for i, (c, new, s) in enumerate(jobs)]
            srv.run()
            out[kind] = [srv.result(h) for h in hs]
            st = srv.stats()
            if kind == "draft":
                assert st["model"]["draft_passes"] > 0 and st["spec"]["drafts_granted"] > 0 and st["graph_captures"] <= 1
        finally:
            srv.close()
    assert out["draft"] == out["plain"] == solo
    with pytest.raises(ValueError):
        rama_amd.Q8Server(mm.m, 3, 12, 10, draft=mm.dm, n_draft=7, hint_cap=8)
