"""The serving chain's drafting kernel on texts longer than its workgroup (serve_draft_kernel: 256 threads, 4 waves, per slot): the
cases of tests/spec_long_cases.py at threads = 256, several resident at once, so that neighbouring rows of the hint table and of
the text table hold different long texts; a slot admitted again under a short request while its rows still hold a long hint and
a long text; Q8Server with hints of 2000 to 3000 tokens.  A request's context is prefilled and admitted over its cached rows
(n_cached = n_context - 1): the admission step emits one token without drafting, so the tail n-gram of the first draft ends with
that token (spec_long_cases' lead = 1).  Every case is asserted discriminating with the model's real run before the chain starts.
After every step the row table, the slot table and the wanted / granted drafts are serve_spec_replay's; at the end the counters,
the tokens and the cache rows.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import spec_long_cases as SL
from tests import test_hip_q8_serve_spec as SS
from tests.test_hip_q8_serve import DECODE, set_graph
from tests.test_hip_q8_serve_spec import SReq, drive, spec_stats
from tests.test_hip_q8_spec import N_SEEDS
from tests.test_hip_q8_spec_long import LONG

pytestmark = pytest.mark.gpu

MAX_NEW, THREADS, HINT_CAP = 24, 256, 3072


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


@pytest.fixture
def long_hints(monkeypatch):
    """drive starts its chain with the short tests' hint_cap: here it takes 3072"""
    monkeypatch.setattr(SS, "begin_spec", functools.partial(SS.begin_spec, hint_cap=HINT_CAP))


def open_long(dev):
    import rama_amd
    return rama_amd.Q8Model.synth(dev, O.Config(**LONG), 32, 11)


class LReq(SReq):
    """a request with an explicit context, prefilled into its run state and admitted over the cached rows"""

    def __init__(self, dev, m, ctx, max_new=MAX_NEW, K=SL.N_DRAFT, N=3, hint=None):
        super().__init__(dev, m, np.random.default_rng(0), 1, max_new, K=K, N=N, hint=hint)
        self.ctx = list(ctx)

    def set_context(self, ctx):
        if list(ctx) != self.ctx:
            self.ctx, self._solo = list(ctx), None
        return self

    def ready(self):
        if len(self.ctx) > 1:
            self.eng.prefill(self.ctx[:-1], 0)
        self.n_cached = len(self.ctx) - 1
        return self


def settled_request(dev, m, case):
    """the case built for the model's real run (asserted discriminating: settle raises otherwise) as a request ready to admit"""
    name, n, ngram = case
    r = LReq(dev, m, [1], N=ngram)
    try:
        c, ref = SL.settle(name, n, ngram, THREADS, 1, MAX_NEW, lambda ctx: r.set_context(ctx).solo(), m.cfg.vocab_size, N_SEEDS)
    except BaseException:
        r.free()
        raise
    assert r.ctx == c.context and r.solo() == ref
    r.hint, r.case = list(c.hint), c
    return r.ready()


def lone(r):
    """what the request shows alone: (want, granted, accepted, emitted) per step, from the restated rule"""
    return [(n_d, n_d, a, emit) for n_d, a, emit in
            SL.replay(r.solo(), r.ctx, r.hint, r.K, r.N, r.max_new, THREADS, lead=1)]


def per_request(rp, n_reqs):
    """serve_spec_replay's steps, per request: (want, granted, accepted, emitted) for every step it has a row in"""
    out, who = [[] for _ in range(n_reqs)], {}
    for st in rp["steps"]:
        for slot, q in st["admitted"]:
            who[slot] = q
        for slot, emit in st["emitted"].items():
            out[who[slot]].append((st["want"][slot], st["granted"][slot], st["accepted"].get(slot, 0), emit))
    return out


def run_cases(dev, m, cases, use_slots, graph, pad_first=False):
    reqs = []
    try:
        for case in cases:
            reqs.append(settled_request(dev, m, case))
        if pad_first:                                             # a hint of exactly hint_cap tokens: filler behind the case's own
            r = reqs[0]
            r.hint = (r.hint + r.hint[:40] * (HINT_CAP // 40 + 1))[:HINT_CAP]
            c = r.case._replace(hint=r.hint)
            assert len(r.hint) == HINT_CAP and SL.undiscriminated(c, r.solo(), MAX_NEW) == []
        for r in reqs:
            assert SL.undiscriminated(r.case._replace(hint=r.hint), r.solo(), MAX_NEW) == [], r.case.name
            print(r.case.name, r.case.n, r.N, "context", len(r.ctx), "hint", len(r.hint), "ref", r.solo()[:4], "alone", lone(r)[:3])
        set_graph(dev, graph)
        rp, trace = drive(dev, m, reqs, 4, 32, use_slots, what=(cases, graph))
        # no grant is cut (two residents, 2 + 15 + 15 rows): every request shows in this run what it shows alone
        assert per_request(rp, len(reqs)) == [lone(r) for r in reqs]
        assert spec_stats(dev)["hint_cap"] == HINT_CAP
        assert max(sum(1 for s in before if s[0] == DECODE) for before, _, _, _ in trace) == 2
        return rp
    finally:
        SS.free_all(dev, reqs, m)


def test_long_cases_two_residents_graph_mode(dev, long_hints):
    run_cases(dev, open_long(dev), SL.SERVE[:6], [1, 2], 1)


def test_long_cases_two_residents_eager_and_a_hint_of_hint_cap_tokens(dev, long_hints):
    """slot 0 takes H-third with its hint padded to exactly hint_cap tokens; P-hint and P-long put rows above position 2000"""
    cases = [("H-third", 1, 4)] + [c for c in SL.SERVE[6:]] + [("H-sweep", 4, 4)]
    run_cases(dev, open_long(dev), cases, [0, 1], 0, pad_first=True)


def test_a_slot_admitted_again_does_not_read_its_old_texts(dev, long_hints):
    """slot 1 serves a request with a 3000-token hint and a 2200-token context that hold the NEXT request's tail 3-gram far out,
    with that request's true continuation behind it; the next request (context 12, hint 40) takes the slot when the first is DONE.
    A kernel that read beyond the new n_hint or L would draft 15 right tokens; the replay knows the new texts only."""
    m = open_long(dev)
    V = m.cfg.vocab_size
    rng = np.random.default_rng(77)
    new = LReq(dev, m, [1] + [int(t) for t in rng.choice(np.arange(2, V), 11, replace=False)], N=3)
    old = LReq(dev, m, [1], max_new=4, N=3)
    try:
        ref = new.solo()
        gram, cont = (new.ctx + ref[:1])[-3:], ref[1:16]
        allowed = np.array([t for t in range(2, V) if t not in set(gram) | set(new.ctx)])
        fill = lambda k: [int(t) for t in rng.choice(allowed, k)]
        new.hint = fill(40)
        old.hint = fill(3000)
        old.hint[2900 - 3:2900 + 15] = gram + cont
        octx = [1] + fill(2199)
        octx[2100 - 3:2100 + 15] = gram + cont
        old.set_context(octx)
        # the condition, before the chain runs: the stale texts would change what the short request shows
        true = SL.replay(ref, new.ctx, new.hint, 15, 3, MAX_NEW, THREADS, lead=1)
        stale = SL.replay(ref, new.ctx, new.hint + old.hint[40:], 15, 3, MAX_NEW, THREADS, lead=1)
        assert true != stale and stale[1] == (15, 15, 16) and true[1][1] < 15
        assert SL.occurrence_ends(octx, gram, (len(new.ctx) + MAX_NEW + 3, len(octx)), THREADS) == [2100]
        old.ready(); new.ready()
        set_graph(dev, 1)
        rp, _ = drive(dev, m, [old, new], 4, 32, [1], what="stale")
        assert rp["slot"] == [1, 1] and per_request(rp, 2)[1] == [(n_d, n_d, a, e) for n_d, a, e in true]
    finally:
        SS.free_all(dev, [old, new], m)


def test_server_with_long_hints_against_solo_runs_and_the_plain_server(dev):
    """Q8Server(n_draft=15, ngram=4, hint_cap=3072): three requests whose hints of 2000 to 3000 tokens hold their own text deep
    inside; the tokens of the solo runs and of the plain server"""
    import rama_amd
    m = open_long(dev)
    V = m.cfg.vocab_size
    rng = np.random.default_rng(91)
    plans = [(1.0, 0.9, 0.3), (0.7, 1.0, 0.6), (1.0, 0.9, 0.8)]    # sampled: a greedy run of this model repeats one token
    reqs = [SReq(dev, m, rng, n_ctx, MAX_NEW, *plan, K=15, N=4) for n_ctx, plan in zip((5, 9, 3), plans)]
    try:
        for r, (n_hint, at) in zip(reqs, ((2000, 1500), (2600, 2300), (3000, 2900))):
            text = r.ctx + r.solo()
            r.hint = [int(t) for t in rng.integers(2, V, n_hint)]
            r.hint[at:at + len(text)] = text
            r.hint = r.hint[:n_hint]
        results = {}
        for K in (15, 0):
            set_graph(dev, 1)
            srv = rama_amd.Q8Server(m, 3, max_rows=48, max_new_cap=MAX_NEW, n_draft=K, ngram=4, hint_cap=HINT_CAP if K else 0)
            hs = [srv.submit(r.ctx, r.max_new, r.T, r.topp, r.u, None, **(dict(hint=r.hint) if K else {})) for r in reqs]
            srv.run()
            results[K] = [srv.result(h) for h in hs]
            if K:
                st = srv.stats()["spec"]
                assert st["drafts_accepted"] >= 15 and st["tokens_emitted"] == 3 * MAX_NEW and st["steps"] < MAX_NEW
            srv.close()
        assert results[15] == results[0] == [r.want() for r in reqs]
    finally:
        SS.free_all(dev, reqs, m)
