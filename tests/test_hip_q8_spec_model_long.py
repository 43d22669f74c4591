"""The speculative chain with a draft model (rama_q8_spec_begin_model) at depth, with drafts of other shapes than their target and
over longer runs -- the cases of tests/spec_model_long_cases.py: the two-row catch-up pass across positions 64, 128, 256, 1024 and
2048; partial accepts at positions 300 and 2100; a draft larger than its target in every extent, then the roles swapped over the
grown scratches; the last rows of a draft's shorter window at position 1279; a stop token and a budget cut at position 1024; the
refusal of a sampled plan above 32768 tokens.  Everything goes through run_and_check of tests/test_hip_q8_spec_model.py: the tokens
against the target's solo run, both caches' rows against solo runs, the sentinel behind them, both reports against the replay.
Every comparison is exact: token lists, integer counters and float bit patterns.

The draft function of the replay.  Pair.draft_fn asks the draft twin for a whole solo run from position 0 at every step, which at
position 2100 costs 2100 forwards a step.  LongPair.draft_fn makes the same solo run incrementally on an engine of its own: the
rows of the prefix it does not hold yet by rama_q8_prefill, then one rama_q8_forward and one rama_sample_topp (Device::sample) per
drafted token.  test_the_incremental_drafter_is_the_draft_models_solo_run holds it against Pair.draft_fn."""
import ctypes as C

import pytest

from tests import q8_ref as R
from tests import spec_model_long_cases as MC
from tests.test_hip_q8 import same_bits
from tests.test_hip_q8_spec_model import (EINVAL, EUNSUP, SENTINEL, Pair, begin, caches, fill, open_model, replay, run_and_check, stats,
                                          steps, sums, tokens)

pytestmark = pytest.mark.gpu

GREEDY, SAMPLED = MC.GREEDY, MC.SAMPLED
PLANS = {"greedy": GREEDY, "sampled": SAMPLED}


def shape_ok(dev, m):
    return dev.lib.rama_q8_batch_shape_ok(C.byref(m.ccfg))


class LongPair(Pair):
    """Pair over two synthetic models of tests/spec_model_long_cases.py, with the incremental draft function"""

    def __init__(self, dev, name, models=None):
        import rama_amd
        self.dev, self.name = dev, name
        target, draft = models or [MC.MODELS[k] for k in MC.PAIRS[name]]
        self.m = open_model(dev, None, target)
        self.dm = self.m if draft == target else open_model(dev, None, draft)
        assert shape_ok(dev, self.m) == 1 and shape_ok(dev, self.dm) == 1, name        # before anything runs
        self.eng, self.twin = rama_amd.Q8Engine(dev, self.m), rama_amd.Q8Engine(dev, self.m)
        self.deng, self.dtwin = rama_amd.Q8Engine(dev, self.dm), rama_amd.Q8Engine(dev, self.dm)
        self.dsolo = rama_amd.Q8Engine(dev, self.dm)
        self.cfg = self.m.cfg
        self._solo, self._draft, self._inc, self._rows = {}, {}, {}, []

    def context(self, seed, n_ctx):
        return MC.context(seed, n_ctx, self.cfg.vocab_size)

    def draft_fn(self, T=0.0, P=0.9, u=0.0):
        def fn(prefix, n):
            key = (tuple(prefix), n, T, P, u)
            if key not in self._inc:
                self._inc[key] = self._continue(prefix, n, T, P, u)
            return self._inc[key]
        return fn

    def _continue(self, prefix, n, T, P, u):
        """the n tokens the draft model gives alone behind prefix; self._rows = the tokens whose rows self.dsolo's caches hold"""
        e, dev = self.dsolo, self.dev
        keep, lim = 0, min(len(self._rows), len(prefix) - 1)
        while keep < lim and self._rows[keep] == prefix[keep]:
            keep += 1
        if keep < len(prefix) - 1:
            e.prefill(prefix[keep:-1], keep)
        self._rows = list(prefix[:-1])
        out, tok, nxt = [], prefix[-1], C.c_int32()
        for pos in range(len(prefix) - 1, len(prefix) - 1 + n):
            e.forward(tok, pos)
            assert dev.lib.rama_sample_topp(dev.ctx, e.state.logits, self.cfg.vocab_size, T, P, u, C.byref(nxt)) == 0
            self._rows.append(tok)
            tok = int(nxt.value)
            out.append(tok)
        return out

    def free(self):
        self.dsolo.free()
        super().free()


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def pairs(dev):
    made = {}

    def get(name):
        if name not in made:
            made[name] = LongPair(dev, name)
        return made[name]
    yield get
    dev.lib.rama_q8_spec_end(dev.ctx)
    for p in made.values():
        p.free()


def discriminating(p, kind, ctx, K, max_new, plan, stop=None):
    """before the chain runs, with the models' real tokens: the restated chain keeps its invariants and is the replay, and every wrong
    rule of the case's kill list would break an invariant or change a counter the run compares -> (trajectory, cursor, step log)"""
    want, _, traj, cursor = replay(p, ctx, max_new, K, *plan, stop)
    fn = p.draft_fn(*plan)
    r_traj, r_cursor, broken, log = MC.restate(want, fn, ctx, K, max_new, stop)
    assert broken is None and (r_traj, r_cursor) == (traj, cursor), (p.name, kind, K, broken)
    assert MC.counters(traj, cursor) == sums(traj, cursor)
    left = MC.unkilled(MC.KILLS[kind], want, fn, ctx, K, max_new, stop)
    assert left == [], f"{p.name} {kind} K={K}: no counter changes and no invariant breaks under {left}; trajectory {traj}"
    return traj, cursor, log


# ------------------------------------------------------------------ 0. the shapes, the reference forward, the draft function

def test_the_cases_are_the_long_model_of_the_ngram_tests(dev):
    from tests.test_hip_q8_spec_long import LONG
    assert MC.MODELS["long"] == (LONG, 32, 11) and MC.MODELS["near"] == (LONG, 16, 11)      # (LongBench: Q8Model.synth(.., 32, 11))


@pytest.mark.parametrize("which", list(MC.MODELS))
def test_each_model_is_the_reference_forward_from_bos(pairs, which):
    """no test held the LONG shape (seq_len 2560, two layers) or any draft shape against tests/q8_ref.py so far: from BOS, Q8Ref over
    synth_q8 of the same configuration gives the twin's greedy tokens and its cache rows, bit for bit"""
    p, twin = {"long": ("long<-self", "twin"), "near": ("long<-near", "dtwin"), "wider": ("long<-wider", "dtwin"),
               "short": ("long<-short", "dtwin")}[which]
    eng = getattr(pairs(p), twin)
    cfg, gs, seed = MC.MODELS[which]
    assert eng.model.group_size == gs and eng.cfg.seq_len == cfg["seq_len"] and eng.cfg.dim == cfg["dim"]
    norms, t = R.synth_q8(cfg, gs, seed)
    ref = R.Q8Ref(cfg, gs, norms, t, (eng.model.tensor("freq_cis_real"), eng.model.tensor("freq_cis_imag")))
    n = MC.ANCHOR_POSITIONS
    assert eng.generate([], n, 0.0) == ref.generate([], n)
    shape = (cfg["n_layers"], cfg["seq_len"], cfg["dim"])
    for got, name in zip(caches(eng), ("key_cache", "value_cache")):
        assert same_bits(got[:, :n], ref.s[name].reshape(shape)[:, :n]), (which, name)


def test_the_incremental_drafter_is_the_draft_models_solo_run(pairs):
    for name, seed, cuts in (("long<-near", 3, ((290, 15), (120, 7), (270, 2), (271, 15))), ("long<-wider", MC.WIDER_SEED, ((1100, 15),))):
        p = pairs(name)
        ctx = p.context(seed, max(c for c, _ in cuts))
        for plan in (GREEDY, SAMPLED):
            whole, inc = Pair.draft_fn(p, *plan), p.draft_fn(*plan)
            for cut, n in cuts:
                assert inc(ctx[:cut], n) == whole(ctx[:cut], n), (name, plan, cut, n)


# ------------------------------------------------------------------ 1. the catch-up pair at each boundary

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("K", MC.BOUNDARY_KS)
@pytest.mark.parametrize("B", list(MC.BOUNDARIES))
def test_the_catch_up_pair_at_each_boundary(pairs, B, K, graph):
    p = pairs("long<-self")
    ctx, max_new = p.context(MC.BOUNDARY_SEED, MC.BOUNDARIES[B]), MC.BOUNDARY_MAX_NEW
    traj, _, log = discriminating(p, "boundary", ctx, K, max_new, GREEDY)
    # from the replay's trajectory: some drafting step opens with L - 1 == B one row behind: its first draft pass holds rows B - 1 and B
    opens = [len(ctx) + sum(e for _, _, e, _ in traj[:i]) for i in range(len(traj))]
    assert any(L - 1 == B and n_d > 0 and c == 1 for L, (n_d, _, _, c) in zip(opens, traj)), (B, K, traj)
    assert MC.opens_at(log, B)
    st, traj = run_and_check(p, ctx, max_new, K, graph=graph)
    assert all(a == n_d for n_d, a, _, _ in traj)
    assert st["catch_up_rows"] == sum(1 for n_d, _, _, _ in traj if n_d) - 1


# ------------------------------------------------------------------ 2. partial accepts at depth

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("K", MC.PARTIAL_KS)
@pytest.mark.parametrize("n_ctx", list(MC.PARTIAL_CONTEXTS))
def test_partial_accepts_at_depth(pairs, n_ctx, K, graph):
    p = pairs("long<-near")
    ctx, max_new = p.context(MC.PARTIAL_CONTEXTS[n_ctx], n_ctx), MC.PARTIAL_MAX_NEW
    traj, _, _ = discriminating(p, "partial", ctx, K, max_new, MC.PARTIAL_PLAN)
    cover = MC.partial_coverage(traj, K)
    print("partial", n_ctx, K, cover, traj)
    assert all(cover.values()), (n_ctx, K, cover, traj)
    run_and_check(p, ctx, max_new, K, *MC.PARTIAL_PLAN, graph=graph)
    _, traj = run_and_check(p, ctx, max_new, K, graph=graph)        # greedy: every draft accepted
    assert all(a == n_d for n_d, a, _, _ in traj)


# ------------------------------------------------------------------ 3. a draft larger than its target

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("n_ctx", MC.WIDER_CONTEXTS)
def test_a_draft_larger_than_its_target(pairs, n_ctx, graph):
    """(test_each_model_is_the_reference_forward_from_bos anchors both shapes)  long<-wider, then wider<-long over the scratches grown
    for the wide model, then long<-wider again: the same tokens and the same reports, one captured graph per chain"""
    p, q = pairs("long<-wider"), pairs("wider<-long")
    ctx, max_new = p.context(MC.WIDER_SEED, n_ctx), MC.WIDER_MAX_NEW
    for plan in (GREEDY, SAMPLED):
        for K in MC.WIDER_KS:
            st, traj = run_and_check(p, ctx, max_new, K, *plan, graph=graph)
            got = tokens(p.dev)
            print("wider", n_ctx, plan[0], K, "accepted", st["accepted"], "of", st["drafts"], "catch-up rows", st["catch_up_rows"])
            run_and_check(q, ctx, max_new, K, *plan, graph=graph)
            again, _ = run_and_check(p, ctx, max_new, K, *plan, graph=graph)
            assert tokens(p.dev) == got and again == st and again["graph_captures"] == graph


# ------------------------------------------------------------------ 4. the end of the draft's window at depth

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("plan", list(PLANS))
def test_the_end_of_the_drafts_window_at_depth(pairs, plan, graph):
    p = pairs("long<-short")
    dev, (T, P, u) = p.dev, PLANS[plan]
    ctx, max_new, K = p.context(MC.SHORT_SEED, MC.SHORT_N_CONTEXT), MC.SHORT_MAX_NEW, MC.SHORT_K
    assert len(ctx) + max_new == p.dm.cfg.seq_len < p.cfg.seq_len
    st, _ = run_and_check(p, ctx, max_new, K, T, P, u, graph=graph)
    got = tokens(dev)
    # one token more: refused, the finished chain's tokens and reports stay readable, neither cache is written
    fill(p.eng); fill(p.deng)
    assert begin(dev, p.m, p.eng, p.dm, p.deng, ctx, max_new + 1, T, P, u, K=K, prefill=False) == EINVAL
    assert tokens(dev) == got and stats(dev) == st
    for eng in (p.eng, p.deng):
        for g in caches(eng):
            assert (g == SENTINEL).all()


# ------------------------------------------------------------------ 5. stop and budget at depth

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("kind", ["budget", "stop"])
def test_stop_and_budget_at_depth(pairs, kind, graph):
    p = pairs("long<-self")
    dev = p.dev
    ctx, max_new, K = p.context(MC.ENDS_SEED, MC.ENDS_N_CONTEXT), MC.ENDS_MAX_NEW, MC.ENDS_K
    want, _ = p.solo(ctx, max_new, *SAMPLED)
    stop = want[MC.stop_index(want, max_new)] if kind == "stop" else None
    traj, cursor, _ = discriminating(p, kind, ctx, K, max_new, SAMPLED, stop)
    if kind == "budget":                                           # 51 tokens at 8 a step: the last step has 3 left and drafts 2
        assert traj == [(7, 7, 8, int(i > 0)) for i in range(6)] + [(2, 2, 3, 1)]
    st, _ = run_and_check(p, ctx, max_new, K, *SAMPLED, stop=stop, graph=graph)
    n_out = st["n_out"]
    assert (n_out == max_new) == (kind == "budget") and st["draft_cursor"] == cursor <= len(ctx) + n_out
    got = tokens(dev)
    below = lambda: [c[:, :len(ctx) - 1 + n_out] for c in caches(p.eng)] + [c[:, :cursor] for c in caches(p.deng)]
    before = below()
    # two steps after the finish: no token, no cache row below either cursor and no counter but `steps` changes.  (run_and_check has
    # left graph mode, which drops every captured graph: back in it, the two idle steps capture the chain's step once more and replay it)
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        assert steps(dev, 2) == 0
        assert tokens(dev) == got and stats(dev) == dict(st, steps=st["steps"] + 2, graph_captures=2 * graph)
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
    for g, r in zip(below(), before):
        assert same_bits(g, r)


# ------------------------------------------------------------------ 6. a sampled plan above 32768 tokens

def test_a_sampled_plan_above_32768_tokens_is_refused(dev):
    p = LongPair(dev, "big-vocabulary", MC.BIG_VOCAB_MODELS)
    try:
        n_ctx, max_new = MC.BIG_VOCAB_SHAPE
        ctx = p.context(5, n_ctx)
        assert p.cfg.vocab_size == p.dm.cfg.vocab_size == 32772
        T, P, u = SAMPLED
        assert begin(dev, p.m, p.eng, p.dm, p.deng, ctx, max_new, T, P, u, K=7) == EUNSUP
        for graph in (0, 1):                                       # greedy, the same pair begins and emits the solo tokens
            run_and_check(p, ctx, max_new, 7, graph=graph)
    finally:
        dev.lib.rama_q8_spec_end(dev.ctx)
        p.free()
