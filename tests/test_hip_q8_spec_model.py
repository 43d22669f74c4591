"""The speculative chain with a draft model on the GPU (rama_q8_spec_begin_model / rama_q8_spec_model_stats,
Q8Engine.generate_spec(draft=...)): whatever the draft model, n_draft, the sampler and the graph mode, the tokens are bit for bit those
of Q8Engine.generate on the target alone and the target's cache rows below its cursor are that run's; the draft's cache rows below the
draft cursor are those of a fresh draft engine prefilled with the same tokens; the device's counters are spec_model_replay's, with the
draft engine's own solo generate as the draft function; stops, budgets, the last rows of the context windows, refusals and
lifetimes.  Every comparison is exact: token lists and float bit patterns.  The pairs and shapes: tests/spec_model_cases.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.spec_model_cases import CONTEXT_SEED, CONTEXT_SEEDS, COVERAGE, N_DRAFTS, NEAR_SEED, PAIRS, SAMPLERS, STORIES15M
from tests.test_hip_q8 import same_bits

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -2
SENTINEL = np.float32(123.25)


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


def open_model(dev, golden_dir, which):
    """which = a fixture's name, "synth15m/<gs>", or the (configuration, group size, seed) of any synthetic model"""
    import rama_amd
    if not isinstance(which, str):
        cfg, gs, seed = which
        return rama_amd.Q8Model.synth(dev, O.Config(**cfg), gs, seed)
    if which.startswith("synth15m/"):
        return rama_amd.Q8Model.synth(dev, O.Config(**STORIES15M), int(which.split("/")[1]), NEAR_SEED)
    return rama_amd.Q8Model.load(dev, golden_dir / f"{which}.bin")


def arr(v):
    return (C.c_int32 * max(len(v), 1))(*v)


def caches(eng):
    c = eng.cfg
    n = c.n_layers * c.seq_len * c.dim
    return eng.buffer("key_cache", n).reshape(c.n_layers, c.seq_len, c.dim), eng.buffer("value_cache", n).reshape(c.n_layers, c.seq_len, c.dim)


def fill(eng):
    """a sentinel in every cache row"""
    c = eng.cfg
    for name in ("key_cache", "value_cache"):
        eng.set_buffer(name, np.full(c.n_layers * c.seq_len * c.dim, SENTINEL))


class Pair:
    """a target model and a draft model (one model twice for a pair with itself), the chain's two engines and a twin of each for the
    solo runs, which are computed once and kept"""

    def __init__(self, dev, golden_dir, name):
        import rama_amd
        self.dev, self.name = dev, name
        target, draft, self.shape = PAIRS[name]
        self.m = open_model(dev, golden_dir, target)
        self.dm = self.m if draft == target else open_model(dev, golden_dir, draft)
        self.eng, self.twin = rama_amd.Q8Engine(dev, self.m), rama_amd.Q8Engine(dev, self.m)
        self.deng, self.dtwin = rama_amd.Q8Engine(dev, self.dm), rama_amd.Q8Engine(dev, self.dm)
        self.cfg = self.m.cfg
        self._solo, self._draft = {}, {}

    def context(self, seed=None, n_ctx=None):
        seed = CONTEXT_SEEDS.get(self.name, CONTEXT_SEED) if seed is None else seed
        n_ctx = self.shape[0] if n_ctx is None else n_ctx
        rng = np.random.default_rng(seed)
        return [1] + [int(t) for t in rng.integers(0, self.cfg.vocab_size, n_ctx - 1)]

    def solo(self, ctx, max_new, T=0.0, P=0.9, u=0.0):
        """the max_new tokens the target gives alone behind ctx (not cut at any stop token), and the twin's caches after that run"""
        key = (tuple(ctx), max_new, T, P, u)
        if key not in self._solo:
            toks = self.twin.generate(ctx[1:], len(ctx) - 1 + max_new, T, P, u)[len(ctx) - 1:]
            self._solo[key] = (toks, caches(self.twin))
        return self._solo[key]

    def draft_fn(self, T=0.0, P=0.9, u=0.0):
        """spec_model_replay's draft function: the draft model's own solo run behind a prefix, under the plan's sampler"""
        def fn(prefix, n):
            key = (tuple(prefix), n, T, P, u)
            if key not in self._draft:
                self._draft[key] = self.dtwin.generate(prefix[1:], len(prefix) - 1 + n, T, P, u)[len(prefix) - 1:]
            return self._draft[key]
        return fn

    def free(self):
        for e in (self.eng, self.twin, self.deng, self.dtwin):
            e.free()
        if self.dm is not self.m:
            self.dm.free()
        self.m.free()


@pytest.fixture(scope="module")
def pairs(dev, golden_dir):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Pair(dev, golden_dir, name)
        return made[name]
    yield get
    dev.lib.rama_q8_spec_end(dev.ctx)
    for p in made.values():
        p.free()


def begin(dev, m, eng, dm, deng, ctx, max_new, T=0.0, P=0.9, u=0.0, stop=-1, K=7, N=3, hint=None, n_hint=None, prefill=True,
          n_context=None, null=()):
    """the context's first n - 1 positions prefilled into both engines, then rama_q8_spec_begin_model -> its return code"""
    from rama_amd._lib import rama_q8_spec_plan
    if prefill and len(ctx) > 1:
        eng.prefill(ctx[:-1], 0)
        deng.prefill(ctx[:-1], 0)
    h = arr(hint or [])
    plan = rama_q8_spec_plan(T, P, u, max_new, stop, K, N, h if hint else None, len(hint or []) if n_hint is None else n_hint)

    def ref(name, obj):
        return None if name in null else C.byref(obj)
    return dev.lib.rama_q8_spec_begin_model(None if "ctx" in null else dev.ctx, ref("cfg", m.ccfg), ref("w", m.weights), ref("state", eng.state),
                                            ref("dcfg", dm.ccfg), ref("dw", dm.weights), ref("dstate", deng.state),
                                            None if "context" in null else arr(ctx), len(ctx) if n_context is None else n_context,
                                            ref("plan", plan))


def steps(dev, n):
    return dev.lib.rama_q8_spec_steps(dev.ctx, n)


def tokens(dev, cap=256):
    out, n = (C.c_int32 * cap)(), C.c_int()
    assert dev.lib.rama_q8_spec_tokens(dev.ctx, out, cap, C.byref(n)) == 0
    return [int(out[i]) for i in range(n.value)]


def stats(dev):
    """rama_q8_spec_stats and rama_q8_spec_model_stats as one dict"""
    from rama_amd._host import _report
    from rama_amd._lib import rama_q8_spec_model_report, rama_q8_spec_report
    r, q = rama_q8_spec_report(), rama_q8_spec_model_report()
    assert dev.lib.rama_q8_spec_stats(dev.ctx, C.byref(r)) == 0 and dev.lib.rama_q8_spec_model_stats(dev.ctx, C.byref(q)) == 0
    return dict(_report(r), **_report(q))


def sums(traj, cursor):
    """what the device's counters must show after the steps of a replayed trajectory"""
    hist = [0] * 16
    for _, a, _, _ in traj:
        hist[a] += 1
    return dict(steps=len(traj), rows_fed=sum(n + 1 for n, _, _, _ in traj), drafts=sum(n for n, _, _, _ in traj),
                accepted=sum(a for _, a, _, _ in traj), emitted=sum(e for _, _, e, _ in traj), accepted_hist=hist,
                draft_passes=sum(n for n, _, _, _ in traj), draft_rows_fed=sum(n + c for n, _, _, c in traj),
                catch_up_rows=sum(c for _, _, _, c in traj), draft_cursor=cursor)


def replay(p, ctx, max_new, K, T=0.0, P=0.9, u=0.0, stop=None):
    from rama_amd.q8 import spec_model_replay
    want, twin_cache = p.solo(ctx, max_new, T, P, u)
    traj, cursor = spec_model_replay(want, p.draft_fn(T, P, u), ctx, K, max_new, stop)
    return want, twin_cache, traj, cursor


def run_and_check(p, ctx, max_new, K, T=0.0, P=0.9, u=0.0, stop=None, graph=0):
    """the chain over p.eng and p.deng for exactly the replayed number of steps, and everything the header promises of it"""
    dev = p.dev
    want, twin_cache, traj, cursor = replay(p, ctx, max_new, K, T, P, u, stop)
    n_out = sum(e for _, _, e, _ in traj)
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        fill(p.eng); fill(p.deng)
        assert begin(dev, p.m, p.eng, p.dm, p.deng, ctx, max_new, T, P, u, -1 if stop is None else stop, K) == 0
        assert steps(dev, len(traj)) == 0
        got = tokens(dev)
        st = stats(dev)
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
    what = (p.name, K, T, stop, graph)
    # 1. the tokens are the target's own, cut after the stop token
    assert got == want[:n_out], what
    assert stop is None or got[-1] == stop or n_out == max_new, what
    # 4. the counters of both reports are the replay's
    ref = sums(traj, cursor)
    assert {k: st[k] for k in ref} == ref, what
    assert st["finished"] == 1 and st["n_out"] == n_out and st["cursor"] == len(ctx) - 1 + n_out, what
    # 6. one captured graph for the whole run
    assert st["graph_captures"] == graph, what
    # 2. the target's rows below its cursor are the solo run's; 5. nothing at or beyond n_context - 1 + max_new is written
    valid, first_untouched = len(ctx) - 1 + n_out, len(ctx) - 1 + max_new
    for g, r in zip(caches(p.eng), twin_cache):
        assert same_bits(g[:, :valid], r[:, :valid]), what
        assert (g[:, first_untouched:] == SENTINEL).all(), what
    # 3. the draft's rows below the draft cursor are a fresh draft engine's over the same tokens; 5. as above
    s = ctx + got
    assert 0 <= cursor <= len(s), what
    draft_cache = caches(p.deng)
    if cursor > 0:
        p.dtwin.prefill(s[:cursor], 0)
        for g, r in zip(draft_cache, caches(p.dtwin)):
            assert same_bits(g[:, :cursor], r[:, :cursor]), what
    for g in draft_cache:
        assert (g[:, first_untouched:] == SENTINEL).all(), what
    return st, traj


# ------------------------------------------------------------------ 1. the grid: pairs x n_draft x sampler x graph mode

@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("n_draft", N_DRAFTS)
@pytest.mark.parametrize("name", list(PAIRS))
def test_tokens_rows_and_counters(dev, pairs, name, n_draft, sampler):
    p = pairs(name)
    n_ctx, max_new = p.shape
    T, P, u = SAMPLERS[sampler]
    ctx = p.context()
    for graph in (0, 1):
        st, traj = run_and_check(p, ctx, max_new, n_draft, T, P, u, graph=graph)
    target, draft, _ = PAIRS[name]
    if target == draft:
        # a model drafting for itself: every draft accepted, a catch-up row on every drafting step but the first
        assert all(a == n_d for n_d, a, _, _ in traj)
        assert [c for n_d, _, _, c in traj if n_d] == [0] + [1] * (sum(1 for n_d, _, _, _ in traj if n_d) - 1)
        assert st["steps"] == -(-max_new // (n_draft + 1))


def test_the_runs_end_at_the_last_row_of_a_context_window(pairs):
    for name in ("untied<-untied", "gs8<-gs8"):
        p = pairs(name)
        assert sum(p.shape) == p.cfg.seq_len
    p = pairs("untied<-tied")
    assert sum(p.shape) == p.dm.cfg.seq_len < p.cfg.seq_len


def test_every_accept_outcome_occurs(pairs):
    """the coverage condition of tests/spec_model_cases.py, on the replays of the grid cases it names: the chain itself runs them in
    test_tokens_rows_and_counters, where the device's histogram must equal the replay's"""
    seen = {}
    for kind, (name, K, sampler) in COVERAGE.items():
        assert name in PAIRS and K in N_DRAFTS and sampler in SAMPLERS
        p = pairs(name)
        _, _, traj, _ = replay(p, p.context(), p.shape[1], K, *SAMPLERS[sampler])
        seen[kind] = sorted({a for n_d, a, _, _ in traj if n_d == K})
        ok = dict(none=0 in seen[kind], full=K in seen[kind], partial=any(0 < a < K for a in seen[kind]))[kind]
        assert ok, (kind, name, K, sampler, traj)


# ------------------------------------------------------------------ 2. ends

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("name", ["untied<-untied", "synth15m<-near"])
def test_a_stop_token_mid_run(pairs, name, graph):
    p = pairs(name)
    n_ctx, max_new = p.shape
    T, P, u = SAMPLERS["sampled"]                                  # (a synthetic model's greedy run repeats one token)
    ctx = p.context()
    want, _ = p.solo(ctx, max_new, T, P, u)
    idx = next(i for i in range(max_new // 2, max_new - 1) if want[i] not in want[:i])
    st, traj = run_and_check(p, ctx, max_new, 7, T, P, u, stop=want[idx], graph=graph)
    assert st["n_out"] == idx + 1 < max_new
    # steps after the finish: all-idle passes that change no token and no counter but `steps`
    dev = p.dev
    assert steps(dev, 2) == 0
    assert stats(dev) == dict(st, steps=st["steps"] + 2) and tokens(dev) == want[:idx + 1]


def test_a_budget_that_cuts_inside_an_accepted_run(pairs):
    """a model drafting for itself, 27 tokens at 8 a step: the last step has 3 left, drafts 2, both are accepted, the pick is the last"""
    p = pairs("untied<-untied")
    n_ctx, max_new = p.shape
    _, traj = run_and_check(p, p.context(), max_new, 7, graph=1)
    assert traj == [(7, 7, 8, 0), (7, 7, 8, 1), (7, 7, 8, 1), (2, 2, 3, 1)]


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("name", list(PAIRS))
def test_bos_alone(pairs, name, graph):
    """n_context == 1: nothing prefilled on either engine; to the end of the shorter context window on the fixtures"""
    p = pairs(name)
    max_new = min(p.cfg.seq_len, p.dm.cfg.seq_len, 25) - 1
    run_and_check(p, [1], max_new, 7, graph=graph)
    run_and_check(p, [1], 1, 15, graph=graph)                      # max_new == 1: one step, no draft row


# ------------------------------------------------------------------ 3. refusals and lifetimes

def test_refusals_leave_a_running_chain_intact(dev, pairs, golden_dir):
    import rama_amd
    p, q = pairs("untied<-untied"), pairs("untied<-tied")
    g8 = pairs("gs8<-gs8")
    n_ctx, max_new = p.shape
    ctx = p.context()
    want, _ = p.solo(ctx, max_new)
    V, S = p.cfg.vocab_size, p.cfg.seq_len
    other, dother = rama_amd.Q8Engine(dev, p.m), rama_amd.Q8Engine(dev, q.dm)
    long_m = rama_amd.Q8Model.synth(dev, O.Config(dim=64, hidden_dim=192, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=64, seq_len=8192,
                                                  shared_weight=True), 32, 9)
    long_e = rama_amd.Q8Engine(dev, long_m)
    assert dev.lib.rama_set_graph_mode(dev.ctx, 1) == 0
    try:
        assert begin(dev, p.m, p.eng, p.m, p.deng, ctx, max_new, K=1) == 0
        assert steps(dev, 2) == 0
        done = 2

        def refused(code, m=p.m, eng=other, dm=q.dm, deng=dother, c=(1, 2, 3), **kw):
            """the call is refused with `code`, and the running chain's next step still emits its own tokens"""
            nonlocal done
            kw = dict(dict(max_new=4, K=2), **kw)
            assert begin(dev, m, eng, dm, deng, list(c), prefill=False, **kw) == code, kw
            assert steps(dev, 1) == 0
            done += 1
            got = tokens(dev)
            assert got == want[:len(got)] and len(got) == min(2 * done, max_new), kw

        for null in ("ctx", "cfg", "w", "state", "dcfg", "dw", "dstate", "context", "plan"):
            refused(EINVAL, null=(null,))
        # the draft side: the vocabulary, the draft's seq_len (16), a shared run state, a hint, n_draft
        refused(EINVAL, dm=g8.m, deng=g8.deng)                     # vocabulary 37 against 64
        refused(EINVAL, max_new=14)                                # 3 + 14 > 16, well inside the target's 32
        refused(EINVAL, dm=p.m, deng=other)                        # dstate is state
        refused(EINVAL, hint=[1, 2])
        refused(EINVAL, n_hint=2)
        for K in (0, -1, 16):
            refused(EINVAL, K=K)
        # everything rama_q8_spec_begin refuses
        for kw in (dict(T=-1.0), dict(T=float("nan")), dict(P=1.5), dict(P=-0.1), dict(u=1.0), dict(u=-0.5), dict(stop=V), dict(stop=-2),
                   dict(n_context=0), dict(max_new=0), dict(c=(1, V, 3)), dict(c=(1, -1, 3))):
            refused(EINVAL, **kw)
        refused(EINVAL, dm=p.m, deng=p.deng, max_new=S - 2)        # beyond the target's seq_len
        # a shape the token-batch pass does not take, on either side
        assert dev.lib.rama_q8_batch_shape_ok(C.byref(long_m.ccfg)) == 0
        refused(EUNSUP, dm=long_m, deng=long_e)
        refused(EUNSUP, m=long_m, eng=long_e, dm=p.m, deng=p.deng)
        assert steps(dev, -1) == EINVAL
        assert steps(dev, max(0, -(-max_new // 2) - done)) == 0
        assert tokens(dev) == want
        st = stats(dev)
        assert st["graph_captures"] == 1 and st["finished"] == 1 and st["accepted"] == st["drafts"]
        # ngram is ignored: any value begins; and n_context + max_new == the draft's seq_len is taken
        assert begin(dev, p.m, other, q.dm, dother, [1, 2, 3], 13, prefill=False, N=-7) == 0
        assert dev.lib.rama_q8_spec_end(dev.ctx) == 0
        from rama_amd._lib import rama_q8_spec_model_report
        assert dev.lib.rama_q8_spec_model_stats(dev.ctx, C.byref(rama_q8_spec_model_report())) == EINVAL      # no chain
        # ... and on a chain begun with rama_q8_spec_begin
        from rama_amd._lib import rama_q8_spec_plan
        plan = rama_q8_spec_plan(0.0, 0.9, 0.0, 4, -1, 2, 2, None, 0)
        assert dev.lib.rama_q8_spec_begin(dev.ctx, C.byref(p.m.ccfg), C.byref(p.m.weights), C.byref(other.state), arr([1]), 1, C.byref(plan)) == 0
        assert dev.lib.rama_q8_spec_model_stats(dev.ctx, C.byref(rama_q8_spec_model_report())) == EINVAL
        assert dev.lib.rama_q8_spec_model_stats(dev.ctx, None) == EINVAL
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        dev.lib.rama_q8_spec_end(dev.ctx)
        other.free(); dother.free(); long_e.free(); long_m.free()


@pytest.mark.parametrize("gone", ["draft state", "draft model", "target state"])
def test_a_freed_draft_model_or_state_refuses_steps(dev, golden_dir, gone):
    import rama_amd
    m, dm = open_model(dev, golden_dir, "ckpt_v2_q80_untied"), open_model(dev, golden_dir, "ckpt_v2_q80_tied")
    eng, twin, deng, bystander = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, dm), rama_amd.Q8Engine(dev, dm)
    ctx = [1, 9, 8, 7]
    try:
        want = twin.generate(ctx[1:], 3 + 8, 0.0)[3:]
        assert dev.lib.rama_set_graph_mode(dev.ctx, 1) == 0
        assert begin(dev, m, eng, dm, deng, ctx, 8, K=2) == 0
        assert steps(dev, 2) == 0
        bystander.forward(1, 0)
        bystander.free()                                           # a draft-model state outside the chain: nothing happens to it
        assert steps(dev, 1) == 0
        got = tokens(dev)
        assert 3 <= len(got) and got == want[:len(got)]
        if gone == "draft state":
            deng.free()
        elif gone == "draft model":
            dm.free(); dm = None                                   # (the draft run state is still there)
        else:
            eng.free()
        assert steps(dev, 1) == EINVAL and steps(dev, 0) == EINVAL
        assert tokens(dev) == got                                  # what was emitted stays readable
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        dev.lib.rama_q8_spec_end(dev.ctx)
        for e in (eng, twin, deng):
            if e is not None:
                e.free()
        m.free()
        if dm is not None:
            dm.free()


# ------------------------------------------------------------------ 4. the Python wrapper

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("name", ["untied<-tied", "synth15m<-near"])
def test_generate_spec_with_a_draft_engine(dev, pairs, name, graph):
    p = pairs(name)
    n_ctx, max_new = p.shape
    ctx = p.context(7)
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        for T, P, u in ((0.0, 0.9, 0.0), (1.0, 0.9, 0.35)):
            want = p.twin.generate(ctx[1:], n_ctx - 1 + max_new, T, P, u)[n_ctx - 1:]
            seen = []
            got = p.eng.generate_spec(ctx, max_new, T, P, u, n_draft=5, draft=p.deng, on_token=lambda i, t: seen.append((i, t)))
            assert got == want and seen == list(enumerate(want))
            assert p.eng.generate_spec(ctx, max_new, T, P, u, n_draft=5) == want       # ... and without a draft engine
            st = p.deng.spec_stats
            assert st is None                                      # the report is the target engine's
            st = p.eng.spec_stats
            assert "draft_cursor" not in st                        # (the run without a draft engine was the last)
            p.eng.generate_spec(ctx, max_new, T, P, u, n_draft=5, draft=p.deng)
            st = p.eng.spec_stats
            assert st["finished"] == 1 and st["n_out"] == max_new and st["graph_captures"] == graph
            assert st["draft_passes"] == st["drafts"] and st["draft_rows_fed"] == st["drafts"] + st["catch_up_rows"]
            assert n_ctx - 1 <= st["draft_cursor"] <= n_ctx + max_new
        assert steps(dev, 1) == EINVAL                             # the wrapper ends its chain
        other = pairs("gs8<-gs8")
        for kw in (dict(draft=p.eng), dict(draft=p.deng, hint=[1, 2]), dict(draft=other.deng), dict(draft=p.deng, n_draft=0)):
            with pytest.raises(ValueError):
                p.eng.generate_spec(ctx, max_new, **kw)
        with pytest.raises(ValueError):
            p.eng.generate_spec(ctx, p.dm.cfg.seq_len - n_ctx + 1, draft=p.deng)       # beyond the draft's seq_len (or the target's)
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
