"""The speculative chain on the GPU (rama_q8_spec_begin / _steps / _poll / _tokens / _stats, Q8Engine.generate_spec): whatever
n_draft, ngram, the hint and the graph mode, the tokens are bit for bit those of Q8Engine.generate on a twin engine and the cache
rows below the cursor are the twin's; the device's counters are those of spec_replay, the rule replayed on the host; stops, budgets,
the last rows of the context window, streaming, refusals and lifetimes.  Every comparison is exact: token lists and float bit
patterns.

The shapes: synth15m (group size 32, seq_len 256) runs 40 new tokens behind a 9-token context; the golden fixtures run to the END of
their context windows (n_context + max_new == seq_len: 16, 32 and 24 positions), so their last steps have room < n_draft and a row
at position seq_len would be a write out of bounds.  ckpt_v2_q80_gs8 takes the bytewise kernels, and its vocabulary (37) is no
multiple of 4."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_hip_q8 import same_bits

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -2
STORIES15M = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=256, shared_weight=True)
SHAPES = {"synth15m": (9, 40), "ckpt_v2_q80_tied": (3, 13), "ckpt_v2_q80_untied": (5, 27), "ckpt_v2_q80_gs8": (4, 20)}      # (n_context, max_new)
MODELS = list(SHAPES)
SENTINEL = np.float32(123.25)
N_SEEDS = 24


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


def open_model(dev, golden_dir, which):
    import rama_amd
    if which == "synth15m":
        return rama_amd.Q8Model.synth(dev, O.Config(**STORIES15M), 32, 11)
    return rama_amd.Q8Model.load(dev, golden_dir / f"{which}.bin")


class Bench:
    """a model, the chain's engine and the twin for the solo runs; the solo runs are computed once and kept"""

    def __init__(self, dev, golden_dir, which):
        import rama_amd
        self.dev, self.which = dev, which
        self.m = open_model(dev, golden_dir, which)
        self.cfg = self.m.cfg
        self.eng, self.twin = rama_amd.Q8Engine(dev, self.m), rama_amd.Q8Engine(dev, self.m)
        self._solo = {}

    def context(self, seed, n_ctx=None):
        n_ctx = SHAPES[self.which][0] if n_ctx is None else n_ctx
        rng = np.random.default_rng(seed)
        return [1] + [int(t) for t in rng.integers(0, self.cfg.vocab_size, n_ctx - 1)]

    def solo(self, ctx, max_new, T=0.0, P=0.9, u=0.0, cache=False):
        """the max_new tokens Q8Engine.generate gives behind ctx on the twin (not cut at any stop token) -- and, asked for, the
        twin's caches after that run"""
        key = (tuple(ctx), max_new, T, P, u)
        if key not in self._solo or (cache and self._solo[key][1] is None):
            toks = self.twin.generate(ctx[1:], len(ctx) - 1 + max_new, T, P, u)[len(ctx) - 1:]
            self._solo[key] = (toks, caches(self.twin) if cache else None)
        return self._solo[key] if cache else self._solo[key][0]

    def free(self):
        self.eng.free(); self.twin.free(); self.m.free()


@pytest.fixture(scope="module")
def benches(dev, golden_dir):
    made = {}

    def get(which):
        if which not in made:
            made[which] = Bench(dev, golden_dir, which)
        return made[which]
    yield get
    dev.lib.rama_q8_spec_end(dev.ctx)
    for b in made.values():
        b.free()


def arr(v):
    return (C.c_int32 * max(len(v), 1))(*v)


def caches(eng):
    c = eng.cfg
    n = c.n_layers * c.seq_len * c.dim
    return eng.buffer("key_cache", n).reshape(c.n_layers, c.seq_len, c.dim), eng.buffer("value_cache", n).reshape(c.n_layers, c.seq_len, c.dim)


def fill_behind(eng, first_row):
    """a sentinel in every cache row from first_row on"""
    c = eng.cfg
    for name in ("key_cache", "value_cache"):
        for l in range(c.n_layers):
            if first_row < c.seq_len:
                eng.set_buffer(name, np.full((c.seq_len - first_row) * c.dim, SENTINEL), (l * c.seq_len + first_row) * c.dim)


def begin(dev, m, eng, ctx, max_new, T=0.0, P=0.9, u=0.0, stop=-1, K=7, N=3, hint=None, prefill=True, n_hint=None, n_context=None,
          null=()):
    """the context's first n - 1 positions prefilled into eng, then rama_q8_spec_begin -> its return code"""
    from rama_amd._lib import rama_q8_spec_plan
    if prefill and len(ctx) > 1:
        eng.prefill(ctx[:-1], 0)
    h = arr(hint or [])
    plan = rama_q8_spec_plan(T, P, u, max_new, stop, K, N, None if "hint" in null or not hint else h, len(hint or []) if n_hint is None else n_hint)
    return dev.lib.rama_q8_spec_begin(None if "ctx" in null else dev.ctx, None if "cfg" in null else C.byref(m.ccfg),
                                      None if "w" in null else C.byref(m.weights), None if "state" in null else C.byref(eng.state),
                                      None if "context" in null else arr(ctx), len(ctx) if n_context is None else n_context,
                                      None if "plan" in null else C.byref(plan))


def steps(dev, n):
    return dev.lib.rama_q8_spec_steps(dev.ctx, n)


def tokens(dev, cap=256):
    out, n = (C.c_int32 * cap)(), C.c_int()
    assert dev.lib.rama_q8_spec_tokens(dev.ctx, out, cap, C.byref(n)) == 0
    return [int(out[i]) for i in range(n.value)]


def stats(dev):
    from rama_amd._lib import rama_q8_spec_report
    from rama_amd.q8 import spec_report
    r = rama_q8_spec_report()
    assert dev.lib.rama_q8_spec_stats(dev.ctx, C.byref(r)) == 0
    return spec_report(r)


def poll(dev, frm=0, cap=256):
    buf = (C.c_int32 * cap)()
    k, fin = C.c_int(), C.c_int(-7)
    assert dev.lib.rama_q8_spec_poll(dev.ctx, frm, buf, cap, C.byref(k), C.byref(fin)) == 0
    assert fin.value in (0, 1)
    return [int(buf[i]) for i in range(k.value)], bool(fin.value)


def corrupt(toks, V):
    """every 5th token replaced by a different one"""
    return [(t + 1) % V if i % 5 == 4 else t for i, t in enumerate(toks)]


def sums(traj):
    """what the device's counters must show after the steps of a replayed trajectory"""
    hist = [0] * 16
    for _, a, _ in traj:
        hist[a] += 1
    return dict(steps=len(traj), rows_fed=sum(n + 1 for n, _, _ in traj), drafts=sum(n for n, _, _ in traj),
                accepted=sum(a for _, a, _ in traj), emitted=sum(e for _, _, e in traj), accepted_hist=hist)


def assert_counters(st, traj, n_ctx, what=None):
    want = sums(traj)
    assert {k: st[k] for k in want} == want, what
    assert st["finished"] == 1 and st["n_out"] == want["emitted"] and st["cursor"] == n_ctx - 1 + want["emitted"], what


def run_and_check(b, ctx, max_new, want, traj, n_out=None, twin_cache=None, **plan):
    """the chain over b.eng for exactly the replayed number of steps: tokens, counters, and -- given the twin's caches -- the rows
    below the cursor against the twin's and the sentinel from row n_context - 1 + max_new on"""
    dev = b.dev
    n_out = len(want) if n_out is None else n_out
    if twin_cache is not None:
        fill_behind(b.eng, 0)
    assert begin(dev, b.m, b.eng, ctx, max_new, **plan) == 0
    assert steps(dev, len(traj)) == 0
    assert tokens(dev) == want[:n_out]
    st = stats(dev)
    assert_counters(st, traj, len(ctx), plan)
    if twin_cache is not None:
        valid, first_untouched = len(ctx) - 1 + n_out, len(ctx) - 1 + max_new
        for got, ref in zip(caches(b.eng), twin_cache):
            assert same_bits(got[:, :valid], ref[:, :valid]), plan
            assert (got[:, first_untouched:] == SENTINEL).all(), plan
    return st


# ------------------------------------------------------------------ 1. tokens and cache rows

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("ngram", [1, 3])
@pytest.mark.parametrize("n_draft", [0, 1, 7, 15])
@pytest.mark.parametrize("which", MODELS)
def test_tokens_and_cache_rows_equal_the_solo_run(dev, benches, which, n_draft, ngram, graph):
    from rama_amd.q8 import spec_replay
    b = benches(which)
    n_ctx, max_new = SHAPES[which]
    ctx = b.context(5)
    want, twin_cache = b.solo(ctx, max_new, cache=True)
    traj = spec_replay(want, ctx, None, n_draft, ngram, max_new, None)
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        st = run_and_check(b, ctx, max_new, want, traj, twin_cache=twin_cache, K=n_draft, N=ngram)
        assert st["graph_captures"] == graph                       # one captured graph serves the whole undisturbed run
        if n_draft == 0:
            assert st["steps"] == max_new and st["drafts"] == 0
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


# ------------------------------------------------------------------ 2. every accept outcome really occurs

def outcomes(traj, K):
    return {"full" if n == K and a == n else "partial" if 0 < a < n else "none" if n == 0 else "zero" if a == 0 else "other"
            for n, a, _ in traj}


def find_covering_case(b, K, N, T=0.0, P=0.9):
    """the first seed whose replay -- over a hint with every 5th token wrong -- has a step of each kind: a = n_d = n_draft,
    0 < a < n_d, a = 0 < n_d, n_d = 0.  A condition on the input, checked before the chain runs."""
    from rama_amd.q8 import spec_replay
    n_ctx, max_new = SHAPES[b.which]
    for seed in range(N_SEEDS):
        ctx, u = b.context(seed), 0.25 + 0.05 * (seed % 10)
        want = b.solo(ctx, max_new, T, P, u)
        hint = corrupt(want, b.cfg.vocab_size)
        traj = spec_replay(want, ctx, hint, K, N, max_new, None)
        if {"full", "partial", "zero", "none"} <= outcomes(traj, K):
            return ctx, u, want, hint, traj
    raise AssertionError(f"{b.which}: no seed below {N_SEEDS} whose replay shows every accept outcome")


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", ["ckpt_v2_q80_untied", "ckpt_v2_q80_gs8"])
def test_every_accept_outcome_occurs_and_the_counters_are_the_replays(dev, benches, which, graph):
    b = benches(which)
    K, N = 3, 2
    ctx, u, want, hint, traj = find_covering_case(b, K, N)
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        run_and_check(b, ctx, SHAPES[which][1], want, traj, K=K, N=N, hint=hint)
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


@pytest.mark.parametrize("which,T", [("synth15m", 1.0), ("ckpt_v2_q80_untied", 0.0)])
def test_a_right_hint_takes_sixteen_tokens_a_step(dev, benches, which, T):
    """hint = the solo run itself, n_draft 15.  synth15m's greedy run repeats one token, whose latest occurrence in the hint is the
    hint's end -- nothing follows it --, so its case samples: 40 different tokens, 1 step without a draft + ceil(39 / 16)."""
    from rama_amd.q8 import spec_replay
    b = benches(which)
    n_ctx, max_new = SHAPES[which]
    for seed in range(N_SEEDS):
        ctx, u = b.context(seed), 0.25 + 0.05 * (seed % 10)
        want = b.solo(ctx, max_new, T, 0.9, u)
        traj = spec_replay(want, ctx, want, 15, 3, max_new, None)
        if len(traj) <= 2 + (max_new + 15) // 16:
            break
    else:
        raise AssertionError(f"{which}: no seed whose solo run the hint lookup follows")
    assert len(traj) < max_new
    if which == "synth15m":
        assert len(traj) == 1 + (max_new - 1 + 15) // 16
    st = run_and_check(b, ctx, max_new, want, traj, T=T, u=u, K=15, N=3, hint=want)
    assert st["steps"] == len(traj) < max_new


# ------------------------------------------------------------------ 3. sampled

@pytest.mark.parametrize("T,P", [(1.0, 0.9), (0.7, 1.0)])
@pytest.mark.parametrize("which", MODELS)
def test_sampled_equals_the_solo_sampled_run(dev, benches, which, T, P):
    from rama_amd.q8 import spec_replay
    b = benches(which)
    n_ctx, max_new = SHAPES[which]
    K, N = (3, 2) if which != "synth15m" else (7, 3)
    if which == "synth15m":
        ctx, u = b.context(3), 0.4
        want = b.solo(ctx, max_new, T, P, u)
        hint = corrupt(want, b.cfg.vocab_size)
        traj = spec_replay(want, ctx, hint, K, N, max_new, None)
        assert {"partial", "none"} <= outcomes(traj, K)
    else:
        ctx, u, want, hint, traj = find_covering_case(b, K, N, T, P)
    _, twin_cache = b.solo(ctx, max_new, T, P, u, cache=True)
    for graph in (0, 1):
        assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
        try:
            run_and_check(b, ctx, max_new, want, traj, twin_cache=twin_cache, T=T, P=P, u=u, K=K, N=N, hint=hint)
        finally:
            dev.lib.rama_set_graph_mode(dev.ctx, 0)


def test_vocabulary_above_32768(dev):
    """a sampled plan is refused with RAMA_EUNSUP; the greedy chain runs"""
    import rama_amd
    from rama_amd.q8 import spec_replay
    cfg = dict(dim=64, hidden_dim=192, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=32772, seq_len=32, shared_weight=True)
    m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), 32, 3)
    eng, twin = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, m)
    try:
        ctx = [1, 32771, 7]
        assert begin(dev, m, eng, ctx, 6, T=1.0, u=0.5) == EUNSUP
        assert begin(dev, m, eng, ctx, 6, T=0.5, P=1.0, u=0.5, K=0) == EUNSUP
        want = twin.generate(ctx[1:], 2 + 6, 0.0)[2:]
        assert begin(dev, m, eng, ctx, 6, hint=want, K=4) == 0
        traj = spec_replay(want, ctx, want, 4, 3, 6, None)
        assert steps(dev, len(traj)) == 0
        assert tokens(dev) == want
        assert_counters(stats(dev), traj, 3)
    finally:
        dev.lib.rama_q8_spec_end(dev.ctx)
        eng.free(); twin.free(); m.free()


# ------------------------------------------------------------------ 4. ends

def first_at(want, idx):
    """the token at idx occurs there first: as a stop token it ends the run exactly there"""
    return want[idx] not in want[:idx]


def find_stop_cases(b, K, N):
    """-> {kind: (ctx, want, hint, stop token, index it ends at)} for a stop token that is the last accepted token of a
    full-accept step and one that is the first rejected pick, over hints with every 5th token wrong"""
    from rama_amd.q8 import spec_replay
    n_ctx, max_new = SHAPES[b.which]
    found = {}
    for seed in range(N_SEEDS):
        ctx = b.context(seed)
        want = b.solo(ctx, max_new)
        hint = corrupt(want, b.cfg.vocab_size)
        e = 0
        for n_d, a, emit in spec_replay(want, ctx, hint, K, N, max_new, None):
            if n_d == K and a == n_d and first_at(want, e + a - 1):
                found.setdefault("last accepted", (ctx, want, hint, want[e + a - 1], e + a - 1))
            if 0 < n_d and a < n_d and emit == a + 1 and first_at(want, e + a):
                found.setdefault("first rejected", (ctx, want, hint, want[e + a], e + a))
            e += emit
        if len(found) == 2:
            return found
    raise AssertionError(f"{b.which}: no seed below {N_SEEDS} with both stop cases: {list(found)}")


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", ["ckpt_v2_q80_untied", "ckpt_v2_q80_gs8"])
def test_stop_tokens(dev, benches, which, graph):
    from rama_amd.q8 import spec_replay
    b = benches(which)
    n_ctx, max_new = SHAPES[which]
    K, N = 3, 2
    cases = find_stop_cases(b, K, N)
    ctx0 = b.context(0)
    want0 = b.solo(ctx0, max_new)
    cases["first output"] = (ctx0, want0, corrupt(want0, b.cfg.vocab_size), want0[0], 0)
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        for kind, (ctx, want, hint, stop, idx) in cases.items():
            traj = spec_replay(want, ctx, hint, K, N, max_new, stop)
            assert sum(e for _, _, e in traj) == idx + 1, kind
            _, twin_cache = b.solo(ctx, max_new, cache=True)
            st = run_and_check(b, ctx, max_new, want, traj, n_out=idx + 1, twin_cache=twin_cache, K=K, N=N, hint=hint, stop=stop)
            assert st["n_out"] == idx + 1 < max_new, kind
            # steps after the finish: all-idle passes that change no token, no counter but `steps`, and no cache bit
            before = caches(b.eng)
            assert steps(dev, 3) == 0
            after = stats(dev)
            assert after == dict(st, steps=st["steps"] + 3), kind
            assert tokens(dev) == want[:idx + 1] and poll(dev) == (want[:idx + 1], True), kind
            for x, y in zip(caches(b.eng), before):
                assert same_bits(x, y), kind
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


@pytest.mark.parametrize("which", ["synth15m", "ckpt_v2_q80_untied"])
def test_budget_ends_inside_an_accepted_run(dev, benches, which):
    """the hint is right, so the last step would accept n_draft tokens: remaining - 1 bounds its drafts, every one of them is accepted
    and the pick behind them is the max_new-th token"""
    from rama_amd.q8 import spec_replay
    b = benches(which)
    n_ctx, max_new = SHAPES[which]
    T = 1.0 if which == "synth15m" else 0.0                        # (synth15m's greedy run repeats one token: see above)
    K = 7
    for seed in range(N_SEEDS):
        ctx, u = b.context(seed), 0.25 + 0.05 * (seed % 10)
        want = b.solo(ctx, max_new, T, 0.9, u)
        traj = spec_replay(want, ctx, want, K, 3, max_new, None)
        n_d, a, emit = traj[-1]
        before = max_new - sum(e for _, _, e in traj[:-1])          # `remaining` when the last step starts
        if 0 < n_d < K and n_d == before - 1 and a == n_d and emit == before:
            break
    else:
        raise AssertionError(f"{which}: no seed whose last step is cut by the budget")
    _, twin_cache = b.solo(ctx, max_new, T, 0.9, u, cache=True)
    run_and_check(b, ctx, max_new, want, traj, twin_cache=twin_cache, T=T, u=u, K=K, N=3, hint=want)


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", MODELS)
def test_bos_alone_and_a_single_token(dev, benches, which, graph):
    from rama_amd.q8 import spec_replay
    b = benches(which)
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        # n_context == 1: BOS alone, nothing prefilled; to the end of the context window on the fixtures
        max_new = min(b.cfg.seq_len - 1, 30)
        want, twin_cache = b.solo([1], max_new, cache=True)
        traj = spec_replay(want, [1], None, 7, 2, max_new, None)
        run_and_check(b, [1], max_new, want, traj, twin_cache=twin_cache, K=7, N=2)
        # max_new == 1: one step, no draft whatever the hint says
        ctx = b.context(2)
        want, twin_cache = b.solo(ctx, 1, cache=True)
        st = run_and_check(b, ctx, 1, want, [(0, 0, 1)], twin_cache=twin_cache, K=15, N=1, hint=ctx + want + [3, 4, 5])
        assert st["rows_fed"] == 1
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


# ------------------------------------------------------------------ 5. streaming

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", ["synth15m", "ckpt_v2_q80_untied"])
def test_poll_sees_a_growing_prefix(dev, benches, which, graph):
    b = benches(which)
    n_ctx, max_new = SHAPES[which]
    ctx = b.context(5)
    want = b.solo(ctx, max_new)
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        assert begin(dev, b.m, b.eng, ctx, max_new, K=3, N=2) == 0
        assert poll(dev) == ([], False)
        seen = []
        for _ in range((max_new + 1) // 2):                        # max_new steps at the least: every step before the finish emits a token
            assert steps(dev, 2) == 0                              # (asynchronous: the poll below may see any prefix of them)
            got, fin = poll(dev, len(seen))
            seen += got
            assert seen == want[:len(seen)]
            if fin:                                                # finished is 1 only with the last token visible
                assert seen == want
                break
        assert dev.lib.rama_sync(dev.ctx) == 0
        got, fin = poll(dev, len(seen))
        seen += got
        assert fin
        assert seen == want and poll(dev, 3, 4) == (want[3:7], True) and poll(dev, max_new) == ([], True)
        assert tokens(dev) == want
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


# ------------------------------------------------------------------ 6. lifetimes and refusals

def test_refusals_leave_a_running_chain_intact(dev, benches, golden_dir):
    import rama_amd
    b = benches("ckpt_v2_q80_untied")
    n_ctx, max_new = SHAPES[b.which]
    ctx = b.context(5)
    want = b.solo(ctx, max_new)
    V, S = b.cfg.vocab_size, b.cfg.seq_len
    other = rama_amd.Q8Engine(dev, b.m)
    long_m = rama_amd.Q8Model.synth(dev, O.Config(dim=64, hidden_dim=192, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=64, seq_len=8192,
                                                  shared_weight=True), 32, 9)
    long_e = rama_amd.Q8Engine(dev, long_m)
    assert dev.lib.rama_set_graph_mode(dev.ctx, 1) == 0
    try:
        assert begin(dev, b.m, b.eng, ctx, max_new, K=0) == 0
        assert steps(dev, 4) == 0
        bad = [dict(null=("ctx",)), dict(null=("cfg",)), dict(null=("w",)), dict(null=("state",)), dict(null=("context",)), dict(null=("plan",)),
               dict(T=-1.0), dict(T=float("nan")), dict(P=1.5), dict(P=-0.1), dict(u=1.0), dict(u=-0.5), dict(stop=V), dict(stop=-2),
               dict(K=-1), dict(K=16), dict(N=0), dict(N=5), dict(hint=[3, V]), dict(hint=[-1]), dict(n_hint=-1),
               dict(hint=[1, 2], null=("hint",), n_hint=2), dict(n_context=0), dict(max_new=0), dict(max_new=S - 2)]
        for kw in bad:
            kw = dict(dict(max_new=4), **kw)
            assert begin(dev, b.m, other, [1, 2, 3], prefill=False, **kw) == EINVAL, kw
        assert begin(dev, b.m, other, [1, V, 3], 4, prefill=False) == EINVAL
        assert begin(dev, b.m, other, [1, 2, 3], S - 3, prefill=False, n_context=S) == EINVAL
        assert dev.lib.rama_q8_batch_shape_ok(C.byref(long_m.ccfg)) == 0
        assert begin(dev, long_m, long_e, [1, 2, 3], 4, prefill=False) == EUNSUP
        assert steps(dev, -1) == EINVAL
        assert steps(dev, max_new - 4) == 0
        assert tokens(dev) == want
        st = stats(dev)
        assert st["steps"] == max_new and st["graph_captures"] == 1 and st["finished"] == 1
        assert begin(dev, b.m, other, [1, 2, 3], S - 3, prefill=False) == 0          # n_context + max_new == seq_len is taken
        assert dev.lib.rama_q8_spec_end(dev.ctx) == 0 and dev.lib.rama_q8_spec_end(dev.ctx) == 0
        assert steps(dev, 1) == EINVAL and dev.lib.rama_q8_spec_stats(dev.ctx, None) == EINVAL
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        dev.lib.rama_q8_spec_end(dev.ctx)
        other.free(); long_e.free(); long_m.free()


def test_freed_state_or_model_refuses_steps(dev, golden_dir):
    import rama_amd
    m = open_model(dev, golden_dir, "ckpt_v2_q80_untied")
    eng, twin, bystander = (rama_amd.Q8Engine(dev, m) for _ in range(3))
    ctx = [1, 9, 8, 7]
    try:
        want = twin.generate(ctx[1:], 3 + 8, 0.0)[3:]
        assert dev.lib.rama_set_graph_mode(dev.ctx, 1) == 0
        assert begin(dev, m, eng, ctx, 8, K=0) == 0
        assert steps(dev, 3) == 0
        bystander.forward(1, 0)
        bystander.free()                                           # a state outside the chain: nothing happens to it
        assert steps(dev, 2) == 0
        assert tokens(dev) == want[:5]
        eng.free()                                                 # the chain's own
        assert steps(dev, 1) == EINVAL and steps(dev, 0) == EINVAL
        eng = rama_amd.Q8Engine(dev, m)
        assert begin(dev, m, eng, ctx, 8, K=2, N=1) == 0           # a new chain runs; then the model goes
        assert steps(dev, 2) == 0
        got = tokens(dev)
        assert 2 <= len(got) and got == want[:len(got)]
        twin.free()
        m.free()                                                   # (the chain's run state is still there)
        assert steps(dev, 1) == EINVAL
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        dev.lib.rama_q8_spec_end(dev.ctx)
        for e in (eng, twin):
            e.free()
        m.free()


def test_other_calls_between_steps_and_a_scratch_that_grows(golden_dir):
    """a context of its own, so that the second model is the largest it has seen: its prefill regrows the batch scratch under the
    running chain, whose graph is captured again; a serving chain and a chained batch live next to it undisturbed"""
    import rama_amd
    from rama_amd.q8 import Q8Server, decode_batch, decode_batch_chained, spec_replay
    d = rama_amd.Hip(0)
    small = open_model(d, golden_dir, "ckpt_v2_q80_untied")
    big = open_model(d, golden_dir, "synth15m")
    eng, twin = rama_amd.Q8Engine(d, small), rama_amd.Q8Engine(d, small)
    extra = [rama_amd.Q8Engine(d, small) for _ in range(3)]
    chained = [rama_amd.Q8Engine(d, small) for _ in range(2)]
    big_e = rama_amd.Q8Engine(d, big)
    srv = None
    rng = np.random.default_rng(4)
    try:
        assert d.lib.rama_set_graph_mode(d.ctx, 1) == 0
        ctx = [1] + [int(t) for t in rng.integers(0, small.cfg.vocab_size, 4)]
        max_new = 27
        want = twin.generate(ctx[1:], 4 + max_new, 1.0, 0.9, 0.3)[4:]
        twin_cache = caches(twin)
        hint = corrupt(want, small.cfg.vocab_size)
        traj = spec_replay(want, ctx, hint, 7, 3, max_new, None)
        assert len(traj) >= 6
        solo_srv = twin.generate([5, 6], 2 + 6, 0.0)[2:]
        solo_chain = [twin.generate([], 5, 0.0), twin.generate([], 5, 1.0, 0.9, 0.6)]
        assert begin(d, small, eng, ctx, max_new, T=1.0, u=0.3, hint=hint) == 0
        assert steps(d, 2) == 0
        extra[0].prefill([1, 4, 5, 6, 7, 8], 0)                    # the same scratch, the same stream
        decode_batch(extra[1:], [3, 4], [0, 0])
        extra[0].forward(7, 6)
        assert steps(d, 1) == 0
        assert stats(d)["graph_captures"] == 1
        big_e.prefill([1] + [int(t) for t in rng.integers(0, big.cfg.vocab_size, 8)], 0)      # the batch scratch grows and moves
        assert steps(d, 1) == 0
        assert stats(d)["graph_captures"] == 2
        # a serving chain and a chained batch on the same context, interleaved with the chain's steps
        srv = Q8Server(small, 2, max_new_cap=8)
        h = srv.submit([1, 5, 6], 6)
        srv.step(2)
        assert steps(d, 1) == 0
        got_chain = decode_batch_chained(chained, [1, 1], [0, 0], 5, temperature=[0.0, 1.0], u=[0.0, 0.6])
        assert steps(d, len(traj) - 5) == 0
        srv.run()
        assert srv.result(h) == solo_srv and got_chain == solo_chain
        assert tokens(d) == want
        assert_counters(stats(d), traj, len(ctx))
        for got, ref in zip(caches(eng), twin_cache):
            assert same_bits(got[:, :4 + max_new], ref[:, :4 + max_new])
    finally:
        d.lib.rama_set_graph_mode(d.ctx, 0)
        if srv is not None:
            srv.close()
        d.lib.rama_q8_spec_end(d.ctx)
        for e in [eng, twin, big_e] + extra + chained:
            e.free()
        small.free(); big.free()
        d.close()


# ------------------------------------------------------------------ 7. the Python wrapper

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", ["ckpt_v2_q80_tied", "ckpt_v2_q80_untied"])
def test_generate_spec_equals_generate(dev, benches, which, graph):
    b = benches(which)
    n_ctx, max_new = SHAPES[which]
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        for T, P, u, stop_at in ((0.0, 0.9, 0.0, None), (1.0, 0.9, 0.35, None), (0.0, 0.9, 0.0, 4)):
            ctx = b.context(7)
            want = b.solo(ctx, max_new, T, P, u)
            stop = None
            if stop_at is not None:
                stop = want[stop_at]
                want = want[:want.index(stop) + 1]
            seen = []
            got = b.eng.generate_spec(ctx, max_new, T, P, u, stop_token=stop, n_draft=5, ngram=2, hint=corrupt(want, b.cfg.vocab_size),
                                      on_token=lambda i, t: seen.append((i, t)))
            assert got == want and seen == list(enumerate(want))
            st = b.eng.spec_stats
            assert st["finished"] == 1 and st["n_out"] == st["emitted"] == len(want) and st["graph_captures"] == graph
            assert st["steps"] >= sum(st["accepted_hist"]) and st["rows_fed"] == st["drafts"] + sum(st["accepted_hist"])
        assert steps(dev, 1) == EINVAL                             # the wrapper ends its chain
        with pytest.raises(ValueError):
            b.eng.generate_spec([1, 2], b.cfg.seq_len)
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


def test_generate_spec_without_drafts_past_64_tokens(dev):
    """n_draft = 0, 70 tokens: the wrapper looks at the ring every SPEC_BLOCK steps, so no look finds a full poll of 64 -- what
    this shows is the drain going on from a count beyond 64"""
    import rama_amd
    cfg = O.Config(dim=64, hidden_dim=192, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=64, seq_len=128, shared_weight=True)
    m = rama_amd.Q8Model.synth(dev, cfg, 64, 3)
    eng, twin = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, m)
    try:
        ctx, new = [1, 7], 70
        want = twin.generate(ctx[1:], 1 + new)[1:]
        seen = []
        got = eng.generate_spec(ctx, new, n_draft=0, on_token=lambda i, t: seen.append((i, t)))
        assert len(want) == new and got == want and seen == list(enumerate(want))
        assert eng.spec_stats["steps"] == new and eng.spec_stats["finished"] == 1
    finally:
        eng.free(); twin.free()
        m.free()
