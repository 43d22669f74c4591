"""The chained Q8 batch on the GPU (rama_q8_decode_batch_begin / _steps / _tokens / _stream_poll): every sequence's tokens and
cache rows are bit for bit those of rama_q8_generate / rama_q8_forward run on it alone -- greedy, sampled, forced, with step
budgets and stop tokens, streamed, in eager and in graph mode -- and the chain survives what may move or free what its
captured step holds.  Every comparison is exact: token lists and float bit patterns."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_hip_q8 import same_bits

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -2
STORIES15M = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=256, shared_weight=True)
MODELS = ["ckpt_v2_q80_tied", "ckpt_v2_q80_untied", "synth15m"]
SENTINEL = np.float32(123.25)


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


def arr(v):
    return (C.c_int32 * max(len(v), 1))(*v)


# ------------------------------------------------------------------ a sequence, its solo run, the raw entry points

class Seq:
    """one sequence of a chain: a context of `pos` tokens (BOS first), the token fed at `pos`, and its plan"""

    def __init__(self, rng, cfg, pos, T=0.0, topp=0.9, u=0.0, prompt=(), max_new=0, stop=-1):
        self.pos, self.T, self.topp, self.u, self.prompt, self.max_new, self.stop = pos, T, topp, u, list(prompt), max_new, stop
        assert pos == 0 or not self.prompt                    # (forced lists count absolute positions: only used from position 0 here)
        self.ctx = [1] + [int(t) for t in rng.integers(0, cfg.vocab_size, max(pos - 1, 0))] if pos else []
        self.token = int(rng.integers(0, cfg.vocab_size)) if pos else 1
        self.eng = self.twin = None

    def prepare(self, dev, m):
        """the chain's engine with its context prefilled; a twin for the solo run"""
        import rama_amd
        self.eng, self.twin = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, m)
        if self.pos:
            self.eng.prefill(self.ctx, 0)

    def solo(self, n):
        """the n tokens Q8Engine.generate gives this sequence alone from the same state (no budget, no stop)"""
        if self.pos == 0:
            return self.twin.generate(self.prompt, n, self.T, self.topp, self.u)
        return self.twin.generate(self.ctx[1:] + [self.token], self.pos + n, self.T, self.topp, self.u)[self.pos:]

    def record(self, keep):
        from rama_amd._lib import rama_q8_seq_plan
        f = arr(self.prompt)
        keep.append(f)
        return rama_q8_seq_plan(self.T, self.topp, self.u, f, len(self.prompt), self.max_new, self.stop)

    def free(self):
        for e in (self.eng, self.twin):
            if e is not None:
                e.free()


def begin(dev, m, seqs, max_steps, plan=True, tokens=None, positions=None, n_seq=None, records=None):
    from rama_amd._lib import rama_q8_seq_plan, rama_run_state
    n = len(seqs)
    keep = []
    states = (rama_run_state * max(n, 1))(*[s.eng.state for s in seqs])
    per = None
    if plan:
        recs = records if records is not None else [s.record(keep) for s in seqs]
        per = (rama_q8_seq_plan * max(n, 1))(*recs)
    return dev.lib.rama_q8_decode_batch_begin(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), states,
                                              arr(tokens if tokens is not None else [s.token for s in seqs]),
                                              arr(positions if positions is not None else [s.pos for s in seqs]),
                                              n if n_seq is None else n_seq, max_steps, per)


def steps(dev, n):
    return dev.lib.rama_q8_decode_batch_steps(dev.ctx, n)


def tokens(dev, n_seq, max_per):
    out = (C.c_int32 * (n_seq * max_per))()
    cnt = (C.c_int32 * n_seq)()
    assert dev.lib.rama_q8_decode_batch_tokens(dev.ctx, out, max_per, cnt) == 0
    return [[int(out[s * max_per + j]) for j in range(cnt[s])] for s in range(n_seq)]


def poll(dev, seq, frm=0, cap=256):
    buf = (C.c_int32 * cap)()
    k, fin = C.c_int(), C.c_int(-7)
    assert dev.lib.rama_q8_decode_batch_stream_poll(dev.ctx, seq, frm, buf, cap, C.byref(k), C.byref(fin)) == 0
    assert fin.value in (0, 1)
    return [int(buf[i]) for i in range(k.value)], bool(fin.value)


def cache(eng):
    c = eng.cfg
    n = c.n_layers * c.seq_len * c.dim
    return eng.buffer("key_cache", n).reshape(c.n_layers, c.seq_len, c.dim), eng.buffer("value_cache", n).reshape(c.n_layers, c.seq_len, c.dim)


def check_cache_rows(s, n_rows, what):
    """rows [0, n_rows) of every layer: the chain's engine against the solo run's"""
    for got, want in zip(cache(s.eng), cache(s.twin)):
        assert same_bits(got[:, :n_rows], want[:, :n_rows]), what


def fill_behind(eng, first_row):
    """a sentinel in every cache row from first_row on"""
    c = eng.cfg
    for name in ("key_cache", "value_cache"):
        for l in range(c.n_layers):
            if first_row < c.seq_len:
                eng.set_buffer(name, np.full((c.seq_len - first_row) * c.dim, SENTINEL), (l * c.seq_len + first_row) * c.dim)


def holds_sentinel(eng, first_row):
    return all((kv[:, first_row:] == SENTINEL).all() for kv in cache(eng))


def expected(solo, n_forced, max_new, stop, n_steps):
    """what a sequence with this solo token list produces in n_steps steps: cut at its budget and at its first sampled stop token"""
    out = []
    for i, t in enumerate(solo[:min(n_steps, max_new or n_steps)]):
        out.append(t)
        if i >= n_forced and t == stop:
            break
    return out


# ------------------------------------------------------------------ 1. greedy

@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_greedy_equals_solo_generate(dev, golden_dir, which, graph):
    m = open_model(dev, golden_dir, which)
    c = m.cfg
    n_steps = 6
    try:
        for n_seq in (1, 2, 5, 33):
            rng = np.random.default_rng(100 * n_seq + graph)
            poss = [int(p) for p in rng.integers(0, c.seq_len - n_steps + 1, n_seq)]
            poss[0] = c.seq_len - n_steps                     # one sequence ends on the last position of the context
            if n_seq > 1:
                poss[1] = 0
            seqs = [Seq(rng, c, p) for p in poss]
            try:
                for s in seqs:
                    s.prepare(dev, m)
                    s.eng.set_buffer("logits", np.full(c.vocab_size, np.float32(-9.0)))
                seqs[0].eng.set_graph_mode(graph)
                # NULL plan, the steps split over three calls
                assert begin(dev, m, seqs, n_steps, plan=False) == 0
                for k in (1, 0, 3, n_steps - 4):
                    assert steps(dev, k) == 0
                got = tokens(dev, n_seq, n_steps)
                want = [s.solo(n_steps) for s in seqs]
                assert got == want, (which, graph, n_seq)
                for i, s in enumerate(seqs):
                    check_cache_rows(s, s.pos + n_steps, (which, graph, n_seq, i))
                    assert (s.eng.logits() == np.float32(-9.0)).all()      # the logits stay in the scratch
                # the same through the wrapper, as one call, over the same engines from a fresh start (the rows are rewritten)
                from rama_amd.q8 import decode_batch_chained
                again = decode_batch_chained([s.eng for s in seqs], [s.token for s in seqs], poss, n_steps)
                assert again == want, (which, graph, n_seq)
            finally:
                seqs[0].eng.set_graph_mode(0) if seqs[0].eng else None
                for s in seqs:
                    s.free()
    finally:
        m.free()


# ------------------------------------------------------------------ 2. sampled

def sampled_rows(rng, cfg, n_steps):
    V = cfg.vocab_size
    p3 = [int(t) for t in rng.integers(0, V, 3)]
    plong = [int(t) for t in rng.integers(0, V, n_steps + 2)]
    return [Seq(rng, cfg, 0), Seq(rng, cfg, 0, T=1.0, topp=0.9, u=0.1), Seq(rng, cfg, 0, T=0.7, topp=0.5, u=0.6),
            Seq(rng, cfg, 0, T=1.0, topp=0.9, u=0.9, prompt=p3), Seq(rng, cfg, 0, T=0.0, prompt=[5]),
            Seq(rng, cfg, 0, T=1.0, topp=0.9, u=0.33, prompt=plong), Seq(rng, cfg, 3, T=1.0, topp=0.9, u=0.45)]


@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_sampled_rows_equal_solo_generate(dev, golden_dir, which, graph):
    m = open_model(dev, golden_dir, which)
    n_steps = 8
    seqs = sampled_rows(np.random.default_rng(7 + graph), m.cfg, n_steps)
    try:
        for s in seqs:
            s.prepare(dev, m)
        seqs[0].eng.set_graph_mode(graph)
        assert begin(dev, m, seqs, n_steps) == 0
        assert steps(dev, 3) == 0 and steps(dev, n_steps - 3) == 0
        got = tokens(dev, len(seqs), n_steps)
        want = [s.solo(n_steps) for s in seqs]
        assert got == want, (which, graph)
        assert want[5] == seqs[5].prompt[:n_steps] and want[3][:3] == seqs[3].prompt
        for i, s in enumerate(seqs):
            check_cache_rows(s, s.pos + n_steps, (which, graph, i))
    finally:
        seqs[0].eng.set_graph_mode(0)
        for s in seqs:
            s.free()
        m.free()


# ------------------------------------------------------------------ 3. + 4. stops, budgets, streaming

def stop_index(t, n_forced):
    """the smallest index >= n_forced + 2 whose token does not occur in t[n_forced:k]; n_forced if there is none"""
    for k in range(n_forced + 2, len(t)):
        if t[k] not in t[n_forced:k]:
            return k
    return n_forced


def stop_case(dev, m, n_steps, mode):
    """seven sequences: [0] stops on a token of its own solo list, [1] has a budget of 3, the rest run on; unless mode is "argmax"
    (no forced row: the steps end in argmax_batch_kernel), [2] carries a stop token that occurs only in its forced prompt and [3]
    stops on a sampled token behind a forced prompt.  mode "sampled": T 1 / top-p 0.9 rows.  -> (seqs, solo lists, expected)"""
    c = m.cfg
    V = c.vocab_size
    rng = np.random.default_rng(31 + len(mode))
    kw = dict(T=1.0, topp=0.9) if mode == "sampled" else {}
    forced = mode != "argmax"
    seqs = [Seq(rng, c, 2, u=0.15, **kw), Seq(rng, c, 0, u=0.25, **kw), None, None, Seq(rng, c, 4, u=0.55, **kw), Seq(rng, c, 0),
            Seq(rng, c, 1, u=0.75, **kw)]
    seqs[3] = Seq(rng, c, 0, u=0.45, prompt=[int(t) for t in rng.integers(0, V, 2)] if forced else (), **kw)
    for i, s in enumerate(seqs):
        if i != 2:
            s.prepare(dev, m)
    for _ in range(8):            # a prompt with a token that the free run behind it does not produce
        seqs[2] = Seq(rng, c, 0, u=0.35, prompt=[int(t) for t in rng.integers(0, V, 3)] if forced else (), **kw)
        seqs[2].prepare(dev, m)
        only_forced = [t for t in seqs[2].prompt if t not in seqs[2].solo(n_steps)[3:]]
        if only_forced or not forced:
            break
        seqs[2].free()
    solo = [s.solo(n_steps) for s in seqs]
    k = stop_index(solo[0], 0)
    seqs[0].stop = solo[0][k]
    seqs[1].max_new = 3
    nf3 = len(seqs[3].prompt)
    seqs[3].stop = solo[3][stop_index(solo[3], nf3)]
    if forced:
        assert only_forced, "no prompt found whose free run avoids one of its tokens"
        seqs[2].stop = only_forced[0]
    want = [expected(solo[i], len(s.prompt), s.max_new, s.stop, n_steps) for i, s in enumerate(seqs)]
    assert want[0] == solo[0][:k + 1] and len(want[1]) == 3 and want[4:] == solo[4:]
    assert want[3] == solo[3][:stop_index(solo[3], nf3) + 1]
    assert not forced or want[2] == solo[2]
    return seqs, solo, want


@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("mode", ["argmax", "greedy", "sampled"])
def test_stops_and_budgets(dev, golden_dir, which, graph, mode):
    m = open_model(dev, golden_dir, which)
    n_steps = 10
    seqs = []
    try:
        seqs, solo, want = stop_case(dev, m, n_steps, mode)
        ends = [s.pos + len(w) for s, w in zip(seqs, want)]      # the first row a sequence never passes
        for s, e in zip(seqs, ends):
            fill_behind(s.eng, e)
        seqs[0].eng.set_graph_mode(graph)
        assert begin(dev, m, seqs, n_steps) == 0
        n1 = 4
        assert steps(dev, n1) == 0
        part = tokens(dev, len(seqs), n_steps)
        assert part == [expected(solo[i], len(s.prompt), s.max_new, s.stop, n1) for i, s in enumerate(seqs)]
        # the finished words: exactly the stopped and the exhausted sequences
        for i, s in enumerate(seqs):
            seen, fin = poll(dev, i)
            assert seen == part[i], i
            assert fin == (len(want[i]) <= n1), (i, fin)
            assert poll(dev, i, 1)[0] == part[i][1:]
        assert steps(dev, n_steps - n1) == 0
        got = tokens(dev, len(seqs), n_steps)
        assert got == want, (which, graph, mode)
        assert [len(g) for g in got] == [len(w) for w in want]
        short = tokens(dev, len(seqs), 2)                          # max_per_seq bounds what is copied and reported
        assert short == [w[:2] for w in want]
        for i, s in enumerate(seqs):
            seen, fin = poll(dev, i)
            assert seen == want[i] and fin, i                      # every budget is used: all finished
            check_cache_rows(s, ends[i], (which, graph, mode, i))
            assert holds_sentinel(s.eng, ends[i]), (which, graph, mode, i)
        assert steps(dev, 1) == EINVAL
    finally:
        if seqs:
            seqs[0].eng.set_graph_mode(0)
        for s in seqs:
            s.free()
        m.free()


@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_streaming_through_the_wrapper(dev, golden_dir, which, graph):
    from rama_amd.q8 import decode_batch_chained
    m = open_model(dev, golden_dir, which)
    n_steps = 10
    seqs = []
    try:
        seqs, solo, want = stop_case(dev, m, n_steps, "sampled")
        seqs[0].eng.set_graph_mode(graph)
        seen = [[] for _ in seqs]

        def on_token(s, i, t):
            assert i == len(seen[s])
            seen[s].append(t)

        got = decode_batch_chained([s.eng for s in seqs], [s.token for s in seqs], [s.pos for s in seqs], n_steps,
                                   temperature=[s.T for s in seqs], topp=[s.topp for s in seqs], u=[s.u for s in seqs],
                                   prompts=[s.prompt for s in seqs], max_new=[s.max_new or None for s in seqs],
                                   stop_tokens=[s.stop if s.stop >= 0 else None for s in seqs], on_token=on_token)
        assert got == want and seen == want, (which, graph)
        assert all(poll(dev, i)[1] for i in range(len(seqs)))
    finally:
        if seqs:
            seqs[0].eng.set_graph_mode(0)
        for s in seqs:
            s.free()
        m.free()


# ------------------------------------------------------------------ 5. refusals

def test_bad_plans_leave_a_running_chain_intact(dev, golden_dir):
    from rama_amd._lib import rama_q8_seq_plan, rama_run_state
    m = open_model(dev, golden_dir, "ckpt_v2_q80_untied")
    c = m.cfg
    V, S = c.vocab_size, c.seq_len
    rng = np.random.default_rng(5)
    run = [Seq(rng, c, 0, T=1.0, u=0.3), Seq(rng, c, 3)]
    other = [Seq(rng, c, 0), Seq(rng, c, 0)]
    n_steps = 7
    try:
        for s in run + other:
            s.prepare(dev, m)
        want = [s.solo(n_steps) for s in run]
        assert begin(dev, m, run, n_steps) == 0
        assert steps(dev, 2) == 0
        f_ok, f_bad, f_neg = arr([1, 2]), arr([1, V]), arr([-1])

        def rec(T=0.0, topp=0.9, u=0.0, forced=f_ok, n_forced=0, max_new=0, stop=-1):
            return rama_q8_seq_plan(T, topp, u, forced, n_forced, max_new, stop)

        nan = float("nan")
        bad_records = [rec(T=-0.5), rec(T=nan), rec(topp=-0.1), rec(topp=1.1), rec(topp=nan), rec(u=-0.1), rec(u=1.0), rec(u=nan),
                       rec(n_forced=-1), rec(forced=None, n_forced=2), rec(forced=f_bad, n_forced=2), rec(forced=f_neg, n_forced=1),
                       rec(stop=V), rec(stop=-2), rec(max_new=-1)]
        for r in bad_records:
            assert begin(dev, m, other, 4, records=[rec(), r]) == EINVAL
        assert begin(dev, m, other, 4, positions=[0, S - 3]) == EINVAL                       # position + budget past seq_len
        assert begin(dev, m, other, 4, positions=[0, S - 3], plan=False) == EINVAL
        assert begin(dev, m, other, 4, positions=[0, S - 2], records=[rec(), rec(max_new=3)]) == EINVAL
        assert begin(dev, m, other, 4, positions=[-1, 0]) == EINVAL
        assert begin(dev, m, other, 4, tokens=[1, V]) == EINVAL
        assert begin(dev, m, other, 4, tokens=[-1, 1]) == EINVAL
        assert begin(dev, m, [other[0], other[0]], 4) == EINVAL                               # a shared run state
        assert begin(dev, m, other, 4, n_seq=0) == EINVAL
        assert begin(dev, m, other * 65, 4, n_seq=129, plan=False) == EINVAL
        assert begin(dev, m, other, 0) == EINVAL
        assert begin(dev, m, other, -1) == EINVAL
        st = (rama_run_state * 2)(*[s.eng.state for s in other])
        L, cfg, w = dev.lib, C.byref(m.ccfg), C.byref(m.weights)
        assert L.rama_q8_decode_batch_begin(dev.ctx, cfg, w, None, arr([1, 1]), arr([0, 0]), 2, 4, None) == EINVAL
        assert L.rama_q8_decode_batch_begin(dev.ctx, cfg, w, st, None, arr([0, 0]), 2, 4, None) == EINVAL
        assert L.rama_q8_decode_batch_begin(dev.ctx, cfg, w, st, arr([1, 1]), None, 2, 4, None) == EINVAL
        assert L.rama_q8_decode_batch_begin(dev.ctx, None, w, st, arr([1, 1]), arr([0, 0]), 2, 4, None) == EINVAL
        assert L.rama_q8_decode_batch_begin(dev.ctx, cfg, None, st, arr([1, 1]), arr([0, 0]), 2, 4, None) == EINVAL
        # the chain that was running goes on to the right tokens
        assert steps(dev, n_steps - 2) == 0
        assert tokens(dev, 2, n_steps) == want
        assert steps(dev, 1) == EINVAL                                                        # beyond max_steps
        assert steps(dev, -1) == EINVAL
        assert tokens(dev, 2, n_steps) == want
        # a budget that ends exactly at seq_len is accepted
        assert begin(dev, m, other, 4, positions=[0, S - 3], records=[rec(), rec(max_new=3)]) == 0
    finally:
        for s in run + other:
            s.free()
        m.free()


def test_vocabulary_above_32768(dev):
    """a sampled or forced plan is refused with RAMA_EUNSUP; the greedy chain runs"""
    import rama_amd
    from rama_amd._lib import rama_q8_seq_plan
    cfg = dict(dim=64, hidden_dim=192, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=32772, seq_len=32, shared_weight=True)
    m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), 32, 3)
    rng = np.random.default_rng(2)
    seqs = [Seq(rng, m.cfg, 0), Seq(rng, m.cfg, 2)]
    try:
        for s in seqs:
            s.prepare(dev, m)
        f = arr([4])
        assert begin(dev, m, seqs, 3, records=[rama_q8_seq_plan(0.0, 0.9, 0.0, f, 0, 0, -1), rama_q8_seq_plan(1.0, 0.9, 0.5, f, 0, 0, -1)]) == EUNSUP
        assert begin(dev, m, seqs, 3, records=[rama_q8_seq_plan(0.0, 0.9, 0.0, f, 1, 0, -1), rama_q8_seq_plan(0.0, 0.9, 0.0, f, 0, 0, -1)]) == EUNSUP
        assert begin(dev, m, seqs, 3) == 0
        assert steps(dev, 3) == 0
        assert tokens(dev, 2, 3) == [s.solo(3) for s in seqs]
    finally:
        for s in seqs:
            s.free()
        m.free()


# ------------------------------------------------------------------ 6. lifetimes, in graph mode

def test_other_q8_calls_and_graph_mode_toggles_between_steps(dev, golden_dir):
    import rama_amd
    from rama_amd.q8 import decode_batch
    m = open_model(dev, golden_dir, "synth15m")
    c = m.cfg
    rng = np.random.default_rng(9)
    seqs = [Seq(rng, c, 0, T=1.0, u=0.2), Seq(rng, c, 5), Seq(rng, c, 2, T=0.7, topp=0.5, u=0.8)]
    extra = [rama_amd.Q8Engine(dev, m) for _ in range(4)]
    n_steps = 9
    try:
        for s in seqs:
            s.prepare(dev, m)
        want = [s.solo(n_steps) for s in seqs]
        seqs[0].eng.set_graph_mode(1)
        assert begin(dev, m, seqs, n_steps) == 0
        assert steps(dev, 2) == 0
        extra[0].prefill([1] + [int(t) for t in rng.integers(0, c.vocab_size, 6)], 0)       # the same scratch, the same stream
        decode_batch(extra[1:], [3, 4, 5], [0, 0, 0])
        extra[0].forward(7, 7)
        assert steps(dev, 2) == 0
        seqs[0].eng.set_graph_mode(0)                                                       # the captured step goes; eager steps
        assert steps(dev, 2) == 0
        seqs[0].eng.set_graph_mode(1)                                                       # ... and is captured again
        assert steps(dev, 1) == 0
        assert dev.lib.rama_set_tuning(dev.ctx, b"spread_pos", 128) == 0                    # a tuning key that drops graphs
        assert steps(dev, n_steps - 7) == 0
        assert tokens(dev, 3, n_steps) == want
        for i, s in enumerate(seqs):
            check_cache_rows(s, s.pos + n_steps, i)
    finally:
        seqs[0].eng.set_graph_mode(0)
        for s in seqs:
            s.free()
        for e in extra:
            e.free()
        m.free()


def test_freed_member_or_model_refuses_steps(dev, golden_dir):
    import rama_amd
    m = open_model(dev, golden_dir, "ckpt_v2_q80_untied")
    rng = np.random.default_rng(12)
    seqs = [Seq(rng, m.cfg, 0), Seq(rng, m.cfg, 2), Seq(rng, m.cfg, 1)]
    bystander = rama_amd.Q8Engine(dev, m)
    try:
        for s in seqs:
            s.prepare(dev, m)
        want = [s.solo(6) for s in seqs]
        seqs[0].eng.set_graph_mode(1)
        assert begin(dev, m, seqs, 6) == 0
        assert steps(dev, 2) == 0
        bystander.forward(1, 0)
        bystander.free()                                           # a state outside the chain: nothing happens to it
        assert steps(dev, 2) == 0
        assert tokens(dev, 3, 6) == [w[:4] for w in want]
        seqs[1].eng.free()                                         # a member
        assert steps(dev, 1) == EINVAL
        assert steps(dev, 0) == EINVAL
        # a new chain over what is left runs; then the model goes
        left = [seqs[0], seqs[2]]
        assert begin(dev, m, left, 6, plan=False) == 0
        assert steps(dev, 3) == 0
        assert tokens(dev, 2, 6) == [want[0][:3], want[2][:3]]
        for s in seqs:
            s.twin.free()
        m.free()
        assert steps(dev, 1) == EINVAL
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        for s in seqs:
            s.free()
        m.free()


def test_second_model_of_another_shape_grows_the_scratch(golden_dir):
    """a context of its own, so that the second chain's model is the largest it has seen: the scratch moves between the chains"""
    import rama_amd
    d = rama_amd.Hip(0)
    small = open_model(d, golden_dir, "ckpt_v2_q80_tied")
    big = open_model(d, golden_dir, "synth15m")
    rng = np.random.default_rng(3)
    a = [Seq(rng, small.cfg, 0, T=1.0, u=0.4), Seq(rng, small.cfg, 2)]
    b = [Seq(rng, big.cfg, 4), Seq(rng, big.cfg, 0, T=1.0, u=0.6), Seq(rng, big.cfg, 1)]
    try:
        assert d.lib.rama_set_graph_mode(d.ctx, 1) == 0
        for s in a:
            s.prepare(d, small)
        assert begin(d, small, a, 5) == 0
        assert steps(d, 3) == 0
        for s in b:                                                # (prefill of the larger model already grows the scratch under the chain)
            s.prepare(d, big)
        assert steps(d, 2) == 0
        assert tokens(d, 2, 5) == [s.solo(5) for s in a]
        assert begin(d, big, b, 6) == 0
        assert steps(d, 6) == 0
        assert tokens(d, 3, 6) == [s.solo(6) for s in b]
        assert begin(d, small, a, 5, plan=False) == 0              # and back to the small one
        assert steps(d, 5) == 0
        a[0].T = 0.0
        assert tokens(d, 2, 5) == [s.solo(5) for s in a]
    finally:
        d.lib.rama_set_graph_mode(d.ctx, 0)
        for s in a + b:
            s.free()
        small.free(); big.free()
        d.close()


# ------------------------------------------------------------------ 7. the full shape

def test_7b_shape_one_layer_32_sequences_around_1024(dev):
    """one llama2-7B-shaped layer (GS 64): 32 sequences at positions 1000 .. 1031 behind a cache written directly, greedy, 4 steps,
    against rama_q8_forward + the last maximal index, one sequence at a time"""
    import rama_amd
    cfg = dict(dim=4096, hidden_dim=11008, n_layers=1, n_heads=32, n_kv_heads=32, vocab_size=32000, seq_len=2048, shared_weight=False)
    m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), 64, 5)
    n_seq, n_steps, d = 32, 4, cfg["dim"]
    rng = np.random.default_rng(0)
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(n_seq)]
    twin = rama_amd.Q8Engine(dev, m)
    try:
        poss = [1000 + i for i in range(n_seq)]
        toks = [int(t) for t in rng.integers(0, 32000, n_seq)]
        kv = (rng.standard_normal((2, 1040, d)) * 0.5).astype(np.float32)
        for e in engs:
            e.set_buffer("key_cache", kv[0]); e.set_buffer("value_cache", kv[1])
        engs[0].set_graph_mode(1)
        from rama_amd.q8 import decode_batch_chained
        got = decode_batch_chained(engs, toks, poss, n_steps)
        for i in range(n_seq):
            twin.set_buffer("key_cache", kv[0]); twin.set_buffer("value_cache", kv[1])
            t, want = toks[i], []
            for p in range(poss[i], poss[i] + n_steps):
                twin.forward(t, p)
                lg = twin.logits()
                t = int(lg.size - 1 - np.argmax(lg[::-1]))        # Device::sample at temperature 0: the last maximal index
                want.append(t)
            assert got[i] == want, i
            for name in ("key_cache", "value_cache"):
                assert same_bits(engs[i].buffer(name, n_steps * d, poss[i] * d), twin.buffer(name, n_steps * d, poss[i] * d)), (i, name)
    finally:
        engs[0].set_graph_mode(0)
        for e in engs + [twin]:
            e.free()
        m.free()
