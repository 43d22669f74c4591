"""The serving chain on the GPU (rama_q8_serve_begin / _admit / _steps / _poll / _tokens / _stats, rama_amd.Q8Server): continuous
batching.  Every admitted sequence's tokens and cache rows are bit for bit those of Q8Engine.generate run on it alone -- whatever
the chunking of its context, whoever shares its steps, admitted at the start or into a slot that has just finished -- in eager
and in graph mode; the device's row table is the host plan's; refusals leave the chain as it was.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_hip_q8 import same_bits

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -2
FREE, PROMPT, DECODE, DONE = 0, 1, 2, 3
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


# ------------------------------------------------------------------ a request, its solo run, the raw entry points

class Req:
    """a sequence to admit: its context (BOS first), its plan, its engine, and a twin for the solo run"""

    def __init__(self, dev, m, rng, n_ctx, max_new, T=0.0, topp=0.9, u=0.0, stop=-1):
        import rama_amd
        self.ctx = [1] + [int(t) for t in rng.integers(2, m.cfg.vocab_size, n_ctx - 1)]
        self.max_new, self.T, self.topp, self.u, self.stop = max_new, T, topp, u, stop
        self.eng, self.twin = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, m)
        fill_all(self.eng)
        self._solo = None

    def solo(self):
        """the max_new tokens Q8Engine.generate gives this sequence alone (no stop)"""
        if self._solo is None:
            n = len(self.ctx)
            self._solo = self.twin.generate(self.ctx[1:], n - 1 + self.max_new, self.T, self.topp, self.u)[n - 1:]
        return self._solo

    def want(self):
        out = []
        for t in self.solo():
            out.append(t)
            if t == self.stop:
                break
        return out

    def plan(self):
        from rama_amd._lib import rama_q8_serve_plan
        return rama_q8_serve_plan(self.T, self.topp, self.u, self.max_new, self.stop)

    def check(self, got, what):
        """tokens, every cache row 0..last, and the sentinel behind last"""
        assert got == self.want(), what
        last = len(self.ctx) + len(got) - 2                   # the last token recorded is not fed
        for a, b in zip(cache(self.eng), cache(self.twin)):
            assert same_bits(a[:, :last + 1], b[:, :last + 1]), what
            assert (a[:, last + 1:] == SENTINEL).all(), what

    def free(self):
        self.eng.free(); self.twin.free()


def cache(eng):
    c = eng.cfg
    n = c.n_layers * c.seq_len * c.dim
    return eng.buffer("key_cache", n).reshape(c.n_layers, c.seq_len, c.dim), eng.buffer("value_cache", n).reshape(c.n_layers, c.seq_len, c.dim)


def fill_all(eng):
    c = eng.cfg
    for name in ("key_cache", "value_cache"):
        eng.set_buffer(name, np.full(c.n_layers * c.seq_len * c.dim, SENTINEL))


def begin(dev, m, n_slots, max_rows, cap):
    return dev.lib.rama_q8_serve_begin(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), n_slots, max_rows, cap)


def admit(dev, slot, r, ctx=None, plan=None, eng=None):
    ctx = r.ctx if ctx is None else ctx
    p = r.plan() if plan is None else plan
    return dev.lib.rama_q8_serve_admit(dev.ctx, slot, C.byref((eng or r.eng).state), (C.c_int32 * max(len(ctx), 1))(*ctx), len(ctx), C.byref(p))


def steps(dev, n):
    return dev.lib.rama_q8_serve_steps(dev.ctx, n)


def poll(dev, slot, frm=0, cap=512):
    buf = (C.c_int32 * cap)()
    k, fin, gen = C.c_int(), C.c_int(-7), C.c_int(-7)
    assert dev.lib.rama_q8_serve_poll(dev.ctx, slot, frm, buf, cap, C.byref(k), C.byref(fin), C.byref(gen)) == 0
    assert fin.value in (0, 1)
    return [int(buf[i]) for i in range(k.value)], bool(fin.value), gen.value


def tokens(dev, slot, cap=512):
    buf = (C.c_int32 * cap)()
    k = C.c_int()
    assert dev.lib.rama_q8_serve_tokens(dev.ctx, slot, buf, cap, C.byref(k)) == 0
    return [int(buf[i]) for i in range(k.value)]


def stats(dev):
    from rama_amd._lib import rama_q8_serve_report
    r = rama_q8_serve_report()
    assert dev.lib.rama_q8_serve_stats(dev.ctx, C.byref(r)) == 0
    return dict(steps=int(r.steps), captures=int(r.graph_captures), decode=int(r.rows_decode), prompt=int(r.rows_prompt), idle=int(r.rows_idle),
                rows=[(x.slot, x.pos, x.logits) for x in r.last_rows[:r.max_rows]],
                slots=[(s.state, s.n_context, s.cursor, s.n_out, s.max_new) for s in r.slots[:r.n_slots]],
                generation=[int(g) for g in r.generation[:r.n_slots]])


def mixed_requests(dev, m, rng, sizes):
    """greedy and sampled plans in turn; every third request stops on a token of its own solo run"""
    samp = [(0.0, 0.9, 0.0), (1.0, 0.9, 0.1), (0.7, 0.5, 0.6), (0.0, 0.9, 0.0), (1.0, 0.95, 0.83)]
    reqs = []
    for i, (n_ctx, new) in enumerate(sizes):
        T, P, U = samp[i % len(samp)]
        r = Req(dev, m, rng, n_ctx, new, T, P, U)
        if i % 3 == 1 and new >= 3:
            r.stop = r.solo()[new // 2]
        reqs.append(r)
    return reqs


def shape(cfg):
    """(n_slots, max_rows, [(context length, max_new)]): one context of length 1, short ones, one longer than max_rows"""
    if cfg.seq_len < 64:
        return 4, 5, [(1, 6), (3, 4), (9, 5), (2, 7)]
    return 5, 8, [(1, 9), (3, 6), (21, 12), (6, 5), (37, 7)]


def set_graph(dev, on):
    assert dev.lib.rama_set_graph_mode(dev.ctx, int(on)) == 0


def run_until_done(dev, slots, limit=4000):
    """steps, one at a time, until the finished words of `slots` are set (read by poll only)"""
    import time
    for _ in range(limit):
        if all(poll(dev, s, 0, 1)[1] for s in slots):
            return
        assert steps(dev, 1) == 0
        while dev.lib.rama_stream_query(dev.ctx) == 1:
            time.sleep(0.0002)
    raise AssertionError("the slots did not finish")


# ------------------------------------------------------------------ 1. admitted at step 0

@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_tokens_and_cache_rows_equal_solo_generate(dev, golden_dir, which, graph):
    m = open_model(dev, golden_dir, which)
    n_slots, max_rows, sizes = shape(m.cfg)
    reqs = mixed_requests(dev, m, np.random.default_rng(7 + graph), sizes)
    try:
        for r in reqs:
            r.solo()
        set_graph(dev, graph)
        assert begin(dev, m, n_slots, max_rows, max(s[1] for s in sizes)) == 0
        for i, r in enumerate(reqs):
            assert admit(dev, i, r) == 0
        assert max(len(r.ctx) for r in reqs) > max_rows
        run_until_done(dev, range(len(reqs)))
        for i, r in enumerate(reqs):
            got = tokens(dev, i)
            assert poll(dev, i)[0] == got
            r.check(got, (which, graph, i))
        st = stats(dev)
        assert st["captures"] == (1 if graph else 0)
        assert all(s[0] == DONE for s in st["slots"][:len(reqs)])
        assert dev.lib.rama_q8_serve_end(dev.ctx) == 0
    finally:
        set_graph(dev, 0)
        for r in reqs:
            r.free()
        m.free()


# ------------------------------------------------------------------ 2. admission mid-run

def plan_steps_to_first_finish(reqs, n_slots, max_rows):
    """by the host plan (no stop token): the steps until the first slot is DONE -- a stop token only makes it earlier"""
    from rama_amd.q8 import serve_plan_step
    t = [(PROMPT, len(r.ctx), 0, 0, r.max_new) for r in reqs] + [(FREE, 0, 0, 0, 0)] * (n_slots - len(reqs))
    k = 0
    while not any(s[0] == DONE for s in t):
        _, t = serve_plan_step(t, max_rows)
        k += 1
    return k


@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_admission_into_a_finished_slot_mid_run(dev, golden_dir, which, graph):
    """all slots busy; a block of steps that runs well past the first finish is enqueued at once; the finished word is watched by
    rama_q8_serve_poll alone (no stream query, no download, no synchronising call); the newcomer -- with a run state of its own --
    is admitted while the rest of the block is in flight, and more steps are enqueued behind it"""
    import time
    m = open_model(dev, golden_dir, which)
    n_slots, max_rows, sizes = shape(m.cfg)
    rng = np.random.default_rng(21 + graph)
    reqs = mixed_requests(dev, m, rng, sizes[:n_slots])
    late = Req(dev, m, rng, sizes[2][0], 5, 1.0, 0.9, 0.37)              # a long context, sampled
    try:
        for r in reqs + [late]:
            r.solo()
        set_graph(dev, graph)
        assert begin(dev, m, n_slots, max_rows, max(s[1] for s in sizes)) == 0
        for i, r in enumerate(reqs):
            assert admit(dev, i, r) == 0
        assert admit(dev, 0, late) == EINVAL                             # every slot is busy
        past = 24
        assert steps(dev, plan_steps_to_first_finish(reqs, n_slots, max_rows) + past) == 0      # one block, asynchronous
        first, deadline = None, time.time() + 60
        while first is None and time.time() < deadline:
            for i in range(n_slots):
                if poll(dev, i, 0, 1)[1]:
                    first = i
                    break
        assert first is not None
        old_tokens, _, gen0 = poll(dev, first)                            # (the finished word is set: every token is there)
        assert admit(dev, first, late) == 0                               # ... behind whatever of the block is still running
        assert steps(dev, 4) == 0
        in_flight = dev.lib.rama_stream_query(dev.ctx) == 1
        after_admit = poll(dev, first)
        assert after_admit[2] == gen0 + 1
        assert after_admit[0] == late.want()[:len(after_admit[0])]        # the ring row holds the newcomer's tokens only
        assert steps(dev, sum(len(r.ctx) + r.max_new for r in reqs + [late])) == 0      # every live slot advances in every step
        if which == "synth15m":
            assert in_flight, "the admission was meant to happen with steps still running"
        old = reqs[first]
        for i, r in enumerate(reqs):
            if i != first:
                r.check(tokens(dev, i), (which, graph, i))
        got_late = tokens(dev, first)
        assert poll(dev, first)[:2] == (got_late, True)
        late.check(got_late, (which, graph, "late"))
        # the old occupant's run state, downloaded only now: its rows are its twin's and nothing behind them was written
        old.check(old_tokens, (which, graph, "old"))
        st = stats(dev)
        assert st["captures"] == (1 if graph else 0)
        assert st["generation"][first] == gen0 + 1
        assert all(s[0] == DONE for s in st["slots"])
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs + [late]:
            r.free()
        m.free()


# ------------------------------------------------------------------ 3. slot reuse through Q8Server

@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("max_rows", [8, 16])
def test_server_pushes_requests_through_reused_slots(dev, golden_dir, which, graph, max_rows):
    import rama_amd
    from rama_amd.q8 import Q8Server
    m = open_model(dev, golden_dir, which)
    c = m.cfg
    rng = np.random.default_rng(300 + max_rows + graph)
    small = c.seq_len < 64
    twin = rama_amd.Q8Engine(dev, m)
    srv = None
    try:
        reqs = []
        for i in range(14):
            n_ctx = int(rng.integers(1, 10 if small else 40))
            new = int(rng.integers(1, (c.seq_len - n_ctx if small else 14) + 1))
            T, P, U = [(0.0, 0.9, 0.0), (1.0, 0.9, 0.21), (0.8, 0.6, 0.7)][i % 3]
            ctx = [1] + [int(t) for t in rng.integers(2, c.vocab_size, n_ctx - 1)]
            want = twin.generate(ctx[1:], n_ctx - 1 + new, T, P, U)[n_ctx - 1:]
            reqs.append((ctx, new, T, P, U, want))
        set_graph(dev, graph)
        srv = Q8Server(m, 4, max_rows, max(r[1] for r in reqs))
        streamed = {}
        hs = [srv.submit(ctx, new, T, P, U) for ctx, new, T, P, U, _ in reqs]
        srv.run(on_token=lambda h, i, t: streamed.setdefault(h, []).append((i, t)))
        for h, r in zip(hs, reqs):
            assert srv.finished(h)
            assert srv.result(h) == r[5], (which, graph, max_rows, h)
            assert streamed[h] == list(enumerate(r[5]))
        st = srv.stats()
        assert st["graph_captures"] == (1 if graph else 0)
        # no stop tokens here, so the host plan is exact: the device's sums are the plan's, idle rows included
        for k in ("steps", "rows_decode", "rows_prompt", "rows_idle"):
            assert st[k] == srv.planned[k], (k, st[k], srv.planned[k])
        assert st["rows_prompt"] == sum(len(r[0]) for r in reqs) and st["rows_decode"] == sum(r[1] - 1 for r in reqs)
        assert max(st["generation"]) >= 3
        # six more through the same slots, a step at a time: the device's row table is the host plan's in every step -- so no row
        # is idle where the plan has none
        more = [srv.submit(ctx, new, T, P, U) for ctx, new, T, P, U, _ in reqs[:6]]
        n_steps = 0
        while not all(srv.finished(h) for h in more):
            srv.step(1)
            now = srv.stats()
            assert now["last_rows"] == srv.last_rows, n_steps
            n_steps += 1
            assert n_steps < 2000
        for h, r in zip(more, reqs[:6]):
            assert srv.result(h) == r[5]
        assert srv.stats()["graph_captures"] == (1 if graph else 0)
    finally:
        if srv is not None:
            srv.close()
        set_graph(dev, 0)
        twin.free()
        m.free()


# ------------------------------------------------------------------ 4. the device's row table is the host plan's

@pytest.mark.parametrize("graph", [0, 1])
def test_device_plan_equals_host_plan(dev, golden_dir, graph):
    from rama_amd.q8 import serve_plan_step
    m = open_model(dev, golden_dir, "synth15m")
    rng = np.random.default_rng(4)
    n_slots, max_rows = 6, 16
    reqs = [Req(dev, m, rng, n, new) for n, new in [(1, 5), (30, 3), (7, 9), (45, 2), (2, 1)]]        # slot 5 stays FREE
    try:
        set_graph(dev, graph)
        assert begin(dev, m, n_slots, max_rows, 16) == 0
        for i, r in enumerate(reqs):
            assert admit(dev, i, r) == 0
        before = stats(dev)
        assert before["steps"] == 0 and [s[0] for s in before["slots"]] == [PROMPT] * 5 + [FREE]
        totals = dict(decode=0, prompt=0, idle=0)
        for step in range(60):
            if not any(s[0] in (PROMPT, DECODE) for s in before["slots"]):
                break
            assert steps(dev, 1) == 0
            now = stats(dev)
            rows, after = serve_plan_step(before["slots"], max_rows)
            assert now["rows"] == rows, step
            assert now["slots"] == after, step                 # (greedy plans without stop tokens: the successor is exact)
            used = [r for r in rows if r[0] >= 0]
            dec = sum(1 for r in used if before["slots"][r[0]][0] == DECODE)
            totals["decode"] += dec; totals["prompt"] += len(used) - dec; totals["idle"] += max_rows - len(used)
            assert (now["decode"], now["prompt"], now["idle"], now["steps"]) == (totals["decode"], totals["prompt"], totals["idle"], step + 1)
            before = now
        assert all(s[0] in (DONE, FREE) for s in before["slots"]) and before["steps"] > 8
        for i, r in enumerate(reqs):
            r.check(tokens(dev, i), i)
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs:
            r.free()
        m.free()


# ------------------------------------------------------------------ 5. the full shape

SIZES_7B = [(2, 14), (1100, 4), (3, 12), (1, 13)]


@pytest.fixture(scope="module")
def shape_7b(dev):
    """one llama2-7B-shaped layer (GS 64), four contexts, and -- taken once, by rama_q8_forward + the last maximal index, position
    by position -- every sequence's tokens and cache rows"""
    import rama_amd
    cfg = dict(dim=4096, hidden_dim=11008, n_layers=1, n_heads=32, n_kv_heads=32, vocab_size=32000, seq_len=2048, shared_weight=False)
    m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), 64, 5)
    rng = np.random.default_rng(0)
    ctxs = [[1] + [int(t) for t in rng.integers(2, 32000, n - 1)] for n, _ in SIZES_7B]
    twin = rama_amd.Q8Engine(dev, m)
    want, want_rows = [], []
    try:
        for ctx, (n, new) in zip(ctxs, SIZES_7B):
            toks, t = [], None
            for p in range(n + new - 1):
                twin.forward(ctx[p] if p < n else t, p)
                if p >= n - 1:
                    lg = twin.logits()
                    t = int(lg.size - 1 - np.argmax(lg[::-1]))        # Device::sample at temperature 0: the last maximal index
                    toks.append(t)
            want.append(toks)
            want_rows.append({name: twin.buffer(name, (n + new - 1) * cfg["dim"]) for name in ("key_cache", "value_cache")})
    finally:
        twin.free()
    yield m, ctxs, want, want_rows
    m.free()


@pytest.mark.parametrize("max_rows", [24, 48, 128])
def test_7b_shape_one_layer_context_across_1024_next_to_decoding_slots(dev, shape_7b, max_rows):
    """one llama2-7B-shaped layer (GS 64): a context of 1 100 tokens ingested in chunks next to three decoding slots, graph mode, at
    24 rows (the products' ksplit<2> form), 48 (the one-wave MFMA form over four token tiles, the fourth one beyond max_rows) and
    128; tokens and cache rows against rama_q8_forward + the last maximal index, position by position (taken once, shape_7b)"""
    import rama_amd
    from rama_amd._lib import rama_q8_serve_plan
    from rama_amd.q8 import serve_plan_step
    m, ctxs, want, want_rows = shape_7b
    sizes = SIZES_7B
    d = m.cfg.dim
    engs = [rama_amd.Q8Engine(dev, m) for _ in sizes]
    try:
        set_graph(dev, 1)
        assert begin(dev, m, 4, max_rows, 16) == 0
        for i, (ctx, (_, new)) in enumerate(zip(ctxs, sizes)):
            p = rama_q8_serve_plan(0.0, 0.9, 0.0, new, -1)
            assert dev.lib.rama_q8_serve_admit(dev.ctx, i, C.byref(engs[i].state), (C.c_int32 * len(ctx))(*ctx), len(ctx), C.byref(p)) == 0
        t, n_steps = [(PROMPT, n, 0, 0, new) for n, new in sizes], 0     # greedy plans without a stop token: the host plan is exact
        while any(s[0] in (PROMPT, DECODE) for s in t):
            _, t = serve_plan_step(t, max_rows)
            n_steps += 1
        assert n_steps == {24: 51, 48: 27, 128: 14}[max_rows]      # (14: the count this test enqueued before it took the plan's)
        assert steps(dev, n_steps) == 0
        st = stats(dev)
        assert all(s[0] == DONE for s in st["slots"]) and st["captures"] == 1 and st["steps"] == n_steps
        assert st["prompt"] == sum(n for n, _ in sizes) and st["decode"] == sum(new - 1 for _, new in sizes)
        set_graph(dev, 0)
        for i, (n, new) in enumerate(sizes):
            assert tokens(dev, i) == want[i], i
            rows = (n + new - 1) * d
            for name in ("key_cache", "value_cache"):
                assert same_bits(engs[i].buffer(name, rows), want_rows[i][name]), (i, name)
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for e in engs:
            e.free()


# ------------------------------------------------------------------ 6. refusals

@pytest.mark.parametrize("graph", [0, 1])
def test_refusals_leave_the_running_chain_as_it_was(dev, golden_dir, graph):
    from rama_amd._lib import rama_q8_serve_plan
    m = open_model(dev, golden_dir, "synth15m")
    c = m.cfg
    rng = np.random.default_rng(6)
    reqs = [Req(dev, m, rng, 5, 10, 1.0, 0.9, 0.3), Req(dev, m, rng, 19, 8)]
    extra = Req(dev, m, rng, 4, 6)
    try:
        assert begin(dev, m, 0, 4, 8) == EINVAL and begin(dev, m, 4, 3, 8) == EINVAL and begin(dev, m, 4, 129, 8) == EINVAL
        assert begin(dev, m, 4, 8, 0) == EINVAL and begin(dev, m, 4, 8, c.seq_len) == EINVAL
        assert steps(dev, 1) == EINVAL                                    # no chain yet
        set_graph(dev, graph)
        assert begin(dev, m, 3, 8, 12) == 0
        for i, r in enumerate(reqs):
            assert admit(dev, i, r) == 0
        assert steps(dev, 2) == 0
        ok = extra.plan()
        refused = [
            admit(dev, 0, extra),                                         # a busy slot
            admit(dev, 2, extra, eng=reqs[1].eng),                        # a run state already live
            admit(dev, 2, extra, ctx=[1] * (c.seq_len - 5)),              # context + budget beyond seq_len
            admit(dev, 2, extra, plan=rama_q8_serve_plan(0.0, 0.9, 0.0, 13, -1)),      # max_new over the cap
            admit(dev, 2, extra, plan=rama_q8_serve_plan(-1.0, 0.9, 0.0, 4, -1)),      # bad plans
            admit(dev, 2, extra, plan=rama_q8_serve_plan(1.0, 1.5, 0.0, 4, -1)),
            admit(dev, 2, extra, plan=rama_q8_serve_plan(1.0, 0.9, 1.0, 4, -1)),
            admit(dev, 2, extra, plan=rama_q8_serve_plan(0.0, 0.9, 0.0, 0, -1)),
            admit(dev, 2, extra, plan=rama_q8_serve_plan(0.0, 0.9, 0.0, 4, c.vocab_size)),
            admit(dev, 2, extra, ctx=[1, c.vocab_size]),
            admit(dev, 2, extra, ctx=[]),
            admit(dev, 3, extra), admit(dev, -1, extra),
        ]
        assert refused == [EINVAL] * len(refused)
        assert steps(dev, -1) == EINVAL
        assert admit(dev, 2, extra, plan=ok) == 0                        # ... and a good one still goes in
        run_until_done(dev, [0, 1, 2])
        for i, r in enumerate(reqs + [extra]):
            r.check(tokens(dev, i), (graph, i))
        assert stats(dev)["captures"] == (1 if graph else 0)
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs + [extra]:
            r.free()
        m.free()


def test_steps_refuse_after_a_free(dev, golden_dir):
    """rama_state_free of an occupied slot's run state, or rama_q8_model_free, ends the chain; a finished occupant's state may go"""
    import rama_amd
    for what in ("state", "done_state", "model"):
        m = open_model(dev, golden_dir, "ckpt_v2_q80_tied")
        rng = np.random.default_rng(9)
        reqs = [Req(dev, m, rng, 3, 2), Req(dev, m, rng, 4, 9)]
        try:
            set_graph(dev, 1)
            assert begin(dev, m, 2, 4, 12) == 0
            for i, r in enumerate(reqs):
                assert admit(dev, i, r) == 0
            assert steps(dev, 3) == 0
            assert dev.lib.rama_sync(dev.ctx) == 0
            assert poll(dev, 0)[1] and not poll(dev, 1)[1]
            if what == "state":
                reqs[1].eng.free()
                assert steps(dev, 1) == EINVAL
                assert admit(dev, 0, reqs[0]) == EINVAL
            elif what == "done_state":
                reqs[0].eng.free()                                        # slot 0 has finished: its run state is its owner's again
                assert steps(dev, 1) == 0
            else:
                m.free()
                assert steps(dev, 1) == EINVAL
            assert dev.lib.rama_q8_serve_end(dev.ctx) == 0
            assert steps(dev, 1) == EINVAL
        finally:
            set_graph(dev, 0)
            dev.lib.rama_q8_serve_end(dev.ctx)
            for r in reqs:
                r.twin.free(); r.eng.free()
            m.free()


@pytest.mark.parametrize("graph", [0, 1])
def test_the_two_chains_alternate_on_one_context(dev, golden_dir, graph):
    """the existing chained batch and the serving chain, stepped in turn: neither disturbs the other"""
    from tests import test_hip_q8_chain as T
    m = open_model(dev, golden_dir, "synth15m")
    rng = np.random.default_rng(12)
    seqs = [T.Seq(rng, m.cfg, 0, T=1.0, topp=0.9, u=0.4), T.Seq(rng, m.cfg, 5), T.Seq(rng, m.cfg, 0)]
    reqs = [Req(dev, m, rng, 11, 9, 0.9, 0.8, 0.55), Req(dev, m, rng, 2, 12)]
    n_steps = 10
    try:
        for s in seqs:
            s.prepare(dev, m)
        want = [s.solo(n_steps) for s in seqs]
        for r in reqs:
            r.solo()
        set_graph(dev, graph)
        assert begin(dev, m, 2, 4, 12) == 0
        assert T.begin(dev, m, seqs, n_steps) == 0
        for i, r in enumerate(reqs):
            assert admit(dev, i, r) == 0
        for _ in range(n_steps // 2):
            assert T.steps(dev, 2) == 0
            assert steps(dev, 3) == 0
        assert T.tokens(dev, len(seqs), n_steps) == want
        run_until_done(dev, [0, 1])
        for i, r in enumerate(reqs):
            r.check(tokens(dev, i), (graph, i))
        assert stats(dev)["captures"] == (1 if graph else 0)
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for s in seqs:
            s.free()
        for r in reqs:
            r.free()
        m.free()


# ------------------------------------------------------------------ 9. the host's drain across a full poll

def test_server_collects_more_than_one_full_poll_at_once(dev):
    """70 tokens wait in a slot's ring when the host first looks: one poll() takes the 64 a call of rama_q8_serve_poll returns
    and the 6 behind them, and sees the finished word only with the short call"""
    import rama_amd
    from rama_amd.q8 import Q8Server
    cfg = O.Config(dim=64, hidden_dim=192, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=64, seq_len=128, shared_weight=True)
    m = rama_amd.Q8Model.synth(dev, cfg, 64, 3)
    twin = rama_amd.Q8Engine(dev, m)
    srv = None
    try:
        ctx, new = [1, 7], 70
        want = twin.generate(ctx[1:], 1 + new)[1:]
        srv = Q8Server(m, 1, max_new_cap=new)
        h = srv.submit(ctx, new)
        srv.step(1 + new)                                     # (one row a step: two steps for the context, the second gives token 0)
        assert dev.lib.rama_sync(dev.ctx) == 0
        assert srv.result(h) == [] and not srv.finished(h)
        streamed = []
        srv.poll(on_token=lambda hh, i, t: streamed.append((hh, i, t)))
        assert len(want) == new and srv.result(h) == want and srv.finished(h)
        assert streamed == [(h, i, t) for i, t in enumerate(want)]
    finally:
        if srv is not None:
            srv.close()
        twin.free()
        m.free()
