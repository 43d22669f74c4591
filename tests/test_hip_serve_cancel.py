"""Cancel, exact resume and preemption in both serving chains on the GPU (rama_q8_serve_cancel / rama_serve_cancel, ServeLoop.cancel /
preempt): a cancelled slot's tokens are the first tokens of its solo run, its rows below the cursor the solo run's and the rows behind it
untouched; its neighbours never notice; every later step's row table is the host rule over the device's previous slot table; a sequence
cancelled after k tokens and admitted again over its own rows ends with the tokens and cache rows of the uninterrupted run.  The yardsticks
are Q8Engine.generate and parity-mode Engine.generate on the sequence alone and the host plan; every comparison is exact."""
import ctypes as C
import time

import numpy as np
import pytest

from oracle import synth as S
from tests import serve_cases as W
from tests import test_hip_q8_serve as Q
from tests import test_hip_serve as F
from tests.helpers import GOLDEN, to_rama_cfg

pytestmark = pytest.mark.gpu

EINVAL = -1
FREE, PROMPT, DECODE, DONE = 0, 1, 2, 3
CANCELLED = 2
SENTINEL = Q.SENTINEL


class Stack:
    """one of the two chains: its entries, its models, its requests (tests/test_hip_q8_serve.py's and tests/test_hip_serve.py's)"""

    def __init__(self, kind):
        import rama_amd
        from rama_amd._lib import check
        self.kind, self.abi = kind, "rama_q8_serve" if kind == "q8" else "rama_serve"
        self.dev = rama_amd.Hip(0)
        if kind == "f32":
            check(self.dev.lib.rama_set_tuning(self.dev.ctx, b"ref_order", 1))
        self._models = {}

    def entry(self, name):
        return getattr(self.dev.lib, f"{self.abi}_{name}")

    def model(self, which):
        """"small": the dim-32 fixture of the stack; "15m": a stories15M-shaped synthetic model -> (config, model)"""
        import rama_amd
        if which not in self._models:
            if self.kind == "q8":
                m = Q.open_model(self.dev, GOLDEN, "ckpt_v2_q80_tied" if which == "small" else "synth15m")
                self._models[which] = (m.cfg, m)
            elif which == "small":
                m = rama_amd.Model.load(self.dev, GOLDEN / "ckpt_tied.bin")
                self._models[which] = (m.cfg, m)
            else:
                cfg = W.STORIES15M
                self._models[which] = (cfg, rama_amd.Model.synth(self.dev, to_rama_cfg(cfg), 23, rope=S.rope_tables(cfg.seq_len, cfg.head_size)))
        return self._models[which]

    def req(self, which, rng, n_ctx, max_new, T=0.0, topp=0.9, u=0.0):
        cfg, m = self.model(which)
        r = Q.Req(self.dev, m, rng, n_ctx, max_new, T, topp, u) if self.kind == "q8" else F.Req(self.dev, cfg, m, rng, n_ctx, max_new, T, topp, u)
        r.shape = cfg
        r.solo()
        return r

    def cache(self, eng, cfg):
        n = cfg.n_layers * cfg.seq_len * cfg.dim
        return [eng.buffer(k, n).reshape(cfg.n_layers, cfg.seq_len, cfg.dim) for k in ("key_cache", "value_cache")]

    def begin(self, which, n_slots, max_rows, cap):
        _, m = self.model(which)
        return self.entry("begin")(self.dev.ctx, C.byref(m.ccfg), C.byref(m.weights), n_slots, max_rows, cap)

    def admit(self, slot, r, ctx=None, n_cached=0, max_new=None, eng=None):
        from rama_amd._lib import rama_q8_serve_plan
        ctx = r.ctx if ctx is None else ctx
        p = rama_q8_serve_plan(r.T, r.topp, r.u, r.max_new if max_new is None else max_new, r.stop)
        return self.entry("admit_at")(self.dev.ctx, slot, C.byref((eng or r.eng).state), (C.c_int32 * len(ctx))(*ctx), len(ctx), n_cached, C.byref(p))

    def steps(self, n):
        return self.entry("steps")(self.dev.ctx, n)

    def cancel(self, slots, n=None):
        arr = (C.c_int32 * max(len(slots), 1))(*slots) if slots is not None else None
        return self.entry("cancel")(self.dev.ctx, arr, len(slots) if n is None else n)

    def poll(self, slot):
        """-> (tokens, the finished word, generation): never touches the stream"""
        buf = (C.c_int32 * 512)()
        k, fin, gen = C.c_int(), C.c_int(-7), C.c_int(-7)
        assert self.entry("poll")(self.dev.ctx, slot, 0, buf, 512, C.byref(k), C.byref(fin), C.byref(gen)) == 0
        return [int(buf[i]) for i in range(k.value)], fin.value, gen.value

    def wait_word(self, slot):
        """the slot's finished word once it is set, by polling alone (0: the stream has drained and it is not)"""
        while True:
            busy = self.dev.lib.rama_stream_query(self.dev.ctx) == 1
            w = self.poll(slot)[1]
            if w or not busy:
                return w
            time.sleep(0.0002)

    def stats(self):
        from rama_amd._lib import rama_q8_serve_report
        r = rama_q8_serve_report()
        assert self.entry("stats")(self.dev.ctx, C.byref(r)) == 0
        return dict(steps=int(r.steps), captures=int(r.graph_captures), counts=(int(r.rows_decode), int(r.rows_prompt), int(r.rows_idle)),
                    rows=[(x.slot, x.pos, x.logits) for x in r.last_rows[:r.max_rows]],
                    slots=[(s.state, s.n_context, s.cursor, s.n_out, s.max_new) for s in r.slots[:r.n_slots]],
                    generation=[int(g) for g in r.generation[:r.n_slots]])

    def cancel_launches(self):
        """serve_cancel_kernel launches since the chain began (an accessor the library exports for this test)"""
        fn = self.dev.lib.rama_internal_serve_cancel_launches
        fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p, C.c_int]
        return fn(self.dev.ctx, int(self.kind == "f32"))

    def graph(self, on):
        assert self.dev.lib.rama_set_graph_mode(self.dev.ctx, int(on)) == 0

    def end(self):
        assert self.entry("end")(self.dev.ctx) == 0

    def close(self):
        from rama_amd._lib import check
        self.entry("end")(self.dev.ctx)
        self.graph(0)
        for _, m in self._models.values():
            m.free()
        if self.kind == "f32":
            check(self.dev.lib.rama_set_tuning(self.dev.ctx, b"ref_order", 0))
        self.dev.close()


@pytest.fixture(scope="module", params=["q8", "f32"])
def stack(request):
    s = Stack(request.param)
    yield s
    s.close()


def ruled_step(S_, max_rows):
    """one step; the device's row table and counters are the host rule applied to the device's slot table before it -> the stats after"""
    from rama_amd.q8 import serve_plan_step
    before = S_.stats()
    assert S_.steps(1) == 0
    after = S_.stats()
    rows, _ = serve_plan_step(before["slots"], max_rows)
    dec = sum(1 for s, _, _ in rows if s >= 0 and before["slots"][s][0] == DECODE)
    used = sum(1 for s, _, _ in rows if s >= 0)
    assert after["rows"] == rows and after["steps"] == before["steps"] + 1
    assert tuple(a - b for a, b in zip(after["counts"], before["counts"])) == (dec, used - dec, max_rows - used)
    return after


def rows_check(S_, r, cursor, what):
    """rows below the cursor are the solo run's, the rows from it on untouched"""
    for a, b in zip(S_.cache(r.eng, r.shape), S_.cache(r.twin, r.shape)):
        assert F.same_bits(a[:, :cursor], b[:, :cursor]), what
        assert (a[:, cursor:] == SENTINEL).all(), what


def free(reqs):
    for r in reqs:
        r.free()


# ------------------------------------------------------------------ a PROMPT slot and a DECODE slot cancelled, the neighbours untouched

@pytest.mark.parametrize("which", ["small", "15m"])
@pytest.mark.parametrize("graph", [0, 1])
def test_cancelled_prompt_and_decode_slots_and_their_neighbours(stack, which, graph):
    rng = np.random.default_rng(5 + graph)
    reqs = [stack.req(which, rng, n, new, *samp) for (n, new), samp in zip([(2, 8), (3, 6), (11, 4), (1, 7)],
                                                                            [(0.0, 0.9, 0.0), (1.0, 0.9, 0.1), (0.0, 0.9, 0.0), (0.7, 0.5, 0.6)])]
    try:
        stack.graph(graph)
        assert stack.begin(which, 4, 8, 8) == 0
        for i, r in enumerate(reqs):
            assert stack.admit(i, r) == 0
        st = ruled_step(stack, 8)
        assert st["slots"][2][0] == PROMPT and 0 < st["slots"][2][2] < 11        # in the middle of a context longer than max_rows
        assert stack.cancel([2]) == 0
        now = stack.stats()
        assert now["slots"][2] == (DONE,) + st["slots"][2][1:] and now["slots"][:2] + now["slots"][3:] == st["slots"][:2] + st["slots"][3:]
        assert stack.poll(2)[:2] == ([], CANCELLED)
        cut = st["slots"][2][2]
        for _ in range(3):
            st = ruled_step(stack, 8)
        assert st["slots"][0][0] == DECODE and st["slots"][0][3] == 4
        assert stack.cancel([0, 0]) == 0                                          # (duplicates are fine)
        now = stack.stats()
        assert now["slots"][0] == (DONE,) + st["slots"][0][1:] and now["slots"][1:] == st["slots"][1:] and now["steps"] == st["steps"]
        toks, word, _ = stack.poll(0)
        assert word == CANCELLED and toks == reqs[0].solo()[:4]
        for _ in range(12):
            st = ruled_step(stack, 8)
            assert all(s != 0 and s != 2 for s, _, _ in st["rows"])               # no row for a cancelled slot, ever
        assert [s[0] for s in st["slots"]] == [DONE] * 4 and st["slots"][0] == now["slots"][0] and st["slots"][2][2] == cut
        assert [stack.poll(i)[1] for i in range(4)] == [CANCELLED, 1, CANCELLED, 1]
        rows_check(stack, reqs[0], now["slots"][0][2], (which, graph, 0))
        rows_check(stack, reqs[2], cut, (which, graph, 2))
        for i in (1, 3):
            reqs[i].check(stack.poll(i)[0], (which, graph, i))
        assert st["captures"] == (1 if graph else 0)
        stack.end()
    finally:
        stack.graph(0)
        free(reqs)


# ------------------------------------------------------------------ the occupant finishes first; cancels that do nothing; refusals

@pytest.mark.parametrize("graph", [0, 1])
def test_a_finish_beats_the_cancel_and_idle_cancels_and_refusals_change_nothing(stack, graph):
    rng = np.random.default_rng(11)
    reqs = [stack.req("small", rng, 2, 3), stack.req("small", rng, 3, 8), stack.req("small", rng, 2, 8)]
    try:
        stack.graph(graph)
        assert stack.begin("small", 4, 8, 8) == 0 and stack.cancel_launches() == 0
        assert stack.admit(0, reqs[0]) == 0 and stack.admit(1, reqs[1]) == 0 and stack.admit(3, reqs[2]) == 0
        assert stack.steps(5) == 0 and stack.cancel([0]) == 0                      # enqueued behind the steps that finish slot 0: no synchronisation
        assert stack.wait_word(0) == 1 and stack.poll(0)[0] == reqs[0].solo()
        st, n0 = stack.stats(), stack.cancel_launches()
        assert n0 in (0, 1)                                                        # (0: the host saw the finished word before the call)
        assert st["slots"][0] == (DONE, 2, 4, 3, 3) and st["slots"][1][0] == DECODE and st["slots"][3][0] == DECODE
        # a slot seen finished, a slot never admitted, an empty list: success, nothing is launched and nothing changes
        for slots in ([0], [2], [0, 2, 2], []):
            assert stack.cancel(slots) == 0
        assert stack.cancel(None, 0) == 0
        assert stack.cancel_launches() == n0
        assert stack.stats() == st and stack.poll(0)[1] == 1 and stack.poll(2)[1] == 0
        # every refusal: nothing is launched, the chain untouched
        for slots, n in ((None, 1), ([1], -1), ([1] * 129, 129), ([4], 1), ([1, -1], 2), ([1, 4], 2)):
            assert stack.cancel(slots, n) == EINVAL
        assert stack.cancel_launches() == n0
        assert stack.stats() == st and stack.poll(1)[1] == 0
        # live and dead slots in one list: exactly one launch, and only the live one of the list ends
        assert stack.cancel([0, 3, 2, 3]) == 0 and stack.cancel_launches() == n0 + 1
        now = stack.stats()
        assert now["slots"][3] == (DONE,) + st["slots"][3][1:] and now["slots"][:3] == st["slots"][:3]
        assert stack.poll(3)[:2] == (reqs[2].solo()[:5], CANCELLED) and stack.poll(0)[1] == 1 and stack.poll(2)[1] == 0
        while not stack.wait_word(1):
            assert stack.steps(2) == 0
        assert stack.poll(1)[:2] == (reqs[1].solo(), 1)
        reqs[1].check(stack.poll(1)[0], graph)
        assert stack.stats()["captures"] == (1 if graph else 0)
        stack.end()
        assert stack.cancel([0]) == EINVAL and stack.cancel([], 0) == EINVAL       # no chain
    finally:
        stack.graph(0)
        free(reqs)


# ------------------------------------------------------------------ cancel, then another sequence into the slot, steps in flight

@pytest.mark.parametrize("graph", [0, 1])
def test_cancel_then_admit_into_the_slot_behind_steps_in_flight(stack, graph):
    rng = np.random.default_rng(13)
    reqs = [stack.req("small", rng, 3, 9), stack.req("small", rng, 2, 9, 1.0, 0.9, 0.3), stack.req("small", rng, 4, 5)]
    try:
        stack.graph(graph)
        assert stack.begin("small", 2, 6, 9) == 0
        assert stack.admit(0, reqs[0]) == 0 and stack.admit(1, reqs[1]) == 0
        assert stack.steps(3) == 0 and stack.cancel([0]) == 0 and stack.steps(4) == 0
        gen = stack.poll(0)[2]
        assert stack.wait_word(0) == CANCELLED                                     # (polling only)
        got0 = stack.poll(0)[0]
        assert stack.admit(0, reqs[2]) == 0 and stack.poll(0)[1:] == (0, gen + 1)
        while not (stack.wait_word(0) and stack.wait_word(1)):
            assert stack.steps(3) == 0
        assert got0 == reqs[0].solo()[:3]
        reqs[2].check(stack.poll(0)[0], graph)
        reqs[1].check(stack.poll(1)[0], graph)
        assert stack.stats()["captures"] == (1 if graph else 0)
        stack.end()
    finally:
        stack.graph(0)
        free(reqs)


# ------------------------------------------------------------------ exact resume

@pytest.mark.parametrize("which,graph", [("small", 0), ("small", 1), ("15m", 1)])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_resume_on_the_same_run_state_gives_the_uninterrupted_run(stack, which, graph, k):
    """three slots -- greedy, sampled (T 1, top-p 0.9), and one with a stop token that falls after the resume (the first token from
    index k on that the run has not produced before; none if there is none) -- cancelled together after k tokens, then admitted again:
    the old context plus the k outputs, n_cached = the cursor, max_new - k left"""
    rng = np.random.default_rng(17 + k)
    new = 9
    reqs = [stack.req(which, rng, 3, new), stack.req(which, rng, 3, new, 1.0, 0.9, 0.37), stack.req(which, rng, 3, new, 1.0, 0.9, 0.81)]
    solo = reqs[2].solo()
    late = [j for j in range(k, new) if solo[j] not in solo[:j]]
    reqs[2].stop = solo[late[0]] if late else -1
    try:
        stack.graph(graph)
        assert stack.begin(which, 3, 9, new) == 0
        for i, r in enumerate(reqs):
            assert stack.admit(i, r) == 0
        assert stack.steps(k) == 0 and stack.cancel([0, 1, 2]) == 0
        st = stack.stats()
        first = [stack.poll(i) for i in range(3)]
        for i, r in enumerate(reqs):
            assert first[i][:2] == (r.solo()[:k], CANCELLED) and st["slots"][i] == (DONE, 3, 3 + k - 1, k, new)
            ctx = r.ctx + first[i][0]
            assert stack.admit(i, r, ctx=ctx, n_cached=min(st["slots"][i][2], len(ctx) - 1), max_new=new - k) == 0
        fed = ruled_step(stack, 9)
        assert fed["rows"][:3] == [(i, 3 + k - 1, 1) for i in range(3)]            # a resume costs one row, not a prompt
        while not all(stack.wait_word(i) for i in range(3)):
            assert stack.steps(2) == 0
        for i, r in enumerate(reqs):
            toks, word, _ = stack.poll(i)
            assert word == 1
            r.check(first[i][0] + toks, (which, graph, k, i))
        assert stack.stats()["captures"] == (1 if graph else 0)
        stack.end()
    finally:
        stack.graph(0)
        free(reqs)


# ------------------------------------------------------------------ both mask words and their edges

@pytest.mark.parametrize("n_slots,live,hit", [(128, [0, 1, 62, 63, 64, 65, 126, 127], [0, 63, 64, 127]), (65, [0, 63, 64], [64])])
def test_one_call_cancels_slots_of_both_mask_words(stack, n_slots, live, hit):
    rng = np.random.default_rng(19)
    reqs = {i: stack.req("small", rng, 1 + i % 3, 6) for i in live}
    try:
        stack.graph(1)
        assert stack.begin("small", n_slots, 128, 6) == 0
        for i, r in reqs.items():
            assert stack.admit(i, r) == 0
        assert stack.steps(2) == 0 and stack.cancel(hit) == 0
        st = stack.stats()
        for i in range(n_slots):
            want = DONE if i in hit else DECODE if i in live else FREE
            assert st["slots"][i][0] == want and stack.poll(i)[1] == (CANCELLED if i in hit else 0), i
        while not all(stack.wait_word(i) for i in live):
            assert stack.steps(2) == 0
        for i, r in reqs.items():
            toks, word, _ = stack.poll(i)
            if i in hit:
                assert (toks, word) == (r.solo()[:2], CANCELLED), i
            else:
                r.check(toks, i)
        assert stack.stats()["captures"] == 1
        stack.end()
    finally:
        stack.graph(0)
        free(list(reqs.values()))


# ------------------------------------------------------------------ the servers: preemption end to end, cancel from a callback

def serve_kw(stack, variant):
    """the server's constructor arguments of a variant (drafts: the n-gram lookup; model: a Q8 draft model -- the Q8 target itself, or
    the fp32 target's Q8 copy)"""
    import rama_amd
    _, m = stack.model("small")
    if variant == "cache":
        return dict(prefix_cache=2), None
    if variant == "drafts":
        return dict(n_draft=3, ngram=2, hint_cap=8), None
    if variant == "model":
        dm = m if stack.kind == "q8" else rama_amd.Q8Model.from_model(m)
        return dict(n_draft=3, draft=dm), (None if stack.kind == "q8" else dm)
    return {}, None


@pytest.mark.parametrize("variant", ["plain", "cache", "drafts", "model"])
def test_server_preempts_for_urgent_requests_and_every_result_is_the_solo_run(stack, variant):
    import rama_amd
    cfg, m = stack.model("small")
    rng = np.random.default_rng(23)
    longs = [stack.req("small", rng, 3, 10, *samp) for samp in [(0.0, 0.9, 0.0), (1.0, 0.9, 0.21), (0.0, 0.9, 0.0)]]
    shorts = [stack.req("small", rng, 2, 2, *samp) for samp in [(0.0, 0.9, 0.0), (1.0, 0.9, 0.66), (0.0, 0.9, 0.0)]]
    kw, made = serve_kw(stack, variant)
    cls = rama_amd.Q8Server if stack.kind == "q8" else rama_amd.Server
    stack.graph(1)
    srv = cls(m, 2, 6, 10, preempt=True, **kw)
    try:
        sub = lambda r, p: srv.submit(r.ctx, r.max_new, r.T, r.topp, r.u, priority=p, retain=variant == "cache")
        hs = {sub(r, 0): r for r in longs}
        seen, late = {}, []

        def on_token(h, i, t):
            seen.setdefault(h, []).append(i)
            if not late and i == 2:                                                # mid-run: the urgent ones arrive
                late.extend(sub(r, 5) for r in shorts)
                hs.update(zip(late, shorts))
        srv.run(on_token)
        st = srv.stats()
        assert st["preemptions"] >= 1 and st["graph_captures"] == 1 and len(late) == 3
        for h, r in hs.items():
            assert srv.finished(h) and not srv.cancelled(h) and srv.result(h) == r.solo(), (variant, h)
            assert seen[h] == list(range(r.max_new)), (variant, h)
    finally:
        srv.close()
        stack.graph(0)
        if made is not None:
            made.free()
        free(longs + shorts)


def test_server_cancel_from_a_callback_inside_run(stack):
    import rama_amd
    _, m = stack.model("small")
    rng = np.random.default_rng(29)
    reqs = [stack.req("small", rng, 3, 12), stack.req("small", rng, 2, 8, 1.0, 0.9, 0.4), stack.req("small", rng, 2, 5)]
    cls = rama_amd.Q8Server if stack.kind == "q8" else rama_amd.Server
    srv = cls(m, 2, 6, 12)      # (the steps to the first finish and the look-ahead, 10 in all, do not finish the first request)
    try:
        hs = [srv.submit(r.ctx, r.max_new, r.T, r.topp, r.u) for r in reqs]

        def on_token(h, i, t):
            if h == hs[0] and i == 3:
                srv.cancel(h)
        srv.run(on_token)
        got = srv.result(hs[0])
        assert srv.cancelled(hs[0]) and srv.finished(hs[0]) and 4 <= len(got) < 12 and got == reqs[0].solo()[:len(got)]
        for h, r in list(zip(hs, reqs))[1:]:
            assert srv.finished(h) and not srv.cancelled(h) and srv.result(h) == r.solo()
    finally:
        srv.close()
        free(reqs)


# ------------------------------------------------------------------ the drafting chains: a speculating slot cancelled and resumed, against the replays

HINT_CAP = 64
CANCEL_BEFORE, RESUME_BEFORE = 4, 6


class DReq:
    """a request of a drafting chain: context (BOS first), budget, sampler, n_draft K, ngram N and a hint made from its own solo run ("own":
    every granted draft is right; "corrupt": every third token is another), an engine and a twin for the solo run, and -- on a chain with a
    draft model -- a draft engine and its twin"""

    def __init__(self, stack, rng, n_ctx, max_new, samp, K, N=2, hint=None, dm=None):
        import rama_amd
        cfg, m = stack.model("small")
        Eng = rama_amd.Q8Engine if stack.kind == "q8" else rama_amd.Engine
        self.stack, self.cfg, self.max_new, self.K, self.N = stack, cfg, max_new, K, N
        self.T, self.topp, self.u = samp
        self.ctx = [1] + [int(t) for t in rng.integers(2, cfg.vocab_size, n_ctx - 1)]
        self.eng, self.twin = Eng(stack.dev, m), Eng(stack.dev, m)
        self.deng, self.dtwin = (rama_amd.Q8Engine(stack.dev, dm), rama_amd.Q8Engine(stack.dev, dm)) if dm is not None else (None, None)
        self.dcfg = dm.cfg if dm is not None else None
        for e, c in ((self.eng, cfg), (self.deng, self.dcfg)):
            if e is not None:
                for name in ("key_cache", "value_cache"):
                    e.set_buffer(name, np.full(c.n_layers * c.seq_len * c.dim, SENTINEL))
        self.solo = [int(t) for t in self.twin.generate(self.ctx[1:], n_ctx - 1 + max_new, self.T, self.topp, self.u)][n_ctx - 1:]
        text = self.ctx + self.solo
        self.hint = text if hint == "own" else [2 + (t - 1) % (cfg.vocab_size - 2) if i % 3 == 2 else t for i, t in enumerate(text)] if hint else []
        self._drafts = {}

    def draft_fn(self, prefix, n):
        """the draft model's own solo run behind a prefix, under the request's sampler"""
        key = (tuple(prefix), n)
        if key not in self._drafts:
            out = self.dtwin.generate(prefix[1:], len(prefix) - 1 + n, self.T, self.topp, self.u)
            self._drafts[key] = [int(t) for t in out][len(prefix) - 1:]
        return self._drafts[key]

    def spec(self, **over):
        return dict(dict(context=self.ctx, max_new=self.max_new, stop_token=None, n_draft=self.K, ngram=self.N, hint=self.hint, n_cached=0), **over)

    def admit(self, slot, ctx=None, n_cached=0, max_new=None):
        """the raw entry of the chain's kind; with a draft model, its rows of the whole context enqueued first (the entry's contract)"""
        from rama_amd._lib import rama_q8_serve_plan, rama_q8_serve_spec
        S_, ctx = self.stack, self.ctx if ctx is None else ctx
        p = rama_q8_serve_plan(self.T, self.topp, self.u, self.max_new if max_new is None else max_new, -1)
        arr = (C.c_int32 * len(ctx))(*ctx)
        if self.deng is not None:
            self.deng.prefill(ctx)
            return S_.entry("admit_model")(S_.dev.ctx, slot, C.byref(self.eng.state), C.byref(self.deng.state), arr, len(ctx), n_cached, C.byref(p), self.K)
        h = (C.c_int32 * max(len(self.hint), 1))(*self.hint)
        rec = rama_q8_serve_spec(self.K, self.N, h if self.hint else None, len(self.hint))
        return S_.entry("admit_spec")(S_.dev.ctx, slot, C.byref(self.eng.state), arr, len(ctx), n_cached, C.byref(p), C.byref(rec))

    def draft_rows_check(self, text, cursor, what):
        """the draft cache's rows below the draft cursor are a fresh draft prefill's of the same tokens"""
        assert 0 < cursor <= len(text), what
        self.dtwin.prefill(text[:cursor])
        for a, b in zip(self.stack.cache(self.deng, self.dcfg), self.stack.cache(self.dtwin, self.dcfg)):
            assert F.same_bits(a[:, :cursor], b[:, :cursor]), what

    def check(self, got, cursor, what):
        """the tokens; the target's rows below the final cursor are the solo run's; nothing from row n_context - 1 + max_new on is written;
        with a draft model the draft rows below the final draft cursor"""
        assert got == self.solo, what
        valid, untouched = len(self.ctx) + len(got) - 1, len(self.ctx) - 1 + self.max_new
        for a, b in zip(self.stack.cache(self.eng, self.cfg), self.stack.cache(self.twin, self.cfg)):
            assert F.same_bits(a[:, :valid], b[:, :valid]), what
            assert (a[:, untouched:] == SENTINEL).all(), what
        if self.deng is not None:
            self.draft_rows_check(self.ctx + got, cursor, what)
            for a in self.stack.cache(self.deng, self.dcfg):
                assert (a[:, untouched:] == SENTINEL).all(), what

    def free(self):
        for e in (self.eng, self.twin, self.deng, self.dtwin):
            if e is not None:
                e.free()


def chain_stats(stack, kind):
    """-> (<ABI>_stats, <ABI>_spec_stats, and on a chain with a draft model <ABI>_model_stats)"""
    from rama_amd._lib import rama_q8_serve_model_report, rama_q8_serve_spec_report
    from rama_amd.q8 import serve_model_report, serve_spec_report
    q = rama_q8_serve_spec_report()
    assert stack.entry("spec_stats")(stack.dev.ctx, C.byref(q)) == 0
    ms = None
    if kind == "model":
        r = rama_q8_serve_model_report()
        assert stack.entry("model_stats")(stack.dev.ctx, C.byref(r)) == 0
        ms = serve_model_report(r)
    return stack.stats(), serve_spec_report(q), ms


SPEC_COUNTERS = ("steps", "rows_decode", "rows_draft", "rows_prompt", "rows_idle", "drafts_wanted", "drafts_granted", "drafts_accepted",
                 "tokens_emitted", "accepted_hist")
MODEL_COUNTERS = ("draft_passes", "draft_rows_fed", "catch_up_rows")


@pytest.mark.parametrize("kind", ["spec", "model"])
@pytest.mark.parametrize("graph", [0, 1])
def test_a_speculating_slot_cancelled_and_resumed_equals_the_replay_step_by_step(stack, kind, graph):
    """3 slots at max_rows 8 on a chain begun with _begin_spec (hints) or _begin_model (a small synthetic draft model): slot 0 speculates
    (sampled, T 1, top-p 0.9; at most 3 tokens a step, so 4 steps leave it short of its budget of 12), slot 1 speculates beside it, slot 2 ingests a context longer than max_rows without drafts.  Slot 0 is cancelled
    before step 4 and admitted again before step 6 on its run state -- the old context plus its outputs, n_cached = its cursor, the budget left.
    After every step the device's row table, slot table, wants, grants, draft cursors and reports equal the replay with the same cancels."""
    import rama_amd
    from rama_amd.q8 import serve_model_replay, serve_spec_replay
    from tests.serve_model_f32_cases import SMALL_DRAFT, SMALL_GS, SMALL_SEED
    cfg, m = stack.model("small")
    dm = rama_amd.Q8Model.synth(stack.dev, rama_amd.Config(vocab_size=cfg.vocab_size, seq_len=cfg.seq_len, **SMALL_DRAFT), SMALL_GS, SMALL_SEED) \
        if kind == "model" else None
    rng = np.random.default_rng(31)
    reqs = [DReq(stack, rng, 3, 12, (1.0, 0.9, 0.37), 2, 2, "own", dm), DReq(stack, rng, 2, 10, (0.0, 0.9, 0.0), 4, 1, "corrupt", dm),
            DReq(stack, rng, 9, 3, (0.0, 0.9, 0.0), 0, dm=dm)]
    a = reqs[0]
    cancels = {CANCEL_BEFORE: [0]}

    def replay(specs, refs, fns):
        if kind == "model":
            return serve_model_replay(specs, refs, fns, 3, 8, cancels=cancels)
        return serve_spec_replay(specs, refs, 3, 8, cancels=cancels)
    try:
        first = replay([r.spec() for r in reqs], [r.solo for r in reqs], [r.draft_fn for r in reqs])
        state, _, cursor, n, _ = first["steps"][CANCEL_BEFORE - 1]["slots"][0]
        assert state == DECODE and 0 < n < a.max_new and first["cancelled_at"][0] == CANCEL_BEFORE       # a speculating slot, mid-run
        text = a.ctx + a.solo[:n]
        cont = a.spec(context=text, max_new=a.max_new - n, n_cached=min(cursor, len(text) - 1), after_step=RESUME_BEFORE)
        rp = replay([r.spec() for r in reqs] + [cont], [r.solo for r in reqs] + [a.solo[n:]], [r.draft_fn for r in reqs] + [a.draft_fn])
        assert rp["slot"] == [0, 1, 2, 0] and rp["outputs"][0] == a.solo[:n] and rp["steps"][RESUME_BEFORE]["admitted"] == [(0, 3)]
        stack.graph(graph)
        if kind == "model":
            assert stack.entry("begin_model")(stack.dev.ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(dm.ccfg), C.byref(dm.weights), 3, 8, 12, 15) == 0
        else:
            assert stack.entry("begin_spec")(stack.dev.ctx, C.byref(m.ccfg), C.byref(m.weights), 3, 8, 12, 15, HINT_CAP) == 0
        who, got, cur, cum = {}, {}, {}, dict(tokens_emitted=0, drafts_wanted=0, rows_draft=0)
        for k, st in enumerate(rp["steps"]):
            what = (kind, graph, k)
            if k in cancels:
                before = chain_stats(stack, kind)
                assert stack.cancel(cancels[k]) == 0
                s, ss, ms = chain_stats(stack, kind)
                assert s["slots"][0] == (DONE, 3, cursor, n, a.max_new) and s["slots"][1:] == before[0]["slots"][1:], what
                assert stack.poll(0)[:2] == (a.solo[:n], CANCELLED) and ss == before[1] and ms == before[2], what
                for x, y in zip(stack.cache(a.eng, cfg), stack.cache(a.twin, cfg)):       # target rows below the cursor: the solo run's
                    assert F.same_bits(x[:, :cursor], y[:, :cursor]), what
                if kind == "model":
                    a.draft_rows_check(text, ms["draft_cursor"][0], what)
            assert st["cancelled"] == ([0] if k in cancels else []), what
            for slot, q in st["admitted"]:
                if q == 3:                                    # the continuation, over the device's own tokens and cursor
                    toks, word, _ = stack.poll(0)
                    dev_cursor = stack.stats()["slots"][0][2]
                    assert word == CANCELLED and (a.ctx + toks, min(dev_cursor, len(text) - 1)) == (cont["context"], cont["n_cached"]), what
                    assert a.admit(0, a.ctx + toks, min(dev_cursor, len(text) - 1), a.max_new - len(toks)) == 0, what
                else:
                    assert reqs[q].admit(slot) == 0, what
                who[slot] = q
            assert stack.steps(1) == 0
            s, ss, ms = chain_stats(stack, kind)
            assert s["rows"] == st["rows"] and s["slots"] == st["slots"], what
            assert (ss["last_want"], ss["last_granted"]) == (st["want"], st["granted"]), what
            cum["tokens_emitted"] += sum(st["emitted"].values())
            cum["drafts_wanted"] += sum(st["want"])
            cum["rows_draft"] += sum(st["granted"])
            assert ss["steps"] == k + 1 and {c: ss[c] for c in cum} == cum, what
            if kind == "model":
                assert [ms["draft_cursor"][i] for i in who] == [st["cursors"][i] for i in who], what
            for slot in st["finished"]:
                toks, word, _ = stack.poll(slot)
                assert word == 1, what
                got[who[slot]], cur[who[slot]] = toks, ms["draft_cursor"][slot] if ms else None
        s, ss, ms = chain_stats(stack, kind)
        assert {c: ss[c] for c in SPEC_COUNTERS} == {c: rp["counters"][c] for c in SPEC_COUNTERS}
        if kind == "model":
            assert {c: ms[c] for c in MODEL_COUNTERS} == {c: rp["counters"][c] for c in MODEL_COUNTERS}
            assert [cur[q] for q in (1, 2, 3)] == [rp["cursor"][q] for q in (1, 2, 3)]
        assert s["captures"] == (1 if graph else 0) and sorted(got) == [1, 2, 3]
        assert [got[q] for q in (1, 2, 3)] == [rp["outputs"][q] for q in (1, 2, 3)]
        a.check(a.solo[:n] + got[3], cur[3], (kind, graph, "resumed"))
        reqs[1].check(got[1], cur[1], (kind, graph, 1))
        reqs[2].check(got[2], cur[2], (kind, graph, 2))
        stack.end()
    finally:
        stack.graph(0)
        stack.entry("end")(stack.dev.ctx)
        free(reqs)
        if dm is not None:
            dm.free()
