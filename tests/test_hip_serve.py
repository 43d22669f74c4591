"""The serving chain in parity mode on the GPU (rama_serve_begin / _admit / _steps / _poll / _tokens / _stats, rama_amd.Server): continuous
batching for an fp32 model.  Every admitted sequence's tokens and cache rows are bit for bit those of parity-mode Engine.generate run on it
alone -- the oracle's --, whatever the chunking of its context, its neighbours, max_rows, the tile a row lands in and the graph mode; the
device's row table is the host plan's; an idle tile is never touched; refusals leave the chain as it was.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from oracle import synth as S
from tests import serve_cases as W
from tests.helpers import to_rama_cfg
from tests.serve_cases import DECODE, DONE, FREE, PROMPT, TILE

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -2
SENTINEL = np.float32(123.25)
SEED = 23


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    from rama_amd._lib import check
    d = rama_amd.Hip(0)
    check(d.lib.rama_set_tuning(d.ctx, b"ref_order", 1))
    yield d
    d.lib.rama_serve_end(d.ctx)
    d.lib.rama_set_graph_mode(d.ctx, 0)
    check(d.lib.rama_set_tuning(d.ctx, b"ref_order", 0))
    d.close()


@pytest.fixture(scope="module")
def models(dev):
    """name -> (oracle config, Model), made on first use"""
    import rama_amd
    made = {}

    def get(name):
        if name not in made:
            cfg = getattr(W, name)
            made[name] = (cfg, rama_amd.Model.synth(dev, to_rama_cfg(cfg), SEED, rope=S.rope_tables(cfg.seq_len, cfg.head_size)))
        return made[name]
    yield get
    dev.lib.rama_serve_end(dev.ctx)
    for _, m in made.values():
        m.free()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def cache(eng, cfg):
    n = cfg.n_layers * cfg.seq_len * cfg.dim
    return (eng.buffer("key_cache", n).reshape(cfg.n_layers, cfg.seq_len, cfg.dim),
            eng.buffer("value_cache", n).reshape(cfg.n_layers, cfg.seq_len, cfg.dim))


class Req:
    """a sequence to admit: its context (BOS first), its plan, its engine, and a twin for the solo run"""

    def __init__(self, dev, cfg, m, rng, n_ctx, max_new, T=0.0, topp=0.9, u=0.0, stop=-1):
        import rama_amd
        self.cfg, self.m = cfg, m
        self.ctx = [1] + [int(t) for t in rng.integers(2, cfg.vocab_size, n_ctx - 1)]
        self.max_new, self.T, self.topp, self.u, self.stop = max_new, T, topp, u, stop
        self.eng, self.twin = rama_amd.Engine(dev, m), rama_amd.Engine(dev, m)
        for name in ("key_cache", "value_cache"):
            self.eng.set_buffer(name, np.full(cfg.n_layers * cfg.seq_len * cfg.dim, SENTINEL))
        self._solo = None

    def solo(self):
        """the max_new tokens parity-mode Engine.generate gives this sequence alone (no stop)"""
        if self._solo is None:
            n = len(self.ctx)
            self._solo = [int(t) for t in self.twin.generate(self.ctx[1:], n - 1 + self.max_new, self.T, self.topp, self.u)][n - 1:]
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

    def check(self, got, what, rows=None):
        """tokens, cache rows 0..last (all of them, or the given ones), and the sentinel behind last"""
        assert got == self.want(), what
        last = len(self.ctx) + len(got) - 2                   # the last token recorded is not fed
        for a, b in zip(cache(self.eng, self.cfg), cache(self.twin, self.cfg)):
            pick = list(range(last + 1)) if rows is None else [r for r in rows if r <= last]
            assert same_bits(a[:, pick], b[:, pick]), what
            assert (a[:, last + 1:] == SENTINEL).all(), what

    def free(self):
        self.eng.free(); self.twin.free()


def begin(dev, m, n_slots, max_rows, cap):
    return dev.lib.rama_serve_begin(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), n_slots, max_rows, cap)


def admit(dev, slot, r, plan=None):
    p = r.plan() if plan is None else plan
    return dev.lib.rama_serve_admit(dev.ctx, slot, C.byref(r.eng.state), (C.c_int32 * len(r.ctx))(*r.ctx), len(r.ctx), C.byref(p))


def steps(dev, n):
    return dev.lib.rama_serve_steps(dev.ctx, n)


def poll(dev, slot, frm=0, cap=512):
    buf = (C.c_int32 * cap)()
    k, fin, gen = C.c_int(), C.c_int(-7), C.c_int(-7)
    assert dev.lib.rama_serve_poll(dev.ctx, slot, frm, buf, cap, C.byref(k), C.byref(fin), C.byref(gen)) == 0
    return [int(buf[i]) for i in range(k.value)], bool(fin.value), gen.value


def tokens(dev, slot, cap=512):
    buf = (C.c_int32 * cap)()
    k = C.c_int()
    assert dev.lib.rama_serve_tokens(dev.ctx, slot, buf, cap, C.byref(k)) == 0
    return [int(buf[i]) for i in range(k.value)]


def stats(dev):
    from rama_amd._lib import rama_q8_serve_report
    r = rama_q8_serve_report()
    assert dev.lib.rama_serve_stats(dev.ctx, C.byref(r)) == 0
    return dict(steps=int(r.steps), captures=int(r.graph_captures), decode=int(r.rows_decode), prompt=int(r.rows_prompt), idle=int(r.rows_idle),
                rows=[(x.slot, x.pos, x.logits) for x in r.last_rows[:r.max_rows]],
                slots=[(s.state, s.n_context, s.cursor, s.n_out, s.max_new) for s in r.slots[:r.n_slots]])


def plan_step(slots, max_rows):
    from rama_amd.q8 import serve_plan_step
    return serve_plan_step(slots, max_rows)


SAMPLERS = [(0.0, 0.9, 0.0), (1.0, 0.9, 0.1), (0.7, 0.5, 0.6), (0.0, 0.9, 0.0), (1.0, 0.95, 0.83)]


def requests(dev, cfg, m, rng, sizes, stops=False):
    """greedy and sampled plans in turn; with stops every third request stops on a token of its own solo run"""
    reqs = []
    for i, (n_ctx, new) in enumerate(sizes):
        T, P, U = SAMPLERS[i % len(SAMPLERS)]
        r = Req(dev, cfg, m, rng, n_ctx, new, T, P, U)
        if stops and i % 3 == 1 and new >= 3:
            r.stop = r.solo()[new // 2]
        reqs.append(r)
    return reqs


def run_all(dev, reqs, bound=400):
    """slot i serves reqs[i]: one step at a time until every slot is DONE -> the steps taken"""
    for k in range(bound):
        if all(poll(dev, i)[1] for i in range(len(reqs))):
            return k
        assert steps(dev, 1) == 0
        assert dev.lib.rama_sync(dev.ctx) == 0
    raise AssertionError("the chain did not finish")


def oracle_tokens(cfg, r):
    """generate() of the reference on the CPU oracle: forced context, then Device::sample with the plan's (T, topp, u)"""
    orc = O.Oracle(cfg, S.synth_weights(cfg, SEED, rope=S.rope_tables(cfg.seq_len, cfg.head_size)))
    out, tok = [], r.ctx[0]
    for pos in range(len(r.ctx) - 1 + r.max_new):
        lg = orc.forward(tok, pos)
        if pos + 1 < len(r.ctx):
            tok = r.ctx[pos + 1]
        else:
            tok = int(O.argmax(lg)) if r.T == 0.0 else int(O.sample(lg.copy(), r.T, r.topp, r.u))
            out.append(tok)
    return out


# ------------------------------------------------------------------ solo requests, tile boundaries

@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name", ["TINY", "STORIES15M"])
def test_solo_requests_are_the_solo_run_and_the_oracle(dev, models, name, graph):
    cfg, m = models(name)
    rng = np.random.default_rng(5)
    dev.lib.rama_set_graph_mode(dev.ctx, int(graph))
    try:
        for n_ctx, (T, P, U) in [(1, SAMPLERS[0]), (5, SAMPLERS[1]), (40, SAMPLERS[2]), (40, SAMPLERS[0])]:
            r = Req(dev, cfg, m, rng, n_ctx, 5, T, P, U)
            assert begin(dev, m, 1, 8, 8) == 0
            assert admit(dev, 0, r) == 0
            run_all(dev, [r])
            r.check(tokens(dev, 0), f"{name} context {n_ctx} T {T}")
            assert poll(dev, 0)[0] == r.want()
            if name == "TINY":
                assert r.want() == oracle_tokens(cfg, r), f"oracle: context {n_ctx} T {T}"
            if graph:
                assert stats(dev)["captures"] == 1
            r.free()
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


@pytest.mark.parametrize("max_rows", [8, 32, 64])
def test_a_context_across_the_tile_boundary(dev, models, max_rows):
    """40 context tokens at max_rows 8, 32 and 64 (there one step takes them, rows 31 and 32 both its own), and the straddling pair"""
    cfg, m = models("TINY")
    rng = np.random.default_rng(6)
    r = Req(dev, cfg, m, rng, 40, 4, *SAMPLERS[1])
    assert begin(dev, m, 1, max_rows, 8) == 0
    assert admit(dev, 0, r) == 0
    assert steps(dev, 1) == 0
    if max_rows == 64:
        rows = stats(dev)["rows"]
        assert [x[0] for x in rows[:40]] == [0] * 40 and rows[TILE - 1][1] == TILE - 1 and rows[TILE][1] == TILE and rows[40] == (-1, -1, 0)
    run_all(dev, [r])
    r.check(tokens(dev, 0), f"max_rows {max_rows}")
    r.free()
    if max_rows == 64:
        reqs = requests(dev, cfg, m, rng, W.STRADDLE["sizes"])
        assert begin(dev, m, 2, 64, 8) == 0
        for i, q in enumerate(reqs):
            assert admit(dev, i, q) == 0
        assert steps(dev, 1) == 0
        rows = stats(dev)["rows"]
        assert rows[TILE - 1][0] == rows[TILE][0] == 1
        run_all(dev, reqs)
        for i, q in enumerate(reqs):
            q.check(tokens(dev, i), f"straddling pair, slot {i}")
            q.free()


def test_row_table_is_the_host_plan_around_free_holes(dev, models):
    """33 slots at 64 rows, FREE holes at slots 0, 31 and 32: the device's tables step by step against rama_q8_serve_plan_step applied to the
    device's own previous slot table; then two idle steps move nothing"""
    cfg, m = models("TINY")
    w = W.HOLES
    rng = np.random.default_rng(7)
    reqs = requests(dev, cfg, m, rng, w["sizes"])
    assert begin(dev, m, w["n_slots"], w["max_rows"], 8) == 0
    live = [i for i in range(w["n_slots"]) if i not in w["holes"]]
    for i, r in zip(live, reqs):
        assert admit(dev, i, r) == 0
    before = stats(dev)
    assert before["slots"] == W.admitted(w["sizes"], w["n_slots"], w["holes"])
    for k in range(200):
        if not any(s[0] in (PROMPT, DECODE) for s in before["slots"]):
            break
        rows, after = plan_step(before["slots"], w["max_rows"])
        assert steps(dev, 1) == 0
        now = stats(dev)
        assert now["rows"] == rows and now["slots"] == after, f"step {k}"
        used, dec = sum(1 for x in rows if x[0] >= 0), sum(1 for x in rows if x[0] >= 0 and before["slots"][x[0]][0] == DECODE)
        assert (now["steps"], now["decode"], now["prompt"], now["idle"]) == (
            before["steps"] + 1, before["decode"] + dec, before["prompt"] + used - dec, before["idle"] + w["max_rows"] - used)
        before = now
    for i, r in zip(live, reqs):
        r.check(tokens(dev, i), f"slot {i}")
    caches = [cache(r.eng, cfg) for r in reqs]
    assert steps(dev, 2) == 0
    now = stats(dev)
    assert now["slots"] == before["slots"] and (now["decode"], now["prompt"]) == (before["decode"], before["prompt"])
    assert (now["steps"], now["idle"]) == (before["steps"] + 2, before["idle"] + 2 * w["max_rows"])
    assert all(x == (-1, -1, 0) for x in now["rows"])
    for r, (k0, v0) in zip(reqs, caches):
        k1, v1 = cache(r.eng, cfg)
        assert same_bits(k0, k1) and same_bits(v0, v1)
    for r in reqs:
        r.free()


# ------------------------------------------------------------------ the idle tile

def pass_rows(dev, cfg):
    """the pass's five row buffers (X, XN, Q, XB, HB): device addresses and widths"""
    bufs = (C.POINTER(C.c_float) * 5)()
    n = C.c_int()
    dev.lib.rama_internal_serve_scratch.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_float) * 5), C.POINTER(C.c_int)]
    assert dev.lib.rama_internal_serve_scratch(dev.ctx, C.byref(bufs), C.byref(n)) == 0
    return [(C.cast(bufs[i], C.c_void_p).value, cfg.hidden_dim if i == 4 else cfg.dim) for i in range(5)], n.value


@pytest.mark.parametrize("graph", [False, True])
def test_an_idle_tile_is_never_touched(dev, models, graph):
    """max_rows 64 with at most 8 wanted rows: tokens and cache rows are the max_rows 32 run's (and the solo run's), and the pass's rows of
    tile 1, filled with a sentinel before every step, still hold it afterwards"""
    cfg, m = models("TINY")
    w = W.IDLE_TILE
    got = {}
    dev.lib.rama_set_graph_mode(dev.ctx, int(graph))
    try:
        for max_rows in (w["narrow_rows"], w["max_rows"]):
            rng = np.random.default_rng(8)
            reqs = requests(dev, cfg, m, rng, w["sizes"])
            assert begin(dev, m, w["n_slots"], max_rows, 8) == 0
            for i, r in enumerate(reqs):
                assert admit(dev, i, r) == 0
            bufs, n_rows = pass_rows(dev, cfg)
            assert n_rows == max_rows
            for k in range(100):
                if all(poll(dev, i)[1] for i in range(len(reqs))):
                    break
                if max_rows > TILE:
                    for base, width in bufs:
                        fill = np.full((max_rows - TILE) * width, SENTINEL)
                        assert dev.lib.rama_copy_h2d_f32(dev.ctx, C.c_void_p(base + 4 * TILE * width), fill.ctypes.data, fill.size) == 0
                assert steps(dev, 1) == 0
                assert dev.lib.rama_sync(dev.ctx) == 0
                assert all(x == (-1, -1, 0) for x in stats(dev)["rows"][8:])
                if max_rows > TILE:
                    for base, width in bufs:
                        back = np.empty((max_rows - TILE) * width, np.float32)
                        assert dev.lib.rama_download_f32(dev.ctx, C.c_void_p(base + 4 * TILE * width), back.size, back.ctypes.data) == 0
                        assert (back == SENTINEL).all(), f"step {k}: the idle tile's rows were written"
            for i, r in enumerate(reqs):
                r.check(tokens(dev, i), f"max_rows {max_rows} slot {i}")
            got[max_rows] = [(tokens(dev, i), cache(r.eng, cfg)) for i, r in enumerate(reqs)]
            if graph:
                assert stats(dev)["captures"] == 1
            for r in reqs:
                r.free()
        for (ta, (ka, va)), (tb, (kb, vb)) in zip(got[w["narrow_rows"]], got[w["max_rows"]]):
            assert ta == tb and same_bits(ka, kb) and same_bits(va, vb)
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


# ------------------------------------------------------------------ slot reuse, the 7B shape

@pytest.mark.parametrize("max_rows", [8, 32])
def test_fourteen_requests_through_four_reused_slots(dev, models, max_rows):
    """greedy, sampled and stop-token plans in turn; every admission goes into a just-finished slot behind a block of steps; one slot goes
    from PROMPT to DONE without being DECODE.  (That an admission lands while steps are still RUNNING is the next test's.)"""
    cfg, m = models("TINY")
    w = W.REUSE
    rng = np.random.default_rng(9)
    reqs = requests(dev, cfg, m, rng, w["sizes"], stops=True)
    dev.lib.rama_set_graph_mode(dev.ctx, 1)
    try:
        for r in reqs:
            r.want()                                        # (the solo runs first: an fp32 entry that sizes scratch drops every captured graph of the context)
        assert begin(dev, m, w["n_slots"], max_rows, 8) == 0
        waiting, serving, served = list(range(len(reqs))), [None] * w["n_slots"], 0
        prompt_to_done = 0
        for _ in range(400):
            for slot in range(w["n_slots"]):
                if serving[slot] is not None and poll(dev, slot)[1]:
                    i = serving[slot]
                    got = poll(dev, slot)[0]
                    if len(reqs[i].ctx) > 1 and reqs[i].max_new == 1:
                        prompt_to_done += 1
                    assert got == reqs[i].want(), f"request {i}"
                    serving[slot], served = None, served + 1
                if serving[slot] is None and waiting:
                    i = waiting.pop(0)
                    assert admit(dev, slot, reqs[i]) == 0
                    serving[slot] = i
            if served == len(reqs):
                break
            assert steps(dev, 3) == 0                       # a block: finishes fall inside it, the admission goes in behind what is left of it
            while dev.lib.rama_stream_query(dev.ctx) == 1 and not any(s is not None and poll(dev, k)[1] for k, s in enumerate(serving)):
                pass                                        # (until a finished word shows or the block has run: no sleep, no synchronisation)
        assert served == len(reqs) and prompt_to_done >= 1
        assert dev.lib.rama_sync(dev.ctx) == 0
        assert stats(dev)["captures"] == 1
        for r in reqs:
            last = len(r.ctx) + len(r.want()) - 2
            for a, b in zip(cache(r.eng, cfg), cache(r.twin, cfg)):
                assert same_bits(a[:, :last + 1], b[:, :last + 1]) and (a[:, last + 1:] == SENTINEL).all()
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        for r in reqs:
            r.free()


def test_admission_into_a_finished_slot_while_a_block_is_in_flight(dev, models):
    """all slots busy on the stories15M shape; ONE block of steps that runs well past the first finish by the host plan is enqueued at once; the
    finished word is watched by rama_serve_poll alone (no stream query, no synchronising call); the newcomer is admitted while the rest of
    the block is still running -- asserted --, and more steps go in behind it"""
    import time
    cfg, m = models("STORIES15M")
    n_slots, max_rows, sizes = 4, 8, [(1, 9), (3, 6), (21, 12), (6, 40)]
    rng = np.random.default_rng(14)
    reqs = requests(dev, cfg, m, rng, sizes)
    late = Req(dev, cfg, m, rng, 21, 5, 1.0, 0.9, 0.37)
    dev.lib.rama_set_graph_mode(dev.ctx, 1)
    try:
        for r in reqs + [late]:
            r.want()
        assert begin(dev, m, n_slots, max_rows, 40) == 0
        for i, r in enumerate(reqs):
            assert admit(dev, i, r) == 0
        assert admit(dev, 0, late) == EINVAL                      # every slot is busy
        t, first_at = W.admitted(sizes, n_slots), 0
        while not any(x[0] == DONE for x in t):
            _, t = plan_step(t, max_rows)
            first_at += 1
        assert steps(dev, first_at + 30) == 0                     # one block, asynchronous: 30 steps past the first finish
        first, deadline = None, time.time() + 60
        while first is None and time.time() < deadline:
            for i in range(n_slots):
                if poll(dev, i, 0, 1)[1]:
                    first = i
                    break
        assert first is not None
        old_tokens, _, gen0 = poll(dev, first)
        assert admit(dev, first, late) == 0                       # ... behind whatever of the block is still running
        assert steps(dev, 4) == 0
        in_flight = dev.lib.rama_stream_query(dev.ctx) == 1
        after_admit = poll(dev, first)
        assert after_admit[2] == gen0 + 1
        assert after_admit[0] == late.want()[:len(after_admit[0])]    # the ring row holds the newcomer's tokens only
        assert steps(dev, sum(len(r.ctx) + r.max_new for r in reqs + [late])) == 0
        assert in_flight, "the admission was meant to happen with steps still running"
        for i, r in enumerate(reqs):
            if i != first:
                r.check(tokens(dev, i), f"slot {i}")
        late.check(tokens(dev, first), "the newcomer")
        reqs[first].check(old_tokens, "the old occupant")
        assert stats(dev)["captures"] == 1
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        for r in reqs + [late]:
            r.free()


def test_7b_shape_a_long_context_next_to_two_decoding_slots(dev, models):
    cfg, m = models("L1_7B")
    w = W.LONG_7B
    rng = np.random.default_rng(10)
    reqs = requests(dev, cfg, m, rng, w["sizes"])
    reqs[2].T = 0.0
    dev.lib.rama_set_graph_mode(dev.ctx, 1)
    try:
        for r in reqs:
            r.want()
        assert begin(dev, m, w["n_slots"], w["max_rows"], 64) == 0
        for i in (0, 1):
            assert admit(dev, i, reqs[i]) == 0
        assert steps(dev, 4) == 0                           # both are decoding when the long context arrives
        assert admit(dev, 2, reqs[2]) == 0
        run_all(dev, reqs)
        n = len(reqs[2].ctx)
        for i, r in enumerate(reqs):
            r.check(tokens(dev, i), f"slot {i}", rows=[0, 1, 1022, 1023, 1024, 1025, n - 2, n - 1, n] if i == 2 else None)
        assert stats(dev)["captures"] == 1
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        for r in reqs:
            r.free()


# ------------------------------------------------------------------ refusals, both chains, the Python server

def test_refusals_leave_the_running_chain_as_it_was(dev, models):
    from rama_amd._lib import check, rama_q8_serve_plan
    cfg, m = models("TINY")
    rng = np.random.default_rng(11)
    r, other = Req(dev, cfg, m, rng, 6, 6, *SAMPLERS[1]), Req(dev, cfg, m, rng, 3, 2)
    assert begin(dev, m, 2, 8, 8) == 0
    assert admit(dev, 0, r) == 0
    assert steps(dev, 2) == 0
    L, ctx = dev.lib, dev.ctx
    for mode in (0, 2, 3):                                   # fast mode, tolerance mode, bar mode
        check(L.rama_set_tuning(ctx, b"ref_order", mode))
        try:
            assert begin(dev, m, 2, 8, 8) == EUNSUP
            assert steps(dev, 1) == EUNSUP
        finally:
            check(L.rama_set_tuning(ctx, b"ref_order", 1))
    check(L.rama_set_tuning(ctx, b"prefill_chain", 0))      # no chain-order token batch: the weights are not taken
    try:
        assert begin(dev, m, 2, 8, 8) == EUNSUP
    finally:
        check(L.rama_set_tuning(ctx, b"prefill_chain", 1))
    import rama_amd
    for bad in (O.Config(72, 176, 1, 4, 4, 320, 32, False), O.Config(64, 168, 1, 4, 4, 320, 32, False)):      # dim, hidden_dim no multiple of 16
        mo = rama_amd.Model.synth(dev, to_rama_cfg(bad), SEED, rope=S.rope_tables(bad.seq_len, bad.head_size))
        assert begin(dev, mo, 2, 8, 8) == EUNSUP
        mo.free()
    assert begin(dev, m, 3, 2, 8) == EINVAL                 # n_slots > max_rows
    assert begin(dev, m, 0, 8, 8) == EINVAL and begin(dev, m, 2, 129, 8) == EINVAL and begin(dev, m, 2, 8, cfg.seq_len) == EINVAL
    assert admit(dev, 0, other) == EINVAL                   # busy
    assert admit(dev, 2, other) == EINVAL                   # no such slot
    assert admit(dev, 1, r) == EINVAL                       # the run state is already in a live slot
    assert admit(dev, 1, other, rama_q8_serve_plan(0.0, 0.9, 0.0, 9, -1)) == EINVAL          # max_new beyond max_new_cap
    assert admit(dev, 1, other, rama_q8_serve_plan(-1.0, 0.9, 0.0, 2, -1)) == EINVAL
    assert admit(dev, 1, other, rama_q8_serve_plan(0.0, 0.9, 0.0, 2, cfg.vocab_size)) == EINVAL
    assert stats(dev)["slots"][1][0] == FREE
    run_all(dev, [r])
    r.check(tokens(dev, 0), "after the refusals")
    # a sampled plan on a vocabulary beyond 32768
    big = O.Config(64, 176, 1, 4, 4, 32772, 32, False)
    mb = rama_amd.Model.synth(dev, to_rama_cfg(big), SEED, rope=S.rope_tables(big.seq_len, big.head_size))
    rb = Req(dev, big, mb, rng, 2, 2, 1.0, 0.9, 0.5)
    assert begin(dev, mb, 1, 4, 4) == 0
    assert admit(dev, 0, rb) == EUNSUP
    rb.T = 0.0
    assert admit(dev, 0, rb) == 0
    run_all(dev, [rb])
    rb.check(tokens(dev, 0), "greedy on the large vocabulary")
    assert L.rama_serve_end(ctx) == 0
    # rama_state_free of an occupied slot's run state ends the chain; a finished occupant's does not
    assert begin(dev, m, 2, 8, 8) == 0
    a, b = Req(dev, cfg, m, rng, 2, 1), Req(dev, cfg, m, rng, 2, 6)
    assert admit(dev, 0, a) == 0 and admit(dev, 1, b) == 0
    assert steps(dev, 2) == 0 and L.rama_sync(ctx) == 0
    a.eng.free()                                             # DONE as the host can see it
    assert steps(dev, 1) == 0
    b.eng.free()
    assert steps(dev, 1) == EINVAL and admit(dev, 0, other) == EINVAL
    assert L.rama_serve_end(ctx) == 0
    a.twin.free(); b.twin.free(); rb.free(); mb.free(); r.free(); other.free()


def test_model_free_ends_a_live_chain_and_a_context_goes_with_its_chains_begun(dev):
    """rama_model_free under a live chain with a captured step: what the chain produced stays the solo run's and readable, _steps and _admit
    refuse.  Then a context of its own is destroyed with a serving chain and a chained batch both still begun (no rama_serve_end; the
    chained batch has no end entry) after each has produced its solo / oracle tokens."""
    import rama_amd
    from rama_amd._lib import check
    cfg = W.TINY
    rope = S.rope_tables(cfg.seq_len, cfg.head_size)
    d = rama_amd.Hip(0)
    L = d.lib
    check(L.rama_set_tuning(d.ctx, b"ref_order", 1))
    L.rama_set_graph_mode(d.ctx, 1)
    m1, m2 = (rama_amd.Model.synth(d, to_rama_cfg(cfg), SEED, rope=rope) for _ in range(2))
    rng = np.random.default_rng(14)
    r, late = Req(d, cfg, m1, rng, 3, 6), Req(d, cfg, m1, rng, 2, 2)
    want = r.want()
    assert begin(d, m1, 2, 8, 8) == 0 and admit(d, 0, r) == 0
    assert steps(d, 3) == 0 and L.rama_sync(d.ctx) == 0
    got, fin, _ = poll(d, 0)
    assert got and got == want[:len(got)] and not fin
    m1.free()                                                # the chain's model goes: the chain is dead
    assert steps(d, 1) == EINVAL and admit(d, 1, late) == EINVAL
    assert tokens(d, 0) == got
    r.free(); late.free()
    # a chain over the second model (it takes the dead one's place) and, in fast mode, a chained batch
    q = Req(d, cfg, m2, rng, 3, 4)
    assert begin(d, m2, 2, 8, 8) == 0 and admit(d, 0, q) == 0
    run_all(d, [q])
    q.check(tokens(d, 0), "the chain begun after the first model went")
    check(L.rama_set_tuning(d.ctx, b"ref_order", 0))
    pair = [rama_amd.Engine(d, m2), rama_amd.Engine(d, m2)]
    batch = rama_amd.decode_batch_chained(pair, [3, 7], [0, 0], 6)
    w = S.synth_weights(cfg, SEED, rope=rope)
    for i, t in enumerate((3, 7)):
        orc, greedy = O.Oracle(cfg, w), []
        for p in range(6):
            t = O.argmax(orc.forward(t, p)); greedy.append(t)
        assert batch[i] == greedy, i
    assert L.rama_ctx_destroy(d.ctx) == 0                    # both chains begun, the serving chain live with its step captured
    d.ctx = None
    # the run states and the model outlive their context: freed through the module's
    for e in (q.eng, q.twin, *pair):
        assert dev.lib.rama_state_free(dev.ctx, C.byref(e.state)) == 0
    assert dev.lib.rama_model_free(dev.ctx, m2.handle) == 0
    m2.handle = None


def test_a_q8_chain_and_the_fp32_chain_on_one_context(dev, models, golden_dir):
    """their steps interleaved; both end with their solo tokens, each with one captured step"""
    import rama_amd
    from rama_amd._lib import rama_q8_serve_plan, rama_q8_serve_report
    cfg, m = models("TINY")
    rng = np.random.default_rng(12)
    reqs = requests(dev, cfg, m, rng, [(5, 6), (11, 4)])
    qm = rama_amd.Q8Model.load(dev, golden_dir / "ckpt_v2_q80_tied.bin")
    qe, qt = rama_amd.Q8Engine(dev, qm), rama_amd.Q8Engine(dev, qm)
    qctx = [1] + [int(t) for t in rng.integers(2, qm.cfg.vocab_size, 4)]
    qwant = [int(t) for t in qt.generate(qctx[1:], len(qctx) - 1 + 6, 0.0, 0.9, 0.0)][len(qctx) - 1:]
    L, ctx = dev.lib, dev.ctx
    L.rama_set_graph_mode(ctx, 1)
    try:
        for r in reqs:
            r.want()
        assert L.rama_q8_serve_begin(ctx, C.byref(qm.ccfg), C.byref(qm.weights), 1, 4, 8) == 0
        assert begin(dev, m, 2, 8, 8) == 0
        plan = rama_q8_serve_plan(0.0, 0.9, 0.0, 6, -1)
        assert L.rama_q8_serve_admit(ctx, 0, C.byref(qe.state), (C.c_int32 * len(qctx))(*qctx), len(qctx), C.byref(plan)) == 0
        for i, r in enumerate(reqs):
            assert admit(dev, i, r) == 0
        for _ in range(12):
            assert steps(dev, 1) == 0
            assert L.rama_q8_serve_steps(ctx, 1) == 0
        assert L.rama_sync(ctx) == 0
        for i, r in enumerate(reqs):
            r.check(tokens(dev, i), f"fp32 slot {i}")
        buf, k = (C.c_int32 * 16)(), C.c_int()
        assert L.rama_q8_serve_tokens(ctx, 0, buf, 16, C.byref(k)) == 0
        assert [int(buf[i]) for i in range(k.value)] == qwant
        q = rama_q8_serve_report()
        assert L.rama_q8_serve_stats(ctx, C.byref(q)) == 0
        assert int(q.graph_captures) == 1 and stats(dev)["captures"] == 1
    finally:
        L.rama_set_graph_mode(ctx, 0)
        L.rama_q8_serve_end(ctx)
        L.rama_serve_end(ctx)
        for r in reqs:
            r.free()
        qe.free(); qt.free(); qm.free()


def test_server_serves_twelve_requests_over_four_slots(dev, models):
    import rama_amd
    cfg, m = models("STORIES15M")
    w = W.SERVER
    rng = np.random.default_rng(13)
    reqs = requests(dev, cfg, m, rng, w["sizes"], stops=True)
    srv = rama_amd.Server(m, w["n_slots"], max_rows=32, max_new_cap=8)
    try:
        hs = [srv.submit(r.ctx, r.max_new, r.T, r.topp, r.u, None if r.stop < 0 else r.stop) for r in reqs]
        srv.run()
        for h, r in zip(hs, reqs):
            assert srv.finished(h) and srv.result(h) == r.want(), f"request {h}"
        st = srv.stats()
        assert st["steps"] >= srv.planned["steps"] > 0
    finally:
        srv.close()
        for r in reqs:
            r.free()
