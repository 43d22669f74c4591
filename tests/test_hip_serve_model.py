"""The parity-mode serving chain with a Q8 draft model on the GPU (rama_serve_begin_model / _admit_model / _model_stats, Server(draft=...)).
Whatever the draft model, n_draft, the samplers, the neighbours, max_rows, the tile a row lands in and the graph mode, every request's
tokens are bit for bit parity-mode Engine.generate's on a twin engine and its cache rows below its final cursor the twin's; the draft
cache's rows below the final draft cursor are a fresh rama_q8_prefill's; nothing from row n_context - 1 + max_new on is written in either
cache; after every step the device's row table, slot table, wants, grants and draft cursors equal serve_model_replay's.  Every comparison
is exact.  The cases: tests/serve_model_f32_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import serve_model_f32_cases as W
from tests.helpers import GOLDEN, load_case, to_rama_cfg
from tests.serve_model_cases import ARRIVALS_SHORT, FREE
from tests.test_hip_q8_serve import cache, fill_all
from tests.test_hip_q8_serve_model import MODEL_COUNTERS
from tests.test_hip_serve import EINVAL, EUNSUP, SENTINEL, dev, models, poll, same_bits, stats, steps, tokens  # noqa: F401
from tests.test_hip_serve_spec import COUNTERS, fork, logits_rows, prefill, set_graph, spec_stats

pytestmark = pytest.mark.gpu

TILE = W.TILE


class Pair:
    """an fp32 target and its Q8 drafts, made on first use: "self" = Q8Model.from_model(target), "small" = an unrelated synthetic Q8 model
    of a smaller shape over the same vocabulary"""

    def __init__(self, dev, cfg, m):
        self.dev, self.cfg, self.m, self._d = dev, cfg, m, {}

    def draft(self, kind):
        import rama_amd
        if kind not in self._d:
            if kind == "self":
                self._d[kind] = rama_amd.Q8Model.from_model(self.m)
            elif kind == "q80_untied":                            # the Q8 fixture: vocabulary 64, seq_len 32
                self._d[kind] = rama_amd.Q8Model.load(self.dev, GOLDEN / "ckpt_v2_q80_untied.bin")
            else:
                c = rama_amd.Config(vocab_size=self.cfg.vocab_size, seq_len=self.cfg.seq_len, **W.SMALL_DRAFT)
                self._d[kind] = rama_amd.Q8Model.synth(self.dev, c, W.SMALL_GS, W.SMALL_SEED)
        return self._d[kind]

    def free(self):
        for q in self._d.values():
            q.free()
        self._d = {}


@pytest.fixture(scope="module")
def pairs(dev, models):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Pair(dev, *models(name))
        return made[name]
    yield get
    dev.lib.rama_serve_end(dev.ctx)
    for p in made.values():
        p.free()


class MReq:
    """a request: its context (BOS first), its plan, the target and draft engines of its slot and a twin of each for the solo runs"""

    def __init__(self, pair, dm, ctx, max_new, K, sampler=W.GREEDY, stop_at=None, n_cached=0):
        import rama_amd
        self.pair, self.dm, self.ctx, self.max_new, self.K, self.n_cached = pair, dm, list(ctx), max_new, K, n_cached
        self.T, self.topp, self.u = sampler
        d = pair.dev
        self.eng, self.twin = rama_amd.Engine(d, pair.m), rama_amd.Engine(d, pair.m)
        self.deng, self.dtwin = rama_amd.Q8Engine(d, dm), rama_amd.Q8Engine(d, dm)
        fill_all(self.eng); fill_all(self.deng)
        n = len(self.ctx)
        self.solo = [int(t) for t in self.twin.generate(self.ctx[1:], n - 1 + max_new, self.T, self.topp, self.u)][n - 1:]
        self.stop = -1 if stop_at is None else self.solo[stop_at]
        self._drafts = {}

    def want(self):
        return self.solo[:self.solo.index(self.stop) + 1] if self.stop in self.solo else list(self.solo)

    def draft_fn(self, prefix, n):
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
        assert got == self.want(), what
        valid, untouched = len(self.ctx) + len(got) - 1, len(self.ctx) - 1 + self.max_new
        for a, b in zip(cache(self.eng), cache(self.twin)):
            assert same_bits(a[:, :valid], b[:, :valid]), what
            assert (a[:, untouched:] == SENTINEL).all(), what
        if cursor is None:                                        # admitted without drafts: the draft cache is not the chain's
            return
        text = self.ctx + got
        assert len(self.ctx) <= cursor <= len(text), what
        self.dtwin.prefill(text[:cursor])
        for a, b in zip(cache(self.deng), cache(self.dtwin)):
            assert same_bits(a[:, :cursor], b[:, :cursor]), what
            assert (a[:, untouched:] == SENTINEL).all(), what

    def free(self):
        for e in (self.eng, self.twin, self.deng, self.dtwin):
            if e is not None:
                e.free()


def requests(pair, dm, workload, seed=3):
    """the workload's requests over W.contexts -- the contexts the host replay of tests/test_serve_model_f32_host.py uses"""
    ctxs = W.contexts(workload, pair.cfg.vocab_size, seed)
    return [MReq(pair, dm, c, new, K, samp, stop_at) for c, (_, new, K, samp, stop_at) in zip(ctxs, workload[3])]


def arr(v):
    return (C.c_int32 * max(len(v), 1))(*v)


def begin_model(dev, m, dm, n_slots, max_rows, cap, n_draft_cap=15):
    return dev.lib.rama_serve_begin_model(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(dm.ccfg), C.byref(dm.weights), n_slots, max_rows, cap,
                                          n_draft_cap)


def admit_model(dev, slot, r, K=None, prefill=True, eng=None, deng=None, ctx=None, n_cached=None, plan=None):
    """the draft model's rows of the whole context enqueued first (rama_q8_prefill), then rama_serve_admit_model"""
    ctx = r.ctx if ctx is None else ctx
    n_cached = r.n_cached if n_cached is None else n_cached
    eng, deng = eng or r.eng, deng or r.deng
    if prefill:
        deng.prefill(ctx)
    p = r.plan() if plan is None else plan
    return dev.lib.rama_serve_admit_model(dev.ctx, slot, C.byref(eng.state), C.byref(deng.state), arr(ctx), len(ctx), n_cached, C.byref(p),
                                          r.K if K is None else K)


def model_stats(dev):
    from rama_amd._lib import rama_q8_serve_model_report
    from rama_amd.q8 import serve_model_report
    r = rama_q8_serve_model_report()
    assert dev.lib.rama_serve_model_stats(dev.ctx, C.byref(r)) == 0
    return serve_model_report(r)


def drive(dev, pair, dm, reqs, workload, graph, what=None, between=None):
    """the workload under serve_model_replay's admission rule, one step at a time: after every step the device's tables against the replay's; at
    the end both reports, every request's tokens and both caches -> the replay.  between(k): called before step k"""
    from rama_amd.q8 import serve_model_replay
    n_slots, max_rows, use_slots = workload[:3]
    rp = serve_model_replay([r.spec() for r in reqs], [r.solo for r in reqs], [r.draft_fn for r in reqs], n_slots, max_rows, use_slots)
    set_graph(dev, graph)
    try:
        assert begin_model(dev, pair.m, dm, n_slots, max_rows, max(r.max_new for r in reqs)) == 0
        who, got, cursor = {}, {}, {}
        for k, st in enumerate(rp["steps"]):
            for slot, q in st["admitted"]:
                assert admit_model(dev, slot, reqs[q]) == 0, (what, k, slot)
                who[slot] = q
            if between:
                between(k)
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


def run(dev, pair, kind, workload, graph, what, seed=3, between=None):
    dm = pair.draft(kind)
    reqs = requests(pair, dm, workload, seed)
    try:
        return drive(dev, pair, dm, reqs, workload, graph, what, between)
    finally:
        dev.lib.rama_serve_end(dev.ctx)
        for r in reqs:
            r.free()


# ------------------------------------------------------------------ 1. the geometries, the drafts, the settings

@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("kind", ["self", "small"])
def test_one_slot_one_row_the_draft_cache_follows_without_a_grant(dev, pairs, kind, graph):
    rp = run(dev, pairs("TINY"), kind, W.ONE, graph, (kind, graph))
    assert rp["counters"]["drafts_granted"] == 0 and rp["counters"]["draft_passes"] > 0 and rp["counters"]["drafts_wanted"] > 0


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("kind", ["self", "small"])
def test_three_slots_around_a_free_hole(dev, pairs, kind, graph):
    rp = run(dev, pairs("TINY"), kind, W.HOLE, graph, (kind, graph))
    assert all(st["slots"][1][0] == FREE for st in rp["steps"]) and rp["counters"]["drafts_granted"] > 0


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("kind", ["self", "small"])
def test_prompts_arrive_while_others_decode(dev, pairs, kind, graph):
    """4 x 16: n_draft 0, 1, 2, 7 and 15, greedy and sampled plans, a stop token and a budget cut inside accepted runs, grants cut by a prompt"""
    rp = run(dev, pairs("TINY"), kind, W.ARRIVALS, graph, (kind, graph))
    assert rp["counters"]["drafts_granted"] > 0
    if kind == "small":
        assert "a == 0" in W.conditions(rp)


@pytest.mark.parametrize("graph", [0, 1])
def test_two_tiles_a_decode_slot_across_row_32(dev, pairs, graph):
    rp = run(dev, pairs("TINY"), "self", W.TWO_TILES, graph, ("two tiles", graph))
    assert any(W.straddles(st["rows"]) for st in rp["steps"])
    assert rp["counters"]["drafts_accepted"] > 0


@pytest.mark.parametrize("graph", [0, 1])
def test_sixteen_slots_fill_the_first_draft_pass_six_heads(dev, pairs, graph):
    """16 x 32 on the stories15M shape (six heads of 48): the draft is the target's own quantization, group size backed off to 32"""
    pair = pairs("STORIES15M")
    assert pair.draft("self").group_size == 32
    rp = run(dev, pair, "self", W.WIDE16, graph, ("wide", graph))
    assert max(len(st["drafting"]) for st in rp["steps"]) == 16 and rp["counters"]["drafts_granted"] > 0


def test_the_workloads_reach_every_condition_on_the_device(dev, pairs):
    """the workloads of the host replay (tests/test_serve_model_f32_host.py), driven on the device with the device's own solo and draft runs: the
    same eight conditions -- every outcome of a drafting slot-step, every state of the second tile -- occur, each step checked against the replay"""
    pair = pairs("TINY")
    seen = set()
    for name in ("HOLE", "ARRIVALS", "TWO_TILES", "GUARD"):
        for kind in ("self", "small"):
            seen |= W.conditions(run(dev, pair, kind, getattr(W, name), 1, (name, kind), W.SEEDS[name]))
    assert seen == W.ALL_CONDITIONS, seen


@pytest.fixture(scope="module")
def named(dev):
    """the fp32 fixtures by name -> Pair: a loaded legacy checkpoint, or rama_model_synth of the golden file's shape and seed"""
    import rama_amd
    made = {}

    def get(name):
        if name not in made:
            cfg, _, g = load_case(name)
            if name.startswith("ckpt_"):
                m = rama_amd.Model.load(dev, GOLDEN / f"{name}.bin")
            else:
                m = rama_amd.Model.synth(dev, to_rama_cfg(cfg), int(g["seed"]), rope=(g["freq_cis_real"], g["freq_cis_imag"]))
            made[name] = Pair(dev, cfg, m)
        return made[name]
    yield get
    dev.lib.rama_serve_end(dev.ctx)
    for p in made.values():
        p.free()
        p.m.free()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("target,kind,workload", [("ckpt_tied", "self", ARRIVALS_SHORT), ("ckpt_tied", "q80_untied", ARRIVALS_SHORT),
                                                  ("synth_d64_h4", "self", W.ARRIVALS), ("synth_d64_h4", "small", W.HOLE),
                                                  ("synth_d288_h6", "self", W.ARRIVALS), ("synth_d288_h6", "small", W.HOLE)],
                         ids=["tied-self", "tied-q80_untied", "d64-self", "d64-small", "d288-self", "d288-small"])
def test_named_targets_and_drafts(dev, named, target, kind, workload, graph):
    """ckpt_tied (dim 32, seq_len 16: the workload runs to the end of its window; from_model backs the group size off to 32), synth_d64_h4
    (seq_len 32) and synth_d288_h6 (six heads of 48); the drafts: the target's own quantization, the Q8 fixture over the same 64 tokens, a small
    unrelated model"""
    pair = named(target)
    if target == "ckpt_tied" and kind == "self":
        assert pair.draft("self").group_size == 32
    rp = run(dev, pair, kind, workload, graph, (target, kind, graph))
    assert rp["counters"]["drafts_granted"] > 0 and rp["counters"]["draft_passes"] > 0


# ------------------------------------------------------------------ 2. admissions: cached rows, the next turn, a block in flight

def finish_slots(dev, slots, bound=60):
    for _ in range(bound):
        if all(poll(dev, s, 0, 1)[1] for s in slots):
            return
        assert steps(dev, 1) == 0 and dev.lib.rama_sync(dev.ctx) == 0
    raise AssertionError("the chain did not finish")


@pytest.mark.parametrize("graph", [0, 1])
def test_admission_over_forked_rows_then_the_chats_next_turn_on_the_same_states(dev, pairs, graph):
    """n_cached > 0 twice: rows 0..7 of the target cache forked from a donor's prefill (the draft cache prefilled whole), then -- the same slot, the
    same two run states -- the chat's next turn over every row the first turn left, with a draft cursor that starts over at the new context's end"""
    pair = pairs("TINY")
    dm = pair.draft("self")
    rng = np.random.default_rng(11)
    V = pair.cfg.vocab_size
    long_ctx = [1] + [int(t) for t in rng.integers(2, V, 11)]
    a = MReq(pair, dm, long_ctx, 9, 7, W.SAMPLED, n_cached=8)
    donor = MReq(pair, dm, long_ctx[:9], 1, 0)
    b = None
    try:
        set_graph(dev, graph)
        assert begin_model(dev, pair.m, dm, 2, 8, 12) == 0
        prefill(dev, pair.m, donor.eng, long_ctx[:8])
        assert fork(dev, pair.m, donor.eng, a.eng, 8) == 0
        a.deng.prefill(a.ctx)
        assert admit_model(dev, 0, a, prefill=False) == 0
        finish_slots(dev, [0])
        got = tokens(dev, 0)
        a.check(got, model_stats(dev)["draft_cursor"][0], "forked")
        assert stats(dev)["prompt"] == len(long_ctx) - 8
        # the next turn: the first turn's text and three more tokens; every row the first turn wrote below its cursor is cached
        turn = long_ctx + got + [int(t) for t in rng.integers(2, V, 3)]
        cached = len(long_ctx) + len(got) - 1
        b = MReq(pair, dm, turn, 12, 15, W.GREEDY, n_cached=cached)
        b.eng.free(); b.deng.free()
        b.eng, b.deng = a.eng, a.deng
        assert admit_model(dev, 0, b) == 0                        # (the draft prefill of the whole new context goes first)
        finish_slots(dev, [0])
        b.check(tokens(dev, 0), model_stats(dev)["draft_cursor"][0], "next turn")
        assert poll(dev, 0)[2] == 2 and stats(dev)["prompt"] == len(long_ctx) - 8 + len(turn) - cached
        assert stats(dev)["captures"] == (1 if graph else 0)
        b.eng, b.deng = None, None
    finally:
        set_graph(dev, 0)
        dev.lib.rama_serve_end(dev.ctx)
        for r in (a, donor, b):
            if r is not None:
                r.free()


def test_admission_and_polling_while_a_block_is_in_flight(dev, pairs):
    import time
    pair = pairs("TINY")
    dm = pair.draft("self")
    reqs = requests(pair, dm, (2, 8, None, [(3, 20, 7, W.GREEDY, None), (5, 14, 2, W.SAMPLED, None)]), 5)
    try:
        set_graph(dev, 1)
        assert begin_model(dev, pair.m, dm, 2, 8, 20) == 0
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
        dev.lib.rama_serve_end(dev.ctx)
        for r in reqs:
            r.free()


# ------------------------------------------------------------------ 3. the classifier guard, the plain chain

def test_a_tile_without_a_logits_row_is_not_classified(dev, pairs):
    pair = pairs("TINY")
    dm = pair.draft("small")
    reqs = requests(pair, dm, W.GUARD, 5)
    n_slots, max_rows = W.GUARD[:2]
    try:
        set_graph(dev, 1)
        assert begin_model(dev, pair.m, dm, n_slots, max_rows, 6) == 0
        for i, r in enumerate(reqs):
            assert admit_model(dev, i, r) == 0
        base, rows, V = logits_rows(dev)
        assert (rows, V) == (max_rows, pair.cfg.vocab_size)
        n = (rows - TILE) * V
        fill = np.full(n, SENTINEL)
        assert dev.lib.rama_copy_h2d_f32(dev.ctx, C.c_void_p(base + 4 * TILE * V), fill.ctypes.data, n) == 0
        back = np.empty(n, np.float32)
        for k in range(3):      # step 0: tile 1 holds only rows inside slot 1's context (a live tile without a logits row); steps 1 and 2: it is wholly idle
            assert steps(dev, 1) == 0
            s = stats(dev)
            assert all(x[2] == 0 and x[0] == (1 if k == 0 else -1) for x in s["rows"][TILE:]), k
            assert dev.lib.rama_download_f32(dev.ctx, C.c_void_p(base + 4 * TILE * V), n, back.ctypes.data) == 0
            assert (back == SENTINEL).all(), k
        for _ in range(20):
            if all(poll(dev, i, 0, 1)[1] for i in range(2)):
                break
            assert steps(dev, 1) == 0 and dev.lib.rama_sync(dev.ctx) == 0
        ms = model_stats(dev)
        for i, r in enumerate(reqs):
            r.check(tokens(dev, i), ms["draft_cursor"][i], ("guard", i))
    finally:
        set_graph(dev, 0)
        dev.lib.rama_serve_end(dev.ctx)
        for r in reqs:
            r.free()


def test_without_drafts_the_chain_is_the_plain_chain(dev, pairs):
    """n_draft = 0 everywhere, by rama_serve_admit_model and by rama_serve_admit: the plain rama_serve_begin chain's tokens and row counters"""
    pair = pairs("TINY")
    dm = pair.draft("small")
    work = (3, 8, None, [(3, 7, 0, W.GREEDY, None), (5, 6, 0, W.SAMPLED, None), (2, 9, 0, W.GREEDY, None)])
    out = {}
    for kind in ("plain", "model"):
        reqs = requests(pair, dm, work, 8)
        try:
            if kind == "plain":
                assert dev.lib.rama_serve_begin(dev.ctx, C.byref(pair.m.ccfg), C.byref(pair.m.weights), 3, 8, 9) == 0
            else:
                assert begin_model(dev, pair.m, dm, 3, 8, 9) == 0
            for i, r in enumerate(reqs):
                if kind == "model" and i < 2:
                    assert admit_model(dev, i, r) == 0
                else:
                    p = r.plan()
                    assert dev.lib.rama_serve_admit(dev.ctx, i, C.byref(r.eng.state), arr(r.ctx), len(r.ctx), C.byref(p)) == 0
            for _ in range(20):
                if all(poll(dev, i, 0, 1)[1] for i in range(3)):
                    break
                assert steps(dev, 1) == 0 and dev.lib.rama_sync(dev.ctx) == 0
            s = stats(dev)
            out[kind] = ([tokens(dev, i) for i in range(3)], s["steps"], s["decode"], s["prompt"], s["idle"])
            for i, r in enumerate(reqs):
                r.check(out[kind][0][i], None, (kind, i))
            if kind == "model":
                assert spec_stats(dev)["drafts_wanted"] == 0 and model_stats(dev)["draft_passes"] == 0
        finally:
            dev.lib.rama_serve_end(dev.ctx)
            for r in reqs:
                r.free()
    assert out["plain"] == out["model"]


# ------------------------------------------------------------------ 4. refusals, lifetimes, neighbours

def test_every_refusal_leaves_the_chain_stepping(dev, pairs):
    from rama_amd._lib import check, rama_q8_serve_model_report, rama_q8_serve_plan, rama_q8_serve_spec
    import rama_amd
    pair = pairs("TINY")
    dm = pair.draft("small")
    d = dev
    reqs = requests(pair, dm, (3, 8, None, [(3, 13, 7, W.GREEDY, None), (2, 6, 2, W.SAMPLED, None), (2, 5, 1, W.GREEDY, None)]), 9)
    r0, r1, r2 = reqs
    c = rama_amd.Config(vocab_size=pair.cfg.vocab_size + 4, seq_len=pair.cfg.seq_len, **W.SMALL_DRAFT)
    other = rama_amd.Q8Model.synth(d, c, W.SMALL_GS, 3)
    try:
        assert begin_model(d, pair.m, dm, 3, 8, 13, 7) == 0
        assert admit_model(d, 0, r0) == 0 and steps(d, 2) == 0
        # begin: the vocabulary, n_draft_cap, the slots of the first draft pass, a NULL draft, the mode -- the running chain is untouched
        assert begin_model(d, pair.m, other, 3, 8, 13, 7) == EINVAL
        assert begin_model(d, pair.m, dm, 3, 8, 13, 0) == EINVAL and begin_model(d, pair.m, dm, 3, 8, 13, 16) == EINVAL
        assert begin_model(d, pair.m, dm, 65, 128, 9, 7) == EINVAL
        assert d.lib.rama_serve_begin_model(d.ctx, C.byref(pair.m.ccfg), C.byref(pair.m.weights), None, C.byref(dm.weights), 3, 8, 9, 7) == EINVAL
        for mode in (0, 2, 3):
            check(d.lib.rama_set_tuning(d.ctx, b"ref_order", mode))
            try:
                assert begin_model(d, pair.m, dm, 3, 8, 13, 7) == EUNSUP and steps(d, 1) == EUNSUP, mode
            finally:
                check(d.lib.rama_set_tuning(d.ctx, b"ref_order", 1))
        # admit
        assert admit_model(d, 0, r1) == EINVAL                                        # busy
        assert admit_model(d, 1, r1, K=8) == EINVAL and admit_model(d, 1, r1, K=-1) == EINVAL
        assert admit_model(d, 1, r1, deng=r1.eng, prefill=False) == EINVAL            # dstate is the target's
        assert admit_model(d, 1, r1, deng=r0.deng, prefill=False) == EINVAL           # a live slot's draft state
        assert admit_model(d, 1, r1, eng=r0.eng, prefill=False) == EINVAL             # a live slot's target state
        assert admit_model(d, 1, r1, n_cached=2, prefill=False) == EINVAL             # n_cached > n_context - 1
        p = r1.plan()
        assert d.lib.rama_serve_admit_model(d.ctx, 1, C.byref(r1.eng.state), None, arr(r1.ctx), len(r1.ctx), 0, C.byref(p), 2) == EINVAL
        spec = rama_q8_serve_spec(2, 3, None, 0)
        assert d.lib.rama_serve_admit_spec(d.ctx, 1, C.byref(r1.eng.state), arr(r1.ctx), len(r1.ctx), 0, C.byref(p), C.byref(spec)) == EINVAL
        # the fork refuses a live slot's draft run state
        assert d.lib.rama_q8_kv_fork(d.ctx, C.byref(dm.ccfg), C.byref(r1.deng.state), C.byref(r0.deng.state), 1, 1) == EINVAL
        # the plain admission on such a chain: n_draft = 0
        p2 = r2.plan()
        assert d.lib.rama_serve_admit(d.ctx, 2, C.byref(r2.eng.state), arr(r2.ctx), len(r2.ctx), C.byref(p2)) == 0
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
        assert d.lib.rama_serve_begin_spec(d.ctx, C.byref(pair.m.ccfg), C.byref(pair.m.weights), 3, 8, 9, 7, 0) == 0
        assert admit_model(d, 0, r0, prefill=False) == EINVAL
        assert d.lib.rama_serve_model_stats(d.ctx, C.byref(rama_q8_serve_model_report())) == EINVAL
    finally:
        d.lib.rama_serve_end(d.ctx)
        other.free()
        for r in reqs:
            r.free()


@pytest.mark.parametrize("gone", ["target model", "draft model", "draft state", "target state"])
def test_steps_refuse_once_a_model_or_a_live_run_state_is_freed(dev, gone):
    import rama_amd
    from oracle import synth as S
    from tests import serve_cases
    cfg = serve_cases.TINY
    m = rama_amd.Model.synth(dev, to_rama_cfg(cfg), 23, rope=S.rope_tables(cfg.seq_len, cfg.head_size))
    pair = Pair(dev, cfg, m)
    dm = pair.draft("small")
    r = MReq(pair, dm, [1, 5, 9], 9, 7)
    try:
        assert begin_model(dev, m, dm, 2, 8, 9) == 0
        assert admit_model(dev, 0, r) == 0 and steps(dev, 2) == 0
        if gone == "target model":
            r.twin.free(); r.twin = None
            m.free(); pair.m = None
        elif gone == "draft model":
            r.dtwin.free(); r.dtwin = None
            pair.free()
        elif gone == "draft state":
            r.deng.free()
        else:
            r.eng.free(); r.eng = None
        assert steps(dev, 1) == EINVAL
        assert admit_model(dev, 1, r, prefill=False, eng=r.twin if gone == "target state" else None) == EINVAL
    finally:
        dev.lib.rama_serve_end(dev.ctx)
        r.free()
        pair.free()
        if pair.m is not None:
            m.free()


def test_a_larger_q8_prefill_between_two_steps_moves_nothing_the_step_holds():
    """graph mode, on a context of its own (whose Q8 scratches no earlier test has grown): between two steps a rama_q8_prefill with a Q8 model
    larger than the draft (wider FFN, longer seq_len) regrows the context's Q8 scratches -- the captured step holds none of them, so it is
    replayed, not captured again (drive: one capture), and every token and cache row stays exact"""
    import rama_amd
    from oracle import synth as S
    from rama_amd._lib import check
    from tests import serve_cases
    d = rama_amd.Hip(0)
    check(d.lib.rama_set_tuning(d.ctx, b"ref_order", 1))
    cfg = serve_cases.TINY
    m = rama_amd.Model.synth(d, to_rama_cfg(cfg), 23, rope=S.rope_tables(cfg.seq_len, cfg.head_size))
    pair = Pair(d, cfg, m)
    c = rama_amd.Config(dim=128, hidden_dim=512, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=cfg.vocab_size, seq_len=4 * cfg.seq_len,
                        shared_weight=True)
    big = rama_amd.Q8Model.synth(d, c, 32, 5)
    be = rama_amd.Q8Engine(d, big)

    from rama_amd._lib import rama_q8_serve_plan, rama_q8_serve_report
    dm = pair.draft("small")
    qe = rama_amd.Q8Engine(d, dm)

    def q8_captures():
        r = rama_q8_serve_report()
        assert d.lib.rama_q8_serve_stats(d.ctx, C.byref(r)) == 0
        return int(r.graph_captures)

    def between(k):
        if k == 0:      # the witness: a Q8 serving chain over the draft's shape on the same context, its one step captured -- it holds the context's Q8 scratches
            assert d.lib.rama_q8_serve_begin(d.ctx, C.byref(dm.ccfg), C.byref(dm.weights), 1, 2, 20) == 0
            p = rama_q8_serve_plan(0.0, 0.9, 0.0, 20, -1)
            assert d.lib.rama_q8_serve_admit(d.ctx, 0, C.byref(qe.state), arr([1, 4]), 2, C.byref(p)) == 0
            assert d.lib.rama_q8_serve_steps(d.ctx, 1) == 0 and q8_captures() == 1
        if k == 3:
            assert d.lib.rama_q8_serve_steps(d.ctx, 1) == 0 and q8_captures() == 1       # (nothing so far has moved them)
            be.prefill([1] + list(range(2, 40)))
    try:
        rp = run(d, pair, "small", W.ARRIVALS, 1, "regrow", between=between)
        assert len(rp["steps"]) > 4
        # the scratches DID move: the witness's step was dropped with them and is captured again; drive() saw the fp32 chain's one capture throughout
        set_graph(d, 1)                                           # (drive() left graph mode off)
        assert d.lib.rama_q8_serve_steps(d.ctx, 1) == 0 and q8_captures() == 2
    finally:
        set_graph(d, 0)
        d.lib.rama_q8_serve_end(d.ctx)
        d.lib.rama_serve_end(d.ctx)
        qe.free()
        be.free(); big.free(); pair.free(); m.free()
        d.close()


def test_a_q8_chain_and_the_model_drafted_fp32_chain_step_in_turn(dev, pairs):
    import rama_amd
    from rama_amd._lib import rama_q8_serve_plan
    pair = pairs("TINY")
    dm = pair.draft("self")
    reqs = requests(pair, dm, (2, 8, None, [(3, 12, 7, W.GREEDY, None), (2, 9, 2, W.SAMPLED, None)]), 13)
    L = dev.lib
    qe, qt = rama_amd.Q8Engine(dev, dm), rama_amd.Q8Engine(dev, dm)
    try:
        set_graph(dev, 1)
        ctx = [1, 7, 4]
        solo = qt.generate(ctx[1:], 2 + 10)[2:]
        assert L.rama_q8_serve_begin(dev.ctx, C.byref(dm.ccfg), C.byref(dm.weights), 1, 4, 10) == 0
        p = rama_q8_serve_plan(0.0, 0.9, 0.0, 10, -1)
        assert L.rama_q8_serve_admit(dev.ctx, 0, C.byref(qe.state), arr(ctx), 3, C.byref(p)) == 0
        assert begin_model(dev, pair.m, dm, 2, 8, 12) == 0
        for i, r in enumerate(reqs):
            assert admit_model(dev, i, r) == 0
        for _ in range(16):
            assert L.rama_q8_serve_steps(dev.ctx, 1) == 0 and steps(dev, 1) == 0
        assert L.rama_sync(dev.ctx) == 0
        buf, k = (C.c_int32 * 16)(), C.c_int()
        assert L.rama_q8_serve_tokens(dev.ctx, 0, buf, 16, C.byref(k)) == 0
        assert [int(buf[i]) for i in range(k.value)] == solo
        ms = model_stats(dev)
        for i, r in enumerate(reqs):
            assert poll(dev, i, 0, 1)[1]
            r.check(tokens(dev, i), ms["draft_cursor"][i], ("in turn", i))
    finally:
        set_graph(dev, 0)
        L.rama_q8_serve_end(dev.ctx)
        L.rama_serve_end(dev.ctx)
        qe.free(); qt.free()
        for r in reqs:
            r.free()


# ------------------------------------------------------------------ 5. the server

def test_server_with_a_draft_model_gives_the_plain_servers_tokens(dev, pairs):
    import rama_amd
    pair = pairs("TINY")
    rng = np.random.default_rng(21)
    V = pair.cfg.vocab_size
    jobs = [([1] + [int(t) for t in rng.integers(2, V, n - 1)], new, samp) for n, new, samp in
            [(3, 9, W.GREEDY), (1, 6, W.SAMPLED), (6, 8, W.GREEDY), (2, 10, W.SAMPLED), (4, 5, W.GREEDY)]]
    twin = rama_amd.Engine(dev, pair.m)
    solo = [[int(t) for t in twin.generate(c[1:], len(c) - 1 + new, *s)][len(c) - 1:] for c, new, s in jobs]
    twin.free()
    out = {}
    for kind in ("plain", "draft"):
        srv = rama_amd.Server(pair.m, 3, 12, 10, **(dict(draft=pair.draft("self"), n_draft=7) if kind == "draft" else {}))
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
        rama_amd.Server(pair.m, 3, 12, 10, draft=pair.draft("self"), n_draft=7, hint_cap=8)
