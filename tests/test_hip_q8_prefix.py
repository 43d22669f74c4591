"""Prompt caching for the serving chain on the GPU (rama_q8_kv_fork, rama_q8_serve_admit_at, Q8Server(prefix_cache=k)).  The
fork copies rows [0, n) of every layer of both caches and touches nothing else; a sequence admitted over forked rows gives, bit
for bit, the tokens and cache rows of Q8Engine.generate run on it alone -- whatever n, the chunking of the tail, the
neighbours, max_rows and the graph mode; a chat's next turn re-admits its own run state; refusals leave everything as it was.
Every comparison is exact (bits as int32)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_hip_q8 import same_bits
from tests.test_hip_q8_serve import (DECODE, DONE, EINVAL, FREE, PROMPT, SENTINEL, STORIES15M, Req, admit, begin, cache, dev,  # noqa: F401
                                     open_model, poll, run_until_done, set_graph, stats, steps, tokens)

pytestmark = pytest.mark.gpu

MODELS = ["ckpt_v2_q80_tied", "ckpt_v2_q80_untied", "synth15m"]
SHAPE_7B_L1 = dict(dim=4096, hidden_dim=11008, n_layers=1, n_heads=32, n_kv_heads=32, vocab_size=32000, seq_len=2048, shared_weight=False)
SHAPE_TIED = dict(dim=32, hidden_dim=96, n_layers=2, n_heads=2, n_kv_heads=2, vocab_size=64, seq_len=16, shared_weight=True)      # ckpt_v2_q80_tied's


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------ raw run states for the fork (it needs no model)

class Caches:
    """two device buffers of n_layers * seq_len * dim floats as the key and value cache of a rama_run_state; `shift` floats into
    their allocations (1: bases that are not 16-byte aligned)"""

    def __init__(self, dev, cfg, shift=0):
        from rama_amd._lib import rama_run_state
        self.dev, self.cfg, self.shift = dev, cfg, shift
        self.n = cfg["n_layers"] * cfg["seq_len"] * cfg["dim"]
        self.base = []
        for _ in range(2):
            ptr = C.c_void_p()
            assert dev.lib.rama_alloc_f32(dev.ctx, self.n + 4, C.byref(ptr)) == 0
            self.base.append(ptr.value)
        self.state = rama_run_state()
        self.state.key_cache, self.state.value_cache = self.base[0] + 4 * shift, self.base[1] + 4 * shift

    def put(self, k, v):
        for ptr, a in ((self.state.key_cache, k), (self.state.value_cache, v)):
            a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
            assert a.size == self.n
            assert self.dev.lib.rama_copy_h2d_f32(self.dev.ctx, ptr, a.ctypes.data, a.size) == 0

    def get(self):
        out = []
        for ptr in (self.state.key_cache, self.state.value_cache):
            a = np.empty(self.n, dtype=np.float32)
            assert self.dev.lib.rama_download_f32(self.dev.ctx, ptr, a.size, a.ctypes.data) == 0
            out.append(a.reshape(self.cfg["n_layers"], self.cfg["seq_len"], self.cfg["dim"]))
        return out

    def free(self):
        for b in self.base:
            self.dev.lib.rama_free(self.dev.ctx, b)
        self.base = []


def ccfg(cfg):
    from rama_amd._lib import rama_config
    return rama_config(*[int(cfg[k]) for k in ("dim", "hidden_dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size", "seq_len", "shared_weight")])


def fork(dev, cfg, src, dsts, n_rows, n_dst=None):
    from rama_amd._lib import rama_run_state
    arr = (rama_run_state * max(len(dsts), 1))(*[d.state for d in dsts])
    return dev.lib.rama_q8_kv_fork(dev.ctx, C.byref(ccfg(cfg)), C.byref(src.state), arr, len(dsts) if n_dst is None else n_dst, n_rows)


def patterns(cfg, n_dst):
    """the source: every float distinct within a cache and between the two; destination d: one sentinel value of its own"""
    n = cfg["n_layers"] * cfg["seq_len"] * cfg["dim"]
    shape = (cfg["n_layers"], cfg["seq_len"], cfg["dim"])
    sk = (np.arange(n, dtype=np.int64) % (1 << 23)).astype(np.float32).reshape(shape) + np.float32(0.5)
    sv = -sk - np.float32(1.0)
    return sk, sv, [np.float32(1000.25 + d) for d in range(n_dst)]


def check_fork(dev, cfg, n_rows, n_dst, shift_src=0, shift_dst=0):
    src = Caches(dev, cfg, shift_src)
    dsts = [Caches(dev, cfg, shift_dst) for _ in range(n_dst)]
    try:
        sk, sv, marks = patterns(cfg, n_dst)
        src.put(sk, sv)
        for d, m in zip(dsts, marks):
            d.put(np.full(sk.shape, m), np.full(sk.shape, -m))
        assert fork(dev, cfg, src, dsts, n_rows) == 0
        gk, gv = src.get()
        assert np.array_equal(bits(gk), bits(sk)) and np.array_equal(bits(gv), bits(sv)), "the source changed"
        for d, m in zip(dsts, marks):
            for got, s_, fill in zip(d.get(), (sk, sv), (m, -m)):
                want = np.full(sk.shape, fill, dtype=np.float32)
                want[:, :n_rows] = s_[:, :n_rows]
                assert np.array_equal(bits(got), bits(want)), (n_rows, n_dst, shift_src, shift_dst)
    finally:
        for c in [src] + dsts:
            c.free()


@pytest.mark.parametrize("cfg", [SHAPE_TIED, STORIES15M], ids=["dim32_seq16", "stories15M"])
@pytest.mark.parametrize("n_dst", [1, 2, 16])
def test_fork_copies_rows_and_nothing_else(dev, cfg, n_dst):
    """dim 32: one row is 8 sixteen-byte words, less than one wave; dim 288: 3 rows are 216 words, no multiple of 64, and
    seq_len rows are 18 432 words, 18 workgroups per span"""
    for n_rows in (0, 1, 3, cfg["seq_len"]):
        check_fork(dev, cfg, n_rows, n_dst)


@pytest.mark.parametrize("n_dst", [1, 16])
def test_fork_7b_shape_one_layer_1100_rows(dev, n_dst):
    check_fork(dev, SHAPE_7B_L1, 1100, n_dst)


@pytest.mark.parametrize("cfg", [SHAPE_TIED, STORIES15M], ids=["dim32_seq16", "stories15M"])
@pytest.mark.parametrize("shifts", [(1, 1), (1, 0), (0, 1)])
def test_fork_from_and_to_cache_bases_offset_by_one_float(dev, cfg, shifts):
    for n_rows in (1, 3, cfg["seq_len"]):
        check_fork(dev, cfg, n_rows, 2, *shifts)


def test_fork_refusals_change_nothing(dev):
    from rama_amd._lib import rama_run_state
    cfg = STORIES15M
    src, a, b = Caches(dev, cfg), Caches(dev, cfg), Caches(dev, cfg)
    try:
        sk, sv, marks = patterns(cfg, 2)
        src.put(sk, sv)
        for d, m in zip((a, b), marks):
            d.put(np.full(sk.shape, m), np.full(sk.shape, -m))
        L, cc = dev.lib, ccfg(cfg)
        one = (rama_run_state * 1)(a.state)
        crossed = Caches.__new__(Caches)                     # a destination whose key cache is the source's value cache
        crossed.state = rama_run_state()
        crossed.state.key_cache, crossed.state.value_cache = src.state.value_cache, b.state.value_cache
        inside = Caches.__new__(Caches)                      # ... and one that starts inside another destination's
        inside.state = rama_run_state()
        inside.state.key_cache, inside.state.value_cache = a.state.key_cache + 4 * cfg["dim"], b.state.value_cache
        hollow = Caches.__new__(Caches)
        hollow.state = rama_run_state()
        refused = [
            L.rama_q8_kv_fork(None, C.byref(cc), C.byref(src.state), one, 1, 3),
            L.rama_q8_kv_fork(dev.ctx, None, C.byref(src.state), one, 1, 3),
            L.rama_q8_kv_fork(dev.ctx, C.byref(cc), None, one, 1, 3),
            L.rama_q8_kv_fork(dev.ctx, C.byref(cc), C.byref(src.state), None, 1, 3),
            fork(dev, cfg, src, [a], 3, n_dst=0), fork(dev, cfg, src, [a] * 17, 3),
            fork(dev, cfg, src, [a], -1), fork(dev, cfg, src, [a], cfg["seq_len"] + 1),
            fork(dev, cfg, src, [src], 3), fork(dev, cfg, src, [a, src], 3),
            fork(dev, cfg, src, [a, b, a], 3), fork(dev, cfg, src, [crossed], 3), fork(dev, cfg, src, [a, inside], 3),
            fork(dev, cfg, src, [hollow], 3), fork(dev, cfg, hollow, [a], 3),
            fork(dev, cfg, src, [src], 0),                    # (checked before the no-op)
        ]
        assert refused == [EINVAL] * len(refused)
        assert fork(dev, cfg, src, [a, b], 0) == 0
        assert dev.lib.rama_sync(dev.ctx) == 0
        for d, m in zip((a, b), marks):
            gk, gv = d.get()
            assert (gk == m).all() and (gv == -m).all()
        gk, gv = src.get()
        assert np.array_equal(bits(gk), bits(sk)) and np.array_equal(bits(gv), bits(sv))
    finally:
        for c in (src, a, b):
            c.free()


# ------------------------------------------------------------------ admission over forked rows

def fork_eng(dev, m, donor, dst_engs, n):
    from rama_amd._lib import rama_run_state
    arr = (rama_run_state * len(dst_engs))(*[e.state for e in dst_engs])
    return dev.lib.rama_q8_kv_fork(dev.ctx, C.byref(m.ccfg), C.byref(donor.state), arr, len(dst_engs), n)


def admit_at(dev, slot, r, n_cached, ctx=None, eng=None):
    ctx = r.ctx if ctx is None else ctx
    p = r.plan()
    return dev.lib.rama_q8_serve_admit_at(dev.ctx, slot, C.byref((eng or r.eng).state), (C.c_int32 * max(len(ctx), 1))(*ctx), len(ctx), n_cached, C.byref(p))


def cached_req(dev, m, rng, n_ctx, max_new, n, donors, T=0.0, topp=0.9, u=0.0, ctx=None):
    """a request whose engine holds sentinels everywhere but rows 0..n-1, forked from a donor that ingested the context by
    rama_q8_prefill"""
    import rama_amd
    r = Req(dev, m, rng, n_ctx, max_new, T, topp, u)
    if ctx is not None:
        r.ctx = list(ctx)
    donor = rama_amd.Q8Engine(dev, m)
    donors.append(donor)
    donor.prefill(r.ctx)
    assert fork_eng(dev, m, donor, [r.eng], n) == 0
    r.n_cached = n
    return r


def cases(cfg, max_rows):
    """(n_context, max_new, n_cached): n = 1, the middle, n_context - 1, and -- where seq_len has room for it -- a tail longer
    than max_rows (seq_len 16 has room at max_rows 8 only)"""
    long_ctx = min(cfg.seq_len - 4, max_rows + 24)
    if cfg.seq_len < 64:
        return [(long_ctx, 3, 1), (9, 4, 4), (7, 5, 6), (2, 6, 1)]
    return [(long_ctx, 6, 1), (21, 8, 10), (13, 5, 12), (max_rows + 21, 7, 3)]


SAMPLERS = [(0.0, 0.9, 0.0), (1.0, 0.9, 0.1), (0.0, 0.9, 0.0), (0.7, 0.5, 0.6)]


@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("max_rows", [8, 16])
def test_admit_at_equals_the_solo_run(dev, golden_dir, which, graph, max_rows):
    from rama_amd.q8 import serve_plan_step
    m = open_model(dev, golden_dir, which)
    rng = np.random.default_rng(100 * max_rows + graph)
    todo = cases(m.cfg, max_rows)
    reqs, donors = [], []
    try:
        for i, (n_ctx, new, n) in enumerate(todo):
            reqs.append(cached_req(dev, m, rng, n_ctx, new, n, donors, *SAMPLERS[i]))
        assert any(len(r.ctx) - r.n_cached > max_rows for r in reqs) or m.cfg.seq_len - 5 <= max_rows
        for i, r in enumerate(reqs):
            r.solo()
            if i == 1:
                r.stop = r.solo()[r.max_new // 2]              # one sequence stops on a token of its own solo run
        set_graph(dev, graph)
        assert begin(dev, m, len(reqs), max_rows, max(t[1] for t in todo)) == 0
        for i, r in enumerate(reqs):
            assert admit_at(dev, i, r, r.n_cached) == 0
        before = stats(dev)
        assert before["slots"] == [(PROMPT, len(r.ctx), r.n_cached, 0, r.max_new) for r in reqs]
        n_steps = 0
        while any(s[0] in (PROMPT, DECODE) for s in before["slots"]):
            assert steps(dev, 1) == 0
            now = stats(dev)
            rows, after = serve_plan_step(before["slots"], max_rows)
            assert now["rows"] == rows, n_steps                 # the device's row table is the host plan's, from cursor = n_cached
            for i, r in enumerate(reqs):
                if r.stop < 0:
                    assert now["slots"][i] == after[i], (n_steps, i)
            before = now
            n_steps += 1
            assert n_steps < 400
        assert before["prompt"] == sum(len(r.ctx) - r.n_cached for r in reqs)
        assert before["captures"] == (1 if graph else 0)
        for i, r in enumerate(reqs):
            r.check(tokens(dev, i), (which, graph, max_rows, i))
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs:
            r.free()
        for d in donors:
            d.free()
        m.free()


# ------------------------------------------------------------------ neighbours

@pytest.mark.parametrize("graph", [0, 1])
def test_cached_admission_next_to_running_slots(dev, golden_dir, graph):
    """two slots decode and one ingests a 45-token context in chunks when a cached admission joins; a second one goes into a
    just-finished slot while a block of steps is still in flight.  Everybody equals their solo run."""
    import time
    m = open_model(dev, golden_dir, "synth15m")
    rng = np.random.default_rng(31 + graph)
    donors = []
    reqs = [Req(dev, m, rng, 2, 30), Req(dev, m, rng, 3, 5, 1.0, 0.9, 0.3), Req(dev, m, rng, 45, 6)]
    try:
        joiner = cached_req(dev, m, rng, 26, 7, 14, donors, 0.8, 0.7, 0.45)
        late = cached_req(dev, m, rng, 33, 5, 20, donors, 1.0, 0.9, 0.37)
        for r in reqs + [joiner, late]:
            r.solo()
        set_graph(dev, graph)
        assert begin(dev, m, 4, 8, 30) == 0
        for i, r in enumerate(reqs):
            assert admit(dev, i, r) == 0
        assert steps(dev, 3) == 0                                # slots 0 and 1 decode, slot 2 is inside its context
        st = stats(dev)
        assert [s[0] for s in st["slots"]] == [DECODE, DECODE, PROMPT, FREE] and 0 < st["slots"][2][2] < 45
        assert admit_at(dev, 3, joiner, joiner.n_cached) == 0
        # one block, asynchronous: slot 1 (5 tokens) finishes early in it; the finished word is watched by poll alone
        assert steps(dev, 40) == 0
        deadline = time.time() + 60
        while not poll(dev, 1, 0, 1)[1] and time.time() < deadline:
            pass
        assert poll(dev, 1, 0, 1)[1]
        old_tokens, _, gen0 = poll(dev, 1)
        assert admit_at(dev, 1, late, late.n_cached) == 0        # behind whatever of the block is still running
        assert steps(dev, 60) == 0
        assert poll(dev, 1)[2] == gen0 + 1
        for i, r in [(0, reqs[0]), (2, reqs[2]), (3, joiner), (1, late)]:
            r.check(tokens(dev, i), (graph, i))
        reqs[1].check(old_tokens, (graph, "old"))
        st = stats(dev)
        assert st["captures"] == (1 if graph else 0) and all(s[0] == DONE for s in st["slots"])
        assert st["prompt"] == sum(len(r.ctx) for r in reqs) + (26 - 14) + (33 - 20)
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs + [joiner, late]:
            r.free()
        for d in donors:
            d.free()
        m.free()


# ------------------------------------------------------------------ a live donor

@pytest.mark.parametrize("graph", [0, 1])
def test_fork_from_a_slot_that_is_still_decoding(dev, golden_dir, graph):
    m = open_model(dev, golden_dir, "synth15m")
    rng = np.random.default_rng(41)
    a = Req(dev, m, rng, 30, 20, 1.0, 0.9, 0.2)
    b = Req(dev, m, rng, 24, 9)
    try:
        n = 17
        b.ctx = a.ctx[:n] + b.ctx[n:]
        a.solo(); b.solo()
        set_graph(dev, graph)
        assert begin(dev, m, 2, 8, 20) == 0
        assert admit(dev, 0, a) == 0
        assert steps(dev, 8) == 0                                # 30 context positions in 4 steps of 8 rows, then it decodes
        st = stats(dev)
        assert st["slots"][0][0] == DECODE
        assert fork_eng(dev, m, a.eng, [a.eng], n) == EINVAL
        assert fork_eng(dev, m, b.eng, [a.eng], n) == EINVAL    # a live slot's run state is no destination
        assert fork_eng(dev, m, a.eng, [b.eng], n) == 0         # ... but a source, for rows below what it has written
        assert admit_at(dev, 1, b, n) == 0
        run_until_done(dev, [0, 1])
        a.check(tokens(dev, 0), (graph, "donor"))
        b.check(tokens(dev, 1), (graph, "copy"))
        assert stats(dev)["prompt"] == 30 + (24 - n)
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        a.free(); b.free()
        m.free()


# ------------------------------------------------------------------ the next turn of a chat

@pytest.mark.parametrize("which", ["ckpt_v2_q80_untied", "synth15m"])
@pytest.mark.parametrize("graph", [0, 1])
def test_next_turn_on_the_same_run_state(dev, golden_dir, which, graph):
    m = open_model(dev, golden_dir, which)
    rng = np.random.default_rng(51 + graph)
    small = m.cfg.seq_len < 64
    T = (1.0, 0.9, 0.6) if graph else (0.0, 0.9, 0.0)
    a = Req(dev, m, rng, 4 if small else 9, 3 if small else 6, *T)
    turn = Req(dev, m, rng, 1, 3 if small else 5, *T)
    spare = turn.eng
    try:
        a.solo()
        set_graph(dev, graph)
        assert begin(dev, m, 2, 8, 8) == 0
        assert admit(dev, 0, a) == 0
        run_until_done(dev, [0])
        got = tokens(dev, 0)
        a.check(got, (which, graph, "first turn"))
        turn.ctx = a.ctx + got + [int(t) for t in rng.integers(2, m.cfg.vocab_size, 5)]
        n_cached = len(a.ctx) + len(got) - 1
        turn.eng.free()
        turn.eng = a.eng                                         # the same run state: rows 0 .. n_cached - 1 are there
        turn.solo()
        assert admit_at(dev, 0, turn, n_cached) == 0
        run_until_done(dev, [0])
        turn.check(tokens(dev, 0), (which, graph, "next turn"))
        st = stats(dev)
        assert st["prompt"] == len(a.ctx) + len(turn.ctx) - n_cached
        assert st["captures"] == (1 if graph else 0) and st["generation"][0] == 2
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        a.free(); turn.twin.free(); spare.free()
        m.free()


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("graph", [0, 1])
def test_bad_n_cached_is_refused_and_the_chain_runs_on(dev, golden_dir, graph):
    m = open_model(dev, golden_dir, "synth15m")
    rng = np.random.default_rng(61)
    donors = []
    reqs = [Req(dev, m, rng, 5, 10, 1.0, 0.9, 0.3), Req(dev, m, rng, 19, 8)]
    try:
        extra = cached_req(dev, m, rng, 11, 6, 5, donors)
        for r in reqs + [extra]:
            r.solo()
        set_graph(dev, graph)
        assert begin(dev, m, 3, 8, 12) == 0
        for i, r in enumerate(reqs):
            assert admit(dev, i, r) == 0
        assert steps(dev, 2) == 0
        n = len(extra.ctx)
        assert [admit_at(dev, 2, extra, k) for k in (-1, n, n + 1)] == [EINVAL] * 3
        assert admit_at(dev, 0, extra, 5) == EINVAL                          # admit's own checks apply: a busy slot
        assert admit_at(dev, 2, extra, 5, eng=reqs[1].eng) == EINVAL         # ... a run state already live
        assert admit_at(dev, 2, extra, 0, ctx=[1, m.cfg.vocab_size]) == EINVAL
        st = stats(dev)
        assert st["slots"][2][0] == FREE and st["generation"][2] == 0
        assert admit_at(dev, 2, extra, 5) == 0
        run_until_done(dev, [0, 1, 2])
        for i, r in enumerate(reqs + [extra]):
            r.check(tokens(dev, i), (graph, i))
        assert stats(dev)["captures"] == (1 if graph else 0)
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for r in reqs + [extra]:
            r.free()
        for d in donors:
            d.free()
        m.free()


def test_admit_at_zero_is_admit(dev, golden_dir):
    m = open_model(dev, golden_dir, "ckpt_v2_q80_tied")
    rng = np.random.default_rng(62)
    r = Req(dev, m, rng, 6, 5)
    try:
        r.solo()
        assert begin(dev, m, 1, 4, 8) == 0
        assert admit_at(dev, 0, r, 0) == 0
        assert stats(dev)["slots"][0] == (PROMPT, 6, 0, 0, 5)
        run_until_done(dev, [0])
        r.check(tokens(dev, 0), "n_cached 0")
        assert stats(dev)["prompt"] == 6
    finally:
        dev.lib.rama_q8_serve_end(dev.ctx)
        r.free()
        m.free()


# ------------------------------------------------------------------ a deep context

def test_7b_shape_one_layer_tail_behind_1100_forked_rows(dev):
    """one llama2-7B-shaped layer (GS 64): 1 100 rows forked, a 20-token tail, 4 new tokens -- the attention's staged path
    beyond position 1 024 reads copied rows"""
    import rama_amd
    m = rama_amd.Q8Model.synth(dev, O.Config(**SHAPE_7B_L1), 64, 5)
    rng = np.random.default_rng(70)
    donors = []
    r = None
    try:
        r = cached_req(dev, m, rng, 1120, 4, 1100, donors)
        r.solo()
        set_graph(dev, 1)
        assert begin(dev, m, 2, 32, 8) == 0
        assert admit_at(dev, 0, r, 1100) == 0
        assert steps(dev, 4) == 0
        st = stats(dev)
        assert st["slots"][0][0] == DONE and st["prompt"] == 20 and st["captures"] == 1
        got = tokens(dev, 0)
        assert got == r.want()
        last = len(r.ctx) + len(got) - 2
        d = SHAPE_7B_L1["dim"]
        for name in ("key_cache", "value_cache"):
            mine = r.eng.buffer(name, (last + 9) * d)
            assert same_bits(mine[:(last + 1) * d], r.twin.buffer(name, (last + 1) * d)), name
            assert (mine[(last + 1) * d:] == SENTINEL).all(), name
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        if r is not None:
            r.free()
        for e in donors:
            e.free()
        m.free()


# ------------------------------------------------------------------ Q8Server(prefix_cache=2)

@pytest.mark.parametrize("graph", [0, 1])
def test_server_prefix_cache(dev, golden_dir, graph):
    """12 requests over 3 shared prefixes through 4 slots; the first of each prefix is retained, the two-donor pool evicts the
    first prefix's donor, whose requests are then ingested in full.  Tokens equal the cache-off run and the solo runs."""
    import rama_amd
    from rama_amd.q8 import Q8Server, common_prefix
    m = open_model(dev, golden_dir, "synth15m")
    c = m.cfg
    rng = np.random.default_rng(80 + graph)
    twin = rama_amd.Q8Engine(dev, m)
    servers = []
    try:
        prefixes = [[1] + [int(t) for t in rng.integers(2, c.vocab_size, 23)] for _ in range(3)]
        reqs = []                                                # (context, max_new, T, topp, u, prefix index)
        for k in range(4):
            for pi, pre in enumerate(prefixes):
                tail = [int(t) for t in rng.integers(2, c.vocab_size, int(rng.integers(3, 10)))]
                new = [2, 6, 10][pi] if k == 0 else int(rng.integers(2, 9))       # the first ones finish in the order 0, 1, 2
                T, P, U = [(0.0, 0.9, 0.0), (1.0, 0.9, 0.21), (0.8, 0.6, 0.7)][(k + pi) % 3]
                reqs.append((pre + tail, new, T, P, U, pi))
        want = [twin.generate(r[0][1:], len(r[0]) - 1 + r[1], r[2], r[3], r[4])[len(r[0]) - 1:] for r in reqs]
        set_graph(dev, graph)
        results = {}
        for k_pool in (2, 0):
            srv = Q8Server(m, 4, 8, 16, prefix_cache=k_pool)
            servers.append(srv)
            first = [srv.submit(*r[:5], retain=True) for r in reqs[:3]]
            srv.run()
            rest = [srv.submit(*r[:5]) for r in reqs[3:]]
            srv.run()
            hs = first + rest
            results[k_pool] = [srv.result(h) for h in hs]
            st = srv.stats()
            cached = [srv.cached(h) for h in hs]
            if k_pool == 0:
                assert cached == [0] * 12 and st["rows_cached"] == 0 and len(srv.pool) == 0
            else:
                # the donors: prefix 0's left the pool when prefix 2's came (prefix 1's went in between)
                keys = {pi: reqs[pi][0] + want[pi][:-1] for pi in (1, 2)}
                expect = [0, 0, 0] + [0 if r[5] == 0 else min(common_prefix(keys[r[5]], r[0]), len(r[0]) - 1) for r in reqs[3:]]
                assert cached == expect
                assert all(n >= 24 for n, r in zip(cached[3:], reqs[3:]) if r[5] != 0)
                assert len(srv.pool) == 2
                assert st["rows_cached"] == sum(cached) > 0
            assert st["rows_prompt"] == sum(len(r[0]) for r in reqs) - sum(cached)
            for key in ("steps", "rows_decode", "rows_prompt", "rows_idle"):
                assert st[key] == srv.planned[key], (key, st[key], srv.planned[key])
            assert st["graph_captures"] == (1 if graph else 0)
            srv.close()
        assert results[2] == want and results[0] == want
    finally:
        for srv in servers:
            srv.close()
        set_graph(dev, 0)
        twin.free()
        m.free()
