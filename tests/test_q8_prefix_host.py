"""Prompt caching for the serving chain, host side (no GPU): the two new symbols are declared everywhere; the scheduling rule
handles PROMPT slots that start behind position 0 (rama_q8_serve_plan_step against a restatement); a whole workload replayed
through the host plan with and without cached rows feeds exactly the rows that are not cached, reaches the same successor
states and never needs more steps; and the donor pool of Q8Server's prefix cache -- longest prefix, the cap, ties, eviction --
with fake engines."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests.test_q8_serve_host import check_properties, rule

REPO = Path(__file__).resolve().parent.parent
FREE, PROMPT, DECODE, DONE = 0, 1, 2, 3
SYMBOLS = ["rama_q8_serve_admit_at", "rama_q8_kv_fork"]


def test_prefix_symbols_are_declared_everywhere():
    import rama_amd
    from rama_amd import _lib
    L = rama_amd.load()
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "rama_hip.h").read_text(), flags=re.S)
    rust = (REPO / "integration" / "rust" / "hip_sys.rs").read_text()
    for s in SYMBOLS:
        decl = re.search(rf"\b{s}\s*\(([^;]*)\)\s*;", header)
        assert decl, f"include/rama_hip.h lacks {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES lacks {s}"
        assert hasattr(L, s), f"librama_hip.so lacks {s}"
        assert len(re.findall(rf"pub fn {s}\s*\(", rust)) == 1, f"hip_sys.rs must declare {s} once"
        res, args = _lib.SIGNATURES[s]
        assert res is C.c_int and decl.group(1).count(",") + 1 == len(args), s
    # admit_at is admit with n_cached in front of the plan
    a, b = _lib.SIGNATURES["rama_q8_serve_admit"][1], _lib.SIGNATURES["rama_q8_serve_admit_at"][1]
    assert b == a[:-1] + [C.c_int] + a[-1:]


# ------------------------------------------------------------------ the rule with cursors behind 0

def table_with_cached_prompts(rng, n_slots, seq_len=96):
    """every live slot PROMPT or DECODE; PROMPT slots start anywhere in 1 .. n_context - 1 (or at 0)"""
    t = []
    for _ in range(n_slots):
        state = int(rng.choice([FREE, PROMPT, PROMPT, PROMPT, DECODE, DONE]))
        n_ctx = int(rng.integers(2, seq_len // 2))
        max_new = int(rng.integers(1, seq_len // 2))
        if state == PROMPT:
            cur = int(rng.choice([0, 1, n_ctx - 1, int(rng.integers(0, n_ctx))]))
            t.append((PROMPT, n_ctx, cur, 0, max_new))
        elif state == DECODE:
            max_new = max(max_new, 2)
            n_out = int(rng.integers(1, max_new))
            t.append((DECODE, n_ctx, n_ctx + n_out - 1, n_out, max_new))
        elif state == DONE:
            t.append((DONE, n_ctx, n_ctx + max_new - 1, max_new, max_new))
        else:
            t.append((FREE, 0, 0, 0, 0))
    return t


def test_plan_step_with_cursors_behind_zero_equals_the_rule():
    from rama_amd.q8 import serve_plan_step
    rng = np.random.default_rng(20261017)
    seen_cached = 0
    for case in range(240):
        n_slots = int(rng.integers(1, 33)) if case % 8 else int(rng.choice([1, 128]))
        max_rows = int(rng.integers(n_slots, 129)) if case % 5 else n_slots
        t = table_with_cached_prompts(rng, n_slots)
        seen_cached += sum(1 for s in t if s[0] == PROMPT and s[2] > 0)
        rows, after = serve_plan_step(t, max_rows)
        assert (rows, after) == rule(t, max_rows), (case, t, max_rows)
        check_properties(t, rows, after, max_rows)
        for i, s in enumerate(t):                       # a cached slot never gets a row below its cursor
            if s[0] == PROMPT:
                assert min(r[1] for r in rows if r[0] == i) == s[2]
    assert seen_cached > 500


# ------------------------------------------------------------------ a whole workload, with and without cached rows

def replay(requests, n_slots, max_rows, cached):
    """requests: (n_context, max_new, n_cached) admitted in order into the first FREE / DONE slot -> (steps, prompt rows, the
    final state of every request, every request's rows fed as (first position, count of context rows))"""
    from rama_amd.q8 import serve_plan_step
    pending = list(enumerate(requests))
    t, who = [(FREE, 0, 0, 0, 0)] * n_slots, [None] * n_slots
    steps = prompt_rows = 0
    final, fed = {}, {k: [] for k in range(len(requests))}
    while True:
        for i in range(n_slots):
            if t[i][0] in (FREE, DONE) and pending:
                if who[i] is not None:
                    final[who[i]] = t[i]
                k, (n_ctx, new, n_c) = pending.pop(0)
                t[i], who[i] = (PROMPT, n_ctx, n_c if cached else 0, 0, new), k
        if not any(s[0] in (PROMPT, DECODE) for s in t):
            break
        rows, after = serve_plan_step(t, max_rows)
        assert (rows, after) == rule(t, max_rows)
        check_properties(t, rows, after, max_rows)
        for r in rows:
            if r[0] >= 0 and t[r[0]][0] == PROMPT:
                prompt_rows += 1
                fed[who[r[0]]].append(r[1])
        t = after
        steps += 1
        assert steps < 100000
    for i in range(n_slots):
        if who[i] is not None:
            final[who[i]] = t[i]
    return steps, prompt_rows, final, fed


@pytest.mark.parametrize("n_slots,max_rows", [(4, 4), (4, 8), (4, 16), (16, 64), (32, 128), (1, 1), (1, 128)])
def test_workload_replay_with_and_without_cached_rows(n_slots, max_rows):
    rng = np.random.default_rng(77 * n_slots + max_rows)
    reqs = []
    for k in range(5 * n_slots + 3):
        n_ctx, new = int(rng.integers(1, 90)), int(rng.integers(1, 40))
        n_c = int(rng.choice([0, n_ctx - 1, int(rng.integers(0, n_ctx))]))       # 0 <= n_cached <= n_context - 1
        reqs.append((n_ctx, new, n_c))
    s0, p0, f0, fed0 = replay(reqs, n_slots, max_rows, cached=False)
    s1, p1, f1, fed1 = replay(reqs, n_slots, max_rows, cached=True)
    assert p0 == sum(r[0] for r in reqs)
    assert p1 == sum(r[0] - r[2] for r in reqs)
    assert p1 < p0
    # every request ends in the same state either way, and is fed exactly its positions n_cached .. n_context - 1, in order
    assert f0 == f1 and len(f0) == len(reqs)
    for k, (n_ctx, new, n_c) in enumerate(reqs):
        assert f1[k] == (DONE, n_ctx, n_ctx + new - 1, new, new)
        assert fed0[k] == list(range(n_ctx)) and fed1[k] == list(range(n_c, n_ctx))
    assert s1 <= s0


# ------------------------------------------------------------------ the donor pool

class FakeEngine:
    def __init__(self, name):
        self.name = name

    def __eq__(self, other):            # the pool must compare by identity: equal-looking engines are different engines
        return True

    __hash__ = None


def test_pool_longest_prefix_cap_ties_and_empty():
    from rama_amd.q8 import PrefixPool, common_prefix
    assert common_prefix([1, 2, 3], [1, 2, 4, 5]) == 2 and common_prefix([], [1]) == 0 and common_prefix([1, 2], [1, 2]) == 2
    pool = PrefixPool(4)
    assert pool.match([1, 2, 3]) == (None, 0) and len(pool) == 0             # an empty pool
    a, b, c = FakeEngine("a"), FakeEngine("b"), FakeEngine("c")
    assert pool.put([1, 2, 3, 4, 5, 6], a) == []
    assert pool.put([1, 2, 3, 9, 9], b) == []
    assert pool.put([7, 7, 7], c) == []
    e, n = pool.match([1, 2, 3, 4, 8, 8])
    assert e is a and n == 4                                                  # the longest shared prefix
    e, n = pool.match([1, 2, 3, 9, 9, 1])
    assert e is b and n == 5
    e, n = pool.match([1, 2, 3, 4, 5, 6])
    assert e is a and n == 5                                                  # the cap: the final context position is fed
    e, n = pool.match([1, 2, 3, 4])
    assert e is a and n == 3
    assert pool.match([1]) == (None, 0)                                       # a one-token context has nothing to take
    assert pool.match([5, 1, 2, 3]) == (None, 0)                              # no shared first token
    # a tie (both share [1, 2, 3]): the most recently used donor, and it stays the most recently used
    e, n = pool.match([1, 2, 3, 0])
    assert e is a and n == 3
    pool.match([1, 2, 3, 9, 0])                                               # b is used
    e, n = pool.match([1, 2, 3, 0])
    assert e is b and n == 3
    with pytest.raises(ValueError):
        PrefixPool(-1)


def test_pool_evicts_the_least_recently_used_at_k():
    from rama_amd.q8 import PrefixPool
    pool = PrefixPool(2)
    a, b, c, d = (FakeEngine(x) for x in "abcd")
    assert pool.put([1, 1], a) == [] and pool.put([2, 2], b) == []
    out = pool.put([3, 3], c)
    assert len(out) == 1 and out[0] is a and len(pool) == 2                   # a was put first and never used
    assert pool.match([2, 2, 5])[0] is b                                      # b is used: c is now the oldest
    out = pool.put([4, 4], d)
    assert len(out) == 1 and out[0] is c
    assert [e.name for e in pool.engines()] == ["b", "d"]
    assert a not in pool and c not in pool and b in pool and d in pool       # (identity, not ==)
    with pytest.raises(ValueError):
        pool.put([9], b)                                                      # a donor is in the pool once
    none = PrefixPool(0)
    out = none.put([1, 2], a)
    assert len(out) == 1 and out[0] is a and len(none) == 0                   # no cache: nothing is kept


class _Cfg:
    dim, hidden_dim, n_layers, n_heads, n_kv_heads, vocab_size, seq_len, shared_weight = 64, 128, 2, 4, 4, 512, 64, True


class _Engine:
    """stands for a Q8Engine the server made or was given"""
    made = 0

    def __init__(self, model):
        self.model, self.state, self.freed = model, C.c_int(1), False

    def free(self):
        self.freed = True


class _Lib:
    """records the library calls of a Q8Server; every slot finishes as soon as it is polled"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name,) + a)
            if name == "rama_q8_serve_poll":
                a[5]._obj.value = 1          # n_ready: one token
                a[3][0] = 42
                a[6]._obj.value = 1          # finished
            if name == "rama_q8_serve_stats":          # (a finish the host plan did not foresee makes the server look)
                r = a[1]._obj
                r.n_slots, r.max_rows = 2, 4
                for i in range(2):
                    r.slots[i].state = DONE
            return 0
        return call


class _Device:
    def __init__(self):
        self.lib, self.ctx = _Lib(), None


class _Model:
    cfg = _Cfg()
    ccfg = C.c_int()
    weights = C.c_int()

    def __init__(self):
        self.device = _Device()


def _server(monkeypatch, k):
    from rama_amd import q8
    made = []

    def engine(device, model):
        e = _Engine(model)
        made.append(e)
        return e
    monkeypatch.setattr(q8, "Q8Engine", engine)
    m = _Model()
    return q8.Q8Server(m, 2, 4, 8, prefix_cache=k), m, made


def _poll_once(srv):
    """the fake library finishes a slot at its first poll; one token each (so a donor's key is its context)"""
    srv.poll()


def test_server_pool_never_hands_out_a_donor_and_retain_false_leaves_the_pool_alone(monkeypatch):
    srv, m, made = _server(monkeypatch, 2)
    calls = m.device.lib.calls
    h0 = srv.submit([1, 2, 3, 4, 5], 1, retain=True)
    h1 = srv.submit([1, 9, 9], 1)                                             # retain=False
    assert len(made) == 2 and srv.cached(h0) == 0 and srv.cached(h1) == 0
    assert not any(c[0] == "rama_q8_kv_fork" for c in calls)                  # an empty pool: no fork
    _poll_once(srv)
    assert srv.finished(h0) and srv.finished(h1)
    assert len(srv.pool) == 1 and srv.pool.engines()[0] is made[0]
    # the donor is no slot's engine any more; the other engine still is
    assert all(e is not made[0] for e in srv._own) and any(e is made[1] for e in srv._own)
    # the next requests: slot 0 needs a NEW engine (the donor is never handed out), and the match is forked into it
    h2 = srv.submit([1, 2, 3, 4, 5, 6, 7], 1)
    assert len(made) == 3 and srv.cached(h2) == 5
    fork = [c for c in calls if c[0] == "rama_q8_kv_fork"]
    assert len(fork) == 1 and fork[0][5:] == (1, 5)
    assert fork[0][3]._obj is made[0].state and fork[0][4]._obj is made[2].state
    at = [c for c in calls if c[0] == "rama_q8_serve_admit_at"]
    assert len(at) == 1 and at[0][2] == 0 and at[0][5:7] == (7, 5)
    assert srv._mirror[0] == (PROMPT, 7, 5, 0, 1)                             # the mirrored slot starts at cursor = n_cached
    h3 = srv.submit([1, 2, 3, 4, 5], 1)                                       # the whole context is cached: capped at n_context - 1
    assert srv.cached(h3) == 4 and srv._mirror[1] == (PROMPT, 5, 4, 0, 1)
    assert srv.rows_cached == 9
    with pytest.raises(ValueError):
        srv.submit([1, 2], 1, engine=made[0])                                 # a donor cannot be a request's engine
    with pytest.raises(ValueError):
        srv.submit([1, 2, 3], 1, n_cached=3, engine=_Engine(m))               # n_cached <= n_context - 1
    with pytest.raises(ValueError):
        srv.submit([1, 2, 3], 1, n_cached=-1, engine=_Engine(m))
    with pytest.raises(ValueError):
        srv.submit([1, 2, 3], 1, n_cached=1)                                  # whose rows?
    _poll_once(srv)
    assert len(srv.pool) == 1                                                 # h1, h2, h3 did not retain: the pool is as it was
    # the caller's own rows: no fork, no pool lookup, admitted at the cursor given
    mine = _Engine(m)
    n_fork = len([c for c in calls if c[0] == "rama_q8_kv_fork"])
    h4 = srv.submit([1, 2, 3, 4, 5, 6], 1, engine=mine, n_cached=2)
    assert srv.cached(h4) == 2 and len([c for c in calls if c[0] == "rama_q8_kv_fork"]) == n_fork
    _poll_once(srv)
    # two more donors: the oldest leaves, and -- the server made it -- serves requests again instead of a new engine
    h5 = srv.submit([7, 7, 7], 1, retain=True)
    _poll_once(srv)
    h6 = srv.submit([8, 8, 8], 1, retain=True)
    _poll_once(srv)
    assert len(srv.pool) == 2 and made[0] not in srv.pool and any(e is made[0] for e in srv._spare)
    n_made = len(made)
    srv.submit([6, 6], 1)
    srv.submit([6, 5], 1)
    assert len(made) <= n_made + 1 and not srv._spare
    srv.close()
    assert all(e.freed for e in made) and not mine.freed


def test_server_without_a_prefix_cache_ignores_retain(monkeypatch):
    srv, m, made = _server(monkeypatch, 0)
    h = srv.submit([1, 2, 3], 1, retain=True)
    _poll_once(srv)
    assert srv.finished(h) and len(srv.pool) == 0 and srv._own[0] is made[0]
    srv.submit([1, 2, 3, 4], 1)
    assert len(made) == 1 and not any(c[0] in ("rama_q8_kv_fork", "rama_q8_serve_admit_at") for c in m.device.lib.calls)
    srv.close()
