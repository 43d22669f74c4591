"""Trees from a draft model on the GPU (rama_q8_spec_begin_model_tree): whatever the draft model proposes, the
tokens are bit for bit Q8Engine.generate's on the target alone, the target's rows below its cursor are that run's, the draft's rows
below the draft cursor a fresh draft prefill's, nothing behind the last position either cache may hold is written, the tree the
device built in every step is spec_model_tree_replay's -- with the draft engine's own forward as the logits function -- and all three
reports are the replay's.  Every comparison is exact.  The cases: tests/spec_model_tree_cases.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.spec_model_tree_cases import COVERAGE, GRID, LINE, OFF_TRUNK, PAIRS, SAMPLERS
from tests.test_hip_q8 import same_bits
from tests.test_hip_q8_spec_model import (SENTINEL, arr, caches, dev, fill, pairs, steps, tokens)  # noqa: F401  (dev, pairs: fixtures)
from tests.test_hip_q8_spec_model import begin as begin_line
from tests.test_hip_q8_spec_model import stats as stats_line

pytestmark = pytest.mark.gpu

EINVAL = -1


def begin(dev, m, eng, dm, deng, ctx, max_new, T=0.0, P=0.9, u=0.0, stop=-1, K=4, B=2, R=16, prefill=True, hint=None):
    from rama_amd._lib import rama_q8_spec_plan
    if prefill and len(ctx) > 1:
        eng.prefill(ctx[:-1], 0)
        deng.prefill(ctx[:-1], 0)
    h = arr(hint or [])
    plan = rama_q8_spec_plan(T, P, u, max_new, stop, K, 3, h if hint else None, len(hint or []))
    return dev.lib.rama_q8_spec_begin_model_tree(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state), C.byref(dm.ccfg),
                                                 C.byref(dm.weights), C.byref(deng.state), arr(ctx), len(ctx), C.byref(plan), B, R)


def stats(dev):
    """all three reports as one dict"""
    from rama_amd._host import _report
    from rama_amd._lib import rama_q8_spec_tree_report
    q = rama_q8_spec_tree_report()
    assert dev.lib.rama_q8_spec_tree_stats(dev.ctx, C.byref(q)) == 0
    return dict(stats_line(dev), **_report(q))


def logits_fn(p):
    """the draft model's logits row after a prefix: the draft twin's own prefill and forward, computed once per prefix"""
    memo, where = p.__dict__.setdefault("_rows", {}), p.__dict__.setdefault("_where", {})

    def fn(prefix):
        key = tuple(prefix)
        if key not in memo:
            if len(prefix) > 1:
                p.dtwin.prefill(list(prefix[:-1]), 0)
            p.dtwin.forward(int(prefix[-1]), len(prefix) - 1)
            memo[key] = p.dtwin.logits().copy()
            where[id(memo[key])] = key
        return memo[key]
    return fn


def sampler(p, T, P, u):
    """Device::sample of a row logits_fn gave: the last maximal index, or -- sampled -- the draft twin's own next token behind the row's
    prefix under (T, P, u), the draft function of tests/test_hip_q8_spec_model.py"""
    draft = p.draft_fn(T, P, u)

    def pick(row):
        if T == 0.0:
            return int(len(row) - 1 - np.argmax(np.asarray(row)[::-1]))
        return int(draft(list(p._where[id(row)]), 1)[0])
    return pick


def replay(p, ctx, max_new, K, B, R, T=0.0, P=0.9, u=0.0, stop=None):
    from rama_amd.q8 import spec_model_tree_replay
    key = ("tree", tuple(ctx), max_new, K, B, R, T, P, u, stop)
    memo = p.__dict__.setdefault("_replays", {})
    if key not in memo:
        want, twin_cache = p.solo(ctx, max_new, T, P, u)
        traj, cursors = spec_model_tree_replay(want, logits_fn(p), ctx, K, B, R, max_new, stop, sampler(p, T, P, u))
        memo[key] = (want, twin_cache, traj, cursors)
    return memo[key]


def sums(traj, cursors, depth_fed):
    """what the three reports must show after the steps of a replayed trajectory"""
    hist, nodes = [0] * 16, [0] * 16
    off = [sum(1 for k, j in enumerate(path) if j != k) for *_, path, _, _ in traj]
    for cap, tok, _, _, _, a, _, _, _ in traj:
        hist[a] += 1
        nodes[len(tok) - 1] += 1
    return dict(steps=len(traj), rows_fed=sum(len(s[1]) for s in traj), drafts=sum(len(s[1]) - 1 for s in traj), accepted=sum(s[5] for s in traj),
                emitted=sum(len(s[7]) for s in traj), accepted_hist=hist, draft_passes=sum(s[0] for s in traj),
                draft_rows_fed=sum(depth_fed(s) + s[8] for s in traj), catch_up_rows=sum(s[8] for s in traj), draft_cursor=cursors[1],
                off_trunk_accepted=sum(off), off_trunk_steps=sum(1 for o in off if o), nodes_hist=nodes)


def fed_rows(step):
    cap, depth = step[0], step[3]
    return sum(1 for d in depth if d <= cap - 1) if cap else 0


def run_and_check(p, ctx, max_new, K, B, R, T=0.0, P=0.9, u=0.0, stop=None, graph=0):
    """the chain step by step for exactly the replayed number of steps, and everything the header promises of it"""
    from rama_amd.q8 import spec_model_tree_last
    dev = p.dev
    want, twin_cache, traj, cursors = replay(p, ctx, max_new, K, B, R, T, P, u, stop)
    n_out = sum(len(s[7]) for s in traj)
    what = (p.name, K, B, R, T, stop, graph)
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        fill(p.eng); fill(p.deng)
        assert begin(dev, p.m, p.eng, p.dm, p.deng, ctx, max_new, T, P, u, -1 if stop is None else stop, K, B, R) == 0
        for cap, tok, parent, depth, picks, a, path, emitted, _ in traj:
            assert steps(dev, 1) == 0
            last = spec_model_tree_last(dev)
            assert (last["tok"], last["parent"], last["depth"], last["path"], last["m"], last["a"]) == (tok, parent, depth, path, len(tok) - 1, a), what
            assert all(g == w for g, w in zip(last["picks"], picks) if w != -2), what      # (a pick off every right path is never compared)
        got = tokens(dev)
        st = stats(dev)
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
    assert got == want[:n_out], what
    assert stop is None or got[-1] == stop or n_out == max_new, what
    ref = sums(traj, cursors, fed_rows)
    assert {k: st[k] for k in ref} == ref, what
    assert st["finished"] == 1 and st["n_out"] == n_out and st["cursor"] == cursors[0] == len(ctx) - 1 + n_out, what
    assert (st["n_branch"], st["n_rows"]) == (B, R) and st["graph_captures"] == graph, what
    # the target's rows below its cursor are the solo run's; a sentinel at and behind the last position the cache may hold
    valid = len(ctx) - 1 + n_out
    for g, r in zip(caches(p.eng), twin_cache):
        assert same_bits(g[:, :valid], r[:, :valid]), what
        assert (g[:, valid:] == SENTINEL).all(), what
    # the draft's rows below the draft cursor are a fresh draft prefill's; nothing at or behind max(Dc, the last root's position + 1)
    s, Dc = ctx + got, cursors[1]
    draft_cache = caches(p.deng)
    if Dc > 0:
        p.dtwin.prefill(s[:Dc], 0)
        for g, r in zip(draft_cache, caches(p.dtwin)):
            assert same_bits(g[:, :Dc], r[:, :Dc]), what
    drafted = [len(ctx) - 1 + sum(len(t[7]) for t in traj[:i]) for i, t in enumerate(traj) if t[0]]      # the roots the draft model was fed
    for g in draft_cache:
        assert (g[:, max([Dc] + [r + 1 for r in drafted]):] == SENTINEL).all(), what
    return st, traj


# ------------------------------------------------------------------ 1. the grid

@pytest.mark.parametrize("sampler_name", list(SAMPLERS))
@pytest.mark.parametrize("K,B,R", GRID)
@pytest.mark.parametrize("name", list(PAIRS))
def test_tokens_rows_trees_and_reports(pairs, name, K, B, R, sampler_name):
    p = pairs(name)
    ctx = p.context()
    for graph in (0, 1):
        run_and_check(p, ctx, p.shape[1], K, B, R, *SAMPLERS[sampler_name], graph=graph)


@pytest.mark.parametrize("K,B,R", GRID)
def test_the_off_trunk_case(pairs, K, B, R):
    """the case of tests/spec_model_tree_cases.py chosen on the CPU for accepted nodes off the trunk: the chain against the replay as above,
    and the replay's counts those recorded"""
    p = pairs(OFF_TRUNK["pair"])
    ctx = p.context(OFF_TRUNK["context_seed"])
    for graph in (0, 1):
        st, traj = run_and_check(p, ctx, p.shape[1], K, B, R, *OFF_TRUNK["sampler"], graph=graph)
    assert (st["steps"], st["accepted"], st["off_trunk_accepted"]) == OFF_TRUNK["counts"][(K, B, R)]


def test_every_outcome_occurs(pairs):
    """the coverage condition of tests/spec_model_tree_cases.py on the replays of the recorded cases, which the tests above hold the device to"""
    cases = [(name, None, smp) for name in PAIRS for smp in SAMPLERS.values()] + [(OFF_TRUNK["pair"], OFF_TRUNK["context_seed"], OFF_TRUNK["sampler"])]
    seen = set()
    for name, seed, smp in cases:
        p = pairs(name)
        for K, B, R in GRID:
            for cap, tok, _, _, _, a, path, _, cu in replay(p, p.context(seed), p.shape[1], K, B, R, *smp)[2]:
                if cap:
                    seen |= {"zero"} if a == 0 else set()
                    seen |= {"full"} if a == cap else set()
                    seen |= {"partial"} if 0 < a < cap else set()
                seen |= {"catch_up"} if cu else set()
                seen |= {"off_trunk"} if any(j != k for k, j in enumerate(path)) else set()
                assert len(path) - 1 == a
    assert seen == set(COVERAGE), sorted(set(COVERAGE) - seen)


# ------------------------------------------------------------------ 2. the linear chain again

@pytest.mark.parametrize("K,name", LINE)
def test_one_branch_is_the_model_chain(pairs, K, name):
    p, dev = pairs(name), pairs(name).dev
    ctx, max_new = p.context(), p.shape[1]
    out = []
    for tree in (False, True):
        fill(p.eng); fill(p.deng)
        if tree:
            assert begin(dev, p.m, p.eng, p.dm, p.deng, ctx, max_new, K=K, B=1, R=K + 1) == 0
        else:
            assert begin_line(dev, p.m, p.eng, p.dm, p.deng, ctx, max_new, K=K) == 0
        assert steps(dev, max_new) == 0
        out.append((tokens(dev), stats_line(dev)))
    assert out[0] == out[1]


# ------------------------------------------------------------------ 3. stops and bounds

@pytest.mark.parametrize("graph", [0, 1])
def test_a_stop_token_and_a_budget_inside_an_accepted_path(pairs, graph):
    p = pairs("untied<-untied")
    ctx = p.context()
    want = p.solo(ctx, p.shape[1])[0]
    run_and_check(p, ctx, p.shape[1], 4, 2, 16, stop=want[2], graph=graph)      # emitted at depth 2 of the first step's path
    run_and_check(p, ctx, 7, 4, 2, 16, graph=graph)                              # 5 + 2: the second step's tree is cut to cap = 1
    run_and_check(p, ctx, 3, 7, 3, 16, graph=graph)                              # the budget binds inside the first path


def test_bos_alone_and_the_last_rows_of_both_windows(pairs):
    p = pairs("untied<-untied")
    run_and_check(p, [1], 12, 4, 2, 16)
    assert sum(p.shape) == p.cfg.seq_len
    run_and_check(p, p.context(), p.shape[1], 7, 2, 16, graph=1)
    q = pairs("untied<-tied")
    assert sum(q.shape) == q.dm.cfg.seq_len < q.cfg.seq_len
    run_and_check(q, q.context(), q.shape[1], 7, 2, 16, graph=1)


# ------------------------------------------------------------------ 4. refusals and frees

def test_refusals_leave_a_running_chain_stepping(pairs):
    p, dev = pairs("untied<-untied"), pairs("untied<-untied").dev
    ctx, max_new = p.context(), p.shape[1]
    want = p.solo(ctx, max_new)[0]
    fill(p.eng); fill(p.deng)
    assert begin(dev, p.m, p.eng, p.dm, p.deng, ctx, max_new) == 0
    assert steps(dev, 1) == 0
    for kw in (dict(B=0), dict(B=5), dict(R=1), dict(R=17), dict(K=0), dict(K=16), dict(hint=[1, 2]), dict(max_new=0),
               dict(max_new=p.cfg.seq_len)):
        args = dict(dict(max_new=max_new), **kw)
        assert begin(dev, p.m, p.eng, p.dm, p.deng, ctx, prefill=False, **args) == EINVAL, kw
    assert begin(dev, p.m, p.eng, p.m, p.eng, ctx, max_new, prefill=False) == EINVAL          # the draft run state is the target's
    other = pairs("gs8<-gs8")
    assert begin(dev, p.m, p.eng, other.m, other.deng, ctx, max_new, prefill=False) == EINVAL  # another vocabulary
    assert steps(dev, max_new) == 0
    assert tokens(dev) == want


def test_n_branch_beyond_the_vocabulary_is_refused(dev):
    import rama_amd
    cfg = dict(dim=64, hidden_dim=128, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=3, seq_len=16, shared_weight=True)
    m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), 32, 1)
    e, d = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, m)
    try:
        assert begin(dev, m, e, m, d, [1, 2], 4, K=2, B=4, R=16) == EINVAL
        assert begin(dev, m, e, m, d, [1, 2], 4, K=2, B=3, R=16) == 0
        assert steps(dev, 4) == 0
        assert dev.lib.rama_q8_spec_end(dev.ctx) == 0
    finally:
        e.free(); d.free(); m.free()


@pytest.mark.parametrize("which", ["draft state", "draft model", "target state"])
def test_steps_refuse_once_a_model_or_a_state_is_freed(dev, golden_dir, which):
    import rama_amd
    m = rama_amd.Q8Model.load(dev, golden_dir / "ckpt_v2_q80_untied.bin")
    dm = rama_amd.Q8Model.load(dev, golden_dir / "ckpt_v2_q80_untied.bin")
    e, d = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, dm)
    assert begin(dev, m, e, dm, d, [1, 5, 9], 8) == 0 and steps(dev, 1) == 0
    if which == "draft state":
        d.free()
    elif which == "target state":
        e.free()
    else:
        dm.free()                                                  # (the draft run state is still there)
    assert steps(dev, 1) == EINVAL
    assert dev.lib.rama_q8_spec_end(dev.ctx) == 0
    for x in (e, d):
        x.free()
    dm.free(); m.free()


# ------------------------------------------------------------------ 5. ancestors across position 1 024

LONG = dict(dim=64, hidden_dim=128, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=64, seq_len=1100, shared_weight=True)


@pytest.mark.parametrize("n_ctx", [1022, 1030])
def test_ancestors_across_the_switch_of_the_score_paths(dev, n_ctx):
    """P = 1021: the nodes of depths 3.. sit at positions >= 1024 (staged pieces) with ancestors below it (straight); P = 1029: every row staged"""
    import rama_amd
    from rama_amd.q8 import spec_model_tree_last, spec_model_tree_replay
    m = rama_amd.Q8Model.synth(dev, O.Config(**LONG), 32, 3)
    e, d, twin = (rama_amd.Q8Engine(dev, m) for _ in range(3))
    try:
        ctx = [1] + [int(t) for t in np.random.default_rng(4).integers(0, 64, n_ctx - 1)]
        max_new = 12
        want = twin.generate(ctx[1:], len(ctx) - 1 + max_new, 0.0)[len(ctx) - 1:]
        rows = {}

        def fn(prefix):
            if len(prefix) not in rows or rows[len(prefix)][0] != prefix:
                twin.prefill(list(prefix[:-1]), 0)
                twin.forward(int(prefix[-1]), len(prefix) - 1)
                rows[len(prefix)] = (list(prefix), twin.logits().copy())
            return rows[len(prefix)][1]
        traj, cursors = spec_model_tree_replay(want, fn, ctx, 6, 2, 16, max_new, None, lambda row: int(len(row) - 1 - np.argmax(row[::-1])))
        assert begin(dev, m, e, m, d, ctx, max_new, K=6, B=2, R=16) == 0
        for cap, tok, parent, depth, picks, a, path, emitted, _ in traj:
            assert steps(dev, 1) == 0
            last = spec_model_tree_last(dev)
            assert (last["tok"], last["path"], last["a"]) == (tok, path, a)
        assert tokens(dev) == want
        assert traj[0][5] == 6                                     # a model drafting for itself: the whole trunk, across the switch
        twin.prefill((ctx + want)[:cursors[1]], 0)
        for g, r in zip(caches(d), caches(twin)):
            assert same_bits(g[:, :cursors[1]], r[:, :cursors[1]])
        assert dev.lib.rama_q8_spec_end(dev.ctx) == 0
    finally:
        for x in (e, d, twin):
            x.free()
        m.free()
