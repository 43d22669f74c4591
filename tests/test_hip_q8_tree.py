"""Tree drafts on the GPU (q8_tree.hpp).

The building block, rama_q8_tree_forward / _commit: every node's logits row is bit-identical to rama_q8_forward's on a twin engine fed
the prefix and then the node's path tokens -- rejected nodes included, which is where a wrong ancestor read would hide --, the cache
after the pass is its state before but for the root's row (a sentinel stands behind pos0), and after the commit of a path rows
pos0..pos0+a are the twin's and the rest is still the sentinel.  The shapes: a line of 16, a star, a binary tree, two 7-node branches
that diverge at depth 3, 5 live rows, one row; the positions: 0 (every timestep but one from ancestors), around the 64-row value tiles
and their two buffers (62..64, 126..128), 250..256, and on the seq_len-2560 model 1016 with depth 15 (a row's timesteps straddle the
staged-score switch at 1024) and 2040.

The chain, rama_q8_spec_begin_tree: tokens, cache rows below the cursor and the sentinel FROM THE CURSOR ON (stricter than the linear
chain) against Q8Engine.generate on a twin; both reports against spec_tree_replay step by step; one captured graph.  n_branch in
{1, 2, 4} x n_rows in {2, 8, 16}, eager and graph mode, greedy and sampled, with the solo output followed by a copy with every fifth
token changed as hint, and the two parts in the other order.  Where the rule can send the run off the trunk -- two or more branches, 16
rows, the true text in front (the corrupted copy, which ends later, is then branch 0) -- the case first ASSERTS that the replay on the
solo tokens has at least 3 steps with off-trunk accepted nodes at depth >= 2 and counters that differ from the n_branch = 1 replay's.
With one branch no node is off the trunk, with 2 rows no node has depth 2, and with the true text behind the copy the trunk is the true
text: there the rule itself rules the property out, and the case compares everything else.

Every comparison is exact: token lists and float bit patterns."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_hip_q8 import same_bits
from tests.test_hip_q8_spec import SENTINEL, STORIES15M, arr, caches, corrupt, fill_behind, poll, stats, steps, tokens
from tests.test_hip_q8_spec_long import LONG

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -2
GOLDEN = ("ckpt_v2_q80_tied", "ckpt_v2_q80_untied", "ckpt_v2_q80_gs8")

LINE = [-1] + list(range(15))
STAR = [-1] + [0] * 15
BINARY = [-1] + [(j - 1) // 2 for j in range(1, 16)]
FORK = [-1, 0, 1, 2, 3, 4, 5, 6, 3, 8, 9, 10]          # 7 nodes in a line; a second branch shares the first 3 and has 4 of its own
FIVE = [-1, 0, 0, 1, 2]
ONE = [-1]
TREES = dict(line=LINE, star=STAR, binary=BINARY, fork=FORK, five=FIVE, one=ONE)


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


class Pair:
    """a model, the engine under test and the twin for the solo runs"""

    def __init__(self, dev, golden_dir, which):
        import rama_amd
        self.dev, self.which = dev, which
        if which.startswith(("synth15m", "long")):               # "_untied": a classifier of its own, so that a greedy run does not repeat its input
            shape = dict(STORIES15M if which.startswith("synth15m") else LONG, shared_weight=not which.endswith("_untied"))
            self.m = rama_amd.Q8Model.synth(dev, O.Config(**shape), 32, 11)
        else:
            self.m = rama_amd.Q8Model.load(dev, golden_dir / f"{which}.bin")
        self.cfg = self.m.cfg
        self.eng, self.twin = rama_amd.Q8Engine(dev, self.m), rama_amd.Q8Engine(dev, self.m)
        self._solo = {}

    def solo(self, ctx, max_new, T=0.0, P=0.9, u=0.0):
        """(the max_new tokens Q8Engine.generate gives behind ctx on the twin, the twin's caches after that run), computed once"""
        key = (tuple(ctx), max_new, T, P, u)
        if key not in self._solo:
            toks = self.twin.generate(ctx[1:], len(ctx) - 1 + max_new, T, P, u)[len(ctx) - 1:]
            self._solo[key] = (toks, caches(self.twin))
        return self._solo[key]

    def free(self):
        self.eng.free(); self.twin.free(); self.m.free()


@pytest.fixture(scope="module")
def pairs(dev, golden_dir):
    made = {}

    def get(which):
        if which not in made:
            made[which] = Pair(dev, golden_dir, which)
        return made[which]
    yield get
    dev.lib.rama_q8_spec_end(dev.ctx)
    for b in made.values():
        b.free()


def depths(parent):
    d = [0] * len(parent)
    for j in range(1, len(parent)):
        d[j] = d[parent[j]] + 1
    return d


def path_to(parent, j):
    out = [j]
    while parent[out[-1]] >= 0:
        out.append(parent[out[-1]])
    return out[::-1]


# ------------------------------------------------------------------ 1. the building block

def tree_cases():
    out = []
    for pos0 in (0, 62, 63, 64, 126, 127, 128, 250, 251, 252, 253, 254, 255, 256, 2040):
        for name in ("line", "fork") if pos0 not in (0, 63, 255) else tuple(TREES):
            out.append(("long", name, pos0))
    out += [("long", name, 1016) for name in ("line", "binary", "fork")]          # depth 15 from 1016: positions 1016..1031
    out += [("synth15m", name, pos0) for name in TREES for pos0 in (0, 63, 128, 240)]
    out += [("synth15m", "star", 254), ("synth15m", "one", 255)]
    for which, seq_len in zip(GOLDEN, (16, 32, 24)):
        for name in TREES:
            deepest = max(depths(TREES[name]))
            out += [(which, name, pos0) for pos0 in (0, 3, seq_len - 1 - deepest) if 0 <= pos0 < seq_len - deepest]
    return sorted(set(out))


@pytest.mark.parametrize("which,tree,pos0", tree_cases())
def test_tree_forward_rows_and_commit_equal_the_twin(pairs, which, tree, pos0):
    b = pairs(which)
    parent, V, S = TREES[tree], b.cfg.vocab_size, b.cfg.seq_len
    dep = depths(parent)
    assert pos0 + max(dep) < S
    rng = np.random.default_rng(1000 * pos0 + len(parent))
    prefix = [1] + [int(t) for t in rng.integers(0, V, max(pos0 - 1, 0))] if pos0 else []
    toks = [int(t) for t in rng.integers(0, V, len(parent))]
    fill_behind(b.eng, 0)
    if pos0:
        b.eng.prefill(prefix, 0)
        b.twin.prefill(prefix, 0)
    before = caches(b.eng)
    lg = b.eng.tree_forward(toks, parent, pos0)
    after = caches(b.eng)
    for got, old in zip(after, before):
        assert same_bits(got[:, :pos0], old[:, :pos0])
        assert (got[:, pos0 + 1:] == SENTINEL).all(), "a row other than the root's was written during the pass"
    leaf = max(range(len(parent)), key=lambda j: (dep[j], j))                     # the deepest node, walked last: the twin then holds its path
    for j in [j for j in range(len(parent)) if j != leaf] + [leaf]:
        for k, r in enumerate(path_to(parent, j)):
            b.twin.forward(toks[r], pos0 + k)
        assert same_bits(lg[j], b.twin.logits()), f"node {j} (depth {dep[j]}) of {tree} at pos0 {pos0}"
    ref = caches(b.twin)
    for got, want in zip(after, ref):
        assert same_bits(got[:, pos0], want[:, pos0])
    path = path_to(parent, leaf)
    b.eng.tree_commit(path, pos0)
    a = len(path) - 1
    for got, want, old in zip(caches(b.eng), ref, before):
        assert same_bits(got[:, :pos0], old[:, :pos0])
        assert same_bits(got[:, pos0:pos0 + a + 1], want[:, pos0:pos0 + a + 1])
        assert (got[:, pos0 + a + 1:] == SENTINEL).all()


def test_tree_commit_of_a_side_path(pairs):
    """the commit takes the rows of the path it is given, not the deepest or the first"""
    b = pairs("synth15m")
    rng = np.random.default_rng(3)
    pos0, V = 70, b.cfg.vocab_size
    prefix = [1] + [int(t) for t in rng.integers(0, V, pos0 - 1)]
    toks = [int(t) for t in rng.integers(0, V, len(FORK))]
    fill_behind(b.eng, 0)
    b.eng.prefill(prefix, 0); b.twin.prefill(prefix, 0)
    b.eng.tree_forward(toks, FORK, pos0)
    path = path_to(FORK, 11)
    for k, r in enumerate(path):
        b.twin.forward(toks[r], pos0 + k)
    b.eng.tree_commit(path, pos0)
    for got, want in zip(caches(b.eng), caches(b.twin)):
        assert same_bits(got[:, :pos0 + len(path)], want[:, :pos0 + len(path)])
        assert (got[:, pos0 + len(path):] == SENTINEL).all()


def test_tree_forward_and_commit_refusals(dev, pairs):
    b = pairs("ckpt_v2_q80_tied")
    L, m, eng = dev.lib, b.m, b.eng
    buf = C.c_void_p()
    assert L.rama_alloc_f32(dev.ctx, 16 * b.cfg.vocab_size, C.byref(buf)) == 0
    head = (dev.ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state))

    def fwd(toks, parent, pos0, n=None, head=head, out=buf):
        return L.rama_q8_tree_forward(*head, arr(toks), arr(parent), len(toks) if n is None else n, pos0, out)
    S = b.cfg.seq_len
    assert fwd([1, 2], [-1, 0], 0) == 0
    assert fwd([1, 2], [0, 0], 0) == EINVAL            # the root has no parent
    assert fwd([1, 2], [-1, 1], 0) == EINVAL           # parent < index
    assert fwd([1, 2], [-1, -1], 0) == EINVAL
    assert fwd([1, 2], [-1, 0], 0, n=0) == EINVAL
    assert fwd([1] * 17, [-1] + list(range(16)), 0, n=17) == EINVAL
    assert fwd([1, b.cfg.vocab_size], [-1, 0], 0) == EINVAL
    assert fwd([1, 2], [-1, 0], -1) == EINVAL
    assert fwd([1, 2], [-1, 0], S - 1) == EINVAL       # the child would sit at seq_len
    assert fwd([1, 2], [-1, 0], S - 2) == 0
    assert fwd([1, 2], [-1, 0], 0, out=None) == EINVAL
    assert fwd([1, 2], [-1, 0], 0, head=(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), None)) == EINVAL

    def commit(path, pos0, state=eng.state, n=None):
        return L.rama_q8_tree_commit(dev.ctx, C.byref(m.ccfg), C.byref(state), arr(path), len(path) if n is None else n, pos0)
    assert fwd([1, 2, 3, 4], [-1, 0, 0, 1], 2) == 0
    assert commit([0, 1, 3], 2) == 0
    assert commit([0], 2) == 0
    assert commit([0, 2, 3], 2) == EINVAL              # 3 is no child of 2
    assert commit([1, 3], 2) == EINVAL                 # a path starts at the root
    assert commit([0, 4], 2) == EINVAL
    assert commit([0, 1], 3) == EINVAL                 # not the pass's position
    assert commit([0, 1], 2, n=0) == EINVAL
    assert commit([0, 1], 2, state=b.twin.state) == EINVAL      # no tree pass on that run state
    assert L.rama_free(dev.ctx, buf) == 0


def test_tree_commit_after_the_state_is_gone(dev, pairs):
    import rama_amd
    b = pairs("ckpt_v2_q80_tied")
    e = rama_amd.Q8Engine(dev, b.m)
    e.tree_forward([1, 2], [-1, 0], 0)
    state = rama_amd._lib.rama_run_state.from_buffer_copy(e.state)
    e.free()
    assert dev.lib.rama_q8_tree_commit(dev.ctx, C.byref(b.m.ccfg), C.byref(state), arr([0, 1]), 2, 0) == EINVAL


# ------------------------------------------------------------------ 2. the chain

def begin_tree(dev, m, eng, ctx, max_new, B, R, T=0.0, P=0.9, u=0.0, stop=-1, K=7, N=3, hint=None, prefill=True):
    from rama_amd._lib import rama_q8_spec_plan
    if prefill and len(ctx) > 1:
        eng.prefill(ctx[:-1], 0)
    h = arr(hint or [])
    plan = rama_q8_spec_plan(T, P, u, max_new, stop, K, N, h if hint else None, len(hint or []))
    return dev.lib.rama_q8_spec_begin_tree(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state), arr(ctx), len(ctx), C.byref(plan), B, R)


def begin_linear(dev, m, eng, ctx, max_new, T=0.0, P=0.9, u=0.0, stop=-1, K=7, N=3, hint=None):
    from rama_amd._lib import rama_q8_spec_plan
    if len(ctx) > 1:
        eng.prefill(ctx[:-1], 0)
    h = arr(hint or [])
    plan = rama_q8_spec_plan(T, P, u, max_new, stop, K, N, h if hint else None, len(hint or []))
    return dev.lib.rama_q8_spec_begin(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state), arr(ctx), len(ctx), C.byref(plan))


def tree_stats(dev):
    from rama_amd._lib import rama_q8_spec_tree_report
    from rama_amd._host import _report
    r = rama_q8_spec_tree_report()
    assert dev.lib.rama_q8_spec_tree_stats(dev.ctx, C.byref(r)) == 0
    return _report(r)


def tree_sums(traj):
    hist, nodes = [0] * 16, [0] * 16
    for m, a, _, _, _ in traj:
        hist[a] += 1
        nodes[m] += 1
    lin = dict(steps=len(traj), rows_fed=sum(t[0] + 1 for t in traj), drafts=sum(t[0] for t in traj), accepted=sum(t[1] for t in traj),
               emitted=sum(t[2] for t in traj), accepted_hist=hist)
    tree = dict(off_trunk_accepted=sum(t[3] for t in traj), off_trunk_steps=sum(1 for t in traj if t[3]), nodes_hist=nodes)
    return lin, tree


def run_tree(b, ctx, max_new, want, twin_cache, B, R, hint, n_out=None, extra_steps=0, **plan):
    """the tree chain over b.eng for the replayed number of steps: tokens, both reports, the cache rows below the cursor against the
    twin's and the sentinel from the cursor on"""
    from rama_amd.q8 import spec_tree_replay
    dev = b.dev
    traj = spec_tree_replay(want, ctx, hint, plan.get("K", 7), plan.get("N", 3), B, R, max_new, plan.get("stop", -1))
    n_out = sum(t[2] for t in traj) if n_out is None else n_out
    fill_behind(b.eng, 0)
    assert begin_tree(dev, b.m, b.eng, ctx, max_new, B, R, hint=hint, **plan) == 0
    assert steps(dev, len(traj) + extra_steps) == 0
    assert tokens(dev) == want[:n_out]
    st, ts = stats(dev), tree_stats(dev)
    lin, tree = tree_sums(traj)
    lin["steps"] += extra_steps
    assert {k: st[k] for k in lin} == lin, (B, R, plan)
    assert {k: ts[k] for k in tree} == tree and ts["n_branch"] == B and ts["n_rows"] == R, (B, R, plan)
    cursor = len(ctx) - 1 + n_out
    assert st["finished"] == 1 and st["n_out"] == n_out and st["cursor"] == cursor
    for got, ref in zip(caches(b.eng), twin_cache):
        assert same_bits(got[:, :cursor], ref[:, :cursor]), (B, R, plan)
        assert (got[:, cursor:] == SENTINEL).all(), (B, R, plan)
    return st, traj


N_CTX, MAX_NEW, N_SEEDS = 9, 48, 24


def off_trunk_case(b, T):
    """the first seed whose solo run, with itself and its corrupted copy as hint, sends the two-branch replay off the trunk in at least 3
    steps at depth >= 2 and away from the one-branch replay's counters -> (ctx, want, twin_cache, hint parts)"""
    from rama_amd.q8 import spec_tree_replay
    V = b.cfg.vocab_size
    for seed in range(N_SEEDS):
        rng = np.random.default_rng(seed)
        ctx = [1] + [int(t) for t in rng.integers(0, V, N_CTX - 1)]
        want, _ = b.solo(ctx, MAX_NEW, T=T, u=0.37)
        hint = want + corrupt(want, V)
        two = spec_tree_replay(want, ctx, hint, 7, 3, 2, 16, MAX_NEW, None)
        one = spec_tree_replay(want, ctx, hint, 7, 3, 1, 16, MAX_NEW, None)
        if sum(1 for t in two if t[4]) >= 3 and tree_sums(two) != tree_sums(one):
            return ctx, want, b.solo(ctx, MAX_NEW, T=T, u=0.37)[1], (want, corrupt(want, V))
    return None


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("T", [0.0, 1.0])
@pytest.mark.parametrize("order", ["true_first", "copy_first"])
@pytest.mark.parametrize("which", ["synth15m", "long"])
def test_chain_equals_the_solo_run_and_the_replay(dev, pairs, which, order, T, graph):
    from rama_amd.q8 import spec_tree_replay
    b = pairs(which if T else which + "_untied")                # (the tied synthetic models' greedy runs repeat their last token)
    case = off_trunk_case(b, T)
    assert case is not None, f"no seed below {N_SEEDS} sends {which} (T {T}) off the trunk"
    ctx, want, twin_cache, (true, copy) = case
    hint = true + copy if order == "true_first" else copy + true
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        for B in (1, 2, 4):
            for R in (2, 8, 16):
                if B >= 2 and R == 16 and order == "true_first":
                    traj = spec_tree_replay(want, ctx, hint, 7, 3, B, R, MAX_NEW, None)
                    one = spec_tree_replay(want, ctx, hint, 7, 3, 1, R, MAX_NEW, None)
                    assert sum(1 for t in traj if t[4]) >= 3
                    assert tree_sums(traj) != tree_sums(one)
                st, _ = run_tree(b, ctx, MAX_NEW, want, twin_cache, B, R, hint, T=T, u=0.37)
                assert st["graph_captures"] == graph
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", GOLDEN)
def test_chain_on_the_golden_fixtures_to_the_end_of_the_window(dev, pairs, which, graph):
    """n_context + max_new == seq_len: the last steps have room < n_draft, and a row at seq_len would be out of bounds"""
    b = pairs(which)
    V, S = b.cfg.vocab_size, b.cfg.seq_len
    ctx = [1] + [int(t) for t in np.random.default_rng(5).integers(0, V, 3)]
    max_new = S - len(ctx)
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        for T in (0.0, 1.0):
            want, twin_cache = b.solo(ctx, max_new, T=T, u=0.37)
            for hint in (want + corrupt(want, V), corrupt(want, V) + want, None):
                for B, R in ((1, 2), (2, 8), (4, 16), (2, 16)):
                    st, _ = run_tree(b, ctx, max_new, want, twin_cache, B, R, hint, T=T, u=0.37, K=15)
                    assert st["graph_captures"] == graph
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


@pytest.mark.parametrize("T", [0.0, 1.0])
@pytest.mark.parametrize("which", ["synth15m", "ckpt_v2_q80_untied"])
def test_one_branch_is_the_linear_chain(dev, pairs, which, T):
    """n_branch = 1, n_rows = n_draft + 1: report and tokens equal to rama_q8_spec_begin's on the same inputs"""
    b = pairs(which)
    V = b.cfg.vocab_size
    ctx = [1] + [int(t) for t in np.random.default_rng(8).integers(0, V, 4)]
    max_new = min(40, b.cfg.seq_len - len(ctx))
    want, _ = b.solo(ctx, max_new, T=T, u=0.37)
    for K in (1, 7, 15):
        for hint in (want + corrupt(want, V), None):
            assert begin_linear(b.dev, b.m, b.eng, ctx, max_new, T=T, u=0.37, K=K, hint=hint) == 0
            assert steps(dev, max_new) == 0
            lin_toks, lin = tokens(dev), stats(dev)
            assert begin_tree(b.dev, b.m, b.eng, ctx, max_new, 1, K + 1, T=T, u=0.37, K=K, hint=hint) == 0
            assert steps(dev, max_new) == 0
            assert tokens(dev) == lin_toks == want
            tr, ts = stats(dev), tree_stats(dev)
            assert tr == lin
            assert ts["off_trunk_accepted"] == 0 and ts["off_trunk_steps"] == 0


def stop_case(b, where):
    """a stop token placed by the replay: `root` = a step's first pick, `off_trunk` = the pick of an accepted off-trunk node,
    `rejected` = the pick behind the last accepted node of a step whose tree went on -> (ctx, want, cache, hint, stop, n_out)"""
    from rama_amd.q8_replay import spec_tree_accept, spec_tree_draft
    case = off_trunk_case(b, 1.0)
    assert case is not None
    ctx, want, cache, (true, copy) = case
    hint = true + copy
    s, e = list(ctx), 0
    while e < MAX_NEW:
        tok, parent, depth = spec_tree_draft(hint, s, 7, 3, MAX_NEW - e - 1, 2, 16)
        right, picks = [True], [want[e]]
        for j in range(1, len(tok) + 1):
            ok = right[parent[j - 1]] and tok[j - 1] == want[e + depth[j - 1] - 1]
            right.append(ok)
            picks.append(want[e + depth[j - 1]] if ok and e + depth[j - 1] < MAX_NEW else -2)
        path, emitted, _fin = spec_tree_accept(tok, parent, picks, MAX_NEW - e, None)
        at = None
        if where == "root" and e > 0:
            at = e
        elif where == "off_trunk":
            offs = [k for k, j in enumerate(path) if j != k]
            at = e + offs[0] if offs else None
        elif where == "rejected" and len(path) - 1 < len(tok) and len(path) >= 2:
            at = e + len(path) - 1
        if at is not None and want[at] not in want[:at]:
            return ctx, want, cache, hint, want[at], at + 1
        s += emitted
        e += len(emitted)
    return None


@pytest.mark.parametrize("where", ["root", "off_trunk", "rejected"])
def test_stop_tokens(dev, pairs, where):
    b = pairs("synth15m")
    case = stop_case(b, where)
    assert case is not None, where
    ctx, want, cache, hint, stop, n_out = case
    st, traj = run_tree(b, ctx, MAX_NEW, want, cache, 2, 16, hint, n_out=n_out, T=1.0, u=0.37, stop=stop)
    assert st["n_out"] == n_out < MAX_NEW
    if where == "off_trunk":
        assert traj[-1][3] >= 1


def test_budget_ends_inside_an_off_trunk_run_and_idle_steps(dev, pairs):
    from rama_amd.q8 import spec_tree_replay
    b = pairs("synth15m")
    case = off_trunk_case(b, 1.0)
    ctx, want, _, (true, copy) = case
    hint = true + copy
    full = spec_tree_replay(want, ctx, hint, 7, 3, 2, 16, MAX_NEW, None)
    e, budget = 0, None
    for m, a, emit, off, deep in full:                           # a budget that ends in the middle of the first off-trunk run of >= 3 nodes
        if off >= 3:
            budget = e + emit - 1
            break
        e += emit
    assert budget is not None
    short, cache = b.solo(ctx, budget, T=1.0, u=0.37)
    assert short == want[:budget]
    st, traj = run_tree(b, ctx, budget, short, cache, 2, 16, hint, T=1.0, u=0.37, extra_steps=3)       # (three idle steps after the finish)
    assert traj[-1][3] >= 1 and st["n_out"] == budget


def test_bos_alone_and_one_token(dev, pairs):
    b = pairs("synth15m")
    want, cache = b.solo([1], 12)
    run_tree(b, [1], 12, want, cache, 2, 16, want + corrupt(want, b.cfg.vocab_size))
    want1, cache1 = b.solo([1, 5, 9], 1)
    st, traj = run_tree(b, [1, 5, 9], 1, want1, cache1, 4, 16, [5, 9, 3, 5, 9, 4])
    assert traj == [(0, 0, 1, 0, 0)]


def test_streaming_through_poll(dev, pairs):
    b = pairs("synth15m")
    case = off_trunk_case(b, 1.0)
    ctx, want, _, (true, copy) = case
    assert begin_tree(dev, b.m, b.eng, ctx, MAX_NEW, 2, 16, T=1.0, u=0.37, hint=true + copy) == 0
    got, fin = [], False
    for _ in range(MAX_NEW):
        assert steps(dev, 1) == 0
        stats(dev)                                               # (synchronises)
        new, fin = poll(dev, len(got))
        got += new
        assert got == want[:len(got)]
        if fin:
            break
    assert fin and got == want


def test_long_case_above_position_1024(dev, pairs):
    """steps whose rows sit above position 1 024: the staged score path, its groups of 64 timesteps holding cache rows and ancestors"""
    b = pairs("long")
    V = b.cfg.vocab_size
    rng = np.random.default_rng(2)
    ctx = [1] + [int(t) for t in rng.integers(0, V, 1029)]
    want, cache = b.solo(ctx, 40, T=1.0, u=0.37)
    for graph in (0, 1):
        assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
        try:
            st, traj = run_tree(b, ctx, 40, want, cache, 2, 16, want + corrupt(want, V), T=1.0, u=0.37)
            assert sum(t[3] for t in traj) >= 1
        finally:
            dev.lib.rama_set_graph_mode(dev.ctx, 0)


def test_refusals_of_begin_tree_and_tree_stats(dev, pairs):
    from rama_amd._lib import rama_q8_spec_tree_report
    b = pairs("ckpt_v2_q80_tied")
    ok = dict(B=2, R=8)
    assert begin_tree(dev, b.m, b.eng, [1, 2], 4, **ok) == 0
    for B, R, K in ((0, 8, 7), (5, 8, 7), (2, 1, 7), (2, 17, 7), (2, 8, 0), (2, 8, 16)):
        assert begin_tree(dev, b.m, b.eng, [1, 2], 4, B, R, K=K) == EINVAL, (B, R, K)
    assert begin_tree(dev, b.m, b.eng, [1, 2], 4, N=5, **ok) == EINVAL
    assert begin_tree(dev, b.m, b.eng, [1, 2], 0, **ok) == EINVAL
    assert begin_tree(dev, b.m, b.eng, [1, 2], b.cfg.seq_len, **ok) == EINVAL
    assert begin_tree(dev, b.m, b.eng, [1, b.cfg.vocab_size], 4, prefill=False, **ok) == EINVAL
    assert begin_tree(dev, b.m, b.eng, [1, 2], 4, T=-1.0, **ok) == EINVAL
    assert begin_tree(dev, b.m, b.eng, [1, 2], 4, stop=b.cfg.vocab_size, **ok) == EINVAL
    assert steps(dev, 1) == 0                                    # the refusals left the chain begun first as it was
    assert tree_stats(dev)["n_rows"] == 8
    assert begin_linear(dev, b.m, b.eng, [1, 2], 4) == 0
    assert dev.lib.rama_q8_spec_tree_stats(dev.ctx, C.byref(rama_q8_spec_tree_report())) == EINVAL
    assert dev.lib.rama_q8_spec_end(dev.ctx) == 0
    assert dev.lib.rama_q8_spec_tree_stats(dev.ctx, C.byref(rama_q8_spec_tree_report())) == EINVAL


def test_linear_after_tree_and_tree_after_linear(dev, pairs):
    b = pairs("synth15m")
    V = b.cfg.vocab_size
    ctx = [1, 7, 7, 3]
    want, cache = b.solo(ctx, 20)
    hint = want + corrupt(want, V)
    assert dev.lib.rama_set_graph_mode(dev.ctx, 1) == 0
    try:
        for _ in range(2):
            run_tree(b, ctx, 20, want, cache, 2, 16, hint)
            assert begin_linear(dev, b.m, b.eng, ctx, 20, hint=hint) == 0
            assert steps(dev, 20) == 0
            assert tokens(dev) == want
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)


def test_lifetimes(dev, golden_dir):
    """rama_q8_model_free / rama_state_free end the chain: _steps refuses afterwards"""
    import rama_amd
    for gone in ("model", "state"):
        m = rama_amd.Q8Model.load(dev, golden_dir / "ckpt_v2_q80_tied.bin")
        e = rama_amd.Q8Engine(dev, m)
        assert begin_tree(dev, m, e, [1, 2], 6, 2, 8) == 0
        assert steps(dev, 1) == 0
        if gone == "model":
            m.free()
        else:
            e.free()
        assert steps(dev, 1) == EINVAL
        assert dev.lib.rama_q8_spec_end(dev.ctx) == 0
        e.free(); m.free()


def test_generate_spec_with_tree_drafts(dev, pairs):
    b = pairs("synth15m")
    V = b.cfg.vocab_size
    ctx = [1, 4, 4, 8]
    want, _ = b.solo(ctx, 24, T=1.0, u=0.37)
    seen = []
    got = b.eng.generate_spec(ctx, 24, 1.0, 0.9, 0.37, hint=want + corrupt(want, V), n_branch=2, tree_rows=16, on_token=lambda i, t: seen.append((i, t)))
    assert got == want and seen == list(enumerate(want))
    assert b.eng.spec_stats["n_branch"] == 2 and b.eng.spec_stats["off_trunk_accepted"] >= 0
    with pytest.raises(ValueError):
        b.eng.generate_spec(ctx, 24, n_branch=5)
    with pytest.raises(ValueError):
        b.eng.generate_spec(ctx, 24, n_branch=2, tree_rows=1)
    with pytest.raises(ValueError):
        b.eng.generate_spec(ctx, 24, n_branch=2, n_draft=0)
