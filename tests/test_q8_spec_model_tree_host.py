"""Trees from a draft model on the host: the C statements of the static shape and of the candidate order
(rama_q8_spec_model_tree_shape / _candidates) against their Python restatements, and spec_model_tree_replay against a row-by-row
restatement on scripted draft models.  No GPU."""
import numpy as np
import pytest

from rama_amd import q8, q8_replay

V = 37


# ------------------------------------------------------------------ the shape

def test_the_c_shape_is_the_restatement_and_keeps_its_promises():
    for cap in range(16):
        for B in range(1, 5):
            for R in range(2, 17):
                par, dep, rank = q8_replay.spec_model_tree_shape(cap, B, R)
                assert tuple(map(list, q8.spec_model_tree_shape(cap, B, R))) == (par, dep, rank), (cap, B, R)
                m = len(par)
                assert m <= R - 1
                parent, depth = [-1] + par, [0] + dep
                for j in range(1, m + 1):
                    assert 0 <= parent[j] < j and depth[j] == depth[parent[j]] + 1 <= cap
                trunk = min(cap, R - 1)
                assert [(parent[j], depth[j], rank[j - 1]) for j in range(1, trunk + 1)] == [(j - 1, j, 0) for j in range(1, trunk + 1)]
                assert all(depth[j] != j for j in range(trunk + 1, m + 1))          # everything behind the trunk is off it
                assert max([depth.count(d) for d in range(1, 16)] + [0]) <= 15
                if B == 1:
                    assert m == trunk and par == list(range(trunk))
                # children of one node have distinct ranks; a trunk node's are 0..B-1, any other node has rank 0 alone
                for p in range(m + 1):
                    kids = [rank[j - 1] for j in range(1, m + 1) if parent[j] == p]
                    assert kids == sorted(set(kids)) and (p == depth[p] or kids in ([], [0]))


def test_the_example_of_the_header():
    par, dep, rank = q8.spec_model_tree_shape(4, 2, 16)
    assert len(par) == 14
    assert par == [0, 1, 2, 3, 0, 1, 5, 2, 6, 7, 3, 8, 9, 10]
    assert dep == [1, 2, 3, 4, 1, 2, 2, 3, 3, 3, 4, 4, 4, 4]
    assert rank == [0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 0]


def test_shape_refusals():
    L = q8.load()
    import ctypes as C
    buf = [(C.c_int32 * 16)() for _ in range(3)]
    for cap, B, R in [(-1, 1, 2), (16, 1, 2), (1, 0, 2), (1, 5, 2), (1, 1, 1), (1, 1, 17)]:
        assert L.rama_q8_spec_model_tree_shape(cap, B, R, *buf) < 0
    assert L.rama_q8_spec_model_tree_shape(1, 1, 2, None, buf[1], buf[2]) < 0


# ------------------------------------------------------------------ the candidates

def numpy_candidates(row, rank0, n):
    bits = np.asarray(row, np.float32).view(np.uint32).astype(np.uint64)
    hi = np.where(bits >> np.uint64(31), bits ^ np.uint64(0xFFFFFFFF), bits ^ np.uint64(0x80000000))
    key = (hi << np.uint64(32)) | np.arange(len(row), dtype=np.uint64)
    order = [int(i) for i in np.argsort(key)[::-1] if int(i) != rank0]
    return order[:n]


def candidate_rows():
    rng = np.random.default_rng(3)
    plain = rng.standard_normal(V).astype(np.float32)
    ties = np.round(plain * 2) / 2
    zeros = plain.copy(); zeros[[3, 9, 20]] = 0.0; zeros[[4, 30]] = -0.0; zeros[zeros > 0] *= -1      # the maxima are +0.0 and -0.0
    infs = plain.copy(); infs[[5, 6]] = np.inf; infs[[7, 36]] = -np.inf
    nans = plain.copy(); nans[2] = np.nan; nans[11] = -np.nan
    flat = np.zeros(V, np.float32)
    return dict(plain=plain, ties=ties.astype(np.float32), zeros=zeros, infs=infs, nans=nans, flat=flat)


@pytest.mark.parametrize("name", list(candidate_rows()))
def test_the_c_candidates_are_the_restatement(name):
    row = candidate_rows()[name]
    top = numpy_candidates(row, -1, V)
    for rank0 in (top[0], top[1], top[2], top[5], top[-1], 0, V - 1):       # inside and outside the top B
        for n in range(4):
            want = numpy_candidates(row, rank0, n)
            assert q8.spec_model_tree_candidates(row, rank0, n) == want, (name, rank0, n)
            assert q8_replay.spec_model_tree_candidates(row, rank0, n) == want, (name, rank0, n)
            assert rank0 not in want and len(set(want)) == n


def test_ties_take_the_higher_index_and_negative_zero_sorts_below_zero():
    row = np.full(V, -1.0, np.float32); row[[3, 8]] = 0.0; row[12] = -0.0
    assert q8.spec_model_tree_candidates(row, 8, 3) == [3, 12, V - 1]
    assert q8.spec_model_tree_candidates(row, 0, 3) == [8, 3, 12]


def test_candidate_refusals():
    row = np.zeros(3, np.float32)
    for rank0, n in [(-1, 1), (3, 1), (0, -1), (0, 4), (0, 3)]:
        with pytest.raises(Exception):
            q8.spec_model_tree_candidates(row, rank0, n)


# ------------------------------------------------------------------ the replay on scripted draft models

def greedy(row):
    row = np.asarray(row)
    return int(len(row) - 1 - np.argmax(row[::-1]))               # the LAST maximal index


def scripted(ref_full, n_context, wrong_at=None, second_at=None, always_wrong=False):
    """a draft model as logits_fn: after a prefix of length n its first choice is the reference's token at n (ref_full = context ++
    reference) -- or, at the emitted indices in wrong_at / always, a wrong one; at those in second_at the right token is its SECOND choice"""
    wrong_at, second_at = set(wrong_at or ()), set(second_at or ())

    def fn(prefix):
        n = len(prefix)
        right = ref_full[n] if n < len(ref_full) else 0
        row = np.zeros(V, np.float32)
        e = n - n_context
        if always_wrong or e in wrong_at:
            row[(right + 1) % V] = 3.0; row[(right + 2) % V] = 2.0
        elif e in second_at:
            row[(right + 1) % V] = 3.0; row[right] = 2.0
        else:
            row[right] = 3.0; row[(right + 5) % V] = 2.0
        return row
    return fn


def restated(ref, logits_fn, ctx, K, B, R, max_new, stop):
    """the chain row by row: every level's rows fed in order, every fed row's children picked, the accept walk, the cursors"""
    s, e, Dc, out, fin = list(ctx), 0, len(ctx) - 1, [], False
    while not fin:
        L, P, remaining = len(s), len(s) - 1, max_new - e
        cap = max(min(K, remaining - 1), 0)
        gap = P - Dc
        assert gap in (0, 1)
        par, dep, rank = q8_replay.spec_model_tree_shape(cap, B, R)
        parent, depth, rank = [-1] + par, [0] + dep, [0] + rank
        tok = [s[-1]] + [None] * len(par)
        for level in range(1, cap + 1):                            # pass `level` feeds the nodes of depth level - 1
            for p in [j for j in range(len(tok)) if depth[j] == level - 1]:
                chain, c = [], p
                while c > 0:
                    chain.insert(0, tok[c]); c = parent[c]
                row = logits_fn(s + chain)
                first = greedy(row)
                order = [first] + [t for t in sorted(range(V), key=lambda i: (row[i], i), reverse=True) if t != first]
                for j in range(1, len(tok)):
                    if parent[j] == p:
                        tok[j] = order[rank[j]]
        # the target's picks: the reference behind every right path
        cur, path, emitted = 0, [0], [ref[e]]
        while emitted[-1] != stop and len(emitted) < remaining:
            kids = [j for j in range(1, len(tok)) if parent[j] == cur and tok[j] == emitted[-1]]
            if not kids:
                break
            cur = kids[0]; path.append(cur); emitted.append(ref[e + len(path) - 1])
        fin = len(emitted) >= remaining or emitted[-1] == stop
        a = len(path) - 1
        s += emitted; e += len(emitted)
        if cap:
            Dc = min(L + min(a, cap - 1), len(s))
        out.append((cap, tok, a, path, emitted, gap if cap else 0))
    return out, (len(s) - 1, Dc)


def check_replay(ref, fn, ctx, K, B, R, max_new, stop=None):
    got, cursors = q8_replay.spec_model_tree_replay(ref, fn, ctx, K, B, R, max_new, stop, greedy)
    want, wcursors = restated(ref, fn, ctx, K, B, R, max_new, -1 if stop is None else stop)
    assert [(cap, tok, a, path, em, cu) for cap, tok, _, _, _, a, path, em, cu in got] == want
    assert cursors == wcursors
    # P - Dc stays in {0, 1}: the replay raises otherwise; the catch-up row follows exactly a step that accepted a leaf of depth cap
    for prev, step in zip(got, got[1:]):
        if step[0]:
            assert step[8] == (1 if prev[0] and prev[5] == prev[0] else 0)
    return got


CTX = [1, 7, 7, 3]
REF = [int(t) for t in np.random.default_rng(11).integers(0, V, 24)]
GRID = [(1, 2, 16), (4, 2, 16), (3, 3, 16), (7, 2, 8), (7, 4, 2), (4, 1, 5)]


@pytest.mark.parametrize("K,B,R", GRID)
def test_replay_always_right_on_the_trunk(K, B, R):
    got = check_replay(REF, scripted(CTX + REF, len(CTX)), CTX, K, B, R, 24)
    full = [s for s in got if s[0] == K]
    assert full and all(s[5] == min(K, R - 1) and s[6] == list(range(s[5] + 1)) for s in full)


@pytest.mark.parametrize("K,B,R", [(4, 2, 16), (3, 3, 16), (7, 2, 12)])      # (R = 12: the trunk's 7 nodes leave room for 4 on the sides)
@pytest.mark.parametrize("at", [0, 1, 2])
def test_replay_right_only_as_rank_1_at_a_chosen_depth(K, B, R, at):
    got = check_replay(REF, scripted(CTX + REF, len(CTX), second_at=[at]), CTX, K, B, R, 24)
    first = got[0]
    assert first[6][at + 1] != at + 1                              # the accepted node of depth at + 1 is off the trunk ...
    par, dep, _ = q8_replay.spec_model_tree_shape(K, B, R)
    deepest = max(d for j, d in enumerate(dep, 1) if d > at and _under(par, j, first[6][at + 1]))
    assert first[5] == deepest                                     # ... and its first-choice chain is followed as deep as R lets it go


def _under(par, j, top):
    while j > 0:
        if j == top:
            return True
        j = par[j - 1]
    return False


@pytest.mark.parametrize("K,B,R", GRID)
def test_replay_always_wrong(K, B, R):
    got = check_replay(REF, scripted(CTX + REF, len(CTX), always_wrong=True), CTX, K, B, R, 12)
    assert all(s[5] == 0 and s[8] == 0 for s in got) and len(got) == 12


def test_replay_budget_and_stop_cuts():
    fn = scripted(CTX + REF, len(CTX))
    got = check_replay(REF, fn, CTX, 4, 2, 16, 7)                  # 5 + 2: the budget cuts the second step's tree to cap = 1
    assert [s[0] for s in got] == [4, 1] and sum(len(s[7]) for s in got) == 7
    stop = REF[2]
    got = check_replay(REF, fn, CTX, 7, 2, 16, 24, stop=stop)      # the stop token is emitted inside an accepted path
    assert got[-1][7][-1] == stop and sum(len(s[7]) for s in got) == REF.index(stop) + 1
    got = check_replay(REF, fn, CTX, 4, 3, 16, 1)                  # a budget of one: cap = 0, nothing drafted
    assert [(s[0], s[5], s[8]) for s in got] == [(0, 0, 0)]


@pytest.mark.parametrize("K", [1, 2, 7])
def test_one_branch_is_the_linear_chain(K):
    """B = 1, R = K + 1: the steps of spec_model_replay on the same inputs (no stop token: section 8.13's difference in `a`)"""
    for kw in (dict(), dict(wrong_at=[3, 4, 9]), dict(always_wrong=True)):
        fn = scripted(CTX + REF, len(CTX), **kw)

        def draft_fn(prefix, n):
            out = []
            for _ in range(n):
                out.append(greedy(fn(list(prefix) + out)))
            return out
        tree, (_, dc) = q8_replay.spec_model_tree_replay(REF, fn, CTX, K, 1, K + 1, 20, None, greedy)
        line, cursor = q8_replay.spec_model_replay(REF, draft_fn, CTX, K, 20, None)
        assert [(s[0], s[5], len(s[7]), s[8]) for s in tree] == line and dc == cursor
