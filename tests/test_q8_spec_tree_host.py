"""The tree drafting rule and the tree accept rule on the CPU (no GPU): rama_q8_spec_tree_draft / rama_q8_spec_tree_accept (host-only
entries of the C ABI) against rama_amd.q8_replay's restatements and against brute-force restatements written here, on dense random
texts over small vocabularies (occurrences abound), and on the named edges of DESIGN.md 8.13."""
import ctypes as C
import itertools

import numpy as np
import pytest

from rama_amd import _lib
from rama_amd import q8 as Q
from rama_amd import q8_replay as R

EINVAL = -1
NEW = ("rama_q8_spec_begin_tree", "rama_q8_spec_tree_stats", "rama_q8_spec_tree_draft", "rama_q8_spec_tree_accept", "rama_q8_tree_forward",
       "rama_q8_tree_commit")


def test_the_abi_exports_the_tree_entries():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None, name


# ------------------------------------------------------------------ brute force

def brute_draft(hint, seq, K, N, room, B, Rn):
    """the rule from its statement: every occurrence's key, sorted; the branches as token lists; the trie as a dict of paths"""
    cap, L = min(K, room), len(seq)
    if cap <= 0:
        return [], [], []
    for n in range(min(N, L), 0, -1):
        keys = [(1, e) for e in range(n, len(hint) + 1) if hint[e - n:e] == seq[L - n:]]
        keys += [(0, e) for e in range(n, L) if seq[e - n:e] == seq[L - n:]]
        if keys:
            break
    else:
        return [], [], []
    keys.sort(reverse=True)
    nodes = {(): 0}                                               # path of tokens -> node index
    tok, parent, depth = [], [], []
    for in_hint, e in keys[:B]:
        text = hint if in_hint else seq
        branch = text[e:e + cap]
        for i in range(1, len(branch) + 1):
            p = tuple(branch[:i])
            if p in nodes:
                continue
            if len(tok) >= Rn - 1:
                return tok, parent, depth
            nodes[p] = len(tok) + 1
            tok.append(branch[i - 1]); parent.append(nodes[p[:-1]]); depth.append(i)
    return tok, parent, depth


def brute_accept(tok, parent, picks, remaining, stop):
    kids = {}
    for j, (t, p) in enumerate(zip(tok, parent), start=1):
        assert (p, t) not in kids
        kids[(p, t)] = j
    path, out = [0], [picks[0]]
    while True:
        if out[-1] == stop or len(out) >= remaining or (path[-1], out[-1]) not in kids:
            break
        path.append(kids[(path[-1], out[-1])])
        out.append(picks[path[-1]])
    return path, len(out), out[-1] == stop or len(out) >= remaining


def check_tree(tok, parent, depth, Rn):
    assert len(tok) == len(parent) == len(depth) <= Rn - 1
    seen = set()
    for j, (t, p, d) in enumerate(zip(tok, parent, depth), start=1):
        assert 0 <= p < j and d == (depth[p - 1] if p else 0) + 1
        assert (p, t) not in seen, "children of one node have distinct tokens"
        seen.add((p, t))


# ------------------------------------------------------------------ random texts

@pytest.mark.parametrize("vocab", [2, 3, 5])
def test_draft_equals_the_restatements_on_dense_texts(vocab):
    rng = np.random.default_rng(vocab)
    for _ in range(400):
        hint = [int(t) for t in rng.integers(0, vocab, int(rng.integers(0, 40)))]
        seq = [int(t) for t in rng.integers(0, vocab, int(rng.integers(1, 40)))]
        K, N, room = int(rng.integers(0, 16)), int(rng.integers(1, 5)), int(rng.integers(-1, 20))
        B, Rn = int(rng.integers(1, 5)), int(rng.integers(2, 17))
        got = Q.spec_tree_draft(hint, seq, K, N, room, B, Rn)
        assert got == R.spec_tree_draft(hint, seq, K, N, room, B, Rn) == brute_draft(hint, seq, K, N, room, B, Rn), (hint, seq, K, N, room, B, Rn)
        check_tree(*got, Rn)
        if B == 1 and Rn == K + 1 and K >= 1:                      # the linear chain's draft, as a line
            d = R._draft_py(hint, seq, K, N, room)
            assert got == (d, list(range(len(d))), list(range(1, len(d) + 1)))
        trunk = R._draft_py(hint, seq, K, N, room)[:Rn - 1]        # branch 0 is today's draft: index == depth
        assert got[0][:len(trunk)] == trunk and got[2][:len(trunk)] == list(range(1, len(trunk) + 1))


@pytest.mark.parametrize("vocab", [2, 4])
def test_accept_equals_the_restatements_on_random_trees(vocab):
    rng = np.random.default_rng(10 + vocab)
    for _ in range(600):
        hint = [int(t) for t in rng.integers(0, vocab, 40)]
        seq = [int(t) for t in rng.integers(0, vocab, 12)]
        tok, parent, depth = R.spec_tree_draft(hint, seq, 15, 2, 15, int(rng.integers(1, 5)), int(rng.integers(2, 17)))
        picks = [int(t) for t in rng.integers(0, vocab, len(tok) + 1)]
        remaining, stop = int(rng.integers(1, 18)), int(rng.integers(-1, vocab))
        got = Q.spec_tree_accept(tok, parent, picks, stop, remaining)
        path, out, fin = R.spec_tree_accept(tok, parent, picks, remaining, stop)
        assert got == (path, len(out), fin) == brute_accept(tok, parent, picks, remaining, stop), (tok, parent, picks, remaining, stop)
        assert all(depth[j - 1] == k for k, j in enumerate(path) if k)


# ------------------------------------------------------------------ named edges

def both(hint, seq, K, N, room, B, Rn):
    got = Q.spec_tree_draft(hint, seq, K, N, room, B, Rn)
    assert got == R.spec_tree_draft(hint, seq, K, N, room, B, Rn) == brute_draft(hint, seq, K, N, room, B, Rn)
    return got


def test_more_branches_than_occurrences():
    assert both([7, 8, 1, 2], [5, 7, 8], 7, 2, 9, 4, 16) == ([1, 2], [0, 1], [1, 2])


def test_identical_continuations_add_no_node():
    assert both([7, 8, 1, 2, 3, 9, 7, 8, 1, 2, 3, 9], [7, 8], 3, 2, 9, 2, 16) == ([1, 2, 3], [0, 1, 2], [1, 2, 3])


def test_branches_diverging_at_depth_0_in_the_middle_and_in_the_last_token():
    assert both([7, 1, 2, 3, 9, 7, 4, 5, 6], [7], 3, 1, 9, 2, 16) == ([4, 5, 6, 1, 2, 3], [0, 1, 2, 0, 4, 5], [1, 2, 3, 1, 2, 3])
    assert both([7, 1, 2, 3, 9, 7, 1, 5, 6], [7], 3, 1, 9, 2, 16) == ([1, 5, 6, 2, 3], [0, 1, 2, 1, 4], [1, 2, 3, 2, 3])
    assert both([7, 1, 2, 3, 9, 7, 1, 2, 6], [7], 3, 1, 9, 2, 16) == ([1, 2, 6, 3], [0, 1, 2, 2], [1, 2, 3, 3])


def test_the_row_budget_runs_out_inside_a_branch():
    assert both([7, 1, 2, 3, 9, 7, 4, 5, 6], [7], 3, 1, 9, 2, 5) == ([4, 5, 6, 1], [0, 1, 2, 0], [1, 2, 3, 1])
    assert both([7, 1, 2, 3, 9, 7, 4, 5, 6], [7], 3, 1, 9, 2, 3) == ([4, 5], [0, 1], [1, 2])
    # everything stops: a third branch that would only need existing nodes plus one more gets nothing either
    assert both([7, 4, 8, 9, 7, 1, 2, 9, 7, 4, 5], [7], 2, 1, 9, 3, 4) == ([4, 5, 1], [0, 1, 0], [1, 2, 1])


def test_an_occurrence_at_the_very_end_of_the_hint_has_an_empty_continuation():
    assert both([1, 2, 9, 7], [7], 3, 1, 9, 1, 16) == ([], [], [])            # it still decides: no fall-through
    assert both([7, 1, 2, 9, 7], [7], 3, 1, 9, 2, 16) == ([1, 2, 9], [0, 1, 2], [1, 2, 3])      # ... and the next occurrence is branch 1


def test_hint_occurrences_come_before_sequence_occurrences():
    assert both([7, 1], [7, 2, 3, 7], 2, 1, 9, 2, 16) == ([1, 2, 3], [0, 0, 2], [1, 1, 2])
    assert both([7, 1], [7, 2, 3, 7], 2, 1, 9, 1, 16) == ([1], [0], [1])


def test_room_0_and_1():
    assert both([7, 1, 2, 7, 3, 4], [7], 7, 1, 0, 4, 16) == ([], [], [])
    assert both([7, 1, 2, 7, 3, 4], [7], 7, 1, 1, 4, 16) == ([3, 1], [0, 0], [1, 1])
    assert both([7, 1, 2, 7, 3, 4], [7], 0, 1, 5, 4, 16) == ([], [], [])


def test_a_stop_token_on_an_off_trunk_node():
    tok, parent = [4, 5, 6, 1, 2, 3], [0, 1, 2, 0, 4, 5]
    picks = [1, 0, 0, 0, 2, 9, 8]                                  # root -> 1 (node 4) -> 2 (node 5) -> pick 9
    for got in (Q.spec_tree_accept(tok, parent, picks, 9, 10), brute_accept(tok, parent, picks, 10, 9)):
        assert got == ([0, 4, 5], 3, True)
    assert Q.spec_tree_accept(tok, parent, picks, 2, 10) == ([0, 4], 2, True)      # the stop token is emitted, its node is not entered
    assert Q.spec_tree_accept(tok, parent, picks, 1, 10) == ([0], 1, True)         # on the root's pick
    assert Q.spec_tree_accept(tok, parent, picks, None, 10) == ([0, 4, 5], 3, False)


def test_a_budget_that_ends_inside_an_off_trunk_run():
    tok, parent = [4, 5, 6, 1, 2, 3], [0, 1, 2, 0, 4, 5]
    picks = [1, 0, 0, 0, 2, 3, 8]
    assert Q.spec_tree_accept(tok, parent, picks, None, 10) == ([0, 4, 5, 6], 4, False)
    assert Q.spec_tree_accept(tok, parent, picks, None, 4) == ([0, 4, 5, 6], 4, True)
    assert Q.spec_tree_accept(tok, parent, picks, None, 3) == ([0, 4, 5], 3, True)
    assert Q.spec_tree_accept(tok, parent, picks, None, 1) == ([0], 1, True)


def test_one_branch_replays_as_the_linear_chain():
    """B = 1, R = K + 1: the drafts and the replay's counters are _draft_py's / spec_replay's (no stop token inside a matched run:
    there the tree's a stops at the stop token, the linear rule's counts on)"""
    rng = np.random.default_rng(4)
    for _ in range(40):
        V = int(rng.integers(2, 6))
        ref = [int(t) for t in rng.integers(0, V, 48)]
        ctx = [int(t) for t in rng.integers(0, V, int(rng.integers(1, 6)))]
        hint = ref + [(t + 1) % V if i % 5 == 4 else t for i, t in enumerate(ref)] if rng.integers(0, 2) else None
        K, N = int(rng.integers(1, 16)), int(rng.integers(1, 5))
        tree = R.spec_tree_replay(ref, ctx, hint, K, N, 1, K + 1, 48, None)
        assert [t[:3] for t in tree] == R.spec_replay(ref, ctx, hint, K, N, 48, None)
        assert all(t[3] == 0 for t in tree)


def test_the_replay_leaves_the_trunk_on_a_corrupted_copy():
    """DESIGN.md 8.13's example: a random 48-token output, the true text then a copy with every fifth token changed as hint"""
    rng = np.random.default_rng(0)
    ref = [int(t) for t in rng.integers(0, 200, 48)]
    hint = ref + [(t + 1) % 200 if i % 5 == 4 else t for i, t in enumerate(ref)]
    one = R.spec_tree_replay(ref, [1], hint, 7, 3, 1, 16, 48, None)
    two = R.spec_tree_replay(ref, [1], hint, 7, 3, 2, 16, 48, None)
    assert (len(one), len(two)) == (11, 7)
    assert sum(1 for t in two if t[4]) == 3 and sum(t[3] for t in two) >= 17
    assert sum(t[2] for t in one) == sum(t[2] for t in two) == 48


# ------------------------------------------------------------------ refusals

def test_every_refusal_of_the_two_host_entries():
    L = _lib.load()
    i32 = lambda v: (C.c_int32 * max(len(v), 1))(*v)      # noqa: E731
    out = [(C.c_int32 * 16)() for _ in range(3)]
    ok = dict(hint=i32([7, 1]), n_hint=2, seq=i32([7]), L=1, K=7, N=2, room=5, B=2, R=16, o=out)

    def draft(**kw):
        a = dict(ok, **kw)
        return L.rama_q8_spec_tree_draft(a["hint"], a["n_hint"], a["seq"], a["L"], a["K"], a["N"], a["room"], a["B"], a["R"], *a["o"])
    assert draft() == 1
    for bad in (dict(seq=None), dict(L=0), dict(n_hint=-1), dict(hint=None), dict(K=-1), dict(K=16), dict(N=0), dict(N=5), dict(B=0), dict(B=5),
                dict(R=1), dict(R=17), dict(o=[None, out[1], out[2]]), dict(o=[out[0], None, out[2]]), dict(o=[out[0], out[1], None])):
        assert draft(**bad) == EINVAL, bad
    assert draft(hint=None, n_hint=0) == 0

    def accept(tok, parent, m, picks, stop=-1, remaining=4):
        return L.rama_q8_spec_tree_accept(tok, parent, m, picks, stop, remaining, None, None, None)
    assert accept(i32([4, 5]), i32([0, 1]), 2, i32([4, 5, 6])) == 3
    assert accept(None, None, 0, i32([4])) == 1
    assert accept(i32([4, 5]), i32([0, 1]), 2, None) == EINVAL
    assert accept(i32([4, 5]), i32([0, 1]), -1, i32([4, 5, 6])) == EINVAL
    assert accept(i32([4] * 16), i32([0] * 16), 16, i32([4] * 17)) == EINVAL
    assert accept(None, i32([0, 1]), 2, i32([4, 5, 6])) == EINVAL
    assert accept(i32([4, 5]), None, 2, i32([4, 5, 6])) == EINVAL
    assert accept(i32([4, 5]), i32([0, 1]), 2, i32([4, 5, 6]), remaining=0) == EINVAL
    assert accept(i32([4, 5]), i32([0, 2]), 2, i32([4, 5, 6])) == EINVAL        # parent[j] < j
    assert accept(i32([4, 5]), i32([-1, 1]), 2, i32([4, 5, 6])) == EINVAL


def test_python_checks_of_generate_spec():
    for bad in (dict(n_branch=0), dict(n_branch=5), dict(tree_rows=1), dict(tree_rows=17)):
        with pytest.raises(ValueError):
            Q.spec_tree_check(None, 7, bad.get("n_branch", 1), bad.get("tree_rows", 16))
    with pytest.raises(ValueError):
        Q.spec_tree_check(None, 0, 2, 16)
    with pytest.raises(ValueError):
        Q.spec_tree_check(object(), 7, 2, 16)
    assert Q.spec_tree_check(None, 7, 2, 16) == (2, 16)
    assert list(itertools.islice(iter(R.spec_tree_draft([], [1], 7, 3, 5, 2, 16)), 3)) == [[], [], []]
