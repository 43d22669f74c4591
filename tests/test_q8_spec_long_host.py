"""The drafting rule on texts longer than a drafting workgroup (no GPU): rama_q8_spec_draft, rama_amd.q8._draft_py and the rule
restated in tests/spec_long_cases.py agree on every long case and on random texts of up to 3000 tokens; every case with a kill
list is discriminating -- each of its mutants replays to another trajectory than the true rule --; spec_replay and
serve_spec_replay over the long cases equal the restated replay step by step.  The reference run is synthetic here: 24 distinct
tokens that depend on nothing but the context's length."""
import numpy as np
import pytest

from tests import spec_long_cases as SL

MAX_NEW = 24
CHAINS = [(1024, 0, SL.ALL), (256, 1, SL.SERVE), (256, 0, SL.ALL)]
EVERY = [(threads, lead) + c for threads, lead, table in CHAINS for c in table]


def synthetic_solo(n):
    def solo(ctx):
        rng = np.random.default_rng(7 * len(ctx) + n)
        return [int(t) for t in rng.choice(np.arange(2, 512), MAX_NEW, replace=False)]
    return solo


_settled = {}


def settled(threads, lead, name, n, ngram):
    key = (threads, lead, name, n, ngram)
    if key not in _settled:
        _settled[key] = SL.settle(name, n, ngram, threads, lead, MAX_NEW, synthetic_solo(n))
    return _settled[key]


def ids(c):
    return f"t{c[0]}-lead{c[1]}-{SL.case_id(c[2:])}"


def test_the_table_is_whole():
    assert {name for name, _ in SL.TABLE} == set(SL.KILLS) and all(set(k) <= set(SL.MUTANTS) for k in SL.KILLS.values())
    for group in "HSP":
        assert any(ngram == 4 for name, pairs in SL.TABLE if name[0] == group for _, ngram in pairs), group
    assert {n for _, pairs in SL.TABLE for n, _ in pairs} == {1, 2, 3, 4}
    want = {"H-wave", "H-next", "H-sweep", "H-third", "H-end", "H-cut", "S-sweep", "S-last", "P-hint", "P-long", "P-fall"}
    assert {c[0] for c in SL.SERVE} == want


@pytest.mark.parametrize("case", EVERY, ids=ids)
def test_the_three_rules_agree_and_the_case_is_discriminating(case):
    from rama_amd.q8 import _draft_py, spec_draft
    threads, lead, name, n, ngram = case
    c, ref = settled(*case)
    assert SL.undiscriminated(c, ref, MAX_NEW) == []               # (settle has asserted it; said again where it is read)
    assert len(c.kill) > 0 or name == "H-first"
    # what the placement is for: the planted occurrences sit in the threads and sweeps the table names
    text = c.hint if name[0] in "HP" and name != "P-long" else c.context
    gram = (c.context + ref[:lead])[-n:]
    ends = SL.occurrence_ends(text, gram, (n, len(text)), threads)
    slots = {((e - n) // threads, (e - n) % threads) for e in ends}
    expect = {"H-wave": {(0, threads - 1), (0, 5)}, "H-next": {(0, 64), (0, 20)}, "H-sweep": {(1, 3), (0, threads - 40)},
              "H-third": {(2, 70)}, "H-first": {(0, 0)}, "H-end": {(1, 30)}, "H-cut": {(1, 10), (0, 12)},
              "S-wave": {(0, threads - 1), (0, 5)}, "S-sweep": {(1, 3), (0, threads - 40)}, "S-third": {(2, 70)}, "P-hint": {(0, 7)},
              "P-fall": {(2, 70)}}
    if name in expect:
        assert expect[name] <= slots, (slots, expect[name])
    if name in ("P-hint", "P-long"):
        assert 2000 in SL.occurrence_ends(c.context, gram, (n, len(c.context)), threads)
    # every state the chain's text passes through: the library, the package's Python rule and the restated one
    s, e = list(c.context), 0
    for k, (n_d, a, emit) in enumerate(SL.replay(ref, c.context, c.hint, c.n_draft, ngram, MAX_NEW, threads, lead=lead)):
        room = MAX_NEW - e - 1
        want = SL.draft(c.hint, s, c.n_draft, ngram, room, threads)
        assert spec_draft(c.hint, s, c.n_draft, ngram, room) == want == _draft_py(c.hint, s, c.n_draft, ngram, room), (case, k)
        assert k < lead or len(want) == n_d
        s += ref[e:e + emit]
        e += emit
    assert e == MAX_NEW


def test_model_free_cases_show_the_draft_counts_they_are_for():
    for threads, lead in ((1024, 0), (256, 0)):
        first = lambda name, n, ngram: SL.replay(settled(threads, lead, name, n, ngram)[1], *settled(threads, lead, name, n, ngram)[0][5:7],
                                                 15, ngram, MAX_NEW, threads, lead=lead)[0]
        assert first("H-end", 2, 2) == (0, 0, 1) and first("H-end", 4, 4) == (0, 0, 1)
        assert first("H-cut", 2, 2) == (3, 3, 4) and first("H-cut", 3, 4) == (3, 3, 4)
        assert first("S-last", 1, 1)[0] == 1 and first("S-last", 4, 4)[0] == 1
        assert first("H-wave", 4, 4) == (15, 15, 16) and first("P-fall", 1, 4) == (15, 15, 16)


def test_random_long_texts_over_four_tokens():
    """L and n_hint up to 3000, every ngram, several n_draft and room: the library against the restated rule and the Python rule"""
    from rama_amd.q8 import _draft_py, spec_draft
    rng = np.random.default_rng(30001)
    n_found = n_hint_wins = n_seq_wins = n_cut = 0
    for k in range(320):
        L, n_hint = int(rng.integers(1, 3001)), int(rng.integers(0, 3001))
        if k % 8 == 0:                                            # the library's edges: a hint of nothing, a text of one token
            L, n_hint = (1, n_hint) if k % 16 == 0 else (L, 0)
        seq = [int(t) for t in rng.integers(0, 4, size=L)]
        hint = [int(t) for t in rng.integers(0, 4, size=n_hint)]
        if k % 5 == 0 and L > 8:                                   # a tail the random text does not hold: the rule falls through
            seq[-4:] = [5, 6, 7, 6]
        ngram = 1 + k % 4
        n_draft, room = (0, 1, 7, 15)[(k // 4) % 4], (0, 2, 15, 40)[(k // 16) % 4]
        want = SL.draft(hint, seq, n_draft, ngram, room, 1024)
        assert spec_draft(hint, seq, n_draft, ngram, room) == want == _draft_py(hint, seq, n_draft, ngram, room), (k, L, n_hint, ngram)
        n_found += bool(want)
        n_cut += 0 < len(want) < min(n_draft, room)
        if want:
            in_hint = any(SL.occurrence_ends(hint, seq[L - n:], (n, n_hint), 1024) for n in range(min(ngram, L), 0, -1))
            n_hint_wins += in_hint
            n_seq_wins += not in_hint
    assert n_found >= 100 and n_hint_wins >= 40 and n_seq_wins >= 5, (n_found, n_hint_wins, n_seq_wins, n_cut)


@pytest.mark.parametrize("case", [(1024, 0) + c for c in SL.ALL], ids=ids)
def test_spec_replay_equals_the_restated_replay(case):
    from rama_amd.q8 import spec_replay
    threads, lead, name, n, ngram = case
    c, ref = settled(*case)
    for stop in (None, ref[17]):
        assert spec_replay(ref, c.context, c.hint, c.n_draft, ngram, MAX_NEW, stop) == \
            SL.replay(ref, c.context, c.hint, c.n_draft, ngram, MAX_NEW, threads, None, stop)


@pytest.mark.parametrize("case", [(256, 1) + c for c in SL.SERVE], ids=ids)
def test_serve_spec_replay_equals_the_restated_replay(case):
    """one request alone in a chain wide enough for its drafts, admitted over its cached context: want == granted == n_d"""
    from rama_amd.q8 import serve_spec_replay
    threads, lead, name, n, ngram = case
    c, ref = settled(*case)
    req = dict(context=c.context, max_new=MAX_NEW, n_draft=c.n_draft, ngram=ngram, hint=c.hint, n_cached=len(c.context) - 1)
    rp = serve_spec_replay([req], [ref], 4, 32, [2])
    got = [(st["want"][2], st["granted"][2], st["accepted"].get(2, 0), st["emitted"][2]) for st in rp["steps"]]
    want = SL.replay(ref, c.context, c.hint, c.n_draft, ngram, MAX_NEW, threads, lead=1)
    assert got == [(n_d, n_d, a, emit) for n_d, a, emit in want]
    assert rp["outputs"] == [ref]
