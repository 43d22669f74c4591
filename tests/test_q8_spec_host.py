"""The speculative chain's host side (no GPU): the new symbols are declared everywhere; rama_q8_spec_draft -- the drafting rule as
a pure function -- equals a brute-force restatement written here over dense random texts, and gives what the rule says on its
named edges; rama_q8_spec_accept on every accept outcome and every end; spec_replay reproduces a hand-written trajectory."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
SYMBOLS = ["rama_q8_spec_begin", "rama_q8_spec_steps", "rama_q8_spec_poll", "rama_q8_spec_tokens", "rama_q8_spec_stats",
           "rama_q8_spec_end", "rama_q8_spec_draft", "rama_q8_spec_accept"]


def test_spec_symbols_are_declared_everywhere():
    import rama_amd
    from rama_amd import _lib
    L = rama_amd.load()
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "rama_hip.h").read_text(), flags=re.S)
    rust = (REPO / "integration" / "rust" / "hip_sys.rs").read_text()
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), f"include/rama_hip.h lacks {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES lacks {s}"
        assert hasattr(L, s), f"librama_hip.so lacks {s}"
        decl = re.findall(rf"pub fn {s}\s*\((.*?)\)\s*->", rust, flags=re.S)
        assert len(decl) == 1, f"hip_sys.rs must declare {s} once"
        assert decl[0].count(",") + 1 == len(_lib.SIGNATURES[s][1]), f"{s}: hip_sys.rs and _lib.py disagree on the argument count"
    for name in ("rama_q8_spec_plan", "rama_q8_spec_report"):
        assert re.search(rf"\}}\s*{name};", header) and f"pub struct {name}" in rust and hasattr(_lib, name), name
    # the structs as the header lays them out (LP64): 7 four-byte words, padding, a pointer, an int; 22 uint64 and 3 ints
    assert C.sizeof(_lib.rama_q8_spec_plan) == 48 and _lib.rama_q8_spec_plan.hint.offset == 32
    assert C.sizeof(_lib.rama_q8_spec_report) == 22 * 8 + 16 and _lib.rama_q8_spec_report.accepted_hist.offset == 48


# ------------------------------------------------------------------ the drafting rule, restated by brute force

def occurrences(text, tail, before):
    """every exclusive end e <= before with text[e - n:e] == tail"""
    n = len(tail)
    return [e for e in range(n, before + 1) if list(text[e - n:e]) == list(tail)]


def rule_draft(hint, seq, n_draft, ngram, room):
    L = len(seq)
    for n in range(min(ngram, L), 0, -1):
        tail = seq[L - n:]
        for text, before in ((hint, len(hint)), (seq, L - 1)):     # the hint first; in seq the occurrence ends before L
            ends = occurrences(text, tail, before)
            if ends:
                e = max(ends)                                      # the latest one
                return list(text[e:])[:max(min(n_draft, room), 0)]
    return []


def test_draft_equals_the_restated_rule_on_dense_random_texts():
    from rama_amd.q8 import spec_draft
    rng = np.random.default_rng(20260)
    n_cases = n_nonempty = n_short = 0
    for L in range(1, 41):
        for ngram in range(1, 5):
            for n_draft in range(0, 16):
                seq = [int(t) for t in rng.integers(0, 4, size=L)]
                hint = [int(t) for t in rng.integers(0, 4, size=int(rng.integers(1, 30)))]
                room = int(rng.integers(0, 20))
                for h in ([], hint):
                    want = rule_draft(h, seq, n_draft, ngram, room)
                    assert spec_draft(h, seq, n_draft, ngram, room) == want, (h, seq, n_draft, ngram, room)
                    n_cases += 1
                    n_nonempty += bool(want)
                    n_short += 0 < len(want) < min(n_draft, room)
    assert n_cases == 40 * 4 * 16 * 2 and n_nonempty > n_cases // 3 and n_short > 50      # the texts are dense: the rule is exercised


def test_draft_named_edges():
    from rama_amd.q8 import spec_draft
    # L < ngram: the longest n tried is L
    assert spec_draft([7, 5, 6, 8], [5, 6], 4, 4, 9) == [8]
    assert spec_draft([], [5], 4, 3, 9) == []
    # no match anywhere
    assert spec_draft([1, 2, 3], [4, 5, 6], 7, 3, 9) == []
    # the only match is the tail itself: it does not count, and shorter tails find nothing either
    assert spec_draft([], [1, 2, 3], 7, 3, 9) == []
    assert spec_draft([], [3, 1, 2, 3], 7, 3, 9) == [1, 2, 3]          # (n = 1: the earlier 3 does count)
    # a periodic text: the latest occurrence of the tail ends one period back, its continuation runs into the end of s
    assert spec_draft([], [1, 2, 3, 1, 2, 3, 1, 2], 7, 3, 9) == [3, 1, 2]
    assert spec_draft([], [9, 9, 9, 9], 7, 2, 9) == [9]
    # the same match in the hint and in s: the hint wins
    assert spec_draft([1, 2, 3, 40, 41], [1, 2, 3, 50, 1, 2, 3], 2, 3, 9) == [40, 41]
    # ... but a longer n in s beats a shorter n in the hint
    assert spec_draft([2, 3, 40], [1, 2, 3, 50, 1, 2, 3], 2, 3, 9) == [50, 1]
    # the latest occurrence inside the hint
    assert spec_draft([1, 2, 7, 1, 2, 8], [0, 1, 2], 1, 2, 9) == [8]
    # the hint's match on its last token: it decides, with nothing to follow
    assert spec_draft([4, 5, 1, 2, 3], [1, 2, 3, 50, 1, 2, 3], 2, 3, 9) == []
    # room 0 and 1, and n_draft 0
    assert spec_draft([1, 2, 3, 40, 41], [1, 2, 3], 7, 3, 0) == []
    assert spec_draft([1, 2, 3, 40, 41], [1, 2, 3], 7, 3, 1) == [40]
    assert spec_draft([1, 2, 3, 40, 41], [1, 2, 3], 0, 3, 9) == []
    assert spec_draft([1, 2, 3, 40, 41], [1, 2, 3], 7, 3, -3) == []


def test_draft_refuses_bad_arguments():
    import rama_amd
    L = rama_amd.load()
    seq = (C.c_int32 * 3)(1, 2, 3)
    out = (C.c_int32 * 16)()
    assert L.rama_q8_spec_draft(None, 0, seq, 3, 16, 3, 9, out) == -1
    assert L.rama_q8_spec_draft(None, 0, seq, 3, -1, 3, 9, out) == -1
    assert L.rama_q8_spec_draft(None, 0, seq, 3, 4, 0, 9, out) == -1
    assert L.rama_q8_spec_draft(None, 0, seq, 3, 4, 5, 9, out) == -1
    assert L.rama_q8_spec_draft(None, 2, seq, 3, 4, 3, 9, out) == -1
    assert L.rama_q8_spec_draft(None, -1, seq, 3, 4, 3, 9, out) == -1
    assert L.rama_q8_spec_draft(None, 0, None, 3, 4, 3, 9, out) == -1
    assert L.rama_q8_spec_draft(None, 0, seq, 0, 4, 3, 9, out) == -1
    assert L.rama_q8_spec_draft(None, 0, seq, 3, 4, 3, 9, None) == -1
    picks = (C.c_int32 * 4)(1, 2, 3, 4)
    assert L.rama_q8_spec_accept(seq, 3, None, -1, 5, None) == -1
    assert L.rama_q8_spec_accept(None, 3, picks, -1, 5, None) == -1
    assert L.rama_q8_spec_accept(seq, 16, picks, -1, 5, None) == -1
    assert L.rama_q8_spec_accept(seq, 3, picks, -1, 0, None) == -1
    assert L.rama_q8_spec_accept(None, 0, picks, -1, 5, None) == 1          # (no drafts: one pick, one token; finished may be NULL)


# ------------------------------------------------------------------ the accept rule

def test_accept_outcomes():
    from rama_amd.q8 import spec_accept
    d = [10, 11, 12]
    assert spec_accept(d, [20, 21, 22, 23], None, 9) == (1, False)             # a = 0
    assert spec_accept(d, [10, 11, 22, 23], None, 9) == (3, False)             # partial: a = 2, pick_0 .. pick_2
    assert spec_accept(d, [10, 11, 12, 23], None, 9) == (4, False)             # a = n_d: every draft and the pick behind them
    assert spec_accept(d, [20, 11, 12, 23], None, 9) == (1, False)             # a later agreement behind a rejection does not count
    assert spec_accept([], [20], None, 9) == (1, False)                        # n_d = 0
    # the stop token as pick_0, inside the accepted run, and as the first rejected pick (which is emitted: it is the model's own)
    assert spec_accept(d, [10, 11, 12, 23], 10, 9) == (1, True)
    assert spec_accept(d, [10, 11, 12, 23], 11, 9) == (2, True)
    assert spec_accept(d, [10, 11, 22, 23], 22, 9) == (3, True)
    assert spec_accept(d, [10, 11, 12, 23], 23, 9) == (4, True)
    assert spec_accept([], [20], 20, 9) == (1, True)
    # a pick behind the first rejected one is not emitted, so it does not stop
    assert spec_accept(d, [10, 21, 22, 23], 22, 9) == (2, False)
    # the stop token as a draft that the pick does not reproduce: it does not stop
    assert spec_accept([10, 99, 12], [10, 21, 22, 23], 99, 9) == (2, False)
    # the budget cuts inside the run; ending exactly on it finishes too; the stop token beyond the cut is not reached
    assert spec_accept(d, [10, 11, 12, 23], None, 2) == (2, True)
    assert spec_accept(d, [10, 11, 12, 23], None, 4) == (4, True)
    assert spec_accept(d, [10, 11, 12, 23], None, 5) == (4, False)
    assert spec_accept(d, [10, 11, 12, 23], 12, 2) == (2, True)
    assert spec_accept(d, [10, 11, 12, 23], 10, 2) == (1, True)
    assert spec_accept([], [20], None, 1) == (1, True)
    with pytest.raises(ValueError):
        spec_accept(d, [10, 11, 12], None, 9)


def test_accept_equals_the_restated_rule_on_random_runs():
    from rama_amd.q8 import spec_accept
    rng = np.random.default_rng(7)
    for _ in range(2000):
        n_d = int(rng.integers(0, 16))
        d = [int(t) for t in rng.integers(0, 3, size=n_d)]
        p = [int(t) for t in rng.integers(0, 3, size=n_d + 1)]
        stop = int(rng.integers(-1, 3))
        remaining = int(rng.integers(1, 20))
        a = 0
        while a < n_d and p[a] == d[a]:
            a += 1
        emitted = p[:a + 1][:remaining]
        fin = len(emitted) == remaining
        if stop in emitted:
            emitted, fin = emitted[:emitted.index(stop) + 1], True
        assert spec_accept(d, p, stop, remaining) == (len(emitted), fin), (d, p, stop, remaining)


# ------------------------------------------------------------------ the replay

def test_replay_reproduces_a_hand_written_trajectory():
    from rama_amd.q8 import spec_replay
    context = [1, 5, 6, 7]
    #      emitted so far: the solo run's tokens
    ref = [5, 6, 7, 5, 6, 8, 9, 5, 6, 8, 2, 3]
    # step 1: s = 1 5 6 7, tail (n = 3) 5 6 7 only at the end; n = 2: 6 7 only at the end; n = 1: 7 only at the end -> n_d 0, emits 5
    # step 2: s = .. 7 5, tail 6 7 5 no, 7 5 no, n = 1: 5 at e = 2 -> drafts 6 7 5 (to the end of s); picks 6 7 5 6: a = 3, emits 4
    # step 3: s = 1 5 6 7 5 6 7 5 6, tail 7 5 6 at e = 6 -> drafts 7 5 6; picks 8 ..: a = 0, emits 8
    # step 4: s = .. 5 6 8, no 5 6 8 / 6 8 / 8 earlier -> n_d 0, emits 9
    # step 5: s = .. 8 9, nothing -> emits 5
    # step 6: s = 1 5 6 7 5 6 7 5 6 8 9 5: n = 1: 5 latest at e = 8 -> 6 8 9 5 follow, remaining = 4 so room = 3 cuts them to 6 8 9;
    #         picks 6 8 2 ..: a = 2, emits 6 8 2
    # step 7: remaining = 1: room 0, n_d 0, emits 3 -- the 12th token
    want = [(0, 0, 1), (3, 3, 4), (3, 0, 1), (0, 0, 1), (0, 0, 1), (3, 2, 3), (0, 0, 1)]
    assert spec_replay(ref, context, None, 7, 3, 12, None) == want
    # the same run with a stop token: step 2 emits 6 7 and ends
    assert spec_replay(ref, context, None, 7, 3, 12, 7) == [(0, 0, 1), (3, 3, 2)]
    # with the solo run as the hint (no n-gram of it twice) every draft is right: n_draft + 1 tokens a step, and the budget's
    # remaining - 1 bounds the last step's drafts
    context, ref = [1, 2], list(range(10, 22))
    assert spec_replay(ref, context, context + ref, 3, 3, 12, None) == [(3, 3, 4), (3, 3, 4), (3, 3, 4)]
    assert spec_replay(ref, context, context + ref, 7, 2, 12, None) == [(7, 7, 8), (3, 3, 4)]
    # n_draft 0: one token a step
    assert spec_replay(ref, context, context + ref, 0, 3, 5, None) == [(0, 0, 1)] * 5
    with pytest.raises(ValueError):
        spec_replay(ref[:5], context, None, 7, 3, 12, None)


def test_replay_drafts_equal_the_library_rule():
    """spec_replay's own drafting (pure Python) and rama_q8_spec_draft agree along whole random runs"""
    from rama_amd import q8
    rng = np.random.default_rng(11)
    for _ in range(40):
        context = [1] + [int(t) for t in rng.integers(0, 4, size=int(rng.integers(0, 6)))]
        max_new = int(rng.integers(1, 30))
        ref = [int(t) for t in rng.integers(0, 4, size=max_new)]
        hint = [int(t) for t in rng.integers(0, 4, size=int(rng.integers(0, 20)))]
        K, N = int(rng.integers(0, 16)), int(rng.integers(1, 5))
        s, e = list(context), 0
        for n_d, a, emit in q8.spec_replay(ref, context, hint, K, N, max_new, None):
            d = q8.spec_draft(hint, s, K, N, max_new - e - 1)
            assert len(d) == n_d
            assert q8.spec_accept(d, ref[e:e + n_d + 1], None, max_new - e)[0] == emit
            s += ref[e:e + emit]
            e += emit
        assert e == max_new


def test_generate_spec_checks_before_any_library_call():
    from rama_amd.q8 import spec_plan
    from rama_amd.transformer import Config
    cfg = Config(64, 128, 2, 4, 4, 100, 32, True)
    ok = dict(context=[1, 2, 3], max_new=5)
    ctx, hint, plan = spec_plan(cfg, **ok)
    assert ctx == [1, 2, 3] and hint == [] and plan[:2] == (0.0, 0.9) and plan[3:] == (5, -1, 7, 3)
    for bad in (dict(context=[]), dict(context=[1, 100]), dict(max_new=0), dict(max_new=30), dict(n_draft=16), dict(n_draft=-1),
                dict(ngram=0), dict(ngram=5), dict(hint=[100]), dict(hint=[-1]), dict(stop_token=100), dict(temperature=-1.0),
                dict(topp=1.5), dict(u=1.0), dict(temperature=float("nan"))):
        with pytest.raises(ValueError):
            spec_plan(cfg, **{**ok, **bad})
    with pytest.raises(ValueError):
        spec_plan(Config(64, 128, 2, 4, 4, 40000, 32, True), [1], 3, temperature=1.0)
    assert spec_plan(cfg, [1, 2], 30)[2][3] == 30          # n_context + max_new == seq_len is allowed
