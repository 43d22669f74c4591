"""spec_model_replay (rama_amd/q8_replay.py), the speculative chain with a draft model replayed on the host -- no GPU, no library
call: toy draft functions against a brute-force restatement of the step written here, the draft cursor's invariant, the catch-up
row, the budget and stop cuts, the last step without drafts."""
import pytest

from rama_amd.q8_replay import _accept_py, spec_model_replay


def ref_run(n, seed=3, V=997):
    """n reference tokens, a fixed pseudo-random list (no two neighbours equal, so `wrong` below is really wrong)"""
    out, x = [], seed
    for _ in range(n):
        x = (x * 1103515245 + 12345) % (1 << 31)
        t = 2 + x % V
        out.append(t if not out or t != out[-1] else 2 + (t - 1) % V)
    return out


def make_draft_fn(ctx, ref, kind, m=0):
    """the draft model as a function of the prefix alone: `right` continues the reference run, `wrong` never does, `first` is right
    for the first m tokens of a call and wrong behind them"""
    def fn(prefix, n):
        at = len(prefix) - len(ctx)                                # tokens of the reference the prefix holds
        assert prefix == ctx + ref[:at]
        right = (ref + [0] * n)[at:at + n]
        if kind == "right":
            return right
        if kind == "wrong":
            return [t + 100 for t in right]
        return [t if j < m else t + 100 for j, t in enumerate(right)]
    return fn


def brute(ref, draft_fn, ctx, K, max_new, stop):
    """the step of include/rama_hip.h, restated row by row: which draft-cache rows hold which tokens, which of them still belong
    to the sequence afterwards"""
    s, e, steps = list(ctx), 0, []
    rows = list(ctx[:-1])                                          # rows[p] = the token whose draft-model row sits at position p
    Dc = len(rows)
    while True:
        L = len(s)
        P, remaining = L - 1, max_new - e
        n_d = min(K, remaining - 1)
        gap = P - Dc
        assert gap in (0, 1)
        d, fed = [], 0
        if n_d > 0:
            del rows[Dc:]
            for p in range(Dc, P + 1):                             # the first pass: the catch-up row (if any) and s[P]
                rows.append(s[p]); fed += 1
            d = list(draft_fn(list(s), n_d))
            for j in range(1, n_d):                                # pass j feeds d[j - 1] at position P + j
                rows.append(d[j - 1]); fed += 1
        picks = ref[e:e + n_d + 1]
        a = 0
        while a < n_d and picks[a] == d[a]:
            a += 1
        emit, fin = [], False
        for t in picks[:a + 1]:
            emit.append(t)
            if len(emit) == remaining or t == stop:
                fin = True
                break
        s += emit
        e += len(emit)
        if n_d > 0:                                                # the rows that carry tokens of s, from the front
            Dc = 0
            while Dc < len(rows) and Dc < len(s) and rows[Dc] == s[Dc]:
                Dc += 1
        steps.append(dict(n_d=n_d, a=a, emit=len(emit), catch=gap if n_d > 0 else 0, fed=fed, gap=gap))
        if fin:
            return steps, Dc, s[len(ctx):]


CTX = [1, 5, 9]
CASES = [(kind, m, K, max_new, stop_at)
         for kind, m in (("right", 0), ("wrong", 0), ("first", 1), ("first", 2), ("first", 3))
         for K in (1, 2, 3, 7, 15)
         for max_new, stop_at in ((1, None), (2, None), (9, None), (16, None), (17, None), (33, None), (33, 6), (33, 0))]


@pytest.mark.parametrize("kind,m,K,max_new,stop_at", CASES)
def test_replay_equals_the_brute_force_restatement(kind, m, K, max_new, stop_at):
    ref = ref_run(max_new)
    stop = None
    if stop_at is not None:
        stop = ref[stop_at]
        assert stop not in ref[:stop_at]
    fn = make_draft_fn(CTX, ref, kind, m)
    traj, cursor = spec_model_replay(ref, fn, CTX, K, max_new, stop)
    want, want_cursor, out = brute(ref, fn, CTX, K, max_new, -1 if stop is None else stop)
    assert [(t["n_d"], t["a"], t["emit"], t["catch"]) for t in want] == traj
    assert cursor == want_cursor
    n_out = max_new if stop is None else stop_at + 1
    assert out == ref[:n_out] and sum(e for _, _, e, _ in traj) == n_out
    # the draft rows a step feeds: its live passes and its catch-up row
    assert [t["fed"] for t in want] == [n_d + c for n_d, _, _, c in traj]
    # the gap P - Dc is 0 or 1 at every step (brute asserts it), and a catch-up row follows exactly a step that accepted all K drafts
    for i, (n_d, a, emit, catch) in enumerate(traj):
        after_full = i > 0 and traj[i - 1][0] == K and traj[i - 1][1] == K
        assert want[i]["gap"] == (1 if after_full else 0)
        assert catch == (1 if after_full and n_d > 0 else 0)
    # the cuts are _accept_py's
    e = 0
    for n_d, a, emit, _ in traj:
        d = fn(CTX + ref[:e], n_d) if n_d else []
        assert (a, emit) == _accept_py(d, ref[e:e + n_d + 1], max_new - e, -1 if stop is None else stop)[:2]
        e += emit


def test_always_right_takes_k_plus_one_tokens_a_step_and_a_catch_up_row_every_step_but_the_first():
    ref = ref_run(33)
    traj, cursor = spec_model_replay(ref, make_draft_fn(CTX, ref, "right"), CTX, 7, 33, None)
    assert traj == [(7, 7, 8, 0), (7, 7, 8, 1), (7, 7, 8, 1), (7, 7, 8, 1), (0, 0, 1, 0)]
    assert cursor == len(CTX) + 32 - 2                             # d[6] of the last drafting step and the pick behind it were never fed


def test_always_wrong_is_one_token_a_step_without_catch_up():
    ref = ref_run(9)
    traj, cursor = spec_model_replay(ref, make_draft_fn(CTX, ref, "wrong"), CTX, 3, 9, None)
    assert traj == [(3, 0, 1, 0)] * 6 + [(2, 0, 1, 0), (1, 0, 1, 0), (0, 0, 1, 0)]
    assert cursor == len(CTX) - 1 + 8                              # every step's first row belongs to the sequence


def test_the_final_step_has_no_drafts_when_one_token_remains():
    for K in (1, 4):
        ref = ref_run(5)
        traj, _ = spec_model_replay(ref, make_draft_fn(CTX, ref, "wrong"), CTX, K, 5, None)
        assert traj[-1] == (0, 0, 1, 0) and all(n_d >= 1 for n_d, _, _, _ in traj[:-1])
    assert spec_model_replay([4], make_draft_fn(CTX, [4], "right"), CTX, 15, 1, None) == ([(0, 0, 1, 0)], len(CTX) - 1)


def test_budget_cut_inside_an_accepted_run_and_stop_inside_one():
    ref = ref_run(11)
    fn = make_draft_fn(CTX, ref, "right")
    traj, cursor = spec_model_replay(ref, fn, CTX, 7, 11, None)
    assert traj == [(7, 7, 8, 0), (2, 2, 3, 1)]                    # remaining 3: two drafts, both accepted, the pick is the 11th token
    assert cursor == len(CTX) + 8 + 1
    stop = ref[3]
    assert stop not in ref[:3]
    traj, cursor = spec_model_replay(ref, fn, CTX, 7, 11, stop)
    assert traj == [(7, 7, 4, 0)]                                  # all seven reproduced, four emitted: the stop token ends the run
    assert cursor == len(CTX) + 4                                  # ... and the cursor stops at the sequence's end


def test_bad_arguments():
    with pytest.raises(ValueError):
        spec_model_replay([1, 2], lambda p, n: [0] * n, CTX, 3, 5, None)
    with pytest.raises(ValueError):
        spec_model_replay([1, 2, 3], lambda p, n: [0], CTX, 3, 3, None)
