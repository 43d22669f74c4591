"""spec_model_replay (rama_amd/q8_replay.py) on runs of several hundred tokens, and the cases of tests/spec_model_long_cases.py
-- no GPU, no library call.  Toy models (functions of the prefix) against the chain restated row by row with the draft cache's rows
tracked: the gap, what every draft pass reads, what lies below the cursor; the replay's trajectory and cursor are the
restatement's at every K; every wrong rule of the kill lists is caught by the exact inputs the GPU tests run.  Every comparison
is exact: token lists and integer counters."""
import pytest

from rama_amd.q8_replay import spec_model_replay
from tests import spec_model_long_cases as MC

CTX = MC.context(3, 6)
N_OUT = 400
#        toy draft: the target's own function, one answer in m changed, an unrelated function
DRAFTS = [("same", 0), ("every", 2), ("every", 5), ("every", 17), ("other", 0)]
TARGET = MC.toy("same")


@pytest.mark.parametrize("draft", DRAFTS, ids=lambda d: f"{d[0]}{d[1] or ''}")
@pytest.mark.parametrize("K", range(1, 16))
def test_the_restated_chain_keeps_its_invariants_and_is_the_replay(K, draft):
    ref = MC.toy_run(TARGET, CTX, N_OUT)
    fn = MC.toy_draft_fn(*draft)
    stops = [None] + [ref[i] for i in (N_OUT - 2, N_OUT // 2 + K) if ref[i] not in ref[:i]]
    for stop in stops:
        traj, cursor, broken, log = MC.restate(ref, fn, CTX, K, N_OUT, stop)
        assert broken is None, (K, draft, stop, broken)            # the gap, the rows read, the rows below the cursor: every step
        n_out = N_OUT if stop is None else ref.index(stop) + 1
        assert sum(e for _, _, e, _ in traj) == n_out and all(st["gap"] in (0, 1) for st in log)
        assert 0 <= cursor <= len(CTX) + n_out
        assert spec_model_replay(ref, fn, CTX, K, N_OUT, stop) == (traj, cursor), (K, draft, stop)
        # the draft rows a step feeds are its passes and its catch-up row, at consecutive positions from the cursor
        for (n_d, a, emit, catch), st in zip(traj, log):
            assert len(st["fed"]) == n_d + catch and catch == (st["gap"] if n_d else 0)
            assert st["fed"] == list(range(st["L"] - 1 - catch, st["L"] - 1 + n_d))
    # the runs are long and of the kind the draft is for
    traj, _, _, _ = MC.restate(ref, fn, CTX, K, N_OUT)
    full = [a for n_d, a, _, _ in traj if n_d == K]
    if draft[0] == "same":
        assert len(traj) == -(-N_OUT // (K + 1)) and all(a == n_d for n_d, a, _, _ in traj)
        assert sum(c for _, _, _, c in traj) == sum(1 for n_d, _, _, _ in traj if n_d) - 1
    elif draft[0] == "other":
        assert len(traj) >= N_OUT * 0.9 and sum(c for _, _, _, c in traj) <= len(traj) * 0.05
    else:
        assert len(traj) >= 20 and any(a < K for a in full) and sum(a for _, a, _, _ in traj) > 0


def test_the_kill_lists_are_whole():
    assert set(MC.KILLS) == {kind for kind, *_ in MC.case_inputs().values()}
    assert all(set(k) <= set(MC.MUTANTS) for k in MC.KILLS.values())
    assert {m for k in MC.KILLS.values() for m in k} == set(MC.MUTANTS)


@pytest.mark.parametrize("name", list(MC.case_inputs()))
def test_every_wrong_rule_of_the_kill_list_is_caught_by_the_case(name):
    """the exact context, K and budget of the GPU test, the tokens from the toy functions"""
    kind, ctx, K, max_new, draft = MC.case_inputs()[name]
    ref = MC.toy_run(TARGET, ctx, max_new)
    fn = MC.toy_draft_fn(*draft)
    stop = ref[MC.stop_index(ref, max_new)] if kind == "stop" else None
    traj, cursor, broken, log = MC.restate(ref, fn, ctx, K, max_new, stop)
    assert broken is None and spec_model_replay(ref, fn, ctx, K, max_new, stop) == (traj, cursor), name
    left = MC.unkilled(MC.KILLS[kind], ref, fn, ctx, K, max_new, stop)
    assert left == [], f"{name}: no counter changes and no invariant breaks under {left}"
    # what the case is for
    if kind == "boundary":
        B = int(name.split("-")[1])
        assert MC.opens_at(log, B), name
        assert traj == [(K, K, K + 1, int(i > 0)) for i in range(max_new // (K + 1))]
    elif kind == "partial":
        assert all(MC.partial_coverage(traj, K).values()), (name, MC.partial_coverage(traj, K))
    elif kind == "budget":
        assert traj == [(7, 7, 8, int(i > 0)) for i in range(6)] + [(2, 2, 3, 1)]
    else:
        n_out = MC.stop_index(ref, max_new) + 1
        assert sum(e for _, _, e, _ in traj) == n_out < max_new and cursor == len(ctx) + n_out


def test_every_mutant_dies_somewhere_and_the_true_rule_nowhere():
    """mutant -> the cases that kill it; a mutant that no case kills fails here, with the cases it survived"""
    killed = {m: [] for m in MC.MUTANTS}
    for name, (kind, ctx, K, max_new, draft) in MC.case_inputs().items():
        ref = MC.toy_run(TARGET, ctx, max_new)
        fn = MC.toy_draft_fn(*draft)
        stop = ref[MC.stop_index(ref, max_new)] if kind == "stop" else None
        alive = MC.unkilled(MC.MUTANTS, ref, fn, ctx, K, max_new, stop)
        for m in MC.MUTANTS:
            if m not in alive:
                killed[m].append(name)
    for m, names in killed.items():
        assert names, f"{m}: survives every case: {sorted(MC.case_inputs())}"


def test_the_boundary_lengths():
    """n_context = B - 15: L - 1 == B at step 1 of K = 15 and at step 2 of K = 7, inside max_new and inside the window"""
    assert sorted(MC.BOUNDARIES) == [64, 128, 256, 1024, 2048]
    for B, n_ctx in MC.BOUNDARIES.items():
        for K in MC.BOUNDARY_KS:
            i, rest = divmod(B + 1 - n_ctx, K + 1)
            assert rest == 0 and 1 <= i < MC.BOUNDARY_MAX_NEW // (K + 1), (B, K)
        assert n_ctx + MC.BOUNDARY_MAX_NEW <= MC.LONG["seq_len"]


def test_the_shapes_of_the_other_cases():
    assert MC.SHORT_N_CONTEXT + MC.SHORT_MAX_NEW == MC.SHORT["seq_len"] < MC.LONG["seq_len"]
    assert MC.ENDS_MAX_NEW % (MC.ENDS_K + 1) == 3 and MC.ENDS_N_CONTEXT - 1 < 1024 < MC.ENDS_N_CONTEXT - 1 + MC.ENDS_K
    assert max(MC.WIDER_CONTEXTS) + MC.WIDER_MAX_NEW <= min(MC.LONG["seq_len"], MC.WIDER["seq_len"])
    assert all(n + MC.PARTIAL_MAX_NEW <= MC.LONG["seq_len"] for n in MC.PARTIAL_CONTEXTS)
    assert MC.BIG_VOCAB["vocab_size"] > 32768 and MC.BIG_VOCAB["vocab_size"] % 4 == 0
    assert sum(MC.BIG_VOCAB_SHAPE) <= MC.BIG_VOCAB["seq_len"]
