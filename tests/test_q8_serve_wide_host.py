"""The wide workloads of tests/serve_wide_cases.py, replayed with rama_amd.q8.serve_plan_step alone (no GPU): every workload
really reaches the code it is in the table for, so the GPU test over the same table cannot pass vacuously.  These are
conditions on the workloads, not measurements: a seed changed so that one of them no longer holds fails here.

A stop token only ends a sequence earlier than the plan foresees, so each workload is replayed twice: with no stop token
falling (the host plan proper), and with every '+stop' slot ending on its first token -- the device's run lies between."""
import pytest

from tests.serve_wide_cases import SEQ_LEN, WORKLOADS, case_id, occupied, plan_kind

FREE, PROMPT, DECODE, DONE = 0, 1, 2, 3
TILE = 16                                                         # token rows of one tile of the batched pass


def start_table(w, stops_at_once=False):
    t = [(FREE, 0, 0, 0, 0)] * w.n_slots
    for i, (n_ctx, new, kind) in zip(occupied(w), w.sizes):
        t[i] = (PROMPT, n_ctx, 0, 0, 1 if stops_at_once and kind.endswith("+stop") else new)
    return t


def replay(w, stops_at_once=False):
    """[(the slot table before the step, the step's rows)] until no slot is live"""
    from rama_amd.q8 import serve_plan_step
    t, trace = start_table(w, stops_at_once), []
    while any(s[0] in (PROMPT, DECODE) for s in t):
        rows, after = serve_plan_step(t, w.max_rows)
        trace.append((t, rows))
        t = after
        assert len(trace) < 10000
    return trace


def reached(trace, n_slots, max_rows):
    """what a run -- [(slot table before, rows)] per step, the host plan's or the device's own -- got to"""
    out = dict(over_64_rows=False, prompt_slot_64_up_two_rows=False, straddles_63_64=False, idle_rows=False, full_step=False,
               last_tile_partly_idle=False, early_finish_below_64=False, early_finish_from_64=False)
    done_at = {}
    for k, (before, rows) in enumerate(trace):
        used = [r for r in rows if r[0] >= 0]
        n = len(used)
        out["over_64_rows"] |= n > 64
        out["idle_rows"] |= n < max_rows
        out["full_step"] |= n == max_rows
        out["last_tile_partly_idle"] |= n % TILE != 0 and n < max_rows
        for i in range(n_slots):
            mine = [j for j, r in enumerate(used) if r[0] == i]
            if before[i][0] == PROMPT and i >= 64 and len(mine) >= 2:
                out["prompt_slot_64_up_two_rows"] = True
            if mine and mine[0] <= 63 and mine[-1] >= 64:
                out["straddles_63_64"] = True
            if mine:
                done_at[i] = k                                    # the last step the slot had rows in
    last = len(trace) - 1
    out["early_finish_below_64"] = any(k < last for i, k in done_at.items() if i < 64)
    out["early_finish_from_64"] = any(k < last for i, k in done_at.items() if i >= 64)
    return out


def required(n_slots, max_rows):
    """the conditions that apply at these sizes"""
    need = ["idle_rows", "full_step", "last_tile_partly_idle"]
    if max_rows > 64:
        need += ["over_64_rows", "straddles_63_64"]
    if n_slots > 64:
        need += ["prompt_slot_64_up_two_rows", "early_finish_below_64", "early_finish_from_64"]
    return need


def test_the_table_is_the_one_the_gpu_tests_are_meant_to_run():
    want = {"ckpt_v2_q80_tied": [(17, 17), (33, 33), (64, 64), (65, 70), (128, 128), (40, 64)],
            "ckpt_v2_q80_untied": [(24, 32), (65, 96), (128, 128)],
            "synth15m": [(33, 48), (65, 96), (128, 128)]}
    for model, sizes in want.items():
        assert sorted((w.n_slots, w.max_rows) for w in WORKLOADS if w.model == model) == sorted(sizes)
    graphs = {(w.n_slots, w.max_rows): w.graphs for w in WORKLOADS if w.model == "synth15m"}
    assert graphs == {(33, 48): (1,), (65, 96): (0,), (128, 128): (1,)}
    assert all(w.graphs == (0, 1) for w in WORKLOADS if w.model != "synth15m")
    # FREE holes at both ends of both waves, in a workload that has a second wave
    assert any(w.n_slots > 64 and {0, 63, 64, w.n_slots - 1} <= set(w.holes) for w in WORKLOADS)


@pytest.mark.parametrize("w", WORKLOADS, ids=case_id)
def test_requests_fit_and_plan_kinds_cycle(w):
    assert 1 <= w.n_slots <= w.max_rows <= 128
    assert len(w.sizes) == w.n_slots - len(w.holes) and all(0 <= h < w.n_slots for h in w.holes)
    for k, (n_ctx, new, kind) in enumerate(w.sizes):
        assert n_ctx >= 1 and new >= 1 and n_ctx + new <= SEQ_LEN[w.model], (k, n_ctx, new)
        assert kind == plan_kind(k, new)
    kinds = {kind for _, _, kind in w.sizes}
    assert {"greedy", "sampled"} <= kinds and any(k.endswith("+stop") for k in kinds)
    if w.model == "synth15m":                                     # the solo runs of the twins dominate the time
        assert all(n_ctx <= 40 and new <= 8 for n_ctx, new, _ in w.sizes)


@pytest.mark.parametrize("stops_at_once", [False, True], ids=["no_stop_falls", "stops_fall_at_once"])
@pytest.mark.parametrize("w", WORKLOADS, ids=case_id)
def test_workload_reaches_what_it_is_for(w, stops_at_once):
    trace = replay(w, stops_at_once)
    got = reached(trace, w.n_slots, w.max_rows)
    missing = [c for c in required(w.n_slots, w.max_rows) if not got[c]]
    assert not missing, (case_id(w), missing)
    # (the rule itself: every context position fed once, every slot ends DONE -- test_q8_serve_host.py holds the rest)
    fed = sum(1 for before, rows in trace for r in rows if r[0] >= 0 and before[r[0]][0] == PROMPT)
    assert fed == sum(n_ctx for n_ctx, _, _ in w.sizes)

