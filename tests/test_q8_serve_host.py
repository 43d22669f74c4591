"""The serving chain's host side (no GPU): the new symbols are declared everywhere, rama_q8_serve_plan_step -- the scheduling
rule as a pure function -- equals a restatement of the rule written here, over random slot tables and whole simulated
workloads, the rule's properties hold one by one, and Q8Server's argument checking raises before any library call."""
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
FREE, PROMPT, DECODE, DONE = 0, 1, 2, 3
SYMBOLS = ["rama_q8_serve_begin", "rama_q8_serve_admit", "rama_q8_serve_steps", "rama_q8_serve_poll", "rama_q8_serve_tokens",
           "rama_q8_serve_stats", "rama_q8_serve_plan_step", "rama_q8_serve_end"]


def test_serve_symbols_are_declared_everywhere():
    import rama_amd
    from rama_amd import _lib
    L = rama_amd.load()
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "rama_hip.h").read_text(), flags=re.S)
    rust = (REPO / "integration" / "rust" / "hip_sys.rs").read_text()
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), f"include/rama_hip.h lacks {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES lacks {s}"
        assert hasattr(L, s), f"librama_hip.so lacks {s}"
        assert len(re.findall(rf"pub fn {s}\s*\(", rust)) == 1, f"hip_sys.rs must declare {s} once"


# ------------------------------------------------------------------ the rule, restated

def rule(slots, max_rows):
    """slots: (state, n_context, cursor, n_out, max_new) -> (rows [(slot, pos, logits)] * max_rows, slots after, no stop sampled)"""
    n = [1 if s[0] in (PROMPT, DECODE) else 0 for s in slots]          # 1. and 2.: one row per DECODE and per PROMPT slot
    left = max_rows - sum(n)
    for i, s in enumerate(slots):                                      # 3.: the rest to PROMPT slots, ascending
        if s[0] == PROMPT:
            extra = min(s[1] - s[2] - 1, left)
            n[i] += extra
            left -= extra
    rows, after = [], []
    for i, (state, n_ctx, cur, n_out, max_new) in enumerate(slots):
        logits = state == DECODE or (state == PROMPT and cur + n[i] == n_ctx)
        rows += [(i, cur + k, int(logits and k == n[i] - 1)) for k in range(n[i])]
        if n[i]:
            cur += n[i]
            if logits:
                n_out += 1
                state = DONE if n_out >= max_new else DECODE
        after.append((state, n_ctx, cur, n_out, max_new))
    return rows + [(-1, -1, 0)] * (max_rows - len(rows)), after          # 4.: idle


def random_table(rng, n_slots, seq_len=96):
    t = []
    for _ in range(n_slots):
        state = int(rng.choice([FREE, PROMPT, PROMPT, DECODE, DECODE, DONE]))
        n_ctx = int(rng.integers(1, seq_len // 2))
        max_new = int(rng.integers(1, seq_len // 2))
        if state == PROMPT:
            t.append((state, n_ctx, int(rng.integers(0, n_ctx)), 0, max_new))
        elif state == DECODE:
            max_new = max(max_new, 2)
            n_out = int(rng.integers(1, max_new))
            t.append((state, n_ctx, n_ctx + n_out - 1, n_out, max_new))
        elif state == DONE:
            t.append((state, n_ctx, n_ctx + max_new - 1, max_new, max_new))
        else:
            t.append((FREE, 0, 0, 0, 0))
    return t


def check_properties(slots, rows, after, max_rows):
    assert len(rows) == max_rows
    used = [r for r in rows if r[0] >= 0]
    assert all(r == (-1, -1, 0) for r in rows[len(used):]) and rows[:len(used)] == used          # idle rows last
    for i, s in enumerate(slots):
        mine = [r for r in used if r[0] == i]
        if s[0] == DECODE:
            assert mine == [(i, s[2], 1)]                                  # exactly one row, its position, with logits
        elif s[0] == PROMPT:
            assert len(mine) >= 1
            assert [r[1] for r in mine] == list(range(s[2], s[2] + len(mine)))      # consecutive, from its cursor
            assert mine[-1][1] < s[1]
            assert [r[2] for r in mine[:-1]] == [0] * (len(mine) - 1)
            assert mine[-1][2] == int(mine[-1][1] == s[1] - 1)             # logits only at the final context position
        else:
            assert mine == []
        assert sum(r[2] for r in mine) <= 1
    # no idle row in a step after which some PROMPT slot still has context left
    if any(a[0] == PROMPT for a in after):
        assert len(used) == max_rows


def test_plan_step_equals_the_rule_on_random_tables():
    from rama_amd.q8 import serve_plan_step
    rng = np.random.default_rng(20260117)
    for case in range(240):
        n_slots = int(rng.integers(1, 33)) if case % 8 else int(rng.choice([1, 128]))
        max_rows = int(rng.integers(n_slots, 129)) if case % 5 else n_slots
        t = random_table(rng, n_slots)
        rows, after = serve_plan_step(t, max_rows)
        want_rows, want_after = rule(t, max_rows)
        assert rows == want_rows, (case, t, max_rows)
        assert after == want_after, (case, t, max_rows)
        check_properties(t, rows, after, max_rows)


@pytest.mark.parametrize("n_slots,max_rows", [(4, 4), (4, 8), (4, 16), (16, 64), (32, 128), (1, 1), (1, 128)])
def test_plan_step_over_whole_workloads(n_slots, max_rows):
    """requests of different lengths admitted into finished slots until all are served: every step's table and successor are the rule's"""
    from rama_amd.q8 import serve_plan_step
    rng = np.random.default_rng(1000 * n_slots + max_rows)
    pending = [(int(rng.integers(1, 90)), int(rng.integers(1, 40))) for _ in range(5 * n_slots + 3)]
    total_ctx, total_new = sum(p[0] for p in pending), sum(p[1] for p in pending)
    t = [(FREE, 0, 0, 0, 0)] * n_slots
    steps = prompt_rows = logit_rows = 0
    while True:
        for i in range(n_slots):
            if t[i][0] in (FREE, DONE) and pending:
                n_ctx, new = pending.pop(0)
                t[i] = (PROMPT, n_ctx, 0, 0, new)
        if not any(s[0] in (PROMPT, DECODE) for s in t):
            break
        rows, after = serve_plan_step(t, max_rows)
        assert (rows, after) == rule(t, max_rows)
        check_properties(t, rows, after, max_rows)
        prompt_rows += sum(1 for r in rows if r[0] >= 0 and t[r[0]][0] == PROMPT)
        logit_rows += sum(r[2] for r in rows)
        t = after
        steps += 1
        assert steps < 100000
    assert not pending and prompt_rows == total_ctx and logit_rows == total_new      # every context position fed once, every token picked once


def test_plan_step_refuses_bad_tables():
    from rama_amd import _lib
    from rama_amd._lib import rama_q8_serve_row, rama_q8_serve_slot
    L = _lib.load()
    rows = (rama_q8_serve_row * 128)()

    def rc(slots, max_rows, n=None):
        arr = (rama_q8_serve_slot * max(len(slots), 1))(*[rama_q8_serve_slot(*s) for s in slots])
        return L.rama_q8_serve_plan_step(arr, len(slots) if n is None else n, max_rows, rows, None)

    ok = (PROMPT, 5, 0, 0, 3)
    assert rc([ok], 4) == 0
    assert rc([ok], 0) == -1 and rc([ok], 129) == -1 and rc([ok, ok], 1) == -1 and rc([ok], 4, n=0) == -1
    assert rc([(7, 5, 0, 0, 3)], 4) == -1
    assert rc([(PROMPT, 5, 5, 0, 3)], 4) == -1                # a cursor behind the context
    assert rc([(PROMPT, 0, 0, 0, 3)], 4) == -1
    assert rc([(DECODE, 5, 5, 3, 3)], 4) == -1                # a DECODE slot that has spent its budget
    assert L.rama_q8_serve_plan_step(None, 1, 4, rows, None) == -1


# ------------------------------------------------------------------ Q8Server / serve_plan argument errors, no library call

class _Cfg:
    dim, hidden_dim, n_layers, n_heads, n_kv_heads, vocab_size, seq_len, shared_weight = 64, 128, 2, 4, 4, 512, 64, True


class _Model:
    """stands for a Q8Model: touching its device would be a library call"""
    cfg = _Cfg()

    @property
    def device(self):
        raise AssertionError("argument checking reached the library")

    ccfg = weights = property(lambda self: (_ for _ in ()).throw(AssertionError("argument checking reached the library")))


@pytest.mark.parametrize("n_slots,max_rows,cap", [(0, 4, 8), (129, 129, 8), (4, 3, 8), (4, 129, 8), (4, 8, 0), (4, 8, 64)])
def test_server_sizes_are_checked_without_a_library_call(n_slots, max_rows, cap):
    from rama_amd.q8 import Q8Server
    with pytest.raises(ValueError):
        Q8Server(_Model(), n_slots, max_rows, cap)


def test_serve_plan_argument_errors():
    from rama_amd.q8 import serve_plan
    cfg = _Cfg()
    ctx, plan = serve_plan(cfg, [1, 5, 9], 7, 0.8, 0.9, 0.25, stop_token=2, max_new_cap=8)
    assert ctx == [1, 5, 9] and plan == (pytest.approx(0.8), pytest.approx(0.9), 0.25, 7, 2)
    assert serve_plan(cfg, [1], 63)[1][3:] == (63, -1)
    bad = [dict(context=[]), dict(context=[1, 512]), dict(context=[-1]), dict(max_new=0), dict(max_new=9, max_new_cap=8),
           dict(context=[1] * 60, max_new=5), dict(temperature=-0.5), dict(temperature=float("nan")), dict(topp=1.5), dict(u=1.0),
           dict(stop_token=512), dict(stop_token=-2)]
    for kw in bad:
        args = dict(context=[1, 2, 3], max_new=4)
        args.update(kw)
        with pytest.raises(ValueError):
            serve_plan(cfg, **args)
    big = _Cfg()
    big.vocab_size = 50000
    with pytest.raises(ValueError):
        serve_plan(big, [1, 2], 4, temperature=0.7)
    assert serve_plan(big, [1, 2], 4)[1][0] == 0.0
