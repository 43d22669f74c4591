"""Host side of prompt caching and drafts on the fp32 serving chain (rama_serve_admit_at / _begin_spec / _admit_spec / _spec_stats,
rama_amd.Server): no GPU.  The workloads tests/test_hip_serve_spec.py runs on the GPU are replayed here with q8_replay.serve_spec_replay over
the CPU oracle's tokens -- parity mode's own -- and must reach what they are there for: all six accept outcomes, a DECODE slot whose rows
straddle row 32, a second tile that is live without a logits row, a second tile that is wholly idle, a grant cut by the rows left.  Then the
declarations of the new entries, and Server's argument checks."""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from oracle import synth as S
from tests import serve_spec_cases as W
from tests.serve_cases import DECODE, PROMPT, TILE, TINY

REPO = Path(__file__).resolve().parents[1]
NEW = ["rama_serve_admit_at", "rama_serve_begin_spec", "rama_serve_admit_spec", "rama_serve_spec_stats"]


@pytest.fixture(scope="module")
def solo():
    """case -> the max_new tokens the reference's generate gives it alone: forced context, then Device::sample with the plan's (T, topp, u)"""
    weights = S.synth_weights(TINY, W.SEED, rope=S.rope_tables(TINY.seq_len, TINY.head_size))

    def run(c):
        orc, out, tok = O.Oracle(TINY, weights), [], c.ctx[0]
        for pos in range(len(c.ctx) - 1 + c.max_new):
            lg = orc.forward(tok, pos)
            if pos + 1 < len(c.ctx):
                tok = c.ctx[pos + 1]
            else:
                tok = int(O.argmax(lg)) if c.T == 0.0 else int(O.sample(lg.copy(), c.T, c.topp, c.u))
                out.append(tok)
        return out
    return run


def replay(w, max_rows=None, use=None):
    from rama_amd.q8_replay import serve_spec_replay
    return serve_spec_replay([c.spec() for c in w["cases"]], [c.solo for c in w["cases"]], w["n_slots"], max_rows or w["max_rows"], use)


def test_mixed_workload_reaches_all_six_accept_outcomes_and_a_cut_grant(solo):
    w = W.mixed(solo, TINY.vocab_size)
    rp = replay(w)
    seen = W.outcomes(W.replay_trace(rp, w["n_slots"]))
    assert seen == W.SIX, W.SIX - seen
    assert any(g < x for st in rp["steps"] for g, x in zip(st["granted"], st["want"]))          # a grant cut by `left`
    assert len(w["cases"][4].ctx) > w["max_rows"] and w["cases"][3].K == 0
    assert rp["outputs"] == [c.want() for c in w["cases"]]


@pytest.mark.parametrize("kind", ["own", "corrupt", None])
def test_hint_workloads_draft_as_their_hints_say(solo, kind):
    w = W.hints(solo, TINY.vocab_size, kind)
    for max_rows, use in W.LAYOUTS:
        c = replay(w, max_rows, use)["counters"]
        assert c["drafts_granted"] > 0, (kind, max_rows)
        if kind == "own":
            assert c["drafts_accepted"] == c["drafts_granted"]
        if kind == "corrupt":
            assert c["drafts_accepted"] < c["drafts_granted"]
    assert {p[0] == 0.0 for p in W.PLANS} == {True, False}                # greedy and sampled


def test_straddle_workload_puts_a_decode_slot_on_both_sides_of_row_32_and_leaves_tile_1_idle_later(solo):
    w = W.straddle(solo, TINY.vocab_size)
    rp = replay(w)
    straddling = idle = False
    for st in rp["steps"]:
        before = {i for i, s in enumerate(st["slots"]) if i in st["accepted"]}      # the slots that were DECODE in this step
        rows = st["rows"]
        straddling = straddling or (rows[TILE - 1][0] == rows[TILE][0] and rows[TILE][0] in before and rows[TILE][2] == 1)
        idle = idle or (rows[0][0] >= 0 and all(r == (-1, -1, 0) for r in rows[TILE:]))
    assert straddling and idle
    assert rp["counters"]["drafts_accepted"] == rp["counters"]["drafts_granted"] > 0


def test_guard_workload_has_a_live_second_tile_without_a_logits_row_then_one_with(solo):
    w = W.guard(solo, TINY.vocab_size)
    rp = replay(w)
    first, second = rp["steps"][0]["rows"], rp["steps"][1]["rows"]
    assert all(r[0] == 1 and r[2] == 0 for r in first[TILE:]) and first[TILE - 3] == (0, 29, 1)       # tile 1: slot 1 inside its context
    assert second[36] == (1, 45, 1) and [r[2] for r in second[TILE:]].count(1) == 1                    # tile 1: slot 1's final context row
    assert rp["steps"][1]["emitted"][1] == 1


def test_new_entries_are_declared_everywhere_with_the_q8_arguments():
    import rama_amd
    from rama_amd import _lib
    L = rama_amd.load()
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "rama_hip.h").read_text(), flags=re.S)
    rust = (REPO / "integration" / "rust" / "hip_sys.rs").read_text()
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", header), f"include/rama_hip.h lacks {s}"
        assert hasattr(L, s), f"librama_hip.so lacks {s}"
        assert len(re.findall(rf"pub fn {s}\s*\(", rust)) == 1, f"hip_sys.rs must declare {s} once"
        mine, q8 = _lib.SIGNATURES[s], _lib.SIGNATURES[s.replace("rama_serve", "rama_q8_serve")]
        assert mine[0] is q8[0] and len(mine[1]) == len(q8[1]), s
        for a, b in zip(mine[1], q8[1]):
            assert a is b or (a is _lib.C.POINTER(_lib.rama_weights) and b is _lib.C.POINTER(_lib.rama_q8_weights)), s
    assert hasattr(L, "rama_internal_serve_logits") and "rama_internal_serve_logits" not in header


# ------------------------------------------------------------------ rama_amd.Server over a library that records its calls

class FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


class FakeModel:
    def __init__(self, cfg):
        import rama_amd
        from tests.helpers import to_rama_cfg

        class Dev:
            lib, ctx = FakeLib(), None
        self.device, self.cfg = Dev(), to_rama_cfg(cfg)
        self.ccfg, self.weights = self.cfg.c(), rama_amd._lib.rama_weights()


@pytest.fixture
def fake(monkeypatch):
    from rama_amd import server
    from rama_amd._lib import rama_run_state

    class Eng:
        def __init__(self, device, model):
            self.state, self.model = rama_run_state(), model

        def free(self):
            pass
    monkeypatch.setattr(server, "Engine", Eng)
    return FakeModel(TINY), Eng


def test_server_picks_its_entries_by_what_it_was_asked_for(fake):
    import rama_amd
    model, Eng = fake
    names = lambda: [c[0] for c in model.device.lib.calls]
    srv = rama_amd.Server(model, 2, 8, 16)                      # the defaults: the plain chain's entries alone
    srv.submit([1, 2, 3], 4)
    assert names() == ["rama_serve_begin", "rama_serve_admit"] and not srv.spec and "spec" not in srv.stats()
    eng = Eng(None, model)
    srv.submit([1, 2, 3, 4], 4, engine=eng, n_cached=3)
    assert names()[-1] == "rama_serve_admit_at" and model.device.lib.calls[-1][1][-2] == 3 and srv.rows_cached == 3
    del model.device.lib.calls[:]
    srv = rama_amd.Server(model, 2, 8, 16, n_draft=5, ngram=2, hint_cap=8, prefix_cache=1)
    srv.submit([1, 2, 3], 4, hint=[4, 5], n_draft=3)
    assert names() == ["rama_serve_begin_spec", "rama_serve_admit_spec"] and model.device.lib.calls[0][1][-2:] == (5, 8)
    assert srv.spec and srv.pool.k == 1
    srv.stats()
    assert names()[-1] == "rama_serve_spec_stats"


def test_server_argument_checks(fake):
    import rama_amd
    model, Eng = fake
    for bad in (dict(n_draft=16), dict(n_draft=-1), dict(n_draft=3, ngram=5), dict(hint_cap=4), dict(n_draft=3, hint_cap=-1), dict(prefix_cache=-1)):
        with pytest.raises(ValueError):
            rama_amd.Server(model, 2, 8, 16, **bad)
    assert model.device.lib.calls == []                          # every refusal before any library call
    srv = rama_amd.Server(model, 2, 8, 16, n_draft=4, hint_cap=8, prefix_cache=2)
    eng = Eng(None, model)
    for n_cached in (-1, 3, 4):                                  # outside [0, n_context - 1]
        with pytest.raises(ValueError, match="n_cached"):
            srv.submit([1, 2, 3], 4, engine=eng, n_cached=n_cached)
    with pytest.raises(ValueError, match="n_cached needs the engine"):
        srv.submit([1, 2, 3], 4, n_cached=1)
    with pytest.raises(ValueError, match="n_draft"):
        srv.submit([1, 2, 3], 4, n_draft=5)                      # beyond the server's n_draft
    with pytest.raises(ValueError, match="hint"):
        srv.submit([1, 2, 3], 4, hint=[2] * 9)
    with pytest.raises(ValueError, match="hint"):
        srv.submit([1, 2, 3], 4, hint=[TINY.vocab_size])
    donor = Eng(None, model)
    srv.pool.put([1, 2, 3], donor)
    with pytest.raises(ValueError, match="donor"):
        srv.submit([1, 2, 3], 4, engine=donor)                   # a donor submitted as an engine
    h = srv.submit([1, 2, 3], 4, engine=eng)
    with pytest.raises(ValueError, match="already serves"):
        srv.submit([1, 2], 4, engine=eng)
    assert srv.cached(h) == 2                                    # (matched against the donor: the longest prefix, n_context - 1 at most)
    assert [c[0] for c in model.device.lib.calls][-2:] == ["rama_q8_kv_fork", "rama_serve_admit_spec"]
