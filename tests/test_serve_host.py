"""The fp32 serving chain's host side (no GPU): the rama_serve_* symbols are declared everywhere, rama_amd.Server's host mirror foresees the
steps a replay of rama_q8_serve_plan_step gives, and the workloads of tests/test_hip_serve.py reach what they are there for -- a wholly idle
second tile, one slot's rows on both sides of row 32 -- by the host plan, so the GPU cases cannot pass on workloads that never get there."""
import re
from pathlib import Path

import pytest

from tests import serve_cases as W
from tests.serve_cases import DECODE, DONE, FREE, PROMPT, TILE

REPO = Path(__file__).resolve().parent.parent
SYMBOLS = ["rama_serve_begin", "rama_serve_admit", "rama_serve_steps", "rama_serve_poll", "rama_serve_tokens", "rama_serve_stats", "rama_serve_end"]


def plan_step(slots, max_rows):
    """the host rule of both chains, as rama_amd.Server's loop calls it"""
    from rama_amd.q8 import ServeLoop, serve_plan_step
    from rama_amd.server import Server
    assert issubclass(Server, ServeLoop)
    return serve_plan_step(slots, max_rows)


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
    # the same arguments as the Q8 entries, the model's weights apart
    for s in SYMBOLS:
        q8 = _lib.SIGNATURES[s.replace("rama_serve", "rama_q8_serve")]
        mine = _lib.SIGNATURES[s]
        assert mine[0] is q8[0] and len(mine[1]) == len(q8[1]), s
        for a, b in zip(mine[1], q8[1]):
            assert a is b or (a is _lib.C.POINTER(_lib.rama_weights) and b is _lib.C.POINTER(_lib.rama_q8_weights)), s
    from rama_amd.q8 import ServeLoop
    assert rama_amd.Server.ABI == "rama_serve" and issubclass(rama_amd.Server, ServeLoop) and not issubclass(rama_amd.Server, rama_amd.Q8Server)
    assert not hasattr(rama_amd.Server, "pool") and not hasattr(rama_amd.Server, "_run_spec")


class FakeLib:
    """records the entries a server calls; every call succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


class FakeDevice:
    def __init__(self):
        self.lib, self.ctx = FakeLib(), None


class FakeModel:
    def __init__(self, cfg):
        import rama_amd
        from tests.helpers import to_rama_cfg
        self.device, self.cfg = FakeDevice(), to_rama_cfg(cfg)
        self.ccfg, self.weights = self.cfg.c(), rama_amd._lib.rama_weights()


def make_server(monkeypatch, sizes, n_slots, max_rows):
    """a Server over a library that records calls: what its host side does, without a GPU"""
    import rama_amd
    from rama_amd import server
    from rama_amd._lib import rama_run_state

    class Eng:
        def __init__(self, device, model):
            self.state, self.model = rama_run_state(), model

        def free(self):
            pass
    monkeypatch.setattr(server, "Engine", Eng)
    srv = rama_amd.Server(FakeModel(W.TINY), n_slots, max_rows, 64)
    for n, new in sizes:
        srv.submit([1] + [2] * (n - 1), new)
    return srv


@pytest.mark.parametrize("max_rows", [8, 32, 64])
def test_server_mirror_foresees_the_replayed_plan(monkeypatch, max_rows):
    sizes, n_slots = W.SERVER["sizes"], W.SERVER["n_slots"]
    srv = make_server(monkeypatch, sizes, n_slots, max_rows)
    names = [c[0] for c in srv.device.lib.calls]
    assert names[0] == "rama_serve_begin" and names.count("rama_serve_admit") == n_slots and all(n.startswith("rama_serve_") for n in names)
    table = W.admitted(sizes, n_slots)
    assert srv._mirror == table
    # requests wait: the steps to the FIRST finish; by a replay of the rule over the same table
    k = next(i + 1 for i, (_, after) in enumerate(W.replay(table, max_rows, plan_step)) if any(s[0] == DONE for s in after))
    assert srv._steps_to_next_finish() == k
    srv._count_and_enqueue(k)
    assert srv.device.lib.calls[-1][0] == "rama_serve_steps" and srv.device.lib.calls[-1][1][-1] == k
    assert srv._mirror == W.replay(table, max_rows, plan_step)[k - 1][1] and srv.planned["steps"] == k
    # nobody waits: the steps until all have finished
    srv._queue.clear()
    assert srv._steps_to_next_finish() == len(W.replay(srv._mirror, max_rows, plan_step))


def test_idle_tile_workload_leaves_tile_1_idle_in_every_step():
    w = W.IDLE_TILE
    for max_rows in (w["max_rows"], w["narrow_rows"]):
        steps = W.replay(W.admitted(w["sizes"], w["n_slots"]), max_rows, plan_step)
        assert steps
        for rows, _ in steps:
            assert sum(1 for r in rows if r[0] >= 0) <= 8
            assert all(r == (-1, -1, 0) for r in rows[TILE:])            # tile 1 wholly idle (and idle rows last)
    # the same rows in the same steps at both widths: the narrow run is the reference of the wide one
    a = W.replay(W.admitted(w["sizes"], w["n_slots"]), w["max_rows"], plan_step)
    b = W.replay(W.admitted(w["sizes"], w["n_slots"]), w["narrow_rows"], plan_step)
    assert [r[:w["narrow_rows"]] for r, _ in a] == [r for r, _ in b]


def test_straddling_workload_puts_one_slot_on_both_sides_of_row_32():
    w = W.STRADDLE
    rows, _ = plan_step(W.admitted(w["sizes"], w["n_slots"]), 64)
    assert rows[TILE - 1][0] == rows[TILE][0] == 1 and rows[TILE][1] == rows[TILE - 1][1] + 1
    assert rows[0][0] == 0
    # the 40-token context alone: at 64 rows one step takes it whole, rows 31 and 32 both its own
    rows, after = plan_step([(PROMPT, 40, 0, 0, 4)], 64)
    assert [r[0] for r in rows[:40]] == [0] * 40 and rows[39][2] == 1 and after[0][0] == DECODE


def test_holes_workload_reaches_tile_1_around_the_holes():
    w = W.HOLES
    table = W.admitted(w["sizes"], w["n_slots"], w["holes"])
    assert [i for i, s in enumerate(table) if s[0] == FREE] == list(w["holes"])
    rows, _ = plan_step(table, w["max_rows"])
    used = [r for r in rows if r[0] >= 0]
    assert len(used) > TILE and all(r[0] not in w["holes"] for r in used)
    assert rows[TILE][0] >= rows[TILE - 1][0] >= 0                        # live rows on both sides of the tile boundary


def test_reuse_workload_has_a_prompt_to_done_slot_and_more_requests_than_slots():
    w = W.REUSE
    assert len(w["sizes"]) == 14 and w["n_slots"] == 4
    assert any(n > 1 and new == 1 for n, new in w["sizes"])               # PROMPT -> DONE without being DECODE
    _, after = plan_step([(PROMPT, 3, 0, 0, 1)], 8)
    assert after[0][0] == DONE
