"""The speculative chain's drafting kernel on texts longer than its workgroup (spec_draft_kernel: 1024 threads, 16 waves): the
cases of tests/spec_long_cases.py place the tail n-gram's occurrences in chosen waves and sweeps of the hint and of the sequence's
own context, so that the stride loop's later iterations, the running maximum, the reduction over the waves, the hint bit and the
fall-through from ngram = 4 decide what the counters show.  Every case is asserted discriminating with the model's real run before
the chain starts: each mutant rule of its kill list would give other counters.  The same runs put up to 16 rows of one sequence
at positions above 1024 and above 2048.  Every comparison is exact: token lists, integer counters and float bit patterns.

The model: dim 64, hidden 192, 2 layers, 2 heads, vocabulary 512, seq_len 2560, group size 32; max_new 24.  Its greedy run repeats
the context's last token, so a 1-gram whose choice shows through the model runs sampled (T 1, top-p 0.9, a fixed u), as does one
S case; the others run greedy."""
import ctypes as C

import pytest

from oracle import oracle as O
from tests import spec_long_cases as SL
from tests.test_hip_q8_spec import N_SEEDS, caches, run_and_check

pytestmark = pytest.mark.gpu

LONG = dict(dim=64, hidden_dim=192, n_layers=2, n_heads=2, n_kv_heads=2, vocab_size=512, seq_len=2560, shared_weight=True)
MAX_NEW, THREADS = 24, 1024
GREEDY, SAMPLED = (0.0, 0.9, 0.0), (1.0, 0.9, 0.35)
SAMPLED_CASES = {("H-wave", 1, 1), ("H-sweep", 1, 2), ("S-last", 4, 4)}
BOTH_MODES = {"H-wave", "H-sweep", "S-sweep", "P-hint"}
RUNS = [(c, g) for c in SL.ALL for g in ((0, 1) if c[0] in BOTH_MODES else (1,))]


class LongBench:
    """the model, the chain's engine and the twin; the solo runs -- and the twin's caches after them -- kept per context"""

    def __init__(self, dev):
        import rama_amd
        self.dev = dev
        self.m = rama_amd.Q8Model.synth(dev, O.Config(**LONG), 32, 11)
        self.cfg = self.m.cfg
        self.eng, self.twin = rama_amd.Q8Engine(dev, self.m), rama_amd.Q8Engine(dev, self.m)
        self._solo, self._settled = {}, {}

    def solo(self, ctx, plan, cache=False):
        key = (tuple(ctx), plan)
        if key not in self._solo or (cache and self._solo[key][1] is None):
            toks = self.twin.generate(ctx[1:], len(ctx) - 1 + MAX_NEW, *plan)[len(ctx) - 1:]
            # (a long context is an S or a P case's: its caches will be asked for, and the run is not made twice)
            self._solo[key] = (toks, caches(self.twin) if cache or len(ctx) > 100 else None)
        return self._solo[key] if cache else self._solo[key][0]

    def settled(self, case):
        """the case built for the model's real run, asserted discriminating (spec_long_cases.settle raises otherwise)"""
        if case not in self._settled:
            plan = SAMPLED if case in SAMPLED_CASES else GREEDY
            c, ref = SL.settle(*case, THREADS, 0, MAX_NEW, lambda ctx: self.solo(ctx, plan), self.cfg.vocab_size, N_SEEDS)
            self._settled[case] = (c, ref, plan)
        return self._settled[case]

    def free(self):
        self.eng.free(); self.twin.free(); self.m.free()


@pytest.fixture(scope="module")
def bench():
    import rama_amd
    dev = rama_amd.Hip(0)
    b = LongBench(dev)
    yield b
    dev.lib.rama_q8_spec_end(dev.ctx)
    b.free()
    dev.close()


def test_the_long_shape_is_taken(bench):
    assert bench.dev.lib.rama_q8_batch_shape_ok(C.byref(bench.m.ccfg)) == 1
    assert bench.cfg.seq_len == 2560 >= 2 * THREADS + 100 + MAX_NEW


@pytest.mark.parametrize("case,graph", RUNS, ids=[f"{SL.case_id(c)}-graph{g}" for c, g in RUNS])
def test_the_choice_of_occurrence_shows_in_the_counters(bench, case, graph):
    dev = bench.dev
    name, n, ngram = case
    c, ref, (T, P, u) = bench.settled(case)
    assert SL.undiscriminated(c, ref, MAX_NEW) == [], case           # before the chain runs, with the real run
    traj = SL.replay(ref, c.context, c.hint, c.n_draft, ngram, MAX_NEW, THREADS)
    print(case, graph, "context", len(c.context), "hint", len(c.hint), "ref", ref[:4], "trajectory", traj[:3], "steps", len(traj))
    twin_cache = bench.solo(c.context, (T, P, u), cache=True)[1] if name[0] in "SP" else None
    assert dev.lib.rama_set_graph_mode(dev.ctx, graph) == 0
    try:
        st = run_and_check(bench, c.context, MAX_NEW, ref, traj, twin_cache=twin_cache, T=T, P=P, u=u, K=c.n_draft, N=ngram,
                           hint=c.hint or None)
        assert st["graph_captures"] == graph
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
