"""Speculation inside the serving chain on the GPU (rama_q8_serve_begin_spec / _admit_spec / _spec_stats, Q8Server(n_draft=...)): a
DECODE slot's drafts ride on the rows no slot wants.  Whatever the drafts, the hints, the neighbours, max_rows and the graph mode,
every request's tokens are bit for bit those of Q8Engine.generate on a twin engine, its cache rows below its final cursor are the
twin's, and nothing from row n_context - 1 + max_new on is written; the device's row table, slot table, wanted and granted drafts
and counters equal serve_spec_replay's step by step.  Every comparison is exact: token lists and float bit patterns.

The models: ckpt_v2_q80_untied (seq_len 32), ckpt_v2_q80_gs8 (dim 72: the generic product kernels; a vocabulary of 37, no multiple
of 4) and a stories15M-shaped synthetic model (the K-split kernels)."""
import ctypes as C
import time

import numpy as np
import pytest

from tests.test_hip_q8 import same_bits
from tests.test_hip_q8_serve import (DECODE, DONE, EINVAL, FREE, PROMPT, SENTINEL, Req, cache, open_model, poll, set_graph, stats, steps, tokens)
from tests.test_hip_q8_spec import corrupt

pytestmark = pytest.mark.gpu

MODELS = ["ckpt_v2_q80_untied", "ckpt_v2_q80_gs8", "synth15m"]
HINT_CAP = 64


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


class SReq(Req):
    """a request with drafting fields: n_draft K, ngram N and a hint made from its own solo run"""

    def __init__(self, dev, m, rng, n_ctx, max_new, T=0.0, topp=0.9, u=0.0, stop=-1, K=0, N=3, hint=None, periodic=0):
        super().__init__(dev, m, rng, n_ctx, max_new, T, topp, u, stop)
        if periodic:                                              # BOS, then a pattern of `periodic` tokens over and over
            self.ctx = [1] + [self.ctx[1 + (i % periodic)] for i in range(n_ctx - 1)]
        self.K, self.N, self.n_cached = K, N, 0
        V = m.cfg.vocab_size
        if hint == "own":                                         # the text the sequence will have: every granted draft is right
            self.hint = self.ctx + self.solo()
        elif hint == "corrupt":
            self.hint = corrupt(self.ctx + self.solo(), V)
        elif hint == "wrong":                                     # behind every token of the solo run one that the run never has
            z = next(t for t in range(V) if t not in self.solo() and t not in self.ctx)
            self.hint = [t for x in self.solo() for t in (x, z)]
        else:
            self.hint = list(hint or [])

    def spec(self):
        return dict(context=self.ctx, max_new=self.max_new, stop_token=None if self.stop < 0 else self.stop, n_draft=self.K, ngram=self.N,
                    hint=self.hint, n_cached=self.n_cached)

    def check(self, got, what):
        """tokens, every cache row below the final cursor, and the sentinel from row n_context - 1 + max_new on"""
        assert got == self.want(), what
        valid, untouched = len(self.ctx) + len(got) - 1, len(self.ctx) - 1 + self.max_new
        for a, b in zip(cache(self.eng), cache(self.twin)):
            assert same_bits(a[:, :valid], b[:, :valid]), what
            assert (a[:, untouched:] == SENTINEL).all(), what


def begin_spec(dev, m, n_slots, max_rows, cap, n_draft_cap=15, hint_cap=HINT_CAP):
    return dev.lib.rama_q8_serve_begin_spec(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), n_slots, max_rows, cap, n_draft_cap, hint_cap)


def admit_spec(dev, slot, r, K=None, N=None, hint=None, n_cached=None, ctx=None, eng=None, null=False):
    from rama_amd._lib import rama_q8_serve_spec
    ctx = r.ctx if ctx is None else ctx
    hint = r.hint if hint is None else hint
    p = r.plan()
    h = (C.c_int32 * max(len(hint), 1))(*hint)
    s = rama_q8_serve_spec(r.K if K is None else K, r.N if N is None else N, h if hint else None, len(hint))
    return dev.lib.rama_q8_serve_admit_spec(dev.ctx, slot, C.byref((eng or r.eng).state), (C.c_int32 * max(len(ctx), 1))(*ctx), len(ctx),
                                            r.n_cached if n_cached is None else n_cached, C.byref(p), None if null else C.byref(s))


def spec_stats(dev):
    from rama_amd._lib import rama_q8_serve_spec_report
    from rama_amd.q8 import serve_spec_report
    r = rama_q8_serve_spec_report()
    assert dev.lib.rama_q8_serve_spec_stats(dev.ctx, C.byref(r)) == 0
    return serve_spec_report(r)


COUNTERS = ("steps", "rows_decode", "rows_draft", "rows_prompt", "rows_idle", "drafts_wanted", "drafts_granted", "drafts_accepted",
            "tokens_emitted", "accepted_hist")


def drive(dev, m, reqs, n_slots, max_rows, use_slots=None, what=None):
    """the workload under serve_spec_replay's admission rule, one step at a time: after every step the device's row table, slot table and
    wanted / granted drafts against the replay's; at the end the counters, every request's tokens and cache rows.  -> (the replay, the
    device's own trace: per step (slots before, slots after, want, granted))"""
    from rama_amd.q8 import serve_spec_replay
    rp = serve_spec_replay([r.spec() for r in reqs], [r.solo() for r in reqs], n_slots, max_rows, use_slots)
    assert begin_spec(dev, m, n_slots, max_rows, max(r.max_new for r in reqs)) == 0
    who, got, trace = {}, {}, []
    before = [(FREE, 0, 0, 0, 0)] * n_slots
    for k, st in enumerate(rp["steps"]):
        for slot, q in st["admitted"]:
            assert admit_spec(dev, slot, reqs[q]) == 0, (what, k, slot)
            who[slot] = q
            before[slot] = (PROMPT, len(reqs[q].ctx), reqs[q].n_cached, 0, reqs[q].max_new)
        assert steps(dev, 1) == 0
        s, ss = stats(dev), spec_stats(dev)
        assert s["rows"] == st["rows"], (what, k)
        assert s["slots"] == st["slots"], (what, k)
        assert (ss["last_want"], ss["last_granted"]) == (st["want"], st["granted"]), (what, k)
        trace.append((list(before), s["slots"], ss["last_want"], ss["last_granted"]))
        before = list(s["slots"])
        for slot in st["finished"]:
            got[who[slot]] = tokens(dev, slot)
            assert poll(dev, slot)[:2] == (got[who[slot]], True), (what, k, slot)
    s, ss = stats(dev), spec_stats(dev)
    assert {c: ss[c] for c in COUNTERS} == rp["counters"], what
    assert (s["steps"], s["decode"], s["prompt"], s["idle"]) == tuple(rp["counters"][c] for c in ("steps", "rows_decode", "rows_prompt", "rows_idle"))
    assert ss["rows_draft"] == ss["drafts_granted"] and sum(ss["accepted_hist"]) == ss["rows_decode"]
    assert sorted(got) == list(range(len(reqs))), what
    for q, r in enumerate(reqs):
        assert got[q] == rp["outputs"][q], (what, q)
        r.check(got[q], (what, q))
    return rp, trace


def outcomes(trace):
    """which of the six outcomes the DEVICE's run shows (its slot tables and its wanted / granted drafts, step by step)"""
    seen = set()
    for before, after, want, granted in trace:
        ingesting = [i for i, b in enumerate(before) if b[0] == PROMPT and after[i][0] == PROMPT]
        for i, (b, a) in enumerate(zip(before, after)):
            if b[0] != DECODE:
                continue
            emitted, fin = a[3] - b[3], a[0] == DONE
            if granted[i] < want[i]:
                seen.add("grant cut")
            if granted[i] > 0 and emitted == granted[i] + 1:
                seen.add("all accepted")
            if granted[i] > 0 and emitted == 1 and not fin:
                seen.add("first rejected")
            if fin and emitted > 1 and a[3] == a[4]:
                seen.add("budget ends in an accepted run")
            if fin and emitted > 1 and a[3] < a[4]:
                seen.add("stop among the accepted drafts")
            if fin and ingesting:
                seen.add("finish next to an ingestion")
    return seen


SIX = {"grant cut", "all accepted", "first rejected", "budget ends in an accepted run", "stop among the accepted drafts",
       "finish next to an ingestion"}


def mixed_workload(dev, m, seed):
    """six requests for 4 slots at max_rows 8, built from their own solo runs so that the six outcomes are certain: c stops on its third
    token, which its second step reaches inside an accepted run; a is always right and ends on its budget; b's first draft is always
    wrong; e never drafts and ends while d -- admitted into c's slot, a context longer than max_rows -- is still ingesting"""
    rng = np.random.default_rng(seed)
    for _ in range(12):                                           # c's first three tokens must differ: its stop token is the third
        c = SReq(dev, m, rng, 3, 8, 1.0, 0.9, 0.37, K=7, N=3, hint="own")
        if c.solo()[2] not in c.solo()[:2]:
            break
        c.free()
    else:
        raise AssertionError("no context whose first three tokens differ")
    c.stop = c.solo()[2]
    a = SReq(dev, m, rng, 4, 12, 1.0, 0.9, 0.77, K=7, N=3, hint="own")
    b = SReq(dev, m, rng, 2, 9, 0.7, 1.0, 0.3, K=3, N=1, hint="wrong")
    e = SReq(dev, m, rng, 1, 5, K=0)
    d = SReq(dev, m, rng, 21, 2, K=2, N=2)
    f = SReq(dev, m, rng, 2, 6, 1.0, 0.9, 0.6, K=7, N=2, hint="corrupt")
    return [c, a, b, e, d, f]


def free_all(dev, reqs, m):
    set_graph(dev, 0)
    dev.lib.rama_q8_serve_end(dev.ctx)
    for r in reqs:
        r.free()
    m.free()


# ------------------------------------------------------------------ 1. a mixed workload: every outcome, every model, both modes

@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_mixed_workload_equals_the_replay_and_reaches_every_outcome(dev, golden_dir, which, graph):
    """greedy and sampled plans (T 1 / top-p 0.9, T 0.7 / top-p 1), a spec slot next to a slot with n_draft = 0 and next to a PROMPT slot
    that ingests a context longer than max_rows, hints that are right, corrupted and always wrong"""
    m = open_model(dev, golden_dir, which)
    reqs = mixed_workload(dev, m, 3)
    try:
        set_graph(dev, graph)
        rp, trace = drive(dev, m, reqs, 4, 8, what=(which, graph))
        assert outcomes(trace) == SIX, SIX - outcomes(trace)
        assert stats(dev)["captures"] == (1 if graph else 0)
        assert len(reqs[4].ctx) > 8 and reqs[3].K == 0
    finally:
        free_all(dev, reqs, m)


# ------------------------------------------------------------------ 2. the three kinds of hint, the layouts

@pytest.mark.parametrize("hint", ["own", "corrupt", None])
@pytest.mark.parametrize("n_slots,max_rows,use", [(4, 8, None), (4, 16, None), (4, 16, [0, 2, 3])])
def test_hint_kinds_and_layouts(dev, golden_dir, hint, n_slots, max_rows, use):
    """hint = the request's own solo output (every granted draft accepted), that output corrupted (rejections), none (lookup in a
    periodic context); 4 slots at max_rows 8 and 16, 3 slots at max_rows 16 around a FREE hole"""
    m = open_model(dev, golden_dir, "synth15m")
    rng = np.random.default_rng(17)
    plans = [(0.0, 0.9, 0.0), (1.0, 0.9, 0.21), (0.7, 1.0, 0.55), (0.0, 0.9, 0.0), (1.0, 0.9, 0.8)]
    reqs = [SReq(dev, m, rng, n_ctx, new, *plans[i], K=K, N=N, hint=hint, periodic=0 if hint else 3)
            for i, (n_ctx, new, K, N) in enumerate([(13, 14, 7, 3), (4, 10, 15, 2), (10, 9, 3, 3), (7, 16, 7, 4), (2, 6, 5, 2)])]
    try:
        set_graph(dev, 1)
        rp, trace = drive(dev, m, reqs, n_slots, max_rows, use, what=(hint, n_slots, max_rows))
        c = rp["counters"]
        if hint == "own":
            assert c["drafts_granted"] > 0
            assert c["drafts_accepted"] == c["drafts_granted"] and "all accepted" in outcomes(trace)
        if hint == "corrupt":
            assert 0 < c["drafts_granted"] and c["drafts_accepted"] < c["drafts_granted"]
        if use:
            assert all(t[1][1][0] == FREE for t in trace)
    finally:
        free_all(dev, reqs, m)


# ------------------------------------------------------------------ 3. no drafts anywhere: the plain chain's tables and tokens

@pytest.mark.parametrize("which", MODELS)
def test_a_spec_chain_without_drafts_is_the_plain_chain(dev, golden_dir, which):
    from tests.test_hip_q8_serve import admit, begin
    m = open_model(dev, golden_dir, which)
    rng = np.random.default_rng(5)
    sizes = [(1, 6), (3, 4), (11, 5), (2, 7)]
    reqs = [SReq(dev, m, rng, n, new, *((1.0, 0.9, 0.4) if i % 2 else (0.0, 0.9, 0.0))) for i, (n, new) in enumerate(sizes)]
    twins = [SReq(dev, m, rng, n, new) for n, new in sizes]
    try:
        for r, t in zip(reqs, twins):
            t.ctx = r.ctx
        tables = {}
        for kind in ("plain", "spec"):
            assert (begin(dev, m, 4, 6, 8) if kind == "plain" else begin_spec(dev, m, 4, 6, 8, 7, 0)) == 0
            for i, r in enumerate(reqs):
                eng = r.eng if kind == "spec" else twins[i].eng
                # (rama_q8_serve_admit on a spec chain admits with n_draft = 0; so does _admit_spec with n_draft 0)
                assert (admit(dev, i, r, eng=eng) if kind == "plain" or i % 2 else admit_spec(dev, i, r, K=0)) == 0
            tables[kind] = []
            for _ in range(14):
                assert steps(dev, 1) == 0
                s = stats(dev)
                tables[kind].append((s["rows"], s["slots"]))
            tables[kind].append([tokens(dev, i) for i in range(4)])
            if kind == "spec":
                ss = spec_stats(dev)
                assert ss["rows_draft"] == ss["drafts_wanted"] == ss["drafts_granted"] == 0 and ss["accepted_hist"][0] == ss["rows_decode"]
        assert tables["plain"] == tables["spec"]
        for i, r in enumerate(reqs):
            r.check(tables["spec"][-1][i], (which, i))
    finally:
        free_all(dev, reqs + twins, m)


# ------------------------------------------------------------------ 4. admissions while steps are in flight; polling

@pytest.mark.parametrize("graph", [0, 1])
def test_admission_into_a_finished_slot_while_a_block_is_in_flight(dev, golden_dir, graph):
    """all slots busy; a block of steps that runs past the first finish is enqueued at once; the finished word is watched by
    rama_q8_serve_poll alone, every poll sees a prefix of the final tokens and a set finished word only with all of them; the newcomer
    is admitted behind the steps still in flight, with drafts of its own"""
    m = open_model(dev, golden_dir, "synth15m")
    rng = np.random.default_rng(31 + graph)
    reqs = [SReq(dev, m, rng, 3, 6, K=7, hint="own"), SReq(dev, m, rng, 5, 30, 1.0, 0.9, 0.2, K=7, hint="corrupt"),
            SReq(dev, m, rng, 9, 30, K=4, N=2, periodic=3)]
    late = SReq(dev, m, rng, 12, 8, 0.7, 1.0, 0.45, K=7, hint="own")
    try:
        for r in reqs + [late]:
            r.solo()
        set_graph(dev, graph)
        assert begin_spec(dev, m, 3, 8, 30) == 0
        for i, r in enumerate(reqs):
            assert admit_spec(dev, i, r) == 0
        assert steps(dev, 24) == 0
        deadline = time.monotonic() + 60
        while True:                                               # no stream query, no synchronising call
            for i, r in enumerate(reqs):
                got, fin, _ = poll(dev, i)
                assert got == r.want()[:len(got)] and (not fin or got == r.want()), i
            if poll(dev, 0)[1]:
                break
            assert time.monotonic() < deadline, "slot 0 never finished"
        assert admit_spec(dev, 0, late) == 0
        assert steps(dev, 30) == 0
        assert dev.lib.rama_sync(dev.ctx) == 0
        for i, r in enumerate([late] + reqs[1:]):
            assert poll(dev, i)[1]
            r.check(tokens(dev, i), (graph, i))
        assert stats(dev)["captures"] == (1 if graph else 0) and stats(dev)["generation"][0] == 2
    finally:
        free_all(dev, reqs + [late], m)


# ------------------------------------------------------------------ 5. prompt caching next to drafts

def test_fork_from_a_live_speculating_donor_and_admit_at_with_drafts(dev, golden_dir):
    """the donor speculates (rows at and behind its cursor may hold rejected drafts); rows BELOW its cursor, as far as the host has seen
    its tokens, are forked into another engine, which is admitted over them with drafts on and continues the donor's text"""
    m = open_model(dev, golden_dir, "synth15m")
    rng = np.random.default_rng(41)
    donor = SReq(dev, m, rng, 6, 40, K=7, N=2, hint="corrupt")
    heir = SReq(dev, m, rng, 2, 9, 1.0, 0.9, 0.7, K=7, N=3)
    try:
        donor.solo()
        set_graph(dev, 1)
        assert begin_spec(dev, m, 2, 12, 40) == 0
        assert admit_spec(dev, 0, donor) == 0
        assert steps(dev, 6) == 0
        assert dev.lib.rama_sync(dev.ctx) == 0
        seen = poll(dev, 0)[0]
        assert 6 <= len(seen) < 40 and not poll(dev, 0)[1]
        heir.ctx = donor.ctx + seen                               # the rows of all of it but the last token lie below the donor's cursor
        heir.n_cached = len(heir.ctx) - 1
        heir.hint = heir.ctx + heir.solo()
        assert dev.lib.rama_q8_kv_fork(dev.ctx, C.byref(m.ccfg), C.byref(donor.eng.state), C.byref(heir.eng.state), 1, heir.n_cached) == 0
        assert admit_spec(dev, 1, heir) == 0                      # rama_q8_serve_admit_at's cursor, with drafts
        assert steps(dev, 40) == 0
        assert dev.lib.rama_sync(dev.ctx) == 0
        for i, r in enumerate([donor, heir]):
            assert poll(dev, i)[1]
            r.check(tokens(dev, i), i)
        ss = spec_stats(dev)
        assert 0 < ss["drafts_accepted"] and ss["rows_prompt"] == len(donor.ctx) + 1
    finally:
        free_all(dev, [donor, heir], m)


# ------------------------------------------------------------------ 6. the server

def test_server_with_drafts_against_solo_runs_and_the_plain_server(dev, golden_dir):
    """Q8Server(n_draft=7): 10 requests through 3 slots; the tokens of the solo runs and of Q8Server(n_draft=0)"""
    import rama_amd
    m = open_model(dev, golden_dir, "synth15m")
    rng = np.random.default_rng(51)
    plans = [(0.0, 0.9, 0.0), (1.0, 0.9, 0.12), (0.7, 1.0, 0.9)]
    reqs = [SReq(dev, m, rng, int(rng.integers(1, 20)), int(rng.integers(3, 14)), *plans[i % 3], hint="own" if i % 2 else None, periodic=i % 2 == 0 and 2)
            for i in range(10)]
    try:
        reqs[4].stop = reqs[4].solo()[len(reqs[4].solo()) // 2]
        results = {}
        for K in (7, 0):
            set_graph(dev, 1)
            srv = rama_amd.Q8Server(m, 3, max_rows=12, max_new_cap=16, n_draft=K, ngram=3, hint_cap=HINT_CAP if K else 0)
            hs = [srv.submit(r.ctx, r.max_new, r.T, r.topp, r.u, None if r.stop < 0 else r.stop,
                             **(dict(hint=r.hint, n_draft=None if i % 3 else 3) if K else {})) for i, r in enumerate(reqs)]
            streamed = {h: [] for h in hs}
            srv.run(on_token=lambda h, k, t: streamed[h].append((k, t)))
            st = srv.stats()
            assert all(srv.finished(h) for h in hs)
            results[K] = [srv.result(h) for h in hs]
            assert all([t for _, t in streamed[h]] == srv.result(h) and [k for k, _ in streamed[h]] == list(range(len(srv.result(h)))) for h in hs)
            assert ("spec" in st) == bool(K)
            if K:
                assert st["spec"]["drafts_accepted"] > 0 and st["spec"]["tokens_emitted"] == sum(len(r) for r in results[K])
            srv.close()
        assert results[7] == results[0] == [r.want() for r in reqs]
    finally:
        free_all(dev, reqs, m)


# ------------------------------------------------------------------ 7. refusals and lifetimes

@pytest.mark.parametrize("graph", [0, 1])
def test_refusals_leave_the_running_chain_as_it_was(dev, golden_dir, graph):
    from tests.test_hip_q8_serve import admit, begin
    m = open_model(dev, golden_dir, "ckpt_v2_q80_untied")
    V = m.cfg.vocab_size
    rng = np.random.default_rng(61)
    reqs = [SReq(dev, m, rng, 3, 9, 1.0, 0.9, 0.3, K=5, hint="own"), SReq(dev, m, rng, 11, 7, K=3, N=2, periodic=2)]
    extra = SReq(dev, m, rng, 4, 6, K=5, hint="own")
    try:
        for bad in [(16, 8), (-1, 8), (3, -1)]:                   # n_draft_cap in 0..15, hint_cap >= 0; and rama_q8_serve_begin's own checks
            assert begin_spec(dev, m, 3, 8, 12, *bad) == EINVAL
        assert begin_spec(dev, m, 4, 3, 12) == EINVAL and begin_spec(dev, m, 3, 8, 0) == EINVAL and begin_spec(dev, m, 0, 8, 12) == EINVAL
        assert begin(dev, m, 3, 8, 12) == 0                       # a plain chain takes no drafting admission and has no spec report
        assert admit_spec(dev, 0, extra) == EINVAL
        from rama_amd._lib import rama_q8_serve_spec_report
        assert dev.lib.rama_q8_serve_spec_stats(dev.ctx, C.byref(rama_q8_serve_spec_report())) == EINVAL
        assert admit(dev, 0, extra) == 0 and steps(dev, 1) == 0   # ... and is intact
        set_graph(dev, graph)
        assert begin_spec(dev, m, 3, 8, 12, 5, 20) == 0
        for i, r in enumerate(reqs):
            assert admit_spec(dev, i, r) == 0
        assert steps(dev, 2) == 0
        refused = [
            admit_spec(dev, 2, extra, K=6),                       # beyond n_draft_cap
            admit_spec(dev, 2, extra, K=-1),
            admit_spec(dev, 2, extra, N=0), admit_spec(dev, 2, extra, N=5),
            admit_spec(dev, 2, extra, hint=[1] * 21),             # beyond hint_cap
            admit_spec(dev, 2, extra, hint=[1, V]), admit_spec(dev, 2, extra, hint=[-1]),
            admit_spec(dev, 2, extra, null=True),
            admit_spec(dev, 0, extra),                            # serve_admit's own: a busy slot, a live run state, sizes
            admit_spec(dev, 2, extra, eng=reqs[1].eng),
            admit_spec(dev, 2, extra, n_cached=len(extra.ctx)),
            admit_spec(dev, 2, extra, ctx=[1] * (m.cfg.seq_len - 5)),
            admit_spec(dev, 2, extra, ctx=[1, V]),
            admit_spec(dev, 3, extra), admit_spec(dev, -1, extra),
        ]
        assert refused == [EINVAL] * len(refused)
        assert dev.lib.rama_q8_serve_spec_stats(dev.ctx, None) == EINVAL and steps(dev, -1) == EINVAL
        assert admit_spec(dev, 2, extra) == 0                     # ... and a good one still goes in
        assert steps(dev, 16) == 0
        assert dev.lib.rama_sync(dev.ctx) == 0
        for i, r in enumerate(reqs + [extra]):
            assert poll(dev, i)[1]
            r.check(tokens(dev, i), (graph, i))
        assert stats(dev)["captures"] == (1 if graph else 0)
    finally:
        free_all(dev, reqs + [extra], m)


def test_steps_refuse_after_a_free(dev, golden_dir):
    """rama_state_free of an occupied slot's run state, or rama_q8_model_free, ends a chain with drafts as it ends a plain one; a
    finished occupant's state may go"""
    for what in ("state", "done_state", "model"):
        m = open_model(dev, golden_dir, "ckpt_v2_q80_untied")
        rng = np.random.default_rng(9)
        reqs = [SReq(dev, m, rng, 3, 2, K=3, hint="own"), SReq(dev, m, rng, 4, 20, K=0)]
        try:
            for r in reqs:
                r.solo()
            set_graph(dev, 1)
            assert begin_spec(dev, m, 2, 6, 20) == 0
            for i, r in enumerate(reqs):
                assert admit_spec(dev, i, r) == 0
            assert steps(dev, 3) == 0
            assert dev.lib.rama_sync(dev.ctx) == 0
            assert poll(dev, 0)[1] and not poll(dev, 1)[1]
            if what == "state":
                reqs[1].eng.free()
                assert steps(dev, 1) == EINVAL and admit_spec(dev, 0, reqs[0]) == EINVAL
            elif what == "done_state":
                reqs[0].eng.free()
                assert steps(dev, 1) == 0
            else:
                m.free()
                assert steps(dev, 1) == EINVAL
            assert dev.lib.rama_q8_serve_end(dev.ctx) == 0
            assert steps(dev, 1) == EINVAL
        finally:
            set_graph(dev, 0)
            dev.lib.rama_q8_serve_end(dev.ctx)
            for r in reqs:
                r.twin.free(); r.eng.free()
            m.free()
