"""Cancel, priorities, preemption and resume on the host (no GPU): the replays with `cancels` against a straightforward restatement of the
cancel rule over random tables and whole workloads; and ServeLoop over a stand-in library that records (entry, scalar arguments) -- the
stand-in of tests/test_serve_loop_host.py with a finished WORD per slot -- for the exact call order of cancel, preempt and resume on both
ABIs, the queue order under priorities, the victim, the engines' books and every ValueError before any library call."""
import ctypes as C
import random

import pytest

from rama_amd.q8_replay import (SERVE_DECODE as DECODE, SERVE_DONE as DONE, SERVE_FREE as FREE, SERVE_PROMPT as PROMPT, _spec_plan_py,
                                serve_model_replay, serve_replay, serve_spec_replay)

ABIS = ["rama_q8_serve", "rama_serve"]
CANCELLED = 2


# ------------------------------------------------------------------ the rule, restated

def plain_run(table, max_rows, cancels, n_steps):
    """the plain chain, one token per DECODE slot and step, no stop tokens: table = [state, n_context, cursor, n_out, max_new] lists ->
    per step (the slots a cancel ended before it, its rows, the table after it)"""
    t, out = [list(s) for s in table], []
    for k in range(n_steps):
        hit = [i for i in sorted(set(cancels.get(k, []))) if t[i][0] in (PROMPT, DECODE)]
        for i in hit:
            t[i][0] = DONE                                   # the state, and nothing else
        rows, _ = _spec_plan_py(t, [0] * len(t), max_rows)
        for i, s in enumerate(t):
            n = sum(1 for r in rows if r[0] == i)
            if n == 0:
                continue
            if s[0] == PROMPT and s[2] + n < s[1]:
                s[2] += n
                continue
            s[2] = s[1] if s[0] == PROMPT else s[2] + 1
            s[3] += 1
            s[0] = DONE if s[3] >= s[4] else DECODE
        out.append((hit, rows, [tuple(s) for s in t]))
    return out


@pytest.mark.parametrize("seed", range(12))
def test_replays_with_cancels_equal_the_restated_rule_on_random_workloads(seed):
    rng = random.Random(seed)
    n_slots = rng.randint(1, 6)
    max_rows = rng.randint(n_slots, n_slots + 6)
    reqs = [dict(context=[1] + [rng.randint(2, 60) for _ in range(rng.randint(0, 12))], max_new=rng.randint(1, 9)) for _ in range(n_slots)]
    refs = [[rng.randint(2, 60) for _ in range(r["max_new"])] for r in reqs]
    # (steps from 1 on: a cancel before step 0 comes before the admissions and finds nobody)
    cancels = {rng.randint(1, 8): [rng.randrange(n_slots) for _ in range(rng.randint(1, 3))] for _ in range(rng.randint(1, 4))}
    got = serve_replay(reqs, refs, n_slots, max_rows, cancels=cancels)
    table = [[PROMPT, len(r["context"]), 0, 0, r["max_new"]] for r in reqs]
    want = plain_run(table, max_rows, cancels, len(got["steps"]))
    assert got["steps"], seed
    for k, (st, (hit, rows, after)) in enumerate(zip(got["steps"], want)):
        assert (st["cancelled"], st["rows"], st["slots"]) == (hit, rows, after), (seed, k)
    # a cancelled request has the first tokens of its run, the others all of theirs; nobody lives on (a cancel that ends the last live
    # slot ends the replay before a further step)
    final = want[-1][2]
    last = [i for i in set(cancels.get(len(want), [])) if final[i][0] in (PROMPT, DECODE)]
    for q, r in enumerate(reqs):
        at, n = got["cancelled_at"][q], final[q][3]
        assert got["outputs"][q] == refs[q][:n] and (n == r["max_new"]) == (at is None) == (got["finish_step"][q] is not None), (seed, q)
    assert all(s[0] == DONE or i in last for i, s in enumerate(final))
    # the same schedule on the two kinds of chain with drafts, nobody drafting: the same steps
    for other in (serve_spec_replay(reqs, refs, n_slots, max_rows, cancels=cancels),
                  serve_model_replay(reqs, refs, lambda p, n: [0] * n, n_slots, max_rows, cancels=cancels)):
        assert [(s["cancelled"], s["rows"], s["slots"]) for s in other["steps"]] == [(s["cancelled"], s["rows"], s["slots"]) for s in got["steps"]]
        assert other["outputs"] == got["outputs"] and other["cancelled_at"] == got["cancelled_at"]


def test_replay_without_cancels_is_unchanged_and_a_cancel_changes_the_state_only():
    reqs = [dict(context=[1, 5, 6], max_new=6, n_draft=3, ngram=2, hint=[5, 6, 7, 8]), dict(context=[1, 9], max_new=4)]
    refs = [[7, 8, 9, 10, 11, 12], [3, 4, 5, 6]]
    a = serve_spec_replay(reqs, refs, 2, 6)
    assert "cancelled_at" not in a and all("cancelled" not in s for s in a["steps"])
    b = serve_spec_replay(reqs, refs, 2, 6, cancels={})
    assert [{k: v for k, v in s.items() if k != "cancelled"} for s in b["steps"]] == a["steps"] and b["cancelled_at"] == [None, None]
    reqs, refs = reqs + [dict(context=[1, 3], max_new=5)], refs + [[2, 3, 4, 5, 6]]
    c = serve_spec_replay(reqs, refs, 3, 6, cancels={2: [0, 0, 1]})
    before, after = c["steps"][1]["slots"], c["steps"][2]["slots"]
    assert c["steps"][2]["cancelled"] == [0, 1] and c["cancelled_at"] == [2, 2, None]
    assert [s[1:] for s in after[:2]] == [s[1:] for s in before[:2]] and [s[0] for s in after] == [DONE, DONE, DECODE]
    assert c["steps"][2]["rows"] == [(2, before[2][2], 1)] + [(-1, -1, 0)] * 5 and c["steps"][2]["want"] == [0, 0, 0]
    assert c["outputs"] == [refs[0][:before[0][3]], refs[1][:before[1][3]], refs[2]]


def test_a_continuation_replays_to_the_tokens_of_the_uninterrupted_run():
    """cancel after step k, then the continuation -- context ++ outputs, n_cached = cursor, the budget left -- admitted not before step k + 2"""
    ctx, ref = [1, 4, 5, 6, 7], [9, 8, 7, 6, 5, 4, 3]
    whole = serve_replay([dict(context=ctx, max_new=7)], [ref], 1, 3)
    for k in range(1, 8):
        first = serve_replay([dict(context=ctx, max_new=7)], [ref], 1, 3, cancels={k: [0]})
        s = first["steps"][k - 1]["slots"][0]
        n = s[3]
        if s[0] == DONE:
            assert first["outputs"] == [ref] and first["cancelled_at"] == [None]
            continue
        cont = dict(context=ctx + ref[:n], max_new=7 - n, n_cached=min(s[2], len(ctx) + n - 1), after_step=k + 2)
        both = serve_replay([dict(context=ctx, max_new=7), cont], [ref, ref[n:]], 1, 3, cancels={k: [0]})
        assert both["outputs"][0] + both["outputs"][1] == ref == whole["outputs"][0], k
        assert both["steps"][k]["rows"] == [(-1, -1, 0)] * 3 and both["steps"][k + 2]["admitted"] == [(0, 1)], k
        # the one row fed again is the last position (or the rest of a context the cancel cut short)
        assert both["steps"][k + 2]["rows"][0] == (0, cont["n_cached"], 1 if cont["n_cached"] == len(cont["context"]) - 1 else 0), k


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_model_replay_cancels_a_drafting_slot_and_its_draft_cursor_stays(k):
    """two slots that both draft with a draft model (slot 0's drafts are right, slot 1's are wrong); slot 0 is cancelled before step k"""
    ctx0, ref0 = [1, 4, 5], [9, 8, 7, 6, 5, 4, 3, 2, 11, 12, 13, 14, 15, 16, 17, 18]      # (at most 3 tokens a step: DECODE until step 5)
    ctx1, ref1 = [1, 6], [20, 21, 22, 23, 24, 25, 26, 27]
    right = lambda prefix, n: (ctx0 + ref0)[len(prefix):len(prefix) + n]
    wrong = lambda prefix, n: [50] * n
    reqs = [dict(context=ctx0, max_new=16, n_draft=2), dict(context=ctx1, max_new=8, n_draft=3)]
    whole = serve_model_replay(reqs, [ref0, ref1], [right, wrong], 2, 6, cancels={})
    cut = serve_model_replay(reqs, [ref0, ref1], [right, wrong], 2, 6, cancels={k: [0]})
    assert cut["steps"][:k] == [dict(s, cancelled=[]) for s in whole["steps"][:k]]                # nothing changes before the cancel
    before = cut["steps"][k - 1]
    assert before["slots"][0][0] == DECODE and 0 in before["drafting"] and cut["cancelled_at"] == [k, None]
    for st in cut["steps"][k:]:
        assert st["slots"][0] == (DONE,) + before["slots"][0][1:] and st["cursors"][0] == before["cursors"][0]
        assert st["want"][0] == 0 and st["granted"][0] == 0 and 0 not in st["drafting"] and all(r[0] != 0 for r in st["rows"])
    n = before["slots"][0][3]
    assert cut["outputs"] == [ref0[:n], ref1] and cut["cursor"][0] == before["cursors"][0] and cut["finish_step"][0] is None
    assert cut["steps"][k]["cancelled"] == [0] and cut["counters"]["drafts_wanted"] < whole["counters"]["drafts_wanted"]
    # the continuation drafts again from a draft cursor at its new context's end, and the tokens are the uninterrupted run's
    cont = dict(context=ctx0 + ref0[:n], max_new=16 - n, n_draft=2, n_cached=min(before["slots"][0][2], len(ctx0) + n - 1), after_step=k + 1)
    both = serve_model_replay(reqs + [cont], [ref0, ref1, ref0[n:]], [right, wrong, right], 2, 6, cancels={k: [0]})
    assert both["outputs"][0] + both["outputs"][2] == ref0 and both["outputs"][1] == ref1 and both["slot"][2] == 0
    assert both["steps"][k + 1]["admitted"] == [(0, 2)] and both["steps"][k + 1]["cursors"][0] == len(ctx0) + n
    assert any(0 in st["drafting"] for st in both["steps"][k + 2:])


# ------------------------------------------------------------------ the stand-in device (tests/test_serve_loop_host.py's, with a finished word)

class Lib:
    """records (entry, scalar arguments) and answers 0.  A poll of a slot in `finish` gives that slot's tokens and its finished word
    (tokens, word), of any other slot nothing; stats gives the slot table `slots`; a cancel records the slots of its list."""

    def __init__(self):
        self.calls, self.finish, self.slots = [], {}, []

    def __getattr__(self, name):
        def entry(*a):
            scalars = tuple(v for v in a if isinstance(v, (int, float)))
            if name.endswith("_serve_cancel"):             # (ctx, slots, n)
                scalars = (tuple(a[1][:a[2]]), a[2])
            self.calls.append((name, scalars))
            if name.endswith("_serve_poll"):               # (ctx, slot, start, tokens, 64, &n, &finished, NULL)
                toks, word = self.finish.get(a[1], ([], 0))
                toks = toks[a[2]:a[2] + a[4]]
                for i, t in enumerate(toks):
                    a[3][i] = t
                a[5]._obj.value, a[6]._obj.value = len(toks), word
            if name.endswith("_serve_stats"):              # (ctx, &report)
                r = a[1]._obj
                r.n_slots, r.max_rows = len(self.slots), 4
                for i, s in enumerate(self.slots):
                    r.slots[i].state, r.slots[i].n_context, r.slots[i].cursor, r.slots[i].n_out, r.slots[i].max_new = s
            return 0
        return entry


class Cfg:
    vocab_size, seq_len = 512, 64


class Model:
    def __init__(self, cfg=Cfg):
        class Device:
            lib, ctx = Lib(), None
        self.device, self.cfg, self.ccfg, self.weights = Device(), cfg(), C.c_int(), C.c_int()


class Engine:
    def __init__(self, device, model):
        self.model, self.state, self.freed = model, C.c_int(), False

    def free(self):
        self.freed = True


@pytest.fixture(params=ABIS)
def stand_in(request, monkeypatch):
    import rama_amd
    from rama_amd import q8, server
    monkeypatch.setattr(q8, "Q8Engine", Engine)
    monkeypatch.setattr(server, "Engine", Engine)
    cls = {"rama_q8_serve": rama_amd.Q8Server, "rama_serve": rama_amd.Server}[request.param]
    return cls, request.param, cls.NAME


def trace(model, clear=True):
    out = [c for c in model.device.lib.calls if not c[0].endswith("_poll")]
    if clear:
        del model.device.lib.calls[:]
    return out


# ------------------------------------------------------------------ cancel

def test_cancel_of_a_queued_a_running_and_a_finished_request(stand_in):
    cls, A, _ = stand_in
    m = Model()
    lib = m.device.lib
    srv = cls(m, 1, 4, 8)
    a, b = srv.submit([1, 2, 3], 4), srv.submit([1, 2], 4)
    assert trace(m) == [(A + "_begin", (1, 4, 8)), (A + "_admit", (0, 3))]
    srv.cancel(b)                                            # queued: it leaves the queue, no call
    assert trace(m) == [] and srv.finished(b) and srv.cancelled(b) and srv.result(b) == [] and srv._queue == []
    srv.cancel(a)                                            # running: the entry, and the mirror DONE behind the steps enqueued
    assert trace(m) == [(A + "_cancel", ((0,), 1))] and srv._mirror[0] == (DONE, 3, 0, 0, 4)
    assert not srv.finished(a) and not srv.cancelled(a)
    srv.cancel(a)                                            # once is enough
    assert trace(m) == []
    lib.finish[0] = ([7, 8], CANCELLED)
    seen = []
    srv.poll(lambda h, i, t: seen.append((h, i, t)))
    assert srv.finished(a) and srv.cancelled(a) and srv.result(a) == [7, 8] and seen == [(a, 0, 7), (a, 1, 8)]
    assert trace(m) == [] and srv._req == [None] and srv._own[0] is not None and srv._spare == []
    srv.cancel(a)                                            # finished: nothing
    assert trace(m) == []
    # one that finishes by itself before the cancel runs is not cancelled
    del lib.finish[0]
    c = srv.submit([1, 2], 3)
    srv.cancel(c)
    lib.finish[0] = ([4, 5, 6], 1)
    srv.poll()
    assert srv.finished(c) and not srv.cancelled(c) and srv.result(c) == [4, 5, 6]
    srv.close()


def test_cancel_from_a_callback_inside_run_returns(stand_in):
    cls, A, _ = stand_in
    m = Model()
    lib = m.device.lib
    srv = cls(m, 1, 4, 8)
    a = srv.submit([1, 2, 3], 6)
    trace(m)
    lib.finish[0] = ([7], 0)                                 # one token, not finished: the callback cancels, and the word follows the entry

    def on_token(h, i, t):
        srv.cancel(h)
        lib.finish[0] = ([7], CANCELLED)
    m.device.lib.rama_stream_query = lambda ctx: 0
    srv.run(on_token)
    assert srv.finished(a) and srv.cancelled(a) and srv.result(a) == [7]
    assert (A + "_cancel", ((0,), 1)) in trace(m)
    srv.close()


# ------------------------------------------------------------------ priorities and preemption

def test_queue_order_under_priorities(stand_in):
    cls, A, _ = stand_in
    m = Model()
    srv = cls(m, 1, 4, 8)
    srv.submit([1, 2], 2)
    hs = [srv.submit([1, 2], 2, priority=p) for p in (0, 5, 1, 5, 0, 9)]
    assert srv._queue == [hs[5], hs[1], hs[3], hs[2], hs[0], hs[4]]
    assert [c[0] for c in trace(m)] == [A + "_begin", A + "_admit"]          # no preemption unless asked for
    srv.close()


def test_preempt_picks_the_victim_and_resumes_it_on_its_engine(stand_in):
    cls, A, _ = stand_in
    m = Model()
    lib = m.device.lib
    srv = cls(m, 2, 4, 8, preempt=True)
    a = srv.submit([1, 2, 3], 6, temperature=1.0, topp=0.5, u=0.25, stop_token=9, priority=1)
    b = srv.submit([1, 2], 6, priority=0)
    c = srv.submit([1, 4], 6, priority=0)                    # equal to the lowest running: waits
    assert trace(m) == [(A + "_begin", (2, 4, 8)), (A + "_admit", (0, 3)), (A + "_admit", (1, 2))] and srv._queue == [c]
    own_b = srv._own[1]
    d = srv.submit([1, 5], 2, priority=3)                    # outranks both: the lowest priority goes -- b, not the longer-running a
    assert trace(m) == [(A + "_cancel", ((1,), 1))] and srv._queue == [d, c] and srv._ending == {b: "preempt"}
    e = srv.submit([1, 6], 2, priority=3)                    # a second one: the next victim is a (priority 1 < 3)
    assert trace(m) == [(A + "_cancel", ((0,), 1))] and srv._queue == [d, e, c]
    srv.submit([1, 7], 2, priority=3)                        # nobody is left to preempt
    assert trace(m) == []
    # b's word shows: cancelled after two tokens at cursor 3 -> a continuation on its engine, at the front of its priority
    lib.finish[1] = ([11, 12], CANCELLED)
    lib.slots = [(DECODE, 3, 5, 2, 6), (DONE, 2, 3, 2, 6)]
    seen = []
    srv.poll(lambda h, i, t: seen.append((h, i, t)))
    assert srv.preemptions == 1 and not srv.finished(b) and not srv.cancelled(b) and srv.result(b) == [11, 12]
    assert srv._plans[b][:2] == ([1, 2, 11, 12], (0.0, 0.9, srv._plans[b][1][2], 4, -1)) and srv._plans[b][2] is own_b and srv._plans[b][3] == 3
    assert srv._own[1] is None and srv._req[1] is None and srv._queue[-2:] == [b, c]
    assert trace(m) == [(A + "_stats", ())]
    del lib.finish[1]
    srv.step(0)                                              # d takes slot 1 on a fresh engine of the server's
    assert trace(m) == [(A + "_admit", (1, 2))] and srv._req[1] == d and srv._own[1] is not own_b
    # a's word shows: one token, cursor 3 = n_context of the continuation - 1
    lib.finish[0] = ([21], CANCELLED)
    lib.slots = [(DONE, 3, 3, 1, 6), (PROMPT, 2, 0, 0, 2)]
    srv.poll()
    assert srv.preemptions == 2 and srv._plans[a][0] == [1, 2, 3, 21] and srv._plans[a][1] == (1.0, 0.5, 0.25, 5, 9) and srv._plans[a][3] == 3
    del lib.finish[0]
    trace(m)
    srv.step(0)
    assert trace(m) == [(A + "_admit", (0, 2))] and srv._req[0] == e
    # d and e finish; the next of the queue is the third urgent one, then a (priority 1), then b before c
    lib.finish = {0: ([1, 2], 1), 1: ([3, 4], 1)}
    srv.poll()
    lib.finish = {}
    srv.step(0)
    assert [c for c in trace(m) if not c[0].endswith("_stats")] == [(A + "_admit", (0, 2)), (A + "_admit_at", (1, 4, 3))] and srv._req[1] == a and srv._eng[1] is srv._plans[a][2]
    lib.finish = {1: ([22, 9], 1)}                           # a's continuation stops: indices run on, the engine is spare again
    srv.poll(lambda h, i, t: seen.append((h, i, t)))
    assert srv.finished(a) and srv.result(a) == [21, 22, 9] and seen[-2:] == [(a, 1, 22), (a, 2, 9)]
    assert any(x is srv._plans[a][2] for x in srv._spare) and srv.stats()["preemptions"] == 2
    srv.close()
    assert all(x.freed for x in srv._mine) or srv._mine == []


def test_suspend_and_resume_are_the_two_halves(stand_in):
    cls, A, _ = stand_in
    m = Model()
    lib = m.device.lib
    srv = cls(m, 1, 4, 8)
    mine = Engine(None, m)
    a = srv.submit([1, 2, 3], 5, engine=mine)
    q = srv.submit([1, 2], 2)
    trace(m)
    srv.suspend(q)                                           # queued: it waits outside the queue, no call
    assert trace(m) == [] and srv._queue == [] and srv._suspended == {q}
    srv.suspend(a)
    assert trace(m) == [(A + "_cancel", ((0,), 1))]
    with pytest.raises(ValueError, match="suspend"):
        srv.suspend(a)
    lib.finish[0] = ([7, 8, 9], CANCELLED)
    lib.slots = [(DONE, 3, 5, 3, 5)]
    srv.poll()
    assert srv._suspended == {q, a} and srv.preemptions == 0 and not srv.finished(a) and srv._queue == [] and srv._req == [None]
    with pytest.raises(ValueError, match="already serves"):
        srv.submit([1, 2], 2, engine=mine)                   # the engine stays with the handle while it waits
    del lib.finish[0]
    trace(m)
    srv.resume(a)
    assert trace(m) == [(A + "_admit_at", (0, 6, 5))] and srv._eng[0] is mine and srv._suspended == {q}
    with pytest.raises(ValueError, match="resume"):
        srv.resume(a)
    srv.cancel(q)
    assert srv.cancelled(q) and srv._suspended == set()
    lib.finish[0] = ([4, 5], 1)
    srv.poll()
    assert srv.result(a) == [7, 8, 9, 4, 5] and srv.finished(a) and not mine.freed and srv._spare == []
    srv.close()


def test_a_cancelled_request_with_retain_leaves_a_donor_keyed_by_the_rows_it_holds(stand_in):
    cls, A, _ = stand_in
    m = Model()
    lib = m.device.lib
    srv = cls(m, 1, 4, 8, prefix_cache=2)
    a = srv.submit([1, 2, 3], 6, retain=True)
    eng = srv._eng[0]
    srv.cancel(a)
    lib.finish[0] = ([7, 8, 9], CANCELLED)
    srv.poll()
    assert srv.cancelled(a) and eng in srv.pool and srv.pool._donors == [[[1, 2, 3, 7, 8], eng]] and srv._own[0] is None
    # cancelled inside its context: the rows below the cursor
    lib.finish = {}
    b = srv.submit([1, 2, 3, 4, 5, 6], 2, retain=True)
    eng_b = srv._eng[0]
    srv.cancel(b)
    lib.finish[0] = ([], CANCELLED)
    lib.slots = [(DONE, 6, 4, 0, 2)]
    srv.poll()
    assert srv.pool._donors[-1] == [[1, 2, 3, 4], eng_b]
    srv.close()


def test_every_refusal_comes_before_any_call(stand_in):
    cls, A, NAME = stand_in
    m = Model()
    srv = cls(m, 1, 4, 8)
    a = srv.submit([1, 2], 2)
    trace(m)
    for call, text in ((lambda: srv.cancel(99), f"{NAME}.cancel: no request 99"), (lambda: srv.cancelled(99), f"{NAME}.cancelled: no request 99"),
                       (lambda: srv.suspend(99), f"{NAME}.suspend: no request 99"), (lambda: srv.resume(99), f"{NAME}.resume: no request 99"),
                       (lambda: srv.resume(a), f"{NAME}.resume: request {a} is not suspended")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    with pytest.raises(ValueError):
        srv.submit([1, 2], 2, priority="urgent")
    assert trace(m) == []
    m.device.lib.finish[0] = ([3, 4], 1)
    srv.poll()
    trace(m)
    with pytest.raises(ValueError, match="has finished"):
        srv.suspend(a)
    assert trace(m) == []
    srv.close()
