"""CPU: rama_pipe_tick_plan (csrc/pipe.hip) alone, for every rank and every tick of 675 plans (tests/pipe_plan_cases.py GRID: world x
n_seq x n_pos x wrap x n_prompt), ticks 0 .. rama_pipe_plan_ticks + 1.  The plan is pure arithmetic and librama_hip.so loads without a
GPU, so the bookkeeping the first run on N > 1 GPUs rests on is pinned here: a send without its receive is a rendezvous that never
completes, not a wrong number.

  matching   every tick's sends over all ranks are that tick's receives
  dataflow   a symbolic run: what every stage pass reads was written by the pass it depends on, every history cell is written once
  fields     pos_wrapped, token_kind / token, samples, idle slots and idle ticks, against the rule of DESIGN.md's schedule section
  schedule   item, sends and receives equal rama_amd.pipeline.Schedule wherever Schedule takes the case (n_seq >= world)
  refusals   -1 and *out untouched for every bad argument"""
import ctypes as C
import functools

import pytest

from . import pipe_plan_cases as P


@pytest.fixture(scope="module")
def lib():
    import rama_amd
    return rama_amd.load()


@functools.lru_cache(maxsize=None)
def _table(case):
    """case -> (n_ticks, rows): rows[tick][rank] = the rama_pipe_tick, for ticks 0 .. n_ticks + 1 (computed once, shared by the tests)"""
    import rama_amd
    lib = rama_amd.load()
    world, n_seq, n_pos, wrap, n_prompt = case
    plan = P.make_plan(n_seq, n_pos, wrap, P.GRID_PROMPT[:n_prompt])
    n_ticks = P.plan_ticks(lib, plan, world)
    return n_ticks, [[P.tick(lib, plan, world, r, t) for r in range(world)] for t in range(n_ticks + 2)]


def test_grid_has_the_675_cases():
    assert len(P.GRID) == 675 and len(set(P.GRID)) == 675


def test_every_send_has_its_receive_in_the_same_tick():
    for case in P.GRID:
        world = case[0]
        last = world - 1
        _, rows = _table(case)
        for t, row in enumerate(rows):
            sends = {(r, k.send_peer, k.send_kind, k.send_seq) for r, k in enumerate(row) if k.send_kind != P.NONE}
            recvs = {(k.recv_peer, r, k.recv_kind, k.recv_seq) for r, k in enumerate(row) if k.recv_kind != P.NONE}
            assert sends == recvs, (case, t, sends, recvs)
            for src, dst, kind, _ in sends:
                assert world > 1, (case, t)
                # x to the next rank, the token from the last rank to rank 0, nothing else
                assert (kind, dst) == ((P.X, src + 1) if src < last else (P.TOKEN, 0)), (case, t, src, dst, kind)
            for k in row:
                assert k.send_kind in (P.NONE, P.X, P.TOKEN) and k.recv_kind in (P.NONE, P.X, P.TOKEN), (case, t)


def test_symbolic_dataflow_writes_every_history_cell_once():
    for case in P.GRID:
        world, n_seq, n_pos, wrap, n_prompt = case
        _, rows = _table(case)
        x_tag = [dict() for _ in range(world)]        # rank -> seq -> what its x buffer holds: (seq, pos, rank that wrote it)
        tok_tag = [dict() for _ in range(world)]      # rank -> seq -> what its token word holds: (seq, pos sampled after)
        written = {}
        for t, row in enumerate(rows):
            for r, k in enumerate(row):
                if not k.on:
                    continue
                if r > 0:
                    assert x_tag[r].get(k.seq) == (k.seq, k.pos, r - 1), (case, t, r, x_tag[r].get(k.seq))
                elif k.token_kind == P.TOKEN_WORD:
                    assert tok_tag[0].get(k.seq) == (k.seq, k.pos - 1), (case, t, tok_tag[0].get(k.seq))
                x_tag[r][k.seq] = (k.seq, k.pos, r)
                if k.samples:
                    tok_tag[r][k.seq] = (k.seq, k.pos)
                    if world == 1:      # the sampling rank writes the history itself (rama_pipe_run_ticks, world == 1)
                        written[(k.seq, k.pos)] = written.get((k.seq, k.pos), 0) + 1
            # a grouped exchange: every send buffer is read before any receive lands
            flying = {}
            for r, k in enumerate(row):
                if k.send_kind != P.NONE:
                    src = x_tag[r] if k.send_kind == P.X else tok_tag[r]
                    assert k.send_seq in src, (case, t, r, "sends a buffer nothing was written to")
                    flying[(r, k.send_peer, k.send_kind, k.send_seq)] = src[k.send_seq]
            for r, k in enumerate(row):
                if k.recv_kind == P.NONE:
                    continue
                key = (k.recv_peer, r, k.recv_kind, k.recv_seq)
                assert key in flying, (case, t, r, key)
                tag = flying.pop(key)
                if k.recv_kind == P.X:
                    x_tag[r][k.recv_seq] = tag
                else:
                    assert r == 0 and tag == (k.recv_seq, k.recv_pos), (case, t, r, tag, k.recv_seq, k.recv_pos)
                    tok_tag[0][k.recv_seq] = tag
                    written[(k.recv_seq, k.recv_pos)] = written.get((k.recv_seq, k.recv_pos), 0) + 1
            assert not flying, (case, t, flying)
        assert written == {(s, p): 1 for s in range(n_seq) for p in range(n_pos)}, (case, written)


def test_fields_follow_the_documented_rule():
    for case in P.GRID:
        world, n_seq, n_pos, wrap, n_prompt = case
        n_ticks, rows = _table(case)
        slots = max(n_seq, world)
        for t, row in enumerate(rows):
            for r, k in enumerate(row):
                j = t - r
                on = 0 <= j < slots * n_pos and j % slots < n_seq
                assert k.on == int(on), (case, t, r)
                assert k.samples == int(on and r == world - 1), (case, t, r)
                if not on:
                    # an idle slot (seq >= n_seq) or an idle tick: no pass, no sample, nothing sent
                    assert k.send_kind == P.NONE, (case, t, r)
                    continue
                assert (k.seq, k.pos) == (j % slots, j // slots), (case, t, r)
                pw = k.pos % wrap if wrap else k.pos
                assert k.pos_wrapped == pw, (case, t, r, k.pos, k.pos_wrapped)
                if r > 0:
                    assert k.token_kind == P.TOKEN_WORD, (case, t, r)
                elif pw == 0:
                    assert (k.token_kind, k.token) == (P.TOKEN_BOS, P.BOS), (case, t, k.token_kind, k.token)
                elif pw <= n_prompt:
                    assert (k.token_kind, k.token) == (P.TOKEN_FORCED, P.GRID_PROMPT[pw - 1]), (case, t, k.token_kind, k.token)
                else:
                    assert k.token_kind == P.TOKEN_WORD, (case, t, k.token_kind)
            # nobody receives from an idle upstream neighbour
            for r, k in enumerate(row):
                up = row[r - 1 if r > 0 else world - 1]
                assert (k.recv_kind != P.NONE) == bool(world > 1 and up.on), (case, t, r)
        for row in rows[n_ticks:]:      # past the end: idle, no legs
            for k in row:
                assert (k.on, k.samples, k.send_kind, k.recv_kind) == (0, 0, P.NONE, P.NONE), case


def test_plan_agrees_with_the_python_schedule():
    from rama_amd.pipeline import Schedule
    names = {"x": P.X, "tok": P.TOKEN}
    for case in P.GRID:
        world, n_seq, n_pos, wrap, n_prompt = case
        n_ticks, rows = _table(case)
        assert n_ticks == max(n_seq, world) * n_pos + world - 1, case
        if n_seq < world:      # Schedule refuses these; the native plan idles the extra slots
            with pytest.raises(AssertionError):
                Schedule(world, n_seq, n_pos)
            continue
        sched = Schedule(world, n_seq, n_pos)
        assert n_ticks == sched.ticks, case
        for t, row in enumerate(rows):
            for r, k in enumerate(row):
                it = sched.item(r, t)
                assert k.on == int(it is not None), (case, t, r)
                if it is not None:
                    assert (k.seq, k.pos) == (it.seq, it.pos), (case, t, r)
                sends = [(names[kind], seq, peer) for kind, seq, peer in sched.sends(r, t)]
                recvs = [(names[kind], seq, peer) for kind, seq, peer in sched.recvs(r, t)]
                assert sends == ([(k.send_kind, k.send_seq, k.send_peer)] if k.send_kind != P.NONE else []), (case, t, r)
                assert recvs == ([(k.recv_kind, k.recv_seq, k.recv_peer)] if k.recv_kind != P.NONE else []), (case, t, r)


def test_refusals_leave_out_untouched(lib):
    from rama_amd._lib import rama_pipe_plan, rama_pipe_tick
    prompt = (C.c_int32 * 2)(11, 12)

    def plan(n_seq=2, n_pos=3, pr=prompt, n_prompt=2):
        return rama_pipe_plan(n_seq, n_pos, 0, pr, n_prompt, 0.0, 0.9, 0.0, None)

    def refused(pl, world, rank, with_out=True):
        out = rama_pipe_tick()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        before = bytes(out)
        rc = lib.rama_pipe_tick_plan(C.byref(pl) if pl is not None else None, world, rank, 1, C.byref(out) if with_out else None)
        assert rc == -1
        assert bytes(out) == before

    good = plan()
    assert lib.rama_pipe_tick_plan(C.byref(good), 2, 1, 1, C.byref(rama_pipe_tick())) == 0      # the arguments the refusals vary
    refused(None, 2, 1)                                  # NULL plan
    refused(good, 2, 1, with_out=False)                  # NULL out
    refused(good, 0, 0)                                  # world < 1
    refused(good, -1, 0)
    refused(good, 2, -1)                                 # rank outside the world
    refused(good, 2, 2)
    refused(plan(n_seq=0), 2, 1)                         # n_seq < 1
    refused(plan(n_pos=0), 2, 1)                         # n_pos < 1
    refused(plan(n_prompt=-1), 2, 1)                     # n_prompt < 0
    refused(plan(pr=None, n_prompt=2), 2, 1)             # a prompt length without a prompt
    assert lib.rama_pipe_plan_ticks(None, 2) == -1
    assert lib.rama_pipe_plan_ticks(C.byref(good), 0) == -1
    assert lib.rama_pipe_plan_ticks(C.byref(plan(n_seq=0)), 2) == -1
    assert lib.rama_pipe_plan_ticks(C.byref(plan(n_pos=0)), 2) == -1
    assert lib.rama_pipe_plan_ticks(C.byref(good), 2) == 2 * 3 + 1
