"""The native pipeline tick plan (csrc/pipe.hip rama_pipe_tick_plan), shared by its tests (no test, no GPU): the ctypes call, the
executor of one tick's compute half, the 675-case grid and the reference history.

rama_pipe_run_ticks is a loop over rama_pipe_tick_plan: per tick it runs the stage pass the plan names (rama_forward_stage for BOS
and forced tokens, rama_forward_stage_devtok for the device token word), samples when the plan says so, then posts the exchange
legs the plan names.  `execute_tick` does the compute half of exactly that for any backend with compute() and sample(), and hands
the legs back, so a caller moves the bytes its own way: tests/test_pipeline_gloo.py with one batch_isend_irecv per tick between real
ranks, tests/test_hip_pipe_stages.py through the host between N contexts on one GPU.  The plan is the only source of decisions here:
nothing in this module knows rama_amd.pipeline.Schedule.

A backend is one rank's stage:
    backend.rank                          the rank it stands for
    backend.compute(seq, pos, token)      the stage pass of sequence `seq` at (wrapped) position `pos`; token is an int (BOS or a forced
                                          prompt token) or None = the sequence's token word on rank 0, no token at all on other ranks
    backend.sample(seq)                   Device::sample of the sequence's logits into its token word

The reference history (`reference`) is generate() of the whole model in one process, the loop tests/test_hip_pipe_native.py uses:
token 1 at position 0; forward; nxt = sample(logits); nxt is recorded for EVERY position; the next token is prompt[pos] while forced,
else nxt.  wrap > 0: every `wrap` positions the sequence starts over at position 0 with BOS and the prompt; the history stays indexed
by the unwrapped position.  All sequences of a plan share the prompt, so they share the history."""
import ctypes as C
import itertools
from collections import namedtuple

import numpy as np

NONE, X, TOKEN = 0, 1, 2                 # RAMA_PIPE_NONE / RAMA_PIPE_X / RAMA_PIPE_TOKEN (include/rama_hip.h)
TOKEN_BOS, TOKEN_FORCED, TOKEN_WORD = 0, 1, 2
BOS = 1
U_CONST = 0.2721174359321594             # the reference's constant draw (cpu.rs:161-162, tests/test_sampler_const.py)

# the host tests' grid: world x n_seq x n_pos x wrap x n_prompt
GRID = list(itertools.product((1, 2, 3, 4, 8), (1, 2, 3, 5, 8), (1, 2, 5), (0, 2, 3), (0, 1, 4)))
GRID_PROMPT = (11, 12, 13, 14)           # none of them BOS, all different


def make_plan(n_seq, n_pos, wrap=0, prompt=(), temperature=0.0, topp=0.9, u=0.0, out=None):
    """-> rama_pipe_plan (ctypes keeps the prompt array alive with the structure that points to it)"""
    from rama_amd._lib import rama_pipe_plan
    arr = (C.c_int32 * len(prompt))(*prompt) if len(prompt) else None
    return rama_pipe_plan(n_seq, n_pos, wrap, arr, len(prompt), temperature, topp, u, out)


def tick(lib, plan, world, rank, t):
    """rama_pipe_tick_plan(plan, world, rank, t) -> rama_pipe_tick"""
    from rama_amd._lib import rama_pipe_tick
    out = rama_pipe_tick()
    rc = lib.rama_pipe_tick_plan(C.byref(plan), world, rank, t, C.byref(out))
    assert rc == 0, ("rama_pipe_tick_plan", rc, world, rank, t)
    return out


def plan_ticks(lib, plan, world):
    n = lib.rama_pipe_plan_ticks(C.byref(plan), world)
    assert n > 0, ("rama_pipe_plan_ticks", n, world)
    return n


def execute_tick(t, rank, backend):
    """the compute half of one tick of rama_pipe_run_ticks, as the plan `t` of `rank` has it.
    -> (send, recv): send = (kind, seq, peer) or None, recv = (kind, seq, peer, recv_pos) or None"""
    assert backend.rank == rank
    if t.on:
        backend.compute(t.seq, t.pos_wrapped, None if t.token_kind == TOKEN_WORD else t.token)
        if t.samples:
            backend.sample(t.seq)
    send = (t.send_kind, t.send_seq, t.send_peer) if t.send_kind != NONE else None
    recv = (t.recv_kind, t.recv_seq, t.recv_peer, t.recv_pos) if t.recv_kind != NONE else None
    return send, recv


Reference = namedtuple("Reference", "history gaps oracle")


def reference(cfg, w, prompt, n_pos, wrap=0, temperature=0.0, topp=0.9, u=0.0):
    """-> Reference: history[pos] = the id sampled after unwrapped position pos; gaps[pos] = the logits' top-two gap there; the
    oracle itself, as the last position left it (its logits and its key / value cache rows are what a stage must hold at the end)"""
    from oracle import oracle as O
    orc = O.Oracle(cfg, w)
    history, gaps = [], []
    token = BOS
    for pos in range(n_pos):
        pw = pos % wrap if wrap else pos
        if pw == 0:
            token = BOS
        lo = orc.forward(token, pw)
        top = np.sort(lo)[-2:]
        gaps.append(float(top[1]) - float(top[0]))
        nxt = int(O.sample(lo.copy(), temperature, topp, u))
        history.append(nxt)
        token = prompt[pw] if pw < len(prompt) else nxt
    return Reference(history, gaps, orc)
