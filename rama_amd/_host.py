"""What the host layers of both stacks share (engine.py, q8.py, serve.py): the marshalling into the C ABI's arrays and tables, the refusals
the entry points word alike, the drain of a host-visible ring and the wait on the stream behind it.  No model, no engine, no serving loop."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from ._lib import check, rama_q8_serve_slot

MAX_BATCH = 128
MAX_DRAFT, MAX_NGRAM = 15, 4


# ------------------------------------------------------------------ marshalling

def _i32(values):
    """a c_int32 array of the values; one unused entry for none, so that the library always gets a pointer"""
    return (C.c_int32 * max(len(values), 1))(*values)


def _slot_table(slots):
    """(state, n_context, cursor, n_out, max_new) tuples -> rama_q8_serve_slot[]"""
    return (rama_q8_serve_slot * max(len(slots), 1))(*[rama_q8_serve_slot(*[int(v) for v in s]) for s in slots])


def _row_table(rows, n):
    """rama_q8_serve_row[] -> n (slot, pos, logits) tuples"""
    return [(r.slot, r.pos, r.logits) for r in rows[:n]]


def _report(r, skip=()):
    """a report struct as a dict of its fields: a counter as an int, an array as a list"""
    out = {}
    for name, _ in r._fields_:
        if name not in skip:
            v = getattr(r, name)
            out[name] = v if isinstance(v, int) else list(v)
    return out


def _per_seq(v, n: int, counted: str) -> list:
    """a scalar (or None) for every sequence, or one value per sequence; `counted` is the caller's wording of a wrong count, with {} for
    the count: "temperature: {} values", "decode_batch_chained: {} topp values" """
    if v is None or np.ndim(v) == 0:
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f"{counted.format(len(v))} for {n} sequences")
    return v


# ------------------------------------------------------------------ the refusals the entry points share (as check_* in q8_host.hpp / q8_api.hip:
# each takes the caller's prefix and, where two callers word a cap differently, that text)

def _tokens(tokens, vocab_size: int, what: str) -> list:
    out = [int(t) for t in tokens]
    bad = [t for t in out if not 0 <= t < vocab_size]
    if bad:
        raise ValueError(f"{what}: token {bad[0]} outside the vocabulary [0, {vocab_size})")
    return out


def _check_batch(what, engines, tokens, positions):
    """1..128 distinct engines over one Q8Model, a token and a position for each"""
    n = len(engines)
    if not 1 <= n <= MAX_BATCH:
        raise ValueError(f"{what}: {n} sequences, not 1..{MAX_BATCH}")
    if len(tokens) != n or len(positions) != n:
        raise ValueError(f"{what}: {len(tokens)} tokens and {len(positions)} positions for {n} sequences")
    if any(e.model is not engines[0].model for e in engines):
        raise ValueError(f"{what}: the engines do not share one Q8Model")
    if len({id(e) for e in engines}) != n:
        raise ValueError(f"{what}: an engine appears twice")


def _check_sampler(what, temperature, topp, u):
    T, P, U = float(temperature), float(topp), float(u)
    if not (T >= 0.0 and 0.0 <= P <= 1.0 and 0.0 <= U < 1.0):       # (false for NaN)
        raise ValueError(f"{what}: temperature >= 0, topp in [0, 1], u in [0, 1) -- not {T}, {P}, {U}")
    return T, P, U


def _check_stop(what, stop_token, vocab_size):
    """None: no stop token, -1 to the library"""
    stop = -1 if stop_token is None else int(stop_token)
    if not -1 <= stop < vocab_size:
        raise ValueError(f"{what}: stop token {stop} outside the vocabulary [0, {vocab_size})")
    return stop


def _check_context(what, context, vocab_size):
    ctx = _tokens(context, vocab_size, what)
    if not ctx:
        raise ValueError(f"{what}: an empty context (the caller includes BOS)")
    return ctx


def _check_budget(what, n_context, new, seq_len, cap=None):
    """max_new >= 1, within the server's cap where there is one, and the context with it within seq_len"""
    if new < 1:
        raise ValueError(f"{what}: max_new {new} < 1")
    if cap is not None and new > int(cap):
        raise ValueError(f"{what}: max_new {new} beyond the server's max_new_cap {int(cap)}")
    if n_context + new > seq_len:
        raise ValueError(f"{what}: {n_context} context tokens + {new} new ones beyond seq_len {seq_len}")


def _check_n_draft(what, n_draft, cap, cap_text):
    if not 0 <= n_draft <= cap:
        raise ValueError(f"{what}: n_draft {n_draft} outside [0, {cap_text}]")


def _check_drafting(what, n_draft, ngram):
    """the drafting sizes against the library's own caps"""
    _check_n_draft(what, n_draft, MAX_DRAFT, MAX_DRAFT)
    if not 1 <= ngram <= MAX_NGRAM:
        raise ValueError(f"{what}: ngram {ngram} outside [1, {MAX_NGRAM}]")


def _check_sampled_vocab(what, temperature, vocab_size):
    if temperature != 0.0 and vocab_size > 32768:
        raise ValueError(f"{what}: a sampled plan needs vocab_size <= 32768")


# ------------------------------------------------------------------ the host-visible rings and the stream behind them

def _ring_poll(entry, name, *before, after=()):
    """one of the three poll entries, entry(*before, start, tokens, 64, &n, &finished, *after), as _drain's poll(start)"""
    buf, k, fin = (C.c_int32 * 64)(), C.c_int(), C.c_int()
    rest = (buf, 64, C.byref(k), C.byref(fin)) + tuple(after)

    def poll(start):
        check(entry(*before, start, *rest), name)
        return buf[:k.value], fin.value
    return poll


def _drain(poll, seen, sink):
    """empties a ring from its token `seen` on, 64 tokens at a time: poll(start) -> (the tokens from start on, 64 at most, the
    finished word), sink(index, token) for each of them -> (tokens taken, finished).  The poll entries read the finished word before
    the ring: once it is set every token of the sequence is there, and the sequence has finished when a poll with the word set
    comes back short -- a full one may have left tokens behind."""
    n = 0
    while True:
        toks, fin = poll(seen + n)
        for t in toks:
            sink(seen + n, t)
            n += 1
        if len(toks) < 64:
            return n, bool(fin)


def _stream_busy(device, sleep):
    """rama_stream_query: the stream still has work -> True after `sleep` seconds, and the caller looks at its rings again; it has
    drained -> False: one more look collects what is there.  A failed stream raises instead of being waited for."""
    q = device.lib.rama_stream_query(device.ctx)
    if q == 1:
        time.sleep(sleep)
        return True
    check(q, "rama_stream_query")
    return False
