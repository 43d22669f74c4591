"""The Q8 host layer's own rules, on the host alone (no GPU): every refusal rama_amd.q8 writes in Python with its exception type
and full text (the texts are those of the commit before the checks were shared: the table passes on that q8.py too), the ring
drain against a scripted poll, and the restated accept rule against rama_q8_spec_accept over a whole small case set."""
import itertools
from types import SimpleNamespace

import pytest

from tests.test_q8_chain_host import fake_engines

V, S = 64, 32
CFG = SimpleNamespace(vocab_size=V, seq_len=S)
BIG = SimpleNamespace(vocab_size=40000, seq_len=S)            # beyond the sampled plans' 32768
NAN = float("nan")
SAMPLER = "temperature >= 0, topp in [0, 1], u in [0, 1) -- not "


def _q8():
    from rama_amd import q8
    return q8


# ------------------------------------------------------------------ the refusals

def batch(fn, engines=None, tokens=(1, 2, 3), positions=(0, 1, 2)):
    return lambda q8: getattr(q8, fn)(E if engines is None else engines, list(tokens), list(positions))


def chain(engines=None, tokens=(1, 2, 3), positions=(0, 1, 2), n_steps=4, **kw):
    kw = {**dict(temperature=0.0, topp=0.9, u=0.5), **kw}
    return lambda q8: q8.chain_plan(E if engines is None else engines, list(tokens), list(positions), n_steps, **kw)


def serve(context=(1, 2, 3), max_new=5, T=0.0, P=0.9, U=0.5, stop=None, cap=None, n_cached=0, cfg=CFG):
    return lambda q8: q8.serve_plan(cfg, list(context), max_new, T, P, U, stop, cap, n_cached)


def spec(context=(1, 2, 3), max_new=5, T=0.0, P=0.9, U=0.5, stop=None, n_draft=7, ngram=3, hint=None, cfg=CFG):
    return lambda q8: q8.spec_plan(cfg, list(context), max_new, T, P, U, stop, n_draft, ngram, hint)


def pool_put_twice(q8):
    p, e = q8.PrefixPool(2), object()
    p.put([1, 2], e)
    p.put([1, 2, 3], e)


E = fake_engines(3, vocab_size=V, seq_len=S)
OTHER = fake_engines(1, vocab_size=V, seq_len=S)[0]           # an engine of another model
MANY = fake_engines(129, vocab_size=V, seq_len=S)


def batch_refusals(what, run):
    """the four refusals decode_batch and chain_plan share, and their order"""
    return [
        (run([], [], []), f"{what}: 0 sequences, not 1..128"),
        (run(MANY, [1] * 129, [0] * 129), f"{what}: 129 sequences, not 1..128"),
        (run(None, [1, 2]), f"{what}: 2 tokens and 3 positions for 3 sequences"),
        (run(None, [1, 2, 3], [0, 1]), f"{what}: 3 tokens and 2 positions for 3 sequences"),
        (run([E[0], OTHER], [1, 2], [0, 0]), f"{what}: the engines do not share one Q8Model"),
        (run([E[0], E[1], E[0]]), f"{what}: an engine appears twice"),
        # two faults: the count before the lengths, the lengths before the model, the model before the repeated engine
        (run(MANY, [1], [0]), f"{what}: 129 sequences, not 1..128"),
        (run([E[0], OTHER], [1], [0, 0]), f"{what}: 1 tokens and 2 positions for 2 sequences"),
        (run([E[0], OTHER, E[0]]), f"{what}: the engines do not share one Q8Model"),
    ]


REFUSALS = (
    batch_refusals("decode_batch", lambda *a: batch("decode_batch", *a)) + [
        (batch("decode_batch", None, [1, V, 3]), "decode_batch: token 64 outside the vocabulary [0, 64)"),
        (batch("decode_batch", None, [1, 2, -1]), "decode_batch: token -1 outside the vocabulary [0, 64)"),
        (batch("decode_batch", None, [1, 2, 3], [0, S, 0]), "decode_batch: position 32 outside [0, 32)"),
        (batch("decode_batch", None, [1, 2, 3], [0, 0, -1]), "decode_batch: position -1 outside [0, 32)"),
        (batch("decode_batch", [E[0], E[0]], [V, 2], [0, 0]), "decode_batch: an engine appears twice"),          # two faults
        (batch("decode_batch", None, [1, V, 3], [-1, 0, 0]), "decode_batch: token 64 outside the vocabulary [0, 64)"),
    ] +
    # ---- chain_plan (and _per_seq through it)
    batch_refusals("decode_batch_chained", lambda *a: chain(*a)) + [
        (chain(n_steps=0), "decode_batch_chained: n_steps 0 < 1"),
        (chain(tokens=[1, V, 3]), "decode_batch_chained: token 64 outside the vocabulary [0, 64)"),
        (chain(temperature=[0.0, 1.0]), "decode_batch_chained: 2 temperature values for 3 sequences"),
        (chain(topp=[0.9] * 4), "decode_batch_chained: 4 topp values for 3 sequences"),
        (chain(u=[0.1]), "decode_batch_chained: 1 u values for 3 sequences"),
        (chain(max_new=[1, 2]), "decode_batch_chained: 2 max_new values for 3 sequences"),
        (chain(stop_tokens=[1, 2, 3, 4]), "decode_batch_chained: 4 stop_tokens values for 3 sequences"),
        (chain(prompts=[[1, 2], [3, V], []]), "decode_batch_chained prompt: token 64 outside the vocabulary [0, 64)"),
        (chain(prompts=[[1], [2]]), "decode_batch_chained: 2 prompts for 3 sequences"),
        (chain(temperature=[0.0, NAN, 0.0]), "decode_batch_chained: sequence 1: " + SAMPLER + "nan, 0.9, 0.5"),
        (chain(topp=[0.9, 0.9, NAN]), "decode_batch_chained: sequence 2: " + SAMPLER + "0.0, nan, 0.5"),
        (chain(u=NAN), "decode_batch_chained: sequence 0: " + SAMPLER + "0.0, 0.9, nan"),
        (chain(temperature=-0.5), "decode_batch_chained: sequence 0: " + SAMPLER + "-0.5, 0.9, 0.5"),
        (chain(topp=1.5), "decode_batch_chained: sequence 0: " + SAMPLER + "0.0, 1.5, 0.5"),
        (chain(topp=-0.1), "decode_batch_chained: sequence 0: " + SAMPLER + "0.0, -0.1, 0.5"),
        (chain(u=[0.0, 0.5, 1.0]), "decode_batch_chained: sequence 2: " + SAMPLER + "0.0, 0.9, 1.0"),
        (chain(u=-0.25), "decode_batch_chained: sequence 0: " + SAMPLER + "0.0, 0.9, -0.25"),
        (chain(max_new=[0, -1, 0]), "decode_batch_chained: sequence 1: max_new -1 < 0"),
        (chain(stop_tokens=[None, V, None]), "decode_batch_chained: sequence 1: stop token 64 outside the vocabulary [0, 64)"),
        (chain(stop_tokens=-2), "decode_batch_chained: sequence 0: stop token -2 outside the vocabulary [0, 64)"),
        (chain(positions=[0, S - 3, 0]), "decode_batch_chained: sequence 1: position 29 + 4 steps outside [0, 32]"),
        (chain(positions=[0, -1, 0]), "decode_batch_chained: sequence 1: position -1 + 4 steps outside [0, 32]"),
        (chain(positions=[0, S - 2, 0], max_new=[None, 3, None]), "decode_batch_chained: sequence 1: position 30 + 3 steps outside [0, 32]"),
        (chain(positions=[0, S, 0], max_new=1), "decode_batch_chained: sequence 1: position 32 + 1 steps outside [0, 32]"),
        # two faults: n_steps before the tokens, the tokens before a count, sequence 0 before sequence 1, and within a sequence
        # the sampler, max_new, the stop token, the position
        (chain(n_steps=0, tokens=[V, 2, 3]), "decode_batch_chained: n_steps 0 < 1"),
        (chain(tokens=[V, 2, 3], u=[0.1]), "decode_batch_chained: token 64 outside the vocabulary [0, 64)"),
        (chain(u=[0.1], prompts=[[V], [], []]), "decode_batch_chained: 1 u values for 3 sequences"),
        (chain(temperature=[0.0, -1.0, 0.0], stop_tokens=[V, None, None]), "decode_batch_chained: sequence 0: stop token 64 outside the vocabulary [0, 64)"),
        (chain(temperature=-1.0, max_new=-1), "decode_batch_chained: sequence 0: " + SAMPLER + "-1.0, 0.9, 0.5"),
        (chain(max_new=-1, stop_tokens=V), "decode_batch_chained: sequence 0: max_new -1 < 0"),
        (chain(stop_tokens=V, positions=[S, 0, 0]), "decode_batch_chained: sequence 0: stop token 64 outside the vocabulary [0, 64)"),
    ] +
    # ---- serve_sizes
    [
        (lambda q8: q8.serve_sizes(CFG, 0, None, 8), "Q8Server: 0 slots, not 1..128"),
        (lambda q8: q8.serve_sizes(CFG, 129, None, 8), "Q8Server: 129 slots, not 1..128"),
        (lambda q8: q8.serve_sizes(CFG, 4, 3, 8), "Q8Server: max_rows 3 outside [n_slots = 4, 128]"),
        (lambda q8: q8.serve_sizes(CFG, 4, 129, 8), "Q8Server: max_rows 129 outside [n_slots = 4, 128]"),
        (lambda q8: q8.serve_sizes(CFG, 4, 8, 0), "Q8Server: max_new_cap 0 outside [1, seq_len - 1 = 31]"),
        (lambda q8: q8.serve_sizes(CFG, 4, 8, S), "Q8Server: max_new_cap 32 outside [1, seq_len - 1 = 31]"),
        (lambda q8: q8.serve_sizes(CFG, 0, 0, 0), "Q8Server: 0 slots, not 1..128"),                              # two faults
        (lambda q8: q8.serve_sizes(CFG, 4, 3, 0), "Q8Server: max_rows 3 outside [n_slots = 4, 128]"),
    ] +
    # ---- serve_plan
    [
        (serve(context=[1, V]), "Q8Server.submit: token 64 outside the vocabulary [0, 64)"),
        (serve(context=[]), "Q8Server.submit: an empty context (the caller includes BOS)"),
        (serve(n_cached=3), "Q8Server.submit: n_cached 3 outside [0, n_context - 1 = 2] (the final context position is always fed)"),
        (serve(n_cached=-1), "Q8Server.submit: n_cached -1 outside [0, n_context - 1 = 2] (the final context position is always fed)"),
        (serve(T=NAN), "Q8Server.submit: " + SAMPLER + "nan, 0.9, 0.5"),
        (serve(P=NAN), "Q8Server.submit: " + SAMPLER + "0.0, nan, 0.5"),
        (serve(U=NAN), "Q8Server.submit: " + SAMPLER + "0.0, 0.9, nan"),
        (serve(T=-1.0), "Q8Server.submit: " + SAMPLER + "-1.0, 0.9, 0.5"),
        (serve(P=1.5), "Q8Server.submit: " + SAMPLER + "0.0, 1.5, 0.5"),
        (serve(U=1.0), "Q8Server.submit: " + SAMPLER + "0.0, 0.9, 1.0"),
        (serve(max_new=0), "Q8Server.submit: max_new 0 < 1"),
        (serve(max_new=9, cap=8), "Q8Server.submit: max_new 9 beyond the server's max_new_cap 8"),
        (serve(max_new=S - 3 + 1), "Q8Server.submit: 3 context tokens + 30 new ones beyond seq_len 32"),
        (serve(stop=V), "Q8Server.submit: stop token 64 outside the vocabulary [0, 64)"),
        (serve(stop=-2), "Q8Server.submit: stop token -2 outside the vocabulary [0, 64)"),
        (serve(T=1.0, cfg=BIG), "Q8Server.submit: a sampled plan needs vocab_size <= 32768"),
        # two faults, in the order the refusals stand: context, n_cached, sampler, max_new, its cap, seq_len, stop token, vocabulary
        (serve(context=[], T=NAN), "Q8Server.submit: an empty context (the caller includes BOS)"),
        (serve(n_cached=3, T=-1.0), "Q8Server.submit: n_cached 3 outside [0, n_context - 1 = 2] (the final context position is always fed)"),
        (serve(U=1.0, max_new=0), "Q8Server.submit: " + SAMPLER + "0.0, 0.9, 1.0"),
        (serve(max_new=0, stop=V), "Q8Server.submit: max_new 0 < 1"),
        (serve(max_new=30, cap=8), "Q8Server.submit: max_new 30 beyond the server's max_new_cap 8"),
        (serve(max_new=30, stop=V), "Q8Server.submit: 3 context tokens + 30 new ones beyond seq_len 32"),
        (serve(T=1.0, stop=40000, cfg=BIG), "Q8Server.submit: stop token 40000 outside the vocabulary [0, 40000)"),
    ] +
    # ---- serve_spec_sizes, serve_spec_request
    [
        (lambda q8: q8.serve_spec_sizes(16, 3, 0), "Q8Server: n_draft 16 outside [0, 15]"),
        (lambda q8: q8.serve_spec_sizes(-1, 3, 0), "Q8Server: n_draft -1 outside [0, 15]"),
        (lambda q8: q8.serve_spec_sizes(7, 0, 0), "Q8Server: ngram 0 outside [1, 4]"),
        (lambda q8: q8.serve_spec_sizes(7, 5, 0), "Q8Server: ngram 5 outside [1, 4]"),
        (lambda q8: q8.serve_spec_sizes(7, 3, -1), "Q8Server: hint_cap -1 (>= 0, and 0 on a server without drafts)"),
        (lambda q8: q8.serve_spec_sizes(0, 3, 5), "Q8Server: hint_cap 5 (>= 0, and 0 on a server without drafts)"),
        (lambda q8: q8.serve_spec_sizes(16, 0, -1), "Q8Server: n_draft 16 outside [0, 15]"),                       # two faults
        (lambda q8: q8.serve_spec_sizes(7, 0, -1), "Q8Server: ngram 0 outside [1, 4]"),
        (lambda q8: q8.serve_spec_request(CFG, 7, 3, 4, n_draft=8), "Q8Server.submit: n_draft 8 outside [0, the server's n_draft = 7]"),
        (lambda q8: q8.serve_spec_request(CFG, 7, 3, 4, n_draft=-1), "Q8Server.submit: n_draft -1 outside [0, the server's n_draft = 7]"),
        (lambda q8: q8.serve_spec_request(CFG, 7, 3, 4, hint=[1, V]), "Q8Server.submit hint: token 64 outside the vocabulary [0, 64)"),
        (lambda q8: q8.serve_spec_request(CFG, 7, 3, 4, hint=[1] * 5), "Q8Server.submit: 5 hint tokens beyond the server's hint_cap 4"),
        (lambda q8: q8.serve_spec_request(CFG, 7, 3, 4, n_draft=8, hint=[V]), "Q8Server.submit: n_draft 8 outside [0, the server's n_draft = 7]"),
        (lambda q8: q8.serve_spec_request(CFG, 7, 3, 4, hint=[V] * 5), "Q8Server.submit hint: token 64 outside the vocabulary [0, 64)"),
    ] +
    # ---- spec_plan
    [
        (spec(context=[1, V]), "generate_spec: token 64 outside the vocabulary [0, 64)"),
        (spec(context=[]), "generate_spec: an empty context (the caller includes BOS)"),
        (spec(hint=[2, -1]), "generate_spec hint: token -1 outside the vocabulary [0, 64)"),
        (spec(T=NAN), "generate_spec: " + SAMPLER + "nan, 0.9, 0.5"),
        (spec(P=NAN), "generate_spec: " + SAMPLER + "0.0, nan, 0.5"),
        (spec(U=NAN), "generate_spec: " + SAMPLER + "0.0, 0.9, nan"),
        (spec(T=-1.0), "generate_spec: " + SAMPLER + "-1.0, 0.9, 0.5"),
        (spec(P=1.5), "generate_spec: " + SAMPLER + "0.0, 1.5, 0.5"),
        (spec(U=1.0), "generate_spec: " + SAMPLER + "0.0, 0.9, 1.0"),
        (spec(max_new=0), "generate_spec: max_new 0 < 1"),
        (spec(max_new=S - 3 + 1), "generate_spec: 3 context tokens + 30 new ones beyond seq_len 32"),
        (spec(n_draft=16), "generate_spec: n_draft 16 outside [0, 15]"),
        (spec(n_draft=-1), "generate_spec: n_draft -1 outside [0, 15]"),
        (spec(ngram=0), "generate_spec: ngram 0 outside [1, 4]"),
        (spec(ngram=5), "generate_spec: ngram 5 outside [1, 4]"),
        (spec(stop=V), "generate_spec: stop token 64 outside the vocabulary [0, 64)"),
        (spec(stop=-2), "generate_spec: stop token -2 outside the vocabulary [0, 64)"),
        (spec(T=1.0, cfg=BIG), "generate_spec: a sampled plan needs vocab_size <= 32768"),
        # two faults: context, hint, sampler, max_new, seq_len, n_draft, ngram, stop token, vocabulary
        (spec(context=[], hint=[V]), "generate_spec: an empty context (the caller includes BOS)"),
        (spec(hint=[V], T=NAN), "generate_spec hint: token 64 outside the vocabulary [0, 64)"),
        (spec(T=NAN, max_new=0), "generate_spec: " + SAMPLER + "nan, 0.9, 0.5"),
        (spec(max_new=30, n_draft=16), "generate_spec: 3 context tokens + 30 new ones beyond seq_len 32"),
        (spec(n_draft=16, ngram=0), "generate_spec: n_draft 16 outside [0, 15]"),
        (spec(ngram=0, stop=V), "generate_spec: ngram 0 outside [1, 4]"),
        (spec(T=1.0, stop=40000, cfg=BIG), "generate_spec: stop token 40000 outside the vocabulary [0, 40000)"),
    ] +
    # ---- the pure host functions and the pool
    [
        (lambda q8: q8.serve_spec_plan_step([(0, 0, 0, 0, 0)] * 2, [0], 4), "serve_spec_plan_step: 1 want values for 2 slots"),
        (lambda q8: q8.spec_accept([1], [1], None, 3), "spec_accept: 1 picks for 1 drafts, not one more"),
        (lambda q8: q8.spec_accept([], [1, 2], None, 3), "spec_accept: 2 picks for 0 drafts, not one more"),
        (lambda q8: q8.spec_replay([5, 6, 7, 8, 9], [1, 2], None, 7, 3, 12, None), "spec_replay: 5 reference tokens for max_new 12"),
        (lambda q8: q8.serve_spec_replay([dict(context=[1, 2], max_new=4)], [[5, 6, 7]], 2, 4), "serve_spec_replay: 3 reference tokens for max_new 4"),
        (lambda q8: q8.serve_spec_replay([dict(context=[1, 2], max_new=2)], [[5, 6]], 2, 4, use_slots=[]),
         "serve_spec_replay: requests are waiting but no slot can take them"),
        (lambda q8: q8.PrefixPool(-1), "PrefixPool: -1 donors"),
        (pool_put_twice, "PrefixPool.put: the engine is already a donor"),
    ])


def test_every_python_refusal_has_its_type_and_text():
    q8 = _q8()
    for i, (call, text) in enumerate(REFUSALS):
        with pytest.raises(ValueError) as info:
            call(q8)
        assert type(info.value) is ValueError and str(info.value) == text, (i, text)


def test_boundary_values_are_accepted():
    """the last value inside every range of the table above"""
    q8 = _q8()
    assert serve(U=0.0, P=1.0, stop=-1)(q8) == ([1, 2, 3], (0.0, 1.0, 0.0, 5, -1))
    assert serve(P=0.0, stop=V - 1, n_cached=2)(q8) == ([1, 2, 3], (0.0, 0.0, 0.5, 5, V - 1))
    assert serve(max_new=S - 3, T=1.0)(q8)[1] == (1.0, 0.9, 0.5, S - 3, -1)                     # n_context + max_new == seq_len
    assert serve(max_new=8, cap=8)(q8)[1][3] == 8
    assert serve(T=0.0, cfg=BIG)(q8)[1][0] == 0.0                                                # greedy: any vocabulary
    assert spec(U=0.0, P=1.0, stop=-1, n_draft=0, ngram=1)(q8) == ([1, 2, 3], [], (0.0, 1.0, 0.0, 5, -1, 0, 1))
    assert spec(max_new=S - 3, n_draft=15, ngram=4, stop=V - 1, hint=[V - 1])(q8) == ([1, 2, 3], [V - 1], (0.0, 0.9, 0.5, S - 3, V - 1, 15, 4))
    assert spec(T=0.0, cfg=BIG)(q8)[2][0] == 0.0
    # the chained batch: no budget of its own (0 or None), no cap on a sampled vocabulary, a budget that ends exactly at seq_len
    toks, poss, plan = chain(positions=[S - 4, S - 2, S - 1], temperature=[0.0, 1.0, 0.7], topp=[1.0, 0.0, 0.5], u=[0.0, 0.25, 0.5],
                             max_new=[None, 2, 1], stop_tokens=[None, -1, V - 1])(q8)
    assert (toks, poss) == ([1, 2, 3], [S - 4, S - 2, S - 1])
    assert plan == [(0.0, 1.0, 0.0, [], 0, -1), (1.0, 0.0, 0.25, [], 2, -1), (0.7, 0.5, 0.5, [], 1, V - 1)]
    big = fake_engines(2, vocab_size=40000, seq_len=S)
    assert chain(big, [1, 2], [0, 0], temperature=1.0, max_new=0)(q8)[2] == [(1.0, 0.9, 0.5, [], 0, -1)] * 2
    assert q8.serve_sizes(CFG, 4, None, S - 1) == (4, 4, S - 1) and q8.serve_sizes(CFG, 128, 128, 1) == (128, 128, 1)
    assert q8.serve_spec_sizes(0, 1, 0) == (0, 1, 0) and q8.serve_spec_sizes(15, 4, 100) == (15, 4, 100)
    assert q8.serve_spec_request(CFG, 7, 3, 4) == (7, 3, [])
    assert q8.serve_spec_request(CFG, 7, 3, 4, n_draft=0, hint=[1, 2, 3, V - 1]) == (0, 3, [1, 2, 3, V - 1])
    assert q8.serve_spec_request(CFG, 7, 9, 4, n_draft=7) == (7, 9, [])                          # (the server's ngram is passed through)


# ------------------------------------------------------------------ the ring drain

class Ring:
    """a ring as the poll entries show it: the tokens from `start` on, 64 at most, and the finished word; `then`, when given, is
    run after a poll has been answered (what the device does between two polls)"""

    def __init__(self, tokens, finished, then=None):
        self.tokens, self.finished, self.then, self.polls = list(tokens), finished, then, []

    def __call__(self, start):
        fin = int(self.finished)                      # (the finished word is read before the ring)
        out = self.tokens[start:start + 64]
        self.polls.append((start, len(out), fin))
        if self.then is not None:
            self.then(self)
        return out, fin


def drain(ring, seen=0):
    from rama_amd.q8 import _drain
    got = []
    n, fin = _drain(ring, seen, lambda i, t: got.append((i, t)))
    assert isinstance(fin, bool)
    return n, fin, got


def text(n):
    return [1000 + i for i in range(n)]


def test_drain_against_a_scripted_poll():
    # nothing there, not finished
    r = Ring([], False)
    assert drain(r) == (0, False, []) and r.polls == [(0, 0, 0)]
    # a short poll with the word set: finished
    r = Ring(text(63), True)
    assert drain(r) == (63, True, list(enumerate(text(63)))) and r.polls == [(0, 63, 1)]
    r = Ring(text(63), False)
    assert drain(r) == (63, False, list(enumerate(text(63)))) and r.polls == [(0, 63, 0)]
    # exactly 64 with the word already set: the full poll does not finish the sequence, the next one -- no tokens, the word set -- does
    r = Ring(text(64), True)
    assert drain(r) == (64, True, list(enumerate(text(64)))) and r.polls == [(0, 64, 1), (64, 0, 1)]
    r = Ring(text(64), False)
    assert drain(r) == (64, False, list(enumerate(text(64)))) and r.polls == [(0, 64, 0), (64, 0, 0)]
    # one and two full polls and a remainder
    r = Ring(text(65), True)
    assert drain(r) == (65, True, list(enumerate(text(65)))) and r.polls == [(0, 64, 1), (64, 1, 1)]
    r = Ring(text(129), True)
    assert drain(r) == (129, True, list(enumerate(text(129)))) and r.polls == [(0, 64, 1), (64, 64, 1), (128, 1, 1)]
    r = Ring(text(129), False)
    assert drain(r) == (129, False, list(enumerate(text(129)))) and r.polls == [(0, 64, 0), (64, 64, 0), (128, 1, 0)]
    # from a count already seen: the sink's indices go on from it, and a later drain takes what came since
    r = Ring(text(80), False)
    assert drain(r, 10) == (70, False, list(enumerate(text(80)))[10:]) and r.polls == [(10, 64, 0), (74, 6, 0)]
    r.tokens += [7, 8]
    r.finished = True
    assert drain(r, 80) == (2, True, [(80, 7), (81, 8)]) and r.polls[2:] == [(80, 2, 1)]
    assert drain(r, 82) == (0, True, [])


def test_drain_when_the_finished_word_is_set_between_two_polls():
    def finish(ring):
        ring.finished = True
    # the first poll of the drain sees 64 of 70 tokens and no word; the word is set before the second
    r = Ring(text(70), False, then=finish)
    assert drain(r) == (70, True, list(enumerate(text(70)))) and r.polls == [(0, 64, 0), (64, 6, 1)]

    # ... and with the last tokens written between the two polls as well
    def emit_and_finish(ring):
        if not ring.finished:
            ring.tokens += [5, 6, 7]
            ring.finished = True
    r = Ring(text(64), False, then=emit_and_finish)
    assert drain(r) == (67, True, list(enumerate(text(64) + [5, 6, 7]))) and r.polls == [(0, 64, 0), (64, 3, 1)]
    # a short poll without the word ends the drain unfinished even if the word is set right behind it: the next drain sees it
    r = Ring(text(3), False, then=finish)
    assert drain(r) == (3, False, list(enumerate(text(3)))) and r.polls == [(0, 3, 0)]
    assert drain(r, 3) == (0, True, [])


# ------------------------------------------------------------------ the accept rule

def check_accept(drafts, picks, remaining, stop):
    from rama_amd.q8 import spec_accept
    from rama_amd.q8_replay import _accept_py
    a, emitted, fin = _accept_py(list(drafts), list(picks), remaining, -1 if stop is None else stop)
    assert (emitted, fin) == spec_accept(drafts, picks, stop, remaining), (drafts, picks, remaining, stop)
    assert 0 <= a <= len(drafts) and list(picks[:a]) == list(drafts[:a]) and (a == len(drafts) or picks[a] != drafts[a])
    assert 1 <= emitted <= min(a + 1, remaining)


def test_accept_rule_equals_the_library_on_every_small_case():
    """0..3 drafts, 1..4 tokens remaining, drafts, picks and the stop token over a 3-token vocabulary (and no stop token)"""
    n = 0
    for n_d in range(4):
        for drafts in itertools.product(range(3), repeat=n_d):
            for picks in itertools.product(range(3), repeat=n_d + 1):
                for remaining in range(1, 5):
                    for stop in (None, 0, 1, 2):
                        check_accept(drafts, picks, remaining, stop)
                        n += 1
    assert n == sum(3 ** d * 3 ** (d + 1) for d in range(4)) * 4 * 4


def test_accept_rule_equals_the_library_at_15_drafts():
    drafts = [i % 3 for i in range(15)]
    for a in range(16):                               # the first a drafts are right (all of them at a == 15)
        picks = drafts[:a] + [(drafts[a] + 1) % 3 if a < 15 else 2] + [0] * (15 - a)
        for remaining in (1, 2, a, a + 1, a + 2, 15, 16, 17):
            for stop in (None, 0, 1, 2):
                if remaining >= 1:
                    check_accept(drafts, picks, remaining, stop)
