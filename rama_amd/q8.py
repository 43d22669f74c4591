"""Q8_0 models over the C ABI: llama2.c version-2 checkpoints (rama_q8_model_load) and synthetic Q8 models
(rama_q8_model_synth), decoded by the Q8 forward (runq.c's quantized products, rama's exact ops elsewhere;
include/rama_hip.h).  The fp32 Model / Engine are untouched.  No CPU fallback anywhere."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from ._lib import (Q8_TENSORS, check, load, rama_config, rama_q8_seq_plan, rama_q8_serve_plan, rama_q8_serve_report, rama_q8_serve_row,
                   rama_q8_serve_slot, rama_q8_serve_spec, rama_q8_serve_spec_report, rama_q8_spec_plan, rama_q8_spec_report,
                   rama_q8_weights, rama_run_state)
from .q8_replay import (SERVE_DECODE, SERVE_DONE, SERVE_FREE, SERVE_PROMPT,  # noqa: F401  (the restatements: re-exported)
                        _accept_py, _draft_py, _spec_plan_py, serve_spec_replay, spec_replay)
from .sampler_const import TOPP_U_CPU
from .transformer import Config, Hip

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


# ------------------------------------------------------------------ the refusals the entry points share (as check_* in q8_api.hip:
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


class Q8Model:
    def __init__(self, device: Hip, handle):
        self.device, self.handle = device, handle
        c = rama_config()
        check(device.lib.rama_q8_model_config(handle, C.byref(c)))
        self.ccfg = c
        self.config = self.cfg = Config(c.dim, c.hidden_dim, c.n_layers, c.n_heads, c.n_kv_heads, c.vocab_size,
                                         c.seq_len, bool(c.shared_weight))
        self.weights = rama_q8_weights()
        check(device.lib.rama_q8_model_weights(handle, C.byref(self.weights)))
        self.group_size = int(self.weights.group_size)

    @staticmethod
    def load(device: Hip, path) -> "Q8Model":
        """llama2.c version-2 (Q8_0) .bin -> HBM"""
        h = C.c_void_p()
        check(device.lib.rama_q8_model_load(device.ctx, str(path).encode(), C.byref(h)), "rama_q8_model_load")
        return Q8Model(device, h)

    @staticmethod
    def synth(device: Hip, cfg: Config, group_size: int, seed: int) -> "Q8Model":
        """rama_model_synth's fp32 weights, quantized in HBM by export.py's quantize_q80 rule"""
        h = C.c_void_p()
        c = rama_config(cfg.dim, cfg.hidden_dim, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.vocab_size, cfg.seq_len, int(cfg.shared_weight))
        check(device.lib.rama_q8_model_synth(device.ctx, C.byref(c), group_size, seed, C.byref(h)), "rama_q8_model_synth")
        return Q8Model(device, h)

    @property
    def bytes(self) -> int:
        """bytes a decode step streams: int8 values, scales and fp32 norms"""
        return self.device.lib.rama_q8_model_bytes(self.handle)

    def _numel(self, name: str) -> int:
        c = self.cfg
        L, d, h, V, S, hs = c.n_layers, c.dim, c.hidden_dim, c.vocab_size, c.seq_len, c.head_size
        return dict(tok=V * d, wcls=V * d, wq=L * d * d, wk=L * d * d, wv=L * d * d, wo=L * d * d, w1=L * h * d, w2=L * d * h,
                    w3=L * h * d, token_embedding_table=V * d, rms_att_weight=L * d, rms_ffn_weight=L * d,
                    rms_final_weight=d, freq_cis_real=S * (hs // 2), freq_cis_imag=S * (hs // 2))[name]

    def tensor(self, name: str):
        """download a tensor: a quantized one (tok, wq, ..., wcls) as (int8 values, fp32 scales), an fp32 one as an array"""
        n = self._numel(name)
        L = self.device.lib
        if name in Q8_TENSORS:
            q = np.empty(n, dtype=np.int8)
            s = np.empty(n // self.group_size, dtype=np.float32)
            if n % 4:
                raise ValueError("tensor size not a multiple of 4 bytes")
            check(L.rama_download_f32(self.device.ctx, getattr(self.weights, name), n // 4, q.ctypes.data))
            check(L.rama_download_f32(self.device.ctx, getattr(self.weights, name + "_s"), s.size, s.ctypes.data))
            return q, s
        out = np.empty(n, dtype=np.float32)
        check(L.rama_download_f32(self.device.ctx, getattr(self.weights, name), n, out.ctypes.data))
        return out

    def free(self):
        if self.handle:
            check(self.device.lib.rama_q8_model_free(self.device.ctx, self.handle))
            self.handle = None


class Q8Engine:
    """Q8 model + run state + decode cursor on one device / stream"""

    def __init__(self, device: Hip, model: Q8Model):
        self.device, self.model, self.cfg = device, model, model.cfg
        self.state = rama_run_state()
        check(device.lib.rama_state_create(device.ctx, C.byref(model.ccfg), self.cfg.n_layers, C.byref(self.state)), "rama_state_create")

    def forward(self, token: int, pos: int):
        check(self.device.lib.rama_q8_forward(self.device.ctx, C.byref(self.model.ccfg), C.byref(self.model.weights),
                                              C.byref(self.state), token, pos), "rama_q8_forward")

    def buffer(self, name: str, n: int, offset: int = 0) -> np.ndarray:
        out = np.empty(n, dtype=np.float32)
        check(self.device.lib.rama_download_f32(self.device.ctx, getattr(self.state, name) + 4 * offset, n, out.ctypes.data))
        return out

    def set_buffer(self, name: str, data: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
        check(self.device.lib.rama_copy_h2d_f32(self.device.ctx, getattr(self.state, name) + 4 * offset, a.ctypes.data, a.size))

    def logits(self) -> np.ndarray:
        return self.buffer("logits", self.cfg.vocab_size)

    def prefill(self, tokens, pos0: int = 0):
        """the prompt positions pos0 .. pos0 + len(tokens) - 1 in shared weight passes (rama_q8_prefill): the caches, x and
        logits rama_q8_forward would leave after them"""
        toks = _tokens(tokens, self.cfg.vocab_size, "prefill")
        if not toks:
            raise ValueError("prefill: no tokens")
        pos0 = int(pos0)
        if pos0 < 0 or pos0 + len(toks) > self.cfg.seq_len:
            raise ValueError(f"prefill: positions {pos0} .. {pos0 + len(toks) - 1} outside [0, {self.cfg.seq_len})")
        check(self.device.lib.rama_q8_prefill(self.device.ctx, C.byref(self.model.ccfg), C.byref(self.model.weights),
                                              C.byref(self.state), _i32(toks), len(toks), pos0), "rama_q8_prefill")

    def generate(self, prompt_tokens, steps: int, temperature: float = 0.0, topp: float = 0.9, u: float = TOPP_U_CPU):
        """generate() chained on the device (rama_q8_generate); u defaults to the reference's constant draw"""
        out = (C.c_int32 * max(steps, 1))()
        check(self.device.lib.rama_q8_generate(self.device.ctx, C.byref(self.model.ccfg), C.byref(self.model.weights),
                                               C.byref(self.state), _i32(prompt_tokens), len(prompt_tokens), steps, temperature, topp, u, out),
              "rama_q8_generate")
        return [int(v) for v in out[:steps]]

    def generate_greedy(self, prompt_tokens, steps: int):
        return self.generate(prompt_tokens, steps, 0.0)

    SPEC_BLOCK = 4     # steps enqueued between two looks at the ring

    spec_stats = None  # the last generate_spec's report (rama_q8_spec_stats)

    def generate_spec(self, context, max_new, temperature=0.0, topp=0.9, u=TOPP_U_CPU, stop_token=None, n_draft=7, ngram=3,
                      hint=None, on_token=None):
        """speculative decode (rama_q8_spec_begin / _steps / _poll): context = the tokens fed at positions
        0..n-1 (the caller includes BOS) -> the up to max_new sampled tokens, those generate(context[1:], n - 1 + max_new,
        ...)[n-1:] gives, cut after stop_token.  Up to n_draft tokens per step are guessed by looking the last <= ngram
        tokens up in `hint` (a token list, optional) and in the sequence itself, and verified in one weight pass.
        context[:-1] is prefilled here; on_token(index, token), when given, is fed from the host-visible ring while the steps
        run.  The report of the run stays behind as self.spec_stats."""
        ctx_toks, hint_toks, (T, P, U, new, stop, K, N) = spec_plan(self.cfg, context, max_new, temperature, topp, u, stop_token,
                                                                    n_draft, ngram, hint)
        L, ctx = self.device.lib, self.device.ctx
        if len(ctx_toks) > 1:
            self.prefill(ctx_toks[:-1])
        harr = _i32(hint_toks)
        rec = rama_q8_spec_plan(T, P, U, new, stop, K, N, harr if hint_toks else None, len(hint_toks))
        check(L.rama_q8_spec_begin(ctx, C.byref(self.model.ccfg), C.byref(self.model.weights), C.byref(self.state),
                                   _i32(ctx_toks), len(ctx_toks), C.byref(rec)), "rama_q8_spec_begin")
        out, poll = [], _ring_poll(L.rama_q8_spec_poll, "rama_q8_spec_poll", ctx)

        def sink(index, token):
            if on_token is not None:
                on_token(index, token)
            out.append(token)

        def collect():
            """what the ring holds -> True once the sequence has finished and every token has been taken"""
            return _drain(poll, len(out), sink)[1]

        left, done = new, False          # every step before the finish emits at least one token
        while not done:
            if left <= 0:
                raise RuntimeError("generate_spec: max_new steps have run but the sequence has not finished")
            n = min(self.SPEC_BLOCK, left)
            check(L.rama_q8_spec_steps(ctx, n), "rama_q8_spec_steps")
            left -= n
            done = collect()
            while not done and _stream_busy(self.device, 0.0001):
                done = collect()
            if not done:                 # the stream has drained: what the steps emitted is there
                done = collect()
        r = rama_q8_spec_report()
        check(L.rama_q8_spec_stats(ctx, C.byref(r)), "rama_q8_spec_stats")
        self.spec_stats = spec_report(r)
        check(L.rama_q8_spec_end(ctx), "rama_q8_spec_end")
        return out

    def set_graph_mode(self, on: bool):
        check(self.device.lib.rama_set_graph_mode(self.device.ctx, int(bool(on))), "rama_set_graph_mode")

    def free(self):
        if self.state.x:        # (rama_state_free drops the Q8 steps captured over this state; the context's graph mode stays)
            check(self.device.lib.rama_state_free(self.device.ctx, C.byref(self.state)))
            self.state = rama_run_state()


def decode_batch(engines, tokens, positions):
    """one decode step of up to 128 independent sequences over one Q8Model, sharing every weight pass (rama_q8_decode_batch):
    engines[i]'s caches and logits() become what engines[i].forward(tokens[i], positions[i]) would leave"""
    engines = list(engines)
    _check_batch("decode_batch", engines, tokens, positions)
    n, e0 = len(engines), engines[0]
    toks = _tokens(tokens, e0.cfg.vocab_size, "decode_batch")
    poss = [int(p) for p in positions]
    bad = [p for p in poss if not 0 <= p < e0.cfg.seq_len]
    if bad:
        raise ValueError(f"decode_batch: position {bad[0]} outside [0, {e0.cfg.seq_len})")
    states = (rama_run_state * n)(*[e.state for e in engines])
    check(e0.device.lib.rama_q8_decode_batch(e0.device.ctx, C.byref(e0.model.ccfg), C.byref(e0.model.weights), states,
                                             _i32(toks), _i32(poss), n), "rama_q8_decode_batch")


def _per_seq(v, n: int, what: str) -> list:
    """a scalar for every sequence, or one value per sequence"""
    if v is None or np.ndim(v) == 0:
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f"decode_batch_chained: {len(v)} {what} values for {n} sequences")
    return v


def chain_plan(engines, tokens, positions, n_steps, temperature=0.0, topp=0.9, u=TOPP_U_CPU, prompts=None, max_new=None,
               stop_tokens=None):
    """the checked arguments of decode_batch_chained: (tokens, positions, per-sequence records as tuples (temperature, topp, u,
    forced list, max_new, stop token)); ValueError for anything rama_q8_decode_batch_begin would refuse.  No library call."""
    engines = list(engines)
    what = "decode_batch_chained"
    _check_batch(what, engines, tokens, positions)
    n, e0 = len(engines), engines[0]
    n_steps = int(n_steps)
    if n_steps < 1:
        raise ValueError(f"{what}: n_steps {n_steps} < 1")
    V, S = e0.cfg.vocab_size, e0.cfg.seq_len
    toks = _tokens(tokens, V, what)
    poss = [int(p) for p in positions]
    Ts, Ps, Us = (_per_seq(x, n, k) for x, k in ((temperature, "temperature"), (topp, "topp"), (u, "u")))
    news, stops = _per_seq(max_new, n, "max_new"), _per_seq(stop_tokens, n, "stop_tokens")
    prompts = [[] if p is None else _tokens(p, V, what + " prompt") for p in prompts] if prompts is not None else [[] for _ in range(n)]
    if len(prompts) != n:
        raise ValueError(f"{what}: {len(prompts)} prompts for {n} sequences")
    plan = []
    for i in range(n):
        seq = f"{what}: sequence {i}"
        T, P, U = _check_sampler(seq, Ts[i], Ps[i], Us[i])
        new = 0 if news[i] is None else int(news[i])                    # (0 or None: no budget of its own, and no cap on a sampled vocabulary here)
        if new < 0:
            raise ValueError(f"{seq}: max_new {new} < 0")
        stop = _check_stop(seq, stops[i], V)
        budget = min(new, n_steps) if new else n_steps
        if not 0 <= poss[i] <= S - budget:
            raise ValueError(f"{seq}: position {poss[i]} + {budget} steps outside [0, {S}]")
        plan.append((T, P, U, prompts[i], new, stop))
    return toks, poss, plan


def decode_batch_chained(engines, tokens, positions, n_steps, temperature=0.0, topp=0.9, u=TOPP_U_CPU, prompts=None, max_new=None,
                         stop_tokens=None, on_token=None):
    """up to n_steps decode steps of up to 128 independent sequences over one Q8Model, chained on the device
    (rama_q8_decode_batch_begin / _steps / _tokens) -> per sequence the tokens it produced; the lists may differ in length.
    temperature, topp, u, max_new and stop_tokens are scalars or one value per sequence (None: no budget of its own / no
    stop token); prompts is None or one token list per sequence, forced by absolute position as in generate().  A sequence
    ends after max_new tokens or on a sampled stop token, which it still returns.  on_token(sequence, index, token), when
    given, is fed from the host-visible rings (rama_q8_decode_batch_stream_poll) while the steps run, until every sequence
    has set its finished word or the steps have run.  engines[i]'s caches are advanced; its logits() are not written."""
    engines = list(engines)
    toks, poss, plan = chain_plan(engines, tokens, positions, n_steps, temperature, topp, u, prompts, max_new, stop_tokens)
    n, n_steps = len(engines), int(n_steps)
    e0 = engines[0]
    L, ctx = e0.device.lib, e0.device.ctx
    states = (rama_run_state * n)(*[e.state for e in engines])
    forced = [_i32(p[3]) for p in plan]
    per = (rama_q8_seq_plan * n)(*[rama_q8_seq_plan(p[0], p[1], p[2], forced[i], len(p[3]), p[4], p[5]) for i, p in enumerate(plan)])
    check(L.rama_q8_decode_batch_begin(ctx, C.byref(e0.model.ccfg), C.byref(e0.model.weights), states, _i32(toks), _i32(poss), n,
                                       n_steps, per), "rama_q8_decode_batch_begin")
    check(L.rama_q8_decode_batch_steps(ctx, n_steps), "rama_q8_decode_batch_steps")
    if on_token is not None:
        polls = [_ring_poll(L.rama_q8_decode_batch_stream_poll, "rama_q8_decode_batch_stream_poll", ctx, s_) for s_ in range(n)]
        seen, done = [0] * n, [False] * n
        ran = False                   # the stream has drained: one more sweep collects what is there
        while not all(done):
            progress = 0
            for s_ in range(n):
                if not done[s_]:
                    k, done[s_] = _drain(polls[s_], seen[s_], lambda i, t: on_token(s_, i, t))
                    seen[s_] += k
                    progress += k
            if progress or all(done):
                continue
            if ran:
                raise RuntimeError(f"decode_batch_chained: the steps have run but sequences {[i for i in range(n) if not done[i]]} have not finished")
            ran = not _stream_busy(e0.device, 0.0002)
    out = (C.c_int32 * (n * n_steps))()
    cnt = (C.c_int32 * n)()
    check(L.rama_q8_decode_batch_tokens(ctx, out, n_steps, cnt), "rama_q8_decode_batch_tokens")
    return [[int(out[s_ * n_steps + j]) for j in range(cnt[s_])] for s_ in range(n)]


# ------------------------------------------------------------------ the serving chain: continuous batching (rama_q8_serve_*)

def serve_sizes(cfg, n_slots, max_rows, max_new_cap, who="Q8Server"):
    """the checked sizes of a serving chain; ValueError for what rama_q8_serve_begin would refuse as a bad size.  No library call."""
    n_slots, max_new_cap = int(n_slots), int(max_new_cap)
    max_rows = n_slots if max_rows is None else int(max_rows)
    if not 1 <= n_slots <= MAX_BATCH:
        raise ValueError(f"{who}: {n_slots} slots, not 1..{MAX_BATCH}")
    if not n_slots <= max_rows <= MAX_BATCH:
        raise ValueError(f"{who}: max_rows {max_rows} outside [n_slots = {n_slots}, {MAX_BATCH}]")
    if not 1 <= max_new_cap <= cfg.seq_len - 1:
        raise ValueError(f"{who}: max_new_cap {max_new_cap} outside [1, seq_len - 1 = {cfg.seq_len - 1}]")
    return n_slots, max_rows, max_new_cap


def serve_plan(cfg, context, max_new, temperature=0.0, topp=0.9, u=TOPP_U_CPU, stop_token=None, max_new_cap=None, n_cached=0, who="Q8Server"):
    """the checked arguments of Q8Server.submit: (context tokens, (temperature, topp, u, max_new, stop token)); ValueError for
    everything rama_q8_serve_admit / rama_q8_serve_admit_at would refuse in them.  No library call."""
    what = who + ".submit"
    V, S = cfg.vocab_size, cfg.seq_len
    ctx = _check_context(what, context, V)
    if not 0 <= int(n_cached) <= len(ctx) - 1:
        raise ValueError(f"{what}: n_cached {int(n_cached)} outside [0, n_context - 1 = {len(ctx) - 1}] (the final context position is always fed)")
    T, P, U = _check_sampler(what, temperature, topp, u)
    new = int(max_new)
    _check_budget(what, len(ctx), new, S, max_new_cap)
    stop = _check_stop(what, stop_token, V)
    _check_sampled_vocab(what, T, V)
    return ctx, (T, P, U, new, stop)


def serve_plan_step(slots, max_rows):
    """rama_q8_serve_plan_step, the scheduling rule as a pure host function: slots = (state, n_context, cursor, n_out, max_new)
    tuples -> (rows [(slot, pos, logits)] * max_rows, the slots after the step when no stop token is sampled).  No GPU."""
    n, table, max_rows = len(slots), _slot_table(slots), int(max_rows)
    rows = (rama_q8_serve_row * max(max_rows, 1))()
    after = (rama_q8_serve_slot * max(n, 1))()
    check(load().rama_q8_serve_plan_step(table, n, max_rows, rows, after), "rama_q8_serve_plan_step")
    return _row_table(rows, max_rows), [(a.state, a.n_context, a.cursor, a.n_out, a.max_new) for a in after[:n]]


def common_prefix(a, b) -> int:
    """the number of leading tokens two sequences share"""
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


def serve_spec_sizes(n_draft, ngram, hint_cap, who="Q8Server"):
    """the checked drafting sizes of a Q8Server (or, `who`, a Server); ValueError for what rama_q8_serve_begin_spec would refuse.
    No library call."""
    n_draft, ngram, hint_cap = int(n_draft), int(ngram), int(hint_cap)
    _check_drafting(who, n_draft, ngram)
    if hint_cap < 0 or (hint_cap and not n_draft):
        raise ValueError(f"{who}: hint_cap {hint_cap} (>= 0, and 0 on a server without drafts)")
    return n_draft, ngram, hint_cap


def serve_spec_request(cfg, n_draft_cap, ngram, hint_cap, n_draft=None, hint=None, who="Q8Server"):
    """the checked drafting arguments of Q8Server.submit: (n_draft, ngram, hint tokens); ValueError for everything
    rama_q8_serve_admit_spec would refuse in them.  No library call."""
    what = who + ".submit"
    K = n_draft_cap if n_draft is None else int(n_draft)
    _check_n_draft(what, K, n_draft_cap, f"the server's n_draft = {n_draft_cap}")
    toks = [] if hint is None else _tokens(hint, cfg.vocab_size, what + " hint")
    if len(toks) > hint_cap:
        raise ValueError(f"{what}: {len(toks)} hint tokens beyond the server's hint_cap {hint_cap}")
    return K, ngram, toks


def serve_spec_report(r) -> dict:
    """a rama_q8_serve_spec_report as a dict: its counters and caps, and the last step's drafts of its n_slots slots"""
    d = _report(r, skip=("n_slots", "max_rows"))
    d["last_want"], d["last_granted"] = d["last_want"][:r.n_slots], d["last_granted"][:r.n_slots]
    return d


def serve_spec_plan_step(slots, want, max_rows):
    """rama_q8_serve_spec_plan_step, the scheduling rule with drafts as a pure host function: slots = (state, n_context, cursor,
    n_out, max_new) tuples, want = the drafts every slot has for the step -> (rows [(slot, pos, logits)] * max_rows, the drafts
    granted per slot).  No GPU."""
    n = len(slots)
    if len(want) != n:
        raise ValueError(f"serve_spec_plan_step: {len(want)} want values for {n} slots")
    table, warr, max_rows = _slot_table(slots), _i32([int(v) for v in want]), int(max_rows)
    rows = (rama_q8_serve_row * max(max_rows, 1))()
    granted = (C.c_int32 * max(n, 1))()
    check(load().rama_q8_serve_spec_plan_step(table, n, max_rows, warr, rows, granted), "rama_q8_serve_spec_plan_step")
    return _row_table(rows, max_rows), granted[:n]


class PrefixPool:
    """the donors of Q8Server's prefix cache: at most k engines, each keyed by the tokens whose cache rows it holds (row t is a
    function of tokens 0..t only, and its bits do not depend on who computed it).  Least recently used goes first.  Pure host
    logic: an engine is any object, compared by identity.  While an engine is here it is a donor and nothing else."""

    def __init__(self, k: int):
        self.k = int(k)
        if self.k < 0:
            raise ValueError(f"PrefixPool: {self.k} donors")
        self._donors = []                                 # [tokens, engine], least recently used first

    def __len__(self):
        return len(self._donors)

    def __contains__(self, engine):
        return any(d[1] is engine for d in self._donors)

    def engines(self):
        return [d[1] for d in self._donors]

    def match(self, context, at_least: int = 1):
        """-> (engine, n): the donor that shares the longest token prefix with `context`, n capped at len(context) - 1 (the final
        context position is always fed: its logits are needed); (None, 0) when no donor shares at_least tokens.  Of equally
        long matches the most recently used wins.  The donor found becomes the most recently used."""
        best, best_n = None, 0
        for d in self._donors:                            # (later = more recently used: >= lets it win a tie)
            n = min(common_prefix(d[0], context), len(context) - 1)
            if n >= max(at_least, 1) and n >= best_n:
                best, best_n = d, n
        if best is None:
            return None, 0
        self._donors.remove(best)
        self._donors.append(best)
        return best[1], best_n

    def put(self, tokens, engine):
        """`engine` holds the rows of `tokens` and becomes the most recently used donor -> the engines that left the pool for
        it (none while there is room; the engine itself when k == 0)"""
        if engine in self:
            raise ValueError("PrefixPool.put: the engine is already a donor")
        if self.k == 0:
            return [engine]
        self._donors.append([list(tokens), engine])
        out = []
        while len(self._donors) > self.k:
            out.append(self._donors.pop(0)[1])
        return out

    def clear(self):
        out, self._donors = self.engines(), []
        return out


class ServeLoop:
    """What a serving chain's host loop does whatever the model: the queue, the slots' engines, the mirror of the device's slot table kept
    by the host plan (rama_q8_serve_plan_step), the steps to the next finish, admissions behind the steps in flight, the host-visible
    rings.  Q8Server (rama_q8_serve_*) and rama_amd.Server (rama_serve_*, parity mode) are this loop over their entries' family; a
    subclass says how a chain begins (_begin), what engine a slot gets (_new_engine) and how a request goes in (_admit_slot).
    CachingServeLoop below adds what both servers offer on request: prompt caching and drafts."""

    ABI = None         # the C entries' family: <ABI>_begin / _admit / _steps / _poll / _stats / _end
    NAME = "ServeLoop"
    spec = False       # with drafts the rows of a step depend on what is accepted: no host plan (CachingServeLoop)

    def _call(self, name, *args):
        entry = f"{self.ABI}_{name}"
        check(getattr(self.device.lib, entry)(self.device.ctx, *args), entry)

    def _start(self, model, n_slots, max_rows, max_new_cap):
        """the sizes (checked before any library call), the chain's begin, the loop's books"""
        self.n_slots, self.max_rows, self.max_new_cap = serve_sizes(model.cfg, n_slots, max_rows, max_new_cap, self.NAME)
        self.model, self.device, self.cfg = model, model.device, model.cfg
        self._begin()
        L = self.device.lib
        self._open = True
        self._own = [None] * self.n_slots                 # the server's own engine of a slot, made on first use and reused
        self._eng = [None] * self.n_slots                 # the engine the slot's occupant runs on
        self._spare = []                                  # the server's own engines that serve nobody
        self._mine = []                                   # every engine the server made (close frees them)
        self._req = [None] * self.n_slots                 # the handle a slot serves
        self._seen = [0] * self.n_slots
        self._poll = [_ring_poll(getattr(L, self.ABI + "_poll"), self.ABI + "_poll", self.device.ctx, slot, after=(None,)) for slot in range(self.n_slots)]
        self._mirror =[(SERVE_FREE, 0, 0, 0, 0)] * self.n_slots      # the host's copy of the slot table (exact unless a stop token fell)
        self._queue, self._results, self._finished, self._plans = [], {}, set(), {}
        self._next = 0
        self.planned = dict(steps=0, rows_decode=0, rows_prompt=0, rows_idle=0)      # the host plan's sums over the steps enqueued (none with drafts: no host plan)
        self.last_rows = []                               # ... and its row table of the last one

    def _begin(self):
        self._call("begin", C.byref(self.model.ccfg), C.byref(self.model.weights), self.n_slots, self.max_rows, self.max_new_cap)

    def _new_engine(self):
        raise NotImplementedError

    def _admit_slot(self, slot, h, eng, toks, rec, n_cached):
        """the request h goes into the slot on engine eng -> the n_cached it was admitted with"""
        self._call("admit", slot, C.byref(eng.state), _i32(toks), len(toks), C.byref(rec))
        return 0

    def _admitted(self, h, n_cached):
        pass

    def _retire(self, slot, h):
        """a finished occupant leaves its engine"""
        self._eng[slot] = None

    def _closed(self):
        pass

    # -- requests
    def _submit(self, ctx, plan, engine, n_cached=0, retain=False):
        """a checked request joins the queue -> its handle"""
        if engine is not None and engine.model is not self.model:
            raise ValueError(f"{self.NAME}.submit: the engine belongs to another {type(self.model).__name__}")
        if engine is not None and any(e is engine for e in self._engines_in_use()):
            raise ValueError(f"{self.NAME}.submit: the engine already serves a queued or running request")
        h = self._next
        self._next += 1
        self._plans[h] = (ctx, plan, engine, n_cached, bool(retain))
        self._results[h] = []
        self._queue.append(h)
        return h

    def _engines_in_use(self):
        waiting = [self._plans[h][2] for h in self._queue]
        running = [self._eng[i] for i, h in enumerate(self._req) if h is not None]
        return [e for e in waiting + running if e is not None]

    def _admit(self):
        for slot in range(self.n_slots):
            if not self._queue:
                return
            if self._req[slot] is not None:
                continue
            h = self._queue[0]                             # (it leaves the queue once the library has taken it)
            toks, (T, P, U, new, stop), eng, n_cached, _ = self._plans[h]
            if eng is None:
                if self._own[slot] is None:
                    self._own[slot] = self._spare.pop() if self._spare else self._new_engine()
                eng = self._own[slot]
            n_cached = self._admit_slot(slot, h, eng, toks, rama_q8_serve_plan(T, P, U, new, stop), n_cached)
            self._queue.pop(0)
            self._req[slot], self._seen[slot], self._eng[slot] = h, 0, eng
            self._admitted(h, n_cached)
            self._mirror[slot] = (SERVE_PROMPT, len(toks), n_cached, 0, new)

    def _collect(self, on_token=None):
        """what the rings hold: new tokens of every occupied slot; a finished occupant frees its slot"""
        early = False
        for slot in range(self.n_slots):
            h = self._req[slot]
            if h is None:
                continue
            got = self._results[h]

            def sink(index, token):
                if on_token is not None:
                    on_token(h, index, token)
                got.append(token)
            n, fin = _drain(self._poll[slot], self._seen[slot], sink)
            self._seen[slot] += n
            if fin:
                self._finished.add(h)
                self._req[slot] = None
                self._retire(slot, h)
                early = early or self._mirror[slot][0] != SERVE_DONE
                self._mirror[slot] = (SERVE_DONE,) + tuple(self._mirror[slot][1:])
        return early

    def step(self, n: int = 1, on_token=None):
        """collect what has arrived, admit queued requests into free slots, then enqueue n steps (asynchronous)"""
        if self._collect(on_token):
            self._resync()
        self._admit()
        self._count_and_enqueue(int(n))

    def _count_and_enqueue(self, n):
        for _ in range(0 if self.spec else n):            # (with drafts the rows of a step depend on what is accepted: no host plan)
            before = self._mirror
            rows, self._mirror = serve_plan_step(before, self.max_rows)
            self.last_rows = rows
            dec = sum(1 for s, _, _ in rows if s >= 0 and before[s][0] == SERVE_DECODE)
            used = sum(1 for s, _, _ in rows if s >= 0)
            self.planned["steps"] += 1
            self.planned["rows_decode"] += dec
            self.planned["rows_prompt"] += used - dec
            self.planned["rows_idle"] += self.max_rows - used
        if n:
            self._call("steps", n)

    def _resync(self):
        """a stop token ended a sequence before its budget: the host's copy of the slot table is taken from the device again"""
        st = self.stats()
        self._mirror = [s if self._req[i] is not None or s[0] in (SERVE_FREE, SERVE_DONE) else (SERVE_DONE,) + s[1:] for i, s in enumerate(st["slots"])]

    def _steps_to_next_finish(self):
        """by the host plan: the steps until a slot finishes (requests waiting) or until all have (none waiting)"""
        m, k = list(self._mirror), 0
        live = lambda t: [s[0] in (SERVE_PROMPT, SERVE_DECODE) for s in t]
        start = live(m)
        while any(live(m)):
            _, m = serve_plan_step(m, self.max_rows)
            k += 1
            if self._queue and live(m) != start:
                break
        return k

    LOOKAHEAD = 2      # steps enqueued past a foreseen finish while requests wait: the admission then goes in behind running steps

    def run(self, on_token=None):
        """serve every submitted request to its end.  on_token(handle, index, token), when given, is fed from the host-visible
        rings.  The steps up to the next finish the host plan foresees -- and, while requests wait, LOOKAHEAD more, so that the
        device does not idle until the host has seen the finished word and admitted -- are enqueued at once; a DONE slot takes
        no rows, and an admission is stream-ordered behind them, so the host plan stays exact.  A stop token that ends a sequence
        earlier is seen at the next collection."""
        done_in = lambda t: {i for i in range(self.n_slots) if self._req[i] is not None and t[i][0] == SERVE_DONE}
        while True:
            if self._collect(on_token):
                self._resync()
            self._admit()
            expect = done_in(self._mirror)                # finished by the plan, not yet seen
            k = self._steps_to_next_finish()
            if k == 0 and not expect:
                if self._queue:
                    raise RuntimeError(f"{self.NAME}.run: requests are waiting but no slot can take them")
                return
            if k:
                after = self._after(k)
                expect |= done_in(after)
                live_on = any(s[0] in (SERVE_PROMPT, SERVE_DECODE) for s in after)
                self._count_and_enqueue(k + (self.LOOKAHEAD if self._queue and live_on else 0))
            while True:                       # until the slots the plan ends here have set their finished words
                if self._collect(on_token):
                    self._resync()
                if all(self._req[i] is None for i in expect):
                    break
                if _stream_busy(self.device, 0.0001):
                    continue
                self._collect(on_token)
                if not all(self._req[i] is None for i in expect):
                    raise RuntimeError(f"{self.NAME}.run: the steps have run but slots {[i for i in expect if self._req[i] is not None]} have not finished")
                break

    def _after(self, k):
        m = list(self._mirror)
        for _ in range(k):
            _, m = serve_plan_step(m, self.max_rows)
        return m

    def finished(self, handle) -> bool:
        return handle in self._finished

    def poll(self, on_token=None):
        """collect what the rings hold now (never touches the stream); on_token(handle, index, token) for every new token"""
        if self._collect(on_token):
            self._resync()

    def result(self, handle):
        """the tokens of request `handle` collected so far by run / step / poll (all of them once finished(handle))"""
        return list(self._results[handle])

    def stats(self):
        """<ABI>_stats (synchronises): the device's counters, the slot table, the last step's row table"""
        r = rama_q8_serve_report()
        self._call("stats", C.byref(r))
        return dict(steps=int(r.steps), graph_captures=int(r.graph_captures), rows_decode=int(r.rows_decode), rows_prompt=int(r.rows_prompt),
                    rows_idle=int(r.rows_idle), n_slots=int(r.n_slots), max_rows=int(r.max_rows),
                    last_rows=_row_table(r.last_rows, r.max_rows),
                    slots=[(s.state, s.n_context, s.cursor, s.n_out, s.max_new) for s in r.slots[:r.n_slots]],
                    generation=[int(g) for g in r.generation[:r.n_slots]])

    def close(self):
        if self._open:
            self._open = False
            self._call("end")
            self._closed()
            for e in self._mine:
                e.free()
            self._mine, self._spare = [], []
            self._own, self._eng = [None] * self.n_slots, [None] * self.n_slots


class CachingServeLoop(ServeLoop):
    """ServeLoop with what both serving chains offer on request, one copy for Q8Server (rama_q8_serve_*) and rama_amd.Server
    (rama_serve_*): prompt caching -- submit(n_cached=), the donor pool of prefix_cache=k, the fork (rama_q8_kv_fork: the KV cache
    is fp32 in both stacks) and <ABI>_admit_at -- and drafts -- <ABI>_begin_spec / _admit_spec / _spec_stats and the run loop of a
    chain whose steps the host cannot foresee."""

    def _start_caching(self, model, n_slots, max_rows, max_new_cap, prefix_cache, n_draft, ngram, hint_cap):
        serve_sizes(model.cfg, n_slots, max_rows, max_new_cap, self.NAME)      # (every size is checked before any library call, in this order)
        self.n_draft, self.ngram, self.hint_cap = serve_spec_sizes(n_draft, ngram, hint_cap, self.NAME)
        self.spec = self.n_draft > 0                      # n_draft == 0: the plain chain, <ABI>_begin
        self.pool = PrefixPool(prefix_cache)              # (raises before any library call)
        self._cached = {}                                 # handle -> the n_cached it was admitted with
        self._drafts = {}                                 # handle -> (n_draft, ngram, hint tokens)
        self.rows_cached = 0                              # ... summed over the admissions
        self._start(model, n_slots, max_rows, max_new_cap)

    def _begin(self):
        if not self.spec:
            return super()._begin()
        m = self.model
        self._call("begin_spec", C.byref(m.ccfg), C.byref(m.weights), self.n_slots, self.max_rows, self.max_new_cap, self.n_draft, self.hint_cap)

    # -- requests
    def submit(self, context, max_new, temperature=0.0, topp=0.9, u=TOPP_U_CPU, stop_token=None, engine=None, n_cached=0,
               retain=False, n_draft=None, hint=None):
        """queue a request -> its handle.  It is admitted at once if a slot is free, else when one finishes (step / run).
        engine: the engine whose run state the sequence uses (default: one the server owns for the slot).
        n_cached: rows 0..n_cached-1 of `engine` already hold context[0..n_cached) -- written by work enqueued earlier on the
        device's stream; the slot feeds the rest (at most n_context - 1: the final position is always fed).  Such a request is
        not matched against the prefix cache.
        retain: with a prefix cache, the engine stays behind as a donor when the request finishes (a caller's engine too: it
        is the pool's until it is evicted).
        n_draft, hint: on a server made with n_draft > 0, the drafts per step of this request (default: the server's; 0: none)
        and a token list to look up in besides the request's own text (at most hint_cap tokens).  The tokens are the same
        whatever they are."""
        ctx, plan = serve_plan(self.cfg, context, max_new, temperature, topp, u, stop_token, self.max_new_cap, n_cached, self.NAME)
        draft = serve_spec_request(self.cfg, self.n_draft, self.ngram, self.hint_cap, n_draft, hint, self.NAME)
        n_cached = int(n_cached)
        if n_cached and engine is None:
            raise ValueError(f"{self.NAME}.submit: n_cached needs the engine that holds the rows")
        if engine is not None and engine.model is not self.model:
            raise ValueError(f"{self.NAME}.submit: the engine belongs to another {type(self.model).__name__}")
        if engine is not None and any(e is engine for e in self._engines_in_use()):
            raise ValueError(f"{self.NAME}.submit: the engine already serves a queued or running request")
        if engine is not None and engine in self.pool:
            raise ValueError(f"{self.NAME}.submit: the engine is a donor of the prefix cache")
        h = self._submit(ctx, plan, engine, n_cached, retain)
        self._drafts[h] = draft
        self._admit()
        return h

    def _admit_slot(self, slot, h, eng, toks, rec, n_cached):
        L, ctx = self.device.lib, self.device.ctx
        if not n_cached and len(self.pool):
            # the donor stays in the pool whatever happens below: donors leave it in _collect only, so a fork that was
            # enqueued and an admission that then failed find it there at the next attempt; an evicted donor is reused or
            # freed behind the fork in stream order
            donor, n_cached = self.pool.match(toks, self.MIN_CACHED)
            if n_cached:
                check(L.rama_q8_kv_fork(ctx, C.byref(self.model.ccfg), C.byref(donor.state), C.byref(eng.state), 1, n_cached),
                      "rama_q8_kv_fork")
        arr = _i32(toks)
        if self.spec:
            K, N, hint = self._drafts[h]
            harr = _i32(hint)
            srec = rama_q8_serve_spec(K, N, harr if hint else None, len(hint))
            self._call("admit_spec", slot, C.byref(eng.state), arr, len(toks), n_cached, C.byref(rec), C.byref(srec))
        elif n_cached:
            self._call("admit_at", slot, C.byref(eng.state), arr, len(toks), n_cached, C.byref(rec))
        else:
            self._call("admit", slot, C.byref(eng.state), arr, len(toks), C.byref(rec))
        return n_cached

    def _admitted(self, h, n_cached):
        self._cached[h] = n_cached
        self.rows_cached += n_cached

    def _retire(self, slot, h):
        """a finished occupant: with retain and a prefix cache its engine becomes a donor, keyed by the tokens it was fed (the
        context and every output but the last); whoever leaves the pool for it serves requests again if the server made it"""
        toks, _, _, _, retain = self._plans[h]
        eng, self._eng[slot] = self._eng[slot], None
        if not retain or self.pool.k == 0:
            return
        if self._own[slot] is eng:
            self._own[slot] = None
        for e in self.pool.put(toks + self._results[h][:-1], eng):
            if any(e is m for m in self._mine):
                self._spare.append(e)

    def cached(self, handle) -> int:
        """the n_cached request `handle` was admitted with (None while it waits)"""
        return self._cached.get(handle)

    MIN_CACHED = 2     # a shorter match is not worth a launch: every context shares its first token (BOS) with every donor

    def run(self, on_token=None):
        """ServeLoop.run; with drafts, _run_drafting"""
        return self._run_drafting(on_token) if self.spec else super().run(on_token)

    SPEC_BLOCK = 4     # with drafts: at most this many steps between two looks at the device's slot table

    def _run_drafting(self, on_token=None):
        """run() on a server with drafts.  A slot may finish earlier than the host plan foresees, so the plan -- one token per
        DECODE slot and step -- is an upper bound: the slot table is taken from the device before every block, the steps to the
        next finish by that plan -- SPEC_BLOCK at most -- are enqueued, and the finished words alone say who has finished.  A request that waits is
        admitted as soon as a finished word shows, behind the steps still in flight; the device never idles past a finish by
        more than the block enqueued."""
        while True:
            self._resync()                                # (synchronises: the block before has run)
            self._collect(on_token)
            self._admit()
            if all(h is None for h in self._req):
                if self._queue:
                    raise RuntimeError(f"{self.NAME}.run: requests are waiting but no slot can take them")
                return
            self._count_and_enqueue(max(min(self._steps_to_next_finish(), self.SPEC_BLOCK), 1))
            while True:
                self._collect(on_token)
                self._admit()
                if not _stream_busy(self.device, 0.0001):
                    break

    def stats(self):
        """<ABI>_stats (synchronises): the device's counters, the slot table, the last step's row table; rows_cached is the
        host's sum of n_cached over the admissions (context positions taken from cached rows instead of being fed); with drafts,
        spec = <ABI>_spec_stats"""
        out = dict(super().stats(), rows_cached=self.rows_cached)
        if self.spec:
            q = rama_q8_serve_spec_report()
            self._call("spec_stats", C.byref(q))
            out["spec"] = serve_spec_report(q)
        return out

    def _closed(self):
        self.pool.clear()                             # (a caller's engine that was a donor is the caller's again)


class Q8Server(CachingServeLoop):
    """continuous batching over one Q8Model (rama_q8_serve_begin / _admit / _steps / _poll): n_slots sequence slots share weight
    passes of max_rows rows; a finished sequence frees its slot for the next queued request while the others run on, and a new
    request's context is ingested in chunks next to the decoding slots.  Every request's tokens are those Q8Engine.generate gives
    it alone.  One serving chain per device context at a time.

    Prompt caching.  submit(..., n_cached=n) admits over rows 0..n-1 that the caller's engine already holds
    (a chat's next turn on the same engine).  prefix_cache=k keeps a pool of at most k donor engines: a request submitted with
    retain=True leaves its engine there when it finishes, keyed by the tokens whose rows it holds; every later request is
    matched against the pool at its admission, the longest shared prefix is forked into its engine (rama_q8_kv_fork) and the
    slot starts at that cursor (rama_q8_serve_admit_at).  The tokens are the same with the cache on and off.

    Drafts.  n_draft=K > 0 begins the chain with rama_q8_serve_begin_spec: a decoding request guesses up to K
    tokens per step by looking its last <= ngram tokens up in its own text and in the hint it was submitted with (at most
    hint_cap tokens), the guesses take the rows of the step that no slot wants -- prompts first -- and are verified in the same
    weight pass.  The tokens are the same with drafts on and off; n_draft=0 (the default) is the plain chain."""

    ABI = "rama_q8_serve"
    NAME = "Q8Server"

    def __init__(self, model: Q8Model, n_slots: int, max_rows=None, max_new_cap: int = 256, prefix_cache: int = 0, n_draft: int = 0,
                 ngram: int = 3, hint_cap: int = 0):
        self._start_caching(model, n_slots, max_rows, max_new_cap, prefix_cache, n_draft, ngram, hint_cap)

    def _new_engine(self):
        e = Q8Engine(self.device, self.model)
        self._mine.append(e)
        return e


# ------------------------------------------------------------------ the speculative chain: n-gram lookup drafts (rama_q8_spec_*)

def spec_plan(cfg, context, max_new, temperature=0.0, topp=0.9, u=TOPP_U_CPU, stop_token=None, n_draft=7, ngram=3, hint=None):
    """the checked arguments of Q8Engine.generate_spec: (context tokens, hint tokens, (temperature, topp, u, max_new, stop token,
    n_draft, ngram)); ValueError for everything rama_q8_spec_begin would refuse in them.  No library call."""
    what = "generate_spec"
    V, S = cfg.vocab_size, cfg.seq_len
    ctx = _check_context(what, context, V)
    hint_toks = [] if hint is None else _tokens(hint, V, what + " hint")
    T, P, U = _check_sampler(what, temperature, topp, u)
    new, K, N = int(max_new), int(n_draft), int(ngram)
    _check_budget(what, len(ctx), new, S)
    _check_drafting(what, K, N)
    stop = _check_stop(what, stop_token, V)
    _check_sampled_vocab(what, T, V)
    return ctx, hint_toks, (T, P, U, new, stop, K, N)


def spec_report(r) -> dict:
    """a rama_q8_spec_report as a dict"""
    return _report(r)


def spec_draft(hint, seq, n_draft, ngram, room):
    """rama_q8_spec_draft, the drafting rule as a pure host function: the tokens that follow the latest occurrence of the last
    <= ngram tokens of seq -- in hint first, then in seq itself -- at most min(n_draft, room) of them.  No GPU."""
    hint, seq = [int(t) for t in (hint or [])], [int(t) for t in seq]
    out = (C.c_int32 * (MAX_DRAFT + 1))()
    n = load().rama_q8_spec_draft(_i32(hint) if hint else None, len(hint), _i32(seq), len(seq), int(n_draft), int(ngram), int(room), out)
    if n < 0:
        check(n, "rama_q8_spec_draft")
    return out[:n]


def spec_accept(drafts, picks, stop_token, remaining):
    """rama_q8_spec_accept, the accept rule as a pure host function: picks = Device::sample of rows 0..len(drafts) ->
    (tokens emitted, finished).  No GPU."""
    drafts, picks = [int(t) for t in drafts], [int(t) for t in picks]
    if len(picks) != len(drafts) + 1:
        raise ValueError(f"spec_accept: {len(picks)} picks for {len(drafts)} drafts, not one more")
    fin = C.c_int()
    n = load().rama_q8_spec_accept(_i32(drafts), len(drafts), _i32(picks), -1 if stop_token is None else int(stop_token), int(remaining), C.byref(fin))
    if n < 0:
        check(n, "rama_q8_spec_accept")
    return n, bool(fin.value)
