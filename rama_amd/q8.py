"""Q8_0 models over the C ABI: llama2.c version-2 checkpoints (rama_q8_model_load) and synthetic Q8 models
(rama_q8_model_synth), decoded by the Q8 forward (runq.c's quantized products, rama's exact ops elsewhere;
include/rama_hip.h).  The fp32 Model / Engine are untouched.  No CPU fallback anywhere."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Q8_TENSORS, check, rama_config, rama_q8_weights, rama_run_state
from .sampler_const import TOPP_U_CPU
from .transformer import Config, Hip


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
        arr = (C.c_int32 * len(toks))(*toks)
        check(self.device.lib.rama_q8_prefill(self.device.ctx, C.byref(self.model.ccfg), C.byref(self.model.weights),
                                              C.byref(self.state), arr, len(toks), pos0), "rama_q8_prefill")

    def generate(self, prompt_tokens, steps: int, temperature: float = 0.0, topp: float = 0.9, u: float = TOPP_U_CPU):
        """generate() chained on the device (rama_q8_generate); u defaults to the reference's constant draw"""
        pt = (C.c_int32 * max(len(prompt_tokens), 1))(*prompt_tokens)
        out = (C.c_int32 * max(steps, 1))()
        check(self.device.lib.rama_q8_generate(self.device.ctx, C.byref(self.model.ccfg), C.byref(self.model.weights),
                                               C.byref(self.state), pt, len(prompt_tokens), steps, temperature, topp, u, out),
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
        from ._lib import rama_q8_spec_plan, rama_q8_spec_report
        import time
        ctx_toks, hint_toks, (T, P, U, new, stop, K, N) = spec_plan(self.cfg, context, max_new, temperature, topp, u, stop_token,
                                                                    n_draft, ngram, hint)
        L, ctx = self.device.lib, self.device.ctx
        if len(ctx_toks) > 1:
            self.prefill(ctx_toks[:-1])
        harr = (C.c_int32 * max(len(hint_toks), 1))(*hint_toks)
        rec = rama_q8_spec_plan(T, P, U, new, stop, K, N, harr if hint_toks else None, len(hint_toks))
        check(L.rama_q8_spec_begin(ctx, C.byref(self.model.ccfg), C.byref(self.model.weights), C.byref(self.state),
                                   (C.c_int32 * len(ctx_toks))(*ctx_toks), len(ctx_toks), C.byref(rec)), "rama_q8_spec_begin")
        out, buf = [], (C.c_int32 * 64)()
        k, fin = C.c_int(), C.c_int()

        def collect():
            """what the ring holds -> True once the finished word is set and every token has been taken"""
            while True:
                # the finished word is read before the ring: once it is set, every token is there
                check(L.rama_q8_spec_poll(ctx, len(out), buf, 64, C.byref(k), C.byref(fin)), "rama_q8_spec_poll")
                for i in range(k.value):
                    if on_token is not None:
                        on_token(len(out), int(buf[i]))
                    out.append(int(buf[i]))
                if k.value < 64:
                    return bool(fin.value)

        left, done = new, False          # every step before the finish emits at least one token
        while not done:
            if left <= 0:
                raise RuntimeError("generate_spec: max_new steps have run but the sequence has not finished")
            n = min(self.SPEC_BLOCK, left)
            check(L.rama_q8_spec_steps(ctx, n), "rama_q8_spec_steps")
            left -= n
            while True:
                done = collect()
                if done:
                    break
                q = L.rama_stream_query(ctx)
                if q == 1:
                    time.sleep(0.0001)
                    continue
                check(q, "rama_stream_query")
                done = collect()
                break
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


MAX_BATCH = 128


def _tokens(tokens, vocab_size: int, what: str) -> list:
    out = [int(t) for t in tokens]
    bad = [t for t in out if not 0 <= t < vocab_size]
    if bad:
        raise ValueError(f"{what}: token {bad[0]} outside the vocabulary [0, {vocab_size})")
    return out


def decode_batch(engines, tokens, positions):
    """one decode step of up to 128 independent sequences over one Q8Model, sharing every weight pass (rama_q8_decode_batch):
    engines[i]'s caches and logits() become what engines[i].forward(tokens[i], positions[i]) would leave"""
    engines = list(engines)
    n = len(engines)
    if not 1 <= n <= MAX_BATCH:
        raise ValueError(f"decode_batch: {n} sequences, not 1..{MAX_BATCH}")
    if len(tokens) != n or len(positions) != n:
        raise ValueError(f"decode_batch: {len(tokens)} tokens and {len(positions)} positions for {n} sequences")
    e0 = engines[0]
    if any(e.model is not e0.model for e in engines):
        raise ValueError("decode_batch: the engines do not share one Q8Model")
    if len({id(e) for e in engines}) != n:
        raise ValueError("decode_batch: an engine appears twice")
    toks = _tokens(tokens, e0.cfg.vocab_size, "decode_batch")
    poss = [int(p) for p in positions]
    bad = [p for p in poss if not 0 <= p < e0.cfg.seq_len]
    if bad:
        raise ValueError(f"decode_batch: position {bad[0]} outside [0, {e0.cfg.seq_len})")
    states = (rama_run_state * n)(*[e.state for e in engines])
    check(e0.device.lib.rama_q8_decode_batch(e0.device.ctx, C.byref(e0.model.ccfg), C.byref(e0.model.weights), states,
                                             (C.c_int32 * n)(*toks), (C.c_int32 * n)(*poss), n), "rama_q8_decode_batch")


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
    n = len(engines)
    what = "decode_batch_chained"
    if not 1 <= n <= MAX_BATCH:
        raise ValueError(f"{what}: {n} sequences, not 1..{MAX_BATCH}")
    if len(tokens) != n or len(positions) != n:
        raise ValueError(f"{what}: {len(tokens)} tokens and {len(positions)} positions for {n} sequences")
    e0 = engines[0]
    if any(e.model is not e0.model for e in engines):
        raise ValueError(f"{what}: the engines do not share one Q8Model")
    if len({id(e) for e in engines}) != n:
        raise ValueError(f"{what}: an engine appears twice")
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
        T, P, U = float(Ts[i]), float(Ps[i]), float(Us[i])
        if not (T >= 0.0 and 0.0 <= P <= 1.0 and 0.0 <= U < 1.0):       # (false for NaN)
            raise ValueError(f"{what}: sequence {i}: temperature >= 0, topp in [0, 1], u in [0, 1) -- not {T}, {P}, {U}")
        new = 0 if news[i] is None else int(news[i])
        if new < 0:
            raise ValueError(f"{what}: sequence {i}: max_new {new} < 0")
        stop = -1 if stops[i] is None else int(stops[i])
        if not -1 <= stop < V:
            raise ValueError(f"{what}: sequence {i}: stop token {stop} outside the vocabulary [0, {V})")
        budget = min(new, n_steps) if new else n_steps
        if not 0 <= poss[i] <= S - budget:
            raise ValueError(f"{what}: sequence {i}: position {poss[i]} + {budget} steps outside [0, {S}]")
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
    from ._lib import rama_q8_seq_plan
    engines = list(engines)
    toks, poss, plan = chain_plan(engines, tokens, positions, n_steps, temperature, topp, u, prompts, max_new, stop_tokens)
    n, n_steps = len(engines), int(n_steps)
    e0 = engines[0]
    L, ctx = e0.device.lib, e0.device.ctx
    states = (rama_run_state * n)(*[e.state for e in engines])
    forced = [(C.c_int32 * max(len(p[3]), 1))(*p[3]) for p in plan]
    per = (rama_q8_seq_plan * n)(*[rama_q8_seq_plan(p[0], p[1], p[2], forced[i], len(p[3]), p[4], p[5]) for i, p in enumerate(plan)])
    check(L.rama_q8_decode_batch_begin(ctx, C.byref(e0.model.ccfg), C.byref(e0.model.weights), states, (C.c_int32 * n)(*toks),
                                       (C.c_int32 * n)(*poss), n, n_steps, per), "rama_q8_decode_batch_begin")
    check(L.rama_q8_decode_batch_steps(ctx, n_steps), "rama_q8_decode_batch_steps")
    if on_token is not None:
        import time
        seen, done = [0] * n, [False] * n
        buf = (C.c_int32 * 64)()
        k, fin = C.c_int(), C.c_int()
        ran = False                   # the stream has drained: one more sweep collects what is there
        while not all(done):
            progress = 0
            for s_ in range(n):
                if done[s_]:
                    continue
                # the finished word is read before the ring: once it is set, every token of the sequence is there
                check(L.rama_q8_decode_batch_stream_poll(ctx, s_, seen[s_], buf, 64, C.byref(k), C.byref(fin)), "rama_q8_decode_batch_stream_poll")
                for i in range(k.value):
                    on_token(s_, seen[s_] + i, int(buf[i]))
                seen[s_] += k.value
                progress += k.value
                done[s_] = bool(fin.value) and k.value < 64
            if progress or all(done):
                continue
            if ran:
                raise RuntimeError(f"decode_batch_chained: the steps have run but sequences {[i for i in range(n) if not done[i]]} have not finished")
            q = L.rama_stream_query(ctx)
            if q == 1:
                time.sleep(0.0002)
                continue
            check(q, "rama_stream_query")
            ran = True
    out = (C.c_int32 * (n * n_steps))()
    cnt = (C.c_int32 * n)()
    check(L.rama_q8_decode_batch_tokens(ctx, out, n_steps, cnt), "rama_q8_decode_batch_tokens")
    return [[int(out[s_ * n_steps + j]) for j in range(cnt[s_])] for s_ in range(n)]


# ------------------------------------------------------------------ the serving chain: continuous batching (rama_q8_serve_*)

SERVE_FREE, SERVE_PROMPT, SERVE_DECODE, SERVE_DONE = 0, 1, 2, 3


def serve_sizes(cfg, n_slots, max_rows, max_new_cap):
    """the checked sizes of a serving chain; ValueError for what rama_q8_serve_begin would refuse as a bad size.  No library call."""
    n_slots, max_new_cap = int(n_slots), int(max_new_cap)
    max_rows = n_slots if max_rows is None else int(max_rows)
    if not 1 <= n_slots <= MAX_BATCH:
        raise ValueError(f"Q8Server: {n_slots} slots, not 1..{MAX_BATCH}")
    if not n_slots <= max_rows <= MAX_BATCH:
        raise ValueError(f"Q8Server: max_rows {max_rows} outside [n_slots = {n_slots}, {MAX_BATCH}]")
    if not 1 <= max_new_cap <= cfg.seq_len - 1:
        raise ValueError(f"Q8Server: max_new_cap {max_new_cap} outside [1, seq_len - 1 = {cfg.seq_len - 1}]")
    return n_slots, max_rows, max_new_cap


def serve_plan(cfg, context, max_new, temperature=0.0, topp=0.9, u=TOPP_U_CPU, stop_token=None, max_new_cap=None, n_cached=0):
    """the checked arguments of Q8Server.submit: (context tokens, (temperature, topp, u, max_new, stop token)); ValueError for
    everything rama_q8_serve_admit / rama_q8_serve_admit_at would refuse in them.  No library call."""
    what = "Q8Server.submit"
    V, S = cfg.vocab_size, cfg.seq_len
    ctx = _tokens(context, V, what)
    if not ctx:
        raise ValueError(f"{what}: an empty context (the caller includes BOS)")
    if not 0 <= int(n_cached) <= len(ctx) - 1:
        raise ValueError(f"{what}: n_cached {int(n_cached)} outside [0, n_context - 1 = {len(ctx) - 1}] (the final context position is always fed)")
    T, P, U = float(temperature), float(topp), float(u)
    if not (T >= 0.0 and 0.0 <= P <= 1.0 and 0.0 <= U < 1.0):       # (false for NaN)
        raise ValueError(f"{what}: temperature >= 0, topp in [0, 1], u in [0, 1) -- not {T}, {P}, {U}")
    new = int(max_new)
    if new < 1:
        raise ValueError(f"{what}: max_new {new} < 1")
    if max_new_cap is not None and new > int(max_new_cap):
        raise ValueError(f"{what}: max_new {new} beyond the server's max_new_cap {int(max_new_cap)}")
    if len(ctx) + new > S:
        raise ValueError(f"{what}: {len(ctx)} context tokens + {new} new ones beyond seq_len {S}")
    stop = -1 if stop_token is None else int(stop_token)
    if not -1 <= stop < V:
        raise ValueError(f"{what}: stop token {stop} outside the vocabulary [0, {V})")
    if T != 0.0 and V > 32768:
        raise ValueError(f"{what}: a sampled plan needs vocab_size <= 32768")
    return ctx, (T, P, U, new, stop)


def serve_plan_step(slots, max_rows):
    """rama_q8_serve_plan_step, the scheduling rule as a pure host function: slots = (state, n_context, cursor, n_out, max_new)
    tuples -> (rows [(slot, pos, logits)] * max_rows, the slots after the step when no stop token is sampled).  No GPU."""
    from ._lib import load, rama_q8_serve_row, rama_q8_serve_slot
    n = len(slots)
    arr = (rama_q8_serve_slot * max(n, 1))(*[rama_q8_serve_slot(*[int(v) for v in s]) for s in slots])
    rows = (rama_q8_serve_row * max(int(max_rows), 1))()
    after = (rama_q8_serve_slot * max(n, 1))()
    check(load().rama_q8_serve_plan_step(arr, n, int(max_rows), rows, after), "rama_q8_serve_plan_step")
    return ([(r.slot, r.pos, r.logits) for r in rows[:int(max_rows)]],
            [(a.state, a.n_context, a.cursor, a.n_out, a.max_new) for a in after[:n]])


def common_prefix(a, b) -> int:
    """the number of leading tokens two sequences share"""
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


MAX_DRAFT, MAX_NGRAM = 15, 4


def serve_spec_sizes(n_draft, ngram, hint_cap):
    """the checked drafting sizes of a Q8Server; ValueError for what rama_q8_serve_begin_spec would refuse.  No library call."""
    n_draft, ngram, hint_cap = int(n_draft), int(ngram), int(hint_cap)
    if not 0 <= n_draft <= MAX_DRAFT:
        raise ValueError(f"Q8Server: n_draft {n_draft} outside [0, {MAX_DRAFT}]")
    if not 1 <= ngram <= MAX_NGRAM:
        raise ValueError(f"Q8Server: ngram {ngram} outside [1, {MAX_NGRAM}]")
    if hint_cap < 0 or (hint_cap and not n_draft):
        raise ValueError(f"Q8Server: hint_cap {hint_cap} (>= 0, and 0 on a server without drafts)")
    return n_draft, ngram, hint_cap


def serve_spec_request(cfg, n_draft_cap, ngram, hint_cap, n_draft=None, hint=None):
    """the checked drafting arguments of Q8Server.submit: (n_draft, ngram, hint tokens); ValueError for everything
    rama_q8_serve_admit_spec would refuse in them.  No library call."""
    what = "Q8Server.submit"
    K = n_draft_cap if n_draft is None else int(n_draft)
    if not 0 <= K <= n_draft_cap:
        raise ValueError(f"{what}: n_draft {K} outside [0, the server's n_draft = {n_draft_cap}]")
    toks = [] if hint is None else _tokens(hint, cfg.vocab_size, what + " hint")
    if len(toks) > hint_cap:
        raise ValueError(f"{what}: {len(toks)} hint tokens beyond the server's hint_cap {hint_cap}")
    return K, ngram, toks


def serve_spec_report(r) -> dict:
    """a rama_q8_serve_spec_report as a dict"""
    return dict(steps=int(r.steps), rows_decode=int(r.rows_decode), rows_draft=int(r.rows_draft), rows_prompt=int(r.rows_prompt),
                rows_idle=int(r.rows_idle), drafts_wanted=int(r.drafts_wanted), drafts_granted=int(r.drafts_granted),
                drafts_accepted=int(r.drafts_accepted), tokens_emitted=int(r.tokens_emitted), accepted_hist=[int(v) for v in r.accepted_hist],
                n_draft_cap=int(r.n_draft_cap), hint_cap=int(r.hint_cap), last_want=[int(v) for v in r.last_want[:r.n_slots]],
                last_granted=[int(v) for v in r.last_granted[:r.n_slots]])


def serve_spec_plan_step(slots, want, max_rows):
    """rama_q8_serve_spec_plan_step, the scheduling rule with drafts as a pure host function: slots = (state, n_context, cursor,
    n_out, max_new) tuples, want = the drafts every slot has for the step -> (rows [(slot, pos, logits)] * max_rows, the drafts
    granted per slot).  No GPU."""
    from ._lib import load, rama_q8_serve_row, rama_q8_serve_slot
    n = len(slots)
    if len(want) != n:
        raise ValueError(f"serve_spec_plan_step: {len(want)} want values for {n} slots")
    arr = (rama_q8_serve_slot * max(n, 1))(*[rama_q8_serve_slot(*[int(v) for v in s]) for s in slots])
    warr = (C.c_int32 * max(n, 1))(*[int(v) for v in want])
    rows = (rama_q8_serve_row * max(int(max_rows), 1))()
    granted = (C.c_int32 * max(n, 1))()
    check(load().rama_q8_serve_spec_plan_step(arr, n, int(max_rows), warr, rows, granted), "rama_q8_serve_spec_plan_step")
    return [(r.slot, r.pos, r.logits) for r in rows[:int(max_rows)]], [int(g) for g in granted[:n]]


def _spec_plan_py(slots, want, max_rows):
    """the scheduling rule with drafts, in Python: slots = [state, n_context, cursor, ...] -> (rows, granted)"""
    nrows = [1 if s[0] in (SERVE_PROMPT, SERVE_DECODE) else 0 for s in slots]
    left = max_rows - sum(nrows)
    for i, s in enumerate(slots):
        if s[0] == SERVE_PROMPT:
            extra = min(s[1] - s[2] - 1, left)
            nrows[i] += extra
            left -= extra
    granted = [0] * len(slots)
    for i, s in enumerate(slots):
        granted[i] = min(want[i], left) if s[0] == SERVE_DECODE else 0
        left -= granted[i]
    rows = []
    for i, s in enumerate(slots):
        for k in range(nrows[i] + granted[i]):
            rows.append((i, s[2] + k, 1 if s[0] == SERVE_DECODE or s[2] + k == s[1] - 1 else 0))
    return rows + [(-1, -1, 0)] * (max_rows - len(rows)), granted


def serve_spec_replay(requests, ref_tokens, n_slots, max_rows, use_slots=None):
    """a whole workload of a serving chain with drafts as a pure function of its inputs, no library call.  requests = dicts with
    context and max_new, and optionally stop_token, n_draft (0), ngram (3), hint and n_cached (0); ref_tokens[i] = the max_new
    tokens request i produces alone (Q8Engine.generate(context[1:], ...)[len(context) - 1:], not cut at the stop token).
    Admission: before every step the waiting requests, in order, take the slots of use_slots (default: all) that are FREE or
    DONE, in ascending slot index.  Every step is the draft rule per DECODE slot, the scheduling rule, and the accept rule by
    comparison with the reference tokens: row j's pick is ref[n_out + j] as long as the drafts before it were right, which is
    all the accept rule looks at.  -> dict(steps = one dict per step: admitted [(slot, request)], rows, want, granted, accepted
    {slot: a} for the DECODE slots, emitted {slot: n}, finished [slots]; counters = what rama_q8_serve_spec_stats reports;
    finish_step = per request the step it finishes in; slot = per request its slot; outputs = per request its tokens)."""
    reqs = []
    for r, ref in zip(requests, ref_tokens):
        ctx, new = [int(t) for t in r["context"]], int(r["max_new"])
        if len(ref) < new:
            raise ValueError(f"serve_spec_replay: {len(ref)} reference tokens for max_new {new}")
        stop = r.get("stop_token")
        reqs.append(dict(ctx=ctx, new=new, stop=-1 if stop is None else int(stop), K=int(r.get("n_draft", 0)), N=int(r.get("ngram", 3)),
                         hint=[int(t) for t in (r.get("hint") or [])], cached=int(r.get("n_cached", 0)), ref=[int(t) for t in ref]))
    usable = list(range(n_slots)) if use_slots is None else sorted(use_slots)
    slots = [[SERVE_FREE, 0, 0, 0, 0] for _ in range(n_slots)]      # state, n_context, cursor, n_out, max_new
    who, text = [None] * n_slots, [None] * n_slots
    waiting = list(range(len(reqs)))
    steps, finish, slot_of, outputs = [], [None] * len(reqs), [None] * len(reqs), [[] for _ in reqs]
    cnt = dict(steps=0, rows_decode=0, rows_draft=0, rows_prompt=0, rows_idle=0, drafts_wanted=0, drafts_granted=0, drafts_accepted=0,
               tokens_emitted=0, accepted_hist=[0] * 16)
    while waiting or any(s[0] in (SERVE_PROMPT, SERVE_DECODE) for s in slots):
        admitted = []
        for i in usable:
            if waiting and slots[i][0] in (SERVE_FREE, SERVE_DONE):
                q = waiting.pop(0)
                r = reqs[q]
                slots[i] = [SERVE_PROMPT, len(r["ctx"]), r["cached"], 0, r["new"]]
                who[i], text[i], slot_of[q] = q, list(r["ctx"]), i
                admitted.append((i, q))
        if not any(s[0] in (SERVE_PROMPT, SERVE_DECODE) for s in slots):
            raise ValueError("serve_spec_replay: requests are waiting but no slot can take them")
        want, drafts = [0] * n_slots, [[] for _ in range(n_slots)]
        for i, s in enumerate(slots):
            if s[0] == SERVE_DECODE and reqs[who[i]]["K"] > 0:
                r = reqs[who[i]]
                drafts[i] = _draft_py(r["hint"], text[i], r["K"], r["N"], s[4] - s[3] - 1)      # (n_context + max_new <= seq_len: the budget binds first)
                want[i] = len(drafts[i])
        rows, granted = _spec_plan_py(slots, want, max_rows)
        used = sum(1 for r in rows if r[0] >= 0)
        n_dec = sum(1 for s in slots if s[0] == SERVE_DECODE)
        cnt["steps"] += 1
        cnt["rows_decode"] += n_dec
        cnt["rows_draft"] += sum(granted)
        cnt["rows_prompt"] += used - n_dec - sum(granted)
        cnt["rows_idle"] += max_rows - used
        cnt["drafts_wanted"] += sum(want)
        accepted, emitted, finished = {}, {}, []
        for i, s in enumerate(slots):
            n = sum(1 for r in rows if r[0] == i)
            if n == 0:
                continue
            r = reqs[who[i]]
            if s[0] == SERVE_PROMPT and s[2] + n < s[1]:
                s[2] += n
                continue
            if s[0] == SERVE_PROMPT:
                picks, emit = r["ref"][:1], 1
                fin = s[4] <= 1 or picks[0] == r["stop"]
                s[2] = s[1]
            else:
                d, remaining = drafts[i][:granted[i]], s[4] - s[3]
                picks = r["ref"][s[3]:s[3] + len(d) + 1]
                a = 0
                while a < len(d) and picks[a] == d[a]:
                    a += 1
                emit = min(a + 1, remaining)
                fin = emit >= remaining
                for j in range(emit):
                    if picks[j] == r["stop"]:
                        emit, fin = j + 1, True
                        break
                accepted[i] = a
                cnt["drafts_granted"] += len(d)
                cnt["drafts_accepted"] += a
                cnt["accepted_hist"][a] += 1
                s[2] += emit
            emitted[i] = emit
            cnt["tokens_emitted"] += emit
            text[i] += picks[:emit]
            outputs[who[i]] += picks[:emit]
            s[3] += emit
            s[0] = SERVE_DONE if fin else SERVE_DECODE
            if fin:
                finished.append(i)
                finish[who[i]] = len(steps)
        steps.append(dict(admitted=admitted, rows=rows, want=want, granted=granted, accepted=accepted, emitted=emitted, finished=finished,
                          slots=[tuple(s) for s in slots]))
    return dict(steps=steps, counters=cnt, finish_step=finish, slot=slot_of, outputs=outputs)


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


class Q8Server:
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

    def __init__(self, model: Q8Model, n_slots: int, max_rows=None, max_new_cap: int = 256, prefix_cache: int = 0, n_draft: int = 0,
                 ngram: int = 3, hint_cap: int = 0):
        self.n_slots, self.max_rows, self.max_new_cap = serve_sizes(model.cfg, n_slots, max_rows, max_new_cap)
        self.n_draft, self.ngram, self.hint_cap = serve_spec_sizes(n_draft, ngram, hint_cap)
        self.spec = self.n_draft > 0                      # n_draft == 0: the plain chain, rama_q8_serve_begin
        self.pool = PrefixPool(prefix_cache)              # (raises before any library call)
        self.model, self.device, self.cfg = model, model.device, model.cfg
        L = self.device.lib
        if self.spec:
            check(L.rama_q8_serve_begin_spec(self.device.ctx, C.byref(model.ccfg), C.byref(model.weights), self.n_slots, self.max_rows,
                                             self.max_new_cap, self.n_draft, self.hint_cap), "rama_q8_serve_begin_spec")
        else:
            check(L.rama_q8_serve_begin(self.device.ctx, C.byref(model.ccfg), C.byref(model.weights), self.n_slots, self.max_rows,
                                        self.max_new_cap), "rama_q8_serve_begin")
        self._open = True
        self._own = [None] * self.n_slots                 # the server's own engine of a slot, made on first use and reused
        self._eng = [None] * self.n_slots                 # the engine the slot's occupant runs on
        self._spare = []                                  # the server's own engines that serve nobody: evicted donors
        self._mine = []                                   # every engine the server made (close frees them)
        self._cached = {}                                 # handle -> the n_cached it was admitted with
        self._drafts = {}                                 # handle -> (n_draft, ngram, hint tokens)
        self.rows_cached = 0                              # ... summed over the admissions
        self._req = [None] * self.n_slots                 # the handle a slot serves
        self._seen = [0] * self.n_slots
        self._mirror = [(SERVE_FREE, 0, 0, 0, 0)] * self.n_slots      # the host's copy of the slot table (exact unless a stop token fell)
        self._queue, self._results, self._finished, self._plans = [], {}, set(), {}
        self._next = 0
        self.planned = dict(steps=0, rows_decode=0, rows_prompt=0, rows_idle=0)      # the host plan's sums over the steps enqueued (none with drafts: no host plan)
        self.last_rows = []                               # ... and its row table of the last one

    # -- requests
    def submit(self, context, max_new, temperature=0.0, topp=0.9, u=TOPP_U_CPU, stop_token=None, engine=None, n_cached=0,
               retain=False, n_draft=None, hint=None):
        """queue a request -> its handle.  It is admitted at once if a slot is free, else when one finishes (step / run).
        engine: the Q8Engine whose run state the sequence uses (default: one the server owns for the slot).
        n_cached: rows 0..n_cached-1 of `engine` already hold context[0..n_cached) -- written by work enqueued earlier on the
        device's stream; the slot feeds the rest (at most n_context - 1: the final position is always fed).  Such a request is
        not matched against the prefix cache.
        retain: with a prefix cache, the engine stays behind as a donor when the request finishes (a caller's engine too: it
        is the pool's until it is evicted).
        n_draft, hint: on a server made with n_draft > 0, the drafts per step of this request (default: the server's; 0: none)
        and a token list to look up in besides the request's own text (at most hint_cap tokens).  The tokens are the same
        whatever they are."""
        ctx, plan = serve_plan(self.cfg, context, max_new, temperature, topp, u, stop_token, self.max_new_cap, n_cached)
        draft = serve_spec_request(self.cfg, self.n_draft, self.ngram, self.hint_cap, n_draft, hint)
        n_cached = int(n_cached)
        if n_cached and engine is None:
            raise ValueError("Q8Server.submit: n_cached needs the engine that holds the rows")
        if engine is not None and engine.model is not self.model:
            raise ValueError("Q8Server.submit: the engine belongs to another Q8Model")
        if engine is not None and any(e is engine for e in self._engines_in_use()):
            raise ValueError("Q8Server.submit: the engine already serves a queued or running request")
        if engine is not None and engine in self.pool:
            raise ValueError("Q8Server.submit: the engine is a donor of the prefix cache")
        h = self._next
        self._next += 1
        self._plans[h] = (ctx, plan, engine, n_cached, bool(retain))
        self._drafts[h] = draft
        self._results[h] = []
        self._queue.append(h)
        self._admit()
        return h

    def _engines_in_use(self):
        waiting = [self._plans[h][2] for h in self._queue]
        running = [self._eng[i] for i, h in enumerate(self._req) if h is not None]
        return [e for e in waiting + running if e is not None]

    def _admit(self):
        from ._lib import rama_q8_serve_plan
        L, ctx = self.device.lib, self.device.ctx
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
            if not n_cached and len(self.pool):
                # the donor stays in the pool whatever happens below: donors leave it in _collect only, so a fork that was
                # enqueued and an admission that then failed find it there at the next attempt; an evicted donor is reused or
                # freed behind the fork in stream order
                donor, n_cached = self.pool.match(toks, self.MIN_CACHED)
                if n_cached:
                    check(L.rama_q8_kv_fork(ctx, C.byref(self.model.ccfg), C.byref(donor.state), C.byref(eng.state), 1, n_cached),
                          "rama_q8_kv_fork")
            rec = rama_q8_serve_plan(T, P, U, new, stop)
            arr = (C.c_int32 * len(toks))(*toks)
            if self.spec:
                from ._lib import rama_q8_serve_spec
                K, N, hint = self._drafts[h]
                harr = (C.c_int32 * max(len(hint), 1))(*hint)
                srec = rama_q8_serve_spec(K, N, harr if hint else None, len(hint))
                check(L.rama_q8_serve_admit_spec(ctx, slot, C.byref(eng.state), arr, len(toks), n_cached, C.byref(rec), C.byref(srec)),
                      "rama_q8_serve_admit_spec")
            elif n_cached:
                check(L.rama_q8_serve_admit_at(ctx, slot, C.byref(eng.state), arr, len(toks), n_cached, C.byref(rec)), "rama_q8_serve_admit_at")
            else:
                check(L.rama_q8_serve_admit(ctx, slot, C.byref(eng.state), arr, len(toks), C.byref(rec)), "rama_q8_serve_admit")
            self._queue.pop(0)
            self._req[slot], self._seen[slot], self._eng[slot] = h, 0, eng
            self._cached[h] = n_cached
            self.rows_cached += n_cached
            self._mirror[slot] = (SERVE_PROMPT, len(toks), n_cached, 0, new)

    def _new_engine(self):
        e = Q8Engine(self.device, self.model)
        self._mine.append(e)
        return e

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

    def _collect(self, on_token=None):
        """what the rings hold: new tokens of every occupied slot; a finished occupant frees its slot"""
        L, ctx = self.device.lib, self.device.ctx
        buf = (C.c_int32 * 64)()
        k, fin = C.c_int(), C.c_int()
        early = False
        for slot in range(self.n_slots):
            h = self._req[slot]
            if h is None:
                continue
            while True:
                # the finished word is read before the ring: once it is set, every token of the occupant is there
                check(L.rama_q8_serve_poll(ctx, slot, self._seen[slot], buf, 64, C.byref(k), C.byref(fin), None), "rama_q8_serve_poll")
                for i in range(k.value):
                    if on_token is not None:
                        on_token(h, self._seen[slot] + i, int(buf[i]))
                    self._results[h].append(int(buf[i]))
                self._seen[slot] += k.value
                if k.value < 64:
                    break
            if fin.value:
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
            check(self.device.lib.rama_q8_serve_steps(self.device.ctx, n), "rama_q8_serve_steps")

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

    MIN_CACHED = 2     # a shorter match is not worth a launch: every context shares its first token (BOS) with every donor

    LOOKAHEAD = 2      # steps enqueued past a foreseen finish while requests wait: the admission then goes in behind running steps

    def run(self, on_token=None):
        """serve every submitted request to its end.  on_token(handle, index, token), when given, is fed from the host-visible
        rings.  The steps up to the next finish the host plan foresees -- and, while requests wait, LOOKAHEAD more, so that the
        device does not idle until the host has seen the finished word and admitted -- are enqueued at once; a DONE slot takes
        no rows, and an admission is stream-ordered behind them, so the host plan stays exact.  A stop token that ends a sequence
        earlier is seen at the next collection."""
        import time
        if self.spec:
            return self._run_spec(on_token)
        done_in = lambda t: {i for i in range(self.n_slots) if self._req[i] is not None and t[i][0] == SERVE_DONE}
        while True:
            if self._collect(on_token):
                self._resync()
            self._admit()
            expect = done_in(self._mirror)                # finished by the plan, not yet seen
            k = self._steps_to_next_finish()
            if k == 0 and not expect:
                if self._queue:
                    raise RuntimeError("Q8Server.run: requests are waiting but no slot can take them")
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
                q = self.device.lib.rama_stream_query(self.device.ctx)
                if q == 1:
                    time.sleep(0.0001)
                    continue
                check(q, "rama_stream_query")
                self._collect(on_token)
                if not all(self._req[i] is None for i in expect):
                    raise RuntimeError(f"Q8Server.run: the steps have run but slots {[i for i in expect if self._req[i] is not None]} have not finished")
                break

    SPEC_BLOCK = 4     # with drafts: at most this many steps between two looks at the device's slot table

    def _run_spec(self, on_token=None):
        """run() on a server with drafts.  A slot may finish earlier than the host plan foresees, so the plan -- one token per
        DECODE slot and step -- is an upper bound: the slot table is taken from the device before every block, the steps to the
        next finish by that plan -- SPEC_BLOCK at most -- are enqueued, and the finished words alone say who has finished.  A request that waits is
        admitted as soon as a finished word shows, behind the steps still in flight; the device never idles past a finish by
        more than the block enqueued."""
        import time
        while True:
            self._resync()                                # (synchronises: the block before has run)
            self._collect(on_token)
            self._admit()
            if all(h is None for h in self._req):
                if self._queue:
                    raise RuntimeError("Q8Server.run: requests are waiting but no slot can take them")
                return
            self._count_and_enqueue(max(min(self._steps_to_next_finish(), self.SPEC_BLOCK), 1))
            while True:
                self._collect(on_token)
                self._admit()
                q = self.device.lib.rama_stream_query(self.device.ctx)
                if q != 1:
                    check(q, "rama_stream_query")
                    break
                time.sleep(0.0001)

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
        """rama_q8_serve_stats (synchronises): the device's counters, the slot table, the last step's row table; rows_cached is the
        host's sum of n_cached over the admissions (context positions taken from cached rows instead of being fed)"""
        from ._lib import rama_q8_serve_report
        r = rama_q8_serve_report()
        check(self.device.lib.rama_q8_serve_stats(self.device.ctx, C.byref(r)), "rama_q8_serve_stats")
        spec = {}
        if self.spec:
            from ._lib import rama_q8_serve_spec_report
            q = rama_q8_serve_spec_report()
            check(self.device.lib.rama_q8_serve_spec_stats(self.device.ctx, C.byref(q)), "rama_q8_serve_spec_stats")
            spec = dict(spec=serve_spec_report(q))
        return dict(**spec, steps=int(r.steps), graph_captures=int(r.graph_captures), rows_decode=int(r.rows_decode), rows_prompt=int(r.rows_prompt),
                    rows_idle=int(r.rows_idle), rows_cached=self.rows_cached, n_slots=int(r.n_slots), max_rows=int(r.max_rows),
                    last_rows=[(x.slot, x.pos, x.logits) for x in r.last_rows[:r.max_rows]],
                    slots=[(s.state, s.n_context, s.cursor, s.n_out, s.max_new) for s in r.slots[:r.n_slots]],
                    generation=[int(g) for g in r.generation[:r.n_slots]])

    def close(self):
        if self._open:
            self._open = False
            check(self.device.lib.rama_q8_serve_end(self.device.ctx), "rama_q8_serve_end")
            self.pool.clear()                             # (a caller's engine that was a donor is the caller's again)
            for e in self._mine:
                e.free()
            self._mine, self._spare = [], []
            self._own, self._eng = [None] * self.n_slots, [None] * self.n_slots


# ------------------------------------------------------------------ the speculative chain: n-gram lookup drafts (rama_q8_spec_*)

def spec_plan(cfg, context, max_new, temperature=0.0, topp=0.9, u=TOPP_U_CPU, stop_token=None, n_draft=7, ngram=3, hint=None):
    """the checked arguments of Q8Engine.generate_spec: (context tokens, hint tokens, (temperature, topp, u, max_new, stop token,
    n_draft, ngram)); ValueError for everything rama_q8_spec_begin would refuse in them.  No library call."""
    what = "generate_spec"
    V, S = cfg.vocab_size, cfg.seq_len
    ctx = _tokens(context, V, what)
    if not ctx:
        raise ValueError(f"{what}: an empty context (the caller includes BOS)")
    hint_toks = [] if hint is None else _tokens(hint, V, what + " hint")
    T, P, U = float(temperature), float(topp), float(u)
    if not (T >= 0.0 and 0.0 <= P <= 1.0 and 0.0 <= U < 1.0):       # (false for NaN)
        raise ValueError(f"{what}: temperature >= 0, topp in [0, 1], u in [0, 1) -- not {T}, {P}, {U}")
    new, K, N = int(max_new), int(n_draft), int(ngram)
    if new < 1:
        raise ValueError(f"{what}: max_new {new} < 1")
    if len(ctx) + new > S:
        raise ValueError(f"{what}: {len(ctx)} context tokens + {new} new ones beyond seq_len {S}")
    if not 0 <= K <= MAX_DRAFT:
        raise ValueError(f"{what}: n_draft {K} outside [0, {MAX_DRAFT}]")
    if not 1 <= N <= MAX_NGRAM:
        raise ValueError(f"{what}: ngram {N} outside [1, {MAX_NGRAM}]")
    stop = -1 if stop_token is None else int(stop_token)
    if not -1 <= stop < V:
        raise ValueError(f"{what}: stop token {stop} outside the vocabulary [0, {V})")
    if T != 0.0 and V > 32768:
        raise ValueError(f"{what}: a sampled plan needs vocab_size <= 32768")
    return ctx, hint_toks, (T, P, U, new, stop, K, N)


def spec_report(r) -> dict:
    """a rama_q8_spec_report as a dict"""
    return dict(steps=int(r.steps), graph_captures=int(r.graph_captures), rows_fed=int(r.rows_fed), drafts=int(r.drafts),
                accepted=int(r.accepted), emitted=int(r.emitted), accepted_hist=[int(v) for v in r.accepted_hist],
                finished=int(r.finished), n_out=int(r.n_out), cursor=int(r.cursor))


def spec_draft(hint, seq, n_draft, ngram, room):
    """rama_q8_spec_draft, the drafting rule as a pure host function: the tokens that follow the latest occurrence of the last
    <= ngram tokens of seq -- in hint first, then in seq itself -- at most min(n_draft, room) of them.  No GPU."""
    from ._lib import load
    hint, seq = [int(t) for t in (hint or [])], [int(t) for t in seq]
    harr = (C.c_int32 * max(len(hint), 1))(*hint)
    sarr = (C.c_int32 * max(len(seq), 1))(*seq)
    out = (C.c_int32 * (MAX_DRAFT + 1))()
    n = load().rama_q8_spec_draft(harr if hint else None, len(hint), sarr, len(seq), int(n_draft), int(ngram), int(room), out)
    if n < 0:
        check(n, "rama_q8_spec_draft")
    return [int(out[i]) for i in range(n)]


def spec_accept(drafts, picks, stop_token, remaining):
    """rama_q8_spec_accept, the accept rule as a pure host function: picks = Device::sample of rows 0..len(drafts) ->
    (tokens emitted, finished).  No GPU."""
    from ._lib import load
    drafts, picks = [int(t) for t in drafts], [int(t) for t in picks]
    if len(picks) != len(drafts) + 1:
        raise ValueError(f"spec_accept: {len(picks)} picks for {len(drafts)} drafts, not one more")
    darr = (C.c_int32 * max(len(drafts), 1))(*drafts)
    parr = (C.c_int32 * len(picks))(*picks)
    fin = C.c_int()
    n = load().rama_q8_spec_accept(darr, len(drafts), parr, -1 if stop_token is None else int(stop_token), int(remaining), C.byref(fin))
    if n < 0:
        check(n, "rama_q8_spec_accept")
    return n, bool(fin.value)


def _draft_py(hint, seq, n_draft, ngram, room):
    cap = min(n_draft, room)
    if cap <= 0:
        return []
    L = len(seq)
    for n in range(min(ngram, L), 0, -1):
        tail = seq[L - n:]
        for text, hi in ((hint, len(hint)), (seq, L - 1)):          # an occurrence ends at e <= hi: in seq before L
            for e in range(hi, n - 1, -1):
                if text[e - n:e] == tail:
                    return text[e:e + cap]
    return []


def spec_replay(ref_tokens, context, hint, n_draft, ngram, max_new, stop_token):
    """the speculative chain's steps as a pure function of its inputs, no library call: ref_tokens = the max_new tokens the
    sequence produces alone (Q8Engine.generate(context[1:], ...)[len(context) - 1:], not cut at the stop token) -> one
    (n_d, a, emitted) per step up to the one that finishes the sequence.  Row j's pick is ref_tokens[emitted so far + j] as long
    as the drafts before it were right, which is all the accept rule looks at."""
    ref, s = [int(t) for t in ref_tokens], [int(t) for t in context]
    hint = [int(t) for t in (hint or [])]
    stop = -1 if stop_token is None else int(stop_token)
    if len(ref) < max_new:
        raise ValueError(f"spec_replay: {len(ref)} reference tokens for max_new {max_new}")
    out, e, fin = [], 0, False
    while not fin:
        remaining = max_new - e
        d = _draft_py(hint, s, n_draft, ngram, remaining - 1)
        picks = ref[e:e + len(d) + 1]
        a = 0
        while a < len(d) and picks[a] == d[a]:
            a += 1
        emit = min(a + 1, remaining)
        fin = emit >= remaining
        for j in range(emit):
            if picks[j] == stop:
                emit, fin = j + 1, True
                break
        s += picks[:emit]
        e += emit
        out.append((len(d), a, emit))
    return out
