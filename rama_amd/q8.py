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
