"""Q8_0 models over the C ABI: llama2.c version-2 checkpoints (rama_q8_model_load) and synthetic Q8 models
(rama_q8_model_synth), decoded by the Q8 forward (runq.c's quantized products, rama's exact ops elsewhere;
include/rama_hip.h).  The fp32 Model / Engine are untouched.  No CPU fallback anywhere."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._host import (MAX_BATCH, MAX_DRAFT, MAX_NGRAM, _check_batch, _check_budget, _check_context, _check_drafting,  # noqa: F401  (the caps: re-exported)
                    _check_sampled_vocab, _check_sampler, _check_stop, _drain, _i32, _per_seq, _report, _ring_poll, _stream_busy, _tokens)
from ._lib import (Q8_TENSORS, check, load, rama_config, rama_q8_seq_plan, rama_q8_spec_model_report, rama_q8_spec_plan, rama_q8_spec_report,
                   rama_q8_spec_tree_report,
                   rama_q8_weights, rama_run_state)
from .q8_replay import (SERVE_DECODE, SERVE_DONE, SERVE_FREE, SERVE_PROMPT,  # noqa: F401  (the restatements: re-exported)
                        _accept_py, _draft_py, _spec_plan_py, serve_model_replay, serve_spec_replay, spec_model_replay, spec_model_tree_replay, spec_replay,
                        spec_tree_replay)
from .sampler_const import TOPP_U_CPU
from .serve import (PrefixPool, ServeLoop, common_prefix, serve_model_plan_step, serve_model_report, serve_model_sizes,  # noqa: F401  (the serving loop: re-exported)
                    serve_plan, serve_plan_step, serve_sizes, serve_spec_plan_step, serve_spec_report, serve_spec_request, serve_spec_sizes)
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

    @staticmethod
    def from_model(model, group_size: int = 64) -> "Q8Model":
        """a resident fp32 Model (loaded, synthetic, any whole weight set) quantized in HBM by export.py's quantize_q80 rule
        (rama_q8_model_from_f32): the Q8Model that load() gives from the version-2 file export.py writes for those weights.  The
        group size is halved until it fits, as version2_export does (from_f32_group_size); the source model is only read."""
        gs = from_f32_group_size(model.cfg, group_size)
        h = C.c_void_p()
        check(model.device.lib.rama_q8_model_from_f32(model.device.ctx, C.byref(model.ccfg), C.byref(model.weights), gs, C.byref(h)),
              "rama_q8_model_from_f32")
        return Q8Model(model.device, h)

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


def from_f32_group_size(cfg, group_size: int = 64) -> int:
    """the group size Q8Model.from_model quantizes with: version2_export's back-off -- halve the wanted size while it does not
    divide dim -- carried on while it does not divide hidden_dim either, which the Q8 products need as well (every row of W2 is
    whole groups).  ValueError for a size below 1.  No library call."""
    gs = int(group_size)
    if gs < 1:
        raise ValueError(f"from_model: group_size {gs} < 1")
    while gs > 1 and (cfg.dim % gs or cfg.hidden_dim % gs):
        gs //= 2
    return gs


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
                      hint=None, on_token=None, draft=None, n_branch=None, tree_rows=None):
        """speculative decode (rama_q8_spec_begin / _steps / _poll): context = the tokens fed at positions
        0..n-1 (the caller includes BOS) -> the up to max_new sampled tokens, those generate(context[1:], n - 1 + max_new,
        ...)[n-1:] gives, cut after stop_token.  Up to n_draft tokens per step are guessed by looking the last <= ngram
        tokens up in `hint` (a token list, optional) and in the sequence itself, and verified in one weight pass.
        context[:-1] is prefilled here; on_token(index, token), when given, is fed from the host-visible ring while the steps
        run.  The report of the run stays behind as self.spec_stats.
        draft = a Q8Engine over a small model with the same vocabulary, on the same device (rama_q8_spec_begin_model, DESIGN.md
        8.9): the guesses are that model's own next tokens under the same sampler instead of the lookup -- 1 <= n_draft, no hint,
        ngram ignored; context[:-1] is prefilled on both engines, and spec_stats also has rama_q8_spec_model_stats' fields.
        n_branch = B in 1..4 (with tree_rows = R in 2..16, default 16): tree drafts (rama_q8_spec_begin_tree) --
        the continuations of the B latest occurrences share one pass of R rows; 1 <= n_draft, no draft model; spec_stats also
        has rama_q8_spec_tree_stats' fields.  The default (None) stays the linear chain.
        draft together with n_branch / tree_rows: the tree is the draft model's (rama_q8_spec_begin_model_tree) -- its
        first choice below every node, its next B - 1 choices below the trunk's; spec_stats carries all three reports."""
        ctx_toks, hint_toks, (T, P, U, new, stop, K, N) = spec_plan(self.cfg, context, max_new, temperature, topp, u, stop_token,
                                                                    n_draft, ngram, hint)
        if draft is not None:
            spec_model_check(self, draft, len(ctx_toks), new, K, hint_toks)
        tree = n_branch is not None or tree_rows is not None
        if tree and draft is not None:
            B, R = spec_model_tree_check(self.cfg, K, 1 if n_branch is None else n_branch, 16 if tree_rows is None else tree_rows)
        elif tree:
            B, R = spec_tree_check(draft, K, 1 if n_branch is None else n_branch, 16 if tree_rows is None else tree_rows)
        L, ctx = self.device.lib, self.device.ctx
        if len(ctx_toks) > 1:
            self.prefill(ctx_toks[:-1])
            if draft is not None:
                draft.prefill(ctx_toks[:-1])
        harr = _i32(hint_toks)
        rec = rama_q8_spec_plan(T, P, U, new, stop, K, N, harr if hint_toks else None, len(hint_toks))
        head = (ctx, C.byref(self.model.ccfg), C.byref(self.model.weights), C.byref(self.state))
        if tree and draft is not None:
            check(L.rama_q8_spec_begin_model_tree(*head, C.byref(draft.model.ccfg), C.byref(draft.model.weights), C.byref(draft.state),
                                                  _i32(ctx_toks), len(ctx_toks), C.byref(rec), B, R), "rama_q8_spec_begin_model_tree")
        elif tree:
            check(L.rama_q8_spec_begin_tree(*head, _i32(ctx_toks), len(ctx_toks), C.byref(rec), B, R), "rama_q8_spec_begin_tree")
        elif draft is None:
            check(L.rama_q8_spec_begin(*head, _i32(ctx_toks), len(ctx_toks), C.byref(rec)), "rama_q8_spec_begin")
        else:
            check(L.rama_q8_spec_begin_model(*head, C.byref(draft.model.ccfg), C.byref(draft.model.weights), C.byref(draft.state),
                                             _i32(ctx_toks), len(ctx_toks), C.byref(rec)), "rama_q8_spec_begin_model")
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
        if draft is not None:
            q = rama_q8_spec_model_report()
            check(L.rama_q8_spec_model_stats(ctx, C.byref(q)), "rama_q8_spec_model_stats")
            self.spec_stats.update(_report(q))
        if tree:
            q = rama_q8_spec_tree_report()
            check(L.rama_q8_spec_tree_stats(ctx, C.byref(q)), "rama_q8_spec_tree_stats")
            self.spec_stats.update(_report(q))
        check(L.rama_q8_spec_end(ctx), "rama_q8_spec_end")
        return out

    def tree_forward(self, tokens, parent, pos0: int) -> np.ndarray:
        """an eager pass over a tree of up to 16 rows (rama_q8_tree_forward): row j carries tokens[j] below row parent[j]
        (parent[0] = -1, parent[j] < j), the root at position pos0 -> the logits [len(tokens), vocab_size], each row's those of
        forward() after the prefix and the row's path.  Only the root's cache row is written."""
        toks = _tokens(tokens, self.cfg.vocab_size, "tree_forward")
        par = [int(p) for p in parent]
        if len(par) != len(toks):
            raise ValueError(f"tree_forward: {len(par)} parents for {len(toks)} tokens")
        n, V = len(toks), self.cfg.vocab_size
        L, ctx = self.device.lib, self.device.ctx
        buf = C.c_void_p()
        check(L.rama_alloc_f32(ctx, max(n, 1) * V, C.byref(buf)), "rama_alloc_f32")
        try:
            check(L.rama_q8_tree_forward(ctx, C.byref(self.model.ccfg), C.byref(self.model.weights), C.byref(self.state), _i32(toks), _i32(par),
                                         n, int(pos0), buf), "rama_q8_tree_forward")
            out = np.empty((n, V), dtype=np.float32)
            check(L.rama_download_f32(ctx, buf, n * V, out.ctypes.data))
        finally:
            check(L.rama_free(ctx, buf))
        return out

    def tree_commit(self, path, pos0: int):
        """the rows of a root-to-node path of the last tree_forward into cache positions pos0 + 1 .. (rama_q8_tree_commit)"""
        path = [int(p) for p in path]
        check(self.device.lib.rama_q8_tree_commit(self.device.ctx, C.byref(self.model.ccfg), C.byref(self.state), _i32(path), len(path), int(pos0)),
              "rama_q8_tree_commit")

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
    Ts, Ps, Us, news, stops = (_per_seq(x, n, f"{what}: {{}} {k} values") for x, k in ((temperature, "temperature"), (topp, "topp"), (u, "u"),
                                                                                       (max_new, "max_new"), (stop_tokens, "stop_tokens")))
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


class Q8Server(ServeLoop):
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
    weight pass.  The tokens are the same with drafts on and off; n_draft=0 (the default) is the plain chain.

    Model drafts.  draft=Q8Model (a small model over the same vocabulary, on the same device) with n_draft=K in
    1..15 begins the chain with rama_q8_serve_begin_model: the guesses are that model's own next tokens under the request's sampler
    instead of the lookup -- no hint_cap, ngram ignored, at most 64 slots.  The server owns one draft engine per slot and prefills
    it with the request's context before the admission.  The tokens are the same with and without the draft model."""

    ABI = "rama_q8_serve"
    NAME = "Q8Server"

    def __init__(self, model: Q8Model, n_slots: int, max_rows=None, max_new_cap: int = 256, prefix_cache: int = 0, n_draft: int = 0,
                 ngram: int = 3, hint_cap: int = 0, draft: Q8Model = None, preempt: bool = False):
        if draft is not None and draft.device is not model.device:
            raise ValueError("Q8Server: the draft model is on another device context")
        super().__init__(model, n_slots, max_rows, max_new_cap, prefix_cache, n_draft, ngram, hint_cap, draft, preempt)

    def _new_engine(self, model=None):
        return Q8Engine(self.device, model or self.model)


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


def spec_model_check(engine, draft, n_context, max_new, n_draft, hint_toks):
    """ValueError for what rama_q8_spec_begin_model would refuse in a draft engine and can be seen from here.  No library call."""
    what = "generate_spec"
    if draft is engine or draft.state.key_cache == engine.state.key_cache:
        raise ValueError(f"{what}: the draft engine is the target's own")
    if draft.device is not engine.device:
        raise ValueError(f"{what}: the draft engine is on another device context")
    if hint_toks:
        raise ValueError(f"{what}: a hint together with a draft model -- model drafts replace the lookup")
    if draft.cfg.vocab_size != engine.cfg.vocab_size:
        raise ValueError(f"{what}: the draft model's vocabulary {draft.cfg.vocab_size} is not the target's {engine.cfg.vocab_size}")
    if n_context + max_new > draft.cfg.seq_len:
        raise ValueError(f"{what}: n_context {n_context} + max_new {max_new} beyond the draft model's seq_len {draft.cfg.seq_len}")
    if n_draft < 1:
        raise ValueError(f"{what}: n_draft {n_draft} < 1 with a draft model")


def spec_tree_check(draft, n_draft, n_branch, tree_rows):
    """ValueError for what rama_q8_spec_begin_tree would refuse in its own arguments -> (n_branch, n_rows).  No library call."""
    what = "generate_spec"
    B, R = int(n_branch), int(tree_rows)
    if draft is not None:
        raise ValueError(f"{what}: tree drafts together with a draft model")
    if not 1 <= B <= 4:
        raise ValueError(f"{what}: n_branch {B} outside 1..4")
    if not 2 <= R <= 16:
        raise ValueError(f"{what}: tree_rows {R} outside 2..16")
    if n_draft < 1:
        raise ValueError(f"{what}: n_draft {n_draft} < 1 with tree drafts")
    return B, R


def spec_model_tree_check(cfg, n_draft, n_branch, tree_rows):
    """ValueError for what rama_q8_spec_begin_model_tree would refuse in its own arguments, beyond spec_model_check's -> (n_branch,
    n_rows).  No library call."""
    what = "generate_spec"
    B, R = int(n_branch), int(tree_rows)
    if not 1 <= B <= 4:
        raise ValueError(f"{what}: n_branch {B} outside 1..4")
    if not 2 <= R <= 16:
        raise ValueError(f"{what}: tree_rows {R} outside 2..16")
    if B > cfg.vocab_size:
        raise ValueError(f"{what}: n_branch {B} beyond the vocabulary {cfg.vocab_size}")
    if n_draft < 1:
        raise ValueError(f"{what}: n_draft {n_draft} < 1 with a draft model")
    return B, R


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


def spec_tree_draft(hint, seq, n_draft, ngram, room, n_branch, n_rows):
    """rama_q8_spec_tree_draft, the tree drafting rule as a pure host function -> (tok, parent, depth) of nodes 1..m.  No GPU."""
    hint, seq = [int(t) for t in (hint or [])], [int(t) for t in seq]
    tok, par, dep = ((C.c_int32 * 16)() for _ in range(3))
    m = load().rama_q8_spec_tree_draft(_i32(hint) if hint else None, len(hint), _i32(seq), len(seq), int(n_draft), int(ngram), int(room),
                                       int(n_branch), int(n_rows), tok, par, dep)
    if m < 0:
        check(m, "rama_q8_spec_tree_draft")
    return tok[:m], par[:m], dep[:m]


def spec_tree_accept(tok, parent, picks, stop_token, remaining):
    """rama_q8_spec_tree_accept, the tree accept rule as a pure host function: tok / parent of nodes 1..m, picks of rows 0..m ->
    (path, tokens emitted, finished).  No GPU."""
    tok, parent, picks = [int(t) for t in tok], [int(t) for t in parent], [int(t) for t in picks]
    if len(parent) != len(tok) or len(picks) != len(tok) + 1:
        raise ValueError(f"spec_tree_accept: {len(tok)} tokens, {len(parent)} parents, {len(picks)} picks")
    path, a, fin = (C.c_int32 * 16)(), C.c_int(), C.c_int()
    n = load().rama_q8_spec_tree_accept(_i32(tok) if tok else None, _i32(parent) if parent else None, len(tok), _i32(picks),
                                        -1 if stop_token is None else int(stop_token), int(remaining), path, C.byref(a), C.byref(fin))
    if n < 0:
        check(n, "rama_q8_spec_tree_accept")
    return path[:a.value + 1], n, bool(fin.value)



def spec_model_tree_shape(cap, n_branch, n_rows):
    """rama_q8_spec_model_tree_shape, the static shape of a draft model's tree as a pure host function -> (parent, depth, rank) of
    nodes 1..m.  No GPU."""
    par, dep, rank = ((C.c_int32 * 16)() for _ in range(3))
    m = load().rama_q8_spec_model_tree_shape(int(cap), int(n_branch), int(n_rows), par, dep, rank)
    if m < 0:
        check(m, "rama_q8_spec_model_tree_shape")
    return par[:m], dep[:m], rank[:m]


def spec_model_tree_candidates(logits, rank0_token, n):
    """rama_q8_spec_model_tree_candidates, the tokens of ranks 1..n of a logits row as a pure host function: descending by (logit
    bits mapped to unsigned, token index), rank 0's token dropped.  No GPU."""
    row = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    out = (C.c_int32 * 4)()
    k = load().rama_q8_spec_model_tree_candidates(row.ctypes.data_as(C.POINTER(C.c_float)), int(row.size), int(rank0_token), int(n), out)
    if k < 0:
        check(k, "rama_q8_spec_model_tree_candidates")
    return out[:k]


def spec_model_tree_last(device):
    """rama_q8_spec_model_tree_last: the last step's tree as the device built it -> dict(tok, parent, depth, picks of nodes 0..m,
    path = the accepted rows, m, a).  Synchronises."""
    tok, par, dep, picks, path = ((C.c_int32 * 16)() for _ in range(5))
    m, a = C.c_int(), C.c_int()
    check(device.lib.rama_q8_spec_model_tree_last(device.ctx, tok, par, dep, picks, path, C.byref(m), C.byref(a)), "rama_q8_spec_model_tree_last")
    n = m.value + 1
    return dict(tok=tok[:n], parent=par[:n], depth=dep[:n], picks=picks[:n], path=path[:a.value + 1], m=m.value, a=a.value)
