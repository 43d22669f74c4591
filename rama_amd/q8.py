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
