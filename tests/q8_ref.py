"""numpy restatement of the Q8_0 forward (include/rama_hip.h) -- TEST INFRASTRUCTURE.

* quantize(): runq.c's activation rule -- scale = max|x| / 127 in fp32, q = C round(x / scale) with the division
  correctly rounded in fp32 and round-half-away-from-zero evaluated in float64, clamped to [-127, 127]; scale 0 -> 0.
* quantize_q80(): export.py's weight rule -- the same scale, torch.round (halves to even).
* matmul(): vectorised over rows, sequential over groups in np.float32: val = val + ((float)ival * ws) * xs.
* Q8Ref.forward(): infer.rs:8-53 composed from the oracle's per-op functions, every matmul replaced by the above.
* read_v2() / write_v2(): the llama2.c version-2 file (export.py version2_export) and its inverse.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import oracle as O

MAGIC = 0x616B3432
TENSORS = ("tok", "wq", "wk", "wv", "wo", "w1", "w2", "w3", "wcls")


def quantize(x, gs: int):
    x = np.ascontiguousarray(x, np.float32).reshape(-1, gs)
    wmax = np.abs(x).max(axis=1)
    scale = (wmax / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (x / scale[:, None]).astype(np.float32).astype(np.float64)
    q = np.sign(r) * np.floor(np.abs(r) + 0.5)
    q = np.where(scale[:, None] == 0, 0.0, np.clip(np.nan_to_num(q), -127, 127))
    return q.astype(np.int8).reshape(-1), scale


def quantize_q80(w, gs: int):
    """export.py quantize_q80: torch.round = halves to even (np.rint); scale 0 pinned to q = 0"""
    w = np.ascontiguousarray(w, np.float32).reshape(-1, gs)
    scale = (np.abs(w).max(axis=1) / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.rint((w / scale[:, None]).astype(np.float32))
    r = np.where(scale[:, None] == 0, 0.0, np.clip(np.nan_to_num(r), -127, 127))
    return r.astype(np.int8).reshape(-1), scale


def dequantize(q, s, gs: int):
    return (q.reshape(-1, gs).astype(np.float32) * s[:, None]).astype(np.float32).reshape(-1)


def matmul(xq, xs, wq, ws, gs: int):
    """o[i] for wq [d, n] int8 and ws [d, n / gs]"""
    d = ws.size * gs // xq.size
    n = xq.size
    G = n // gs
    W = wq.reshape(d, G, gs).astype(np.int32)
    X = xq.reshape(G, gs).astype(np.int32)
    ival = np.einsum("dgk,gk->dg", W, X).astype(np.float32)       # exact: |ival| < 2^24
    ws = ws.reshape(d, G)
    val = np.zeros(d, np.float32)
    for g in range(G):
        val = (val + ((ival[:, g] * ws[:, g]).astype(np.float32) * xs[g]).astype(np.float32)).astype(np.float32)
    return val


def read_v2(path):
    """-> (cfg dict, group_size, shared, norms dict, tensors dict name -> (int8 [n], fp32 scales), layers stacked); asserts the layout"""
    raw = np.fromfile(path, dtype=np.uint8)
    hdr = raw[:256].tobytes()
    magic, version = np.frombuffer(hdr[:8], "<u4")[0], np.frombuffer(hdr[4:8], "<i4")[0]
    assert magic == MAGIC and version == 2, (hex(magic), version)
    dim, hidden, L, H, KV, V, S = (int(v) for v in np.frombuffer(hdr[8:36], "<i4"))
    shared = bool(hdr[36])
    gs = int(np.frombuffer(hdr[37:41], "<i4")[0])
    assert not any(hdr[41:256])
    cfg = dict(dim=dim, hidden_dim=hidden, n_layers=L, n_heads=H, n_kv_heads=KV, vocab_size=V, seq_len=S, shared_weight=shared)
    off = 256
    norms = {}
    for name, n in (("rms_att_weight", L * dim), ("rms_ffn_weight", L * dim), ("rms_final_weight", dim)):
        norms[name] = np.frombuffer(raw[off:off + 4 * n].tobytes(), "<f4").copy()
        off += 4 * n
    sizes = dict(tok=V * dim, wq=L * dim * dim, wk=L * dim * dim, wv=L * dim * dim, wo=L * dim * dim, w1=L * hidden * dim,
                 w2=L * dim * hidden, w3=L * hidden * dim, wcls=V * dim)
    t = {}
    for name in TENSORS:
        if name == "wcls" and shared:
            t["wcls"] = t["tok"]
            continue
        parts = 1 if name in ("tok", "wcls") else L          # export.py quantizes (and writes) every layer's matrix on its own
        n = sizes[name] // parts
        qs, ss = [], []
        for _ in range(parts):
            qs.append(raw[off:off + n].view(np.int8).copy())
            off += n
            ss.append(np.frombuffer(raw[off:off + 4 * (n // gs)].tobytes(), "<f4").copy())
            off += 4 * (n // gs)
        t[name] = (np.concatenate(qs), np.concatenate(ss))
    assert off == raw.size, (off, raw.size)
    return cfg, gs, shared, norms, t


def write_v2(path, cfg: dict, gs: int, shared: bool, norms: dict, t: dict):
    """the inverse of read_v2: 256-byte header (magic, version, 7 ints, the shared-classifier byte at 36, the group size at 37, zeros),
    the fp32 norms, then every quantized tensor as int8 values followed by its scales -- per-layer tensors layer by layer, as
    export.py writes them -- and no wcls when the classifier is shared"""
    dim, hidden, L, V = cfg["dim"], cfg["hidden_dim"], cfg["n_layers"], cfg["vocab_size"]
    assert bool(cfg["shared_weight"]) == bool(shared) and dim % gs == 0 and hidden % gs == 0
    hdr = bytearray(256)
    hdr[0:4] = np.array([MAGIC], "<u4").tobytes()
    hdr[4:8] = np.array([2], "<i4").tobytes()
    hdr[8:36] = np.array([dim, hidden, L, cfg["n_heads"], cfg["n_kv_heads"], V, cfg["seq_len"]], "<i4").tobytes()
    hdr[36] = int(bool(shared))
    hdr[37:41] = np.array([gs], "<i4").tobytes()
    sizes = dict(tok=V * dim, wq=L * dim * dim, wk=L * dim * dim, wv=L * dim * dim, wo=L * dim * dim, w1=L * hidden * dim,
                 w2=L * dim * hidden, w3=L * hidden * dim, wcls=V * dim)
    with open(path, "wb") as f:
        f.write(bytes(hdr))
        for name, n in (("rms_att_weight", L * dim), ("rms_ffn_weight", L * dim), ("rms_final_weight", dim)):
            a = np.ascontiguousarray(norms[name], "<f4").reshape(-1)
            assert a.size == n, (name, a.size, n)
            f.write(a.tobytes())
        for name in TENSORS:
            if name == "wcls" and shared:
                continue
            q, s = t[name]
            q, s = np.ascontiguousarray(q, np.int8).reshape(-1), np.ascontiguousarray(s, "<f4").reshape(-1)
            assert q.size == sizes[name] and s.size * gs == q.size, (name, q.size, s.size)
            parts = 1 if name in ("tok", "wcls") else L
            n = q.size // parts
            for i in range(parts):
                f.write(q[i * n:(i + 1) * n].tobytes())
                f.write(s[i * (n // gs):(i + 1) * (n // gs)].tobytes())


def oracle_config(cfg: dict) -> O.Config:
    return O.Config(**cfg)


class Q8Ref:
    """the Q8 forward on the host.  t: name -> (int8 values, scales) with per-layer tensors stacked over layers; norms: the
    three fp32 gain tensors; rope: (freq_cis_real, freq_cis_imag) [seq_len, head_size / 2]"""

    def __init__(self, cfg: dict, gs: int, norms: dict, t: dict, rope):
        self.c = O.Config(**cfg)
        self.gs, self.t, self.norms = gs, t, {k: np.asarray(v, np.float32) for k, v in norms.items()}
        self.fr, self.fi = (np.ascontiguousarray(a, np.float32).reshape(self.c.seq_len, -1) for a in rope)
        self.emb = dequantize(*t["tok"], gs).reshape(self.c.vocab_size, self.c.dim)
        c = self.c
        kv = c.n_layers * c.seq_len * c.dim
        sizes = dict(x=c.dim, xb=c.dim, xb2=c.dim, hb=c.hidden_dim, hb2=c.hidden_dim, q=c.dim, k=c.dim, v=c.dim,
                     att=c.n_heads * c.seq_len, logits=c.vocab_size, key_cache=kv, value_cache=kv)
        self.s = {n: np.zeros(sizes[n], np.float32) for n in O._S_FIELDS}
        self._cs = O.OracleState(*[O._p(self.s[n]) for n in O._S_FIELDS])
        self._cc = c.c()

    # the two data-dependent ops as hooks: the host tests plant a fault in a subclass and show the comparison helpers see it
    quantize = staticmethod(quantize)
    rmsnorm = staticmethod(O.rmsnorm)

    def _mm(self, name, layer, xq, xs, rows, K):
        q, s = self.t[name]
        per, G = rows * K, rows * K // self.gs
        return matmul(xq, xs, q[layer * per:(layer + 1) * per], s[layer * G:(layer + 1) * G], self.gs)

    def forward(self, token: int, pos: int, rope_stop=None) -> np.ndarray:
        """rope_stop = l: return after layer l's RoPE with that layer's query and key in s["q"] / s["k"] and nothing of layer l
        appended to the caches (sink_caches_q8 builds layer l's keys for that query); None: the whole forward"""
        c, s, gs = self.c, self.s, self.gs
        d, h, hs = c.dim, c.hidden_dim, c.head_size
        x = s["x"]
        x[:] = self.emb[token]
        for l in range(c.n_layers):
            self.rmsnorm(s["xb"], x, np.ascontiguousarray(self.norms["rms_att_weight"][l * d:(l + 1) * d]), d)
            xq, xs = self.quantize(s["xb"], gs)
            s["q"][:] = self._mm("wq", l, xq, xs, d, d)
            s["k"][:] = self._mm("wk", l, xq, xs, d, d)
            s["v"][:] = self._mm("wv", l, xq, xs, d, d)
            for hh in range(c.n_heads):
                O.apply_position(s["q"][hh * hs:(hh + 1) * hs], s["k"][hh * hs:(hh + 1) * hs], self.fr[pos], self.fi[pos], hs)
            if rope_stop == l:
                return None
            base = (l * c.seq_len + pos) * d
            s["key_cache"][base:base + d] = s["k"]
            s["value_cache"][base:base + d] = s["v"]
            O.lib().oracle_multi_head_attention(C.byref(self._cc), C.byref(self._cs), l, pos)
            xq, xs = self.quantize(s["xb"], gs)
            s["xb2"][:] = self._mm("wo", l, xq, xs, d, d)
            O.array_add(x, s["xb2"], d)
            self.rmsnorm(s["xb"], x, np.ascontiguousarray(self.norms["rms_ffn_weight"][l * d:(l + 1) * d]), d)
            xq, xs = self.quantize(s["xb"], gs)
            s["hb"][:] = self._mm("w1", l, xq, xs, h, d)
            s["hb2"][:] = self._mm("w3", l, xq, xs, h, d)
            O.sinu(s["hb"], h)
            O.array_mult(s["hb"], s["hb2"], h)
            xq, xs = self.quantize(s["hb"], gs)
            s["xb"][:] = self._mm("w2", l, xq, xs, d, h)
            O.array_add(x, s["xb"], d)
        s["xb"][:] = x
        self.rmsnorm(x, s["xb"], self.norms["rms_final_weight"], d)
        xq, xs = self.quantize(x, gs)
        s["logits"][:] = self._mm("wcls", 0, xq, xs, c.vocab_size, d)
        return s["logits"]

    def cache_row(self, which: str, layer: int, pos: int) -> np.ndarray:
        d = self.c.dim
        base = (layer * self.c.seq_len + pos) * d
        return self.s[which][base:base + d]

    def generate(self, prompt, steps, temperature=0.0, topp=0.9, u=0.0):
        token, out = 1, []
        for pos in range(steps):
            lo = self.forward(token, pos)
            if pos < len(prompt):
                nxt = prompt[pos]
            elif temperature == 0.0:
                nxt = O.argmax(lo)
            else:
                nxt = O.sample(lo.copy(), temperature, topp, u)
            out.append(int(nxt))
            token = nxt
        return out


def synth_q8(cfg: dict, gs: int, seed: int, layers=None):
    """numpy twin of rama_q8_model_synth: oracle.synth.fill_numpy's fp32 weights quantized by quantize_q80.
    layers: restrict the per-layer tensors to these layer indices (a big shape's test needs only a few)."""
    from oracle import synth as S
    c = O.Config(**cfg)
    spec = S.synth_spec(c)
    L, d, h, V = c.n_layers, c.dim, c.hidden_dim, c.vocab_size
    norms = {n: S.fill_numpy(L * d if n != "rms_final_weight" else d, seed, *spec[n]) for n in ("rms_att_weight", "rms_ffn_weight", "rms_final_weight")}
    per = dict(wq=d * d, wk=d * d, wv=d * d, wo=d * d, w1=h * d, w2=d * h, w3=h * d)
    big = dict(tok="token_embedding_table", wcls="wcls")
    t = {}
    for name in TENSORS:
        if name == "wcls" and c.shared_weight:
            t["wcls"] = t["tok"]
            continue
        tag, scale, bias = spec[big.get(name, name)]
        if name in per:
            ls = range(L) if layers is None else layers
            parts = [quantize_q80(S.fill_numpy(per[name], seed, tag, scale, bias, offset=l * per[name]), gs) for l in ls]
            t[name] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        else:
            t[name] = quantize_q80(S.fill_numpy(V * d, seed, tag, scale, bias), gs)
    return norms, t
