"""Weights, rows and caches shaped like a trained Llama's, for the tests that judge the kernels on harsh data.

Everything else in the suite feeds the kernels oracle/synth.py's mild matrices (std 0.02, gains 1 +- 0.05) or standard-normal caches.
On that data the exact-order kernels always take their fast branch and fast mode's errors stay far below any fixed bar.  Trained
models are different, and exactly where the kernels branch on the data:

  * massive activations: a few residual channels 10^2 .. 10^4 times the median.  The sum of squares is one huge term and a tail of
    terms near half an ulp of the running sum -- every group of eight a tie group for seqsum_fast.hpp, whose walk list then overflows;
  * attention sinks: one position takes almost all the weight, the rest have exp(s - max) near 2^-24.  The exact softmax sum then
    sits within 2^-13 of a binade edge (seq_sum_predict gives up), and fast mode's split-T combine sees per-split maxima tens apart.

This module builds such data from a seed (nothing is read from disk): two weight kinds (`massive`, `sink`), embedding rows with a
designed property (DESIGNATED), sink caches for a given query, a llama2.c v0 checkpoint writer, and the comparator that judges the
non-parity modes against the float64 forward (`f64_bound`).
"""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O
from oracle import synth as S

KINDS = ("massive", "sink")

# the designated embedding rows: token ids of the rows with a constructed property
TOK_ZERO, TOK_TIE, TOK_SUBNORMAL, TOK_LARGE = 2, 3, 4, 5
DESIGNATED = (TOK_ZERO, TOK_TIE, TOK_SUBNORMAL, TOK_LARGE)

FS_CAP = 1024         # seqsum_fast.hpp kFsCap: items the leader's walk list holds
FS_GROUP = 8          # terms per group of seqsum_fast.hpp


# ------------------------------------------------------------------ checkpoint

def write_checkpoint(path, cfg: O.Config, w: dict):
    """llama2.c v0 .bin: 7 x i32 header (the sign of vocab_size is the shared-classifier flag: > 0 shared), then every tensor of
    O.weight_shapes in order, fp32 little endian.  A shared model writes no wcls."""
    vocab = cfg.vocab_size if cfg.shared_weight else -cfg.vocab_size
    hdr = np.array([cfg.dim, cfg.hidden_dim, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, vocab, cfg.seq_len], dtype="<i4")
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        for name, shp in O.weight_shapes(cfg):
            a = np.ascontiguousarray(w[name], dtype="<f4")
            assert a.shape == tuple(shp), (name, a.shape, shp)
            f.write(a.tobytes())


# ------------------------------------------------------------------ weights

def massive_channels(dim: int):
    """channel 0, the first channel of a 16-column block in the middle, the last channel"""
    return (0, 16 * (dim // 32), dim - 1)


def _student_t(rng, shape, std):
    """Student-t with 4 degrees of freedom scaled to `std`: z / sqrt(chi2_4 / 4), chi2_4 / 4 = Gamma(2) / 2 = (E1 + E2) / 2 (float32
    throughout: the 7B-width tensors are 400 M values)"""
    z = rng.standard_normal(shape, dtype=np.float32)
    g = rng.standard_exponential(shape, dtype=np.float32)
    g += rng.standard_exponential(shape, dtype=np.float32)
    g *= np.float32(0.5)
    np.sqrt(g, out=g)
    z /= g
    z *= np.float32(std / math.sqrt(2.0))          # t_4 has variance 2
    return z


def tie_row(dim: int) -> np.ndarray:
    """[64, 2^-6, 2^-6, ...]: squares 4096 and 2^-12, every add of a tail term a tie to even at the running sum 4096 -- the
    sequential fp32 sum stays 4096.0 while the exact one grows by (dim - 1) 2^-12"""
    x = np.full(dim, 2.0 ** -6, np.float32)
    x[0] = 64.0
    return x


def subnormal_row(dim: int, rng) -> np.ndarray:
    """magnitudes 2^-74 .. 2^-70 with random signs: every square and the whole sum of squares (dim <= 4096) are subnormal"""
    e = rng.integers(-74, -71, dim, endpoint=True)
    m = 1.0 + rng.integers(0, 8, dim) / 8.0
    return (np.where(rng.random(dim) < 0.5, -1.0, 1.0) * m * np.exp2(e)).astype(np.float32)


def large_row(dim: int, rng) -> np.ndarray:
    """|x| in [1e16, 2e17]: squares near 1e34 whose sum stays finite (< 2^127) at dim 4096"""
    return (np.where(rng.random(dim) < 0.5, -1.0, 1.0) * rng.uniform(1e16, 2e17, dim)).astype(np.float32)


def designated_rows(dim: int, seed: int = 0) -> dict:
    rng = np.random.default_rng(1000 + seed)
    return {TOK_ZERO: np.zeros(dim, np.float32), TOK_TIE: tie_row(dim), TOK_SUBNORMAL: subnormal_row(dim, rng),
            TOK_LARGE: large_row(dim, rng)}


def _gains(rng, shape, dim, small):
    """lognormal gains (median 1), small gains on the massive channels, a few near 0, a few of 10..30"""
    g = rng.lognormal(0.0, 0.6, shape).astype(np.float32)
    g2 = g.reshape(-1, dim)
    for r in g2:
        r[list(small)] = rng.uniform(0.01, 0.05, len(small))
        idx = rng.choice([i for i in range(dim) if i not in small], 6, replace=False)
        r[idx[:3]] = rng.uniform(1e-4, 1e-3, 3)
        r[idx[3:]] = rng.uniform(10.0, 30.0, 3)
    return g


def trained_like_weights(cfg: O.Config, kind: str, seed: int) -> dict:
    """The dict of S.synth_weights (rope tables included; wcls aliases the embedding table when shared), shaped like a trained model.

    massive: Student-t matrices (4 degrees of freedom, std 0.02; wo / w3 0.02 / sqrt(2 L) as in synth), the massive channels 400 / 1500 / 3000 times
             the others in every embedding row and re-injected by the matching output rows of wo and w2 (x 300), lognormal gains, a
             few input columns of wq / wk / w1 / w3 x 20, a few classifier rows x 10 (peaked logits);
    sink:    the same matrices without the massive channels, wq / wk scaled so that |scores| reach 30 .. 100 at head size 128, head 0's
             wq rows zero (all scores 0: a uniform softmax of exp = 1.0 terms), head 1's wq rows x 1e-3 (a nearly flat softmax).
    Both kinds carry the DESIGNATED rows in the embedding table."""
    assert kind in KINDS, kind
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    L, d, h, V, hs = cfg.n_layers, cfg.dim, cfg.hidden_dim, cfg.vocab_size, cfg.head_size
    res = 0.02 / math.sqrt(2.0 * L)
    w = {}
    w["token_embedding_table"] = _student_t(rng, (V, d), 0.02)
    w["wq"] = _student_t(rng, (L, d, d), 0.02)
    w["wk"] = _student_t(rng, (L, d, d), 0.02)
    w["wv"] = _student_t(rng, (L, d, d), 0.02)
    w["wo"] = _student_t(rng, (L, d, d), res)
    w["w1"] = _student_t(rng, (L, h, d), 0.02)
    w["w2"] = _student_t(rng, (L, d, h), 0.02)
    w["w3"] = _student_t(rng, (L, h, d), res)
    if not cfg.shared_weight:
        w["wcls"] = _student_t(rng, (V, d), 0.02)
    mc = massive_channels(d) if kind == "massive" else ()
    w["rms_att_weight"] = _gains(rng, (L, d), d, mc)
    w["rms_ffn_weight"] = _gains(rng, (L, d), d, mc)
    w["rms_final_weight"] = _gains(rng, (d,), d, mc)
    if kind == "massive":
        emb = w["token_embedding_table"]
        med = float(np.median(np.abs(emb)))
        for c, mult in zip(mc, (400.0, 1500.0, 3000.0)):
            emb[:, c] = (np.where(rng.random(V) < 0.5, -1.0, 1.0) * mult * med * rng.uniform(0.8, 1.2, V)).astype(np.float32)
        w["wo"][:, list(mc), :] *= np.float32(300.0)
        w["w2"][:, list(mc), :] *= np.float32(300.0)
        for name in ("wq", "wk", "w1", "w3"):
            cols = rng.choice(d, 3, replace=False)
            w[name][:, :, cols] *= np.float32(20.0)
        if not cfg.shared_weight:
            rows = rng.choice([r for r in range(V) if r not in DESIGNATED], 3, replace=False)
            w["wcls"][rows] *= np.float32(10.0)
    else:
        # xb has rms ~1, so q_i, k_i ~ s sqrt(d) and a score ~ s^2 d: s^2 d = 6 puts the largest |scores| of a head at 30 .. 100
        s = math.sqrt(6.0 / d) / 0.02
        w["wq"] *= np.float32(s)
        w["wk"] *= np.float32(s)
        w["wq"][:, 0:hs, :] = 0.0                          # head 0: dead
        if cfg.n_heads > 2:
            w["wq"][:, hs:2 * hs, :] *= np.float32(1e-3)   # head 1: nearly flat
    for tok, row in designated_rows(d, seed).items():
        w["token_embedding_table"][tok] = row
    fr, fi = S.rope_tables(cfg.seq_len, hs)
    w["freq_cis_real"], w["freq_cis_imag"] = fr, fi
    if cfg.shared_weight:
        w["wcls"] = w["token_embedding_table"]
    return w


# ------------------------------------------------------------------ sink caches

LN2 = math.log(2.0)
SINK_GAP = 30.0                                 # the sink's score above the keys that are not in the tail
TAIL_LO, TAIL_HI = 24.0 * LN2, 25.0 * LN2      # the tail's score offsets: exp lands in [2^-25, 2^-24]


def sink_cache_layer(q: np.ndarray, self_k: np.ndarray, n_heads: int, pos: int, sink_at: int, rng, tail_every: int = 1):
    """key and value rows [pos, dim] of one layer for the query q (post-RoPE) at position pos: per head one key along q at a score
    SINK_GAP above the highest other score (the row that pos itself appends, self_k, included), a tail of keys at score offsets
    -TAIL_LO .. -TAIL_HI (exp(s - max) in [2^-25, 2^-24]), every other key SINK_GAP below.  Heads whose query is zero (a dead head)
    keep random keys.  Positions < pos are written; pos is the one forward() appends."""
    dim = q.size
    hs = dim // n_heads
    k = (rng.standard_normal((pos, dim)) * 0.05).astype(np.float64)
    v = rng.standard_normal((pos, dim)).astype(np.float32)
    tail = np.zeros(pos, bool)
    tail[::tail_every] = True
    if 0 <= sink_at < pos:
        tail[sink_at] = False
    for hh in range(n_heads):
        qh = q[hh * hs:(hh + 1) * hs].astype(np.float64)
        nq = float(np.dot(qh, qh))
        if nq < 1e-20:
            continue
        u = qh / nq * math.sqrt(hs)                                    # a key c u scores c
        kh = k[:, hh * hs:(hh + 1) * hs]
        kh -= np.outer(kh @ qh / nq, qh)                              # the noise scores 0
        self_s = float(np.dot(qh, self_k[hh * hs:(hh + 1) * hs])) / math.sqrt(hs)
        top = max(self_s, 0.0) + SINK_GAP
        sc = np.where(tail, top - rng.uniform(TAIL_LO, TAIL_HI, pos), top - SINK_GAP - rng.uniform(0.0, 5.0, pos))
        if 0 <= sink_at < pos:
            sc[sink_at] = top
        kh += np.outer(sc, u)
    return k.astype(np.float32), v


def sink_caches(cfg: O.Config, w: dict, token: int, pos: int, sink_at: int, seed: int = 0, tail_every: int = 1):
    """key / value caches of every layer (the oracle's layout [L, seq, dim]) with a sink at `sink_at` for the query that forward(token,
    pos) forms in each layer.  Built layer by layer: layer l's query depends on the attention of the layers below it."""
    rng = np.random.default_rng([seed, pos, sink_at])
    L, T, d = cfg.n_layers, cfg.seq_len, cfg.dim
    kc = np.zeros((L, T, d), np.float32)
    vc = np.zeros((L, T, d), np.float32)
    orc = O.Oracle(cfg, w)
    for l in range(L):
        orc.s["key_cache"][:] = kc.reshape(-1)
        orc.s["value_cache"][:] = vc.reshape(-1)
        orc.forward_range(token, pos, 0, l + 1, True, False)
        kl, vl = sink_cache_layer(orc.s["q"].copy(), orc.s["k"].copy(), cfg.n_heads, pos, sink_at, rng, tail_every)
        kc[l, :pos] = kl
        vc[l, :pos] = vl
    return kc.reshape(-1), vc.reshape(-1)


# ------------------------------------------------------------------ the Q8 twins (tests/q8_ref.py)

def cfg_dict(cfg) -> dict:
    """O.Config -> the dict Q8Ref / write_v2 take"""
    if isinstance(cfg, dict):
        return dict(cfg)
    return dict(dim=cfg.dim, hidden_dim=cfg.hidden_dim, n_layers=cfg.n_layers, n_heads=cfg.n_heads, n_kv_heads=cfg.n_kv_heads,
                vocab_size=cfg.vocab_size, seq_len=cfg.seq_len, shared_weight=bool(cfg.shared_weight))


def trained_like_q8(cfg, kind: str, gs: int, seed: int):
    """-> (norms, t) for Q8Ref / write_v2: trained_like_weights quantized by export.py's rule (q8_ref.quantize_q80), every layer's
    matrix on its own as synth_q8 does; tok and wcls are one pair when the classifier is shared.  The DESIGNATED rows survive the
    round trip with their property (tests/test_trained_like_host.py): the tie row keeps its 64 and its tail (the tail values that share
    the 64's group round to zero: still SEQ groups), the zero row is zero, the subnormal row stays non-zero with subnormal squares, the
    large row stays finite in the sum."""
    from . import q8_ref as R
    c = O.Config(**cfg) if isinstance(cfg, dict) else cfg
    w = trained_like_weights(c, kind, seed)
    norms = {n: np.ascontiguousarray(w[n], np.float32).reshape(-1) for n in ("rms_att_weight", "rms_ffn_weight", "rms_final_weight")}
    names = dict(tok="token_embedding_table")
    t = {}
    for name in R.TENSORS:
        if name == "wcls" and c.shared_weight:
            t["wcls"] = t["tok"]
            continue
        a = np.ascontiguousarray(w.pop(names.get(name, name)), np.float32)
        if name in ("tok", "wcls"):
            t[name] = R.quantize_q80(a, gs)
        else:
            parts = [R.quantize_q80(a[l], gs) for l in range(c.n_layers)]
            t[name] = (np.concatenate([q for q, _ in parts]), np.concatenate([s_ for _, s_ in parts]))
        del a
    return norms, t


def sink_caches_q8(ref, token: int, pos: int, sink_at: int, seed: int = 0, tail_every: int = 1):
    """sink_caches for the Q8 model: `ref` is a Q8Ref (or a callable returning one); layer l's sink keys are built for the query the
    Q8 forward forms in layer l over the layers below (Q8Ref.forward(..., rope_stop=l)).  The KV cache is fp32 in the Q8 model, so
    sink_cache_layer serves unchanged.  ref's caches are left holding the result."""
    ref = ref() if callable(ref) else ref
    c = ref.c
    rng = np.random.default_rng([seed, pos, sink_at])
    L, T, d = c.n_layers, c.seq_len, c.dim
    kc = np.zeros((L, T, d), np.float32)
    vc = np.zeros((L, T, d), np.float32)
    for l in range(L):
        ref.s["key_cache"][:] = kc.reshape(-1)
        ref.s["value_cache"][:] = vc.reshape(-1)
        ref.forward(token, pos, rope_stop=l)
        kl, vl = sink_cache_layer(ref.s["q"].copy(), ref.s["k"].copy(), c.n_heads, pos, sink_at, rng, tail_every)
        kc[l, :pos] = kl
        vc[l, :pos] = vl
    ref.s["key_cache"][:] = kc.reshape(-1)
    ref.s["value_cache"][:] = vc.reshape(-1)
    return kc.reshape(-1), vc.reshape(-1)


def one_element_groups(q, gs: int) -> float:
    """the share of groups of an int8 vector in which one |q| is 127 and every other |q| <= 1 (a massive channel sets the scale)"""
    a = np.sort(np.abs(np.asarray(q).reshape(-1, gs).astype(np.int32)), axis=1)
    return float(np.mean((a[:, -1] == 127) & (a[:, -2] <= 1)))


MASSIVE_MULTS = (400.0, 1500.0, 3000.0)
FLT_MAX = float(np.finfo(np.float32).max)
Q8_VECTORS = ("massive", "every_group", "equal", "tiny", "large", "fltmax", "near_half")


def near_half_group(gs: int, top: np.float32, ks, rng) -> np.ndarray:
    """one group with max |x| = top (scale = fl(top / 127)) whose other values sit where the quantizer's rounding decides: for each k
    the fp32 values x around (k + 0.5) scale whose fp32 QUOTIENT fl(x / scale) is the largest below k + 0.5, k + 0.5 itself when some
    x gives it, and the smallest above (one or two ulps of the quotient away).  Searched over the fp32 neighbours of fl((k + 0.5) scale) with numpy's correctly rounded fp32
    division -- a float64 quotient would place them differently."""
    top = np.float32(top)
    scale = np.float32(top / np.float32(127.0))
    out = [top]
    for k in ks:
        t = np.float32(k + 0.5)
        x0 = np.float32(t * scale)
        cand = [x0]
        lo = hi = x0
        for _ in range(6):
            lo = np.nextafter(lo, np.float32(-np.inf)); hi = np.nextafter(hi, np.float32(np.inf))
            cand += [lo, hi]
        cand = np.sort(np.array(cand, np.float32))
        r = (cand / scale).astype(np.float32)
        pick = []
        if (r < t).any():
            pick.append(cand[r < t][-1])
        if (r == t).any():
            pick.append(cand[r == t][0])
        if (r > t).any():
            pick.append(cand[r > t][0])
        for x in pick:
            out.append(x if rng.random() < 0.5 else -x)
    out = out[:gs]
    g = np.zeros(gs, np.float32)
    g[:len(out)] = out
    return g


def q8_vector(kind: str, n: int, gs: int, seed: int = 0) -> np.ndarray:
    """one activation vector of n values (gs | n) that is hard on the Q8 activation quantizer and on the in-order group sum:

    massive      N(0, 1) with the three massive_channels 400 / 1500 / 3000 times the median |x|: their groups' scales are set by one
                 element and every other element of the group lands on 0 or +-1;
    every_group  the same with one such element in EVERY group (rotating place and multiplier);
    equal        every group all-equal in magnitude (mixed signs in every second group): all +-127, over 60 binades of scale;
    tiny         groups whose max is the smallest normal over subnormal others, and groups whose max is a subnormal with the others
                 eight times smaller: the scale itself is subnormal;
    large        groups at 1e16 .. 2e17;
    fltmax       groups whose max is FLT_MAX / 2;
    near_half    near_half_group over many scales and every k of 0 .. 126."""
    assert n % gs == 0 and kind in Q8_VECTORS, (kind, n, gs)
    rng = np.random.default_rng([seed, Q8_VECTORS.index(kind), gs])
    G = n // gs
    sign = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    if kind in ("massive", "every_group"):
        x = rng.standard_normal(n).astype(np.float32)
        med = float(np.median(np.abs(x)))
        if kind == "massive":
            where = list(zip(massive_channels(n), MASSIVE_MULTS))
        else:
            where = [(g * gs + (7 * g) % gs, MASSIVE_MULTS[g % 3]) for g in range(G)]
        for c, mult in where:
            x[c] = np.float32(sign(()) * mult * med)
        return x
    if kind == "equal":
        mag = np.exp2(rng.uniform(-40.0, 20.0, G)) * rng.uniform(1.0, 2.0, G)
        x = np.repeat(mag, gs).reshape(G, gs)
        x[1::2] *= sign((len(x[1::2]), gs))
        x[2::4] *= -1.0
        return x.astype(np.float32).reshape(-1)
    if kind == "tiny":
        tiny = float(np.finfo(np.float32).tiny)
        x = np.zeros((G, gs), np.float64)
        for g in range(G):
            if g % 2 == 0:      # max = the smallest normal, the others subnormal
                x[g] = sign(gs) * rng.uniform(0.0, 1.0, gs) * tiny
                x[g, (3 * g) % gs] = tiny * sign(())
            else:               # max subnormal (2^-130 .. 2^-127), the others eight times smaller
                m = tiny * 2.0 ** -int(rng.integers(1, 5))
                x[g] = sign(gs) * rng.uniform(0.5, 1.0, gs) * m / 8.0
                x[g, (5 * g) % gs] = m * sign(())
        return x.astype(np.float32).reshape(-1)
    if kind == "large":
        return (sign(n) * rng.uniform(1e16, 2e17, n)).astype(np.float32)
    if kind == "fltmax":
        x = (sign((G, gs)) * rng.uniform(0.0, 0.5, (G, gs)) * FLT_MAX).astype(np.float32)
        for g in range(G):
            x[g, (11 * g) % gs] = np.float32(FLT_MAX / 2) * np.float32(sign(()))
        return x.reshape(-1)
    per = max(1, (gs - 1) // 3)
    ks = [int(k) for k in rng.permutation(127)]
    out = []
    for g in range(G):
        top = np.float32(127.0 * 0.0371 * 1.37 ** (g % 40) * rng.uniform(1.0, 1.3))
        out.append(near_half_group(gs, top, [ks[(g * per + i) % 127] for i in range(per)], rng))
    return np.concatenate(out)


def q8_rows(n_tok: int, n: int, gs: int, seed: int = 0, kinds=Q8_VECTORS) -> np.ndarray:
    """[n_tok, n]: row t is q8_vector(kinds[t % len(kinds)], seed + t // len(kinds))"""
    return np.stack([q8_vector(kinds[t % len(kinds)], n, gs, seed + t // len(kinds)) for t in range(n_tok)])


def harsh_q8_matrix(d: int, n: int, gs: int, seed: int = 0):
    """(int8 values, scales) of a [d, n] Student-t matrix (std 0.02) with three columns x 20 and three rows x 300, quantized by
    export.py's rule: the group terms of a row span many binades"""
    from . import q8_ref as R
    rng = np.random.default_rng([seed, d, n])
    w = _student_t(rng, (d, n), 0.02)
    w[:, rng.choice(n, 3, replace=False)] *= np.float32(20.0)
    w[rng.choice(d, 3, replace=False), :] *= np.float32(300.0)
    return R.quantize_q80(w, gs)


# ------------------------------------------------------------------ sequential-sum properties (numpy)

def seq_sum_f32(a) -> np.float32:
    a = np.ascontiguousarray(a, np.float32)
    return np.add.accumulate(a, dtype=np.float32)[-1] if a.size else np.float32(0)


def seq_groups(a) -> dict:
    """the groups of FS_GROUP terms of a sequential sum that seqsum_fast.hpp must walk term by term (SEQ groups) for one of these
    reasons: a zero term, a tie (a term an odd multiple of half an ulp of the running sum), or a running sum at either end of the group
    within 2^-12 of a binade edge (or zero) -- and the items they put on its walk list"""
    a = np.ascontiguousarray(a, np.float32)
    acc = np.add.accumulate(a, dtype=np.float32)
    pre = np.concatenate([[np.float32(0)], acc[:-1]]).astype(np.float32)
    ulp = np.spacing(np.abs(pre)).astype(np.float64)
    r = a.astype(np.float64) / ulp
    tie = (pre > 0) & (np.abs(r - np.floor(r) - 0.5) == 0)

    def near_edge(p):
        p = p.astype(np.float64)
        m = np.where(p > 0, p / np.exp2(np.floor(np.log2(np.where(p > 0, p, 1.0)))), 1.0)
        return (p <= 0) | (m < 1.0 + 2.0 ** -12) | (m > 2.0 - 2.0 ** -11)

    n = a.size // FS_GROUP * FS_GROUP
    bad = (tie | (a == 0))[:n].reshape(-1, FS_GROUP).any(axis=1)
    edge = near_edge(pre[:n:FS_GROUP]) | near_edge(acc[FS_GROUP - 1:n:FS_GROUP])
    g = bad | edge
    return {"groups": int(g.sum()), "items": int(g.sum()) * FS_GROUP, "ties": int(tie.sum()), "edge": int(edge.sum())}


# ------------------------------------------------------------------ the comparator against the float64 forward

F64_A = 4.0      # see f64_bound
F64_B = 32.0
EPS = 2.0 ** -24

COMPARED = ("logits", "x", "xb", "hb", "q", "key_cache", "value_cache", "att")


def probabilities_f64(scores: np.ndarray, n_heads: int, seq_len: int, pos: int) -> np.ndarray:
    """oracle_forward_f64 leaves the last layer's SCORES in att; the fp32 forward leaves probabilities: softmax them in float64"""
    s = scores.reshape(n_heads, seq_len)[:, :pos + 1].astype(np.float64)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def state_view(state: dict, cfg: O.Config, pos: int, f64: bool = False) -> dict:
    """the buffers the comparator reads, from a RunState dict (oracle.s or a download): the cache rows of position pos of every layer,
    the last layer's probabilities over positions 0..pos"""
    L, T, d = cfg.n_layers, cfg.seq_len, cfg.dim
    out = {}
    for k in ("logits", "x", "xb", "hb", "q"):
        if k in state:
            out[k] = np.asarray(state[k], np.float64)
    for k in ("key_cache", "value_cache"):
        if k in state:
            out[k] = np.asarray(state[k]).reshape(L, T, d)[:, pos].astype(np.float64)
    if "att" in state:
        out["att"] = (probabilities_f64(state["att"], cfg.n_heads, T, pos) if f64 else
                      np.asarray(state["att"]).reshape(cfg.n_heads, T)[:, :pos + 1].astype(np.float64))
    return out


def f64_bound(P: dict, Ov: dict, F: dict, a: float = F64_A, b: float = F64_B) -> dict:
    """per buffer (err, bound):  err = max|P - F|,  bound = a max|O - F| + b 2^-24 max|F|.

    P: the mode under test, O: the fp32 oracle, F: the float64-accumulated forward (oracle_forward_f64), all over the same inputs.
    The fp32 oracle is a legitimate execution whose distance to F is the reference's own rounding; a mode in another summation order
    may be as far from F as that, in a different direction, but not several times farther.  The second term is a floor for buffers
    where O happens to equal F (exact zeros, a handful of terms) -- 32 ulps of the buffer's largest magnitude.

    a = 4, b = 32, from measurements on MI355X over both kinds, all four shapes and every case of tests/test_hip_trained_like.py: the
    worst err / bound was 0.445 (tolerance mode, d2048 sink), 0.30 at d4096, <= 0.14 in fast mode (split-T over sink caches included),
    0.245 in bar mode beyond its switch -- err stayed below 1.8 max|O - F|.  The fp32 oracle itself scores 1 / a = 0.25.  The planted
    faults of tests/test_trained_like_host.py (attention over pos positions, one dropped 16-column block) score 10^3 .. 10^5."""
    out = {}
    for k, f in F.items():
        if k not in P or k not in Ov:
            continue
        p, o = np.asarray(P[k], np.float64), np.asarray(Ov[k], np.float64)
        err = float(np.max(np.abs(p - f))) if f.size else 0.0
        bound = a * (float(np.max(np.abs(o - f))) if f.size else 0.0) + b * EPS * (float(np.max(np.abs(f))) if f.size else 0.0)
        out[k] = (err, bound)
    return out


def assert_f64_bound(P, Ov, F, what="", a: float = F64_A, b: float = F64_B) -> float:
    """raise if any buffer breaks f64_bound; -> the worst err / bound"""
    worst = 0.0
    for k, (err, bound) in f64_bound(P, Ov, F, a, b).items():
        r = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
        worst = max(worst, r)
        assert err <= bound, f"{what} {k}: max|P - F| = {err:.4g} > {bound:.4g} = {a} max|O - F| + {b} 2^-24 max|F|"
    return worst


def greedy_margin_ok(logits_f: np.ndarray, bound: float) -> bool:
    """the top-2 margin of F's logits is larger than the comparator's bound: every admissible execution picks the same token"""
    t = np.sort(np.asarray(logits_f, np.float64))[-2:]
    return float(t[1] - t[0]) > 2.0 * bound
