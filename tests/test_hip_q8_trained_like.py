"""-m gpu: the Q8_0 paths (rama_q8_forward / generate / prefill / decode_batch and the op-level entries) on trained-like data
(tests/trained_like.py), bit for bit against tests/q8_ref.py and against the single-token rama_q8_forward twin.  No tolerance anywhere.

Why the Q8 path needs its own run on this data: every Q8 norm is a stand-alone rmsnorm_chain_kernel launch whose sum of squares goes
through the whole cascade seq_sum_lds_fast -> seq_sum_predict -> seq_sum_exact (fp32 parity mode folds its layer norms into the matvec
launches, so the fp32 tests prove the leader's fallback and not this kernel's); the token-batch forms run one workgroup per token, so a
fallback taken by ONE workgroup among fast neighbours shows per-block shared state, a non-uniform return in front of a barrier or
wrong stride indexing; q8_variant picks three attention launches by position, none of which had seen a sink under a Q8 model; and
the activation quantizer had only seen Gaussian vectors.

The fallbacks are proven to run (rama_internal_pred_stats counts seq_sum_predict calls of lists longer than 512; the norm makes one
only after seq_sum_lds_fast gave up), not hoped for.  Non-finite inputs are out of scope: q8_ref.quantize pins NaN to 0 through
nan_to_num while a C cast of NaN to int8 is undefined -- the two disagree by construction.

Models up to d2048 are version-2 files written by q8_ref.write_v2 and loaded by Q8Model.load; d4096 runs through an uploaded
rama_q8_weights struct (the caller-owned-weights entry of the ABI), its RoPE tables from oracle.synth.rope_tables.  One big case is
kept alive at a time."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import synth as S
from tests import q8_ref as R
from tests import trained_like as T
from tests.test_hip_q8 import Buf, check_state, dev_matmul, dev_quantize, same_bits
from tests.test_hip_q8_batch import check_rows, dev_matmul_batch, full_state
from tests.test_hip_trained_like import SHAPES, TOKS, pred_stats

pytestmark = pytest.mark.gpu

GS = {"d288": 32, "d768": 64, "d2048": 64, "d4096": 64}
SEED = 11
SPREAD_POS_DEFAULT = 128      # ctx.hpp kSpreadAttnPos
SPREAD_NEVER = 1 << 20
MILD = 7                      # a token of TOKS whose row has no designed property

_cache = {}


def q8_case(shape, kind):
    """(cfg dict, group size, norms, tensors); a 7B-width case (400 MB) is kept alone"""
    key = (shape, kind)
    if key not in _cache:
        if shape == "d4096" or any(k[0] == "d4096" for k in _cache):
            _cache.clear()
        d, h, L, H, V, seq = SHAPES[shape]
        cfg = O.Config(d, h, L, H, H, V, seq, False)
        _cache[key] = (T.cfg_dict(cfg), GS[shape]) + T.trained_like_q8(cfg, kind, GS[shape], SEED)
    return _cache[key]


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    _cache.clear()
    d.close()


@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("q8_trained_like")


def loaded(dev, ckpt_dir, shape, kind):
    """-> (Q8Model from a written version-2 file, a factory of fresh Q8Refs over the device's RoPE tables)"""
    import rama_amd
    cfg, gs, norms, t = q8_case(shape, kind)
    p = ckpt_dir / f"{shape}_{kind}.bin"
    if not p.exists():
        R.write_v2(p, cfg, gs, False, norms, t)
    m = rama_amd.Q8Model.load(dev, p)
    rope = (m.tensor("freq_cis_real"), m.tensor("freq_cis_imag"))
    return m, lambda: R.Q8Ref(cfg, gs, norms, t, rope)


class UploadedQ8:
    """caller-owned weights: a rama_q8_weights struct over plain device allocations (what Q8Engine and decode_batch need of a Q8Model)"""

    def __init__(self, dev, cfg: dict, gs: int, norms: dict, t: dict, rope):
        from rama_amd._lib import rama_config, rama_q8_weights
        from rama_amd.transformer import Config
        self.device, self.group_size = dev, gs
        self.cfg = self.config = Config(cfg["dim"], cfg["hidden_dim"], cfg["n_layers"], cfg["n_heads"], cfg["n_kv_heads"], cfg["vocab_size"],
                                        cfg["seq_len"], bool(cfg["shared_weight"]))
        self.ccfg = rama_config(cfg["dim"], cfg["hidden_dim"], cfg["n_layers"], cfg["n_heads"], cfg["n_kv_heads"], cfg["vocab_size"],
                                cfg["seq_len"], int(cfg["shared_weight"]))
        self.bufs = []
        w = rama_q8_weights()
        w.group_size = gs

        def up(a):
            b = Buf(dev, np.ascontiguousarray(a))
            self.bufs.append(b)
            return b.p

        w.token_embedding_table = up(R.dequantize(*t["tok"], gs))
        for k, v in norms.items():
            setattr(w, k, up(np.asarray(v, np.float32)))
        w.freq_cis_real, w.freq_cis_imag = up(np.asarray(rope[0], np.float32)), up(np.asarray(rope[1], np.float32))
        for k in R.TENSORS:
            if k == "wcls" and cfg["shared_weight"]:
                w.wcls, w.wcls_s = w.tok, w.tok_s
                continue
            setattr(w, k, up(t[k][0]))
            setattr(w, k + "_s", up(t[k][1]))
        self.weights = w

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def uploaded(dev, shape, kind):
    cfg, gs, norms, t = q8_case(shape, kind)
    rope = S.rope_tables(cfg["seq_len"], cfg["dim"] // cfg["n_heads"])
    return UploadedQ8(dev, cfg, gs, norms, t, rope), lambda: R.Q8Ref(cfg, gs, norms, t, rope)


def set_spread(dev, v):
    from rama_amd._lib import check
    check(dev.lib.rama_set_tuning(dev.ctx, b"spread_pos", v))


def quantized_equal(q, s, wq, ws):
    """the device quantizer's output is the reference's: the int8 values and the bits of the scales"""
    return bool(np.array_equal(np.asarray(q, np.int8), wq) and same_bits(s, ws))


def set_caches(eng, kc, vc):
    eng.set_buffer("key_cache", kc); eng.set_buffer("value_cache", vc)


def check_rows_of(eng, ref, positions, what=""):
    """the cache rows of `positions` in every layer are the reference's"""
    c = ref.c
    for l in range(c.n_layers):
        for p in positions:
            o = (l * c.seq_len + p) * c.dim
            assert same_bits(eng.buffer("key_cache", c.dim, o), ref.cache_row("key_cache", l, p)), (what, "key", l, p)
            assert same_bits(eng.buffer("value_cache", c.dim, o), ref.cache_row("value_cache", l, p)), (what, "value", l, p)


def check_more(eng, ref, pos, what=""):
    """check_state plus the buffers the forward leaves behind it: xb (the residual in front of the final norm), hb, the last layer's
    query and its probabilities over 0 .. pos"""
    c = ref.c
    check_state(eng, ref, pos)
    for b, n in (("xb", c.dim), ("hb", c.hidden_dim), ("q", c.dim)):
        assert same_bits(eng.buffer(b, n), ref.s[b]), (what, pos, b)
    att = eng.buffer("att", c.n_heads * c.seq_len).reshape(c.n_heads, c.seq_len)[:, :pos + 1]
    assert same_bits(att, ref.s["att"].reshape(c.n_heads, c.seq_len)[:, :pos + 1]), (what, pos, "att")


# ------------------------------------------------------------------ a. ops

@pytest.mark.parametrize("gs", [32, 64, 128])
def test_quantize_harsh_groups(dev, gs):
    """rama_q8_quantize on the vectors of trained_like.q8_vector, one by one and as a T x n batch in one call (the batch path
    quantizes nt * dim floats at once).  The share of one-element groups is asserted on the reference's output, so that this test
    cannot quietly run on milder data (figures: tests/test_trained_like_host.py)."""
    n = 2048
    for kind in T.Q8_VECTORS:
        x = T.q8_vector(kind, n, gs)
        wq, ws = R.quantize(x, gs)
        if kind == "every_group":
            assert T.one_element_groups(wq, gs) >= 0.9
        if kind == "massive":
            assert T.one_element_groups(wq, gs) * (n // gs) >= 2
        rc, q, s = dev_quantize(dev, x, gs)
        assert rc == 0 and quantized_equal(q, s, wq, ws), (kind, gs, np.flatnonzero(q != wq)[:8])
    rows = T.q8_rows(2 * len(T.Q8_VECTORS) + 1, n, gs, seed=1)
    wq, ws = R.quantize(rows.reshape(-1), gs)
    rc, q, s = dev_quantize(dev, rows.reshape(-1), gs)
    assert rc == 0 and quantized_equal(q, s, wq, ws), (gs, np.flatnonzero(q != wq)[:8])


# (fltmax stays out of the product: a group term (float)ival * ws * xs overflows at xs = 1e36, and inf - inf is a NaN whose bits the
# definition does not fix)
MATMUL_KINDS = tuple(k for k in T.Q8_VECTORS if k != "fltmax")


@pytest.mark.parametrize("gs", [32, 64, 128])
def test_matmul_harsh_activations_and_weights(dev, gs):
    """rama_q8_matmul and rama_q8_matmul_batch at 1, 16, 32, 33 and 128 tokens: the group terms of a row span many binades (x 20
    columns, x 300 rows, one-element groups, scales from subnormal to 1e15), so an out-of-order or fused add changes bits"""
    n, d = 2048, 203
    wq, ws = T.harsh_q8_matrix(d, n, gs)
    rows = T.q8_rows(128, n, gs, seed=2, kinds=MATMUL_KINDS)
    qs = [R.quantize(r, gs) for r in rows]
    xq, xs = np.concatenate([q for q, _ in qs]), np.concatenate([s for _, s in qs])
    G = n // gs
    for t in range(len(MATMUL_KINDS)):
        got = dev_matmul(dev, wq, ws, xq[t * n:(t + 1) * n], xs[t * G:(t + 1) * G], n, d, gs)
        want = R.matmul(xq[t * n:(t + 1) * n], xs[t * G:(t + 1) * G], wq, ws, gs)
        assert np.isfinite(want).all()
        assert same_bits(got, want), (MATMUL_KINDS[t], gs, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
    for n_tok in (1, 16, 32, 33, 128):
        got = dev_matmul_batch(dev, wq, ws, xq[:n_tok * n], xs[:n_tok * G], n, d, gs, n_tok)
        check_rows(got, xq, xs, wq, ws, n, gs)


# ------------------------------------------------------------------ b. rama_q8_forward / rama_q8_generate

def forward_case(dev, eng, ref, shape, kind, graph):
    eng.set_graph_mode(graph)
    try:
        for pos, tok in enumerate(TOKS):
            ref.forward(tok, pos)
            eng.forward(tok, pos)
            check_more(eng, ref, pos, f"{shape} {kind} graph {graph}")
    finally:
        eng.set_graph_mode(0)


def predict_calls(dev, eng, tok, pos):
    """seq_sum_predict calls (held + fell back) around one forward"""
    pred_stats(dev, reset=True)
    eng.forward(tok, pos)
    held, fell = pred_stats(dev)
    return held + fell


def norm_fallback_proof(dev, eng, shape):
    """at the position behind TOKS, over the same caches: the tie row's layer-0 norm makes seq_sum_lds_fast give up from dim 2048 on
    (its 2 048 / 4 096 items pass kFsCap): one seq_sum_predict call more than a mild token's forward.  At 768 the list holds 768 items
    and the counts are to be equal.

    Before seqsum_fast.hpp kept padding off its walk list this read tie 1, mild 0 at d768 (MI355X, both kinds): the kernel's 256
    threads of 8 terms leave 160 threads with nothing but the zeros behind a 768-term list's end, and at a running sum of exactly
    4096.0 -- a binade edge -- each of those groups went on the list as 8 items: 768 + 1 280 = 2 048 > kFsCap.  The sum was exact
    either way (seq_sum_predict served it); the row's norm was the slower one."""
    pos = len(TOKS)
    mild = predict_calls(dev, eng, MILD, pos)
    tie = predict_calls(dev, eng, T.TOK_TIE, pos)
    print(f"seq_sum_predict calls {shape}: tie token {tie}, mild token {mild}")
    if shape == "d768":
        assert tie == mild, (shape, tie, mild)
    else:
        assert tie > mild, (shape, tie, mild)


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("shape,graph", [("d288", 0), ("d288", 1), ("d768", 0), ("d768", 1), ("d2048", 0)])
def test_forward_every_position_loaded_model(dev, ckpt_dir, shape, graph, kind):
    """every position of TOKS (the designated rows early): logits, x, xb, hb, q, the probabilities and the cache rows of every layer
    are Q8Ref's bits"""
    import rama_amd
    m, make_ref = loaded(dev, ckpt_dir, shape, kind)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        forward_case(dev, eng, make_ref(), shape, kind, graph)
    finally:
        eng.free(); m.free()


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("shape", ["d768", "d2048"])
def test_norm_fallback_is_counted(dev, ckpt_dir, shape, kind):
    """proof that the stand-alone norm's fallback ran (d4096: in the uploaded-weights test below)"""
    import rama_amd
    m, _ = loaded(dev, ckpt_dir, shape, kind)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        for pos, tok in enumerate(TOKS):
            eng.forward(tok, pos)
        norm_fallback_proof(dev, eng, shape)
    finally:
        eng.free(); m.free()


@pytest.mark.parametrize("kind", T.KINDS)
def test_forward_every_position_uploaded_weights_d4096(dev, kind):
    """llama2-7B's width through a caller-owned rama_q8_weights struct"""
    import rama_amd
    m, make_ref = uploaded(dev, "d4096", kind)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        forward_case(dev, eng, make_ref(), "d4096", kind, 0)
        norm_fallback_proof(dev, eng, "d4096")
    finally:
        eng.free(); m.free()


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("shape", ["d288", "d768"])
def test_generate_designated_prompt(dev, ckpt_dir, shape, kind):
    """rama_q8_generate with the designated tokens forced as the prompt, greedy and sampled (T 1, top-p 0.9, the CPU draw)"""
    import rama_amd
    from rama_amd.sampler_const import TOPP_U_CPU
    m, make_ref = loaded(dev, ckpt_dir, shape, kind)
    eng = rama_amd.Q8Engine(dev, m)
    steps, prompt = 16, TOKS[1:]
    try:
        for graph in (0, 1):
            eng.set_graph_mode(graph)
            assert eng.generate(prompt, steps) == make_ref().generate(prompt, steps), (shape, kind, graph, "greedy")
            got = eng.generate(prompt, steps, temperature=1.0, topp=0.9)
            assert got == make_ref().generate(prompt, steps, 1.0, 0.9, TOPP_U_CPU), (shape, kind, graph, "sampled")
    finally:
        eng.set_graph_mode(0)
        eng.free(); m.free()


# ------------------------------------------------------------------ c. sinks under the three attention variants

SINK_TOKEN, SINK_POS = 9, 1099


def sink_ats(pos):
    return [a for a in (0, 256, pos - 1) if a < pos]


def test_sinks_under_all_three_attention_variants(dev, ckpt_dir):
    """d2048 / sink over sink_caches_q8: position 200 on 4 waves per head, 300 on 16, both again spread over the chip, and 1099 with
    spread_pos at its default (spread), below 1099 (spread) and above it (one launch of 16 waves).  The three softmax sums are three
    call sites of seq_sum_cascade.  With the sink first at 1099 the walk list overflows and the prediction sits at a binade edge:
    fallbacks are counted."""
    import rama_amd
    m, make_ref = loaded(dev, ckpt_dir, "d2048", "sink")
    eng = rama_amd.Q8Engine(dev, m)
    ref = make_ref()
    plan = [(200, SPREAD_NEVER), (300, SPREAD_NEVER), (200, SPREAD_POS_DEFAULT), (300, SPREAD_POS_DEFAULT),
            (SINK_POS, SPREAD_POS_DEFAULT), (SINK_POS, 1000), (SINK_POS, 2000)]
    caches = {}
    try:
        for pos, spread in plan:
            for at in sink_ats(pos):
                if (pos, at) not in caches:
                    caches[(pos, at)] = T.sink_caches_q8(ref, SINK_TOKEN, pos, at)
                kc, vc = caches[(pos, at)]
                ref.s["key_cache"][:] = kc; ref.s["value_cache"][:] = vc
                ref.forward(SINK_TOKEN, pos)
                set_caches(eng, kc, vc)
                set_spread(dev, spread)
                pred_stats(dev, reset=True)
                eng.forward(SINK_TOKEN, pos)
                held, fell = pred_stats(dev)
                check_more(eng, ref, pos, f"sink at {at} spread_pos {spread}")
                if pos == SINK_POS and at == 0:
                    assert fell > 0, (spread, held, fell)
    finally:
        set_spread(dev, SPREAD_POS_DEFAULT)
        eng.free(); m.free()


# ------------------------------------------------------------------ d. token batches: a fallback in one workgroup among fast neighbours

def prompt_with_designated(cfg, n, rng):
    """n tokens, mild except: rows 0 and 1, a middle row and its neighbour, the last batched row (n - 2; the last token runs as
    forward()) and, for a prompt of two weight passes, the last row of the first pass (127) and the first of the second (128)"""
    toks = [int(t) for t in rng.integers(8, cfg["vocab_size"], n)]
    put = {0: T.TOK_TIE, 1: T.TOK_ZERO, n // 2: T.TOK_SUBNORMAL, n // 2 + 1: T.TOK_LARGE, n - 2: T.TOK_TIE}
    if n > 129:
        put.update({127: T.TOK_TIE, 128: T.TOK_ZERO})
    for i, t in put.items():
        toks[i] = t
    return toks


@pytest.mark.parametrize("n", [40, 131])
@pytest.mark.parametrize("shape", ["d768", "d2048"])
def test_prefill_designated_rows_among_mild_ones(dev, ckpt_dir, shape, n):
    """Q8Engine.prefill on massive weights: 40 tokens (one pass) and 131 (two passes of 128 + 2 and the forward tail).  The full state
    is the per-position forward twin's, the cache rows of every position Q8Ref's."""
    import rama_amd
    m, make_ref = loaded(dev, ckpt_dir, shape, "massive")
    eng, twin = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, m)
    ref = make_ref()
    try:
        toks = prompt_with_designated(q8_case(shape, "massive")[0], n, np.random.default_rng(n))
        eng.prefill(toks, 0)
        for p, t in enumerate(toks):
            twin.forward(t, p)
            ref.forward(t, p)
        got, want = full_state(eng), full_state(twin)
        for k in got:
            assert same_bits(got[k], want[k]), (shape, n, k)
        assert same_bits(got["logits"], ref.s["logits"]) and same_bits(got["x"], ref.s["x"]), (shape, n)
        c = ref.c
        for b in ("key_cache", "value_cache"):
            g = got[b].reshape(c.n_layers, c.seq_len, c.dim)[:, :n]
            assert same_bits(g, ref.s[b].reshape(c.n_layers, c.seq_len, c.dim)[:, :n]), (shape, n, b)
    finally:
        eng.free(); twin.free(); m.free()


@pytest.mark.parametrize("n_seq", [5, 32, 33, 65])
@pytest.mark.parametrize("shape", ["d768", "d2048"])
def test_decode_batch_designated_tokens_in_some_sequences(dev, ckpt_dir, shape, n_seq):
    """three steps of rama_q8_decode_batch on massive weights, each sequence fed its own argmax; 32 / 33 sequences straddle the K-split
    and one-wave product kernels.  Logits and appended rows are the twins', and Q8Ref's for the first and the last sequence."""
    import rama_amd
    from rama_amd.q8 import decode_batch
    m, make_ref = loaded(dev, ckpt_dir, shape, "massive")
    c = m.cfg
    rng = np.random.default_rng(n_seq)
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(n_seq)]
    twins = [rama_amd.Q8Engine(dev, m) for _ in range(n_seq)]
    refs = {0: make_ref(), n_seq - 1: make_ref()}
    try:
        cur = [T.DESIGNATED[i % 4] if i % 3 == 0 else int(rng.integers(8, c.vocab_size)) for i in range(n_seq)]
        pos = [0] * n_seq
        for step in range(3):
            decode_batch(engs, cur, pos)
            for i in range(n_seq):
                twins[i].forward(cur[i], pos[i])
                lo = engs[i].logits()
                assert same_bits(lo, twins[i].logits()), (shape, n_seq, i, step)
                for l in range(c.n_layers):
                    o = (l * c.seq_len + pos[i]) * c.dim
                    for b in ("key_cache", "value_cache"):
                        assert same_bits(engs[i].buffer(b, c.dim, o), twins[i].buffer(b, c.dim, o)), (shape, n_seq, i, step, b, l)
                if i in refs:
                    refs[i].forward(cur[i], pos[i])
                    assert same_bits(lo, refs[i].s["logits"]), (shape, n_seq, i, step)
                    check_rows_of(engs[i], refs[i], [pos[i]], f"{shape} batch {n_seq} sequence {i} step {step}")
                cur[i] = T.DESIGNATED[(i + step) % 4] if (step == 0 and i % 3 == 1) else O.argmax(lo)
                pos[i] += 1
    finally:
        for e in engs + twins:
            e.free()
        m.free()


def test_batched_attention_over_sinks(dev, ckpt_dir):
    """d2048 / sink: a prefill of 12 tokens from 1088 behind sink caches built for the token at 1099, and a decode batch of 6 sequences
    of which two sit at 1099 over sink caches (sink first, sink last) while the others sit at small positions over mild caches -- the
    (heads, tokens) attention grid with long, falling-back rows next to short fast ones"""
    import rama_amd
    from rama_amd.q8 import decode_batch
    m, make_ref = loaded(dev, ckpt_dir, "d2048", "sink")
    c = m.cfg
    ref = make_ref()
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(6)]
    twins = [rama_amd.Q8Engine(dev, m) for _ in range(6)]
    try:
        # --- prefill 1088 .. 1099: the last token (1099, run as forward()) is the one the sinks were built for; the eleven batched
        # rows in front of it see the same keys from other queries
        first = {at: T.sink_caches_q8(ref, SINK_TOKEN, SINK_POS, at) for at in (0, SINK_POS - 1)}
        rng = np.random.default_rng(12)
        toks = [int(t) for t in rng.integers(8, c.vocab_size, 11)] + [SINK_TOKEN]
        toks[3], toks[7] = T.TOK_TIE, T.TOK_ZERO
        kc, vc = first[0]
        ref.s["key_cache"][:] = kc; ref.s["value_cache"][:] = vc
        set_caches(engs[0], kc, vc); set_caches(twins[0], kc, vc)
        engs[0].prefill(toks, 1088)
        for i, t in enumerate(toks):
            twins[0].forward(t, 1088 + i)
            ref.forward(t, 1088 + i)
        got, want = full_state(engs[0]), full_state(twins[0])
        for k in got:
            assert same_bits(got[k], want[k]), ("prefill", k)
        assert same_bits(got["logits"], ref.s["logits"]) and same_bits(got["x"], ref.s["x"])
        check_rows_of(engs[0], ref, range(1088, 1100), "prefill over sinks")
        # --- the decode batch
        refs = [make_ref() for _ in range(6)]
        tokens = [SINK_TOKEN, MILD, T.TOK_TIE, SINK_TOKEN, 21, T.TOK_ZERO]
        positions = [SINK_POS, 3, 0, SINK_POS, 40, 7]
        for i, (r, e, tw) in enumerate(zip(refs, engs, twins)):
            if positions[i] == SINK_POS:
                kc, vc = first[0 if i == 0 else SINK_POS - 1]
            else:
                d = rng.standard_normal((2, c.n_layers * c.seq_len * c.dim)).astype(np.float32) * np.float32(0.5)
                kc, vc = d[0], d[1]
            r.s["key_cache"][:] = kc; r.s["value_cache"][:] = vc
            set_caches(e, kc, vc); set_caches(tw, kc, vc)
        pred_stats(dev, reset=True)
        decode_batch(engs, tokens, positions)
        held, fell = pred_stats(dev)
        for i in range(6):
            twins[i].forward(tokens[i], positions[i])
            refs[i].forward(tokens[i], positions[i])
            lo = engs[i].logits()
            assert same_bits(lo, twins[i].logits()), ("batch", i)
            assert same_bits(lo, refs[i].s["logits"]), ("batch", i)
            check_rows_of(engs[i], refs[i], [positions[i]], f"batch over sinks sequence {i}")
            for l in range(c.n_layers):
                o = (l * c.seq_len + positions[i]) * c.dim
                for b in ("key_cache", "value_cache"):
                    assert same_bits(engs[i].buffer(b, c.dim, o), twins[i].buffer(b, c.dim, o)), ("batch", i, b, l)
        assert fell > 0, (held, fell)
    finally:
        for e in engs + twins:
            e.free()
        m.free()
