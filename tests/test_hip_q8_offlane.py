"""Whole Q8 models on the shapes that leave the fast kernels, bit for bit against tests/q8_ref.py (shapes: tests/q8_offlane_cases.py).

* ckpt_v2_q80_gs16 (exporter-written, dim 48: group size 16): the dot4 matvec with one chunk per group, and the bytewise
  batch kernel under every epilogue (three matrices, residual add, SiLU * gate).
* ckpt_v2_q80_gs8 (dim 72: group size 8, no row a multiple of 16 bytes): the bytewise matvec and the bytewise batch kernel.
* gs128 (synthetic): the matrix-core batch kernel with two chunks per group under every epilogue, never the K-split kernel.
* longctx: a context too long for the chain attention's score buffer: launch_attention_ref in the forward, one forward per
  token in prefill and decode batch, RAMA_EUNSUP from the two chains.

Every test first asserts, through rama_q8_product_path / rama_q8_batch_shape_ok, the kernels its model must take: a later
change of a dispatch rule that moved these models back onto the fast kernels fails here instead of passing unnoticed.

Left out on purpose: the plain-kernel path of the final norm (q8_norm with rmsnorm_chain_ok false) needs dim above about
16 100; the smallest such model is over a gigabyte of weights and its numpy reference takes minutes."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import q8_ref as R
from tests import q8_offlane_cases as K
from tests import test_hip_q8_chain as CH
from tests import test_hip_q8_serve as SV
from tests.test_hip_q8 import check_state, same_bits

pytestmark = pytest.mark.gpu

EUNSUP = -2
MODELS = ["ckpt_v2_q80_gs16", "ckpt_v2_q80_gs8", "gs128"]


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


# ------------------------------------------------------------------ models, references, paths

@functools.lru_cache(maxsize=None)
def ref_parts(golden_dir, which):
    """(cfg, gs, norms, tensors) of a model -- computed once, never written to"""
    if which == "gs128":
        return (K.GS128_CFG, 128) + R.synth_q8(K.GS128_CFG, 128, K.GS128_SEED)
    if which.startswith("longctx"):
        cfg = dict(K.LONGCTX_CFG, seq_len=K.LONGCTX_DEEP_SEQ_LEN if which == "longctx_deep" else K.LONGCTX_SEQ_LEN)
        return (cfg, K.LONGCTX_GS) + R.synth_q8(cfg, K.LONGCTX_GS, K.LONGCTX_SEED)
    cfg, gs, _, norms, t = R.read_v2(golden_dir / f"{which}.bin")
    return cfg, gs, norms, t


def open_model(dev, golden_dir, which):
    import rama_amd
    cfg, gs, _, _ = ref_parts(golden_dir, which)
    if which in K.FIXTURE_CFGS:
        m = rama_amd.Q8Model.load(dev, golden_dir / f"{which}.bin")
    else:
        m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), gs, K.GS128_SEED if which == "gs128" else K.LONGCTX_SEED)
    assert m.group_size == gs and m.cfg.dim == cfg["dim"] and m.cfg.seq_len == cfg["seq_len"]
    return m


def make_ref(golden_dir, which, m):
    cfg, gs, norms, t = ref_parts(golden_dir, which)
    return R.Q8Ref(cfg, gs, norms, t, (m.tensor("freq_cis_real"), m.tensor("freq_cis_imag")))


def batch_shape_ok(dev, m):
    return dev.lib.rama_q8_batch_shape_ok(C.byref(m.ccfg))


def assert_paths(dev, m, which):
    """the kernels this model's products take, by the rule the launchers ask"""
    want = K.MODEL_PATHS[which]
    P = dev.lib.rama_q8_product_path
    assert m.group_size == want["gs"] and set(want["matvec"]) == {m.cfg.dim, m.cfg.hidden_dim}
    for n, path in want["matvec"].items():
        assert P(n, want["gs"], 0, 1) == path, (which, n)
        for n_tok in K.TOKEN_COUNTS:
            assert P(n, want["gs"], n_tok, 1) == want["gemm"], (which, n, n_tok)
    assert batch_shape_ok(dev, m) == 1
    # the loader's and the synthesizer's matrices start on 16-byte boundaries: the aligned answer is the one that holds
    w = m.weights
    for name in ("wq", "wk", "wv", "wo", "w1", "w2", "w3", "wcls"):
        assert getattr(w, name) % 16 == 0, name


def test_fixture_paths_are_the_ones_named(dev, golden_dir):
    """gs16: K = 48 and 80 on the dot4 matvec, the bytewise kernel at every token count; gs8: bytewise throughout; gs128: the dot4
    matvec and the matrix-core kernel at every token count (never the K-split one)"""
    assert K.MODEL_PATHS["ckpt_v2_q80_gs16"] == dict(gs=16, matvec={48: K.MATVEC, 80: K.MATVEC}, gemm=K.GEMM_GENERIC)
    assert K.MODEL_PATHS["ckpt_v2_q80_gs8"] == dict(gs=8, matvec={72: K.MATVEC_GENERIC, 200: K.MATVEC_GENERIC}, gemm=K.GEMM_GENERIC)
    assert K.MODEL_PATHS["gs128"] == dict(gs=128, matvec={256: K.MATVEC, 640: K.MATVEC}, gemm=K.GEMM_MFMA)
    for which in MODELS:
        m = open_model(dev, golden_dir, which)
        try:
            assert_paths(dev, m, which)
        finally:
            m.free()


@functools.lru_cache(maxsize=None)
def stream_tokens(golden_dir, which):
    cfg = ref_parts(golden_dir, which)[0]
    rng = np.random.default_rng(cfg["dim"])
    return tuple([1] + [int(t) for t in rng.integers(0, cfg["vocab_size"], cfg["seq_len"] - 1)])


_STREAMS = {}


def stream_ref(golden_dir, which, m):
    """the reference run over stream_tokens, once per model: per position (logits, x), and the caches after the last one (a
    position's rows do not change once written)"""
    if which not in _STREAMS:
        ref = make_ref(golden_dir, which, m)
        snaps = []
        for pos, t in enumerate(stream_tokens(golden_dir, which)):
            ref.forward(t, pos)
            snaps.append((ref.s["logits"].copy(), ref.s["x"].copy()))
        c = ref.c
        shape = (c.n_layers, c.seq_len, c.dim)
        _STREAMS[which] = (snaps, ref.s["key_cache"].reshape(shape).copy(), ref.s["value_cache"].reshape(shape).copy())
    return _STREAMS[which]


def set_graph(dev, on):
    assert dev.lib.rama_set_graph_mode(dev.ctx, int(on)) == 0


# ------------------------------------------------------------------ forward and generate

@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_forward_every_position(dev, golden_dir, which, graph):
    import rama_amd
    m = open_model(dev, golden_dir, which)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        assert_paths(dev, m, which)
        ref = make_ref(golden_dir, which, m)
        eng.set_graph_mode(graph)
        token = 1
        for pos in range(ref.c.seq_len):
            ref.forward(token, pos)
            eng.forward(token, pos)
            check_state(eng, ref, pos)
            token = O.argmax(ref.s["logits"])
    finally:
        eng.set_graph_mode(0)
        eng.free(); m.free()


@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_generate_equals_the_reference_loop(dev, golden_dir, which, graph):
    import rama_amd
    from rama_amd.sampler_const import TOPP_U_CPU
    m = open_model(dev, golden_dir, which)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        assert_paths(dev, m, which)
        eng.set_graph_mode(graph)
        steps = m.cfg.seq_len
        assert eng.generate_greedy([], steps) == make_ref(golden_dir, which, m).generate([], steps)
        prompt = [5, 9, 33, 2]
        got = eng.generate(prompt, steps)
        assert got[:4] == prompt and got == make_ref(golden_dir, which, m).generate(prompt, steps)
        got = eng.generate([7], steps, temperature=1.0, topp=0.9)
        assert got == make_ref(golden_dir, which, m).generate([7], steps, 1.0, 0.9, TOPP_U_CPU)
    finally:
        eng.set_graph_mode(0)
        eng.free(); m.free()


# ------------------------------------------------------------------ prefill and decode batch

@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_prefill_against_the_per_position_reference(dev, golden_dir, which, graph):
    import rama_amd
    m = open_model(dev, golden_dir, which)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        assert_paths(dev, m, which)
        c = m.cfg
        S = c.seq_len
        toks = list(stream_tokens(golden_dir, which))
        snaps, kref, vref = stream_ref(golden_dir, which, m)
        eng.set_graph_mode(graph)
        for pos0, n in ((0, 2), (0, 3), (0, 17), (0, S - 3), (3, 5)):
            for b in ("key_cache", "value_cache"):
                eng.set_buffer(b, np.full(c.n_layers * S * c.dim, CH.SENTINEL))
            for p in range(pos0):                              # a forward history in front
                eng.forward(toks[p], p)
            eng.prefill(toks[pos0:pos0 + n], pos0)
            last = pos0 + n - 1
            assert same_bits(eng.logits(), snaps[last][0]), (pos0, n)
            assert same_bits(eng.buffer("x", c.dim), snaps[last][1]), (pos0, n)
            for got, want in zip(CH.cache(eng), (kref, vref)):
                assert same_bits(got[:, :last + 1], want[:, :last + 1]), (pos0, n)
                assert (got[:, last + 1:] == CH.SENTINEL).all(), (pos0, n)
    finally:
        eng.set_graph_mode(0)
        eng.free(); m.free()


@pytest.mark.parametrize("which", MODELS)
def test_decode_batch_against_the_reference(dev, golden_dir, which):
    """2, 17 and 33 sequences at mixed positions over caches written directly (each sequence its own): logits and the whole
    cache -- the new rows the reference's, every other row as it was"""
    import rama_amd
    from rama_amd.q8 import decode_batch
    m = open_model(dev, golden_dir, which)
    c = m.cfg
    S, kv = c.seq_len, c.n_layers * c.seq_len * c.dim
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(33)]
    try:
        assert_paths(dev, m, which)
        ref = make_ref(golden_dir, which, m)
        for n_seq in (2, 17, 33):
            rng = np.random.default_rng(n_seq)
            positions = [int(p) for p in rng.integers(0, S, n_seq)]
            positions[:2] = [0, S - 1]
            if n_seq > 2:
                positions[2:4] = [1, S // 2]
            tokens = [int(t) for t in rng.integers(0, c.vocab_size, n_seq)]
            data = (rng.standard_normal((n_seq, 2, kv)) * 0.5).astype(np.float32)
            for i in range(n_seq):
                engs[i].set_buffer("key_cache", data[i, 0]); engs[i].set_buffer("value_cache", data[i, 1])
                engs[i].set_buffer("logits", np.full(c.vocab_size, np.float32(-9.0)))
            decode_batch(engs[:n_seq], tokens, positions)
            for i in range(n_seq):
                ref.s["key_cache"][:] = data[i, 0]; ref.s["value_cache"][:] = data[i, 1]
                ref.forward(tokens[i], positions[i])
                assert same_bits(engs[i].logits(), ref.s["logits"]), (n_seq, i, positions[i])
                assert same_bits(engs[i].buffer("key_cache", kv), ref.s["key_cache"]), (n_seq, i, positions[i])
                assert same_bits(engs[i].buffer("value_cache", kv), ref.s["value_cache"]), (n_seq, i, positions[i])
                for l in range(c.n_layers):                    # (the reference did write the new rows)
                    o = (l * S + positions[i]) * c.dim
                    assert not np.array_equal(ref.s["key_cache"][o:o + c.dim], data[i, 0][o:o + c.dim])
    finally:
        for e in engs:
            e.free()
        m.free()


# ------------------------------------------------------------------ the chained batch and the serving chain

def chain_rows(rng, cfg, n_seq, n_steps):
    """greedy and sampled rows in turn at mixed positions, one with a forced prompt, one with a step budget"""
    S, V = cfg.seq_len, cfg.vocab_size
    seqs = []
    for i in range(n_seq):
        pos = [0, S - n_steps, 1, 3][i] if i < 4 else int(rng.integers(0, S - n_steps + 1))
        kw = dict(T=1.0, topp=0.9, u=float(rng.random() * 0.98)) if i % 2 else {}
        if i == 2:
            pos, kw["prompt"] = 0, [int(t) for t in rng.integers(0, V, 2)]
        seqs.append(CH.Seq(rng, cfg, pos, **kw))
    seqs[1].max_new = 3
    return seqs


@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_chained_batch_equals_solo_generate(dev, golden_dir, which, graph):
    m = open_model(dev, golden_dir, which)
    n_steps = 6
    all_seqs = []
    try:
        assert_paths(dev, m, which)
        for n_seq in (5, 19):
            seqs = chain_rows(np.random.default_rng(n_seq + graph), m.cfg, n_seq, n_steps)
            all_seqs += seqs
            for s in seqs:
                s.prepare(dev, m)
            solo = [s.solo(n_steps) for s in seqs]
            k = CH.stop_index(solo[0], 0)                      # sequence 0 stops on a token of its own run
            seqs[0].stop = solo[0][k]
            want = [CH.expected(solo[i], len(s.prompt), s.max_new, s.stop, n_steps) for i, s in enumerate(seqs)]
            assert len(want[1]) == 3 and want[2][:2] == seqs[2].prompt and (k == 0 or len(want[0]) == k + 1)
            ends = [s.pos + len(w) for s, w in zip(seqs, want)]
            for s, e in zip(seqs, ends):
                CH.fill_behind(s.eng, e)
            set_graph(dev, graph)
            assert CH.begin(dev, m, seqs, n_steps) == 0
            assert CH.steps(dev, 2) == 0 and CH.steps(dev, n_steps - 2) == 0
            assert CH.tokens(dev, n_seq, n_steps) == want, (which, graph, n_seq)
            set_graph(dev, 0)
            for i, s in enumerate(seqs):
                CH.check_cache_rows(s, ends[i], (which, graph, n_seq, i))
                assert CH.holds_sentinel(s.eng, ends[i]), (which, graph, n_seq, i)      # nothing behind its last position
    finally:
        set_graph(dev, 0)
        for s in all_seqs:
            s.free()
        m.free()


@pytest.mark.parametrize("which", MODELS)
@pytest.mark.parametrize("graph", [0, 1])
def test_serving_chain_equals_solo_generate(dev, golden_dir, which, graph):
    """6 requests over 4 slots, 8 rows a step: greedy and sampled plans, a context longer than a step's rows, a stop token, budgets"""
    from rama_amd.q8 import Q8Server
    m = open_model(dev, golden_dir, which)
    S = m.cfg.seq_len
    sizes = [(1, 6), (3, 4), (11, 5), (2, 7), (S - 9, 4), (5, 3)]
    reqs, srv = [], None
    try:
        assert_paths(dev, m, which)
        reqs = SV.mixed_requests(dev, m, np.random.default_rng(40 + graph), sizes)
        assert any(r.stop >= 0 for r in reqs) and any(r.T > 0 for r in reqs)
        for r in reqs:
            r.solo()
        set_graph(dev, graph)
        srv = Q8Server(m, 4, 8, max(s[1] for s in sizes))
        hs = [srv.submit(r.ctx, r.max_new, r.T, r.topp, r.u, stop_token=r.stop if r.stop >= 0 else None, engine=r.eng) for r in reqs]
        srv.run()
        assert srv.stats()["graph_captures"] == (1 if graph else 0)
        for i, (h, r) in enumerate(zip(hs, reqs)):
            assert srv.finished(h)
            r.check(srv.result(h), (which, graph, i))         # tokens, every cache row, the sentinel behind the last one
    finally:
        if srv is not None:
            srv.close()
        set_graph(dev, 0)
        for r in reqs:
            r.free()
        m.free()


# ------------------------------------------------------------------ a context too long for the chain attention

def test_longctx_seq_len_is_the_first_the_batch_pass_refuses(dev, golden_dir):
    from rama_amd._lib import rama_config
    ok = lambda S: dev.lib.rama_q8_batch_shape_ok(C.byref(rama_config(64, 192, 1, 2, 2, 64, S, 1)))
    first = next(S for S in range(1024, 64 * 1024, 1024) if ok(S) != 1)
    assert first == K.LONGCTX_SEQ_LEN == K.LONGCTX_CFG["seq_len"] and ok(first) == 0
    assert ok(K.LONGCTX_DEEP_SEQ_LEN) == 0 and ok(K.LONGCTX_REFUSED_SEQ_LEN) == 0
    assert K.LONGCTX_DEEP_POS == K.LONGCTX_DEEP_SEQ_LEN - 1 == 16383


def test_context_longer_than_the_reference_attention_is_unsupported(dev, golden_dir):
    """past 16384 positions neither attention takes the model: the forward says so and leaves the logits alone"""
    import rama_amd
    cfg = dict(K.LONGCTX_CFG, seq_len=K.LONGCTX_REFUSED_SEQ_LEN)
    m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), K.LONGCTX_GS, K.LONGCTX_SEED)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        eng.set_buffer("logits", np.full(cfg["vocab_size"], np.float32(-9.0)))
        rc = dev.lib.rama_q8_forward(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state), 1, 0)
        assert rc == EUNSUP
        assert (eng.logits() == np.float32(-9.0)).all()
    finally:
        eng.free(); m.free()


@pytest.mark.parametrize("which,deep", [("longctx", K.LONGCTX_SEQ_LEN - 150), ("longctx_deep", K.LONGCTX_DEEP_POS)])
def test_longctx_forward(dev, golden_dir, which, deep):
    """positions 0, 1, 3 and a deep one behind rows written directly, through launch_attention_ref; the second model is the
    longest context that kernel takes, at its last position"""
    import rama_amd
    m = open_model(dev, golden_dir, which)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        assert batch_shape_ok(dev, m) == 0
        assert dev.lib.rama_q8_product_path(64, 32, 0, 1) == K.MATVEC and dev.lib.rama_q8_product_path(192, 32, 0, 1) == K.MATVEC
        ref = make_ref(golden_dir, which, m)
        d = m.cfg.dim
        rng = np.random.default_rng(2)
        for pos, token in ((0, 1), (1, 17), (3, 40), (deep, 23)):
            if pos > 3:
                kv = (rng.standard_normal((2, pos, d)) * 0.5).astype(np.float32)
                ref.s["key_cache"][:pos * d] = kv[0].reshape(-1)
                ref.s["value_cache"][:pos * d] = kv[1].reshape(-1)
                eng.set_buffer("key_cache", kv[0]); eng.set_buffer("value_cache", kv[1])
            ref.forward(token, pos)
            eng.forward(token, pos)
            check_state(eng, ref, pos)
    finally:
        eng.free(); m.free()


def test_longctx_prefill_and_decode_batch_fall_back_to_forwards(dev, golden_dir):
    import rama_amd
    from rama_amd.q8 import decode_batch
    m = open_model(dev, golden_dir, "longctx")
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(4)]
    try:
        assert batch_shape_ok(dev, m) == 0
        c = m.cfg
        ref = make_ref(golden_dir, "longctx", m)
        eng, twin = engs[0], engs[1]
        toks = [1, 9, 33, 2, 60]
        eng.prefill(toks, 0)
        for p, t in enumerate(toks):
            twin.forward(t, p); ref.forward(t, p)
        for e in (eng, twin):
            assert same_bits(e.logits(), ref.s["logits"]) and same_bits(e.buffer("x", c.dim), ref.s["x"])
            for name in ("key_cache", "value_cache"):
                assert same_bits(e.buffer(name, 5 * c.dim), ref.s[name][:5 * c.dim]), name
        # three sequences, each behind the same five rows: positions 5, 2 (a row rewritten) and 0
        engs[2].prefill(toks, 0)
        tokens, positions = [7, 8, 3], [5, 2, 0]
        decode_batch([eng, engs[2], engs[3]], tokens, positions)
        for e, t, p in zip((eng, engs[2], engs[3]), tokens, positions):
            r = make_ref(golden_dir, "longctx", m)
            for q, tk in enumerate(toks if p else []):
                r.forward(tk, q)
            r.forward(t, p)
            assert same_bits(e.logits(), r.s["logits"]), p
            for name in ("key_cache", "value_cache"):
                assert same_bits(e.buffer(name, c.dim, p * c.dim), r.cache_row(name, 0, p)), (p, name)
        twin.forward(7, 5)
        assert same_bits(eng.logits(), twin.logits())
    finally:
        for e in engs:
            e.free()
        m.free()


@pytest.mark.parametrize("graph", [0, 1])
def test_longctx_is_refused_by_the_chains_which_carry_on(dev, golden_dir, graph):
    """rama_q8_decode_batch_begin and rama_q8_serve_begin answer RAMA_EUNSUP; a chained batch and a serving chain running on
    ckpt_v2_q80_untied in the same context give the tokens of their solo runs afterwards"""
    import rama_amd
    from rama_amd._lib import rama_run_state
    m = SV.open_model(dev, golden_dir, "ckpt_v2_q80_untied")
    lm = open_model(dev, golden_dir, "longctx")
    leng = rama_amd.Q8Engine(dev, lm)
    rng = np.random.default_rng(17 + graph)
    n_steps = 8
    seqs = [CH.Seq(rng, m.cfg, 0), CH.Seq(rng, m.cfg, 3, T=1.0, topp=0.9, u=0.4), CH.Seq(rng, m.cfg, 5)]
    reqs = []
    try:
        assert batch_shape_ok(dev, lm) == 0 and batch_shape_ok(dev, m) == 1
        for s in seqs:
            s.prepare(dev, m)
        set_graph(dev, graph)
        assert CH.begin(dev, m, seqs, n_steps) == 0 and CH.steps(dev, 3) == 0
        states = (rama_run_state * 1)(leng.state)
        one = (C.c_int32 * 1)(1)
        zero = (C.c_int32 * 1)(0)
        assert dev.lib.rama_q8_decode_batch_begin(dev.ctx, C.byref(lm.ccfg), C.byref(lm.weights), states, one, zero, 1, 4, None) == EUNSUP
        assert CH.steps(dev, n_steps - 3) == 0
        assert CH.tokens(dev, len(seqs), n_steps) == [s.solo(n_steps) for s in seqs]
        for i, s in enumerate(seqs):
            CH.check_cache_rows(s, s.pos + n_steps, (graph, i))
        reqs = [SV.Req(dev, m, rng, 4, 7, 1.0, 0.9, 0.3), SV.Req(dev, m, rng, 9, 5)]
        for r in reqs:
            r.solo()
        assert SV.begin(dev, m, 2, 4, 8) == 0
        for i, r in enumerate(reqs):
            assert SV.admit(dev, i, r) == 0
        assert SV.steps(dev, 2) == 0
        assert SV.begin(dev, lm, 2, 4, 8) == EUNSUP
        SV.run_until_done(dev, [0, 1])
        for i, r in enumerate(reqs):
            r.check(SV.tokens(dev, i), (graph, i))
    finally:
        set_graph(dev, 0)
        dev.lib.rama_q8_serve_end(dev.ctx)
        for s in seqs:
            s.free()
        for r in reqs:
            r.free()
        leng.free(); lm.free(); m.free()
