"""Q8 token batches on the GPU (rama_q8_matmul_batch, rama_q8_prefill, rama_q8_decode_batch): bit for bit against
tests/q8_ref.py and against the single-token rama_q8_forward."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import q8_ref as R
from tests.test_hip_q8 import FIXTURES, Buf, model_and_ref, same_bits

pytestmark = pytest.mark.gpu

EINVAL = -1
STORIES15M = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=256, shared_weight=True)


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


# ------------------------------------------------------------------ the product

def q8_data(rng, n, d, gs, n_tok):
    """asymmetric int8 weights with +-127 rows, activations quantized per token (one all-zero token: scales 0)"""
    wq = rng.integers(-127, 128, size=d * n, dtype=np.int8)
    ws = (rng.random(d * n // gs, dtype=np.float32) * np.float32(0.02) - np.float32(0.004)).astype(np.float32)
    if d >= 4:
        wq[:n] = 127                                      # saturated rows
        wq[n:2 * n] = -127
        wq[3 * n:4 * n] = 0                               # an all-zero row: +0.0
    x = (rng.standard_normal((n_tok, n)) * rng.choice([1e-2, 1.0, 30.0], size=(n_tok, 1))).astype(np.float32)
    x[:, 0] = np.float32(50.0)                            # a +127 activation in every token's first group
    if n_tok > 2:
        x[1] = 0.0
    qs = [R.quantize(x[t], gs) for t in range(n_tok)]
    xq = np.concatenate([q for q, _ in qs])
    xs = np.concatenate([s for _, s in qs])
    return wq, ws, xq, xs


def dev_matmul_batch(dev, wq, ws, xq, xs, n, d, gs, n_tok):
    bw, bs, bx, bxs = Buf(dev, wq), Buf(dev, ws), Buf(dev, xq), Buf(dev, xs)
    o = Buf(dev, np.full(d * n_tok, np.float32(7.0)))
    rc = dev.lib.rama_q8_matmul_batch(dev.ctx, o.p, bw.p, bs.p, bx.p, bxs.p, n, d, gs, n_tok)
    out = o.get(np.float32, d * n_tok).reshape(n_tok, d)
    for b in (bw, bs, bx, bxs, o):
        b.free()
    assert rc == 0
    return out


def check_rows(got, xq, xs, wq, ws, n, gs):
    G = n // gs
    for t in range(got.shape[0]):
        want = R.matmul(xq[t * n:(t + 1) * n], xs[t * G:(t + 1) * G], wq, ws, gs)
        assert same_bits(got[t], want), (t, np.flatnonzero(got[t].view(np.uint32) != want.view(np.uint32))[:8])


# (n, d, gs): the matrix-core kernel at GS 32 (K = 32 mod 64 too), 64, 128, 256 with ragged rows; the bytewise kernel at
# GS 48 and at K % 16 != 0; one group in one half-filled chunk; one group of 64 chunks (the largest the matrix-core kernel
# takes) and one of 128 (bytewise)
SHAPES = [(256, 40, 32), (288, 37, 32), (512, 48, 64), (768, 33, 128), (1024, 64, 256), (4096, 19, 64), (96, 20, 48), (40, 9, 8),
          (32, 20, 32), (4096, 17, 4096), (8192, 17, 8192)]


@pytest.mark.parametrize("n,d,gs", SHAPES)
def test_matmul_batch_bit_identical(dev, n, d, gs):
    rng = np.random.default_rng(n * 31 + d)
    wq, ws, xq, xs = q8_data(rng, n, d, gs, 130)
    for n_tok in (1, 2, 15, 16, 17, 64, 128, 130):
        got = dev_matmul_batch(dev, wq, ws, xq[:n_tok * n], xs[:n_tok * (n // gs)], n, d, gs, n_tok)
        check_rows(got, xq, xs, wq, ws, n, gs)
        if n_tok > 2:
            assert not got[1].view(np.uint32).any()      # zero activations: every row +0.0
        if d >= 4:
            assert not got[:, 3].view(np.uint32).any()


def test_new_shapes_take_the_paths_they_are_there_for(dev):
    from tests.q8_offlane_cases import GEMM_GENERIC, GEMM_KSPLIT, GEMM_MFMA
    P = dev.lib.rama_q8_product_path
    assert [P(32, 32, t, 1) for t in (1, 17, 64, 130)] == [GEMM_KSPLIT, GEMM_KSPLIT, GEMM_MFMA, GEMM_MFMA]
    assert [P(4096, 4096, t, 1) for t in (1, 17, 64, 130)] == [GEMM_MFMA] * 4
    assert [P(8192, 8192, t, 1) for t in (1, 17, 64, 130)] == [GEMM_GENERIC] * 4


@pytest.mark.parametrize("n,d,gs,n_tok", [(512, 48, 64, 17), (512, 48, 64, 40)])
def test_matmul_batch_misaligned_weights_or_activations(dev, n, d, gs, n_tok):
    """weights or activations 4 bytes off a 16-byte boundary: the bytewise kernel instead of the K-split (17 tokens) or the
    matrix-core kernel (40), the same bits as the aligned call and the reference, nothing written outside o"""
    from tests.q8_offlane_cases import GEMM_GENERIC, GEMM_KSPLIT, GEMM_MFMA
    P = dev.lib.rama_q8_product_path
    assert P(n, gs, n_tok, 1) == (GEMM_KSPLIT if n_tok <= 32 else GEMM_MFMA) and P(n, gs, n_tok, 0) == GEMM_GENERIC
    wq, ws, xq, xs = q8_data(np.random.default_rng(n + n_tok), n, d, gs, n_tok)

    def lead(a, k):
        return np.concatenate([np.full(k, 0x55, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1)])

    aligned = None
    for w_lead, x_lead in ((0, 0), (4, 0), (0, 4)):
        bw, bs, bx, bxs = Buf(dev, lead(wq, w_lead)), Buf(dev, ws), Buf(dev, lead(xq, x_lead)), Buf(dev, xs)
        o = Buf(dev, np.full(d * n_tok + 8, np.float32(7.0)))
        rc = dev.lib.rama_q8_matmul_batch(dev.ctx, o.p + 16, bw.p + w_lead, bs.p, bx.p + x_lead, bxs.p, n, d, gs, n_tok)
        out = o.get(np.float32, d * n_tok + 8)
        for b in (bw, bs, bx, bxs, o):
            b.free()
        assert rc == 0
        assert (out[:4] == np.float32(7.0)).all() and (out[-4:] == np.float32(7.0)).all(), (w_lead, x_lead)
        got = out[4:-4].reshape(n_tok, d)
        check_rows(got, xq, xs, wq, ws, n, gs)
        aligned = got if aligned is None else aligned
        assert same_bits(got, aligned), (w_lead, x_lead)


def test_matmul_batch_equals_single_token_calls(dev):
    n, d, gs, n_tok = 2048, 300, 64, 33
    rng = np.random.default_rng(9)
    wq, ws, xq, xs = q8_data(rng, n, d, gs, n_tok)
    got = dev_matmul_batch(dev, wq, ws, xq, xs, n, d, gs, n_tok)
    bw, bs, o = Buf(dev, wq), Buf(dev, ws), Buf(dev, nbytes=4 * d)
    try:
        G = n // gs
        for t in range(n_tok):
            bx, bxs = Buf(dev, xq[t * n:(t + 1) * n]), Buf(dev, xs[t * G:(t + 1) * G])
            assert dev.lib.rama_q8_matmul(dev.ctx, o.p, bw.p, bs.p, bx.p, bxs.p, n, d, gs) == 0
            assert same_bits(got[t], o.get(np.float32, d)), t
            bx.free(); bxs.free()
    finally:
        for b in (bw, bs, o):
            b.free()


def test_matmul_batch_negative_zero_terms_start_from_plus_zero(dev):
    """row 0's terms are all -0.0 for every token: the +0.0 start gives +0.0 (see test_hip_q8)"""
    for gs, n in ((32, 64), (64, 128), (32, 96)):
        n_tok = 20
        x = np.full((n_tok, n), 0.5, np.float32)
        x[5] = 2.0
        qs = [R.quantize(x[t], gs) for t in range(n_tok)]
        xq, xs = np.concatenate([q for q, _ in qs]), np.concatenate([s for _, s in qs])
        G = n // gs
        wq = np.ones(3 * n, np.int8)
        ws = np.concatenate([np.full(G, -0.0, np.float32), np.array([0.25, -0.0, 1e-3][:G] + [0.5] * max(0, G - 3), np.float32),
                             np.full(G, -0.0, np.float32)])
        ws[-1] = 1e-3
        got = dev_matmul_batch(dev, wq, ws, xq, xs, n, 3, gs, n_tok)
        check_rows(got, xq, xs, wq, ws, n, gs)
        assert not got[:, 0].view(np.uint32).any()


def test_matmul_batch_einval(dev):
    o = Buf(dev, np.full(64, np.float32(3.0)))
    w = Buf(dev, np.zeros(64 * 64, np.int8))
    s = Buf(dev, np.ones(64, np.float32))
    L = dev.lib
    try:
        assert L.rama_q8_matmul_batch(dev.ctx, o.p, w.p, s.p, w.p, s.p, 64, 1, 64, 0) == EINVAL
        assert L.rama_q8_matmul_batch(dev.ctx, o.p, w.p, s.p, w.p, s.p, 64, 1, 64, -3) == EINVAL
        assert L.rama_q8_matmul_batch(dev.ctx, None, w.p, s.p, w.p, s.p, 64, 1, 64, 1) == EINVAL
        assert L.rama_q8_matmul_batch(dev.ctx, o.p, w.p, s.p, w.p, s.p, 96, 1, 64, 1) == EINVAL
        assert (o.get(np.float32, 64) == np.float32(3.0)).all()
    finally:
        for b in (o, w, s):
            b.free()


# ------------------------------------------------------------------ prefill

def make_ref(golden_dir, name, m):
    cfg, gs, _, norms, t = R.read_v2(golden_dir / f"{name}.bin")
    return R.Q8Ref(cfg, gs, norms, t, (m.tensor("freq_cis_real"), m.tensor("freq_cis_imag")))


def full_state(eng):
    c = eng.cfg
    kv = c.n_layers * c.seq_len * c.dim
    return {n: eng.buffer(n, k) for n, k in (("key_cache", kv), ("value_cache", kv), ("x", c.dim), ("logits", c.vocab_size))}


@pytest.mark.parametrize("name,gs", FIXTURES)
@pytest.mark.parametrize("graph", [0, 1])
def test_prefill_fixture(dev, golden_dir, name, gs, graph):
    import rama_amd
    m, _ = model_and_ref(dev, golden_dir, name)
    eng, twin = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, m)
    try:
        eng.set_graph_mode(graph)
        c = m.cfg
        S = c.seq_len
        rng = np.random.default_rng(S)
        for pos0, n in ((0, 1), (0, 2), (0, 5), (0, S), (3, 1), (3, 2), (4, S - 6), (S - 2, 2)):
            ref = make_ref(golden_dir, name, m)
            for e in (eng, twin):
                for b in ("key_cache", "value_cache"):
                    e.set_buffer(b, np.zeros(c.n_layers * S * c.dim, np.float32))
            hist = [int(t) for t in rng.integers(0, c.vocab_size, pos0)]
            toks = [int(t) for t in rng.integers(0, c.vocab_size, n)]
            for p, t in enumerate(hist):                     # a forward history in front
                eng.forward(t, p); twin.forward(t, p); ref.forward(t, p)
            eng.prefill(toks, pos0)
            for i, t in enumerate(toks):
                twin.forward(t, pos0 + i); ref.forward(t, pos0 + i)
            got, want = full_state(eng), full_state(twin)
            for k in got:
                assert same_bits(got[k], want[k]), (pos0, n, k)
            assert same_bits(got["logits"], ref.s["logits"]) and same_bits(got["x"], ref.s["x"]), (pos0, n)
            for l in range(c.n_layers):
                for p in range(pos0 + n):
                    o = (l * S + p) * c.dim
                    assert same_bits(got["key_cache"][o:o + c.dim], ref.cache_row("key_cache", l, p)), (pos0, n, l, p)
                    assert same_bits(got["value_cache"][o:o + c.dim], ref.cache_row("value_cache", l, p)), (pos0, n, l, p)
            if pos0 + n < S:                                 # decoding on after the prompt
                nxt = O.argmax(ref.s["logits"])
                eng.forward(nxt, pos0 + n); twin.forward(nxt, pos0 + n); ref.forward(nxt, pos0 + n)
                assert same_bits(eng.logits(), twin.logits()) and same_bits(eng.logits(), ref.s["logits"]), (pos0, n)
    finally:
        eng.free(); twin.free(); m.free()


def test_prefill_stories15m_shape_200_positions(dev):
    """GS 32, 200 prompt positions: two weight passes (128 + 71) and the last position as forward()"""
    import rama_amd
    m = rama_amd.Q8Model.synth(dev, O.Config(**STORIES15M), 32, 11)
    eng, twin = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, m)
    try:
        rng = np.random.default_rng(1)
        toks = [1] + [int(t) for t in rng.integers(0, 32000, 199)]
        eng.prefill(toks, 0)
        for p, t in enumerate(toks):
            twin.forward(t, p)
        got, want = full_state(eng), full_state(twin)
        for k in got:
            assert same_bits(got[k], want[k]), k
        nxt = O.argmax(want["logits"])
        eng.forward(nxt, 200); twin.forward(nxt, 200)
        assert same_bits(eng.logits(), twin.logits())
        # a second prompt behind it, from position 201
        more = [int(t) for t in rng.integers(0, 32000, 40)]
        eng.prefill(more, 201)
        for i, t in enumerate(more):
            twin.forward(t, 201 + i)
        got, want = full_state(eng), full_state(twin)
        for k in got:
            assert same_bits(got[k], want[k]), k
    finally:
        eng.free(); twin.free(); m.free()


def test_prefill_7b_shape_one_layer_around_1024(dev):
    """one llama2-7B-shaped layer (GS 64), a prompt over positions 1000 .. 1039 behind a cache written directly"""
    import rama_amd
    cfg = dict(dim=4096, hidden_dim=11008, n_layers=1, n_heads=32, n_kv_heads=32, vocab_size=32000, seq_len=2048, shared_weight=False)
    m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), 64, 5)
    eng, twin = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, m)
    try:
        rng = np.random.default_rng(0)
        d, pos0, n = cfg["dim"], 1000, 40
        kv = (rng.standard_normal((2, pos0, d)) * 0.5).astype(np.float32)
        for e in (eng, twin):
            e.set_buffer("key_cache", kv[0]); e.set_buffer("value_cache", kv[1])
        toks = [int(t) for t in rng.integers(0, 32000, n)]
        eng.prefill(toks, pos0)
        for i, t in enumerate(toks):
            twin.forward(t, pos0 + i)
        got, want = full_state(eng), full_state(twin)
        for k in got:
            assert same_bits(got[k], want[k]), k
    finally:
        eng.free(); twin.free(); m.free()


# ------------------------------------------------------------------ decode batch

def fill_history(engs, rng, cfg):
    """the same random cache contents (history rows and sentinel rows behind them) in every engine of a group"""
    kv = cfg.n_layers * cfg.seq_len * cfg.dim
    data = (rng.standard_normal((2, kv)) * 0.5).astype(np.float32)
    for e in engs:
        e.set_buffer("key_cache", data[0]); e.set_buffer("value_cache", data[1])


def run_decode_batch_case(dev, m, n_seq, seed, real_history=0):
    import rama_amd
    from rama_amd.q8 import decode_batch
    c = m.cfg
    rng = np.random.default_rng(seed)
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(n_seq)]
    twins = [rama_amd.Q8Engine(dev, m) for _ in range(n_seq)]
    try:
        positions = [int(p) for p in rng.integers(0, c.seq_len, n_seq)]
        positions[0] = 0
        if n_seq > 1:
            positions[-1] = c.seq_len - 1
        tokens = [int(t) for t in rng.integers(0, c.vocab_size, n_seq)]
        for i in range(n_seq):
            fill_history((engs[i], twins[i]), rng, c)
            for p in range(min(real_history, positions[i])):     # a real forward history for the first rows
                t = int(rng.integers(0, c.vocab_size))
                engs[i].forward(t, p); twins[i].forward(t, p)
            engs[i].set_buffer("logits", np.full(c.vocab_size, np.float32(-9.0)))
        decode_batch(engs, tokens, positions)
        for i in range(n_seq):
            twins[i].forward(tokens[i], positions[i])
        for i in range(n_seq):
            for k in ("key_cache", "value_cache"):
                n = c.n_layers * c.seq_len * c.dim
                assert same_bits(engs[i].buffer(k, n), twins[i].buffer(k, n)), (n_seq, i, k)
            assert same_bits(engs[i].logits(), twins[i].logits()), (n_seq, i, positions[i])
    finally:
        for e in engs + twins:
            e.free()


@pytest.mark.parametrize("name,gs", FIXTURES)
@pytest.mark.parametrize("n_seq", [1, 2, 17, 128])
def test_decode_batch_fixture(dev, golden_dir, name, gs, n_seq):
    m, _ = model_and_ref(dev, golden_dir, name)
    try:
        run_decode_batch_case(dev, m, n_seq, n_seq * 7 + gs, real_history=3 if n_seq <= 17 else 0)
    finally:
        m.free()


def test_decode_batch_fixture_against_reference(dev, golden_dir):
    """two sequences with real histories: logits and appended rows equal Q8Ref's"""
    import rama_amd
    from rama_amd.q8 import decode_batch
    name = "ckpt_v2_q80_untied"
    m, _ = model_and_ref(dev, golden_dir, name)
    refs = [make_ref(golden_dir, name, m) for _ in range(2)]
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(2)]
    try:
        hist = ([1, 5, 9, 11, 3], [1, 40])
        for e, r, h in zip(engs, refs, hist):
            for p, t in enumerate(h):
                e.forward(t, p); r.forward(t, p)
        toks, poss = [7, 8], [len(h) for h in hist]
        decode_batch(engs, toks, poss)
        for e, r, t, p in zip(engs, refs, toks, poss):
            r.forward(t, p)
            assert same_bits(e.logits(), r.s["logits"])
            c = r.c
            for l in range(c.n_layers):
                o = (l * c.seq_len + p) * c.dim
                assert same_bits(e.buffer("key_cache", c.dim, o), r.cache_row("key_cache", l, p))
                assert same_bits(e.buffer("value_cache", c.dim, o), r.cache_row("value_cache", l, p))
    finally:
        for e in engs:
            e.free()
        m.free()


def test_decode_batch_stories15m_shape(dev):
    import rama_amd
    m = rama_amd.Q8Model.synth(dev, O.Config(**STORIES15M), 32, 11)
    try:
        run_decode_batch_case(dev, m, 17, 3)
    finally:
        m.free()


# ------------------------------------------------------------------ argument errors leave every state as it was

def test_errors_leave_states_untouched(dev, golden_dir):
    import rama_amd
    from rama_amd._lib import rama_run_state
    m, _ = model_and_ref(dev, golden_dir, "ckpt_v2_q80_untied")
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(3)]
    L, c = dev.lib, m.cfg
    try:
        rng = np.random.default_rng(4)
        for e in engs:
            fill_history((e,), rng, c)
            e.set_buffer("logits", rng.standard_normal(c.vocab_size).astype(np.float32))
            e.set_buffer("x", rng.standard_normal(c.dim).astype(np.float32))
        before = [full_state(e) for e in engs]
        cfg, w = C.byref(m.ccfg), C.byref(m.weights)

        def states(*idx):
            return (rama_run_state * len(idx))(*[engs[i].state for i in idx])

        def arr(v):
            return (C.c_int32 * max(len(v), 1))(*v)

        S, V = c.seq_len, c.vocab_size
        db = L.rama_q8_decode_batch
        assert db(dev.ctx, cfg, w, None, arr([1]), arr([0]), 1) == EINVAL
        assert db(dev.ctx, cfg, w, states(0), None, arr([0]), 1) == EINVAL
        assert db(dev.ctx, cfg, w, states(0), arr([1]), None, 1) == EINVAL
        assert db(dev.ctx, None, w, states(0), arr([1]), arr([0]), 1) == EINVAL
        assert db(dev.ctx, cfg, None, states(0), arr([1]), arr([0]), 1) == EINVAL
        assert db(dev.ctx, cfg, w, states(0), arr([1]), arr([0]), 0) == EINVAL
        big = (rama_run_state * 129)(*([engs[0].state] * 129))
        assert db(dev.ctx, cfg, w, big, arr([1] * 129), arr([0] * 129), 129) == EINVAL
        assert db(dev.ctx, cfg, w, states(0, 1), arr([1, V]), arr([0, 0]), 2) == EINVAL
        assert db(dev.ctx, cfg, w, states(0, 1), arr([-1, 1]), arr([0, 0]), 2) == EINVAL
        assert db(dev.ctx, cfg, w, states(0, 1), arr([1, 1]), arr([0, S]), 2) == EINVAL
        assert db(dev.ctx, cfg, w, states(0, 1), arr([1, 1]), arr([-1, 0]), 2) == EINVAL
        assert db(dev.ctx, cfg, w, states(0, 1, 0), arr([1, 1, 1]), arr([0, 1, 2]), 3) == EINVAL
        pf = L.rama_q8_prefill
        s0 = C.byref(engs[2].state)
        assert pf(dev.ctx, cfg, w, None, arr([1, 2]), 2, 0) == EINVAL
        assert pf(dev.ctx, cfg, w, s0, None, 2, 0) == EINVAL
        assert pf(dev.ctx, None, w, s0, arr([1, 2]), 2, 0) == EINVAL
        assert pf(dev.ctx, cfg, w, s0, arr([1, 2]), 0, 0) == EINVAL
        assert pf(dev.ctx, cfg, w, s0, arr([1, 2]), 2, -1) == EINVAL
        assert pf(dev.ctx, cfg, w, s0, arr([1, 2]), 2, S - 1) == EINVAL
        assert pf(dev.ctx, cfg, w, s0, arr([1] * (S + 1)), S + 1, 0) == EINVAL
        assert pf(dev.ctx, cfg, w, s0, arr([1, V]), 2, 0) == EINVAL
        assert pf(dev.ctx, cfg, w, s0, arr([-1, 1]), 2, 0) == EINVAL
        for e, b in zip(engs, before):
            a = full_state(e)
            for k in a:
                assert same_bits(a[k], b[k]), k
        # and the wrappers refuse the same before any call
        from rama_amd.q8 import decode_batch
        with pytest.raises(ValueError):
            decode_batch([engs[0], engs[0]], [1, 1], [0, 1])
        with pytest.raises(ValueError):
            engs[0].prefill([1, 2], S - 1)
    finally:
        for e in engs:
            e.free()
        m.free()
