"""Q8_0 (llama2.c version-2) models on the GPU, bit for bit against the numpy restatement of tests/q8_ref.py."""
import ctypes as C
import struct

import numpy as np
import pytest

from oracle import oracle as O
from oracle import synth as S
from tests import q8_ref as R

pytestmark = pytest.mark.gpu

FIXTURES = [("ckpt_v2_q80_tied", 32), ("ckpt_v2_q80_untied", 64)]


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


class Buf:
    """a device allocation filled from / read back into a numpy array of any 4-byte-multiple size"""

    def __init__(self, dev, a=None, nbytes=None):
        from rama_amd._lib import check
        self.dev, self.check = dev, check
        nbytes = a.nbytes if a is not None else nbytes
        self.nbytes = nbytes
        p = C.c_void_p()
        check(dev.lib.rama_alloc_f32(dev.ctx, (nbytes + 3) // 4, C.byref(p)))
        self.p = p.value
        if a is not None:
            b = np.zeros((nbytes + 3) // 4 * 4, np.uint8)
            b[:nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            check(dev.lib.rama_copy_h2d_f32(dev.ctx, self.p, b.ctypes.data, b.size // 4))

    def get(self, dtype, n):
        b = np.empty((self.nbytes + 3) // 4 * 4, np.uint8)
        self.check(self.dev.lib.rama_download_f32(self.dev.ctx, self.p, b.size // 4, b.ctypes.data))
        return b[:np.dtype(dtype).itemsize * n].view(dtype).copy()

    def free(self):
        self.check(self.dev.lib.rama_free(self.dev.ctx, self.p))


def dev_quantize(dev, x, gs):
    xb = Buf(dev, x)
    q, s = Buf(dev, nbytes=x.size), Buf(dev, nbytes=4 * (x.size // gs))
    rc = dev.lib.rama_q8_quantize(dev.ctx, xb.p, x.size, gs, q.p, s.p)
    out = (rc, q.get(np.int8, x.size), s.get(np.float32, x.size // gs)) if rc == 0 else (rc, None, None)
    for b in (xb, q, s):
        b.free()
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("n", [288, 768, 2048, 4096, 11008])
def test_quantize_bit_identical(dev, n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 40.0], size=n)).astype(np.float32)
    for gs in (32, 64):
        if n % gs:
            continue
        rc, q, s = dev_quantize(dev, x, gs)
        assert rc == 0
        wq, ws = R.quantize(x, gs)
        assert np.array_equal(q, wq) and same_bits(s, ws), (n, gs)


def test_quantize_edge_cases_and_bad_group(dev):
    gs = 32
    x = np.zeros(6 * gs, np.float32)
    x[0] = 127.0
    x[1:9] = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, -126.5]     # ties -> away from zero
    x[gs + 3] = -3.0                                              # one-hot
    x[2 * gs] = np.float32(1e-40); x[2 * gs + 1] = np.float32(-5e-41)   # denormals
    x[4 * gs:5 * gs] = np.linspace(-1, 1, gs, dtype=np.float32) * np.float32(1e-39)
    # group 3 and 5 stay all zero
    rc, q, s = dev_quantize(dev, x, gs)
    assert rc == 0
    wq, ws = R.quantize(x, gs)
    assert np.array_equal(q, wq) and same_bits(s, ws)
    assert q[:9].tolist() == [127, 1, -1, 2, -2, 3, -3, 127, -127] and q[gs + 3] == -127
    assert not q[3 * gs:4 * gs].any() and s[3] == 0
    assert dev.lib.rama_q8_quantize(dev.ctx, 0, 100, 32, 0, 0) == -1
    rc, _, _ = dev_quantize(dev, np.ones(96, np.float32), 64)      # 64 does not divide 96
    assert rc == -1


def dev_matmul(dev, wq, ws, xq, xs, n, d, gs):
    bw, bs, bx, bxs = Buf(dev, wq), Buf(dev, ws), Buf(dev, xq), Buf(dev, xs)
    o = Buf(dev, nbytes=4 * d)
    rc = dev.lib.rama_q8_matmul(dev.ctx, o.p, bw.p, bs.p, bx.p, bxs.p, n, d, gs)
    assert rc == 0
    out = o.get(np.float32, d)
    for b in (bw, bs, bx, bxs, o):
        b.free()
    return out


@pytest.mark.parametrize("d,n,gs", [(4096, 4096, 64), (11008, 4096, 64), (4096, 11008, 64), (32000, 4096, 64),
                                    (768, 288, 32), (2048, 768, 64), (288, 768, 32), (37, 4096, 64), (1001, 288, 32), (5, 96, 32)])
def test_matmul_bit_identical(dev, d, n, gs):
    rng = np.random.default_rng(d * 7 + n)
    wq = rng.integers(-127, 128, size=d * n, dtype=np.int8)
    ws = (rng.random(d * n // gs, dtype=np.float32) * np.float32(0.01)).astype(np.float32)
    x = rng.standard_normal(n).astype(np.float32)
    xq, xs = R.quantize(x, gs)
    if d >= 5:
        wq[:n] = 0                                        # an all-zero row: +0.0
        # a row whose products cancel: group terms t and -t -> (t + -t) = +0, then -0-valued terms keep +0; the negated
        # row of row 2 gives exactly the negated sum
        wq[3 * n:4 * n] = -wq[2 * n:3 * n]
        ws[3 * (n // gs):4 * (n // gs)] = ws[2 * (n // gs):3 * (n // gs)]
    got = dev_matmul(dev, wq, ws, xq, xs, n, d, gs)
    want = R.matmul(xq, xs, wq, ws, gs)
    assert same_bits(got, want), (d, n, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
    assert got.view(np.uint32)[0] == 0
    # all-zero x: every row +0.0
    zq, zs = R.quantize(np.zeros(n, np.float32), gs)
    got = dev_matmul(dev, wq[:min(d, 64) * n], ws[:min(d, 64) * (n // gs)], zq, zs, n, min(d, 64), gs)
    assert not got.view(np.uint32).any()


def test_matmul_negative_zero_terms_start_from_plus_zero(dev):
    """every term of row 0 is -0.0 (a positive group sum times a scale of -0.0): the definition's +0.0 start gives +0.0,
    where a sum started from -0.0 -- or from the first term -- would give -0.0.  Row 1 mixes -0.0 terms with real ones."""
    gs, n = 32, 64
    x = np.full(n, 0.5, np.float32)
    xq, xs = R.quantize(x, gs)
    assert (xq > 0).all() and (xs > 0).all()
    wq = np.ones(3 * n, np.int8)
    ws = np.array([-0.0, -0.0, -0.0, 0.25, 1e-3, -0.0], np.float32)
    got = dev_matmul(dev, wq, ws, xq, xs, n, 3, gs)
    want = R.matmul(xq, xs, wq, ws, gs)
    assert want.view(np.uint32)[0] == 0 and np.signbit(np.float32(-0.0) + np.float32(-0.0))   # what a -0.0 start would give
    assert same_bits(got, want) and got.view(np.uint32)[0] == 0


# ------------------------------------------------------------------ off the fast kernels: other group sizes, the LDS ceiling, misalignment

from tests.q8_offlane_cases import MATVEC, MATVEC_GENERIC


def product_path(dev, n, gs, n_tok, aligned):
    return dev.lib.rama_q8_product_path(n, gs, n_tok, int(aligned))


def harsh_groups(gs):
    """the inputs of test_quantize_edge_cases_and_bad_group scaled to group size gs, one kind per group: ties (the last one in
    the group's last element), a one-hot group, denormals, an all-zero group, a denormal ramp over the whole group"""
    x = np.zeros((5, gs), np.float32)
    x[0, 0] = 127.0
    ties = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, -126.5][:gs - 2]
    x[0, 1:1 + len(ties)] = ties
    x[0, gs - 1] = -63.5
    x[1, min(3, gs - 1)] = -3.0
    x[2, 0] = np.float32(1e-40); x[2, gs - 1] = np.float32(-5e-41)
    x[4] = np.linspace(-1, 1, gs, dtype=np.float32) * np.float32(1e-39)
    return x


@pytest.mark.parametrize("gs", [8, 16, 48, 128, 256, 1024, 2048])
def test_quantize_group_sizes_off_the_wave(dev, gs):
    """groups smaller than a wave (one partial stride) and of several 64-lane strides; five groups leave the second workgroup
    of four waves with one group, and every group also goes through alone (n = gs)"""
    x = harsh_groups(gs)
    wq, ws = R.quantize(x.reshape(-1), gs)
    assert wq[gs - 1] == -64 and wq[0] == 127 and ws[3] == 0 and 0 < ws[2] < np.finfo(np.float32).tiny
    rc, q, s = dev_quantize(dev, x.reshape(-1), gs)
    assert rc == 0
    assert np.array_equal(q, wq) and same_bits(s, ws), (gs, np.flatnonzero(q != wq)[:8])
    for g in range(5):
        rc, q, s = dev_quantize(dev, x[g], gs)
        assert rc == 0
        assert np.array_equal(q, wq[g * gs:(g + 1) * gs]) and same_bits(s, ws[g:g + 1]), (gs, g)
    # random data over 5 groups on top of the planted ones
    rng = np.random.default_rng(gs)
    y = (rng.standard_normal(5 * gs) * rng.choice([1e-3, 1.0, 40.0], size=5 * gs)).astype(np.float32)
    rc, q, s = dev_quantize(dev, y, gs)
    wq, ws = R.quantize(y, gs)
    assert rc == 0 and np.array_equal(q, wq) and same_bits(s, ws), gs


def matmul_case(dev, d, n, gs, path):
    """test_matmul_bit_identical's data recipe (an all-zero row, a row and its negation, all-zero activations) on a product
    that must take `path`"""
    assert product_path(dev, n, gs, 0, True) == path, (d, n, gs)
    rng = np.random.default_rng(d * 7 + n)
    G = n // gs
    wq = rng.integers(-127, 128, size=d * n, dtype=np.int8)
    ws = (rng.random(d * G, dtype=np.float32) * np.float32(0.01)).astype(np.float32)
    x = rng.standard_normal(n).astype(np.float32)
    xq, xs = R.quantize(x, gs)
    if d >= 5:
        wq[:n] = 0
        wq[3 * n:4 * n] = -wq[2 * n:3 * n]
        ws[3 * G:4 * G] = ws[2 * G:3 * G]
    got = dev_matmul(dev, wq, ws, xq, xs, n, d, gs)
    want = R.matmul(xq, xs, wq, ws, gs)
    assert same_bits(got, want), (d, n, gs, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
    if d >= 5:
        assert got.view(np.uint32)[0] == 0 and got[3] == -got[2]
    zq, zs = R.quantize(np.zeros(n, np.float32), gs)
    got = dev_matmul(dev, wq[:min(d, 64) * n], ws[:min(d, 64) * G], zq, zs, n, min(d, 64), gs)
    assert not got.view(np.uint32).any()


@pytest.mark.parametrize("d,n,gs", [(37, 72, 8), (9, 40, 8), (257, 96, 48), (20, 144, 24), (5, 64, 8), (33, 4096, 2048), (1, 72, 8)])
def test_matmul_generic_kernel_bit_identical(dev, d, n, gs):
    """q8_matvec_generic_kernel: K % 16 != 0, group sizes below 16, not a power of two, above 1024; 257 rows are two workgroups"""
    matmul_case(dev, d, n, gs, MATVEC_GENERIC)


@pytest.mark.parametrize("d,n,gs", [(37, 48, 16), (1, 48, 16), (255, 1040, 16), (33, 1536, 512), (19, 2048, 1024), (9, 32768, 16)])
def test_matmul_fast_kernel_at_its_edges(dev, d, n, gs):
    """q8_matvec_kernel where its group reduction degenerates (group size 16: one chunk per group, no shuffle) or spans the
    wave (1024: 64 chunks); n = 1040 is 65 chunks, one past a wave; an odd d leaves the last task's second row empty;
    (9, 32768, 16) is 2048 groups: exactly 64 KiB of dynamic LDS"""
    matmul_case(dev, d, n, gs, MATVEC)


def test_matmul_one_group_past_the_lds_ceiling_takes_the_generic_kernel(dev):
    matmul_case(dev, 9, 32784, 16, MATVEC_GENERIC)


def guarded_matmul(dev, wq, ws, xq, xs, n, d, gs, w_lead=0, x_lead=0):
    """rama_q8_matmul with the weights / activations `lead` bytes into their allocations and the output between guard words
    -> (result, guards untouched)"""
    def lead(a, k):
        return np.concatenate([np.full(k, 0x55, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1)])
    bw, bs, bx, bxs = Buf(dev, lead(wq, w_lead)), Buf(dev, ws), Buf(dev, lead(xq, x_lead)), Buf(dev, xs)
    o = Buf(dev, np.full(d + 8, np.float32(7.0)))
    rc = dev.lib.rama_q8_matmul(dev.ctx, o.p + 16, bw.p + w_lead, bs.p, bx.p + x_lead, bxs.p, n, d, gs)
    out = o.get(np.float32, d + 8)
    for b in (bw, bs, bx, bxs, o):
        b.free()
    assert rc == 0
    return out[4:4 + d], bool((out[:4] == np.float32(7.0)).all() and (out[4 + d:] == np.float32(7.0)).all())


def test_matmul_misaligned_weights_or_activations(dev):
    """weights or activations 4 bytes off a 16-byte boundary: the bytewise kernel, the same bits, nothing written outside o"""
    d, n, gs = 64, 4096, 64
    assert product_path(dev, n, gs, 0, True) == MATVEC and product_path(dev, n, gs, 0, False) == MATVEC_GENERIC
    rng = np.random.default_rng(64)
    wq = rng.integers(-127, 128, size=d * n, dtype=np.int8)
    ws = (rng.random(d * n // gs, dtype=np.float32) * np.float32(0.01)).astype(np.float32)
    wq[:n] = 0
    wq[3 * n:4 * n] = -wq[2 * n:3 * n]
    ws[3 * (n // gs):4 * (n // gs)] = ws[2 * (n // gs):3 * (n // gs)]
    xq, xs = R.quantize(rng.standard_normal(n).astype(np.float32), gs)
    want = R.matmul(xq, xs, wq, ws, gs)
    for w_lead, x_lead in ((0, 0), (4, 0), (0, 4)):
        got, clean = guarded_matmul(dev, wq, ws, xq, xs, n, d, gs, w_lead, x_lead)
        assert same_bits(got, want), (w_lead, x_lead)
        assert clean, (w_lead, x_lead)


# ------------------------------------------------------------------ loader

def test_fixtures_load_and_match_file(dev, golden_dir):
    import rama_amd
    for name, gs in FIXTURES:
        cfg, g, shared, norms, t = R.read_v2(golden_dir / f"{name}.bin")
        m = rama_amd.Q8Model.load(dev, golden_dir / f"{name}.bin")
        try:
            assert m.group_size == gs == g and m.cfg.shared_weight == shared and m.cfg.dim == cfg["dim"]
            for k in R.TENSORS:
                q, s = m.tensor(k)
                assert np.array_equal(q, t[k][0]) and same_bits(s, t[k][1]), (name, k)
            for k, v in norms.items():
                assert same_bits(m.tensor(k), v)
            assert same_bits(m.tensor("token_embedding_table"), R.dequantize(*t["tok"], gs))
            fr, fi = S.rope_tables(cfg["seq_len"], cfg["dim"] // cfg["n_heads"])
            for got, want in ((m.tensor("freq_cis_real"), fr), (m.tensor("freq_cis_imag"), fi)):
                assert np.abs(got.view(np.int32).astype(np.int64) - want.reshape(-1).view(np.int32).astype(np.int64)).max() <= 1
        finally:
            m.free()


def test_loader_error_codes(dev, golden_dir, tmp_path):
    import rama_amd
    L = dev.lib
    raw = (golden_dir / "ckpt_v2_q80_untied.bin").read_bytes()

    def rc_of(data):
        p = tmp_path / "f.bin"
        p.write_bytes(data)
        h = C.c_void_p()
        rc = L.rama_q8_model_load(dev.ctx, str(p).encode(), C.byref(h))
        if rc == 0:
            L.rama_q8_model_free(dev.ctx, h)
        return rc

    assert rc_of((golden_dir / "ckpt_tied.bin").read_bytes()) == -2                 # v0
    assert rc_of((golden_dir / "ckpt_v1_ak42.bin").read_bytes()) == -2              # v1
    assert rc_of(raw[:-1]) == -3 and rc_of(raw[:300]) == -3 and rc_of(raw + b"\0") == -3   # truncated / too long
    assert rc_of(raw[:37] + struct.pack("<i", 48) + raw[41:]) == -2                 # 48 does not divide 64
    assert rc_of(raw[:24] + struct.pack("<i", 2) + raw[28:]) == -2                  # GQA header
    assert rc_of(raw) == 0
    # the fp32 loader still refuses every ak42 file
    h = C.c_void_p()
    assert L.rama_model_load(dev.ctx, str(golden_dir / "ckpt_v2_q80_tied.bin").encode(), C.byref(h)) == -2


def test_synth_matches_numpy_quantization(dev):
    import rama_amd
    cfg = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=256, shared_weight=True)
    m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), 32, 7)
    try:
        norms, t = R.synth_q8(cfg, 32, 7)
        for k in ("tok", "wq", "wo", "w1", "w2", "w3"):
            q, s = m.tensor(k)
            assert np.array_equal(q, t[k][0]) and same_bits(s, t[k][1]), k
        for k, v in norms.items():
            assert same_bits(m.tensor(k), v), k
    finally:
        m.free()


# ------------------------------------------------------------------ forward and generation

def model_and_ref(dev, golden_dir, name):
    import rama_amd
    m = rama_amd.Q8Model.load(dev, golden_dir / f"{name}.bin")
    cfg, gs, _, norms, t = R.read_v2(golden_dir / f"{name}.bin")
    ref = R.Q8Ref(cfg, gs, norms, t, (m.tensor("freq_cis_real"), m.tensor("freq_cis_imag")))
    return m, ref


def check_state(eng, ref, pos):
    c = ref.c
    assert same_bits(eng.logits(), ref.s["logits"]), pos
    assert same_bits(eng.buffer("x", c.dim), ref.s["x"]), pos
    for l in range(c.n_layers):
        off = (l * c.seq_len + pos) * c.dim
        assert same_bits(eng.buffer("key_cache", c.dim, off), ref.cache_row("key_cache", l, pos)), (pos, l)
        assert same_bits(eng.buffer("value_cache", c.dim, off), ref.cache_row("value_cache", l, pos)), (pos, l)


@pytest.mark.parametrize("name,gs", FIXTURES)
@pytest.mark.parametrize("graph", [0, 1])
def test_forward_fixture_every_position(dev, golden_dir, name, gs, graph):
    import rama_amd
    m, ref = model_and_ref(dev, golden_dir, name)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        eng.set_graph_mode(graph)
        token = 1
        for pos in range(ref.c.seq_len):
            ref.forward(token, pos)
            eng.forward(token, pos)
            check_state(eng, ref, pos)
            token = O.argmax(ref.s["logits"])
    finally:
        eng.free(); m.free()


def test_forward_stories15m_shape_200_positions(dev):
    import rama_amd
    cfg = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=256, shared_weight=True)
    m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), 32, 11)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        norms, t = R.synth_q8(cfg, 32, 11)
        ref = R.Q8Ref(cfg, 32, norms, t, (m.tensor("freq_cis_real"), m.tensor("freq_cis_imag")))
        token = 1
        for pos in range(200):
            ref.forward(token, pos)
            eng.forward(token, pos)
            check_state(eng, ref, pos)
            token = O.argmax(ref.s["logits"])
    finally:
        eng.free(); m.free()


def test_forward_7b_shape_one_layer_long_positions(dev):
    """one llama2-7B-shaped layer at a few positions, one past 1024; the cache rows in front are written directly"""
    import rama_amd
    cfg = dict(dim=4096, hidden_dim=11008, n_layers=1, n_heads=32, n_kv_heads=32, vocab_size=32000, seq_len=2048, shared_weight=False)
    m = rama_amd.Q8Model.synth(dev, O.Config(**cfg), 64, 5)
    eng = rama_amd.Q8Engine(dev, m)
    try:
        norms, t = R.synth_q8(cfg, 64, 5)
        ref = R.Q8Ref(cfg, 64, norms, t, (m.tensor("freq_cis_real"), m.tensor("freq_cis_imag")))
        rng = np.random.default_rng(0)
        d = cfg["dim"]
        for pos, token in ((0, 1), (3, 17), (300, 901), (1100, 4242)):
            if pos:
                kv = (rng.standard_normal((2, pos, d)) * 0.5).astype(np.float32)
                ref.s["key_cache"][:pos * d] = kv[0].reshape(-1)
                ref.s["value_cache"][:pos * d] = kv[1].reshape(-1)
                eng.set_buffer("key_cache", kv[0]); eng.set_buffer("value_cache", kv[1])
            ref.forward(token, pos)
            eng.forward(token, pos)
            check_state(eng, ref, pos)
    finally:
        eng.free(); m.free()


@pytest.mark.parametrize("graph", [0, 1])
def test_generate_matches_reference_loop(dev, golden_dir, graph):
    import rama_amd
    from rama_amd.sampler_const import TOPP_U_CPU
    m, ref = model_and_ref(dev, golden_dir, "ckpt_v2_q80_untied")
    eng = rama_amd.Q8Engine(dev, m)
    try:
        eng.set_graph_mode(graph)
        steps = ref.c.seq_len
        assert eng.generate_greedy([], steps) == R.Q8Ref(*_ref_args(golden_dir, m)).generate([], steps)
        prompt = [5, 9, 33, 2]
        got = eng.generate(prompt, steps)
        assert got[:4] == prompt and got == R.Q8Ref(*_ref_args(golden_dir, m)).generate(prompt, steps)
        got = eng.generate([7], steps, temperature=1.0, topp=0.9)
        assert got == R.Q8Ref(*_ref_args(golden_dir, m)).generate([7], steps, 1.0, 0.9, TOPP_U_CPU)
        # the chained loop equals per-token forward + the sampler on the device's own logits
        token, want = 1, []
        for pos in range(steps):
            eng.forward(token, pos)
            nxt = prompt[pos] if pos < len(prompt) else O.argmax(eng.logits())
            want.append(int(nxt)); token = nxt
        assert eng.generate(prompt, steps) == want
    finally:
        eng.free(); m.free()


def _ref_args(golden_dir, m):
    cfg, gs, _, norms, t = R.read_v2(golden_dir / "ckpt_v2_q80_untied.bin")
    return cfg, gs, norms, t, (m.tensor("freq_cis_real"), m.tensor("freq_cis_imag"))
