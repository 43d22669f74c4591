"""CPU checks of the Q8_0 fixtures and of the numpy restatement the GPU tests hold the device to (tests/q8_ref.py)."""
import numpy as np
import pytest

from tests import q8_ref as R

CASES = [("ckpt_v2_q80_tied", 32, True), ("ckpt_v2_q80_untied", 64, False)]
# the fixtures whose group size the exporter backed off below 32 (tests/q8_offlane_cases.py)
SMALL_GROUP_CASES = [("ckpt_v2_q80_gs16", 16, True), ("ckpt_v2_q80_gs8", 8, False)]


@pytest.mark.parametrize("name,gs,shared", CASES)
def test_v2_fixture_parses(golden_dir, name, gs, shared):
    cfg, g, sh, norms, t = R.read_v2(golden_dir / f"{name}.bin")       # asserts the size matches the layout
    ref = np.load(golden_dir / f"{name}.npz")
    assert g == gs == int(ref["group_size"]) and sh == shared
    assert [cfg[k] for k in ("dim", "hidden_dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size", "seq_len")] == ref["cfg"][:7].tolist()
    for k, v in norms.items():
        assert np.array_equal(v, ref[k].reshape(-1))
    names = dict(tok="token_embedding_table", wcls="wcls")
    maxerr = float(ref["maxerr"])
    for name_q, (q, s) in t.items():
        if names.get(name_q, name_q) not in ref.files:        # the fixture keeps the token table, wq, w2 and an untied classifier
            continue
        w = ref[names.get(name_q, name_q)].reshape(-1)
        assert q.size == w.size and s.size == w.size // gs
        err = np.abs(R.dequantize(q, s, gs) - w).max()
        assert err <= maxerr * (1 + 1e-6), (name_q, err, maxerr)
    if shared:
        assert t["wcls"][0] is t["tok"][0]
    else:
        assert not np.array_equal(t["wcls"][0], t["tok"][0])


@pytest.mark.parametrize("name,gs,shared", CASES)
def test_quantize_q80_restatement_matches_exporter(golden_dir, name, gs, shared):
    """the file's int8 values and scales are export.py's rule applied to the recorded fp32 weights"""
    _, _, _, _, t = R.read_v2(golden_dir / f"{name}.bin")
    ref = np.load(golden_dir / f"{name}.npz")
    for name_q, w in (("tok", "token_embedding_table"), ("wq", "wq"), ("w2", "w2")) + ((("wcls", "wcls"),) if not shared else ()):
        q, s = R.quantize_q80(ref[w].reshape(-1), gs)
        assert np.array_equal(q, t[name_q][0]), name_q
        assert np.array_equal(s.view(np.uint32), t[name_q][1].view(np.uint32)), name_q


def test_quantize_edge_cases():
    gs = 32
    # ties at +-k.5 go away from zero: wmax 127 -> scale 1, x / 1 = x exactly
    x = np.zeros(gs, np.float32)
    x[0] = 127.0
    x[1:9] = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, -126.5]
    q, s = R.quantize(x, gs)
    assert s[0] == np.float32(1.0)
    assert q[:9].tolist() == [127, 1, -1, 2, -2, 3, -3, 127, -127]
    # an all-zero group gives zeros and scale 0
    q, s = R.quantize(np.zeros(2 * gs, np.float32), gs)
    assert not q.any() and not s.any()
    # one-hot groups give +-127
    x = np.zeros(2 * gs, np.float32)
    x[3], x[gs + 7] = 0.25, -3.0
    q, s = R.quantize(x, gs)
    assert q[3] == 127 and q[gs + 7] == -127 and np.count_nonzero(q) == 2
    # denormals are kept, not flushed
    x = np.zeros(gs, np.float32)
    x[0] = np.float32(1e-40)
    x[1] = np.float32(-5e-41)
    q, s = R.quantize(x, gs)
    assert s[0] > 0 and s[0] < np.finfo(np.float32).tiny
    assert q[0] == 127 and q[1] in (-63, -64)


def test_quantize_q80_rounds_half_to_even():
    x = np.zeros(32, np.float32)
    x[0] = 127.0
    x[1:5] = [0.5, 1.5, 2.5, -2.5]
    q, _ = R.quantize_q80(x, 32)
    assert q[:5].tolist() == [127, 0, 2, 2, -2]


def test_matmul_definition_order_and_negative_zero():
    gs = 32
    rng = np.random.default_rng(3)
    wq = rng.integers(-127, 128, size=(5, 64), dtype=np.int8)
    ws = rng.random(10, dtype=np.float32)
    x = rng.standard_normal(64).astype(np.float32)
    xq, xs = R.quantize(x, gs)
    got = R.matmul(xq, xs, wq.reshape(-1), ws, gs)
    for i in range(5):
        val = np.float32(0.0)
        for g in range(2):
            iv = int(np.dot(xq[g * gs:(g + 1) * gs].astype(np.int64), wq[i, g * gs:(g + 1) * gs].astype(np.int64)))
            val = np.float32(val + np.float32(np.float32(np.float32(iv) * ws[i * 2 + g]) * xs[g]))
        assert got[i].view(np.uint32) == val.view(np.uint32)
    # a zero row starting from +0.0 stays +0.0
    z = R.matmul(xq, xs, np.zeros(64, np.int8), np.ones(2, np.float32), gs)
    assert z.view(np.uint32)[0] == 0


# ------------------------------------------------------------------ write_v2, the inverse of read_v2

@pytest.mark.parametrize("name,gs,shared", CASES)
def test_write_v2_reproduces_the_exporters_file(golden_dir, tmp_path, name, gs, shared):
    """the fixtures were written by the reference exporter: write_v2(*read_v2(file)) is the file, byte for byte"""
    src = golden_dir / f"{name}.bin"
    p = tmp_path / "again.bin"
    R.write_v2(p, *R.read_v2(src))
    assert p.read_bytes() == src.read_bytes()


@pytest.mark.parametrize("shared", [True, False])
def test_write_v2_round_trips_a_trained_like_model(tmp_path, shared):
    from tests import trained_like as T
    cfg = dict(dim=64, hidden_dim=192, n_layers=3, n_heads=4, n_kv_heads=4, vocab_size=40, seq_len=24, shared_weight=shared)
    norms, t = T.trained_like_q8(cfg, "massive", 32, 3)
    p = tmp_path / "m.bin"
    R.write_v2(p, cfg, 32, shared, norms, t)
    cfg2, gs2, shared2, norms2, t2 = R.read_v2(p)
    assert cfg2 == cfg and gs2 == 32 and shared2 == shared
    for k, v in norms.items():
        assert norms2[k].tobytes() == v.tobytes(), k
    for k in R.TENSORS:
        assert np.array_equal(t2[k][0], t[k][0]) and t2[k][1].tobytes() == t[k][1].tobytes(), k
    assert (t2["wcls"][0] is t2["tok"][0]) == shared
    raw = p.read_bytes()
    assert raw[36] == int(shared) and np.frombuffer(raw[37:41], "<i4")[0] == 32 and not any(raw[41:256])


# ------------------------------------------------------------------ group sizes off 32 / 64: fixtures, the restatement, the dispatch rule

@pytest.mark.parametrize("name,gs,shared", SMALL_GROUP_CASES)
def test_small_group_fixture_parses(golden_dir, name, gs, shared):
    """the exporter halved the group size until it divided dim: config and group size as tools/make_q8_goldens.py states them,
    dequantised tensors within the exporter's own recorded error, and the file is what write_v2 writes"""
    from tests.q8_offlane_cases import FIXTURE_CFGS
    cfg, g, sh, _, _ = R.read_v2(golden_dir / f"{name}.bin")
    want_cfg, want_gs = FIXTURE_CFGS[name]
    assert cfg == want_cfg and g == want_gs == gs and sh == shared
    assert cfg["dim"] % (2 * gs) != 0                        # the next larger group size does not divide dim
    test_v2_fixture_parses(golden_dir, name, gs, shared)
    test_quantize_q80_restatement_matches_exporter(golden_dir, name, gs, shared)


def _c_round(r):
    """C roundf on a float32 value, in exact double arithmetic: halves away from zero"""
    import math
    a = math.floor(abs(float(r)) + 0.5)
    return -a if r < 0 else a


def loop_quantize(x, gs):
    """R.quantize as a plain loop over groups and elements, every operation one np.float32 operation"""
    q, s = [], []
    for g in range(len(x) // gs):
        grp = [np.float32(v) for v in x[g * gs:(g + 1) * gs]]
        wmax = np.float32(0.0)
        for v in grp:
            if abs(v) > wmax:
                wmax = np.float32(abs(v))
        scale = np.float32(wmax / np.float32(127.0))
        s.append(scale)
        for v in grp:
            if scale == 0:
                q.append(0)
                continue
            r = _c_round(np.float32(v / scale))
            q.append(int(min(max(r, -127.0), 127.0)))
    return np.array(q, np.int8), np.array(s, np.float32)


def loop_matmul(xq, xs, wq, ws, n, d, gs):
    """R.matmul as a triple loop: int arithmetic per group, then three separately rounded np.float32 operations in group order
    from +0.0"""
    G = n // gs
    out = np.zeros(d, np.float32)
    for i in range(d):
        val = np.float32(0.0)
        for g in range(G):
            ival = 0
            for k in range(gs):
                ival += int(xq[g * gs + k]) * int(wq[i * n + g * gs + k])
            t = np.float32(np.float32(ival) * ws[i * G + g])
            t = np.float32(t * xs[g])
            val = np.float32(val + t)
        out[i] = val
    return out


@pytest.mark.parametrize("n,gs", [(48, 16), (72, 8), (96, 48), (256, 128), (40, 8)])
def test_restatement_at_other_group_sizes_equals_a_plain_loop(n, gs):
    d = 5
    rng = np.random.default_rng(n * 3 + gs)
    x = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 40.0], size=n)).astype(np.float32)
    G = n // gs
    x[:gs] = np.where(np.arange(gs) % 2 == 0, np.float32(3.5), np.float32(-3.5))        # a group of +-127
    if G > 1:
        x[gs:2 * gs] = 0.0                                                           # an all-zero group: scale 0
    if G > 2:
        x[2 * gs] = 127.0
        x[2 * gs + 1:2 * gs + 5] = [0.5, -0.5, 2.5, -126.5]                          # ties go away from zero
    xq, xs = R.quantize(x, gs)
    lq, ls = loop_quantize(x, gs)
    assert np.array_equal(xq, lq) and xs.tobytes() == ls.tobytes()
    assert set(np.abs(xq[:gs]).tolist()) == {127}
    if G > 1:
        assert not xq[gs:2 * gs].any() and xs[1] == 0
    if G > 2:
        assert xq[2 * gs:2 * gs + 5].tolist() == [127, 1, -1, 3, -127]
    wq = rng.integers(-127, 128, size=d * n, dtype=np.int8)
    ws = (rng.random(d * G, dtype=np.float32) * np.float32(0.02) - np.float32(0.004)).astype(np.float32)
    wq[:gs] = np.where(np.arange(gs) % 2 == 0, 127, -127)                            # +-127 against +-127: the largest group sum
    wq[n:2 * n] = 0                                                                   # an all-zero row
    wq[3 * n:4 * n] = -wq[2 * n:3 * n]                                                # a row and its negation
    ws[3 * G:4 * G] = ws[2 * G:3 * G]
    got = R.matmul(xq, xs, wq, ws, gs)
    want = loop_matmul(xq, xs, wq, ws, n, d, gs)
    assert got.tobytes() == want.tobytes()
    assert got.view(np.uint32)[1] == 0                                                # +0.0
    assert got[3] == -got[2]
    z = R.matmul(*R.quantize(np.zeros(n, np.float32), gs), wq, ws, gs)
    assert not z.view(np.uint32).any()


def test_product_path_table():
    """rama_q8_product_path(n, group_size, n_tok, aligned16): the kernel every product takes, row by row"""
    from rama_amd import _lib
    from tests.q8_offlane_cases import GEMM_GENERIC, GEMM_KSPLIT, GEMM_MFMA, MATVEC, MATVEC_GENERIC
    assert (MATVEC, MATVEC_GENERIC, GEMM_KSPLIT, GEMM_MFMA, GEMM_GENERIC) == (0, 1, 2, 3, 4)
    table = [((4096, 64, 0, 1), MATVEC), ((48, 16, 0, 1), MATVEC), ((2048, 1024, 0, 1), MATVEC),
             ((72, 8, 0, 1), MATVEC_GENERIC), ((96, 48, 0, 1), MATVEC_GENERIC), ((4096, 2048, 0, 1), MATVEC_GENERIC),
             ((4096, 64, 0, 0), MATVEC_GENERIC), ((32768, 16, 0, 1), MATVEC), ((32784, 16, 0, 1), MATVEC_GENERIC),
             ((288, 32, 17, 1), GEMM_KSPLIT), ((288, 32, 33, 1), GEMM_MFMA), ((256, 128, 17, 1), GEMM_MFMA),
             ((4096, 4096, 5, 1), GEMM_MFMA), ((8192, 8192, 5, 1), GEMM_GENERIC), ((48, 16, 5, 1), GEMM_GENERIC),
             ((72, 8, 5, 1), GEMM_GENERIC), ((288, 32, 17, 0), GEMM_GENERIC)]
    L = _lib.load()
    for args, want in table:
        assert L.rama_q8_product_path(*args) == want, args
    # a batch call answers for one pass of min(n_tok, 128) tokens
    assert L.rama_q8_product_path(288, 32, 130, 1) == GEMM_MFMA and L.rama_q8_product_path(288, 32, 32, 1) == GEMM_KSPLIT
    # what the entries themselves refuse
    for bad in ((100, 32, 0, 1), (0, 32, 0, 1), (64, 0, 0, 1), (64, 32, -1, 1)):
        assert L.rama_q8_product_path(*bad) == -1, bad


def test_model_paths_of_the_offlane_cases():
    """tests/q8_offlane_cases.py MODEL_PATHS is what the rule answers for each model's products"""
    from rama_amd import _lib
    from tests.q8_offlane_cases import FIXTURE_CFGS, GS128_CFG, MODEL_PATHS, TOKEN_COUNTS
    L = _lib.load()
    cfgs = {k: v[0] for k, v in FIXTURE_CFGS.items()}
    cfgs["gs128"] = GS128_CFG
    for name, want in MODEL_PATHS.items():
        assert set(want["matvec"]) == {cfgs[name]["dim"], cfgs[name]["hidden_dim"]}
        for K, path in want["matvec"].items():
            assert L.rama_q8_product_path(K, want["gs"], 0, 1) == path, (name, K)
            for n_tok in TOKEN_COUNTS:
                assert L.rama_q8_product_path(K, want["gs"], n_tok, 1) == want["gemm"], (name, K, n_tok)


def batch_shape_ok(cfg):
    import ctypes as C
    from rama_amd import _lib
    c = _lib.rama_config(cfg["dim"], cfg["hidden_dim"], cfg["n_layers"], cfg["n_heads"], cfg["n_kv_heads"], cfg["vocab_size"],
                         cfg["seq_len"], int(cfg["shared_weight"]))
    return _lib.load().rama_q8_batch_shape_ok(C.byref(c))


def test_batch_shape_ok(golden_dir):
    from rama_amd import _lib
    from tests.q8_offlane_cases import GS128_CFG, LONGCTX_CFG, LONGCTX_DEEP_SEQ_LEN, LONGCTX_REFUSED_SEQ_LEN, LONGCTX_SEQ_LEN, STORIES15M
    for name, _, _ in CASES + SMALL_GROUP_CASES:
        cfg = R.read_v2(golden_dir / f"{name}.bin")[0]
        assert batch_shape_ok(cfg) == 1, name
    assert batch_shape_ok(STORIES15M) == 1 and batch_shape_ok(GS128_CFG) == 1
    # LONGCTX_SEQ_LEN is the smallest multiple of 1024 the batch pass does not take
    assert LONGCTX_CFG["seq_len"] == LONGCTX_SEQ_LEN and LONGCTX_SEQ_LEN % 1024 == 0
    for S in range(1024, LONGCTX_SEQ_LEN, 1024):
        assert batch_shape_ok(dict(LONGCTX_CFG, seq_len=S)) == 1, S
    assert batch_shape_ok(LONGCTX_CFG) == 0
    assert batch_shape_ok(dict(LONGCTX_CFG, seq_len=LONGCTX_DEEP_SEQ_LEN)) == 0
    assert batch_shape_ok(dict(LONGCTX_CFG, seq_len=LONGCTX_REFUSED_SEQ_LEN)) == 0
    assert _lib.load().rama_q8_batch_shape_ok(None) == -1
    assert batch_shape_ok(dict(LONGCTX_CFG, n_kv_heads=1)) == -2          # a config no Q8 entry takes
