"""CPU checks of the Q8_0 fixtures and of the numpy restatement the GPU tests hold the device to (tests/q8_ref.py)."""
import numpy as np
import pytest

from tests import q8_ref as R

CASES = [("ckpt_v2_q80_tied", 32, True), ("ckpt_v2_q80_untied", 64, False)]


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
