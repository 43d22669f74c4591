"""rama_q8_model_from_f32 / Q8Model.from_model on the GPU: a resident fp32 model quantized where it lies.  On the fp32 fixtures every
tensor of the result equals, bit for bit, the numpy restatement of export.py's rule (tests/q8_from_f32_ref.py); on synthetic shapes it
equals rama_q8_model_synth of the same seed tensor by tensor, and decodes to the same tokens and logits; the refusals; the source model
is left as it was."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import q8_from_f32_ref as R
from tests.helpers import GOLDEN, load_case, to_rama_cfg

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP = -1, -2
FP32 = ("token_embedding_table", "rms_att_weight", "rms_ffn_weight", "rms_final_weight", "freq_cis_real", "freq_cis_imag")


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_model(a, b, what):
    assert a.group_size == b.group_size and a.cfg == b.cfg, what
    names = [n for n in R.SOURCES if n != "wcls" or not a.cfg.shared_weight]
    for n in names:
        (qa, sa), (qb, sb) = a.tensor(n), b.tensor(n)
        assert np.array_equal(qa, qb) and np.array_equal(bits(sa), bits(sb)), (what, n)
    for n in FP32:
        assert np.array_equal(bits(a.tensor(n)), bits(b.tensor(n))), (what, n)
    assert (a.weights.wcls == a.weights.tok) == (b.weights.wcls == b.weights.tok) == bool(a.cfg.shared_weight), what


@pytest.mark.parametrize("name,gs", [("ckpt_tied", 32), ("ckpt_untied", None)])
def test_fixture_equals_the_numpy_restatement(dev, name, gs):
    import rama_amd
    cfg, w, _ = load_case(name)
    m = rama_amd.Model.load(dev, GOLDEN / f"{name}.bin")
    q = None
    try:
        before = m.tensor("w2", cfg.n_layers * cfg.dim * cfg.hidden_dim)
        q = rama_amd.Q8Model.from_model(m)                        # group_size 64, backed off until it divides
        want_gs = R.group_size(cfg.dim, cfg.hidden_dim, 64)
        assert q.group_size == want_gs and (gs is None or want_gs == gs)
        assert rama_amd.q8.from_f32_group_size(m.cfg, 64) == want_gs
        t, norms, table = R.from_f32(cfg, w, want_gs)
        for n in R.SOURCES:
            if n == "wcls" and cfg.shared_weight:
                assert q.weights.wcls == q.weights.tok and q.weights.wcls_s == q.weights.tok_s
                continue
            got_q, got_s = q.tensor(n)
            assert np.array_equal(got_q, t[n][0]), n
            assert np.array_equal(bits(got_s), bits(t[n][1])), n
        for n in R.NORMS:
            assert np.array_equal(bits(q.tensor(n)), bits(norms[n])), n
        assert np.array_equal(bits(q.tensor("token_embedding_table")), bits(table))
        assert bool(q.cfg.shared_weight) == bool(cfg.shared_weight)
        # the source is only read: one of its matrices before and after, and it still decodes
        assert np.array_equal(bits(m.tensor("w2", before.size)), bits(before))
        # the result decodes: the same tokens as the model loaded from ... itself, twice (nothing of the source is aliased)
        e = rama_amd.Q8Engine(dev, q)
        first = e.generate([5, 9], 6)
        m.free(); m = None
        assert e.generate([5, 9], 6) == first
        e.free()
    finally:
        if q is not None:
            q.free()
        if m is not None:
            m.free()


@pytest.mark.parametrize("name,gs", [("synth_d64_h4", 64), ("synth_d64_h4", 32), ("synth_d128_h1", 32)])
def test_synthetic_model_equals_q8_model_synth(dev, name, gs):
    """from_f32(rama_model_synth(cfg, seed)) == rama_q8_model_synth(cfg, gs, seed) in every tensor, and both decode alike; d128_h1 has
    352 = 11 x 32 values per FFN row: an odd count of groups"""
    import rama_amd
    g = np.load(GOLDEN / f"{name}.npz")
    a = [int(v) for v in g["cfg"]]
    cfg = O.Config(a[0], a[1], a[2], a[3], a[4], a[5], a[6], bool(a[7]))
    assert cfg.dim % gs == 0 and cfg.hidden_dim % gs == 0
    seed = int(g["seed"])
    m = rama_amd.Model.synth(dev, to_rama_cfg(cfg), seed)
    a = rama_amd.Q8Model.from_model(m, gs)
    b = rama_amd.Q8Model.synth(dev, to_rama_cfg(cfg), gs, seed)
    try:
        assert a.group_size == gs
        same_model(a, b, (name, gs))
        assert a.bytes == b.bytes
        ea, eb = rama_amd.Q8Engine(dev, a), rama_amd.Q8Engine(dev, b)
        for T in (0.0, 1.0):
            ta, tb = ea.generate([3, 7, 11], 9, T, 0.9, 0.3), eb.generate([3, 7, 11], 9, T, 0.9, 0.3)
            assert ta == tb and np.array_equal(bits(ea.logits()), bits(eb.logits())), (name, gs, T)
        ea.free(); eb.free()
    finally:
        a.free(); b.free(); m.free()


def test_refusals(dev):
    import rama_amd
    from rama_amd._lib import rama_config, rama_weights
    cfg, _, _ = load_case("ckpt_untied")
    m = rama_amd.Model.load(dev, GOLDEN / "ckpt_untied.bin")
    L = dev.lib
    out = C.c_void_p()

    def call(ccfg=None, w=None, gs=16, o=out):
        return L.rama_q8_model_from_f32(dev.ctx, C.byref(ccfg) if ccfg is not None else None, C.byref(w) if w is not None else None, gs,
                                        C.byref(o) if o is not None else None)
    try:
        assert call(None, m.weights) == EINVAL and call(m.ccfg, None) == EINVAL and call(m.ccfg, m.weights, o=None) == EINVAL
        for field in ("wq", "w2", "rms_final_weight", "wcls", "token_embedding_table"):       # an incomplete set: a pipeline stage's
            w = rama_weights.from_buffer_copy(m.weights)
            setattr(w, field, None)
            assert call(m.ccfg, w) == EINVAL, field
        assert call(m.ccfg, m.weights, 0) == EINVAL and call(m.ccfg, m.weights, -8) == EINVAL
        gs_bad = 3 if cfg.dim % 3 else 5
        assert cfg.dim % gs_bad and call(m.ccfg, m.weights, gs_bad) == EINVAL              # the C entry does not back off
        assert call(m.ccfg, m.weights, 2 * max(cfg.dim, cfg.hidden_dim)) == EINVAL
        gqa = rama_config.from_buffer_copy(m.ccfg)
        gqa.n_kv_heads = max(m.ccfg.n_heads // 2, 1) if m.ccfg.n_heads > 1 else 2
        assert call(gqa, m.weights) == EUNSUP
        tied = rama_config.from_buffer_copy(m.ccfg)               # shared_weight set over a classifier of its own: not silently dropped
        tied.shared_weight = 1
        assert m.weights.wcls != m.weights.token_embedding_table and call(tied, m.weights) == EINVAL
        assert not out.value
        with pytest.raises(ValueError):
            rama_amd.Q8Model.from_model(m, 0)
        q = rama_amd.Q8Model.from_model(m, 1 << 20)               # the wrapper backs off from any size
        assert cfg.dim % q.group_size == 0 and cfg.hidden_dim % q.group_size == 0
        q.free()
    finally:
        m.free()
