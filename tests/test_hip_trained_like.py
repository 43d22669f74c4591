"""-m gpu: the decode paths on trained-like data (tests/trained_like.py): massive activations and attention sinks.

Parity mode (ref_order 1) must stay the oracle's bits when the data reaches the exact-sum kernels' fallbacks: the leader workgroup's
one-thread loop (chain.hpp CNORM_LEAD, when seqsum_fast.hpp's walk list passes kFsCap) and seq_sum_cascade's fallbacks
(seq_sum_lds_fast -> seq_sum_predict -> seq_sum_exact) in the parity attention's softmax.  Tests prove those branches ran
(rama_internal_seqsum_fast on the rows the leader sums, rama_internal_pred_stats around a model run) instead of hoping they did.

Fast mode (0), tolerance mode (2) and bar mode beyond its switch (3) are judged against the float64 forward with
trained_like.f64_bound on every buffer they share with forward(), not on the logits alone.

Shapes (dim, hidden, layers, heads, vocab, seq) pick the norm paths of rama_api.hip's parity forward: dim 288 folds the exact norm
into the matvecs (CNORM_EXACT); 768 / 2048 / 4096 take the leader (dim > 512), with a SEQ-heavy walk below kFsCap at 768 and the
fallback loop reachable from 2048 on; 2048 also has split-T attention from position 256 in fast mode.  The 4096 shape runs through
uploaded tensors only (no gigabyte checkpoint), and the 2048 shape too (its file would be 411 MB)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

from . import trained_like as T
from .helpers import gpu_views, to_rama_cfg

pytestmark = pytest.mark.gpu

SHAPES = {"d288": (288, 768, 2, 6, 512, 256), "d768": (768, 2048, 2, 12, 1000, 512),
          "d2048": (2048, 5632, 2, 16, 1000, 1100), "d4096": (4096, 11008, 2, 32, 640, 64)}
TOKS = [1, T.TOK_TIE, T.TOK_ZERO, T.TOK_SUBNORMAL, T.TOK_LARGE, 7, T.TOK_TIE, 9]      # the designated rows at the early positions
BUFS = ("x", "xb", "xb2", "hb", "hb2", "q", "k", "v", "logits", "key_cache", "value_cache")

_cache = {}


def case(shape, kind, shared=False):
    """(cfg, weights); one case is kept at a time (the 7B-width tensors are 1.6 GB)"""
    key = (shape, kind, shared)
    if key not in _cache:
        _cache.clear()
        d, h, L, H, V, seq = SHAPES[shape]
        cfg = O.Config(d, h, L, H, H, V, seq, shared)
        _cache[key] = (cfg, T.trained_like_weights(cfg, kind, 11))
    return _cache[key]


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    _cache.clear()
    d.close()


class mode:
    """with mode(dev, 1): ...  -- rama_set_tuning("ref_order"), back to fast mode on exit"""

    def __init__(self, dev, v, **more):
        self.dev, self.v, self.more = dev, v, more

    def __enter__(self):
        from rama_amd._lib import check
        check(self.dev.lib.rama_set_tuning(self.dev.ctx, b"ref_order", self.v))
        for k, v in self.more.items():
            check(self.dev.lib.rama_set_tuning(self.dev.ctx, k.encode(), v[0]))
        return self

    def __exit__(self, *exc):
        from rama_amd._lib import check
        for k, v in self.more.items():
            check(self.dev.lib.rama_set_tuning(self.dev.ctx, k.encode(), v[1]))
        check(self.dev.lib.rama_set_tuning(self.dev.ctx, b"ref_order", 0))
        return False


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits_equal(got, want, what=""):
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        raise AssertionError(f"{what}: {bad.size} of {g.size} values differ, first at {bad[0]}: "
                             f"{got.reshape(-1)[bad[0]]!r} vs {want.reshape(-1)[bad[0]]!r}")


def assert_state_bits(state, orc, cfg, pos, what):
    for b in BUFS:
        assert_bits_equal(state[b], orc.s[b], f"{what} pos {pos} {b}")
    att = np.asarray(state["att"]).reshape(cfg.n_heads, cfg.seq_len)[:, :pos + 1]
    assert_bits_equal(att, orc.s["att"].reshape(cfg.n_heads, cfg.seq_len)[:, :pos + 1], f"{what} pos {pos} att")


def engine_state(eng, cfg):
    kv = cfg.n_layers * cfg.seq_len * cfg.dim
    sizes = dict(x=cfg.dim, xb=cfg.dim, xb2=cfg.dim, hb=cfg.hidden_dim, hb2=cfg.hidden_dim, q=cfg.dim, k=cfg.dim, v=cfg.dim,
                 att=cfg.n_heads * cfg.seq_len, logits=cfg.vocab_size, key_cache=kv, value_cache=kv)
    return {b: eng.buffer(b, n) for b, n in sizes.items()}


def seqsum_fast(dev, a, nw):
    """rama_internal_seqsum_fast: -> (sum, held, items)"""
    from rama_amd._lib import check
    f = dev.lib.rama_internal_seqsum_fast
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    ta, to = dev.allocate(a), dev.allocate(np.zeros(4, np.float32))
    try:
        check(f(dev.ctx, ta.ptr, a.size, nw, to.ptr), "seqsum_fast")
        out = dev.download(to)
    finally:
        ta.free(); to.free()
    return out[0], out[1], out[2]


def pred_stats(dev, reset=True):
    """rama_internal_pred_stats: -> (held, fell_back) of chain.hpp's seq_sum_predict since the last reset"""
    from rama_amd._lib import check
    f = dev.lib.rama_internal_pred_stats
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.c_int]
    h, fb = C.c_uint(), C.c_uint()
    check(f(dev.ctx, C.byref(h), C.byref(fb), int(reset)), "pred_stats")
    return h.value, fb.value


# ------------------------------------------------------------------ proof that the leader's fallback runs

@pytest.mark.parametrize("dim", [768, 2048, 4096])
def test_leader_sum_gives_up_on_the_designated_rows(dev, dim):
    """the leader workgroup (CNORM_LEAD: one or two waves, the whole of x in registers) sums the squares of x with seqsum_fast.hpp.  On
    the tie row and the zero row every group of 8 is a SEQ group: at dim 768 the walk list still holds them (768 items), from 2048 on it
    overflows and the one-pass sum does not hold -- the leader then runs its one-thread loop over LDS on the layer-0 norm of these
    tokens in the model tests below.  Either way the sum is the sequential one, bit for bit."""
    rows = T.designated_rows(dim)
    for tok in (T.TOK_TIE, T.TOK_ZERO, T.TOK_SUBNORMAL, T.TOK_LARGE):
        sq = (rows[tok] * rows[tok]).astype(np.float32)
        for nw in (1, 2):
            s, held, items = seqsum_fast(dev, sq, nw)
            assert_bits_equal(np.float32(s), T.seq_sum_f32(sq), f"dim {dim} token {tok} waves {nw}")
            if tok in (T.TOK_TIE, T.TOK_ZERO):
                assert (held != 1.0) == (dim > T.FS_CAP), (dim, tok, nw, held, items)


@pytest.mark.parametrize("n", [264, 300, 768, 1000, 1500, 2040, 2044, 4096])
def test_standalone_norm_and_softmax_on_edge_sums_of_ragged_lengths(dev, n):
    """rmsnorm_chain_kernel and softmax_chain_kernel (256 threads) hand seqsum_fast.hpp lists that do not fill their threads: the groups
    of eight wholly behind the list's end stay off its walk list, the group that holds the end is a real one.  Lists whose running sum
    sits exactly on a binade edge (the tie row; a row that reaches 4096.0 half way; one exponential of 1.0 over a tail of 2^-25) and
    the zero row, at lengths that end inside a group, inside a thread and on a thread's edge: the oracle's bits.  At 768 terms and
    below the tie row is now served by the fast sum (no seq_sum_predict call: 768 items; it used to overflow the list on 160 padding
    groups), from 1 025 items on it is not."""
    import rama_amd
    rng = np.random.default_rng(n)
    half = T.tie_row(n); half[0] = 2.0 ** -6; half[n // 2] = 64.0
    w = (1.0 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    with mode(dev, 1):
        for what, x in (("tie", T.tie_row(n)), ("tie half way", half), ("zero", np.zeros(n, np.float32))):
            want = np.empty(n, np.float32)
            O.rmsnorm(want, x, w, n)
            tx, tw, to = (rama_amd.MutView(dev.allocate(a)) for a in (x, w, np.zeros(n, np.float32)))
            pred_stats(dev, reset=True)
            dev.rmsnorm(to, tx.as_view(), tw.as_view(), n)
            got = dev.download(to)
            held, fell = pred_stats(dev)
            assert_bits_equal(got, want, f"rmsnorm n={n} {what}")
            if what == "tie" and n > 512:      # (up to 512 terms seq_sum_predict's ripples serve a list uncounted)
                assert (held + fell > 0) == (n > T.FS_CAP), (n, held, fell)
        sc = (-rng.uniform(T.TAIL_LO, T.TAIL_HI, n)).astype(np.float32)
        sc[0] = 0.0
        want = sc.copy()
        O.softmax(want, n)
        ts = rama_amd.MutView(dev.allocate(sc))
        dev.softmax(ts, n)
        assert_bits_equal(dev.download(ts), want, f"softmax n={n}")


# ------------------------------------------------------------------ parity mode, bit for bit

@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_uploaded_tensors_parity_fast_and_tolerance(dev, shape, kind):
    """forward_fused and the 1:1 Device ops on uploaded tensors, parity mode: every RunState buffer the oracle's after every position,
    with the designated rows at the early positions.  Then fast mode and tolerance mode on the same tensors within f64_bound of the
    float64 forward"""
    import rama_amd
    cfg, w = case(shape, kind)
    orc = O.Oracle(cfg, w)
    rcfg, ws, wv, rs, rsv = gpu_views(dev, cfg, w)
    rs2 = rama_amd.RunState.from_config(rcfg, dev)
    rsv2 = rama_amd.RunStateView.from_rs(rs2)
    try:
        with mode(dev, 1):
            for pos, tok in enumerate(TOKS):
                orc.forward(tok, pos)
                rama_amd.forward_fused(rcfg, wv, rsv, tok, pos, dev)
                rama_amd.forward(rcfg, wv, rsv2, tok, pos, dev)
                for v, what in ((rsv, "fused"), (rsv2, "trait ops")):
                    st = {}
                    dev.to_cpu(v, st)
                    assert_state_bits(st, orc, cfg, pos, f"{shape} {kind} {what}")
    finally:
        rs2.free(); rs.free(); ws.free()
    for ref_order in (0, 2):
        _f64_run(dev, shape, kind, ref_order, list(zip(TOKS, range(len(TOKS)))))


@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("trained_like")


def _model(dev, ckpt_dir, shape, kind, shared=False):
    import rama_amd
    cfg, w = case(shape, kind, shared)
    p = ckpt_dir / f"{shape}_{kind}_{int(shared)}.bin"
    if not p.exists():
        T.write_checkpoint(p, cfg, w)
    return cfg, w, rama_amd.Model.load(dev, p)


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("shape,shared", [("d288", True), ("d768", False)])
def test_parity_resident_model_every_buffer(dev, ckpt_dir, shape, shared, kind):
    """a written checkpoint through Model.load: every buffer bit for bit with the chain-order copies (chain 1) and without (chain 0)"""
    import rama_amd
    cfg, w, model = _model(dev, ckpt_dir, shape, kind, shared)
    orc = O.Oracle(cfg, w)
    try:
        with mode(dev, 1):
            eng = rama_amd.Engine(dev, model)
            for pos, tok in enumerate(TOKS):
                orc.forward(tok, pos)
                eng.forward(tok, pos)
                assert_state_bits(engine_state(eng, cfg), orc, cfg, pos, f"{shape} {kind} model chain 1")
            eng.free()
            eng.set_tuning("chain", 0)
            try:
                eng = rama_amd.Engine(dev, model)
                orc = O.Oracle(cfg, w)
                for pos, tok in enumerate(TOKS):
                    orc.forward(tok, pos)
                    eng.forward(tok, pos)
                    assert_state_bits(engine_state(eng, cfg), orc, cfg, pos, f"{shape} {kind} model chain 0")
                eng.free()
            finally:
                eng.set_tuning("chain", 1)
    finally:
        model.free()


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("shape", ["d288", "d768"])
def test_parity_chained_decode(dev, ckpt_dir, shape, kind):
    """decode_begin / decode_steps with the designated tokens forced at the first positions: greedy eager and from a hipGraph, and one
    sampled run (T 1, top-p 0.9, the CPU draw u), the oracle's tokens"""
    import rama_amd
    from rama_amd.sampler_const import TOPP_U_CPU
    cfg, w, model = _model(dev, ckpt_dir, shape, kind)
    steps = 16
    prompt = TOKS[1:]
    want = O.Oracle(cfg, w).generate_greedy(prompt, steps)
    orc, token, want_s = O.Oracle(cfg, w), 1, []
    for pos in range(steps):
        lo = orc.forward(token, pos).copy()
        token = prompt[pos] if pos < len(prompt) else O.sample(lo, 1.0, 0.9, TOPP_U_CPU)
        want_s.append(int(token))
    try:
        with mode(dev, 1):
            for graph in (False, True):
                eng = rama_amd.Engine(dev, model)
                eng.set_graph_mode(graph)
                try:
                    eng.decode_sampler(0.0)
                    eng.decode_begin(1, 0, prompt)
                    eng.decode_steps(steps)
                    assert eng.decode_tokens() == want, f"{shape} {kind} greedy graph={graph}"
                    eng.decode_sampler(1.0, 0.9, TOPP_U_CPU)
                    eng.decode_begin(1, 0, prompt)
                    eng.decode_steps(steps)
                    assert eng.decode_tokens() == want_s, f"{shape} {kind} sampled graph={graph}"
                finally:
                    eng.decode_sampler(0.0)
                    eng.set_graph_mode(False)
                    eng.free()
    finally:
        model.free()


@pytest.mark.parametrize("kind", T.KINDS)
def test_parity_prefill_and_batches(dev, ckpt_dir, kind):
    """rama_prefill over 40 positions (a 32-position pass boundary) and decode_batch at 5 and 65 sequences (65: the tile-order copies)
    with the designated rows among the tokens: logits and caches the oracle's bits"""
    import rama_amd
    from rama_amd._lib import check
    cfg, w, model = _model(dev, ckpt_dir, "d288", kind, True)
    rng = np.random.default_rng(5)
    toks = [1] + [int(t) for t in rng.integers(0, cfg.vocab_size, 39)]
    toks[3:7] = T.DESIGNATED
    toks[35:39] = T.DESIGNATED
    try:
        with mode(dev, 1):
            orc = O.Oracle(cfg, w)
            for pos, t in enumerate(toks):
                lo = orc.forward(t, pos)
            eng = rama_amd.Engine(dev, model)
            arr = (C.c_int32 * len(toks))(*toks)
            check(dev.lib.rama_prefill(dev.ctx, C.byref(model.ccfg), C.byref(model.weights), C.byref(eng.state), arr, len(toks), 0), "rama_prefill")
            assert_bits_equal(eng.logits(), lo, f"{kind} prefill logits")
            for b in ("key_cache", "value_cache", "x", "xb", "hb", "q"):
                assert_bits_equal(eng.buffer(b, orc.s[b].size), orc.s[b], f"{kind} prefill {b}")
            eng.free()
            for n_seq in (5, 65):
                batch = [rama_amd.Engine(dev, model) for _ in range(n_seq)]
                orcs = [O.Oracle(cfg, w) for _ in range(n_seq)]
                cur = [T.DESIGNATED[i % 4] if i % 3 else int(rng.integers(0, cfg.vocab_size)) for i in range(n_seq)]
                pos = [0] * n_seq
                try:
                    for step in range(3):
                        rama_amd.decode_batch(batch, cur, pos)
                        for i in range(n_seq):
                            lo = orcs[i].forward(cur[i], pos[i])
                            assert_bits_equal(batch[i].logits(), lo, f"{kind} batch {n_seq} sequence {i} step {step}")
                            cur[i] = T.DESIGNATED[(i + step) % 4] if step == 0 else O.argmax(lo)
                            pos[i] += 1
                    for i in (0, n_seq - 1):
                        for b in ("key_cache", "value_cache"):
                            assert_bits_equal(batch[i].buffer(b, orcs[i].s[b].size), orcs[i].s[b], f"{kind} batch {n_seq} sequence {i} {b}")
                finally:
                    for e in batch:
                        e.free()
    finally:
        model.free()


def test_parity_prefill_and_batch_d2048(dev, ckpt_dir):
    """the d2048 companion of test_parity_prefill_and_batches: rama_prefill over 40 positions and a 5-sequence decode_batch at the
    width where the tie and zero rows overflow seqsum_fast's walk list -- one workgroup of the batched rmsnorm_chain_kernel falls back
    while its neighbours take the fast sum.  The batched norm and attention kernels are the ones rama_q8_prefill and
    rama_q8_decode_batch launch (tests/test_hip_q8_trained_like.py): a failure here and there pins them, a failure there alone the
    Q8 product.  One layer, through a written checkpoint (Model.load; the file is 220 MB, two layers would be 411)."""
    import rama_amd
    from rama_amd._lib import check
    _cache.clear()
    d, h, _, H, V, seq = SHAPES["d2048"]
    cfg = O.Config(d, h, 1, H, H, V, seq, False)
    w = T.trained_like_weights(cfg, "massive", 11)
    p = ckpt_dir / "d2048_massive_l1.bin"
    T.write_checkpoint(p, cfg, w)
    model = rama_amd.Model.load(dev, p)
    p.unlink()
    rng = np.random.default_rng(6)
    toks = [1] + [int(t) for t in rng.integers(8, V, 39)]
    toks[1:5] = T.DESIGNATED
    toks[20], toks[31], toks[32], toks[38] = T.TOK_TIE, T.TOK_ZERO, T.TOK_TIE, T.TOK_TIE
    try:
        with mode(dev, 1):
            orc = O.Oracle(cfg, w)
            for pos, t in enumerate(toks):
                lo = orc.forward(t, pos)
            eng = rama_amd.Engine(dev, model)
            arr = (C.c_int32 * len(toks))(*toks)
            check(dev.lib.rama_prefill(dev.ctx, C.byref(model.ccfg), C.byref(model.weights), C.byref(eng.state), arr, len(toks), 0), "rama_prefill")
            assert_bits_equal(eng.logits(), lo, "d2048 prefill logits")
            for b in ("key_cache", "value_cache", "x", "xb", "hb", "q"):
                assert_bits_equal(eng.buffer(b, orc.s[b].size), orc.s[b], f"d2048 prefill {b}")
            eng.free()
            n_seq = 5
            batch = [rama_amd.Engine(dev, model) for _ in range(n_seq)]
            orcs = [O.Oracle(cfg, w) for _ in range(n_seq)]
            cur = [7, T.TOK_TIE, 9, T.TOK_ZERO, T.TOK_LARGE]
            pos = [0] * n_seq
            try:
                for step in range(3):
                    rama_amd.decode_batch(batch, cur, pos)
                    for i in range(n_seq):
                        lo = orcs[i].forward(cur[i], pos[i])
                        assert_bits_equal(batch[i].logits(), lo, f"d2048 batch sequence {i} step {step}")
                        cur[i] = T.DESIGNATED[(i + step) % 4] if step == 0 else O.argmax(lo)
                        pos[i] += 1
                for i in (0, n_seq - 1):
                    for b in ("key_cache", "value_cache"):
                        assert_bits_equal(batch[i].buffer(b, orcs[i].s[b].size), orcs[i].s[b], f"d2048 batch sequence {i} {b}")
            finally:
                for e in batch:
                    e.free()
    finally:
        model.free()


@pytest.mark.parametrize("kind", T.KINDS)
def test_bar_mode_below_its_switch_is_parity(dev, kind):
    import rama_amd
    cfg, w = case("d768", kind)
    orc = O.Oracle(cfg, w)
    rcfg, ws, wv, rs, rsv = gpu_views(dev, cfg, w)
    try:
        with mode(dev, 3):
            for pos, tok in enumerate(TOKS):
                orc.forward(tok, pos)
                rama_amd.forward_fused(rcfg, wv, rsv, tok, pos, dev)
                st = {}
                dev.to_cpu(rsv, st)
                assert_state_bits(st, orc, cfg, pos, f"bar {kind}")
    finally:
        rs.free(); ws.free()


@pytest.mark.parametrize("sink_at", [0, 256, 1098])
def test_parity_sink_softmax_falls_back_and_stays_exact(dev, sink_at):
    """d2048 at position 1099 over sink caches: the softmax sum of 1 100 exponentials of which one is 1.0 and the rest lie in
    [2^-25, 2^-24] stays within 2^-13 of 1.0.  With the sink first, seqsum_fast's walk list overflows (every group SEQ, 1 100 items)
    and seq_sum_predict gives up (every run straddles the binade edge): rama_internal_pred_stats must count fallbacks.  Every buffer,
    the probabilities included, stays the oracle's bits."""
    import rama_amd
    cfg, w = case("d2048", "sink")
    pos = 1099
    kc, vc = T.sink_caches(cfg, w, 9, pos, sink_at)
    orc = O.Oracle(cfg, w)
    orc.s["key_cache"][:] = kc; orc.s["value_cache"][:] = vc
    orc.forward(9, pos)
    rcfg, ws, wv, rs, rsv = gpu_views(dev, cfg, w)
    try:
        with mode(dev, 1):
            dev.upload_into(rsv.key_cache, kc); dev.upload_into(rsv.value_cache, vc)
            pred_stats(dev, reset=True)
            rama_amd.forward_fused(rcfg, wv, rsv, 9, pos, dev)
            held, fell = pred_stats(dev)
            st = {}
            dev.to_cpu(rsv, st)
            assert_state_bits(st, orc, cfg, pos, f"sink at {sink_at}")
            if sink_at == 0:
                assert fell > 0, (held, fell)
    finally:
        rs.free(); ws.free()


# ------------------------------------------------------------------ the other modes against the float64 forward

def _f64_run(dev, shape, kind, ref_order, positions, caches=None, split_pos=None, what=""):
    """over `positions` (token, pos) pairs, with caches (kc, vc) set before each when given: the 1:1 Device ops (forward(), every buffer
    of infer.rs) and forward_fused (logits, caches and the residual stream -- in fast and tolerance mode its x is the residual: the
    final norm rides in the classifier launch, so it is F's xb) within f64_bound of the float64 forward; greedy tokens the oracle's where F's top-2 margin
    exceeds the bound.  -> worst err / bound"""
    import rama_amd
    cfg, w = case(shape, kind)
    orc, f64 = O.Oracle(cfg, w), O.Oracle(cfg, w)
    rcfg, ws, wv, rs, rsv = gpu_views(dev, cfg, w)
    rs2 = rama_amd.RunState.from_config(rcfg, dev)
    rsv2 = rama_amd.RunStateView.from_rs(rs2)
    more = {} if split_pos is None else {"split_pos": (split_pos, -1)}
    worst = 0.0
    try:
        with mode(dev, ref_order, **more):
            for tok, pos in positions:
                if caches is not None:
                    kc, vc = caches(pos)
                    orc.s["key_cache"][:] = kc; orc.s["value_cache"][:] = vc
                    f64.s["key_cache"][:] = kc; f64.s["value_cache"][:] = vc
                    for v in (rsv, rsv2):
                        dev.upload_into(v.key_cache, kc); dev.upload_into(v.value_cache, vc)
                orc.forward(tok, pos); f64.forward_f64(tok, pos)
                rama_amd.forward_fused(rcfg, wv, rsv, tok, pos, dev)
                rama_amd.forward(rcfg, wv, rsv2, tok, pos, dev)
                Ov, F = T.state_view(orc.s, cfg, pos), T.state_view(f64.s, cfg, pos, f64=True)
                st = {}
                dev.to_cpu(rsv2, st)
                P = T.state_view(st, cfg, pos)
                if ref_order != 1:
                    P.pop("att", None)         # (the fast attention keeps no probabilities: judged through xb and the logits)
                worst = max(worst, T.assert_f64_bound(P, Ov, F, f"{what} {shape} {kind} ref_order {ref_order} trait ops pos {pos}"))
                st = {}
                dev.to_cpu(rsv, st)
                Pf = T.state_view(st, cfg, pos)
                if ref_order in (0, 2):
                    Pf = {"logits": Pf["logits"], "xb": Pf["x"], "key_cache": Pf["key_cache"], "value_cache": Pf["value_cache"]}
                else:                          # (bar mode: parity mode's launches, the final norm's output in x as in forward())
                    Pf.pop("att", None)
                worst = max(worst, T.assert_f64_bound(Pf, Ov, F, f"{what} {shape} {kind} ref_order {ref_order} fused pos {pos}"))
                bound = T.f64_bound(Pf, Ov, F)["logits"][1]
                if T.greedy_margin_ok(F["logits"], bound):
                    assert int(np.argmax(Pf["logits"])) == O.argmax(orc.s["logits"]), (what, pos)
    finally:
        rs2.free(); rs.free(); ws.free()
    print(f"f64 margin {what} {shape} {kind} ref_order {ref_order}: worst err/bound {worst:.3f}")
    return worst


@pytest.mark.parametrize("kind", T.KINDS)
def test_bar_mode_beyond_its_switch_against_f64(dev, kind):
    """bar mode from position 128 on runs the fast attention: over prefilled sink caches at 200 and 300"""
    cfg, w = case("d768", kind)
    _f64_run(dev, "d768", kind, 3, [(9, 200), (T.TOK_TIE, 300)], caches=lambda pos: T.sink_caches(cfg, w, 9 if pos == 200 else T.TOK_TIE, pos, 0),
             what="bar beyond switch")


@pytest.mark.parametrize("split_pos", [256, -1])
@pytest.mark.parametrize("sink", ["first", "boundary", "last"])
def test_fast_split_t_over_sink_caches_against_f64(dev, sink, split_pos):
    """fast mode at d2048 over sink caches, split-T forced from 256 and by default: the per-split maxima differ by tens, so a wrong
    or stale rescale in the combine is O(1) wrong in xb and the logits"""
    cfg, w = case("d2048", "sink")

    def at(pos):
        return {"first": 0, "boundary": 256 if pos > 256 else pos // 2, "last": pos - 1}[sink]

    _f64_run(dev, "d2048", "sink", 0, [(9, p) for p in (255, 256, 257, 1000, 1099)],
             caches=lambda pos: T.sink_caches(cfg, w, 9, pos, at(pos)), split_pos=split_pos, what=f"split-T sink {sink}")


# ------------------------------------------------------------------ op level: multi_head_attention on sink / dead / flat heads

@pytest.mark.parametrize("ref_order", [0, 1])
def test_op_attention_sink_dead_and_flat_heads(dev, ref_order):
    """dev.multi_head_attention over sink caches for a query with a dead head (q = 0: uniform over exp = 1.0) and a nearly flat one,
    against a float64 numpy attention; parity mode also the oracle's bits"""
    import rama_amd
    n_heads, hs, seq = 4, 128, 1100
    dim = n_heads * hs
    cfg = O.Config(dim, 4 * dim, 1, n_heads, n_heads, 8, seq, True)
    rcfg = rama_amd.Config(dim, 4 * dim, 1, n_heads, n_heads, 8, seq, True)
    rng = np.random.default_rng(ref_order)
    z1 = np.zeros(1, np.float32)
    orc = O.Oracle(cfg, dict(token_embedding_table=np.zeros((8, dim), np.float32), rms_att_weight=np.zeros((1, dim), np.float32),
                             rms_ffn_weight=np.zeros((1, dim), np.float32), wq=z1, wk=z1, wv=z1, wo=z1, w1=z1, w2=z1, w3=z1,
                             rms_final_weight=np.zeros(dim, np.float32), freq_cis_real=z1, freq_cis_imag=z1))
    rs = rama_amd.RunState.from_config(rcfg, dev)
    rsv = rama_amd.RunStateView.from_rs(rs)
    try:
        with mode(dev, ref_order):
            for pos, sink_at in ((255, 0), (257, 256), (1099, 0), (1099, 1098)):
                q = rng.standard_normal(dim).astype(np.float32) * np.float32(3.0)
                q[:hs] = 0.0
                q[hs:2 * hs] *= np.float32(1e-4)
                kc = np.zeros((seq, dim), np.float32); vc = np.zeros((seq, dim), np.float32)
                self_k = rng.standard_normal(dim).astype(np.float32)
                k, v = T.sink_cache_layer(q, self_k, n_heads, pos, sink_at, rng)
                kc[:pos] = k; vc[:pos] = v
                kc[pos] = self_k; vc[pos] = rng.standard_normal(dim).astype(np.float32)
                kc, vc = kc.reshape(-1), vc.reshape(-1)
                orc.s["key_cache"][:] = kc; orc.s["value_cache"][:] = vc; orc.s["q"][:] = q
                orc.multi_head_attention(0, pos)
                dev.upload_into(rsv.key_cache, kc); dev.upload_into(rsv.value_cache, vc); dev.upload_into(rsv.q, q)
                dev.multi_head_attention(rsv, rcfg, 0, pos)
                xb = dev.download(rsv.xb)
                K = kc.reshape(seq, n_heads, hs)[:pos + 1].astype(np.float64)
                V = vc.reshape(seq, n_heads, hs)[:pos + 1].astype(np.float64)
                s = np.einsum("thd,hd->ht", K, q.reshape(n_heads, hs).astype(np.float64)) / np.sqrt(hs)
                p = np.exp(s - s.max(axis=1, keepdims=True)); p /= p.sum(axis=1, keepdims=True)
                want = np.einsum("ht,thd->hd", p, V).reshape(-1)
                F, Ov, P = {"xb": want}, {"xb": orc.s["xb"].astype(np.float64)}, {"xb": xb.astype(np.float64)}
                T.assert_f64_bound(P, Ov, F, f"attention ref_order {ref_order} pos {pos} sink {sink_at}")
                assert np.abs(xb[:hs] - V[:, 0].mean(axis=0)).max() < 1e-5         # the dead head: the plain mean of the values
                if ref_order == 1:
                    assert_bits_equal(xb, orc.s["xb"], f"attention pos {pos} sink {sink_at} xb")
                    att = dev.download(rsv.att).reshape(n_heads, seq)[:, :pos + 1]
                    assert_bits_equal(att, orc.s["att"].reshape(n_heads, seq)[:, :pos + 1], f"attention pos {pos} sink {sink_at} att")
    finally:
        rs.free()
