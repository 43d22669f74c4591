"""-m gpu: the batched top-p sampler (rama_sample_topp_batch_dev) and the sampled chained batch
(rama_decode_batch_begin_sampled): per-row / per-sequence temperature, top-p, draw and forced prompt, against the
single-row sampler, the single-sequence generate() and the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from oracle import synth as S
from rama_amd.sampler_const import TOPP_U_CPU
from tests.helpers import to_rama_cfg

pytestmark = pytest.mark.gpu

STATE_ATOL = 2e-5
RAMA_EINVAL, RAMA_EUNSUP = -1, -2
TS, TOPPS, US = (0.0, 0.5, 1.0, 1.5), (0.5, 0.9, 0.95, 1.0), (0.0, TOPP_U_CPU, 0.999)


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


def _rnd(n, seed, scale):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def _clear_no_candidate_word(dev):
    """rama_sample_topp_dev leaves the single-row sampler's no-candidate word set after a -1 (the next chained loop's
    rama_decode_tokens reports it); rama_sample_topp reads and clears it -- here on a row where nothing is kept"""
    z = dev.allocate(np.zeros(2, np.float32))
    assert dev.lib.rama_sample_topp(dev.ctx, z.ptr, 2, 1.0, 0.0, 0.5, C.byref(C.c_int32())) == RAMA_EINVAL
    z.free()


def _topp_dev(dev, x, temperature, topp, u):
    """the single-row sampler (rama_sample_topp_dev) on a host vector"""
    from rama_amd._lib import check
    d_x, d_r = dev.allocate(x), dev.alloc(1)
    check(dev.lib.rama_sample_topp_dev(dev.ctx, d_x.ptr, x.size, temperature, topp, u, d_r.ptr))
    out = int(dev.download(d_r).view(np.int32)[0])
    d_x.free(); d_r.free()
    if out < 0:
        _clear_no_candidate_word(dev)
    return out


def _admissible(x, T, topp, u, token):
    """the pick of one of the reference's own executions: rayon splits the softmax's sum as it likes, and a draw
    whose running sum sits on a boundary follows the last bit of that sum"""
    for split in range(1, 12):
        with O.orders(softmax_split=split):
            if O.sample(x.copy(), T, topp, u) == token:
                return True
    return False


def _row_cases(n, n_rows, seed):
    """(logits, T, topp, u) per row: flat rows (all kept), sigma 3, peaked, ties across sorting blocks, a masked
    vocabulary, a row where nothing is kept; (T, topp, u) cycle through the grid at co-prime strides"""
    rng = np.random.default_rng(seed)
    rows, params = [], []
    for r in range(n_rows):
        kind = (r + seed) % 6
        if kind == 0:
            x = _rnd(n, seed + r, 0.05)                                             # flat
        elif kind == 1:
            x = _rnd(n, seed + r, 3.0)
        elif kind == 2:
            x = _rnd(n, seed + r, 12.0)                                             # peaked
        elif kind == 3:
            x = rng.integers(0, 4, n).astype(np.float32) * np.float32(0.6931472)  # few distinct values: ties across blocks
        elif kind == 4:
            x = _rnd(n, seed + r, 2.0); x[rng.random(n) < 0.5] = -np.inf           # masked
        else:
            x = np.zeros(n, np.float32)                                             # with topp 0: nothing kept (p = 1/n <= 1/(n-1))
        T, topp, u = TS[r % 4], TOPPS[(r // 4 + r) % 4], US[r % 3]
        if kind == 5:
            T, topp = 1.0, 0.0
        if kind == 0 and r % 2:
            T, topp = 1.0, 1.0                                                      # every entry kept
        rows.append(x); params.append((T, topp, u))
    return np.stack(rows), params


@pytest.mark.parametrize("n", [512, 4099, 32000])
@pytest.mark.parametrize("n_rows", [1, 3, 37, 128])
def test_batch_sampler_equals_single_row_and_oracle(dev, n_rows, n):
    import rama_amd
    x, params = _row_cases(n, n_rows, seed=n_rows * 7 + n)
    d_x = dev.allocate(x)
    T, P, U = zip(*params)
    got = rama_amd.sample_topp_batch(dev, d_x.ptr, list(T), list(P), list(U), n_rows=n_rows, n=n)
    assert np.array_equal(dev.download(d_x).reshape(n_rows, n), x), "the logits changed"
    d_x.free()
    for r in range(n_rows):
        single = _topp_dev(dev, x[r], *params[r])
        want = O.sample(x[r].copy(), *params[r])
        assert got[r] == single, (r, params[r], got[r], single)
        if params[r][1] == 0.0 and params[r][0] != 0.0 and not np.any(x[r]):
            assert got[r] == -1
        if got[r] != want:
            assert _admissible(x[r], *params[r], got[r]), (r, params[r], got[r], want)


def test_batch_sampler_strided_rows_and_long_rows(dev):
    """rows ld > n floats apart (the last row's slack never read), and n > 32768 (the single-row launches row by row)"""
    import rama_amd
    n, ld, n_rows = 4099, 4160, 9
    x, params = _row_cases(n, n_rows, seed=3)
    slab = np.full((n_rows, ld), np.nan, np.float32); slab[:, :n] = x
    d = dev.allocate(slab)
    T, P, U = zip(*params)
    got = rama_amd.sample_topp_batch(dev, d.ptr, list(T), list(P), list(U), n_rows=n_rows, n=n, ld=ld)
    d.free()
    assert got == [_topp_dev(dev, x[r], *params[r]) for r in range(n_rows)]
    big = np.stack([_rnd(40000, 50 + r, 2.0) for r in range(3)])
    pp = [(1.0, 0.9, TOPP_U_CPU), (0.0, 0.9, 0.5), (0.7, 0.95, 0.3)]
    got = rama_amd.sample_topp_batch(dev, big, [p[0] for p in pp], [p[1] for p in pp], [p[2] for p in pp])
    assert got == [_topp_dev(dev, big[r], *pp[r]) for r in range(3)]
    assert got == [O.sample(big[r].copy(), *pp[r]) for r in range(3)]


def test_batch_sampler_argument_errors(dev):
    L = dev.lib
    d, r = dev.allocate(np.zeros(64, np.float32)), dev.alloc(4)
    ok = (C.c_float * 2)(1.0, 1.0)
    for bad_T, bad_P, bad_U in (((-1.0, 1.0), (0.9, 0.9), (0.1, 0.1)), ((1.0, 1.0), (0.9, 1.5), (0.1, 0.1)),
                                ((1.0, 1.0), (0.9, 0.9), (0.1, 1.0)), ((1.0, 1.0), (-0.1, 0.9), (0.1, 0.1))):
        args = [(C.c_float * 2)(*v) for v in (bad_T, bad_P, bad_U)]
        assert L.rama_sample_topp_batch_dev(dev.ctx, d.ptr, 32, 32, 2, *args, r.ptr) == RAMA_EINVAL
    assert L.rama_sample_topp_batch_dev(dev.ctx, d.ptr, 16, 32, 2, ok, ok, ok, r.ptr) == RAMA_EINVAL      # ld < n
    assert L.rama_sample_topp_batch_dev(dev.ctx, d.ptr, 32, 32, 0, ok, ok, ok, r.ptr) == RAMA_EINVAL      # no rows
    assert L.rama_sample_topp_batch_dev(dev.ctx, d.ptr, 1, 1, 1, ok, ok, ok, r.ptr) == RAMA_EINVAL        # n = 1
    d.free(); r.free()


# ------------------------------------------------------------------ the sampled chained batch

def _model(dev, cfg, seed):
    import rama_amd
    rope = S.rope_tables(cfg.seq_len, cfg.head_size)
    w = S.synth_weights(cfg, seed=seed, rope=rope)
    return w, rama_amd.Model.synth(dev, to_rama_cfg(cfg), seed, rope=rope)


def _oracle_run(orc, t, p, steps, T, topp, u, prompt=()):
    """generate()'s loop from (t, p): next = p < len(prompt) ? prompt[p] : Device::sample (-1 -> 0, as the chain)"""
    out = []
    for _ in range(steps):
        lo = orc.forward(t, p)
        t = prompt[p] if p < len(prompt) else O.sample(lo.copy(), T, topp, u)
        t = max(t, 0)
        out.append(int(t)); p += 1
    return out


def _draws(n_seq, seed):
    rng = np.random.default_rng(seed)
    T = [(1.0, 0.5, 1.5, 0.0)[i % 4] for i in range(n_seq)]                   # (sequence 0 samples: a single sequence is not greedy)
    P = [TOPPS[int(rng.integers(0, 4))] for _ in range(n_seq)]
    U = [US[int(rng.integers(0, 3))] for _ in range(n_seq)]
    return T, P, U


def _device_loop(dev, engines, cur, pos, steps, T, P, U):
    """the host loop the sampled chain replaces: rama_decode_batch (the same token-batch pass), then rama_sample_topp_dev
    row after row on every state's logits (-1 -> 0)"""
    import rama_amd
    res = dev.alloc(len(engines))
    cur, pos, out = list(cur), list(pos), [[] for _ in engines]
    V = engines[0].cfg.vocab_size
    for _ in range(steps):
        rama_amd.decode_batch(engines, cur, pos)
        for i, e in enumerate(engines):
            assert dev.lib.rama_sample_topp_dev(dev.ctx, e.state.logits, V, T[i], P[i], U[i], res.ptr + 4 * i) == 0
        picks = dev.download(res).view(np.int32)
        if (picks < 0).any():
            _clear_no_candidate_word(dev)
        for i in range(len(engines)):
            cur[i] = max(int(picks[i]), 0); pos[i] += 1
            out[i].append(cur[i])
    res.free()
    return out


def _chained_vs_oracle(dev, cfg, seed, n_seq, graph, steps, oracle_sampled=True):
    """every sequence's tokens = the device host loop's (the same logits, the single-row sampler: bit for bit), and = its
    own oracle generation -- for sampled rows only where the draw is not in the far tail and the vocabulary is small
    (oracle_sampled): fast mode's logits differ from the oracle's by up to 1e-4, and a draw over a flat 32 000-way
    distribution picks by those last bits (the parity-mode test below holds the sampler to the oracle on exact logits)"""
    import rama_amd
    w, m = _model(dev, cfg, seed)
    batch = [rama_amd.Engine(dev, m) for _ in range(n_seq)]
    twin = [rama_amd.Engine(dev, m) for _ in range(n_seq)]
    orcs = [O.Oracle(cfg, w) for _ in range(n_seq)]
    rng = np.random.default_rng(200 + n_seq)
    cur = [int(t) for t in rng.integers(0, cfg.vocab_size, n_seq)]
    pos = [0] * n_seq
    for i in range(n_seq):                        # stagger: sequence i is advanced alone i % 4 times first
        for _ in range(i % 4):
            lo = orcs[i].forward(cur[i], pos[i]); batch[i].forward(cur[i], pos[i]); twin[i].forward(cur[i], pos[i])
            cur[i] = O.argmax(lo); pos[i] += 1
    T, P, U = _draws(n_seq, seed + n_seq)
    batch[0].set_graph_mode(graph)
    try:
        got = rama_amd.decode_batch_chained(batch, cur, pos, steps, temperature=T, topp=P, u=U)
    finally:
        batch[0].set_graph_mode(False)
    ref = _device_loop(dev, twin, cur, pos, steps, T, P, U)
    for i in range(n_seq):
        assert got[i] == ref[i], (i, T[i], P[i], U[i], got[i], ref[i])
        want = _oracle_run(orcs[i], cur[i], pos[i], steps, T[i], P[i], U[i])
        if T[i] == 0.0 or (oracle_sampled and U[i] * P[i] <= 0.9):
            assert got[i] == want, (i, T[i], P[i], U[i], got[i], want)
    for i in (0, n_seq // 2, n_seq - 1):
        for buf in ("key_cache", "value_cache"):
            assert np.abs(batch[i].buffer(buf, orcs[i].s[buf].size) - orcs[i].s[buf]).max() <= STATE_ATOL, (i, buf)
    for e in batch + twin: e.free()
    m.free()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("n_seq", [1, 5, 19, 64, 97, 128])
def test_decode_batch_sampled_equals_oracle_generations(dev, n_seq, graph):
    """per-sequence T (T = 0 rows among them), topp and u; every sequence's tokens = its own oracle loop, caches within
    STATE_ATOL; the small model of the greedy chain's test"""
    _chained_vs_oracle(dev, O.Config(128, 352, 2, 4, 4, 256, 40, True), 4, n_seq, graph, 9)


@pytest.mark.parametrize("n_seq,graph", [(1, False), (5, True), (19, False), (64, True), (97, False), (128, True)])
def test_decode_batch_sampled_stories15m_shape(dev, n_seq, graph):
    """a stories15M-shaped synthetic model (its dim, hidden_dim, heads and V = 32000; two layers): every step runs the
    multi-block sort of 32 blocks per row"""
    _chained_vs_oracle(dev, O.Config(288, 768, 2, 6, 6, 32000, 32, True), 15, n_seq, graph, 4, oracle_sampled=False)


@pytest.mark.parametrize("graph", [False, True])
def test_decode_batch_sampled_prompts_equal_generate(dev, graph):
    """every sequence starts at (BOS, 0) with its own prompt of 0..7 tokens: its tokens = the single-sequence
    generate(prompt_i, steps, T_i, topp_i, u_i) and the oracle's generation"""
    import rama_amd
    cfg = O.Config(128, 352, 2, 4, 4, 256, 40, True)
    w, m = _model(dev, cfg, 4)
    n_seq, steps = 11, 14
    rng = np.random.default_rng(5)
    prompts = [[int(t) for t in rng.integers(0, cfg.vocab_size, i % 8)] for i in range(n_seq)]
    T, P, U = _draws(n_seq, 9)
    batch = [rama_amd.Engine(dev, m) for _ in range(n_seq)]
    batch[0].set_graph_mode(graph)
    try:
        got = rama_amd.decode_batch_chained(batch, [1] * n_seq, [0] * n_seq, steps, temperature=T, topp=P, u=U, prompts=prompts)
    finally:
        batch[0].set_graph_mode(False)
    single = rama_amd.Engine(dev, m)
    try:
        for i in range(n_seq):
            want = _oracle_run(O.Oracle(cfg, w), 1, 0, steps, T[i], P[i], U[i], prompts[i])
            assert got[i] == want, (i, prompts[i], got[i], want)
            assert single.generate(prompts[i], steps, T[i], P[i], U[i]) == want, i
    finally:
        single.decode_sampler(0.0)
    for e in batch + [single]: e.free()
    m.free()


def _begin_sampled(batch, toks, pos, steps, per):
    """rama_decode_batch_begin_sampled with records [(T, topp, u, forced)] -> rc"""
    from rama_amd._lib import rama_run_state, rama_seq_sampling
    e0, n = batch[0], len(batch)
    states = (rama_run_state * n)(*[e.state for e in batch])
    keep = [(C.c_int32 * max(len(f), 1))(*f) for (_, _, _, f) in per]
    recs = (rama_seq_sampling * n)(*[rama_seq_sampling(T, P, U, keep[i], len(f)) for i, (T, P, U, f) in enumerate(per)])
    return e0.device.lib.rama_decode_batch_begin_sampled(e0.device.ctx, C.byref(e0.model.ccfg), C.byref(e0.model.weights), states,
                                                         (C.c_int32 * n)(*toks), (C.c_int32 * n)(*pos), n, steps, recs)


def _run_steps(dev, n_seq, steps):
    from rama_amd._lib import check
    check(dev.lib.rama_decode_batch_steps(dev.ctx, steps), "rama_decode_batch_steps")
    out, k = (C.c_int32 * (n_seq * steps))(), C.c_int()
    check(dev.lib.rama_decode_batch_tokens(dev.ctx, out, steps, C.byref(k)), "rama_decode_batch_tokens")
    return [[int(out[s * steps + j]) for j in range(k.value)] for s in range(n_seq)]


@pytest.mark.parametrize("graph", [False, True])
def test_decode_batch_sampled_all_greedy_equals_greedy_chain(dev, graph):
    import rama_amd
    from rama_amd._lib import check
    cfg = O.Config(128, 352, 2, 4, 4, 256, 40, True)
    _, m = _model(dev, cfg, 4)
    n_seq, steps = 70, 12
    toks, pos = [int(t) for t in np.random.default_rng(1).integers(0, 256, n_seq)], [i % 5 for i in range(n_seq)]
    batch = [rama_amd.Engine(dev, m) for _ in range(n_seq)]
    batch[0].set_graph_mode(graph)
    try:
        greedy = rama_amd.decode_batch_chained(batch, toks, pos, steps)
        check(_begin_sampled(batch, toks, pos, steps, [(0.0, 0.9, TOPP_U_CPU, ())] * n_seq), "rama_decode_batch_begin_sampled")
        sampled = _run_steps(dev, n_seq, steps)
    finally:
        batch[0].set_graph_mode(False)
    assert sampled == greedy
    for e in batch: e.free()
    m.free()


def test_decode_batch_sampled_across_score_buffer_buckets(dev):
    """a sampled graph-mode run across position 256 re-captures its step graph (still one replay per step) and keeps
    producing the oracle's tokens"""
    import rama_amd
    cfg = O.Config(64, 176, 1, 4, 4, 96, 300, False)
    w, m = _model(dev, cfg, 8)
    a, b = rama_amd.Engine(dev, m), rama_amd.Engine(dev, m)
    draws = [(1.0, 0.9, TOPP_U_CPU), (0.8, 0.95, 0.5)]
    a.set_graph_mode(True)
    try:
        got = rama_amd.decode_batch_chained([a, b], [3, 7], [0, 0], 270, temperature=[d[0] for d in draws],
                                            topp=[d[1] for d in draws], u=[d[2] for d in draws])
    finally:
        a.set_graph_mode(False)
    for i, t0 in enumerate((3, 7)):
        want = _oracle_run(O.Oracle(cfg, w), t0, 0, 270, *draws[i])
        assert got[i] == want, (i, next(k for k in range(270) if got[i][k] != want[k]))
    a.free(); b.free(); m.free()


def test_decode_batch_sampled_stream_poll_in_order(dev):
    import rama_amd
    cfg = O.Config(128, 352, 2, 4, 4, 256, 40, True)
    _, m = _model(dev, cfg, 4)
    n_seq, steps = 6, 20
    batch = [rama_amd.Engine(dev, m) for _ in range(n_seq)]
    seen = [[] for _ in range(n_seq)]

    def on_token(s, k, t):
        assert k == len(seen[s]), (s, k)
        seen[s].append(t)
    T, P, U = _draws(n_seq, 3)
    got = rama_amd.decode_batch_chained(batch, [1] * n_seq, [0] * n_seq, steps, on_token=on_token, temperature=T, topp=P, u=U,
                                        prompts=[[5, 6]] * n_seq)
    assert seen == got and all(len(g) == steps for g in got)
    for e in batch: e.free()
    m.free()


def test_decode_batch_sampled_argument_errors_leave_the_chain(dev):
    """each bad record gives RAMA_EINVAL and leaves the running chain as it was; parity mode gives RAMA_EUNSUP; a greedy
    chain afterwards still gives the oracle's tokens"""
    import rama_amd
    from rama_amd._lib import check
    cfg = O.Config(128, 352, 2, 4, 4, 256, 40, True)
    w, m = _model(dev, cfg, 4)
    batch = [rama_amd.Engine(dev, m) for _ in range(2)]
    good = [(1.0, 0.9, TOPP_U_CPU, (4, 5, 6)), (0.0, 0.9, 0.0, ())]
    check(_begin_sampled(batch, [1, 1], [0, 0], 8, good), "rama_decode_batch_begin_sampled")
    first = _run_steps(dev, 2, 3)
    bad = [(-0.5, 0.9, 0.1, ()), (1.0, 1.5, 0.1, ()), (1.0, -0.1, 0.1, ()), (1.0, 0.9, 1.0, ()), (1.0, 0.9, -0.2, ()),
           (1.0, 0.9, 0.1, (3, cfg.vocab_size)), (1.0, 0.9, 0.1, (-1,)), (float("nan"), 0.9, 0.1, ())]
    for rec in bad:
        assert _begin_sampled(batch, [1, 1], [0, 0], 8, [good[0], rec]) == RAMA_EINVAL, rec
    # n_forced < 0 (not expressible through the helper's tuple)
    from rama_amd._lib import rama_run_state, rama_seq_sampling
    recs = (rama_seq_sampling * 2)(rama_seq_sampling(1.0, 0.9, 0.1, None, 0), rama_seq_sampling(1.0, 0.9, 0.1, None, -1))
    states = (rama_run_state * 2)(*[e.state for e in batch])
    assert dev.lib.rama_decode_batch_begin_sampled(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), states, (C.c_int32 * 2)(1, 1),
                                                   (C.c_int32 * 2)(0, 0), 2, 8, recs) == RAMA_EINVAL
    assert dev.lib.rama_decode_batch_begin_sampled(dev.ctx, C.byref(m.ccfg), C.byref(m.weights), states, (C.c_int32 * 2)(1, 1),
                                                   (C.c_int32 * 2)(0, 0), 2, 8, None) == RAMA_EINVAL
    # the chain begun above is untouched: its tokens so far, then five more steps, = two oracle generations
    check(dev.lib.rama_decode_batch_steps(dev.ctx, 5))
    out, k = (C.c_int32 * 16)(), C.c_int()
    check(dev.lib.rama_decode_batch_tokens(dev.ctx, out, 8, C.byref(k)))
    assert k.value == 8
    for i, (T, P, U, f) in enumerate(good):
        want = _oracle_run(O.Oracle(cfg, w), 1, 0, 8, T, P, U, f)
        assert [int(out[i * 8 + j]) for j in range(8)] == want and first[i] == want[:3], i
    check(dev.lib.rama_set_tuning(dev.ctx, b"ref_order", 1))
    try:
        assert _begin_sampled(batch, [1, 1], [0, 0], 8, good) == RAMA_EUNSUP
    finally:
        check(dev.lib.rama_set_tuning(dev.ctx, b"ref_order", 0))
    for e in batch: e.free()
    fresh = [rama_amd.Engine(dev, m) for _ in range(2)]
    got = rama_amd.decode_batch_chained(fresh, [3, 9], [0, 0], 6)
    for i, t0 in enumerate((3, 9)):
        assert got[i] == _oracle_run(O.Oracle(cfg, w), t0, 0, 6, 0.0, 0.9, 0.0)
    for e in fresh: e.free()
    m.free()


def test_parity_decode_batch_then_batch_sampler_equals_oracle(dev):
    """parity mode composes: rama_decode_batch at 32 sequences (bit-exact logits), the per-state logits gathered into one
    slab, rama_sample_topp_batch_dev -> exactly the oracle's sampled tokens, step after step"""
    import rama_amd
    from rama_amd._lib import check
    cfg = O.Config(288, 768, 2, 6, 6, 512, 24, True)
    w, m = _model(dev, cfg, 9)
    n_seq = 32
    batch = [rama_amd.Engine(dev, m) for _ in range(n_seq)]
    orcs = [O.Oracle(cfg, w) for _ in range(n_seq)]
    T = [(1.0, 0.7, 0.0, 1.3)[i % 4] for i in range(n_seq)]
    P, U = [0.9] * n_seq, [TOPP_U_CPU] * n_seq
    cur, pos = [int(t) for t in np.random.default_rng(3).integers(0, cfg.vocab_size, n_seq)], [0] * n_seq
    slab = dev.alloc(n_seq * cfg.vocab_size)
    check(dev.lib.rama_set_tuning(dev.ctx, b"ref_order", 1))
    try:
        for _ in range(4):
            rama_amd.decode_batch(batch, cur, pos)
            lg = np.stack([e.logits() for e in batch])
            dev.upload_into(slab, lg)
            got = rama_amd.sample_topp_batch(dev, slab.ptr, T, P, U, n_rows=n_seq, n=cfg.vocab_size)
            for i in range(n_seq):
                lo = orcs[i].forward(cur[i], pos[i])
                assert np.array_equal(lg[i].view(np.uint32), lo.view(np.uint32)), i
                assert got[i] == O.sample(lo.copy(), T[i], P[i], U[i]), i
                cur[i] = got[i]; pos[i] += 1
    finally:
        check(dev.lib.rama_set_tuning(dev.ctx, b"ref_order", 0))
    slab.free()
    for e in batch: e.free()
    m.free()
