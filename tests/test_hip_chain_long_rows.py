"""-m gpu: parity mode's chain-order matvec on rows LONGER than the activations a wave requests up front (csrc/chain.hpp,
gemv_chain_body: 16 x 16 bytes per thread, 4 096 floats on one wave).  The one-wave kernels -- the residual products Wo / W2
with at most one row group per compute unit -- stage the rest of x between the chunks of the chain, a batch at a time; which
chunk may run after which batch is an invariant of the kernel, and every hidden_dim below sits on one of its edges.  W2 is the
only product whose row length is hidden_dim, so a small model with a long hidden layer is enough: one forward() per position
in parity mode against the oracle, every RunState buffer bit for bit, eager launches and hipGraph replays."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import synth as S

from .helpers import to_rama_cfg

pytestmark = pytest.mark.gpu

DIM, LAYERS, HEADS, VOCAB, SEQ, SEED = 128, 2, 4, 256, 32, 11      # dim 128: 8 row groups, the one-wave residual path
POSITIONS = (0, 1, 5)                                               # (compared; 0..5 are run, the cache rows in between are real)
LDS_FLOATS = 64 * 1024 // 4


def pad_floats(w, d, xd=4):      # chain_params.hpp chain_pad_floats: the zeros behind x in LDS
    return 16 * ((w + 1) * d + xd)


# the last row length for which launch_chain_epi keeps W = 1, D = 32 inside its 64 KiB of LDS, and the first that falls back to D = 16
LAST_D32 = (LDS_FLOATS - pad_floats(1, 32)) // 16 * 16
assert LAST_D32 == 15296 and LAST_D32 + 16 + pad_floats(1, 16) <= LDS_FLOATS

HIDDEN = [
    1040,             # shortest row that takes the D = 32 path (more than 64 blocks); nothing behind the up-front pieces
    4096,             # exactly the up-front pieces
    4112,             # one block behind them: almost every lane of the first batch is past the end
    4608,             # one whole batch beside a ring of 16, half a batch beside a ring of 32
    6160,             # a ragged second batch
    8208,             # crosses a batch boundary by one block
    11008,            # llama2-7B's row length
    LAST_D32,         # the last shape before the fallback
    LAST_D32 + 16,    # falls back to D = 16
]
FORCED = [(h, v) for h in (4112, 6160, 11008) for v in (116, 216, 232)]      # "chain_resid_d": the D = 16 ring on one wave, two waves (the barrier path)


@pytest.fixture(scope="module")
def dev():
    import rama_amd
    from rama_amd._lib import check
    d = rama_amd.Hip(0)
    check(d.lib.rama_set_tuning(d.ctx, b"ref_order", 1))
    yield d
    check(d.lib.rama_set_tuning(d.ctx, b"ref_order", 0))
    d.close()


def config(hidden):
    return O.Config(DIM, hidden, LAYERS, HEADS, HEADS, VOCAB, SEQ, False)


def buffer_sizes(cfg):
    return dict(x=cfg.dim, xb=cfg.dim, xb2=cfg.dim, hb=cfg.hidden_dim, hb2=cfg.hidden_dim, q=cfg.dim, k=cfg.dim, v=cfg.dim,
                logits=cfg.vocab_size, key_cache=cfg.n_layers * cfg.seq_len * cfg.dim, value_cache=cfg.n_layers * cfg.seq_len * cfg.dim)


def tokens():
    return [1] + [int(t) for t in np.random.default_rng(SEED).integers(0, VOCAB, max(POSITIONS))]


_ORACLE = {}


def oracle_states(hidden):
    """the oracle's RunState behind each compared position, computed once per hidden_dim and left alone"""
    if hidden not in _ORACLE:
        cfg = config(hidden)
        rope = S.rope_tables(cfg.seq_len, cfg.head_size)
        orc = O.Oracle(cfg, S.synth_weights(cfg, SEED, rope=rope))
        want = {}
        for pos, t in enumerate(tokens()):
            orc.forward(t, pos)
            if pos in POSITIONS:
                want[pos] = {b: np.array(orc.s[b], dtype=np.float32, copy=True).reshape(-1)[:n] for b, n in buffer_sizes(cfg).items()}
                want[pos]["att"] = np.array(orc.s["att"], dtype=np.float32, copy=True).reshape(cfg.n_heads, cfg.seq_len)[:, :pos + 1]
        _ORACLE[hidden] = (rope, want)
    return _ORACLE[hidden]


def assert_bits_equal(got, want, what):
    g, w = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        raise AssertionError(f"{what}: {bad.size} of {g.size} values differ, first at {bad[0]}: "
                             f"{np.asarray(got).reshape(-1)[bad[0]]!r} vs {np.asarray(want).reshape(-1)[bad[0]]!r}")


def run_against_oracle(dev, hidden, resid_d=None):
    import rama_amd
    cfg = config(hidden)
    rope, want = oracle_states(hidden)
    model = rama_amd.Model.synth(dev, to_rama_cfg(cfg), SEED, rope=rope)
    engines = []
    try:
        for graph in (False, True):
            eng = rama_amd.Engine(dev, model)
            engines.append(eng)
            if resid_d is not None:
                eng.set_tuning("chain_resid_d", resid_d)
            eng.set_graph_mode(graph)
            how = f"hidden {hidden} resid_d {resid_d} {'graph' if graph else 'eager'}"
            for pos, t in enumerate(tokens()):
                eng.forward(t, pos)
                if pos not in POSITIONS:
                    continue
                for buf, n in buffer_sizes(cfg).items():
                    assert_bits_equal(eng.buffer(buf, n), want[pos][buf], f"{how} pos {pos} {buf}")
                att = eng.buffer("att", cfg.n_heads * cfg.seq_len).reshape(cfg.n_heads, cfg.seq_len)[:, :pos + 1]
                assert_bits_equal(att, want[pos]["att"], f"{how} pos {pos} att")
            eng.set_graph_mode(False)
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        dev.lib.rama_set_tuning(dev.ctx, b"chain_resid_d", -1)
        for eng in engines:
            eng.free()
        model.free()


@pytest.mark.parametrize("hidden", HIDDEN)
def test_long_rows_every_buffer_bit_exact(dev, hidden):
    """default dispatch: W2 on one wave with a ring of 32 blocks up to LAST_D32 floats a row, a ring of 16 behind that"""
    run_against_oracle(dev, hidden)


@pytest.mark.parametrize("hidden,resid_d", FORCED)
def test_long_rows_forced_geometries_bit_exact(dev, hidden, resid_d):
    """"chain_resid_d" = 100 W + D: one wave with a ring of 16 (the smaller batch), and two waves, which stage all of x in front of their barrier"""
    run_against_oracle(dev, hidden, resid_d)
