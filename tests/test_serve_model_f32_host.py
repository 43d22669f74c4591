"""The parity-mode serving chain with a draft model, without a GPU: the refusals rama_amd.Server makes before any library call, the
group-size back-off of Q8Model.from_model, the numpy restatement of the quantizer (tests/q8_from_f32_ref.py) against tests/q8_ref.py's, and
the row-table condition the two-tile workload of tests/serve_model_f32_cases.py is chosen for."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import q8_from_f32_ref as R
from tests import serve_model_f32_cases as W


def fake(vocab=320, seq_len=96, device="d"):
    cfg = SimpleNamespace(dim=64, hidden_dim=176, n_layers=2, n_heads=4, n_kv_heads=4, vocab_size=vocab, seq_len=seq_len, shared_weight=False, head_size=16)
    return SimpleNamespace(cfg=cfg, device=device)


def test_server_refuses_a_bad_draft_before_any_library_call():
    import rama_amd
    m = fake()
    with pytest.raises(ValueError, match="vocabulary"):
        rama_amd.Server(m, 4, 16, 8, n_draft=7, draft=fake(vocab=321))
    with pytest.raises(ValueError, match="hint_cap"):
        rama_amd.Server(m, 4, 16, 8, n_draft=7, hint_cap=8, draft=fake())
    with pytest.raises(ValueError, match="slots"):
        rama_amd.Server(m, 65, 128, 8, n_draft=7, draft=fake())
    with pytest.raises(ValueError, match="n_draft"):
        rama_amd.Server(m, 4, 16, 8, n_draft=0, draft=fake())
    with pytest.raises(ValueError, match="another device"):
        rama_amd.Server(m, 4, 16, 8, n_draft=7, draft=fake(device="e"))


def test_group_size_backs_off_until_it_divides():
    from rama_amd.q8 import from_f32_group_size
    for dim, hidden, wanted, want in [(32, 96, 64, 32), (64, 176, 64, 16), (288, 768, 64, 32), (4096, 11008, 64, 64), (128, 352, 64, 32), (48, 40, 64, 8)]:
        cfg = SimpleNamespace(dim=dim, hidden_dim=hidden)
        assert from_f32_group_size(cfg, wanted) == R.group_size(dim, hidden, wanted) == want
    with pytest.raises(ValueError):
        from_f32_group_size(SimpleNamespace(dim=32, hidden_dim=96), 0)


def test_the_restatement_is_q8_refs_rule_group_by_group():
    from tests import q8_ref
    rng = np.random.default_rng(4)
    w = rng.standard_normal(64 * 33).astype(np.float32)
    w[:32] = 0                                                    # a zero group: scale 0, values 0
    w[40] = np.float32(63.5) * (np.abs(w[32:64]).max() / np.float32(127))      # near a half: rounds to even
    for gs in (8, 32, 64):
        q, s = R.quantize_groups(w, gs)
        q2, s2 = q8_ref.quantize_q80(w, gs)
        assert np.array_equal(q, np.asarray(q2).reshape(-1)) and np.array_equal(s.view(np.uint32), np.asarray(s2, np.float32).reshape(-1).view(np.uint32))
    assert not R.quantize_groups(w, 32)[0][:32].any()


# ------------------------------------------------------------------ the GPU tests' workloads, replayed on the host

WORKLOADS = ("ONE", "HOLE", "ARRIVALS", "TWO_TILES", "GUARD")


def _cfg_dict(c):
    return dict(dim=c.dim, hidden_dim=c.hidden_dim, n_layers=c.n_layers, n_heads=c.n_heads, n_kv_heads=c.n_kv_heads, vocab_size=c.vocab_size,
                seq_len=c.seq_len, shared_weight=c.shared_weight)


@pytest.fixture(scope="module")
def replays():
    """(workload, draft) -> serve_model_replay over the TINY target of tests/test_hip_serve_model.py: the CPU oracle's parity tokens are every
    request's solo tokens, and the draft function is tests/q8_ref.py's numpy forward of the draft -- "self": the target's own weights quantized
    by the restatement of rama_q8_model_from_f32; "small": the unrelated synthetic model of the cases.  Computed once."""
    from oracle import oracle as O
    from oracle import synth as S
    from rama_amd.q8_replay import serve_model_replay
    from tests import q8_ref, serve_cases
    cfg = serve_cases.TINY
    rope = S.rope_tables(cfg.seq_len, cfg.head_size)
    w = S.synth_weights(cfg, W.TARGET_SEED, rope=rope)
    orc = O.Oracle(cfg, w)
    gs = R.group_size(cfg.dim, cfg.hidden_dim)
    t, norms, _ = R.from_f32(cfg, w, gs)
    sc = dict(vocab_size=cfg.vocab_size, seq_len=cfg.seq_len, **W.SMALL_DRAFT)
    n2, t2 = q8_ref.synth_q8(sc, W.SMALL_GS, W.SMALL_SEED)
    drafts = dict(self=q8_ref.Q8Ref(_cfg_dict(cfg), gs, norms, t, rope),
                  small=q8_ref.Q8Ref(sc, W.SMALL_GS, n2, t2, S.rope_tables(cfg.seq_len, sc["dim"] // sc["n_heads"])))

    def solo(ctx, new, T, P, U):
        out, tok = [], ctx[0]
        for pos in range(len(ctx) - 1 + new):
            lg = orc.forward(tok, pos)
            if pos + 1 < len(ctx):
                tok = ctx[pos + 1]
            else:
                tok = int(O.argmax(lg)) if T == 0.0 else int(O.sample(lg.copy(), T, P, U))
                out.append(tok)
        return out

    out = {}
    for name in WORKLOADS:
        wl = getattr(W, name)
        ctxs = W.contexts(wl, cfg.vocab_size, W.SEEDS[name])
        solos = [solo(c, new, *samp) for c, (_, new, _, samp, _) in zip(ctxs, wl[3])]
        reqs = [dict(context=c, max_new=new, stop_token=None if stop_at is None else so[stop_at], n_draft=K)
                for c, so, (_, new, K, _, stop_at) in zip(ctxs, solos, wl[3])]
        for kind, ref in drafts.items():
            fns = [lambda prefix, n, ref=ref, s=samp: ref.generate(prefix[1:], len(prefix) - 1 + n, *s)[len(prefix) - 1:] for _, _, _, samp, _ in wl[3]]
            out[name, kind] = (serve_model_replay(reqs, solos, fns, wl[0], wl[1], wl[2]), reqs, solos)
    return out


def test_the_recorded_workloads_reach_every_condition(replays):
    """a condition on the workloads, not a measurement: over the replays every outcome of a drafting slot-step and every state of the second tile"""
    seen = {k: W.conditions(rp) for k, (rp, _, _) in replays.items()}
    assert set().union(*seen.values()) == W.ALL_CONDITIONS, seen
    # ... and each where its workload was chosen for it
    assert "a == 0" in seen["ARRIVALS", "small"] and {"a == g > 0", "0 < a < g"} <= seen["ARRIVALS", "self"]
    assert {"0 < g < want", "g == 0 with a live catch-up row"} <= seen["ARRIVALS", "self"]
    assert "a DECODE slot across row 32" in seen["TWO_TILES", "self"]
    assert {"a live second tile without a logits row", "a wholly idle second tile"} <= seen["GUARD", "small"]
    rp = replays["ONE", "self"][0]
    assert all(g == 0 for st in rp["steps"] for g, _, _, _ in st["drafting"].values()) and rp["counters"]["draft_passes"] > 0


def test_every_replay_emits_the_solo_tokens_whatever_the_draft(replays):
    for (name, kind), (rp, reqs, solos) in replays.items():
        for q, (r, so) in enumerate(zip(reqs, solos)):
            want = so[:so.index(r["stop_token"]) + 1] if r["stop_token"] in so else so
            assert rp["outputs"][q] == want, (name, kind, q)
        assert all(len(r["context"]) <= c <= len(r["context"]) + len(o) for r, o, c in zip(reqs, rp["outputs"], rp["cursor"]) if r["n_draft"]), (name, kind)
    # the draft changes the steps, never the tokens: the unrelated draft needs more of them
    assert len(replays["TWO_TILES", "small"][0]["steps"]) > len(replays["TWO_TILES", "self"][0]["steps"])


def test_the_two_tile_workload_puts_a_decode_slot_across_row_32():
    from rama_amd.q8 import serve_model_replay
    n_slots, max_rows, use, reqs = W.TWO_TILES
    rng = np.random.default_rng(0)
    specs = [dict(context=[1] + [int(t) for t in rng.integers(2, 300, n - 1)], max_new=new, stop_token=None, n_draft=K) for n, new, K, _, _ in reqs]
    refs = [[int(t) for t in rng.integers(2, 300, new)] for _, new, _, _, _ in reqs]

    def right(q):
        return lambda prefix, n: refs[q][len(prefix) - len(specs[q]["context"]):][:n]
    rp = serve_model_replay(specs, refs, [right(q) for q in range(3)], n_slots, max_rows, use)
    assert any(W.straddles(st["rows"]) for st in rp["steps"])
    assert any(st["granted"] == [7, 15, 15, 0] for st in rp["steps"])      # the 40 rows are exactly what the three slots want
    assert all(st["slots"][3][0] == 0 for st in rp["steps"])
