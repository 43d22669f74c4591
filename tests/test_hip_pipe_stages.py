"""-m gpu: N pipeline stages on ONE GPU, driven by the native tick plan (csrc/pipe.hip rama_pipe_tick_plan).  One process stands for
world N: every rank has its own context (stream), its stage of the model (split_layers; the embedding on rank 0 only, the classifier
on the last rank only), one run state and one device token word per sequence.  Per tick every rank's plan is executed with the calls
rama_pipe_run_ticks makes (tests/pipe_plan_cases.py execute_tick: rama_forward_stage for BOS and forced tokens,
rama_forward_stage_devtok -- with a NULL token on ranks > 0 -- for the rest, then rama_argmax_dev / rama_sample_topp_dev), every
context is synchronised, and the tick's legs travel through the host where RCCL would send and receive: all send buffers are read
before any receive lands, as in a grouped exchange.  Rank 0 files every received token at history[recv_seq, recv_pos].

synth_d288_h6 has two layers, so the worlds here also hold what an even split never shows: at world 3 the last stage only
classifies (layers 1, 1, 0), at world 4 rank 2 neither embeds, nor owns a layer, nor classifies (layers 1, 1, 0, 0): x passes through.

The history must equal generate() of the whole model (tests/pipe_plan_cases.py reference) at every position of every sequence.  In
parity mode the last rank's logits and every rank's key / value cache rows of its own layers are the oracle's bit for bit; in fast mode
the logits are within LOGIT_ATOL, and the tokens are comparable because the reference is decisive at every sampled position (a
top-two gap above 2 LOGIT_ATOL, asserted on the CPU before the GPU is touched)."""
import ctypes as C

import numpy as np
import pytest

from . import pipe_plan_cases as P
from .helpers import LOGIT_ATOL, load_case, to_rama_cfg

pytestmark = pytest.mark.gpu

CASE = "synth_d288_h6"
PROMPT_WINDOW = (1, 4)      # g["tokens"][1:4]: the reference's top-two gap exceeds 2 LOGIT_ATOL at all 16 positions of the fast case


class GpuStage:
    """one rank of the emulated world: context, stage model, states and token words; the backend of execute_tick"""

    def __init__(self, cfg, g, rank, world, n_seq, sampler, parity, graph):
        import rama_amd
        from rama_amd._lib import check, rama_run_state, rama_stage
        from rama_amd.pipeline import split_layers
        self.check, self.rank, self.world, self.sampler, self.vocab = check, rank, world, sampler, cfg.vocab_size
        self.lo, self.hi = split_layers(cfg.n_layers, world, rank)
        self.stage = rama_stage(self.lo, self.hi, int(rank == 0), int(rank == world - 1))
        self.dev = rama_amd.Hip(0)
        self.model, self.states, self.toks = None, [], []
        L = self.dev.lib
        check(L.rama_set_tuning(self.dev.ctx, b"ref_order", parity), "rama_set_tuning")
        self.model = rama_amd.Model.synth(self.dev, to_rama_cfg(cfg), int(g["seed"]), self.stage, rope=(g["freq_cis_real"], g["freq_cis_imag"]))
        for _ in range(n_seq):
            st = rama_run_state()
            check(L.rama_state_create(self.dev.ctx, C.byref(self.model.ccfg), self.hi - self.lo, C.byref(st)), "rama_state_create")
            self.states.append(st)
            self.toks.append(self.dev.alloc(1))
        if sampler[0] != 0.0 and rank == world - 1:      # the device sampler's scratch is sized outside the loop
            check(L.rama_sample_topp_dev(self.dev.ctx, self.states[0].logits, self.vocab, *sampler, self.toks[0].ptr), "rama_sample_topp_dev")
        check(L.rama_set_graph_mode(self.dev.ctx, graph), "rama_set_graph_mode")      # 1: one hipGraph per (sequence state, stage, attention variant)
        self.dev.sync()

    def _args(self, seq):
        return self.dev.ctx, C.byref(self.model.ccfg), C.byref(self.model.weights), C.byref(self.states[seq])

    def compute(self, seq, pos, token):
        L = self.dev.lib
        if token is not None:
            self.check(L.rama_forward_stage(*self._args(seq), int(token), pos, C.byref(self.stage)), "rama_forward_stage")
        else:
            self.check(L.rama_forward_stage_devtok(*self._args(seq), self.toks[seq].ptr if self.rank == 0 else None, pos, C.byref(self.stage)),
                       "rama_forward_stage_devtok")

    def sample(self, seq):
        L, logits, tok = self.dev.lib, self.states[seq].logits, self.toks[seq].ptr
        if self.sampler[0] == 0.0:
            self.check(L.rama_argmax_dev(self.dev.ctx, logits, self.vocab, tok), "rama_argmax_dev")
        else:
            self.check(L.rama_sample_topp_dev(self.dev.ctx, logits, self.vocab, *self.sampler, tok), "rama_sample_topp_dev")

    def buffer(self, kind, seq):
        return (self.states[seq].x, self.model.cfg.dim) if kind == P.X else (self.toks[seq].ptr, 1)

    def read(self, ptr, n):
        out = np.empty(n, dtype=np.float32)
        self.check(self.dev.lib.rama_download_f32(self.dev.ctx, ptr, n, out.ctypes.data), "rama_download_f32")
        return out

    def write(self, ptr, data):
        self.check(self.dev.lib.rama_copy_h2d_f32(self.dev.ctx, ptr, data.ctypes.data, data.size), "rama_copy_h2d_f32")

    def quiet(self):
        """graphs go before the states they were captured over (rama_state_free), parity mode before the next test's contexts"""
        self.dev.lib.rama_set_graph_mode(self.dev.ctx, 0)
        self.dev.lib.rama_set_tuning(self.dev.ctx, b"ref_order", 0)

    def free(self):
        for st in self.states:
            self.dev.lib.rama_state_free(self.dev.ctx, C.byref(st))
        for t in self.toks:
            t.free()
        if self.model is not None:
            self.model.free()
        self.dev.close()


def drive(lib, plan, ranks, n_seq, n_pos):
    """every tick of the plan for every rank -> the history rank 0 collects"""
    world = len(ranks)
    history = np.full((n_seq, n_pos), -1, dtype=np.int64)
    for t in range(P.plan_ticks(lib, plan, world)):
        legs = [P.execute_tick(P.tick(lib, plan, world, r, t), r, ranks[r]) for r in range(world)]
        for be in ranks:
            be.dev.sync()
        flying = {}      # all send buffers first ...
        for r, (send, _) in enumerate(legs):
            if send is not None:
                kind, seq, peer = send
                assert 0 <= peer < world and 0 <= seq < n_seq, (t, r, send)
                flying[(r, peer, kind, seq)] = ranks[r].read(*ranks[r].buffer(kind, seq))
        for r, (_, recv) in enumerate(legs):      # ... then the receives
            if recv is None:
                continue
            kind, seq, peer, recv_pos = recv
            assert 0 <= seq < n_seq, (t, r, recv)
            data = flying.pop((peer, r, kind, seq))
            ranks[r].write(ranks[r].buffer(kind, seq)[0], data)
            if kind == P.TOKEN:
                assert r == 0 and 0 <= recv_pos < n_pos, (t, r, recv)
                history[seq, recv_pos] = int(data.view(np.int32)[0])
        assert not flying, (t, flying)
    return history


_refs = {}


def reference_for(n_pos, wrap, sampler):
    """one reference per (n_pos, wrap, sampler), shared by the cases and left unchanged"""
    key = (n_pos, wrap, sampler)
    if key not in _refs:
        cfg, w, g = load_case(CASE)
        _refs[key] = P.reference(cfg, w, g["tokens"].tolist()[PROMPT_WINDOW[0]:PROMPT_WINDOW[1]], n_pos, wrap, *sampler)
    return _refs[key]


GREEDY = (0.0, 0.9, 0.0)
SAMPLED = (1.0, 0.9, P.U_CONST)


@pytest.mark.parametrize("world,n_seq,n_pos,parity,graph,sampler,wrap", [
    (2, 2, 16, 1, 0, GREEDY, 0),
    (3, 3, 16, 1, 1, GREEDY, 0),       # a middle stage, which neither embeds nor classifies
    (4, 5, 12, 1, 0, GREEDY, 0),       # more sequences than stages; one stage without any work of its own
    (3, 1, 12, 1, 1, GREEDY, 0),       # one sequence: two of every three ticks are idle on each rank
    (3, 3, 12, 1, 1, SAMPLED, 0),
    (2, 3, 20, 1, 0, GREEDY, 8),       # every slot starts a new generation every 8 positions
    (3, 3, 16, 0, 1, GREEDY, 0),       # fast mode
])
def test_tick_plan_drives_stages_on_one_gpu(world, n_seq, n_pos, parity, graph, sampler, wrap):
    import rama_amd
    cfg, w, g = load_case(CASE)
    prompt = g["tokens"].tolist()[PROMPT_WINDOW[0]:PROMPT_WINDOW[1]]
    assert len(prompt) == 3 and (wrap or n_pos) <= cfg.seq_len
    ref = reference_for(n_pos, wrap, sampler)
    if not parity:      # the tokens of a run that is only close to the oracle are comparable where the oracle is decisive: everywhere, here
        print("fast case: smallest top-two gap of the reference %.6g at position %d (bound %.1e)" % (min(ref.gaps), int(np.argmin(ref.gaps)), 2 * LOGIT_ATOL))
        assert min(ref.gaps) > 2 * LOGIT_ATOL, ref.gaps
    lib = rama_amd.load()
    plan = P.make_plan(n_seq, n_pos, wrap, prompt, *sampler)
    ranks = []
    try:
        for r in range(world):
            ranks.append(GpuStage(cfg, g, r, world, n_seq, sampler, parity, graph))
        history = drive(lib, plan, ranks, n_seq, n_pos)
        for s in range(n_seq):
            assert history[s].tolist() == ref.history, (s, history[s].tolist(), ref.history)
        last, want = ranks[-1], ref.oracle.s["logits"]
        for s in range(n_seq):
            got = last.read(last.states[s].logits, cfg.vocab_size)
            if parity:
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (s, float(np.abs(got - want).max()))
            else:
                assert np.abs(got - want).max() <= LOGIT_ATOL, (s, float(np.abs(got - want).max()))
        if parity:      # every rank's cache rows of its own layers, for the positions written
            rows, per = (min(wrap, n_pos) if wrap else n_pos) * cfg.dim, cfg.seq_len * cfg.dim
            for be in ranks:
                for s in range(n_seq):
                    for name in ("key_cache", "value_cache"):
                        for layer in range(be.lo, be.hi):
                            got = be.read(getattr(be.states[s], name) + 4 * (layer - be.lo) * per, rows)
                            want_rows = ref.oracle.s[name][layer * per:layer * per + rows]
                            assert np.array_equal(got.view(np.uint32), want_rows.view(np.uint32)), (be.rank, s, name, layer)
    finally:
        for be in ranks:
            be.quiet()
        for be in ranks:
            be.free()
