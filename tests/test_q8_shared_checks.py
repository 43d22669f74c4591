"""What the Q8 entries share on the host (q8_host.hpp / q8_api.hip: the check_* refusals, q8_chains): every entry that goes through a shared check
refuses with RAMA_EINVAL in its OWN words -- rama_last_error starts with that entry's prefix and the text it has always had --, and
freeing the model ends all three chains begun on one context, each _steps entry refusing with its own text.  The two plan functions
are pure host functions; everything else needs a context, hence a GPU."""
import ctypes as C

import numpy as np
import pytest

EINVAL = -1
FREE, PROMPT, DECODE, DONE = 0, 1, 2, 3
WHICH = "ckpt_v2_q80_untied"


def refusal(rc, entry, what):
    """the call returned RAMA_EINVAL and left `<entry>: <what>` as the error text"""
    from rama_amd._lib import load
    msg = (load().rama_last_error() or b"").decode()
    assert rc == EINVAL and msg.startswith(f"{entry}: {what} (rama error -1)"), (rc, msg, entry, what)


# ------------------------------------------------------------------ the plan functions (no GPU)

@pytest.mark.parametrize("entry", ["q8_serve_plan_step", "q8_serve_spec_plan_step"])
def test_plan_functions_refuse_a_bad_slot_table_in_their_own_words(entry):
    from rama_amd._lib import load, rama_q8_serve_row, rama_q8_serve_slot
    L = load()

    def call(slots, max_rows, n_slots=None):
        n = len(slots) if n_slots is None else n_slots
        arr = (rama_q8_serve_slot * max(len(slots), 1))(*[rama_q8_serve_slot(*s) for s in slots])
        rows = (rama_q8_serve_row * 128)()
        if entry == "q8_serve_plan_step":
            return L.rama_q8_serve_plan_step(arr, n, max_rows, rows, None)
        return L.rama_q8_serve_spec_plan_step(arr, n, max_rows, (C.c_int32 * 128)(), rows, (C.c_int32 * 128)())

    good = [(PROMPT, 5, 0, 0, 4), (DECODE, 3, 4, 2, 6), (FREE, 0, 0, 0, 0), (DONE, 2, 3, 2, 2)]
    assert call(good, 8) == 0
    for n_slots, max_rows in ((0, 8), (4, 3), (4, 129), (129, 128)):
        refusal(call(good, max_rows, n_slots), entry, "1 <= n_slots <= max_rows <= 128")
    for bad, what in (((4, 1, 0, 0, 1), "bad slot state"), ((-1, 1, 0, 0, 1), "bad slot state"),
                      ((PROMPT, 0, 0, 0, 4), "bad PROMPT slot"), ((PROMPT, 5, 5, 0, 4), "bad PROMPT slot"), ((PROMPT, 5, 0, 0, 0), "bad PROMPT slot"),
                      ((DECODE, 3, -1, 2, 6), "bad DECODE slot"), ((DECODE, 3, 4, 0, 6), "bad DECODE slot"), ((DECODE, 3, 4, 6, 6), "bad DECODE slot")):
        refusal(call(good[:2] + [bad], 8), entry, what)
    # the order of the refusals is each function's own: a slot's drafts are judged before the next slot's state
    if entry == "q8_serve_spec_plan_step":
        arr = (rama_q8_serve_slot * 2)(rama_q8_serve_slot(*good[0]), rama_q8_serve_slot(7, 0, 0, 0, 0))
        want = (C.c_int32 * 2)(1, 0)
        rc = L.rama_q8_serve_spec_plan_step(arr, 2, 8, want, (rama_q8_serve_row * 8)(), (C.c_int32 * 2)())
        refusal(rc, entry, "only a DECODE slot drafts, and at most max_new - n_out - 1 tokens")


# ------------------------------------------------------------------ the entries that need a context

@pytest.fixture(scope="module")
def dev():
    import rama_amd
    d = rama_amd.Hip(0)
    yield d
    d.close()


def arr(v):
    return (C.c_int32 * max(len(v), 1))(*v)


class Calls:
    """the raw entries over one model and one engine per chain, every argument good unless named"""

    def __init__(self, dev, golden_dir):
        import rama_amd
        self.dev, self.L = dev, dev.lib
        self.m = rama_amd.Q8Model.load(dev, golden_dir / f"{WHICH}.bin")
        self.V = self.m.cfg.vocab_size
        self.engs = [rama_amd.Q8Engine(dev, self.m) for _ in range(3)]      # the chained batch's, the serving chain's, the speculative chain's

    def head(self, eng):
        return self.dev.ctx, C.byref(self.m.ccfg), C.byref(self.m.weights), C.byref(eng.state)

    def generate(self, prompt):
        return self.L.rama_q8_generate(*self.head(self.engs[0]), arr(prompt), len(prompt), 4, 0.0, 0.9, 0.0, (C.c_int32 * 8)())

    def prefill(self, toks):
        return self.L.rama_q8_prefill(*self.head(self.engs[0]), arr(toks), len(toks), 0)

    def chain_begin(self, T=0.0, P=0.9, u=0.0, forced=(), stop=-1):
        from rama_amd._lib import rama_q8_seq_plan, rama_run_state
        f = arr(list(forced))
        plan = (rama_q8_seq_plan * 1)(rama_q8_seq_plan(T, P, u, f, len(forced), 0, stop))
        return self.L.rama_q8_decode_batch_begin(*self.head(self.engs[0])[:3], (rama_run_state * 1)(self.engs[0].state), arr([1]), arr([0]), 1, 4, plan)

    def serve_begin(self, n_slots=2, max_rows=4, spec=False):
        head = self.head(self.engs[1])[:3]
        if spec:
            return self.L.rama_q8_serve_begin_spec(*head, n_slots, max_rows, 4, 3, 8)
        return self.L.rama_q8_serve_begin(*head, n_slots, max_rows, 4)

    def admit(self, ctx=(1, 2), T=0.0, P=0.9, u=0.0, stop=-1, spec=None):
        from rama_amd._lib import rama_q8_serve_plan, rama_q8_serve_spec
        plan, state = rama_q8_serve_plan(T, P, u, 3, stop), C.byref(self.engs[1].state)
        if spec is None:
            return self.L.rama_q8_serve_admit(self.dev.ctx, 0, state, arr(list(ctx)), len(ctx), C.byref(plan))
        K, N, hint, n_hint = spec
        h = arr(list(hint))
        s = rama_q8_serve_spec(K, N, h if hint else None, len(hint) if n_hint is None else n_hint)
        return self.L.rama_q8_serve_admit_spec(self.dev.ctx, 0, state, arr(list(ctx)), len(ctx), 0, C.byref(plan), C.byref(s))

    def spec_begin(self, ctx=(1, 2), T=0.0, P=0.9, u=0.0, stop=-1, K=2, N=2, hint=(), n_hint=None):
        from rama_amd._lib import rama_q8_spec_plan
        h = arr(list(hint))
        plan = rama_q8_spec_plan(T, P, u, 3, stop, K, N, h if hint else None, len(hint) if n_hint is None else n_hint)
        return self.L.rama_q8_spec_begin(*self.head(self.engs[2]), arr(list(ctx)), len(ctx), C.byref(plan))

    def end(self):
        self.L.rama_q8_serve_end(self.dev.ctx)
        self.L.rama_q8_spec_end(self.dev.ctx)

    def free(self):
        self.end()
        for e in self.engs:
            e.free()
        self.m.free()


@pytest.mark.gpu
def test_every_entry_refuses_through_a_shared_check_in_its_own_words(dev, golden_dir):
    c = Calls(dev, golden_dir)
    V = c.V
    try:
        # every token of a list is in the vocabulary
        refusal(c.generate([3, V]), "q8_generate", "prompt token outside the vocabulary")
        refusal(c.prefill([1, 2, -1]), "q8_prefill", "token outside the vocabulary")
        refusal(c.chain_begin(forced=[2, V]), "q8_decode_batch_begin", "forced token outside the vocabulary")
        refusal(c.spec_begin(ctx=(1, V)), "q8_spec_begin", "token outside the vocabulary")
        refusal(c.spec_begin(hint=(2, -3)), "q8_spec_begin", "hint token outside the vocabulary")
        # the sampler's parameters and the stop token
        for bad in (dict(T=-1.0), dict(P=1.5), dict(u=1.0)):
            refusal(c.chain_begin(**bad), "q8_decode_batch_begin", "temperature >= 0, topp in [0,1], u in [0,1)")
            refusal(c.spec_begin(**bad), "q8_spec_begin", "temperature >= 0, topp in [0,1], u in [0,1)")
        for stop in (V, -2):
            refusal(c.chain_begin(stop=stop), "q8_decode_batch_begin", "stop token outside the vocabulary")
            refusal(c.spec_begin(stop=stop), "q8_spec_begin", "stop token outside the vocabulary")
        # ... rama_q8_decode_batch_begin judges the forced list between the two
        refusal(c.chain_begin(forced=[V], stop=V), "q8_decode_batch_begin", "forced token outside the vocabulary")
        # the drafting fields
        refusal(c.spec_begin(K=16), "q8_spec_begin", "n_draft outside 0..15")
        refusal(c.spec_begin(N=5), "q8_spec_begin", "ngram outside 1..4")
        refusal(c.spec_begin(n_hint=2), "q8_spec_begin", "bad hint")
        # the serving chain's geometry and admissions
        for n_slots, max_rows in ((0, 4), (4, 3), (2, 129)):
            refusal(c.serve_begin(n_slots, max_rows), "q8_serve_begin", "1 <= n_slots <= max_rows <= 128")
        assert c.serve_begin(spec=True) == 0
        refusal(c.admit(ctx=(1, V)), "q8_serve_admit", "token outside the vocabulary")
        for bad in (dict(T=-1.0), dict(P=1.5), dict(u=1.0)):
            refusal(c.admit(**bad), "q8_serve_admit", "temperature >= 0, topp in [0,1], u in [0,1)")
        refusal(c.admit(stop=V), "q8_serve_admit", "stop token outside the vocabulary")
        refusal(c.admit(spec=(4, 2, (), None)), "q8_serve_admit_spec", "n_draft beyond rama_q8_serve_begin_spec's n_draft_cap")
        refusal(c.admit(spec=(2, 0, (), None)), "q8_serve_admit_spec", "ngram outside 1..4")
        refusal(c.admit(spec=(2, 2, [2] * 9, None)), "q8_serve_admit_spec", "bad hint, or one beyond rama_q8_serve_begin_spec's hint_cap")
        refusal(c.admit(spec=(2, 2, (), 3)), "q8_serve_admit_spec", "bad hint, or one beyond rama_q8_serve_begin_spec's hint_cap")
        refusal(c.admit(spec=(2, 2, (2, V), None)), "q8_serve_admit_spec", "hint token outside the vocabulary")
        # nothing above touched the chain: a good admission goes in and runs
        assert c.admit(spec=(2, 2, (1, 2, 3), None)) == 0 and c.L.rama_q8_serve_steps(dev.ctx, 2) == 0 and c.L.rama_sync(dev.ctx) == 0
    finally:
        c.free()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_freeing_the_model_ends_all_three_chains(dev, golden_dir, graph):
    """the three chains begun on one context over one model, each stepped (its graph captured); rama_q8_model_free ends every one"""
    c = Calls(dev, golden_dir)
    L = c.L
    rng = np.random.default_rng(3)
    ctx = [1] + [int(t) for t in rng.integers(2, c.V, 3)]
    try:
        assert L.rama_set_graph_mode(dev.ctx, graph) == 0
        c.engs[2].prefill(ctx[:-1], 0)
        assert c.chain_begin() == 0 and c.serve_begin() == 0 and c.admit(ctx=ctx) == 0 and c.spec_begin(ctx=ctx) == 0
        for _ in range(2):
            assert L.rama_q8_decode_batch_steps(dev.ctx, 1) == 0 and L.rama_q8_serve_steps(dev.ctx, 1) == 0 and L.rama_q8_spec_steps(dev.ctx, 1) == 0
        assert L.rama_sync(dev.ctx) == 0
        c.m.free()
        refusal(L.rama_q8_decode_batch_steps(dev.ctx, 1), "q8_decode_batch_steps", "the chain's model or one of its run states has been freed")
        refusal(L.rama_q8_serve_steps(dev.ctx, 1), "q8_serve_steps", "the chain's model or the run state of an occupied slot has been freed")
        refusal(L.rama_q8_spec_steps(dev.ctx, 1), "q8_spec_steps", "the chain's model or its run state has been freed")
    finally:
        L.rama_set_graph_mode(dev.ctx, 0)
        c.free()
