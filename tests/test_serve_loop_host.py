"""One ServeLoop for both servers (no GPU, no library): Q8Server and rama_amd.Server are rama_amd.serve.ServeLoop and state nothing but their
entries' family, their name and their engine; rama_amd.q8 still names everything tests and tools import from it; and over a stand-in
device whose library records (entry, scalar arguments) both servers make the same calls in the same order -- a plain admission, one over
the caller's rows, one over a donor's after the fork, one with drafts, the end -- and refuse a bad request, word for word, before any
call.  The traces and the texts were taken with this stand-in from the commit before the two loop classes were merged."""
import ctypes as C

import pytest

from rama_amd.q8_replay import SERVE_DONE as DONE, SERVE_FREE as FREE, SERVE_PROMPT as PROMPT

ABIS = ["rama_q8_serve", "rama_serve"]

# every name tests/ and tools/ import from rama_amd.q8, or reach as an attribute of it (a grep of both trees before the move)
Q8_NAMES = ["PrefixPool", "Q8Engine", "Q8Server", "ServeLoop", "_draft_py", "_drain", "_spec_plan_py", "chain_plan", "common_prefix",
            "decode_batch", "decode_batch_chained", "serve_plan", "serve_plan_step", "serve_sizes", "serve_spec_plan_step",
            "serve_spec_replay", "serve_spec_report", "serve_spec_request", "serve_spec_sizes", "spec_accept", "spec_draft", "spec_plan",
            "spec_replay", "spec_report"]


# ------------------------------------------------------------------ structure

def test_both_servers_are_the_one_loop_and_state_only_their_family():
    import rama_amd
    from rama_amd import q8, serve
    from rama_amd.q8 import Q8Server
    from rama_amd.serve import ServeLoop
    from rama_amd.server import Server
    assert Q8Server.__mro__[1:] == Server.__mro__[1:] == (ServeLoop, object)
    assert q8.ServeLoop is ServeLoop is serve.ServeLoop and rama_amd.Server is Server and rama_amd.Q8Server is Q8Server
    for cls in (Q8Server, Server):
        own = {k for k in vars(cls) if not (k.startswith("__") and k.endswith("__")) or k == "__init__"}
        assert own == {"ABI", "NAME", "__init__", "_new_engine"}, (cls, own)
        assert cls.__doc__
    assert (Q8Server.ABI, Q8Server.NAME, Server.ABI, Server.NAME) == ("rama_q8_serve", "Q8Server", "rama_serve", "Server")
    assert not hasattr(q8, "CachingServeLoop") and not hasattr(serve, "CachingServeLoop")
    assert (ServeLoop.LOOKAHEAD, ServeLoop.SPEC_BLOCK, ServeLoop.MIN_CACHED) == (2, 4, 2)


def test_the_loop_knows_no_engine_class():
    import types

    from rama_amd import engine, q8, serve
    for name, v in vars(serve).items():
        assert v is not q8.Q8Engine and v is not engine.Engine and v is not q8.Q8Model and v is not engine.Model, name
        assert not (isinstance(v, types.ModuleType) and v.__name__ in ("rama_amd.q8", "rama_amd.engine", "rama_amd.server")), name


def test_q8_still_names_what_tests_and_tools_import_from_it():
    from rama_amd import _host, q8, serve
    for name in Q8_NAMES:
        assert hasattr(q8, name), name
    for name in ("PrefixPool", "ServeLoop", "common_prefix", "serve_plan", "serve_plan_step", "serve_sizes", "serve_spec_plan_step",
                 "serve_spec_report", "serve_spec_request", "serve_spec_sizes"):
        assert getattr(q8, name) is getattr(serve, name), name
    for name in ("MAX_BATCH", "MAX_DRAFT", "MAX_NGRAM", "_drain"):
        assert getattr(q8, name) is getattr(_host, name), name


# ------------------------------------------------------------------ the stand-in device

class Lib:
    """records (entry, scalar arguments) and answers 0.  A poll of a slot in `finish` gives that slot's tokens and a set finished word, of
    any other slot nothing; stats gives the slot table `slots`."""

    def __init__(self):
        self.calls, self.finish, self.slots = [], {}, []

    def __getattr__(self, name):
        def entry(*a):
            self.calls.append((name, tuple(v for v in a if isinstance(v, (int, float)))))
            if name.endswith("_serve_poll"):               # (ctx, slot, start, tokens, 64, &n, &finished, NULL)
                toks = self.finish.get(a[1], [])[a[2]:a[2] + a[4]]
                for i, t in enumerate(toks):
                    a[3][i] = t
                a[5]._obj.value, a[6]._obj.value = len(toks), int(a[1] in self.finish)
            if name.endswith("_serve_stats"):              # (ctx, &report)
                r = a[1]._obj
                r.n_slots, r.max_rows = len(self.slots), 4
                for i, s in enumerate(self.slots):
                    r.slots[i].state, r.slots[i].n_context, r.slots[i].cursor, r.slots[i].n_out, r.slots[i].max_new = s
            return 0
        return entry


class Cfg:
    vocab_size, seq_len = 512, 64


class Model:
    def __init__(self, cfg=Cfg):
        class Device:
            lib, ctx = Lib(), None
        self.device, self.cfg, self.ccfg, self.weights = Device(), cfg(), C.c_int(), C.c_int()


class Engine:
    def __init__(self, device, model):
        self.model, self.state, self.freed = model, C.c_int(), False

    def free(self):
        self.freed = True


@pytest.fixture(params=ABIS)
def stand_in(request, monkeypatch):
    """-> (the server class of the ABI, its ABI, its NAME), its engines the stand-in's"""
    import rama_amd
    from rama_amd import q8, server
    monkeypatch.setattr(q8, "Q8Engine", Engine)
    monkeypatch.setattr(server, "Engine", Engine)
    cls = {"rama_q8_serve": rama_amd.Q8Server, "rama_serve": rama_amd.Server}[request.param]
    return cls, request.param, cls.NAME


def trace(model, clear=True):
    """the calls recorded so far, the polls apart"""
    out = [c for c in model.device.lib.calls if not c[0].endswith("_poll")]
    if clear:
        del model.device.lib.calls[:]
    return out


# ------------------------------------------------------------------ same calls, same order

def test_plain_and_caller_cached_admissions(stand_in):
    cls, A, _ = stand_in
    m = Model()
    srv = cls(m, 2, 4, 8)
    h = srv.submit([1, 2, 3], 4)
    assert trace(m) == [(A + "_begin", (2, 4, 8)), (A + "_admit", (0, 3))]
    assert srv.cached(h) == 0 and not srv.spec and len(srv.pool) == 0
    e = Engine(None, m)
    h = srv.submit([1, 2, 3, 4, 5], 2, engine=e, n_cached=3)
    assert trace(m) == [(A + "_admit_at", (1, 5, 3))]
    assert srv.cached(h) == 3 and srv.rows_cached == 3 and srv._mirror[1] == (PROMPT, 5, 3, 0, 2)
    st = srv.stats()
    assert trace(m) == [(A + "_stats", ())] and "spec" not in st and st["rows_cached"] == 3
    srv.close()
    srv.close()
    assert trace(m) == [(A + "_end", ())] and not e.freed


def test_donor_match_forks_then_admits_at_and_a_short_match_does_not(stand_in):
    cls, A, _ = stand_in
    m = Model()
    lib = m.device.lib
    srv = cls(m, 2, 4, 8, prefix_cache=1)
    h0 = srv.submit([1, 2, 3, 4, 5], 1, retain=True)
    assert trace(m) == [(A + "_begin", (2, 4, 8)), (A + "_admit", (0, 5))]
    lib.finish, lib.slots = {0: [42]}, [(DONE, 5, 5, 1, 1), (FREE, 0, 0, 0, 0)]
    srv.poll()                                                      # the finish was not foreseen: the slot table is taken again
    lib.finish = {}
    assert trace(m) == [(A + "_stats", ())]
    assert srv.finished(h0) and srv.result(h0) == [42] and len(srv.pool) == 1 and srv._own[0] is None
    donor = srv.pool.engines()[0]
    h1 = srv.submit([1, 2, 3, 4, 9, 9], 1)                          # shares 4 tokens with the donor
    assert trace(m) == [("rama_q8_kv_fork", (1, 4)), (A + "_admit_at", (0, 6, 4))]
    assert srv.cached(h1) == 4 and srv._eng[0] is not donor and donor in srv.pool
    h2 = srv.submit([1, 7, 7], 1)                                   # shares BOS alone: shorter than MIN_CACHED
    assert trace(m) == [(A + "_admit", (1, 3))]
    assert srv.cached(h2) == 0 and srv.rows_cached == 4
    made = list(srv._mine)
    srv.close()
    assert trace(m) == [(A + "_end", ())] and len(srv.pool) == 0
    assert len(made) == 3 and any(e is donor for e in made) and all(e.freed for e in made)


def test_drafting_server_begins_admits_and_reports_through_the_spec_entries(stand_in):
    cls, A, _ = stand_in
    m = Model()
    srv = cls(m, 2, 4, 8, n_draft=2, hint_cap=4)
    h = srv.submit([1, 2, 3], 4, hint=[5, 6])
    assert trace(m) == [(A + "_begin_spec", (2, 4, 8, 2, 4)), (A + "_admit_spec", (0, 3, 0))]
    e = Engine(None, m)
    srv.submit([1, 2, 3, 4], 4, engine=e, n_cached=2, n_draft=0)
    assert trace(m) == [(A + "_admit_spec", (1, 4, 2))]
    assert srv.spec and srv.cached(h) == 0
    m.device.lib.slots = [(PROMPT, 3, 0, 0, 4), (PROMPT, 4, 2, 0, 4)]
    st = srv.stats()
    assert trace(m) == [(A + "_stats", ()), (A + "_spec_stats", ())] and "spec" in st and st["slots"] == m.device.lib.slots
    srv.close()
    assert trace(m) == [(A + "_end", ())]


def test_every_size_is_refused_before_any_call_in_its_order(stand_in):
    cls, _, N = stand_in
    m = Model()
    for kw, text in ((dict(n_slots=0, n_draft=99, prefix_cache=-1), f"{N}: 0 slots, not 1..128"),
                     (dict(max_rows=1, n_draft=99, prefix_cache=-1), f"{N}: max_rows 1 outside [n_slots = 2, 128]"),
                     (dict(max_new_cap=64, n_draft=99), f"{N}: max_new_cap 64 outside [1, seq_len - 1 = 63]"),
                     (dict(n_draft=99, prefix_cache=-1), f"{N}: n_draft 99 outside [0, 15]"),
                     (dict(n_draft=2, ngram=5, prefix_cache=-1), f"{N}: ngram 5 outside [1, 4]"),
                     (dict(hint_cap=4, prefix_cache=-1), f"{N}: hint_cap 4 (>= 0, and 0 on a server without drafts)"),
                     (dict(prefix_cache=-1), "PrefixPool: -1 donors")):
        args = dict(dict(n_slots=2, max_rows=4, max_new_cap=8), **kw)
        with pytest.raises(ValueError) as e:
            cls(m, **args)
        assert str(e.value) == text
    assert m.device.lib.calls == []


class BigVocab:
    vocab_size, seq_len = 40000, 64


def test_submit_refuses_once_each_in_its_order_before_any_call(stand_in):
    cls, _, N = stand_in
    m, W = Model(), f"{N}.submit"
    srv = cls(m, 2, 4, 8, n_draft=2, hint_cap=3, prefix_cache=2)
    mine, other, busy, donor = Engine(None, m), Engine(None, Model()), Engine(None, m), Engine(None, m)
    srv.submit([1, 2, 3], 1, engine=busy)
    srv.pool.put([1, 2, 3], donor)
    both = Engine(None, Model())                                    # another model's engine that is a donor too
    srv.pool.put([4], both)
    trace(m)
    cases = [
        (dict(context=[]), f"{W}: an empty context (the caller includes BOS)"),
        (dict(context=[1, 512]), f"{W}: token 512 outside the vocabulary [0, 512)"),
        (dict(n_cached=3, engine=mine), f"{W}: n_cached 3 outside [0, n_context - 1 = 2] (the final context position is always fed)"),
        (dict(n_cached=-1, engine=mine), f"{W}: n_cached -1 outside [0, n_context - 1 = 2] (the final context position is always fed)"),
        (dict(temperature=-1.0, u=0.0), f"{W}: temperature >= 0, topp in [0, 1], u in [0, 1) -- not -1.0, 0.9, 0.0"),
        (dict(topp=1.5, u=0.25), f"{W}: temperature >= 0, topp in [0, 1], u in [0, 1) -- not 0.0, 1.5, 0.25"),
        (dict(max_new=0), f"{W}: max_new 0 < 1"),
        (dict(max_new=9), f"{W}: max_new 9 beyond the server's max_new_cap 8"),
        (dict(context=[1] * 60, max_new=5), f"{W}: 60 context tokens + 5 new ones beyond seq_len 64"),
        (dict(stop_token=512), f"{W}: stop token 512 outside the vocabulary [0, 512)"),
        (dict(n_draft=3), f"{W}: n_draft 3 outside [0, the server's n_draft = 2]"),
        (dict(hint=[512]), f"{W} hint: token 512 outside the vocabulary [0, 512)"),
        (dict(hint=[1, 2, 3, 4]), f"{W}: 4 hint tokens beyond the server's hint_cap 3"),
        (dict(n_cached=1), f"{W}: n_cached needs the engine that holds the rows"),
        (dict(engine=other), f"{W}: the engine belongs to another Model"),
        (dict(engine=busy), f"{W}: the engine already serves a queued or running request"),
        (dict(engine=donor), f"{W}: the engine is a donor of the prefix cache"),
        # two faults: the earlier refusal speaks
        (dict(max_new=0, n_draft=3), f"{W}: max_new 0 < 1"),
        (dict(n_draft=3, n_cached=1), f"{W}: n_draft 3 outside [0, the server's n_draft = 2]"),
        (dict(n_cached=1, hint=[512]), f"{W} hint: token 512 outside the vocabulary [0, 512)"),
        (dict(engine=both), f"{W}: the engine belongs to another Model"),
    ]
    for kw, text in cases:
        args = dict(dict(context=[1, 2, 3], max_new=4), **kw)
        with pytest.raises(ValueError) as e:
            srv.submit(**args)
        assert str(e.value) == text, kw
    # a running engine that is a donor as well: it is refused as running
    srv.pool.clear()
    srv.pool.put([9], busy)
    with pytest.raises(ValueError) as e:
        srv.submit([1, 2, 3], 4, engine=busy)
    assert str(e.value) == f"{W}: the engine already serves a queued or running request"
    assert trace(m) == [] and srv._queue == [] and srv._next == 1      # no call, and no handle was spent
    big = Model(BigVocab)
    with pytest.raises(ValueError) as e:
        cls(big, 2, 4, 8).submit([1, 2, 3], 4, temperature=0.5)
    assert str(e.value) == f"{W}: a sampled plan needs vocab_size <= 32768"
    assert [c[0] for c in trace(big)] == [cls.ABI + "_begin"]
