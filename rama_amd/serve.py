"""The serving chains' host loop: continuous batching over the C entries rama_q8_serve_* (Q8Server) and rama_serve_* (rama_amd.Server,
parity mode).  The checked sizes and requests, the scheduling rules as host functions, the donor pool of the prefix cache, and ServeLoop:
the queue, the mirror of the device's slot table, admissions, the rings and the run loops.  Nothing here knows a model's or an engine's
class: a server names its entries' family and makes its engines."""
from __future__ import annotations

import ctypes as C

from ._host import (MAX_BATCH, _check_budget, _check_context, _check_drafting, _check_n_draft, _check_sampled_vocab, _check_sampler,
                    _check_stop, _drain, _i32, _report, _ring_poll, _row_table, _slot_table, _stream_busy, _tokens)
from ._lib import (check, load, rama_q8_serve_model_report, rama_q8_serve_plan, rama_q8_serve_report, rama_q8_serve_row, rama_q8_serve_slot,
                   rama_q8_serve_spec, rama_q8_serve_spec_report)
from .q8_replay import SERVE_DECODE, SERVE_DONE, SERVE_FREE, SERVE_PROMPT
from .sampler_const import TOPP_U_CPU

SERVE_CANCELLED = 2      # RAMA_SERVE_CANCELLED: the finished word of a slot ended by a cancel


def serve_sizes(cfg, n_slots, max_rows, max_new_cap, who="Q8Server"):
    """the checked sizes of a serving chain; ValueError for what rama_q8_serve_begin would refuse as a bad size.  No library call."""
    n_slots, max_new_cap = int(n_slots), int(max_new_cap)
    max_rows = n_slots if max_rows is None else int(max_rows)
    if not 1 <= n_slots <= MAX_BATCH:
        raise ValueError(f"{who}: {n_slots} slots, not 1..{MAX_BATCH}")
    if not n_slots <= max_rows <= MAX_BATCH:
        raise ValueError(f"{who}: max_rows {max_rows} outside [n_slots = {n_slots}, {MAX_BATCH}]")
    if not 1 <= max_new_cap <= cfg.seq_len - 1:
        raise ValueError(f"{who}: max_new_cap {max_new_cap} outside [1, seq_len - 1 = {cfg.seq_len - 1}]")
    return n_slots, max_rows, max_new_cap


def serve_plan(cfg, context, max_new, temperature=0.0, topp=0.9, u=TOPP_U_CPU, stop_token=None, max_new_cap=None, n_cached=0, who="Q8Server"):
    """the checked arguments of Q8Server.submit: (context tokens, (temperature, topp, u, max_new, stop token)); ValueError for
    everything rama_q8_serve_admit / rama_q8_serve_admit_at would refuse in them.  No library call."""
    what = who + ".submit"
    V, S = cfg.vocab_size, cfg.seq_len
    ctx = _check_context(what, context, V)
    if not 0 <= int(n_cached) <= len(ctx) - 1:
        raise ValueError(f"{what}: n_cached {int(n_cached)} outside [0, n_context - 1 = {len(ctx) - 1}] (the final context position is always fed)")
    T, P, U = _check_sampler(what, temperature, topp, u)
    new = int(max_new)
    _check_budget(what, len(ctx), new, S, max_new_cap)
    stop = _check_stop(what, stop_token, V)
    _check_sampled_vocab(what, T, V)
    return ctx, (T, P, U, new, stop)


def serve_plan_step(slots, max_rows):
    """rama_q8_serve_plan_step, the scheduling rule as a pure host function: slots = (state, n_context, cursor, n_out, max_new)
    tuples -> (rows [(slot, pos, logits)] * max_rows, the slots after the step when no stop token is sampled).  No GPU."""
    n, table, max_rows = len(slots), _slot_table(slots), int(max_rows)
    rows = (rama_q8_serve_row * max(max_rows, 1))()
    after = (rama_q8_serve_slot * max(n, 1))()
    check(load().rama_q8_serve_plan_step(table, n, max_rows, rows, after), "rama_q8_serve_plan_step")
    return _row_table(rows, max_rows), [(a.state, a.n_context, a.cursor, a.n_out, a.max_new) for a in after[:n]]


def common_prefix(a, b) -> int:
    """the number of leading tokens two sequences share"""
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


def serve_spec_sizes(n_draft, ngram, hint_cap, who="Q8Server"):
    """the checked drafting sizes of a Q8Server (or, `who`, a Server); ValueError for what rama_q8_serve_begin_spec would refuse.
    No library call."""
    n_draft, ngram, hint_cap = int(n_draft), int(ngram), int(hint_cap)
    _check_drafting(who, n_draft, ngram)
    if hint_cap < 0 or (hint_cap and not n_draft):
        raise ValueError(f"{who}: hint_cap {hint_cap} (>= 0, and 0 on a server without drafts)")
    return n_draft, ngram, hint_cap


def serve_spec_request(cfg, n_draft_cap, ngram, hint_cap, n_draft=None, hint=None, who="Q8Server"):
    """the checked drafting arguments of Q8Server.submit: (n_draft, ngram, hint tokens); ValueError for everything
    rama_q8_serve_admit_spec would refuse in them.  No library call."""
    what = who + ".submit"
    K = n_draft_cap if n_draft is None else int(n_draft)
    _check_n_draft(what, K, n_draft_cap, f"the server's n_draft = {n_draft_cap}")
    toks = [] if hint is None else _tokens(hint, cfg.vocab_size, what + " hint")
    if len(toks) > hint_cap:
        raise ValueError(f"{what}: {len(toks)} hint tokens beyond the server's hint_cap {hint_cap}")
    return K, ngram, toks


def serve_spec_report(r) -> dict:
    """a rama_q8_serve_spec_report as a dict: its counters and caps, and the last step's drafts of its n_slots slots"""
    d = _report(r, skip=("n_slots", "max_rows"))
    d["last_want"], d["last_granted"] = d["last_want"][:r.n_slots], d["last_granted"][:r.n_slots]
    return d


def serve_spec_plan_step(slots, want, max_rows):
    """rama_q8_serve_spec_plan_step, the scheduling rule with drafts as a pure host function: slots = (state, n_context, cursor,
    n_out, max_new) tuples, want = the drafts every slot has for the step -> (rows [(slot, pos, logits)] * max_rows, the drafts
    granted per slot).  No GPU."""
    n = len(slots)
    if len(want) != n:
        raise ValueError(f"serve_spec_plan_step: {len(want)} want values for {n} slots")
    table, warr, max_rows = _slot_table(slots), _i32([int(v) for v in want]), int(max_rows)
    rows = (rama_q8_serve_row * max(max_rows, 1))()
    granted = (C.c_int32 * max(n, 1))()
    check(load().rama_q8_serve_spec_plan_step(table, n, max_rows, warr, rows, granted), "rama_q8_serve_spec_plan_step")
    return _row_table(rows, max_rows), granted[:n]


def serve_model_sizes(cfg, draft, n_slots, n_draft, hint_cap, who="Q8Server"):
    """ValueError for what rama_q8_serve_begin_model would refuse in a draft model and can be seen from here.  No library call."""
    if hint_cap:
        raise ValueError(f"{who}: hint_cap {hint_cap} together with a draft model -- model drafts replace the lookup")
    if not 1 <= int(n_draft) <= 15:
        raise ValueError(f"{who}: n_draft {n_draft} outside 1..15 with a draft model")
    if draft.cfg.vocab_size != cfg.vocab_size:
        raise ValueError(f"{who}: the draft model's vocabulary {draft.cfg.vocab_size} is not the target's {cfg.vocab_size}")
    if 2 * int(n_slots) > MAX_BATCH:
        raise ValueError(f"{who}: {n_slots} slots with a draft model, not 1..{MAX_BATCH // 2} (the first draft pass carries two rows per slot)")


def serve_model_plan_step(slots, n_draft, draft_cursor, max_rows, seq_len, n_passes):
    """rama_q8_serve_model_plan_step, the step's schedule of a chain with a draft model as a pure host function: slots = (state,
    n_context, cursor, n_out, max_new) tuples, n_draft and draft_cursor per slot -> (rows [(slot, pos, logits)] * max_rows, want,
    granted, the draft passes' row tables: [2 n_slots rows] then n_passes - 1 times [n_slots rows]).  No GPU."""
    n = len(slots)
    if len(n_draft) != n or len(draft_cursor) != n:
        raise ValueError(f"serve_model_plan_step: {len(n_draft)} n_draft and {len(draft_cursor)} draft_cursor values for {n} slots")
    table, max_rows, n_passes = _slot_table(slots), int(max_rows), int(n_passes)
    rows = (rama_q8_serve_row * max(max_rows, 1))()
    want, granted = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    drows = (rama_q8_serve_row * (max(n_passes + 1, 2) * max(n, 1)))()
    check(load().rama_q8_serve_model_plan_step(table, n, max_rows, int(seq_len), _i32([int(v) for v in n_draft]), _i32([int(v) for v in draft_cursor]),
                                               n_passes, rows, want, granted, drows), "rama_q8_serve_model_plan_step")
    flat = [(r.slot, r.pos, r.logits) for r in drows[:(n_passes + 1) * n]]
    passes = [flat[:2 * n]] + [flat[(j + 1) * n:(j + 2) * n] for j in range(1, n_passes)]
    return _row_table(rows, max_rows), want[:n], granted[:n], passes


def serve_model_report(r) -> dict:
    """a rama_q8_serve_model_report as a dict: its counters, and the draft cursors of its n_slots slots"""
    d = _report(r, skip=("n_slots",))
    d["draft_cursor"] = d["draft_cursor"][:r.n_slots]
    return d


class PrefixPool:
    """the donors of a server's prefix cache: at most k engines, each keyed by the tokens whose cache rows it holds (row t is a
    function of tokens 0..t only, and its bits do not depend on who computed it).  Least recently used goes first.  Pure host
    logic: an engine is any object, compared by identity.  While an engine is here it is a donor and nothing else."""

    def __init__(self, k: int):
        self.k = int(k)
        if self.k < 0:
            raise ValueError(f"PrefixPool: {self.k} donors")
        self._donors = []                                 # [tokens, engine], least recently used first

    def __len__(self):
        return len(self._donors)

    def __contains__(self, engine):
        return any(d[1] is engine for d in self._donors)

    def engines(self):
        return [d[1] for d in self._donors]

    def match(self, context, at_least: int = 1):
        """-> (engine, n): the donor that shares the longest token prefix with `context`, n capped at len(context) - 1 (the final
        context position is always fed: its logits are needed); (None, 0) when no donor shares at_least tokens.  Of equally
        long matches the most recently used wins.  The donor found becomes the most recently used."""
        best, best_n = None, 0
        for d in self._donors:                            # (later = more recently used: >= lets it win a tie)
            n = min(common_prefix(d[0], context), len(context) - 1)
            if n >= max(at_least, 1) and n >= best_n:
                best, best_n = d, n
        if best is None:
            return None, 0
        self._donors.remove(best)
        self._donors.append(best)
        return best[1], best_n

    def put(self, tokens, engine):
        """`engine` holds the rows of `tokens` and becomes the most recently used donor -> the engines that left the pool for
        it (none while there is room; the engine itself when k == 0)"""
        if engine in self:
            raise ValueError("PrefixPool.put: the engine is already a donor")
        if self.k == 0:
            return [engine]
        self._donors.append([list(tokens), engine])
        out = []
        while len(self._donors) > self.k:
            out.append(self._donors.pop(0)[1])
        return out

    def clear(self):
        out, self._donors = self.engines(), []
        return out


class ServeLoop:
    """A serving chain's host loop, whatever the model: the queue, the slots' engines, the mirror of the device's slot table kept by the
    host plan (rama_q8_serve_plan_step), the steps to the next finish, admissions behind the steps in flight, the host-visible rings --
    and what both chains offer on request: prompt caching (submit(n_cached=), the donor pool of prefix_cache=k, the fork --
    rama_q8_kv_fork: the KV cache is fp32 in both stacks -- and <ABI>_admit_at) and drafts (<ABI>_begin_spec / _admit_spec / _spec_stats
    and the run loop of a chain whose steps the host cannot foresee), and ending a request from outside: cancel /
    cancelled, submit(priority=), preempt=True -- a waiting request that outranks a running one takes its slot, and the request that
    left continues later on its engine over its own rows with the tokens of an uninterrupted run -- and suspend / resume.  Q8Server
    (rama_q8_serve_*) and rama_amd.Server (rama_serve_*, parity mode) are this loop over their entries' family: a subclass states ABI,
    NAME and the engine a slot gets (_new_engine)."""

    ABI = None         # the C entries' family: <ABI>_begin / _admit / _steps / _poll / _stats / _end
    NAME = "ServeLoop"
    LOOKAHEAD = 2      # steps enqueued past a foreseen finish while requests wait: the admission then goes in behind running steps
    SPEC_BLOCK = 4     # with drafts: at most this many steps between two looks at the device's slot table
    PREEMPT_BLOCK = 4  # with preempt: at most this many steps enqueued at once, so that a cancel lands no further behind an urgent arrival
    MIN_CACHED = 2     # a shorter match is not worth a launch: every context shares its first token (BOS) with every donor

    def __init__(self, model, n_slots, max_rows, max_new_cap, prefix_cache, n_draft, ngram, hint_cap, draft=None, preempt=False):
        """the sizes (every one checked before any library call, in this order), the chain's begin, the loop's books"""
        self.preempt = bool(preempt)                      # a waiting request that outranks a running one takes its slot
        self.n_slots, self.max_rows, self.max_new_cap = serve_sizes(model.cfg, n_slots, max_rows, max_new_cap, self.NAME)
        self.n_draft, self.ngram, self.hint_cap = serve_spec_sizes(n_draft, ngram, hint_cap, self.NAME)
        self.draft = draft                                # a Q8 draft model: <ABI>_begin_model / _admit_model
        if draft is not None:
            serve_model_sizes(model.cfg, draft, self.n_slots, self.n_draft, self.hint_cap, self.NAME)
        self._down = [None] * self.n_slots                # the server's draft engine of a slot, made on first use and reused
        self.spec = self.n_draft > 0                      # n_draft == 0: the plain chain, <ABI>_begin
        self.pool = PrefixPool(prefix_cache)              # (raises before any library call)
        self.model, self.device, self.cfg = model, model.device, model.cfg
        self._begin()
        L = self.device.lib
        self._open = True
        self._own = [None] * self.n_slots                 # the server's own engine of a slot, made on first use and reused
        self._eng = [None] * self.n_slots                 # the engine the slot's occupant runs on
        self._spare = []                                  # the server's own engines that serve nobody
        self._mine = []                                   # every engine the server made (close frees them)
        self._req = [None] * self.n_slots                 # the handle a slot serves
        self._seen = [0] * self.n_slots
        self._poll = [_ring_poll(getattr(L, self.ABI + "_poll"), self.ABI + "_poll", self.device.ctx, slot, after=(None,)) for slot in range(self.n_slots)]
        self._mirror = [(SERVE_FREE, 0, 0, 0, 0)] * self.n_slots     # the host's copy of the slot table (exact unless a stop token fell)
        self._queue, self._results, self._finished, self._plans = [], {}, set(), {}
        self._next = 0
        self._cached = {}                                 # handle -> the n_cached it was admitted with
        self._drafts = {}                                 # handle -> (n_draft, ngram, hint tokens)
        self.rows_cached = 0                              # ... summed over the admissions
        self._prio = {}                                   # handle -> priority (the queue: highest first, FIFO within one)
        self._serial = [0] * self.n_slots                 # admissions a slot has seen: tells an occupant from its successor
        self._admitted = {}                               # handle -> the count of admissions at its (last) own: the victim among equals is the latest
        self._n_admitted = 0
        self._off = [0] * self.n_slots                    # tokens the occupant had produced before this admission (a continuation's on_token indices run on)
        self._ending = {}                                 # handle of a running request with a cancel enqueued -> "cancel" / "preempt" / "suspend" / "resume"
        self._cancelled = set()                           # handles ended by cancel()
        self._suspended = set()                           # handles whose continuation waits for resume()
        self.preemptions = 0
        self.planned = dict(steps=0, rows_decode=0, rows_prompt=0, rows_idle=0)      # the host plan's sums over the steps enqueued (none with drafts: no host plan)
        self.last_rows = []                               # ... and its row table of the last one

    def _call(self, name, *args):
        entry = f"{self.ABI}_{name}"
        check(getattr(self.device.lib, entry)(self.device.ctx, *args), entry)

    def _begin(self):
        m = self.model
        sizes = (C.byref(m.ccfg), C.byref(m.weights), self.n_slots, self.max_rows, self.max_new_cap)
        if self.draft is not None:
            d = self.draft
            self._call("begin_model", C.byref(m.ccfg), C.byref(m.weights), C.byref(d.ccfg), C.byref(d.weights), self.n_slots, self.max_rows,
                       self.max_new_cap, self.n_draft)
        elif self.spec:
            self._call("begin_spec", *sizes, self.n_draft, self.hint_cap)
        else:
            self._call("begin", *sizes)

    def _new_engine(self, model=None):
        """an engine over the server's model, or -- a server with a draft model -- over `model`"""
        raise NotImplementedError

    # -- requests
    def submit(self, context, max_new, temperature=0.0, topp=0.9, u=TOPP_U_CPU, stop_token=None, engine=None, n_cached=0,
               retain=False, n_draft=None, hint=None, priority=0):
        """queue a request -> its handle.  It is admitted at once if a slot is free, else when one finishes (step / run).
        engine: the engine whose run state the sequence uses (default: one the server owns for the slot).
        n_cached: rows 0..n_cached-1 of `engine` already hold context[0..n_cached) -- written by work enqueued earlier on the
        device's stream; the slot feeds the rest (at most n_context - 1: the final position is always fed).  Such a request is
        not matched against the prefix cache.
        retain: with a prefix cache, the engine stays behind as a donor when the request finishes (a caller's engine too: it
        is the pool's until it is evicted).
        n_draft, hint: on a server made with n_draft > 0, the drafts per step of this request (default: the server's; 0: none)
        and a token list to look up in besides the request's own text (at most hint_cap tokens).  The tokens are the same
        whatever they are.
        priority: the queue serves the highest first, FIFO within one; on a server made with preempt=True a waiting request that
        outranks a running one takes its slot (the lowest priority, among equals the most recently admitted, is cancelled and
        continues later on its engine with the tokens of an uninterrupted run)."""
        ctx, plan = serve_plan(self.cfg, context, max_new, temperature, topp, u, stop_token, self.max_new_cap, n_cached, self.NAME)
        draft = serve_spec_request(self.cfg, self.n_draft, self.ngram, self.hint_cap, n_draft, hint, self.NAME)
        if self.draft is not None and len(ctx) + plan[3] > self.draft.cfg.seq_len:
            raise ValueError(f"{self.NAME}.submit: n_context {len(ctx)} + max_new {plan[3]} beyond the draft model's seq_len {self.draft.cfg.seq_len}")
        n_cached, priority = int(n_cached), int(priority)
        if n_cached and engine is None:
            raise ValueError(f"{self.NAME}.submit: n_cached needs the engine that holds the rows")
        if engine is not None and engine.model is not self.model:
            raise ValueError(f"{self.NAME}.submit: the engine belongs to another {type(self.model).__name__}")
        if engine is not None and any(e is engine for e in self._engines_in_use()):
            raise ValueError(f"{self.NAME}.submit: the engine already serves a queued or running request")
        if engine is not None and engine in self.pool:
            raise ValueError(f"{self.NAME}.submit: the engine is a donor of the prefix cache")
        h = self._next
        self._next += 1
        self._plans[h] = (ctx, plan, engine, n_cached, bool(retain))
        self._results[h] = []
        self._drafts[h] = draft
        self._prio[h] = priority
        self._enqueue(h)
        self._admit()
        return h

    def _enqueue(self, h, front=False):
        """into the queue behind every request of its priority or a higher one (front: before its equals -- a continuation was
        there before them)"""
        p, k = self._prio[h], 0
        while k < len(self._queue) and (self._prio[self._queue[k]] > p or (not front and self._prio[self._queue[k]] == p)):
            k += 1
        self._queue.insert(k, h)

    def _engines_in_use(self):
        waiting = [self._plans[h][2] for h in list(self._queue) + sorted(self._suspended)]
        running = [self._eng[i] for i, h in enumerate(self._req) if h is not None]
        return [e for e in waiting + running if e is not None]

    def _admit(self):
        """queued requests go into free slots: a match in the prefix cache is forked into the request's engine, then the admission"""
        L, ctx = self.device.lib, self.device.ctx
        for slot in range(self.n_slots):
            if not self._queue:
                break
            if self._req[slot] is not None:
                continue
            h = self._queue[0]                             # (it leaves the queue once the library has taken it)
            toks, (T, P, U, new, stop), eng, n_cached, _ = self._plans[h]
            if eng is None:
                if self._own[slot] is None:
                    if not self._spare:                    # (an engine the server makes is its own to free, and spare until a slot has it)
                        self._spare.append(self._new_engine())
                        self._mine.append(self._spare[-1])
                    self._own[slot] = self._spare.pop()
                eng = self._own[slot]
            if not n_cached and len(self.pool):
                # the donor stays in the pool whatever happens below: donors leave it in _collect only, so a fork that was
                # enqueued and an admission that then failed find it there at the next attempt; an evicted donor is reused or
                # freed behind the fork in stream order
                donor, n_cached = self.pool.match(toks, self.MIN_CACHED)
                if n_cached:
                    check(L.rama_q8_kv_fork(ctx, C.byref(self.model.ccfg), C.byref(donor.state), C.byref(eng.state), 1, n_cached),
                          "rama_q8_kv_fork")
            arr, rec = _i32(toks), rama_q8_serve_plan(T, P, U, new, stop)
            if self.draft is not None:
                # the draft model's rows of the whole context: a prefill enqueued before the admission, stream-ordered between two steps (the
                # chain's begin sized every buffer it runs on, and the captured step holds none that it could regrow)
                if self._down[slot] is None:
                    self._down[slot] = self._new_engine(self.draft)
                    self._mine.append(self._down[slot])
                self._down[slot].prefill(toks)
                self._call("admit_model", slot, C.byref(eng.state), C.byref(self._down[slot].state), arr, len(toks), n_cached, C.byref(rec),
                           self._drafts[h][0])
            elif self.spec:
                K, N, hint = self._drafts[h]
                harr = _i32(hint)
                srec = rama_q8_serve_spec(K, N, harr if hint else None, len(hint))
                self._call("admit_spec", slot, C.byref(eng.state), arr, len(toks), n_cached, C.byref(rec), C.byref(srec))
            elif n_cached:
                self._call("admit_at", slot, C.byref(eng.state), arr, len(toks), n_cached, C.byref(rec))
            else:
                self._call("admit", slot, C.byref(eng.state), arr, len(toks), C.byref(rec))
            self._queue.pop(0)
            self._req[slot], self._seen[slot], self._eng[slot] = h, 0, eng
            self._off[slot] = len(self._results[h])
            self._serial[slot] += 1
            self._n_admitted += 1
            self._admitted[h] = self._n_admitted
            self._cached[h] = n_cached
            self.rows_cached += n_cached
            self._mirror[slot] = (SERVE_PROMPT, len(toks), n_cached, 0, new)
        if self.preempt:
            self._preempt()

    # -- ending a request from outside
    def _slot_of(self, handle):
        for slot, h in enumerate(self._req):
            if h == handle:
                return slot
        return None

    def _end_running(self, slot, why):
        """<ABI>_cancel behind the steps enqueued -- where the host's mirror stands --, and the slot DONE in the mirror"""
        self._call("cancel", _i32([slot]), 1)
        self._ending[self._req[slot]] = why
        self._mirror[slot] = (SERVE_DONE,) + tuple(self._mirror[slot][1:])

    def _preempt(self):
        """while no slot is free and a waiting request outranks a running one: the running request of the lowest priority, among
        equals the most recently admitted, is cancelled.  The k-th cancel under way serves the k-th request of the queue.  A
        preemption may turn out needless: if another slot finishes by itself before the victim's word shows, the urgent request
        takes that slot, and the victim is still requeued as a continuation (and counted) -- exact, one row fed again."""
        while all(h is not None for h in self._req):
            under_way = sum(1 for why in self._ending.values() if why == "preempt")
            if under_way >= len(self._queue):
                return
            running = [h for h in self._req if h not in self._ending]
            if not running:
                return
            victim = min(running, key=lambda h: (self._prio[h], -self._admitted[h]))
            if self._prio[victim] >= self._prio[self._queue[under_way]]:
                return
            self._end_running(self._slot_of(victim), "preempt")

    def _known(self, what, handle):
        if handle not in self._plans:
            raise ValueError(f"{self.NAME}.{what}: no request {handle!r}")

    def _leave(self, h):
        """a request that waits (queued or suspended) ends here: an engine of the server's that stayed with it is spare again"""
        eng = self._plans[h][2]
        if eng is not None and any(eng is m for m in self._mine) and not any(eng is o for o in self._own):
            self._spare.append(eng)
        self._finished.add(h)
        self._cancelled.add(h)

    def cancel(self, handle):
        """end request `handle` now.  Queued (or suspended): it leaves the queue.  Running: <ABI>_cancel, stream-ordered behind the
        steps enqueued; the tokens drained until its finished word shows are its result, and cancelled(handle) says whether the
        cancel ended it -- a request that finishes by itself first is not cancelled.  Finished already: nothing.  May be called
        from an on_token callback inside run()."""
        self._known("cancel", handle)
        if handle in self._finished:
            return
        if handle in self._queue or handle in self._suspended:
            if handle in self._queue:
                self._queue.remove(handle)
            self._suspended.discard(handle)
            self._leave(handle)
        elif handle in self._ending:
            self._ending[handle] = "cancel"
        else:
            self._end_running(self._slot_of(handle), "cancel")

    def cancelled(self, handle) -> bool:
        """request `handle` was ended by cancel() (False while it runs, and for one that finished by itself)"""
        self._known("cancelled", handle)
        return handle in self._cancelled

    def suspend(self, handle):
        """the first half of a preemption, for callers who schedule themselves: a running request is cancelled and, once its
        finished word shows, waits -- with its engine -- as a continuation until resume(handle); a queued one leaves the queue
        and waits the same way.  One that finishes by itself first has simply finished."""
        self._known("suspend", handle)
        if handle in self._finished or handle in self._suspended or self._ending.get(handle) in ("cancel", "suspend"):
            raise ValueError(f"{self.NAME}.suspend: request {handle!r} has finished, is being cancelled or is suspended already")
        if handle in self._queue:
            self._queue.remove(handle)
            self._suspended.add(handle)
        elif handle in self._ending:
            self._ending[handle] = "suspend"
        else:
            self._end_running(self._slot_of(handle), "suspend")

    def resume(self, handle):
        """the second half: the continuation of a suspended request goes back into the queue, before its equals"""
        self._known("resume", handle)
        if handle in self._suspended:
            self._suspended.discard(handle)
            self._enqueue(handle, front=True)
            self._admit()
        elif self._ending.get(handle) == "suspend":
            self._ending[handle] = "resume"                # (its finished word has not shown yet: queued when it does)
        else:
            raise ValueError(f"{self.NAME}.resume: request {handle!r} is not suspended")

    def _continuation(self, slot, h, produced):
        """the request a cancel ended in `slot` as one that can be admitted again on its engine: the context plus the tokens
        it produced since its admission, n_cached = the slot's cursor (every row below it is the uninterrupted run's; the final
        position is always fed), the budget that is left; sampler, stop token and drafts as they were"""
        toks, (T, P, U, new, stop), _, _, retain = self._plans[h]
        cursor = self.stats()["slots"][slot][2]            # (synchronises: once per preemption)
        toks = toks + produced
        self._plans[h] = (toks, (T, P, U, new - len(produced), stop), self._eng[slot], min(cursor, len(toks) - 1), retain)

    def cached(self, handle) -> int:
        """the n_cached request `handle` was admitted with (None while it waits)"""
        return self._cached.get(handle)

    def _collect(self, on_token=None):
        """what the rings hold: new tokens of every occupied slot; a finished occupant frees its slot and leaves its engine -- with
        retain and a prefix cache the engine becomes a donor, keyed by the tokens whose rows it holds (the context and every output
        but the last); whoever leaves the pool for it serves requests again if the server made it.  A finished word of
        RAMA_SERVE_CANCELLED: the request ends as cancelled, or -- preempted or suspended -- becomes a continuation that keeps its
        engine; a request that finished by itself before the cancel ran has simply finished."""
        early = False
        for slot in range(self.n_slots):
            h = self._req[slot]
            if h is None:
                continue
            got, off, word = self._results[h], self._off[slot], [0]

            def sink(index, token):
                if on_token is not None:
                    on_token(h, off + index, token)
                got.append(token)

            def poll(start):
                toks, word[0] = self._poll[slot](start)
                return toks, word[0]
            n, fin = _drain(poll, self._seen[slot], sink)
            self._seen[slot] += n
            if not fin:
                continue
            why = self._ending.pop(h, None)
            if word[0] != SERVE_CANCELLED:
                why = None                                 # (it finished by itself, whatever was enqueued behind)
            elif why is None:
                why = "cancel"                             # (a cancel past this loop, through the entry itself)
            early = early or self._mirror[slot][0] != SERVE_DONE
            self._mirror[slot] = (SERVE_DONE,) + tuple(self._mirror[slot][1:])
            eng = self._eng[slot]
            if why in ("preempt", "suspend", "resume"):
                self._continuation(slot, h, got[off:])
                if self._own[slot] is eng:                 # (the engine stays with the handle; the slot gets another from the spares)
                    self._own[slot] = None
                self._req[slot], self._eng[slot] = None, None
                if why == "suspend":
                    self._suspended.add(h)
                else:
                    self.preemptions += why == "preempt"
                    self._enqueue(h, front=True)
                continue
            self._finished.add(h)
            if why == "cancel":
                self._cancelled.add(h)
            self._req[slot], self._eng[slot] = None, None
            if self._plans[h][4] and self.pool.k:          # retain
                if self._own[slot] is eng:
                    self._own[slot] = None
                held = self._plans[h][0] + got[off:][:-1]
                if why == "cancel" and len(got) == off:    # cancelled inside its context: the rows below the cursor
                    held = self._plans[h][0][:self.stats()["slots"][slot][2]]
                for e in self.pool.put(held, eng):
                    if any(e is m for m in self._mine):
                        self._spare.append(e)
            elif any(eng is m for m in self._mine) and self._own[slot] is not eng:
                self._spare.append(eng)                    # (a continuation's engine: no slot's own any more)
        return early

    def step(self, n: int = 1, on_token=None):
        """collect what has arrived, admit queued requests into free slots, then enqueue n steps (asynchronous)"""
        if self._collect(on_token):
            self._resync()
        self._admit()
        self._count_and_enqueue(int(n))

    def _count_and_enqueue(self, n):
        if not self.spec:                                  # (with drafts the rows of a step depend on what is accepted: no host plan)
            for _ in range(n):
                before = self._mirror
                rows, self._mirror = serve_plan_step(before, self.max_rows)
                self.last_rows = rows
                dec = sum(1 for s, _, _ in rows if s >= 0 and before[s][0] == SERVE_DECODE)
                used = sum(1 for s, _, _ in rows if s >= 0)
                self.planned["steps"] += 1
                self.planned["rows_decode"] += dec
                self.planned["rows_prompt"] += used - dec
                self.planned["rows_idle"] += self.max_rows - used
        if n:
            self._call("steps", n)

    def _resync(self):
        """a stop token ended a sequence before its budget: the host's copy of the slot table is taken from the device again"""
        st = self.stats()
        self._mirror = [s if self._req[i] is not None or s[0] in (SERVE_FREE, SERVE_DONE) else (SERVE_DONE,) + s[1:] for i, s in enumerate(st["slots"])]

    def _steps_to_next_finish(self):
        """by the host plan: the steps until a slot finishes (requests waiting) or until all have (none waiting)"""
        m, k = list(self._mirror), 0
        live = lambda t: [s[0] in (SERVE_PROMPT, SERVE_DECODE) for s in t]
        start = live(m)
        while any(live(m)):
            _, m = serve_plan_step(m, self.max_rows)
            k += 1
            if self._queue and live(m) != start:
                break
        return k

    def run(self, on_token=None):
        """serve every submitted request to its end.  on_token(handle, index, token), when given, is fed from the host-visible
        rings.  The steps up to the next finish the host plan foresees -- and, while requests wait, LOOKAHEAD more, so that the
        device does not idle until the host has seen the finished word and admitted -- are enqueued at once; a DONE slot takes
        no rows, and an admission is stream-ordered behind them, so the host plan stays exact.  A stop token that ends a sequence
        earlier is seen at the next collection.  With drafts the host plan foresees nothing: _run_drafting."""
        if self.spec:
            return self._run_drafting(on_token)
        done_in = lambda t: {i for i in range(self.n_slots) if self._req[i] is not None and t[i][0] == SERVE_DONE}
        while True:
            if self._collect(on_token):
                self._resync()
            self._admit()
            expect = done_in(self._mirror)                # finished by the plan, not yet seen
            k = self._steps_to_next_finish()
            cut = self.preempt and k > self.PREEMPT_BLOCK  # (the block is run to its end before the next look)
            k = min(k, self.PREEMPT_BLOCK) if cut else k
            if k == 0 and not expect:
                if self._queue:
                    raise RuntimeError(f"{self.NAME}.run: requests are waiting but no slot can take them")
                return
            if k:
                after = self._after(k)
                expect |= done_in(after)
                live_on = any(s[0] in (SERVE_PROMPT, SERVE_DECODE) for s in after)
                self._count_and_enqueue(k + (self.LOOKAHEAD if self._queue and live_on and not cut else 0))
            serial = {i: self._serial[i] for i in expect}
            still = lambda: [i for i in expect if self._req[i] is not None and self._serial[i] == serial[i]]     # (not its successor, admitted from a callback)
            while True:                       # until the slots the plan -- or a cancel -- ends here have set their finished words
                if self._collect(on_token):
                    self._resync()
                if not still() and not cut:
                    break
                if _stream_busy(self.device, 0.0001):
                    continue
                self._collect(on_token)
                if still():
                    raise RuntimeError(f"{self.NAME}.run: the steps have run but slots {still()} have not finished")
                break

    def _after(self, k):
        m = list(self._mirror)
        for _ in range(k):
            _, m = serve_plan_step(m, self.max_rows)
        return m

    def _run_drafting(self, on_token=None):
        """run() on a server with drafts.  A slot may finish earlier than the host plan foresees, so the plan -- one token per
        DECODE slot and step -- is an upper bound: the slot table is taken from the device before every block, the steps to the
        next finish by that plan -- SPEC_BLOCK at most -- are enqueued, and the finished words alone say who has finished.  A request that waits is
        admitted as soon as a finished word shows, behind the steps still in flight; the device never idles past a finish by
        more than the block enqueued."""
        while True:
            self._resync()                                # (synchronises: the block before has run)
            self._collect(on_token)
            self._admit()
            if all(h is None for h in self._req):
                if self._queue:
                    raise RuntimeError(f"{self.NAME}.run: requests are waiting but no slot can take them")
                return
            self._count_and_enqueue(max(min(self._steps_to_next_finish(), self.SPEC_BLOCK), 1))
            while True:
                self._collect(on_token)
                self._admit()
                if not _stream_busy(self.device, 0.0001):
                    break

    def finished(self, handle) -> bool:
        return handle in self._finished

    def poll(self, on_token=None):
        """collect what the rings hold now (never touches the stream); on_token(handle, index, token) for every new token"""
        if self._collect(on_token):
            self._resync()

    def result(self, handle):
        """the tokens of request `handle` collected so far by run / step / poll (all of them once finished(handle))"""
        return list(self._results[handle])

    def stats(self):
        """<ABI>_stats (synchronises): the device's counters, the slot table, the last step's row table; rows_cached is the
        host's sum of n_cached over the admissions (context positions taken from cached rows instead of being fed); with drafts,
        spec = <ABI>_spec_stats"""
        r = rama_q8_serve_report()
        self._call("stats", C.byref(r))
        out = dict(steps=int(r.steps), graph_captures=int(r.graph_captures), rows_decode=int(r.rows_decode), rows_prompt=int(r.rows_prompt),
                   rows_idle=int(r.rows_idle), n_slots=int(r.n_slots), max_rows=int(r.max_rows),
                   last_rows=_row_table(r.last_rows, r.max_rows),
                   slots=[(s.state, s.n_context, s.cursor, s.n_out, s.max_new) for s in r.slots[:r.n_slots]],
                   generation=[int(g) for g in r.generation[:r.n_slots]], rows_cached=self.rows_cached, preemptions=self.preemptions)
        if self.spec:
            q = rama_q8_serve_spec_report()
            self._call("spec_stats", C.byref(q))
            out["spec"] = serve_spec_report(q)
        if self.draft is not None:
            q = rama_q8_serve_model_report()
            self._call("model_stats", C.byref(q))
            out["model"] = serve_model_report(q)
        return out

    def close(self):
        if self._open:
            self._open = False
            self._call("end")
            self.pool.clear()                             # (a caller's engine that was a donor is the caller's again)
            for e in self._mine:
                e.free()
            self._mine, self._spare = [], []
            self._own, self._eng, self._down = [None] * self.n_slots, [None] * self.n_slots, [None] * self.n_slots
