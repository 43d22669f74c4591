"""Long texts for the n-gram drafting kernels (data and rules only; no test, no library, no GPU): spec_draft_kernel (one workgroup
of 1024 threads) and serve_draft_kernel (256 threads per slot) scan a hint and the sequence's own text with a stride loop, keep a
running maximum of `hint bit | end` and reduce it over their waves.  tests/test_q8_spec_long_host.py checks the rule and the cases
on the CPU; tests/test_hip_q8_spec_long.py and tests/test_hip_q8_serve_spec_long.py run them on the GPU.

The rule, restated by brute force (`draft`): for n = min(ngram, L) down to 1, every exclusive end e of an occurrence of the text's
last n tokens -- in the hint (n <= e <= n_hint) first, then in the sequence (n <= e <= L - 1: the tail itself does not count) --
and the latest e wins; the draft is the min(n_draft, room, text length - e) tokens behind it, and an occurrence with nothing behind
it still decides (no fall-through).  End e belongs to thread (e - n) % threads in sweep (e - n) // threads.

The mutants, the wrong rules a broken kernel would implement (`MUTANTS`): earliest (the earliest occurrence), seq_first (the
sequence before the hint: the hint bit lost), shortest_first (n ascending), hint_any_n (the hint at every n before the sequence at
any), first_sweep (ends of sweep >= 1 dropped), wave0 (threads >= 64 dropped), last_wave (threads >= threads - 64 dropped),
hint_end (a hint occurrence ending at n_hint dropped), tail_self (the sequence's end e == L admitted).

A case plants the tail n-gram into filler that holds none of the tail's tokens, at chosen (sweep, thread) slots, at least n + 15
tokens apart, with chosen follow tokens.  The choice of occurrence shows in the counters either model-free -- n_d differs: nothing
found, or an occurrence 0, 1 or 3 tokens before its text's end -- or through the model: behind the right occurrence stands the
sequence's true continuation, behind every decoy 15 tokens whose first is not the next true token, so a step accepts 15 drafts under
the right rule and none under a wrong one.  `lead` is the number of reference tokens the text holds when the first draft is made: 0
for the one-stream chain, 1 for the serving chain, whose admission step emits a token without drafting -- there the tail n-gram
ends with that token.

    case     placement (s = sweep, t = thread)                                         kill list
    H-wave   hint: right at s0 t(threads-1), decoy at s0 t5                            earliest, wave0, last_wave
    H-next   hint: right at s0 t64, decoy at s0 t20                                    earliest, wave0
    H-sweep  hint: right at s1 t3, decoy at s0 t(threads-40)                           earliest, first_sweep
    H-third  hint: the only occurrence at s2 t70                                       wave0, first_sweep
    H-first  hint of threads + 50 tokens that begins with the tail (e = n)             (none: against the true rule only)
    H-end    hint: occurrence ending at n_hint (s1 t30); the context holds one         hint_end, seq_first
             with 15 tokens behind it: n_d = 0, no fall-through
    H-cut    hint: right at n_hint - 3 (s1 t10), decoy at s0 t12: n_d = 3              earliest, first_sweep
    S-wave   H-wave's placement in the context (threads + 100 tokens), no hint         earliest, wave0, last_wave, tail_self
    S-sweep  H-sweep's placement in the context (threads + 100 tokens)                 earliest, first_sweep, tail_self
    S-third  H-third's placement in the context (2 threads + 100 tokens)               wave0, first_sweep, tail_self
    S-last   the context (2 threads + 100 tokens) ends x^(n+1), decoy x^n at s0 t9:    tail_self, earliest, first_sweep
             the occurrence ending at L - 1 gives n_d = 1
    P-hint   hint: right at s0 t7; context: decoy ending at 2000                       seq_first
    P-long   ngram 4: the 4-gram only in the context, ending at 2000; the hint holds   hint_any_n, shortest_first
             the tail's last 3 tokens behind another token, 3 tokens before its end
    P-fall   ngram 4: no 4-, 3- or 2-gram anywhere; the 1-gram only in the hint,       first_sweep, wave0
             at s2 t70

Occurrences planted in the CONTEXT with the true continuation behind them (S-wave, S-sweep, S-third, P-long) need a context that
holds what the model will say behind it: `settle` builds the context from a guess (the context's last token repeated, which is what
these synthetic models' greedy runs do), asks for the real run, rebuilds from it and stops when the run no longer changes.  A case
that does not settle, or that is not discriminating -- some mutant of its kill list replays to the true rule's trajectory --, is
tried with the next seed; `settle` raises when no seed serves."""
from collections import namedtuple

import numpy as np

MUTANTS = ("earliest", "seq_first", "shortest_first", "hint_any_n", "first_sweep", "wave0", "last_wave", "hint_end", "tail_self")
N_DRAFT, N_SEEDS = 15, 24

KILLS = {
    "H-wave": ("earliest", "wave0", "last_wave"),
    "H-next": ("earliest", "wave0"),
    "H-sweep": ("earliest", "first_sweep"),
    "H-third": ("wave0", "first_sweep"),
    "H-first": (),
    "H-end": ("hint_end", "seq_first"),
    "H-cut": ("earliest", "first_sweep"),
    "S-wave": ("earliest", "wave0", "last_wave", "tail_self"),
    "S-sweep": ("earliest", "first_sweep", "tail_self"),
    "S-third": ("wave0", "first_sweep", "tail_self"),
    "S-last": ("tail_self", "earliest", "first_sweep"),
    "P-hint": ("seq_first",),
    "P-long": ("hint_any_n", "shortest_first"),
    "P-fall": ("first_sweep", "wave0"),
}

Case = namedtuple("Case", "name n ngram threads lead context hint n_draft kill")


# ------------------------------------------------------------------ the rule and its mutants

def occurrence_ends(text, tail, lo_hi, threads, mutant=None, in_hint=False):
    """every exclusive end e in lo_hi[0]..lo_hi[1] with text[e - n:e] == tail that the (mutant) rule sees"""
    n = len(tail)
    out = []
    for e in range(max(lo_hi[0], n), lo_hi[1] + 1):
        if text[e - 1] != tail[-1] or text[e - n:e] != tail:
            continue
        k = e - n
        if mutant == "first_sweep" and k // threads >= 1:
            continue
        if mutant == "wave0" and k % threads >= 64:
            continue
        if mutant == "last_wave" and k % threads >= threads - 64:
            continue
        if mutant == "hint_end" and in_hint and e == len(text):
            continue
        out.append(e)
    return out


def draft(hint, seq, n_draft, ngram, room, threads, mutant=None):
    """the drafted tokens under the rule, or under one of MUTANTS"""
    assert mutant is None or mutant in MUTANTS, mutant
    hint, seq = list(hint or []), list(seq)
    cap = min(n_draft, room)
    if cap <= 0:
        return []
    L = len(seq)
    ns = list(range(min(ngram, L), 0, -1))
    if mutant == "shortest_first":
        ns.reverse()
    texts = [(hint, len(hint), True), (seq, L if mutant == "tail_self" else L - 1, False)]
    if mutant == "seq_first":
        texts.reverse()
    if mutant == "hint_any_n":
        order = [(n, t) for t in texts for n in ns]
    else:
        order = [(n, t) for n in ns for t in texts]
    for n, (text, hi, in_hint) in order:
        ends = occurrence_ends(text, seq[L - n:], (n, hi), threads, mutant, in_hint)
        if ends:
            e = min(ends) if mutant == "earliest" else max(ends)
            return text[e:e + cap]
    return []


def replay(ref, context, hint, n_draft, ngram, max_new, threads, mutant=None, stop=None, lead=0):
    """the steps of a chain whose picks are the reference run's: one (n_d, a, emitted) per step up to the finish.  lead = 1: the
    first step is an admission step, one token and no draft (the serving chain over a cached context)."""
    ref, s = list(ref), list(context)
    assert len(ref) >= max_new
    stop = -1 if stop is None else stop
    out, e, fin = [], 0, False
    while not fin:
        remaining = max_new - e
        d = [] if len(out) < lead else draft(hint, s, n_draft, ngram, remaining - 1, threads, mutant)
        picks = ref[e:e + len(d) + 1]
        a = 0
        while a < len(d) and picks[a] == d[a]:
            a += 1
        emit = min(a + 1, remaining)
        fin = emit >= remaining
        for j in range(emit):
            if picks[j] == stop:
                emit, fin = j + 1, True
                break
        s += picks[:emit]
        e += emit
        out.append((len(d), a, emit))
    return out


def undiscriminated(case, ref, max_new):
    """the mutants of the case's kill list whose trajectory equals the true rule's: [] for a discriminating case"""
    true = replay(ref, case.context, case.hint, case.n_draft, case.ngram, max_new, case.threads, None, None, case.lead)
    return [m for m in case.kill
            if replay(ref, case.context, case.hint, case.n_draft, case.ngram, max_new, case.threads, m, None, case.lead) == true]


# ------------------------------------------------------------------ the builder

def slot_end(n, threads, sweep, tid):
    """the exclusive end that thread tid visits in its sweep-th iteration"""
    return n + sweep * threads + tid


def _plant(text, e, gram, follow):
    n = len(gram)
    assert e - n >= 0 and e + len(follow) <= len(text), (e, n, len(follow), len(text))
    text[e - n:e] = gram
    text[e:e + len(follow)] = follow


def build(name, n, ngram, threads, seed, ref, lead, max_new=24, vocab=512):
    """the case `name` whose planted n-gram has n tokens, for a chain of `threads` drafting threads.  ref = the reference run the
    case is built for (None: a guess, the context's last token repeated)."""
    assert name in KILLS and 1 <= n <= ngram <= 4 and lead in (0, 1)
    rng = np.random.default_rng([seed, n, ngram, threads, sorted(KILLS).index(name)])
    T, K = threads, N_DRAFT
    periodic = name == "S-last"
    # the context's end: ngram - lead distinct tokens (one at the least), x^(n + 1 - lead) for S-last
    n_end = max(n + 1 - lead if periodic else ngram - lead, 1)
    picks = [int(t) for t in rng.choice(np.arange(2, vocab), size=n_end + 1, replace=False)]
    ctx_end = [picks[0]] * n_end if periodic else picks[:n_end]
    other = picks[n_end]                                            # a token that is in no tail
    if ref is None:
        ref = [ctx_end[-1]] * max_new
    ref = list(ref)
    tail = (ctx_end + ref[:lead])[-ngram:]                          # the text's last ngram tokens when the first draft is made
    gram = tail[-n:]
    cont = ref[lead:lead + K]                                       # what the model says behind the tail
    avoid = set(tail) | set(ctx_end) | {cont[0], other}
    allowed = np.array([t for t in range(2, vocab) if t not in avoid])

    def filler(k):
        return [int(t) for t in rng.choice(allowed, size=k)]

    def context(n_ctx, plants=()):
        c = [1] + filler(n_ctx - 1)
        for e, g, follow in plants:
            assert e - len(g) >= 1 and e + len(follow) <= n_ctx - n_end, (name, e, n_ctx)
            _plant(c, e, g, follow)
        c[n_ctx - n_end:] = ctx_end
        return c

    def hint_text(n_hint, plants):
        h = filler(n_hint)
        for e, g, follow in plants:
            _plant(h, e, g, follow)
        return h

    end = lambda s, t: slot_end(n, T, s, t)
    short = 12
    hint = []
    if name in ("H-wave", "H-next", "H-sweep", "S-wave", "S-sweep"):
        right, decoy = {"wave": ((0, T - 1), (0, 5)), "next": ((0, 64), (0, 20)), "sweep": ((1, 3), (0, T - 40))}[name[2:]]
        plants = [(end(*decoy), gram, filler(K)), (end(*right), gram, cont)]
        assert end(*right) - end(*decoy) >= n + K
        if name[0] == "H":
            ctx, hint = context(short), hint_text(end(*right) + K + 20, plants)
        else:
            ctx = context(T + 100, plants)
    elif name in ("H-third", "S-third", "P-fall"):
        plants = [(end(2, 70), gram, cont)]
        if name == "S-third":
            ctx = context(2 * T + 100, plants)
        else:
            ctx, hint = context(short), hint_text(end(2, 70) + K + 20, plants)
    elif name == "H-first":
        ctx, hint = context(short), hint_text(T + 50, [(n, gram, cont)])
    elif name == "H-end":
        ctx = context(60, [(end(0, 9), gram, filler(K))])
        hint = hint_text(end(1, 30), [(end(1, 30), gram, [])])
    elif name == "H-cut":
        ctx = context(short)
        hint = hint_text(end(1, 10) + 3, [(end(0, 12), gram, filler(K)), (end(1, 10), gram, cont[:3])])
    elif name == "S-last":
        ctx = context(2 * T + 100, [(end(0, 9), gram, filler(K))])
    elif name == "P-hint":
        ctx = context(2040, [(2000, gram, filler(K))])
        hint = hint_text(60, [(end(0, 7), gram, cont)])
    elif name == "P-long":
        assert n == ngram == 4
        ctx = context(2040, [(2000, gram, cont)])
        hint = hint_text(80, [(77, [other] + gram[1:], [])])
    else:
        raise AssertionError(name)
    return Case(name, n, ngram, T, lead, ctx, hint, K, KILLS[name])


def settle(name, n, ngram, threads, lead, max_new, solo, vocab=512, n_seeds=N_SEEDS):
    """the first seed whose case is consistent -- built for the run the model really makes behind its context: solo(context) ->
    the max_new reference tokens -- and discriminating -> (case, ref).  AssertionError when no seed serves."""
    why = []
    for seed in range(n_seeds):
        ref = None
        for _ in range(4):
            case = build(name, n, ngram, threads, seed, ref, lead, max_new, vocab)
            real = list(solo(case.context))
            if real == ref:
                break
            ref = real
        else:
            why.append((seed, "the run behind the context does not settle"))
            continue
        bad = undiscriminated(case, ref, max_new)
        if not bad:
            return case, ref
        why.append((seed, "not killed: " + ", ".join(bad)))
    raise AssertionError(f"{name} n={n} ngram={ngram} threads={threads}: no seed below {n_seeds} serves: {why[:6]}")


#        name       (n, ngram) pairs; ngram 4 at least once per group
TABLE = [
    ("H-wave", [(1, 1), (3, 3), (4, 4)]),
    ("H-next", [(2, 4), (4, 4)]),
    ("H-sweep", [(1, 2), (2, 2), (4, 4)]),
    ("H-third", [(3, 3), (1, 4)]),
    ("H-first", [(2, 2), (4, 4)]),
    ("H-end", [(2, 2), (4, 4)]),
    ("H-cut", [(2, 2), (3, 4)]),
    ("S-wave", [(2, 2), (4, 4)]),
    ("S-sweep", [(2, 3), (3, 3)]),
    ("S-third", [(2, 2), (4, 4)]),
    ("S-last", [(1, 1), (4, 4)]),
    ("P-hint", [(2, 2), (4, 4)]),
    ("P-long", [(4, 4)]),
    ("P-fall", [(1, 4)]),
]
ALL = [(name, n, ngram) for name, pairs in TABLE for n, ngram in pairs]
# the cases the serving chain runs (threads 256).  Its tail ends with the context's last token and the first emitted one; a greedy run
# of these models repeats its last token, so an n-gram of two equal tokens would occur all through the true continuation: the cases that
# observe through the model plant n >= 3 tokens
SERVE = [("H-wave", 3, 3), ("H-next", 3, 4), ("H-sweep", 4, 4), ("H-third", 1, 4), ("H-end", 2, 2), ("H-cut", 3, 4), ("S-sweep", 3, 3),
         ("S-last", 1, 1), ("P-hint", 3, 3), ("P-long", 4, 4), ("P-fall", 1, 4)]


def case_id(c):
    return f"{c[0]}-n{c[1]}of{c[2]}"
