"""The workloads of the fp32 serving chain's prompt-caching and drafting tests, as data: tests/test_serve_spec_host.py asserts with the pure-Python
replay, over the CPU oracle's tokens, that each reaches what it is there for; tests/test_hip_serve_spec.py runs them on the GPU.  A workload is a
list of Case objects; what a request does alone (`solo`: its max_new tokens, not cut at the stop token) comes from whoever builds it -- the
oracle on the host, a twin engine in parity mode on the GPU: the same tokens."""
import numpy as np

from tests.serve_cases import TILE, TINY  # noqa: F401

SEED = 23                      # the synthetic weights' seed (tests/test_hip_serve.py's)
HINT_CAP = 160
SIX = {"grant cut", "all accepted", "first rejected", "budget ends in an accepted run", "stop among the accepted drafts", "finish next to an ingestion"}


def corrupt(toks, V):
    """every fifth token wrong"""
    return [t if i % 5 != 4 else (t + 1) % V for i, t in enumerate(toks)]


class Case:
    """a request: context (BOS first), plan, drafting fields; hint = "own" | "corrupt" | "wrong" | None | a token list, resolved from the solo run"""

    def __init__(self, rng, V, n_ctx, max_new, T=0.0, topp=0.9, u=0.0, stop=-1, K=0, N=3, hint=None, periodic=0):
        self.V = V
        self.ctx = [1] + [int(t) for t in rng.integers(2, V, n_ctx - 1)]
        if periodic:                                              # BOS, then a pattern of `periodic` tokens over and over
            self.ctx = [1] + [self.ctx[1 + (i % periodic)] for i in range(n_ctx - 1)]
        self.max_new, self.T, self.topp, self.u, self.stop = max_new, T, topp, u, stop
        self.K, self.N, self.kind, self.hint, self.n_cached = K, N, hint, [], 0
        self.solo = None

    def resolve(self, solo):
        """solo = the max_new tokens of this request alone -> self, its hint made"""
        self.solo = [int(t) for t in solo]
        assert len(self.solo) == self.max_new
        if self.kind == "own":                                    # the text the sequence will have: every granted draft is right
            self.hint = self.ctx + self.solo
        elif self.kind == "corrupt":
            self.hint = corrupt(self.ctx + self.solo, self.V)
        elif self.kind == "wrong":                                # behind every token of the solo run one that the run never has
            z = next(t for t in range(self.V) if t not in self.solo and t not in self.ctx)
            self.hint = [t for x in self.solo for t in (x, z)]
        else:
            self.hint = list(self.kind or [])
        assert len(self.hint) <= HINT_CAP
        return self

    def want(self):
        out = []
        for t in self.solo:
            out.append(t)
            if t == self.stop:
                break
        return out

    def spec(self):
        return dict(context=self.ctx, max_new=self.max_new, stop_token=None if self.stop < 0 else self.stop, n_draft=self.K, ngram=self.N,
                    hint=self.hint, n_cached=self.n_cached)


PLANS = [(0.0, 0.9, 0.0), (1.0, 0.9, 0.21), (0.7, 1.0, 0.55), (0.0, 0.9, 0.0), (1.0, 0.9, 0.8)]


def mixed(solo, V, seed=3):
    """six requests for 4 slots at max_rows 8, built from their own solo runs so that the six outcomes are certain: c stops on its third token,
    which its second step reaches inside an accepted run; a is always right and ends on its budget; b's first draft is always wrong; e never
    drafts and ends while d -- admitted into c's slot, a context longer than max_rows -- is still ingesting; f's hint is corrupted"""
    rng = np.random.default_rng(seed)
    for _ in range(12):                                           # c's first three tokens must differ: its stop token is the third
        c = Case(rng, V, 3, 8, 1.0, 0.9, 0.37, K=7, N=3, hint="own")
        c.resolve(solo(c))
        if c.solo[2] not in c.solo[:2]:
            break
    else:
        raise AssertionError("no context whose first three tokens differ")
    c.stop = c.solo[2]
    rest = [Case(rng, V, 4, 12, 1.0, 0.9, 0.77, K=7, N=3, hint="own"), Case(rng, V, 2, 9, 0.7, 1.0, 0.3, K=3, N=1, hint="wrong"),
            Case(rng, V, 1, 5, K=0), Case(rng, V, 21, 2, K=2, N=2), Case(rng, V, 2, 6, 1.0, 0.9, 0.6, K=7, N=2, hint="corrupt")]
    return dict(n_slots=4, max_rows=8, cases=[c] + [r.resolve(solo(r)) for r in rest])


def hints(solo, V, kind, seed=17):
    """five requests, greedy and sampled, whose hints are all right ("own"), corrupted ("corrupt": every fifth token wrong) or absent (None: the
    lookup finds the periodic context); run at 4 slots x 8, 16 and 40 rows and around a FREE hole"""
    rng = np.random.default_rng(seed)
    cases = [Case(rng, V, n_ctx, new, *PLANS[i], K=K, N=N, hint=kind, periodic=0 if kind else 3)
             for i, (n_ctx, new, K, N) in enumerate([(13, 14, 7, 3), (4, 10, 15, 2), (10, 9, 3, 3), (7, 16, 7, 4), (2, 6, 5, 2)])]
    return dict(n_slots=4, cases=[r.resolve(solo(r)) for r in cases])


LAYOUTS = [(8, None), (16, None), (40, None), (16, [0, 2, 3])]      # max_rows, the slots in use (None: all four)


def straddle(solo, V, seed=29):
    """4 slots x 40 rows, every hint right: once all four decode, slot 0 takes 16 rows, slot 1 13 and slot 2's token and drafts lie on both sides
    of row 32; towards the end at most 32 rows are wanted and tile 1 is wholly idle"""
    rng = np.random.default_rng(seed)
    cases = [Case(rng, V, 2, 34, 1.0, 0.9, 0.15, K=15, N=3, hint="own"), Case(rng, V, 3, 30, 0.7, 1.0, 0.62, K=12, N=3, hint="own"),
             Case(rng, V, 2, 30, 1.0, 0.95, 0.4, K=7, N=3, hint="own"), Case(rng, V, 1, 5, K=0)]
    return dict(n_slots=4, max_rows=40, cases=[r.resolve(solo(r)) for r in cases])


def guard(solo, V, seed=37):
    """2 slots x 40 rows, no drafts: step 0 gives slot 0 its 30 context rows (the final one carries logits, in tile 0) and slot 1 rows 30..39
    inside its context -- tile 1 is live and carries no logits; step 1 puts slot 1's final context row at row 36, in tile 1"""
    rng = np.random.default_rng(seed)
    cases = [Case(rng, V, 30, 3, 1.0, 0.9, 0.3), Case(rng, V, 46, 3, 0.7, 1.0, 0.8)]
    return dict(n_slots=2, max_rows=40, cases=[r.resolve(solo(r)) for r in cases])


def outcomes(trace):
    """which of the six outcomes a run shows: trace = per step (slots before, slots after, want, granted)"""
    PROMPT, DECODE, DONE = 1, 2, 3
    seen = set()
    for before, after, want, granted in trace:
        ingesting = [i for i, b in enumerate(before) if b[0] == PROMPT and after[i][0] == PROMPT]
        for i, (b, a) in enumerate(zip(before, after)):
            if b[0] != DECODE:
                continue
            emitted, fin = a[3] - b[3], a[0] == DONE
            if granted[i] < want[i]:
                seen.add("grant cut")
            if granted[i] > 0 and emitted == granted[i] + 1:
                seen.add("all accepted")
            if granted[i] > 0 and emitted == 1 and not fin:
                seen.add("first rejected")
            if fin and emitted > 1 and a[3] == a[4]:
                seen.add("budget ends in an accepted run")
            if fin and emitted > 1 and a[3] < a[4]:
                seen.add("stop among the accepted drafts")
            if fin and ingesting:
                seen.add("finish next to an ingestion")
    return seen


def replay_trace(rp, n_slots):
    """serve_spec_replay's steps as outcomes() wants them"""
    before, trace = [(0, 0, 0, 0, 0)] * n_slots, []
    for st in rp["steps"]:
        before = list(before)
        for slot, q in st["admitted"]:
            s = st["slots"][slot]
            before[slot] = (1, s[1], None, 0, s[4])
        trace.append((before, st["slots"], st["want"], st["granted"]))
        before = st["slots"]
    return trace
