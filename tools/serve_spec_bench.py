#!/usr/bin/env python3
"""Drafts in idle rows and cached prefixes on the parity-mode serving chain (rama_amd.Server(n_draft=, prefix_cache=)) against
the plain fp32 serving chain, on a llama2-7B-shaped rama_model_synth model (seq_len 256 so that the run states fit), "ref_order" = 1, graph
mode on.

Workload (fixed seed, tools/serve_bench.py's request mix, i.e. tools/q8_serve_bench.py's): --requests requests, context lengths uniform in
16..128 tokens, budgets uniform in 16..96 new tokens, greedy, no stop tokens -- every variant produces the same tokens and the same number
of them.  For n_slots in 16 and 32 and max_rows in 32 and 64:
 (plain)  the plain chain, Server(n_draft=0).  With --parent-tree PATH (a checkout of the parent commit, built) it is ALSO run from that
          tree's library in a fresh child process in the same session: `parent_tok_s`, and every ratio below is against it.  Without it the
          ratios are against this build's plain chain, and the line says so (`against`).
 (a)      the spec chain with n_draft = 0 on every request (server n_draft 7): the price of the two extra launches, the guard launch and of
          classifying whole tiles where they sit instead of n_slots gathered rows -- `over_plain`.
 (b)      drafts on (n_draft 7, ngram 3), three variants: each request's solo output as its hint (the upper bound: every granted draft
          accepted), hints corrupted (every 5th token replaced) so that drafts are rejected, and no hint.
 (c)      a shared-prefix workload -- --prefixes system prompts of --prefix-len tokens, every request one of them plus a tail of 8..32 tokens,
          budgets 16..48 -- with the prefix cache off (Server()) and on (Server(prefix_cache=--prefixes); the first request of each
          prefix stays behind as its donor; the timed runs find the donors the untimed run left: a warm cache): `over_cache_off`.
Every configuration is run once untimed, then --reps times (wall clock around a drained stream, admissions included); a line carries the
median and the spread.  The tokens of every variant are compared with the plain chain's (the cache-off run's): they must be equal.  Prints
ONE JSON line per configuration and variant and, with --out, appends each to that file as it is measured.  No threshold is fixed: both
features stay opt-in whatever the numbers are.

Usage:  python tools/serve_spec_bench.py [--reps 3] [--requests 96] [--slots 16,32] [--rows 32,64] [--layers 32] [--prefixes 4]
                                         [--prefix-len 96] [--parent-tree PATH] [--out profiles/serve_spec_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve()
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--requests", type=int, default=96)
ap.add_argument("--slots", type=str, default="16,32")
ap.add_argument("--rows", type=str, default="32,64")
ap.add_argument("--layers", type=int, default=32, help="fewer layers: a rehearsal")
ap.add_argument("--prefixes", type=int, default=4)
ap.add_argument("--prefix-len", type=int, default=96)
ap.add_argument("--out", type=str, default="")
ap.add_argument("--parent-tree", type=str, default="", help="a built checkout of the parent commit: its plain chain is timed in a child process")
ap.add_argument("--tree", type=str, default="", help="(the child's) import rama_amd from this tree and time the plain chain only")
args = ap.parse_args()
REPO = Path(args.tree).resolve() if args.tree else HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

import numpy as np  # noqa: E402

import rama_amd  # noqa: E402
from bench import library_stamp  # noqa: E402
from oracle.oracle import Config  # noqa: E402
from q8_serve_bench import CTX_RANGE, DIM, HIDDEN, NEW_RANGE, SEQ, VOCAB, workload  # noqa: E402
from rama_amd._lib import check  # noqa: E402
from tests.helpers import to_rama_cfg  # noqa: E402

N_DRAFT, NGRAM = 7, 3
TAIL_RANGE, PREFIX_NEW_RANGE = (8, 32), (16, 48)        # inclusive


def corrupt(toks):
    """every 5th token replaced by a different one"""
    return [(t + 1) % VOCAB if i % 5 == 4 else t for i, t in enumerate(toks)]


def prefix_workload(n, n_prefixes, prefix_len, seed=1):
    """-> [(context, max_new, the index of its prefix)]: request i takes prefix i % n_prefixes"""
    rng = np.random.default_rng(seed)
    heads = [[1] + [int(t) for t in rng.integers(2, VOCAB, prefix_len - 1)] for _ in range(n_prefixes)]
    out = []
    for i in range(n):
        tail = int(rng.integers(TAIL_RANGE[0], TAIL_RANGE[1] + 1))
        new = int(rng.integers(PREFIX_NEW_RANGE[0], PREFIX_NEW_RANGE[1] + 1))
        out.append((heads[i % n_prefixes] + [int(t) for t in rng.integers(2, VOCAB, tail)], new, i % n_prefixes))
    return out


def main():
    reqs = workload(args.requests)
    total_new = sum(new for _, new in reqs)
    shared = prefix_workload(args.requests, args.prefixes, args.prefix_len)
    assert args.prefix_len + TAIL_RANGE[1] + PREFIX_NEW_RANGE[1] <= SEQ
    shared_new = sum(new for _, new, _ in shared)
    dev = rama_amd.Hip(0)
    L, ctx = dev.lib, dev.ctx
    check(L.rama_set_tuning(ctx, b"ref_order", 1))
    name, cus, _ = dev.info()
    m = rama_amd.Model.synth(dev, to_rama_cfg(Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, False)), 7)
    check(L.rama_set_graph_mode(ctx, 1))

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out and not args.tree:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    def timed(fn):
        fn()                                             # untimed: code objects, scratch, copies, the graph capture (and, (c), the donors)
        ts = []
        for _ in range(args.reps):
            check(L.rama_sync(ctx))
            t0 = time.perf_counter()
            fn()
            check(L.rama_sync(ctx))
            ts.append(time.perf_counter() - t0)
        return ts

    def spread(ts, toks):
        med = statistics.median(ts)
        return dict(wall_s=round(med, 4), wall_s_min=round(min(ts), 4), wall_s_max=round(max(ts), 4), reps=len(ts),
                    tok_s=round(toks / med, 1), tok_s_min=round(toks / max(ts), 1), tok_s_max=round(toks / min(ts), 1))

    def run(n, max_rows, n_draft, hints, drafts):
        """one server per configuration (its slots are reused run after run) -> (times, tokens, the device's counters over one run)"""
        got = {}
        srv = rama_amd.Server(m, n, max_rows, NEW_RANGE[1], **(dict(n_draft=n_draft, ngram=NGRAM, hint_cap=SEQ) if n_draft else {}))

        def serve():
            before = srv.stats()
            hs = [srv.submit(c, new, **(dict(n_draft=drafts, hint=hints[i] if hints else None) if n_draft else {})) for i, (c, new) in enumerate(reqs)]
            srv.run()
            got["out"] = [srv.result(h) for h in hs]
            after = srv.stats()
            got["stats"] = {k: after[k] - before[k] for k in ("steps", "rows_decode", "rows_prompt", "rows_idle")}
            got["stats"]["graph_captures"] = after["graph_captures"]
            if n_draft:
                got["stats"].update({k: after["spec"][k] - before["spec"][k] for k in ("rows_draft", "drafts_wanted", "drafts_granted", "drafts_accepted")})
        try:
            ts = timed(serve)
        finally:
            srv.close()
        return ts, got["out"], got["stats"]

    def run_shared(n, max_rows, k):
        got = {}
        srv = rama_amd.Server(m, n, max_rows, PREFIX_NEW_RANGE[1], **(dict(prefix_cache=k) if k else {}))

        def serve():
            before = srv.stats()
            seen = set()
            hs = []
            for c, new, p in shared:
                hs.append(srv.submit(c, new, **(dict(retain=p not in seen) if k else {})))
                seen.add(p)
            srv.run()
            got["out"] = [srv.result(h) for h in hs]
            after = srv.stats()
            got["stats"] = {key: after[key] - before[key] for key in ("steps", "rows_decode", "rows_prompt", "rows_idle") + (("rows_cached",) if k else ())}
        try:
            ts = timed(serve)
        finally:
            srv.close()
        return ts, got["out"], got["stats"]

    parent = {}
    if args.parent_tree:                                 # the same session, a fresh process, the parent's own library and Python
        cmd = [sys.executable, str(HERE), "--tree", args.parent_tree, "--reps", str(args.reps), "--requests", str(args.requests),
               "--slots", args.slots, "--rows", args.rows, "--layers", str(args.layers)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ))
        if r.returncode != 0:
            raise RuntimeError(f"the parent's run failed:\n{r.stdout}\n{r.stderr}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                d = json.loads(ln)
                parent[(d["n_slots"], d["max_rows"])] = d

    try:
        for n in [int(s) for s in args.slots.split(",")]:
            for max_rows in [int(s) for s in args.rows.split(",")]:
                if max_rows < n:
                    continue
                base = dict(device=name, compute_units=cus, library=library_stamp(), mode="parity", n_layers=args.layers, n_slots=n,
                            max_rows=max_rows, requests=len(reqs), context_range=list(CTX_RANGE), max_new_range=list(NEW_RANGE),
                            generated_tokens=total_new, graph_mode=True, unit="tok/s")
                ts, plain_out, st = run(n, max_rows, 0, None, 0)
                line = dict(base, metric=f"serve_plain_{n}_rows{max_rows}", variant="plain", **spread(ts, total_new), **st)
                line["value"] = plain_tok_s = line["tok_s"]
                p = parent.get((n, max_rows))
                if p:
                    line.update(parent_tok_s=p["tok_s"], parent_tok_s_min=p["tok_s_min"], parent_tok_s_max=p["tok_s_max"], parent_library=p["library"],
                                over_parent=round(line["tok_s"] / p["tok_s"], 4))
                emit(line)
                if args.tree:
                    continue
                ref = p["tok_s"] if p else plain_tok_s
                against = "parent build" if p else "this build's plain chain"
                texts = [c + o for (c, _), o in zip(reqs, plain_out)]
                for variant, hints, drafts in (("spec_n_draft_0", None, 0), ("hint_own", texts, N_DRAFT), ("hint_corrupt", [corrupt(t) for t in texts], N_DRAFT),
                                               ("hint_none", None, N_DRAFT)):
                    ts, out, st = run(n, max_rows, N_DRAFT, hints, drafts)
                    line = dict(base, metric=f"serve_spec_{variant}_{n}_rows{max_rows}", variant=variant, n_draft=drafts, ngram=NGRAM,
                                **spread(ts, total_new), **st, same_tokens=out == plain_out)
                    line["value"] = line["tok_s"]
                    line["over_plain"] = round(line["tok_s"] / ref, 4)
                    line["against"] = against
                    emit(line)
                # (c) shared prefixes: the cache off, then on
                sbase = dict(base, requests=len(shared), generated_tokens=shared_new, prefixes=args.prefixes, prefix_len=args.prefix_len,
                             context_range=[args.prefix_len + TAIL_RANGE[0], args.prefix_len + TAIL_RANGE[1]], max_new_range=list(PREFIX_NEW_RANGE))
                ts, off_out, st = run_shared(n, max_rows, 0)
                line = dict(sbase, metric=f"serve_prefix_off_{n}_rows{max_rows}", variant="prefix_cache_off", **spread(ts, shared_new), **st)
                line["value"] = off_tok_s = line["tok_s"]
                emit(line)
                ts, out, st = run_shared(n, max_rows, args.prefixes)
                line = dict(sbase, metric=f"serve_prefix_on_{n}_rows{max_rows}", variant="prefix_cache_on", prefix_cache=args.prefixes,
                            **spread(ts, shared_new), **st, same_tokens=out == off_out)
                line["value"] = line["tok_s"]
                line["over_cache_off"] = round(line["tok_s"] / off_tok_s, 4)
                emit(line)
    finally:
        m.free()
        check(L.rama_set_graph_mode(ctx, 0))
        check(L.rama_set_tuning(ctx, b"ref_order", 0))
    dev.close()


if __name__ == "__main__":
    main()
