#!/usr/bin/env python3
"""Tree drafts (rama_q8_spec_begin_tree) against the linear speculative chain (rama_q8_spec_begin) on a
llama2-7B-shaped rama_q8_model_synth model (group size 64, a classifier of its own so that a greedy run does not repeat its
input), greedy, graph mode on, in one process.  Nothing here fixes a threshold: the lines are the measurement.

Behind a fixed-seed random context the model produces --new tokens alone, and the tool times
 (a) the step: the tree chain at 16 rows (n_branch 2) against the linear chain at n_draft 15, both with the solo output as hint so
     that every row is live.  The difference is the price of the tree attention plus the commit;
 (b) tok/s with the solo output followed by a copy with every fifth token wrong as hint: the tree chain with n_branch 1, 2 and 3
     (n_draft 7, 16 rows) against the linear chain (n_draft 7);
 (c) the same without a hint.
With --parent-build the library loaded is the parent commit's (RAMA_HIP_LIB names it): the linear legs alone, metric
q8_spec_tree_parent_*; the ratios against them are what the README quotes.  Every leg is run once untimed, then --reps times, wall
clock around a drained device, begin subtracted; the spread is reported.  The chain's tokens are checked against the solo run's
before anything is timed.  Prints ONE JSON line per leg and, with --out, appends each to that file as it is measured.

Usage:  RAMA_HIP_LIB=<the parent's librama_hip.so> python tools/q8_spec_tree_bench.py --parent-build --out profiles/q8_spec_tree_bench.jsonl
        python tools/q8_spec_tree_bench.py [--reps 3] [--new 48] [--position 9] [--layers 32] --out profiles/q8_spec_tree_bench.jsonl
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

DIM, HIDDEN, VOCAB, SEQ = 4096, 11008, 32000, 2048
NEW_SYMBOLS = ("rama_q8_spec_begin_tree", "rama_q8_spec_tree_stats", "rama_q8_spec_tree_draft", "rama_q8_spec_tree_accept",
               "rama_q8_tree_forward", "rama_q8_tree_commit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--new", type=int, default=48, help="tokens produced per run")
    ap.add_argument("--position", type=int, default=9, help="context length: the first produced token's position")
    ap.add_argument("--layers", type=int, default=32, help="fewer layers: a rehearsal")
    ap.add_argument("--parent-build", action="store_true", help="the library loaded is the parent commit's: the linear legs only")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from rama_amd import _lib
    if args.parent_build:
        for s in NEW_SYMBOLS:                            # (the parent's library does not export them, and its legs do not call them)
            _lib.SIGNATURES.pop(s, None)

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    import rama_amd
    from bench import library_stamp
    from oracle.oracle import Config
    from rama_amd._lib import check
    from rama_amd.q8_replay import spec_replay, spec_tree_replay
    dev = rama_amd.Hip(0)
    L, ctx = dev.lib, dev.ctx
    name, cus, _ = dev.info()
    who = "parent" if args.parent_build else "this"
    base = dict(device=name, compute_units=cus, group_size=64, library=library_stamp(), n_layers=args.layers, graph_mode=True,
                parent_build=bool(args.parent_build), new_tokens=args.new, position=args.position)
    m = rama_amd.Q8Model.synth(dev, Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, False), 64, 7)
    eng = rama_amd.Q8Engine(dev, m)
    eng.set_graph_mode(True)
    rng = np.random.default_rng(0)
    n_ctx, new = args.position, args.new

    def timed(run):
        run()                                            # untimed: captures, first touches
        ts = []
        for _ in range(args.reps):
            check(L.rama_sync(ctx))
            t0 = time.perf_counter()
            run()
            check(L.rama_sync(ctx))
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    try:
        context = [1] + [int(t) for t in rng.integers(2, VOCAB, n_ctx - 1)]
        want = eng.generate(context[1:], n_ctx - 1 + new)[n_ctx - 1:]
        copy = [(t + 1) % VOCAB if i % 5 == 4 else t for i, t in enumerate(want)]
        carr = (C.c_int32 * n_ctx)(*context)
        head = (ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state), carr, n_ctx)
        legs = [("a_step", 15, want, [(2, 16)]), ("b_fifth_wrong", 7, want + copy, [(1, 16), (2, 16), (3, 16)]), ("c_no_hint", 7, None, [(2, 16)])]
        for leg, K, hint, trees in legs:
            harr = (C.c_int32 * max(len(hint or []), 1))(*(hint or []))
            plan = _lib.rama_q8_spec_plan(0.0, 0.9, 0.0, new, -1, K, 3, harr if hint else None, len(hint or []))
            runs = [("linear", None, len(spec_replay(want, context, hint, K, 3, new, None)))]
            if not args.parent_build:
                runs += [(f"tree_b{B}", (B, R), len(spec_tree_replay(want, context, hint, K, 3, B, R, new, None))) for B, R in trees]
            for kind, tree, n_steps in runs:
                got = eng.generate_spec(context, new, n_draft=K, ngram=3, hint=hint, **(dict(n_branch=tree[0], tree_rows=tree[1]) if tree else {}))
                if got != want or eng.spec_stats["steps"] < n_steps:
                    raise SystemExit(f"{leg} {kind}: the chain's tokens are not the solo run's")
                stats = dict(eng.spec_stats)

                def begin():
                    if tree:
                        check(L.rama_q8_spec_begin_tree(*head, C.byref(plan), tree[0], tree[1]))
                    else:
                        check(L.rama_q8_spec_begin(*head, C.byref(plan)))

                def run():
                    begin()
                    check(L.rama_q8_spec_steps(ctx, n_steps))
                t_begin = timed(begin)[0]
                med, lo, hi = timed(run)
                line = dict(base, metric=f"q8_spec_tree_{who}_{leg}_{kind}", chain=kind, n_draft=K, hint_tokens=len(hint or []), steps=n_steps,
                            n_branch=tree[0] if tree else None, n_rows=tree[1] if tree else K + 1,
                            tok_s=round(new / (med - t_begin), 1), ms_per_step=round((med - t_begin) * 1e3 / n_steps, 4),
                            spread_ms_per_step=[round((lo - t_begin) * 1e3 / n_steps, 4), round((hi - t_begin) * 1e3 / n_steps, 4)],
                            accepted=stats["accepted"], off_trunk_accepted=stats.get("off_trunk_accepted"))
                emit(line)
                check(L.rama_q8_spec_end(ctx))
    finally:
        eng.set_graph_mode(False)
        eng.free(); m.free()
        dev.close()


if __name__ == "__main__":
    main()
