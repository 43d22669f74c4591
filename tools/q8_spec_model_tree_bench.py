#!/usr/bin/env python3
"""Trees from a draft model (rama_q8_spec_begin_model_tree) against the linear chain with a draft model
(rama_q8_spec_begin_model; 8.9): a llama2-7B-shaped rama_q8_model_synth target (group size 64, a classifier of its own) and a
stories15M-shaped synthetic draft over the same vocabulary, greedy, graph mode on, in one process.  Nothing here fixes a threshold
and nothing here is a speed claim: two synthetic models accept nothing, so the lines are THE STEP WITH NOTHING ACCEPTED.

For K in 2, 4, 7 the tool times a run of --new steps (each emits one token) of
  tree_b<B>   the tree chain, B in 1, 2, 3 at 16 rows                                   metric q8_spec_model_tree_this_k<K>_b<B>
  linear      rama_q8_spec_begin_model at the same K, with --parent-build alone           metric q8_spec_model_tree_parent_k<K>_linear
With --parent-build the library loaded is the parent commit's (RAMA_HIP_LIB names it).  When --out already holds the parent's line
for a K, a tree line also carries extra_ms_per_step against it and break_even_extra_accepted: the extra accepted tokens per step at
which the tree chain's tokens per second equal the linear chain's, extra_ms / linear_ms per token emitted -- with nothing accepted
a linear step emits one token in linear_ms, so the tree step must emit 1 + extra_ms / linear_ms.
Every leg is run once untimed, then --reps times, wall clock around a drained device, begin subtracted; the spread is reported.
Prints ONE JSON line per leg and, with --out, appends each to that file as it is measured.

Usage:  RAMA_HIP_LIB=<the parent's librama_hip.so> python tools/q8_spec_model_tree_bench.py --parent-build --out profiles/q8_spec_model_tree_bench.jsonl
        python tools/q8_spec_model_tree_bench.py [--reps 3] [--new 24] [--position 9] [--layers 32] --out profiles/q8_spec_model_tree_bench.jsonl
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
DRAFT = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=VOCAB, seq_len=256, shared_weight=True)
NEW_SYMBOLS = ("rama_q8_spec_begin_model_tree", "rama_q8_spec_model_tree_shape", "rama_q8_spec_model_tree_candidates",
               "rama_q8_spec_model_tree_last")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--new", type=int, default=24, help="tokens produced per run: one per step when nothing is accepted")
    ap.add_argument("--position", type=int, default=9, help="context length: the first produced token's position")
    ap.add_argument("--layers", type=int, default=32, help="fewer target layers: a rehearsal")
    ap.add_argument("--parent-build", action="store_true", help="the library loaded is the parent commit's: the linear legs only")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from rama_amd import _lib
    if args.parent_build:
        for s in NEW_SYMBOLS:                            # (the parent's library does not export them, and its legs do not call them)
            _lib.SIGNATURES.pop(s, None)

    parent = {}
    if args.out and Path(args.out).exists():
        for text in Path(args.out).read_text().splitlines():
            line = json.loads(text)
            if line.get("parent_build") and line.get("n_layers") == args.layers:
                parent[line["n_draft"]] = line["ms_per_step"]

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
    dev = rama_amd.Hip(0)
    L, ctx = dev.lib, dev.ctx
    name, cus, _ = dev.info()
    who = "parent" if args.parent_build else "this"
    base = dict(device=name, compute_units=cus, group_size=64, draft_group_size=32, library=library_stamp(), n_layers=args.layers,
                graph_mode=True, parent_build=bool(args.parent_build), new_tokens=args.new, position=args.position)
    m = rama_amd.Q8Model.synth(dev, Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, False), 64, 7)
    dm = rama_amd.Q8Model.synth(dev, Config(**DRAFT), 32, 2)
    eng, deng = rama_amd.Q8Engine(dev, m), rama_amd.Q8Engine(dev, dm)
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
        carr = (C.c_int32 * n_ctx)(*context)
        head = (ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state), C.byref(dm.ccfg), C.byref(dm.weights), C.byref(deng.state),
                carr, n_ctx)
        for K in (2, 4, 7):
            plan = _lib.rama_q8_spec_plan(0.0, 0.9, 0.0, new, -1, K, 3, None, 0)
            for tree in ([None] if args.parent_build else [(1, 16), (2, 16), (3, 16)]):
                kw = dict(n_branch=tree[0], tree_rows=tree[1]) if tree else {}
                got = eng.generate_spec(context, new, n_draft=K, draft=deng, **kw)
                stats = dict(eng.spec_stats)
                if got != want:
                    raise SystemExit(f"K {K} {tree}: the chain's tokens are not the solo run's")
                n_steps = stats["steps"]

                def begin():
                    if tree:
                        check(L.rama_q8_spec_begin_model_tree(*head, C.byref(plan), tree[0], tree[1]))
                    else:
                        check(L.rama_q8_spec_begin_model(*head, C.byref(plan)))

                def run():
                    begin()
                    check(L.rama_q8_spec_steps(ctx, n_steps))
                t_begin = timed(begin)[0]
                med, lo, hi = timed(run)
                ms = (med - t_begin) * 1e3 / n_steps
                kind = f"b{tree[0]}" if tree else "linear"
                line = dict(base, metric=f"q8_spec_model_tree_{who}_k{K}_{kind}", n_draft=K, n_branch=tree[0] if tree else None,
                            n_rows=tree[1] if tree else K + 1, steps=n_steps, accepted=stats["accepted"], ms_per_step=round(ms, 4),
                            spread_ms_per_step=[round((lo - t_begin) * 1e3 / n_steps, 4), round((hi - t_begin) * 1e3 / n_steps, 4)])
                if tree and K in parent:
                    line["extra_ms_per_step"] = round(ms - parent[K], 4)
                    line["break_even_extra_accepted"] = round((ms - parent[K]) / parent[K], 4)
                emit(line)
                check(L.rama_q8_spec_end(ctx))
    finally:
        eng.set_graph_mode(False)
        eng.free(); deng.free(); dm.free(); m.free()
        dev.close()


if __name__ == "__main__":
    main()
