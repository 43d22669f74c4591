#!/usr/bin/env python3
"""The speculative chain (rama_q8_spec_begin / _steps) against rama_q8_generate on a llama2-7B-shaped
rama_q8_model_synth model (group size 64), greedy, graph mode on, in one process.

At each start position (5 and around 1 000: the context is a fixed-seed random text, prefilled untimed) the model produces
--new tokens, and the tool times
 (base) rama_q8_generate over the same positions.  With --parent-build the library loaded is the parent commit's (RAMA_HIP_LIB
        names it): this leg alone, and its lines -- metric q8_spec_parent_* -- are the baseline of the comparison.
 (a) the upper bound: hint = the solo run's own output, so every draft is accepted, for n_draft in 1, 3, 7, 15;
 (b) no hint, n_draft 7, ngram 3: what lookup in the model's own greedy output gives;
 (c) n_draft 0: the chain's floor, one row through the batch pass.
Every leg is run once untimed, then --reps times, wall clock around a drained device; the spread is reported.  A line carries
tok/s, ms per step, the mean tokens accepted per step, and -- given --parent-ms, the parent's ms per token from its own line --
the break-even acceptance: the step time at K + 1 rows divided by the parent's time per token.  The chain's tokens are checked
against the solo run's before anything is timed.
Prints ONE JSON line per leg and, with --out, appends each to that file as it is measured.

Usage:  RAMA_HIP_LIB=<the parent's librama_hip.so> python tools/q8_spec_bench.py --parent-build --out profiles/q8_spec_bench.jsonl
        python tools/q8_spec_bench.py [--reps 3] [--new 128] [--positions 5,1000] [--layers 32] [--parent-ms 5:3.48,1000:4.05] --out ...
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
NEW_SYMBOLS = ("rama_q8_spec_begin", "rama_q8_spec_steps", "rama_q8_spec_poll", "rama_q8_spec_tokens", "rama_q8_spec_stats",
               "rama_q8_spec_end", "rama_q8_spec_draft", "rama_q8_spec_accept")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--new", type=int, default=128, help="tokens produced per run")
    ap.add_argument("--positions", type=str, default="5,1000", help="context lengths: the first produced token's position")
    ap.add_argument("--layers", type=int, default=32, help="fewer layers: a rehearsal")
    ap.add_argument("--parent-build", action="store_true", help="the library loaded is the parent commit's: the base leg only")
    ap.add_argument("--parent-ms", type=str, default="", help="position:ms per token of the parent's lines, for the break-even acceptance")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from rama_amd import _lib
    if args.parent_build:
        for s in NEW_SYMBOLS:                            # (the parent's library does not export them, and the base leg does not call them)
            _lib.SIGNATURES.pop(s, None)
    parent_ms = {int(k): float(v) for k, v in (kv.split(":") for kv in args.parent_ms.split(",") if kv)}

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
    from rama_amd.q8 import spec_replay
    dev = rama_amd.Hip(0)
    L, ctx = dev.lib, dev.ctx
    name, cus, _ = dev.info()
    base = dict(device=name, compute_units=cus, group_size=64, library=library_stamp(), n_layers=args.layers, graph_mode=True,
                parent_build=bool(args.parent_build), new_tokens=args.new)
    m = rama_amd.Q8Model.synth(dev, Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, True), 64, 7)
    eng = rama_amd.Q8Engine(dev, m)
    eng.set_graph_mode(True)
    rng = np.random.default_rng(0)

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
        for n_ctx in [int(p) for p in args.positions.split(",")]:
            context = [1] + [int(t) for t in rng.integers(2, VOCAB, n_ctx - 1)]
            want = eng.generate(context[1:], n_ctx - 1 + args.new)[n_ctx - 1:]

            # base: the decode steps alone -- the context is a forced prompt, so its positions are timed apart and subtracted
            def solo(steps):
                return lambda: eng.generate(context[1:], steps)
            t_ctx = timed(solo(n_ctx - 1))[0] if n_ctx > 1 else 0.0
            med, lo, hi = timed(solo(n_ctx - 1 + args.new))
            ms_tok = (med - t_ctx) * 1e3 / args.new
            emit(dict(base, metric=f"q8_spec_{'parent' if args.parent_build else 'base'}_generate_pos{n_ctx}", position=n_ctx,
                      tok_s=round(args.new / (med - t_ctx), 1), ms_per_token=round(ms_tok, 4),
                      spread_ms=[round((lo - t_ctx) * 1e3 / args.new, 4), round((hi - t_ctx) * 1e3 / args.new, 4)]))
            if args.parent_build:
                continue
            ref_ms = parent_ms.get(n_ctx)
            legs = [(f"a_hint_k{k}", k, 3, want) for k in (1, 3, 7, 15)] + [("b_self_k7", 7, 3, None), ("c_floor_k0", 0, 3, None)]
            for leg, K, N, hint in legs:
                traj = spec_replay(want, context, hint, K, N, args.new, None)
                n_steps = len(traj)
                got = eng.generate_spec(context, args.new, n_draft=K, ngram=N, hint=hint)
                if got != want or eng.spec_stats["steps"] < n_steps:
                    raise SystemExit(f"{leg} at {n_ctx}: the chain's tokens are not the solo run's")
                harr = (C.c_int32 * max(len(hint or []), 1))(*(hint or []))
                plan = _lib.rama_q8_spec_plan(0.0, 0.9, 0.0, args.new, -1, K, N, harr if hint else None, len(hint or []))
                carr = (C.c_int32 * n_ctx)(*context)

                def run():
                    # (rows 0 .. n_ctx - 2 are in the caches: the solo run and the check above wrote them, and nothing below the
                    # cursor is ever rewritten with other bits)
                    check(L.rama_q8_spec_begin(ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state), carr, n_ctx, C.byref(plan)))
                    check(L.rama_q8_spec_steps(ctx, n_steps))
                t_begin = timed(lambda: check(L.rama_q8_spec_begin(ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state), carr, n_ctx,
                                                                   C.byref(plan))))[0]
                med, lo, hi = timed(run)
                ms_step = (med - t_begin) * 1e3 / n_steps
                line = dict(base, metric=f"q8_spec_{leg}_pos{n_ctx}", position=n_ctx, n_draft=K, ngram=N, hint=bool(hint), steps=n_steps,
                            tok_s=round(args.new / (med - t_begin), 1), ms_per_step=round(ms_step, 4),
                            spread_ms_per_step=[round((lo - t_begin) * 1e3 / n_steps, 4), round((hi - t_begin) * 1e3 / n_steps, 4)],
                            mean_accepted_per_step=round(sum(a for _, a, _ in traj) / n_steps, 3),
                            mean_emitted_per_step=round(args.new / n_steps, 3), ms_per_token_base=round(ms_tok, 4))
                if ref_ms:
                    line.update(ms_per_token_parent=ref_ms, break_even_tokens_per_step=round(ms_step / ref_ms, 3),
                                speedup_vs_parent=round(ref_ms * args.new / ((med - t_begin) * 1e3), 3))
                emit(line)
                check(L.rama_q8_spec_end(ctx))
    finally:
        eng.set_graph_mode(False)
        eng.free(); m.free()
        dev.close()


if __name__ == "__main__":
    main()
