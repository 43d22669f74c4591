#!/usr/bin/env python3
"""The speculative chain with a draft model (rama_q8_spec_begin_model) against rama_q8_generate: what a step with K
WRONG drafts costs.  The target is a llama2-7B-shaped rama_q8_model_synth model (group size 64), the draft a stories15M-shaped one
with vocabulary 32 000 (group size 32); greedy, graph mode on, one process.  Two synthetic models disagree, so acceptance is about 0:
every step pays K draft passes and a K + 1-row target pass for one token.  No trained checkpoint pair is at hand, so the speed at a
real acceptance rate is NOT what this measures.

At each start position (the context is a fixed-seed random text, prefilled untimed on both engines) the tool times
 (base) rama_q8_generate on the target over the same positions.  With --parent-build the library loaded is the parent commit's
        (RAMA_HIP_LIB names it): this leg alone, and its lines -- metric q8_spec_model_parent_* -- are the baseline;
 (k)    the chain for n_draft in 1, 2, 4, 7 over --new tokens.
Every leg is run once untimed, then --reps times, wall clock around a drained device; the spread is reported.  A line carries ms per
step, the accepted drafts per step and -- given --parent-ms, the parent's ms per token from its own line -- the BREAK-EVEN
acceptance: the tokens a step must emit to match the parent, ms_per_step / ms_per_token_parent, as accepted drafts per step (that
minus one) and as a fraction of K.  The chain's tokens are checked against the solo run's before anything is timed.
Prints ONE JSON line per leg and, with --out, appends each to that file as it is measured.

Usage:  RAMA_HIP_LIB=<the parent's librama_hip.so> python tools/q8_spec_model_bench.py --parent-build --out profiles/q8_spec_model_bench.jsonl
        python tools/q8_spec_model_bench.py [--reps 3] [--new 64] [--positions 5,1000] [--layers 32] [--parent-ms 5:3.48,1000:4.05] --out ...
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
DRAFT = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=VOCAB, seq_len=SEQ, shared_weight=True)
NEW_SYMBOLS = ("rama_q8_spec_begin_model", "rama_q8_spec_model_stats")
KS = (1, 2, 4, 7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--new", type=int, default=64, help="tokens produced per run")
    ap.add_argument("--positions", type=str, default="5,1000", help="context lengths: the first produced token's position")
    ap.add_argument("--layers", type=int, default=32, help="fewer target layers: a rehearsal")
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
    dev = rama_amd.Hip(0)
    L, ctx = dev.lib, dev.ctx
    name, cus, _ = dev.info()
    base = dict(device=name, compute_units=cus, group_size=64, draft_group_size=32, library=library_stamp(), n_layers=args.layers,
                draft_shape="stories15M, vocab 32000", graph_mode=True, parent_build=bool(args.parent_build), new_tokens=args.new)
    m = rama_amd.Q8Model.synth(dev, Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, True), 64, 7)
    eng = rama_amd.Q8Engine(dev, m)
    dm = deng = None
    if not args.parent_build:
        dm = rama_amd.Q8Model.synth(dev, Config(**DRAFT), 32, 8)
        deng = rama_amd.Q8Engine(dev, dm)
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
            emit(dict(base, metric=f"q8_spec_model_{'parent' if args.parent_build else 'base'}_generate_pos{n_ctx}", position=n_ctx,
                      tok_s=round(args.new / (med - t_ctx), 1), ms_per_token=round(ms_tok, 4),
                      spread_ms=[round((lo - t_ctx) * 1e3 / args.new, 4), round((hi - t_ctx) * 1e3 / args.new, 4)]))
            if args.parent_build:
                continue
            ref_ms = parent_ms.get(n_ctx)
            carr = (C.c_int32 * n_ctx)(*context)
            for K in KS:
                got = eng.generate_spec(context, args.new, n_draft=K, draft=deng)
                st = eng.spec_stats
                if got != want:
                    raise SystemExit(f"k{K} at {n_ctx}: the chain's tokens are not the solo run's")
                n_steps = sum(st["accepted_hist"])                 # the steps up to the finish: the same at every repeat
                plan = _lib.rama_q8_spec_plan(0.0, 0.9, 0.0, args.new, -1, K, 1, None, 0)

                def begin():
                    # (rows 0 .. n_ctx - 2 are in both caches: the check above wrote them, and nothing below a cursor is ever
                    # rewritten with other bits)
                    check(L.rama_q8_spec_begin_model(ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(eng.state), C.byref(dm.ccfg),
                                                     C.byref(dm.weights), C.byref(deng.state), carr, n_ctx, C.byref(plan)))

                def run():
                    begin()
                    check(L.rama_q8_spec_steps(ctx, n_steps))
                t_begin = timed(begin)[0]
                med, lo, hi = timed(run)
                ms_step = (med - t_begin) * 1e3 / n_steps
                line = dict(base, metric=f"q8_spec_model_k{K}_pos{n_ctx}", position=n_ctx, n_draft=K, steps=n_steps,
                            tok_s=round(args.new / (med - t_begin), 1), ms_per_step=round(ms_step, 4),
                            spread_ms_per_step=[round((lo - t_begin) * 1e3 / n_steps, 4), round((hi - t_begin) * 1e3 / n_steps, 4)],
                            mean_accepted_per_step=round(st["accepted"] / n_steps, 3), catch_up_rows=st["catch_up_rows"],
                            ms_per_token_base=round(ms_tok, 4), step_overhead_vs_base=round(ms_step / ms_tok, 3))
                if ref_ms:
                    need = ms_step / ref_ms                        # tokens a step must emit to match the parent
                    line.update(ms_per_token_parent=ref_ms, step_overhead_vs_parent=round(ms_step / ref_ms, 3),
                                break_even_accepted_per_step=round(max(need - 1.0, 0.0), 3),
                                break_even_acceptance=round(max(need - 1.0, 0.0) / K, 3), reachable=bool(need <= K + 1))
                emit(line)
                check(L.rama_q8_spec_end(ctx))
    finally:
        eng.set_graph_mode(False)
        for e in (eng, deng):
            if e is not None:
                e.free()
        m.free()
        if dm is not None:
            dm.free()
        dev.close()


if __name__ == "__main__":
    main()
