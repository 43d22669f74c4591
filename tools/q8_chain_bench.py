#!/usr/bin/env python3
"""The chained Q8 batch (rama_q8_decode_batch_begin / _steps / _tokens) against the host-driven loop it replaces, in one process
and run, on a llama2-7B-shaped rama_q8_model_synth model (group size 64, seq_len 256 so that 128 run states fit), graph mode on.

Cases: greedy and sampled (temperature 1, top-p 0.9, one draw per sequence) at 8, 32 and 128 sequences, --steps steps from
positions 200 .. 239 spread.
* chained: rama_q8_decode_batch_steps(steps) + rama_q8_decode_batch_tokens; rama_q8_decode_batch_begin is timed apart (once a chain).
* host-driven, per step: rama_q8_decode_batch, one rama_sample_topp_dev (greedy: rama_argmax_dev) per row on the sequence's own
  logits into one device array, one download of the n tokens, which feed the next step.
Both are run once untimed first (code objects, scratch, the captured step); a time is the best of --reps wall-clock times around
a drained stream.  The token lists of the two loops are compared: they must be equal.
Prints ONE JSON line per case and, with --out, appends each to that file as it is measured.

Usage:  python tools/q8_chain_bench.py [--reps 3] [--steps 16] [--sizes 8,32,128] [--layers 32] [--out profiles/q8_chain_bench.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

import rama_amd  # noqa: E402
from bench import library_stamp  # noqa: E402
from oracle.oracle import Config  # noqa: E402
from rama_amd._lib import check, rama_q8_seq_plan, rama_run_state  # noqa: E402
from rama_amd.q8 import decode_batch  # noqa: E402

DIM, HIDDEN, VOCAB, SEQ = 4096, 11008, 32000, 256


def best_of(dev, fn, reps):
    fn()                                               # warm
    best, out = float("inf"), None
    for _ in range(reps):
        check(dev.lib.rama_sync(dev.ctx))
        t0 = time.perf_counter()
        out = fn()
        check(dev.lib.rama_sync(dev.ctx))
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--sizes", type=str, default="8,32,128")
    ap.add_argument("--layers", type=int, default=32, help="fewer layers: a rehearsal")
    ap.add_argument("--no-baseline", action="store_true", help="the chained loop only (a profiler run)")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    K = args.steps
    dev = rama_amd.Hip(0)
    L, ctx = dev.lib, dev.ctx
    name, cus, _ = dev.info()
    rng = np.random.default_rng(0)
    m = rama_amd.Q8Model.synth(dev, Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, False), 64, 7)
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(max(sizes))]
    engs[0].set_graph_mode(True)
    picks = dev.alloc(max(sizes))                       # the host-driven loop's device array of picks
    cfg, w = C.byref(m.ccfg), C.byref(m.weights)
    try:
        for n in sizes:
            es = engs[:n]
            toks0 = [int(t) for t in rng.integers(0, VOCAB, n)]
            poss0 = [200 + (i * 7) % 40 for i in range(n)]
            us = [float(x) for x in rng.random(n) * 0.98]
            states = (rama_run_state * n)(*[e.state for e in es])
            for mode in ("greedy", "sampled"):
                T = 0.0 if mode == "greedy" else 1.0
                per = (rama_q8_seq_plan * n)(*[rama_q8_seq_plan(T, 0.9, us[i], None, 0, 0, -1) for i in range(n)])
                begin_s = [0.0]

                def chained():
                    t0 = time.perf_counter()
                    check(L.rama_q8_decode_batch_begin(ctx, cfg, w, states, (C.c_int32 * n)(*toks0), (C.c_int32 * n)(*poss0), n, K, per),
                          "rama_q8_decode_batch_begin")
                    check(L.rama_sync(ctx))
                    begin_s[0] = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    check(L.rama_q8_decode_batch_steps(ctx, K), "rama_q8_decode_batch_steps")
                    out = (C.c_int32 * (n * K))()
                    cnt = (C.c_int32 * n)()
                    check(L.rama_q8_decode_batch_tokens(ctx, out, K, cnt), "rama_q8_decode_batch_tokens")
                    chained.steps_s = time.perf_counter() - t0
                    return [[int(out[s * K + j]) for j in range(cnt[s])] for s in range(n)]

                def host_driven():
                    toks, poss, out = list(toks0), list(poss0), [[] for _ in range(n)]
                    for _ in range(K):
                        decode_batch(es, toks, poss)
                        for i, e in enumerate(es):
                            if T == 0.0:
                                check(L.rama_argmax_dev(ctx, e.state.logits, VOCAB, picks.ptr + 4 * i), "rama_argmax_dev")
                            else:
                                check(L.rama_sample_topp_dev(ctx, e.state.logits, VOCAB, T, 0.9, us[i], picks.ptr + 4 * i), "rama_sample_topp_dev")
                        got = dev.download(picks).view(np.int32)[:n]
                        toks = [max(int(t), 0) for t in got]              # (a sample that keeps nothing, -1, feeds token 0)
                        poss = [p + 1 for p in poss]
                        for i in range(n):
                            out[i].append(toks[i])
                    return out

                # the chained time is what the steps and the token download take; begin is reported apart
                chained()
                tc, out_c = float("inf"), None
                for _ in range(args.reps):
                    out_c = chained()
                    tc = min(tc, chained.steps_s)
                line = {"metric": f"q8_chain_tok_s_llama2_7b_{mode}_{n}", "device": name, "compute_units": cus, "group_size": 64,
                        "library": library_stamp(), "n_layers": args.layers, "n_seq": n, "mode": mode, "steps": K, "graph_mode": True,
                        "chained_step_ms": round(tc / K * 1e3, 3), "chained_tok_s": round(n * K / tc, 1), "begin_ms": round(begin_s[0] * 1e3, 3)}
                if not args.no_baseline:
                    th, out_h = best_of(dev, host_driven, args.reps)
                    line.update(host_step_ms=round(th / K * 1e3, 3), host_tok_s=round(n * K / th, 1), chained_over_host=round(th / tc, 4),
                                same_tokens=out_c == out_h)
                line.update(value=line["chained_tok_s"], unit="tok/s")
                print(json.dumps(line), flush=True)
                if args.out:
                    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                    with open(args.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
    finally:
        picks.free()
        for e in engs:
            e.free()
        m.free()
    dev.close()


if __name__ == "__main__":
    main()
