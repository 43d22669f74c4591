#!/usr/bin/env python3
"""Continuous batching (the serving chain, rama_amd.Q8Server) against the schedule the older entry points allow, in one process, on a
llama2-7B-shaped rama_q8_model_synth model (group size 64, seq_len 256 so that the run states fit), graph mode on.

Workload (fixed seed): --requests requests (default 256), context lengths uniform in 16..128 tokens, budgets uniform in 16..96
new tokens, greedy, no stop tokens -- so every schedule produces the same tokens and the same number of them, and the host plan
foresees every step.
 (a) static waves: rama_q8_prefill per request (its context but the last token), then rama_q8_decode_batch_begin / _steps / _tokens
     in waves of n_slots requests, each wave run until its longest member ends.
 (b) the serving chain, Q8Server.run, at max_rows in {n_slots, 64, 128}.
for n_slots in 16 and 32.  Every configuration is run once untimed, then --reps times (wall clock around a drained stream; the
time of (b) includes the admissions; its one graph capture falls into the untimed run).  The tokens of (a) and (b) are compared: they must be equal.
`ideal` is the ratio of weight passes, (a) to (b), counted by the host plan (rama_q8_serve_plan_step) on the CPU: (a)'s passes are
its decode steps plus one pass per 128 prefilled positions and one forward for the last one.
Prints ONE JSON line per configuration and, with --out, appends each to that file as it is measured.

Usage:  python tools/q8_serve_bench.py [--reps 3] [--requests 256] [--slots 16,32] [--layers 32] [--out profiles/q8_serve_bench.jsonl]
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

import rama_amd  # noqa: E402
from bench import library_stamp  # noqa: E402
from oracle.oracle import Config  # noqa: E402
from rama_amd._lib import check  # noqa: E402
from rama_amd.q8 import Q8Server, decode_batch_chained, serve_plan_step  # noqa: E402

DIM, HIDDEN, VOCAB, SEQ = 4096, 11008, 32000, 256
CTX_RANGE, NEW_RANGE = (16, 128), (16, 96)              # inclusive


def workload(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        n_ctx = int(rng.integers(CTX_RANGE[0], CTX_RANGE[1] + 1))
        new = int(rng.integers(NEW_RANGE[0], NEW_RANGE[1] + 1))
        out.append(([1] + [int(t) for t in rng.integers(2, VOCAB, n_ctx - 1)], new))
    return out


def plan_serve(reqs, n_slots, max_rows):
    """the serving chain's schedule by the host plan: steps and row counts"""
    pending = list(reqs)
    t = [(0, 0, 0, 0, 0)] * n_slots
    steps = dec = pro = idle = 0
    while True:
        for i in range(n_slots):
            if t[i][0] in (0, 3) and pending:
                ctx, new = pending.pop(0)
                t[i] = (1, len(ctx), 0, 0, new)
        if not any(s[0] in (1, 2) for s in t):
            return dict(steps=steps, rows_decode=dec, rows_prompt=pro, rows_idle=idle)
        rows, after = serve_plan_step(t, max_rows)
        d = sum(1 for s, _, _ in rows if s >= 0 and t[s][0] == 2)
        used = sum(1 for s, _, _ in rows if s >= 0)
        steps += 1; dec += d; pro += used - d; idle += max_rows - used
        t = after


def plan_waves(reqs, n_slots):
    """schedule (a): decode steps (each wave runs until its longest member ends) and prefill weight passes"""
    steps = sum(max(new for _, new in reqs[i:i + n_slots]) for i in range(0, len(reqs), n_slots))
    passes = sum((max(len(ctx) - 2, 0) + 127) // 128 + (1 if len(ctx) > 1 else 0) for ctx, _ in reqs)
    useful = sum(new for _, new in reqs)
    return dict(decode_steps=steps, prefill_passes=passes, useful_rows=useful, rows=steps * n_slots)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--slots", type=str, default="16,32")
    ap.add_argument("--layers", type=int, default=32, help="fewer layers: a rehearsal")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    reqs = workload(args.requests)
    total_new = sum(new for _, new in reqs)
    dev = rama_amd.Hip(0)
    L, ctx = dev.lib, dev.ctx
    name, cus, _ = dev.info()
    m = rama_amd.Q8Model.synth(dev, Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, False), 64, 7)
    slots = [int(s) for s in args.slots.split(",")]
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(max(slots))]
    engs[0].set_graph_mode(True)

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    def timed(fn):
        fn()                                             # untimed: code objects, scratch
        ts, out = [], None
        for _ in range(args.reps):
            check(L.rama_sync(ctx))
            t0 = time.perf_counter()
            out = fn()
            check(L.rama_sync(ctx))
            ts.append(time.perf_counter() - t0)
        return ts, out

    def spread(ts):
        return dict(wall_s=round(statistics.median(ts), 4), wall_s_min=round(min(ts), 4), wall_s_max=round(max(ts), 4), reps=len(ts),
                    tok_s=round(total_new / statistics.median(ts), 1), tok_s_min=round(total_new / max(ts), 1), tok_s_max=round(total_new / min(ts), 1))

    try:
        for n in slots:
            def waves():
                out = []
                for i in range(0, len(reqs), n):
                    wave = reqs[i:i + n]
                    es = engs[:len(wave)]
                    for e, (c, _) in zip(es, wave):
                        if len(c) > 1:
                            e.prefill(c[:-1], 0)
                    out += decode_batch_chained(es, [c[-1] for c, _ in wave], [len(c) - 1 for c, _ in wave], max(new for _, new in wave),
                                                max_new=[new for _, new in wave])
                return out

            base = dict(device=name, compute_units=cus, group_size=64, library=library_stamp(), n_layers=args.layers, n_slots=n,
                        requests=len(reqs), context_range=list(CTX_RANGE), max_new_range=list(NEW_RANGE), generated_tokens=total_new,
                        graph_mode=True, unit="tok/s")
            pa = plan_waves(reqs, n)
            ts, out_a = timed(waves)
            a_passes = pa["decode_steps"] + pa["prefill_passes"]
            line = dict(base, metric=f"q8_serve_static_waves_{n}", schedule="static_waves", **spread(ts), steps=pa["decode_steps"],
                        prefill_passes=pa["prefill_passes"], rows_decode=pa["useful_rows"], rows_prompt=0, rows_idle=pa["rows"] - pa["useful_rows"])
            line["value"] = line["tok_s"]
            a_tok_s = line["tok_s"]
            emit(line)
            for max_rows in sorted({n, 64, 128}):
                got = {}
                srv = Q8Server(m, n, max_rows, NEW_RANGE[1])     # one server per configuration: its slots are reused run after run

                def serve():
                    before = srv.stats()
                    hs = [srv.submit(c, new) for c, new in reqs]
                    srv.run()
                    got["out"] = [srv.result(h) for h in hs]
                    after = srv.stats()
                    got["stats"] = {k: after[k] - before[k] for k in ("steps", "rows_decode", "rows_prompt", "rows_idle")}
                    got["stats"]["graph_captures"] = after["graph_captures"]

                try:
                    ts, _ = timed(serve)
                finally:
                    srv.close()
                pb, st = plan_serve(reqs, n, max_rows), got["stats"]
                line = dict(base, metric=f"q8_serve_chain_{n}_rows{max_rows}", schedule="serving_chain", max_rows=max_rows, **spread(ts),
                            steps=st["steps"], rows_decode=st["rows_decode"], rows_prompt=st["rows_prompt"], rows_idle=st["rows_idle"],
                            graph_captures=st["graph_captures"], plan_steps=pb["steps"], ideal=round(a_passes / pb["steps"], 4),
                            same_tokens=got["out"] == out_a)
                line["value"] = line["tok_s"]
                line["over_static_waves"] = round(line["tok_s"] / a_tok_s, 4)
                emit(line)
    finally:
        for e in engs:
            e.free()
        m.free()
    dev.close()


if __name__ == "__main__":
    main()
