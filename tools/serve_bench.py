#!/usr/bin/env python3
"""Continuous batching in parity mode (the fp32 serving chain, rama_amd.Server) against the schedule the older entries allow in parity mode,
in one process, on a llama2-7B-shaped rama_model_synth model (seq_len 256 so that the run states fit), "ref_order" = 1, graph mode on.

Workload: tools/q8_serve_bench.py's request mix (fixed seed; contexts 16..128 tokens, budgets 16..96 new tokens, greedy, no stop tokens), so
every schedule produces the same tokens and the host plan foresees every step.
 (a) static waves: rama_prefill per request (its context but the last token), then a HOST loop of rama_decode_batch in waves of n_slots
     requests -- one call and n_seq 4-byte downloads (rama_sample_argmax) per step --, each wave run until its longest member ends.
 (b) the serving chain, Server.run, at max_rows in {32, 64}.
for n_slots in 16 and 32.  `ideal` is the ratio of WEIGHT PASSES, (a) to (b), counted by the host plan (rama_q8_serve_plan_step) on the
CPU; a parity-mode pass takes 32 rows: (a) pays ceil(n / 32) passes per decode step of n sequences, ceil(p / 32) per prefill of p positions
and one forward; (b) pays one pass per tile of a step that holds a wanted row (an idle tile is skipped).
 (c) the idle-tile skip: n_slots requests of one context token each (so <= 32 rows are wanted in every step) at max_rows 64 against
     max_rows 32: the same plan, the second tile wholly idle; `idle_tile_cost` is the ratio of the two times per step.
--plan-only prints the host plan's numbers (no GPU).  Otherwise every configuration is run once untimed, then --reps times; ONE JSON line
per configuration, appended to --out as it is measured.

Usage:  python tools/serve_bench.py [--plan-only] [--reps 3] [--requests 256] [--slots 16,32] [--layers 32] [--out profiles/serve_bench.jsonl]
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
sys.path.insert(0, str(REPO / "tools"))

import rama_amd  # noqa: E402
from q8_serve_bench import CTX_RANGE, DIM, HIDDEN, NEW_RANGE, SEQ, VOCAB, workload  # noqa: E402
from rama_amd.q8 import serve_plan_step  # noqa: E402

TILE = 32
ROWS = (32, 64)


def tiles(n):
    return (n + TILE - 1) // TILE


def plan_serve(reqs, n_slots, max_rows):
    """the serving chain's schedule by the host plan: steps, row counts, weight passes (live tiles)"""
    pending = list(reqs)
    t = [(0, 0, 0, 0, 0)] * n_slots
    steps = dec = pro = idle = passes = 0
    while True:
        for i in range(n_slots):
            if t[i][0] in (0, 3) and pending:
                ctx, new = pending.pop(0)
                t[i] = (1, len(ctx), 0, 0, new)
        if not any(s[0] in (1, 2) for s in t):
            return dict(steps=steps, rows_decode=dec, rows_prompt=pro, rows_idle=idle, passes=passes)
        rows, after = serve_plan_step(t, max_rows)
        d = sum(1 for s, _, _ in rows if s >= 0 and t[s][0] == 2)
        used = sum(1 for s, _, _ in rows if s >= 0)
        steps += 1; dec += d; pro += used - d; idle += max_rows - used; passes += tiles(used)
        t = after


def plan_waves(reqs, n_slots):
    """schedule (a): decode steps (each wave runs until its longest member ends) and weight passes"""
    steps = passes = 0
    for i in range(0, len(reqs), n_slots):
        wave = reqs[i:i + n_slots]
        k = max(new for _, new in wave)
        steps += k
        passes += k * tiles(len(wave))
    passes += sum(tiles(max(len(ctx) - 2, 0)) + (1 if len(ctx) > 1 else 0) for ctx, _ in reqs)
    return dict(decode_steps=steps, passes=passes, useful_rows=sum(new for _, new in reqs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan-only", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--slots", type=str, default="16,32")
    ap.add_argument("--layers", type=int, default=32, help="fewer layers: a rehearsal")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    reqs = workload(args.requests)
    total_new = sum(new for _, new in reqs)
    slots = [int(s) for s in args.slots.split(",")]

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    if args.plan_only:
        for n in slots:
            pa = plan_waves(reqs, n)
            for max_rows in ROWS:
                if max_rows >= n:
                    pb = plan_serve(reqs, n, max_rows)
                    emit(dict(metric=f"serve_plan_{n}_rows{max_rows}", n_slots=n, max_rows=max_rows, requests=len(reqs), generated_tokens=total_new,
                              waves_passes=pa["passes"], waves_decode_steps=pa["decode_steps"], chain_passes=pb["passes"], chain_steps=pb["steps"],
                              rows_idle=pb["rows_idle"], ideal=round(pa["passes"] / pb["passes"], 4), measured=None))
        return

    from bench import library_stamp
    from oracle.oracle import Config
    from rama_amd._lib import check, rama_run_state
    dev = rama_amd.Hip(0)
    L, ctx = dev.lib, dev.ctx
    check(L.rama_set_tuning(ctx, b"ref_order", 1))
    name, cus, _ = dev.info()
    from tests.helpers import to_rama_cfg
    m = rama_amd.Model.synth(dev, to_rama_cfg(Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, False)), 7)
    engs = [rama_amd.Engine(dev, m) for _ in range(max(slots))]
    engs[0].set_graph_mode(True)

    def timed(fn):
        fn()                                             # untimed: code objects, scratch, copies, the one graph capture
        ts, out = [], None
        for _ in range(args.reps):
            check(L.rama_sync(ctx))
            t0 = time.perf_counter()
            out = fn()
            check(L.rama_sync(ctx))
            ts.append(time.perf_counter() - t0)
        return ts, out

    def spread(ts, toks):
        med = statistics.median(ts)
        return dict(wall_s=round(med, 4), wall_s_min=round(min(ts), 4), wall_s_max=round(max(ts), 4), reps=len(ts),
                    tok_s=round(toks / med, 1), tok_s_min=round(toks / max(ts), 1), tok_s_max=round(toks / min(ts), 1))

    def waves_of(n):
        def waves():
            out, nxt = [], C.c_int32()
            for i in range(0, len(reqs), n):
                wave = reqs[i:i + n]
                es = engs[:len(wave)]
                for e, (c, _) in zip(es, wave):
                    if len(c) > 1:
                        arr = (C.c_int32 * (len(c) - 1))(*c[:-1])
                        check(L.rama_prefill(ctx, C.byref(m.ccfg), C.byref(m.weights), C.byref(e.state), arr, len(c) - 1, 0), "rama_prefill")
                states = (rama_run_state * len(es))(*[e.state for e in es])
                toks, pos = [c[-1] for c, _ in wave], [len(c) - 1 for c, _ in wave]
                got = [[] for _ in wave]
                for _ in range(max(new for _, new in wave)):
                    check(L.rama_decode_batch(ctx, C.byref(m.ccfg), C.byref(m.weights), states, (C.c_int32 * len(es))(*toks),
                                              (C.c_int32 * len(es))(*pos), len(es)), "rama_decode_batch")
                    for j, e in enumerate(es):
                        check(L.rama_sample_argmax(ctx, e.state.logits, VOCAB, C.byref(nxt)), "rama_sample_argmax")
                        toks[j] = int(nxt.value)
                        got[j].append(toks[j])
                        pos[j] = min(pos[j] + 1, SEQ - 1)
                out += [g[:new] for g, (_, new) in zip(got, wave)]
            return out
        return waves

    def serve_of(srv, rq, got):
        def serve():
            before = srv.stats()
            hs = [srv.submit(c, new) for c, new in rq]
            srv.run()
            got["out"] = [srv.result(h) for h in hs]
            after = srv.stats()
            got["stats"] = {k: after[k] - before[k] for k in ("steps", "rows_decode", "rows_prompt", "rows_idle")}
            got["stats"]["graph_captures"] = after["graph_captures"]
        return serve

    try:
        for n in slots:
            base = dict(device=name, compute_units=cus, library=library_stamp(), mode="parity", n_layers=args.layers, n_slots=n,
                        requests=len(reqs), context_range=list(CTX_RANGE), max_new_range=list(NEW_RANGE), generated_tokens=total_new,
                        graph_mode=True, unit="tok/s")
            pa = plan_waves(reqs, n)
            ts, out_a = timed(waves_of(n))
            line = dict(base, metric=f"serve_static_waves_{n}", schedule="static_waves", **spread(ts, total_new), steps=pa["decode_steps"], passes=pa["passes"])
            line["value"] = a_tok_s = line["tok_s"]
            emit(line)
            for max_rows in ROWS:
                if max_rows < n:
                    continue
                got = {}
                srv = rama_amd.Server(m, n, max_rows, NEW_RANGE[1])
                try:
                    ts, _ = timed(serve_of(srv, reqs, got))
                finally:
                    srv.close()
                pb, st = plan_serve(reqs, n, max_rows), got["stats"]
                line = dict(base, metric=f"serve_chain_{n}_rows{max_rows}", schedule="serving_chain", max_rows=max_rows, **spread(ts, total_new),
                            steps=st["steps"], rows_decode=st["rows_decode"], rows_prompt=st["rows_prompt"], rows_idle=st["rows_idle"],
                            graph_captures=st["graph_captures"], plan_steps=pb["steps"], passes=pb["passes"], ideal=round(pa["passes"] / pb["passes"], 4),
                            same_tokens=got["out"] == out_a)
                line["value"] = line["tok_s"]
                line["over_static_waves"] = round(line["tok_s"] / a_tok_s, 4)
                emit(line)
            # (c) the idle tile: one context token per request, n <= 32 wanted rows in every step
            short = [([1], 64)] * n
            per_step = {}
            for max_rows in ROWS:
                got = {}
                srv = rama_amd.Server(m, n, max_rows, NEW_RANGE[1])
                try:
                    ts, _ = timed(serve_of(srv, short, got))
                finally:
                    srv.close()
                per_step[max_rows] = [t / got["stats"]["steps"] for t in ts]
                line = dict(base, metric=f"serve_idle_tile_{n}_rows{max_rows}", schedule="serving_chain", max_rows=max_rows, requests=n, generated_tokens=64 * n,
                            **spread(ts, 64 * n), steps=got["stats"]["steps"], rows_idle=got["stats"]["rows_idle"],
                            ms_per_step=round(1e3 * statistics.median(per_step[max_rows]), 4), unit="tok/s")
                line["value"] = line["ms_per_step"]
                if max_rows == 64:
                    line["idle_tile_cost"] = round(statistics.median(per_step[64]) / statistics.median(per_step[32]), 4)
                emit(line)
    finally:
        for e in engs:
            e.free()
        m.free()
        check(L.rama_set_tuning(ctx, b"ref_order", 0))
    dev.close()


if __name__ == "__main__":
    main()
