#!/usr/bin/env python3
"""Prompt caching for the serving chain (rama_q8_kv_fork, rama_q8_serve_admit_at, Q8Server(prefix_cache=k)) on a
llama2-7B-shaped rama_q8_model_synth model (group size 64), graph mode on, in one process.

Workload (fixed seed): 128 requests, four 512-token system prompts with 32 requests each (interleaved), tails uniform in 16..64
tokens, budgets uniform in 16..96 new tokens, greedy, no stop tokens -- so the tokens are the same with the cache on and off and
the host plan foresees every step.
 (a) the serving chain with the cache off: only entries the parent commit has (Q8Server(m, n, max_rows, cap), submit(ctx, new)).
     With --parent-build the tool runs against a library of the parent commit (RAMA_HIP_LIB names it): leg (a) alone, and its
     lines -- metric q8_prefix_off_parent_* -- are the baseline.
 (b) the cache on: Q8Server(..., prefix_cache=4); the first request of each system prompt is submitted with retain=True and
     served to its end before the timed part, which is the 124 others (the same 124 in (a)).
 (c) the fork alone: rama_q8_kv_fork of 128 / 512 / 1 024 / 1 900 rows to 1, 4 and 16 destinations against hipMemcpyAsync
     device-to-device over the same 2 * n_layers spans per destination, wall clock around a drained device, --fork-iters calls
     per timing.
for n_slots in 16 and 32 and max_rows in {n_slots, 64}.  Every configuration is run once untimed, then --reps times; the spread
is reported.  `plan_prompt_rows_ratio` is the ratio of prompt rows by the host plan (rama_q8_serve_plan_step), cache on over
cache off: computable without a GPU (--plan-only), the schedule's ideal gain.
Prints ONE JSON line per configuration and, with --out, appends each to that file as it is measured.

Usage:  python tools/q8_prefix_bench.py [--reps 3] [--slots 16,32] [--layers 32] [--legs abc] [--out profiles/q8_prefix_bench.jsonl]
        RAMA_HIP_LIB=<the parent's librama_hip.so> python tools/q8_prefix_bench.py --parent-build --out ...
        python tools/q8_prefix_bench.py --plan-only
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

DIM, HIDDEN, VOCAB = 4096, 11008, 32000
N_PREFIX, PREFIX_LEN, PER_PREFIX = 4, 512, 32
TAIL_RANGE, NEW_RANGE = (16, 64), (16, 96)             # inclusive
SEQ = 704                                               # 512 + 64 + 96 = 672 positions at most
FORK_SEQ, FORK_ROWS, FORK_DSTS = 2048, (128, 512, 1024, 1900), (1, 4, 16)
NEW_SYMBOLS = ("rama_q8_serve_admit_at", "rama_q8_kv_fork")


def workload(seed=0):
    """-> (the first request of every system prompt, the 124 others): (context, max_new)"""
    rng = np.random.default_rng(seed)
    prefixes = [[1] + [int(t) for t in rng.integers(2, VOCAB, PREFIX_LEN - 1)] for _ in range(N_PREFIX)]
    first, rest = [], []
    for k in range(PER_PREFIX):
        for pre in prefixes:
            tail = [int(t) for t in rng.integers(2, VOCAB, int(rng.integers(TAIL_RANGE[0], TAIL_RANGE[1] + 1)))]
            new = int(rng.integers(NEW_RANGE[0], NEW_RANGE[1] + 1))
            (first if k == 0 else rest).append((pre + tail, new))
    return first, rest


def plan(reqs, n_slots, max_rows, n_cached):
    """the schedule by the host plan: steps and row counts, every request admitted at cursor n_cached"""
    from rama_amd.q8 import serve_plan_step
    pending = list(reqs)
    t = [(0, 0, 0, 0, 0)] * n_slots
    steps = dec = pro = idle = 0
    while True:
        for i in range(n_slots):
            if t[i][0] in (0, 3) and pending:
                ctx, new = pending.pop(0)
                t[i] = (1, len(ctx), min(n_cached, len(ctx) - 1), 0, new)
        if not any(s[0] in (1, 2) for s in t):
            return dict(steps=steps, rows_decode=dec, rows_prompt=pro, rows_idle=idle)
        rows, after = serve_plan_step(t, max_rows)
        d = sum(1 for s, _, _ in rows if s >= 0 and t[s][0] == 2)
        used = sum(1 for s, _, _ in rows if s >= 0)
        steps += 1; dec += d; pro += used - d; idle += max_rows - used
        t = after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=str, default="16,32")
    ap.add_argument("--layers", type=int, default=32, help="fewer layers: a rehearsal")
    ap.add_argument("--legs", type=str, default="abc")
    ap.add_argument("--fork-iters", type=int, default=5)
    ap.add_argument("--parent-build", action="store_true", help="the library loaded is the parent commit's: leg (a) only")
    ap.add_argument("--plan-only", action="store_true", help="the host plan's ratios, no GPU")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from rama_amd import _lib
    if args.parent_build:
        for s in NEW_SYMBOLS:                            # (the parent's library does not export them, and leg (a) does not call them)
            _lib.SIGNATURES.pop(s, None)
        args.legs = "a"
    first, rest = workload()
    slots = [int(s) for s in args.slots.split(",")]
    total_new = sum(new for _, new in rest)

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    def plans(n, max_rows):
        off, on = plan(rest, n, max_rows, 0), plan(rest, n, max_rows, PREFIX_LEN)
        return off, on, dict(plan_prompt_rows_off=off["rows_prompt"], plan_prompt_rows_on=on["rows_prompt"],
                             plan_prompt_rows_ratio=round(on["rows_prompt"] / off["rows_prompt"], 4),
                             plan_steps_off=off["steps"], plan_steps_on=on["steps"], plan_steps_ratio=round(on["steps"] / off["steps"], 4))

    if args.plan_only:
        for n in slots:
            for max_rows in sorted({n, 64}):
                emit(dict(metric=f"q8_prefix_plan_{n}_rows{max_rows}", n_slots=n, max_rows=max_rows, requests=len(rest), **plans(n, max_rows)[2]))
        return

    import rama_amd
    from bench import library_stamp
    from oracle.oracle import Config
    from rama_amd._lib import check, rama_config, rama_run_state
    from rama_amd.q8 import Q8Server
    dev = rama_amd.Hip(0)
    L, ctx = dev.lib, dev.ctx
    name, cus, _ = dev.info()
    base = dict(device=name, compute_units=cus, group_size=64, library=library_stamp(), n_layers=args.layers, graph_mode=True,
                parent_build=bool(args.parent_build))

    def timed(fn, reps):
        fn()                                             # untimed: code objects, scratch, the graph capture
        ts = []
        for _ in range(reps):
            check(L.rama_sync(ctx))
            t0 = time.perf_counter()
            fn()
            check(L.rama_sync(ctx))
            ts.append(time.perf_counter() - t0)
        return ts

    def spread(ts, scale=1.0):
        return dict(wall_s=round(statistics.median(ts) * scale, 6), wall_s_min=round(min(ts) * scale, 6), wall_s_max=round(max(ts) * scale, 6), reps=len(ts))

    if "a" in args.legs or "b" in args.legs:
        m = rama_amd.Q8Model.synth(dev, Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, False), 64, 7)
        check(L.rama_set_graph_mode(ctx, 1))
        try:
            for n in slots:
                for max_rows in sorted({n, 64}):
                    wl = dict(base, n_slots=n, max_rows=max_rows, requests=len(rest), system_prompts=N_PREFIX, prefix_len=PREFIX_LEN,
                              tail_range=list(TAIL_RANGE), max_new_range=list(NEW_RANGE), generated_tokens=total_new, unit="tok/s")
                    _, _, ratios = plans(n, max_rows)
                    out, off_tok_s = {}, None
                    for leg in "ab":
                        if leg not in args.legs:
                            continue
                        # (a): nothing but what the parent commit has
                        srv = Q8Server(m, n, max_rows, NEW_RANGE[1]) if leg == "a" else Q8Server(m, n, max_rows, NEW_RANGE[1], prefix_cache=N_PREFIX)
                        got = {}
                        try:
                            if leg == "b":
                                for c, new in first:
                                    srv.submit(c, new, retain=True)
                                srv.run()

                            def serve():
                                before = srv.stats()
                                hs = [srv.submit(c, new) for c, new in rest]
                                srv.run()
                                got["out"] = [srv.result(h) for h in hs]
                                after = srv.stats()
                                got["stats"] = {k: after[k] - before[k] for k in ("steps", "rows_decode", "rows_prompt", "rows_idle") + (("rows_cached",) if leg == "b" else ())}
                            ts = timed(serve, args.reps)
                        finally:
                            srv.close()
                        out[leg] = got["out"]
                        tag = "off_parent" if args.parent_build else ("off" if leg == "a" else "on")
                        line = dict(wl, metric=f"q8_prefix_{tag}_{n}_rows{max_rows}", prefix_cache=0 if leg == "a" else N_PREFIX, **spread(ts), **got["stats"], **ratios)
                        line["tok_s"] = round(total_new / statistics.median(ts), 1)
                        line["tok_s_min"], line["tok_s_max"] = round(total_new / max(ts), 1), round(total_new / min(ts), 1)
                        line["value"] = line["tok_s"]
                        if leg == "a":
                            off_tok_s = line["tok_s"]
                        elif off_tok_s:
                            line["over_cache_off_same_build"] = round(line["tok_s"] / off_tok_s, 4)
                            line["same_tokens"] = out["b"] == out["a"]
                        emit(line)
        finally:
            check(L.rama_set_graph_mode(ctx, 0))
            m.free()

    if "c" in args.legs:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        cc = rama_config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, FORK_SEQ, 0)
        states = []
        try:
            for _ in range(1 + max(FORK_DSTS)):
                s = rama_run_state()
                check(L.rama_state_create(ctx, C.byref(cc), args.layers, C.byref(s)), "rama_state_create")
                states.append(s)
            layer = FORK_SEQ * DIM * 4
            for rows in FORK_ROWS:
                for n_dst in FORK_DSTS:
                    dsts = (rama_run_state * n_dst)(*states[1:1 + n_dst])
                    span = rows * DIM * 4

                    def fork():
                        for _ in range(args.fork_iters):
                            check(L.rama_q8_kv_fork(ctx, C.byref(cc), C.byref(states[0]), dsts, n_dst, rows), "rama_q8_kv_fork")

                    def copies():
                        for _ in range(args.fork_iters):
                            for d in range(n_dst):
                                for name_ in ("key_cache", "value_cache"):
                                    a, b = getattr(states[0], name_), getattr(dsts[d], name_)
                                    for li in range(args.layers):
                                        if hip.hipMemcpyAsync(b + li * layer, a + li * layer, span, 3, None) != 0:      # 3: device to device
                                            raise RuntimeError("hipMemcpyAsync failed")
                        if hip.hipDeviceSynchronize() != 0:
                            raise RuntimeError("hipDeviceSynchronize failed")
                    tf, tc = timed(fork, args.reps), timed(copies, args.reps)
                    moved = 2 * args.layers * span * n_dst                # bytes written per call
                    f_med, c_med = statistics.median(tf) / args.fork_iters, statistics.median(tc) / args.fork_iters
                    line = dict(base, metric=f"q8_kv_fork_{rows}rows_{n_dst}dst", rows=rows, n_dst=n_dst, bytes_written=moved, calls_per_timing=args.fork_iters,
                                fork=spread(tf, 1.0 / args.fork_iters), memcpy=spread(tc, 1.0 / args.fork_iters),
                                fork_written_GBps=round(moved / f_med / 1e9, 1), memcpy_written_GBps=round(moved / c_med / 1e9, 1),
                                fork_over_memcpy_time=round(f_med / c_med, 4), unit="GB/s written")
                    line["value"] = line["fork_written_GBps"]
                    emit(line)
        finally:
            for s in states:
                L.rama_state_free(ctx, C.byref(s))
    dev.close()


if __name__ == "__main__":
    main()
