#!/usr/bin/env python3
"""Sampled serving in one batch: aggregate tok/s at 8..128 sequences for
  chained_greedy   rama_decode_batch_begin + _steps (argmax per sequence, one hipGraph replay per step)
  chained_sampled  rama_decode_batch_begin_sampled + _steps (T 1, top-p 0.9, the batched top-p sampler in the same replay)
  host_loop        rama_decode_batch per step, rama_sample_topp_dev row after row, one download of the picks per step
at the llama2-7B shape and stories110M (a short context: 128 sequences x 2 048 positions of KV cache would not fit beside
the 7B model).  Prints one JSON line stamped with the library's source hash.
  --op: the batched sampler alone, 128 rows x 32 000 flat logits (every entry kept), timed with events against the
        single-row sampler row after row (run it under rocprofv3 --kernel-trace --stats for the per-launch split)
Usage: python tools/batch_sample_bench.py [--steps K] [--shapes llama2-7B,stories110M] [--seq S] [--op]"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import rama_amd  # noqa: E402
from rama_amd._lib import check, rama_run_state, rama_seq_sampling  # noqa: E402
from rama_amd.sampler_const import TOPP_U_CPU  # noqa: E402
from bench import SHAPES, library_stamp  # noqa: E402

T, TOPP = 1.0, 0.9


def op_bench(dev, iters):
    rows, n = 128, 32000
    x = (np.random.default_rng(0).standard_normal((rows, n)) * 0.05).astype(np.float32)      # flat: every entry kept
    d_x, d_r = dev.allocate(x), dev.alloc(rows)
    Ts, Ps, Us = [(C.c_float * rows)(*([v] * rows)) for v in (T, TOPP, TOPP_U_CPU)]
    L = dev.lib

    def timed(fn, k):                                   # HIP events around k calls on the context's stream
        fn(); dev.sync()
        check(L.rama_timer_start(dev.ctx))
        for _ in range(k): fn()
        ms = C.c_float()
        check(L.rama_timer_stop(dev.ctx, C.byref(ms)))
        return ms.value * 1e3 / k

    batch_us = timed(lambda: check(L.rama_sample_topp_batch_dev(dev.ctx, d_x.ptr, n, n, rows, Ts, Ps, Us, d_r.ptr)), iters)
    got = dev.download(d_r).view(np.int32).tolist()

    def per_row():
        for r in range(rows):
            check(L.rama_sample_topp_dev(dev.ctx, d_x.ptr + 4 * r * n, n, T, TOPP, TOPP_U_CPU, d_r.ptr + 4 * r))
    loop_us = timed(per_row, max(2, iters // 10))
    same = dev.download(d_r).view(np.int32).tolist() == got
    d_x.free(); d_r.free()
    return {"rows": rows, "n": n, "batch_us_per_call": round(batch_us, 1), "row_loop_us_per_call": round(loop_us, 1),
            "speedup": round(loop_us / batch_us, 2), "same_tokens": same}


def shape_bench(dev, name, steps, seq_override):
    d, h, L_, H, V, seq, shared = SHAPES[name]
    seq = min(seq, seq_override)
    cfg = rama_amd.Config(d, h, L_, H, H, V, seq, shared)
    model = rama_amd.Model.synth(dev, cfg, seed=0)
    L = dev.lib
    out = {}
    for B in (8, 16, 32, 64, 128):
        engs = [rama_amd.Engine(dev, model) for _ in range(B)]
        states = (rama_run_state * B)(*[e.state for e in engs])
        toks = (C.c_int32 * B)(*[1 + i for i in range(B)])
        poss = (C.c_int32 * B)(*([0] * B))
        per = (rama_seq_sampling * B)(*[rama_seq_sampling(T, TOPP, TOPP_U_CPU, None, 0) for _ in range(B)])
        row = {}
        engs[0].set_graph_mode(True)
        for mode in ("chained_greedy", "chained_sampled"):
            if mode == "chained_greedy":
                check(L.rama_decode_batch_begin(dev.ctx, C.byref(model.ccfg), C.byref(model.weights), states, toks, poss, B, steps + 4))
            else:
                check(L.rama_decode_batch_begin_sampled(dev.ctx, C.byref(model.ccfg), C.byref(model.weights), states, toks, poss, B,
                                                        steps + 4, per))
            check(L.rama_decode_batch_steps(dev.ctx, 4))
            dev.sync()
            t0 = time.perf_counter()
            check(L.rama_decode_batch_steps(dev.ctx, steps))
            dev.sync()
            dt = time.perf_counter() - t0
            row[mode] = {"ms_per_step": round(dt * 1e3 / steps, 3), "aggregate_tok_s": round(B * steps / dt, 1)}
        engs[0].set_graph_mode(False)
        # the host loop the chained sampler replaces
        res = dev.alloc(B)
        cur = [1 + i for i in range(B)]

        def step(pos):
            rama_amd.decode_batch(engs, cur, [pos] * B)
            for i, e in enumerate(engs):
                check(L.rama_sample_topp_dev(dev.ctx, e.state.logits, V, T, TOPP, TOPP_U_CPU, res.ptr + 4 * i))
            cur[:] = [max(int(t), 0) for t in dev.download(res).view(np.int32)]
        for p in range(4): step(p)
        dev.sync()
        t0 = time.perf_counter()
        for p in range(4, 4 + steps): step(p)
        dt = time.perf_counter() - t0
        row["host_loop"] = {"ms_per_step": round(dt * 1e3 / steps, 3), "aggregate_tok_s": round(B * steps / dt, 1)}
        row["sampled_over_greedy"] = round(row["chained_sampled"]["aggregate_tok_s"] / row["chained_greedy"]["aggregate_tok_s"], 4)
        row["sampled_over_host_loop"] = round(row["chained_sampled"]["aggregate_tok_s"] / row["host_loop"]["aggregate_tok_s"], 3)
        out[B] = row
        res.free()
        for e in engs: e.free()
    model.free()
    return {"seq_len": seq, "by_batch": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--shapes", default="llama2-7B,stories110M")
    ap.add_argument("--seq", type=int, default=64, help="context length cap (KV cache of 128 sequences beside the model)")
    ap.add_argument("--op", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = rama_amd.Hip(0)
    rec = {"tool": "batch_sample_bench", "library": library_stamp(), "temperature": T, "topp": TOPP, "u": TOPP_U_CPU}
    if a.op:
        rec["op"] = op_bench(dev, a.iters)
    else:
        rec["steps"] = a.steps
        rec["shapes"] = {s: shape_bench(dev, s, a.steps, a.seq) for s in a.shapes.split(",")}
    dev.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
