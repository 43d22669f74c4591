#!/usr/bin/env python3
"""Q8_0 token batches: prompt and aggregate decode throughput of rama_q8_prefill / rama_q8_decode_batch on a llama2-7B-shaped
rama_q8_model_synth model (group size 64), against the single-token rama_q8_forward loop.  Prints ONE JSON line.

* prefill: prompts of 128, 512 and 1024 tokens from position 0 (model seq_len 1024); baseline: one rama_q8_forward per position.
* decode batch: 1 .. 128 sequences at positions 200 .. 200 + n - 1 spread (model seq_len 256, so 128 run states fit);
  baseline: one rama_q8_forward per sequence, in rounds of at most 16 run states (the context's Q8 graph cache).
Every timed shape is run once untimed first; a time is the best of --reps, between device events on the context's stream
(rama_timer_start / rama_timer_stop, which synchronises).  Graph mode is on (it only affects the single-token forwards).

Usage:  python tools/q8_batch_bench.py [--reps 3] [--out profiles/q8_batch_bench.jsonl] [--quick] [--no-baseline]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

import rama_amd  # noqa: E402
from bench import library_stamp  # noqa: E402
from oracle.oracle import Config  # noqa: E402
from rama_amd.q8 import decode_batch  # noqa: E402

PEAK_BPS = 8.0e12
PEAK_I8_OPS = 5.0e15          # dense int8 matrix-core peak (2x bf16), MI355X
DIM, HIDDEN, LAYERS, VOCAB = 4096, 11008, 32, 32000


def timed(dev, fn, reps):
    L, best = dev.lib, float("inf")
    fn()                                               # warm: code objects, scratch, graphs
    for _ in range(reps):
        assert L.rama_timer_start(dev.ctx) == 0
        fn()
        ms = C.c_float()
        assert L.rama_timer_stop(dev.ctx, C.byref(ms)) == 0
        best = min(best, ms.value * 1e-3)
    return best


def product_model(n_tok):
    """bytes and int8 ops of one layer stack + classifier pass for n_tok tokens, from shapes"""
    w = LAYERS * (4 * DIM * DIM + 3 * HIDDEN * DIM) + VOCAB * DIM
    scales = w // 64 * 4
    return w + scales, 2 * w * n_tok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="fewer shapes (a rehearsal)")
    ap.add_argument("--no-baseline", action="store_true", help="skip the single-token loops (a profiler run)")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    dev = rama_amd.Hip(0)
    name, cus, _ = dev.info()
    rng = np.random.default_rng(0)
    res = {"metric": "q8_prefill_tok_s_llama2_7b_512", "device": name, "compute_units": cus, "group_size": 64,
           "library": library_stamp()}

    # ---- prefill
    m = rama_amd.Q8Model.synth(dev, Config(DIM, HIDDEN, LAYERS, 32, 32, VOCAB, 1024, False), 64, 7)
    eng = rama_amd.Q8Engine(dev, m)
    eng.set_graph_mode(True)
    try:
        res["bytes_per_pass"] = m.bytes
        pre = {}
        for n in ((128, 512) if args.quick else (128, 512, 1024)):
            toks = [1] + [int(t) for t in rng.integers(0, VOCAB, n - 1)]

            def loop():
                for p, t in enumerate(toks):
                    eng.forward(t, p)
            tb = timed(dev, lambda: eng.prefill(toks, 0), args.reps)
            tl = timed(dev, loop, 1) if not args.no_baseline else float("nan")
            pre[str(n)] = {"prefill_ms": round(tb * 1e3, 2), "prefill_tok_s": round(n / tb, 1),
                           "forward_loop_ms": round(tl * 1e3, 2), "forward_loop_tok_s": round(n / tl, 1),
                           "speedup": round(tl / tb, 2)}
        res["prefill"] = pre
    finally:
        eng.free(); m.free()

    # ---- decode batch
    m = rama_amd.Q8Model.synth(dev, Config(DIM, HIDDEN, LAYERS, 32, 32, VOCAB, 256, False), 64, 7)
    sizes = (8, 32) if args.quick else (1, 2, 4, 8, 16, 32, 64, 128)
    engs = [rama_amd.Q8Engine(dev, m) for _ in range(max(sizes))]
    engs[0].set_graph_mode(True)
    try:
        dec = {}
        for n in sizes:
            es = engs[:n]
            toks = [int(t) for t in rng.integers(0, VOCAB, n)]
            poss = [200 + (i * 7) % 40 for i in range(n)]

            tb = timed(dev, lambda: decode_batch(es, toks, poss), args.reps)
            # the baseline in rounds of at most 16 run states: the context keeps 16 Q8 graphs, so a longer loop would capture a
            # graph on every step; each round is warmed (its graphs captured) before it is timed
            tl = 0.0
            for r in range(0, n, 16):
                def loop(r=r):
                    for e, t, p in zip(es[r:r + 16], toks[r:r + 16], poss[r:r + 16]):
                        e.forward(t, p)
                tl += timed(dev, loop, 1) if not args.no_baseline else float("nan")
            nbytes, ops = product_model(n)
            dec[str(n)] = {"step_ms": round(tb * 1e3, 3), "tok_s": round(n / tb, 1),
                           "forward_loop_ms": round(tl * 1e3, 2), "forward_loop_tok_s": round(n / tl, 1),
                           "speedup": round(tl / tb, 2),
                           "step_bytes_over_8TBs": round(nbytes / tb / PEAK_BPS, 3), "step_i8_ops_over_peak": round(ops / tb / PEAK_I8_OPS, 4)}
        res["decode_batch"] = dec
    finally:
        for e in engs:
            e.free()
        m.free()

    head = res["prefill"]["512"]
    res.update(value=head["prefill_tok_s"], unit="tok/s")
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    dev.close()


if __name__ == "__main__":
    main()
