#!/usr/bin/env python3
"""Preemption in both serving chains (Q8Server / Server(preempt=True)): what a stream of short urgent requests waits
for while every slot holds a long budget, with `preempt` off and on IN THE SAME BUILD.  The model is llama2-7B-shaped and synthetic
(Q8: rama_q8_model_synth, group size 64; fp32: rama_model_synth in parity mode), seq_len 256, greedy, graph mode on.  n_slots long
requests of priority 0 (contexts of 16 tokens, --long-new new tokens) fill every slot; once every one of them has produced --arrive-at
tokens, --urgent short requests of priority 1 (contexts of 16 tokens, --short-new new tokens) are submitted from the token callback,
one every --every tokens of the first long request.  Measured per configuration, --reps repeats after one untimed run, the spread
reported: the urgent requests' time to first token (submit -> its first token in the callback; median and max over them) and the
aggregate tok/s of the whole run; with preempt on also the preemptions.  Every request's tokens with preempt on are checked against
the same request's with preempt off.
Prints ONE JSON line per chain, slot count and preempt setting and, with --out, appends each to that file as it is measured.

Usage:  python tools/serve_preempt_bench.py --out profiles/serve_preempt_bench.jsonl
        [--reps 3] [--layers 32] [--slots 8,16] [--chains q8,f32] [--long-new 192] [--short-new 8] [--urgent 8] [--arrive-at 16] [--every 8]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

from q8_serve_bench import DIM, HIDDEN, SEQ, VOCAB  # noqa: E402  (serve_bench.py's shape)

CTX = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32, help="fewer layers: a rehearsal")
    ap.add_argument("--slots", type=str, default="8,16")
    ap.add_argument("--chains", type=str, default="q8,f32")
    ap.add_argument("--long-new", type=int, default=192)
    ap.add_argument("--short-new", type=int, default=8)
    ap.add_argument("--urgent", type=int, default=8)
    ap.add_argument("--arrive-at", type=int, default=16)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if CTX + args.long_new > SEQ:
        raise SystemExit(f"--long-new: {CTX} + {args.long_new} tokens beyond seq_len {SEQ}")

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    import numpy as np

    import rama_amd
    from bench import library_stamp
    from oracle.oracle import Config
    from rama_amd._lib import check
    from tests.helpers import to_rama_cfg
    cfg = to_rama_cfg(Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, False))
    rng = np.random.default_rng(3)
    ctx = lambda: [1] + [int(t) for t in rng.integers(2, VOCAB, CTX - 1)]

    for chain in args.chains.split(","):
        dev = rama_amd.Hip(0)
        if chain == "f32":
            check(dev.lib.rama_set_tuning(dev.ctx, b"ref_order", 1))
        name, cus, _ = dev.info()
        m = rama_amd.Q8Model.synth(dev, cfg, 64, 7) if chain == "q8" else rama_amd.Model.synth(dev, cfg, 7)
        cls = rama_amd.Q8Server if chain == "q8" else rama_amd.Server
        check(dev.lib.rama_set_graph_mode(dev.ctx, 1))
        try:
            for n_slots in (int(v) for v in args.slots.split(",")):
                longs, shorts = [ctx() for _ in range(n_slots)], [ctx() for _ in range(args.urgent)]
                tokens = {}
                for preempt in (False, True):
                    srv = cls(m, n_slots, max(n_slots, 32), args.long_new, preempt=preempt)
                    try:
                        walls, ttft_med, ttft_max, n_pre, toks = [], [], [], 0, None
                        for rep in range(args.reps + 1):
                            before = srv.stats()["preemptions"]
                            check(dev.lib.rama_sync(dev.ctx))
                            t0 = time.perf_counter()
                            hl = [srv.submit(c, args.long_new, priority=0) for c in longs]
                            hu, sent, first, count = [], {}, {}, {h: 0 for h in hl}

                            def on_token(h, i, t):
                                now = time.perf_counter()
                                if h in sent and h not in first:
                                    first[h] = now - sent[h]
                                if h in count:
                                    count[h] += 1
                                due = len(hu) < len(shorts) and min(count.values()) >= args.arrive_at and \
                                    count[hl[0]] >= args.arrive_at + args.every * len(hu)
                                if h == hl[0] and due:
                                    u = srv.submit(shorts[len(hu)], args.short_new, priority=1)
                                    sent[u] = time.perf_counter()
                                    hu.append(u)
                            srv.run(on_token)
                            while len(hu) < len(shorts):      # (the long requests ended before every urgent one was due)
                                u = srv.submit(shorts[len(hu)], args.short_new, priority=1)
                                sent[u] = time.perf_counter()
                                hu.append(u)
                                srv.run(on_token)
                            check(dev.lib.rama_sync(dev.ctx))
                            dt = time.perf_counter() - t0
                            toks = [srv.result(h) for h in hl + hu]
                            if rep:
                                walls.append(dt)
                                ttft_med.append(statistics.median(first[u] for u in hu))
                                ttft_max.append(max(first[u] for u in hu))
                                n_pre = srv.stats()["preemptions"] - before
                    finally:
                        srv.close()
                    tokens[preempt] = toks
                    if preempt and tokens[True] != tokens[False]:
                        raise SystemExit(f"{chain} at {n_slots} slots: the tokens with preempt on are not those with it off")
                    n_tok = sum(len(t) for t in toks)
                    med = statistics.median(walls)
                    emit(dict(metric=f"serve_preempt_{chain}_s{n_slots}_{'on' if preempt else 'off'}", chain=chain, device=name, compute_units=cus,
                              library=library_stamp(), n_layers=args.layers, seq_len=SEQ, graph_mode=True, n_slots=n_slots, preempt=preempt,
                              long_new=args.long_new, short_new=args.short_new, urgent=args.urgent, arrive_at=args.arrive_at, every=args.every,
                              generated_tokens=n_tok, unit="tok/s", tok_s=round(n_tok / med, 1), wall_s=round(med, 4),
                              wall_s_spread=[round(min(walls), 4), round(max(walls), 4)],
                              urgent_ttft_ms_median=round(statistics.median(ttft_med) * 1e3, 3),
                              urgent_ttft_ms_median_spread=[round(min(ttft_med) * 1e3, 3), round(max(ttft_med) * 1e3, 3)],
                              urgent_ttft_ms_max=round(statistics.median(ttft_max) * 1e3, 3),
                              urgent_ttft_ms_max_spread=[round(min(ttft_max) * 1e3, 3), round(max(ttft_max) * 1e3, 3)], preemptions=n_pre))
        finally:
            dev.lib.rama_set_graph_mode(dev.ctx, 0)
            m.free()
            dev.close()


if __name__ == "__main__":
    main()
