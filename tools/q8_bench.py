#!/usr/bin/env python3
"""Q8_0 decode throughput: a llama2-7B-shaped rama_q8_model_synth model (group size 64), greedy, chained on the device
(rama_q8_generate), graph mode.  bench.py stays the fp32 yardstick; this prints ONE JSON line for the Q8 path.

A position range [a, b) is timed as the difference of two chained generations, 0..b and 0..a, each run after a settle
period of untimed decoding (bench.py's --settle-s idea), best of --reps: (t(b) - t(a)) / (b - a) is the cost of one step
at those positions, launch overhead and sampler included.

Usage:  python tools/q8_bench.py [--reps 3] [--settle-s 3] [--no-stories] [--no-long] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import rama_amd  # noqa: E402
from oracle.oracle import Config  # noqa: E402

PEAK_BPS = 8.0e12
SHAPES = {
    "llama2_7b": Config(4096, 11008, 32, 32, 32, 32000, 2048, False),
    "stories110M": Config(768, 2048, 12, 12, 12, 32000, 1024, True),
    "stories15M": Config(288, 768, 6, 6, 6, 32000, 256, True),
}


def gen_time(eng, steps: int) -> float:
    t = time.perf_counter()
    eng.generate([], steps)          # synchronises (downloads the tokens)
    return time.perf_counter() - t


def per_token(eng, a: int, b: int, reps: int, settle_s: float) -> float:
    t_end = time.perf_counter() + settle_s
    while time.perf_counter() < t_end:
        gen_time(eng, b)
    tb = min(gen_time(eng, b) for _ in range(reps))
    ta = min(gen_time(eng, a) for _ in range(reps)) if a else 0.0
    return (tb - ta) / (b - a)


def run_shape(dev, name, cfg, gs, reps, settle_s, ranges):
    m = rama_amd.Q8Model.synth(dev, cfg, gs, 7)
    eng = rama_amd.Q8Engine(dev, m)
    eng.set_graph_mode(True)
    try:
        out = {"bytes_per_token": m.bytes, "group_size": gs}
        for a, b in ranges:
            s = per_token(eng, a, b, reps, settle_s)
            out[f"pos_{a}_{b - 1}"] = {"ms_per_token": round(s * 1e3, 4), "tok_s": round(1.0 / s, 1),
                                       "roofline_frac": round(m.bytes / s / PEAK_BPS, 3)}
        return out
    finally:
        eng.free(); m.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settle-s", type=float, default=3.0)
    ap.add_argument("--no-stories", action="store_true")
    ap.add_argument("--no-long", action="store_true", help="skip positions 200, 1000 and 1900 at the 7B shape")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    dev = rama_amd.Hip(0)
    name, cus, hbm = dev.info()
    ranges = [(5, 25)] + ([] if args.no_long else [(200, 210), (1000, 1010), (1900, 1910)])
    res = {"metric": "q8_decode_tok_s_llama2_7b_pos5_24", "device": name, "compute_units": cus,
           "llama2_7b": run_shape(dev, "llama2_7b", SHAPES["llama2_7b"], 64, args.reps, args.settle_s, ranges)}
    if not args.no_stories:
        for n in ("stories110M", "stories15M"):
            gs = 64 if SHAPES[n].dim % 64 == 0 else 32
            res[n] = run_shape(dev, n, SHAPES[n], gs, args.reps, args.settle_s, [(5, 25)])
    head = res["llama2_7b"]["pos_5_24"]
    res.update(value=head["tok_s"], unit="tok/s", ms_per_token=head["ms_per_token"], roofline_frac=head["roofline_frac"],
               bytes_per_token=res["llama2_7b"]["bytes_per_token"])
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    dev.close()


if __name__ == "__main__":
    main()
