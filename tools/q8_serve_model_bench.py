#!/usr/bin/env python3
"""The serving chain with a draft model (rama_q8_serve_begin_model, Q8Server(draft=)) against the plain serving chain
BUILT FROM THE PARENT COMMIT.  The target is a llama2-7B-shaped rama_q8_model_synth model (group size 64, seq_len 512), the draft a
stories15M-shaped one with vocabulary 32 000 (group size 32); greedy, graph mode on.  n_slots requests (context 8, --new tokens each)
are submitted at once to a server of n_slots slots and max_rows rows and run to their end: 8 and 16 slots x 32 and 64 rows, K in 1, 2,
4 and 7, --reps repeats (after one untimed run), the spread reported.  Three legs:
 (parent) the plain Q8Server of the tree given by --parent-tree, in a child process that imports that tree's rama_amd and loads that
          tree's library -- the baseline; never this build's own plain chain;
 (a)      a second synthetic model as the draft: the two disagree, so next to nothing is accepted and a step pays K draft passes for
          one token per slot -- the per-step price of K draft passes;
 (b)      the target's own weights as the draft: every granted draft is accepted -- the upper bound on tokens per step (and an absurdly
          expensive drafter: its step time says nothing about a small draft model's).
From (a)'s ms per step and the parent's ms per step a line states the BREAK-EVEN: the tokens per slot-step the chain must emit to
match the parent, as accepted drafts per slot-step and as a fraction of K.  The acceptance of a real model pair is NOT measured: no
trained checkpoint pair is at hand.  Every leg's tokens are checked against the parent leg's.
Prints ONE JSON line per leg and configuration and, with --out, appends each to that file as it is measured.

Usage:  python tools/q8_serve_model_bench.py --parent-tree <a checkout of the parent commit, built> --out profiles/q8_serve_model_bench.jsonl
        [--reps 3] [--new 48] [--layers 32] [--slots 8,16] [--rows 32,64] [--ks 1,2,4,7]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(os.environ.get("RAMA_BENCH_TREE") or Path(__file__).resolve().parent.parent)
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

DIM, HIDDEN, VOCAB, SEQ = 4096, 11008, 32000, 512
DRAFT = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=VOCAB, seq_len=SEQ, shared_weight=True)
N_CTX = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--new", type=int, default=48, help="tokens produced per request")
    ap.add_argument("--layers", type=int, default=32, help="fewer target layers: a rehearsal")
    ap.add_argument("--slots", type=str, default="8,16")
    ap.add_argument("--rows", type=str, default="32,64")
    ap.add_argument("--ks", type=str, default="1,2,4,7")
    ap.add_argument("--parent-tree", type=str, default="", help="a built checkout of the parent commit: its plain chain is the baseline")
    ap.add_argument("--plain-leg", action="store_true", help="(the child process) the plain Q8Server of the tree this runs from, nothing else")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    slots, rows, ks = ([int(v) for v in s.split(",")] for s in (args.slots, args.rows, args.ks))

    def emit(line):
        print(json.dumps(line), flush=True)
        if args.out and not args.plain_leg:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    parent = {}
    if not args.plain_leg:
        if not args.parent_tree:
            raise SystemExit("--parent-tree: the baseline is the plain chain built from the parent commit, never this build's own")
        tree = Path(args.parent_tree).resolve()
        env = dict(os.environ, RAMA_BENCH_TREE=str(tree), RAMA_HIP_LIB=str(tree / "rama_amd" / "librama_hip.so"))
        cmd = [sys.executable, str(Path(__file__).resolve()), "--plain-leg", "--reps", str(args.reps), "--new", str(args.new), "--layers", str(args.layers),
               "--slots", args.slots, "--rows", args.rows]
        out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True).stdout
        for text in out.splitlines():
            line = json.loads(text)
            parent[(line["n_slots"], line["max_rows"])] = line
            emit({k: v for k, v in line.items() if k != "tokens"})      # (the tokens are for the check below, not for the record)

    import rama_amd
    from bench import library_stamp
    from oracle.oracle import Config
    from rama_amd._lib import check
    dev = rama_amd.Hip(0)
    name, cus, _ = dev.info()
    base = dict(device=name, compute_units=cus, group_size=64, draft_group_size=32, library=library_stamp(), n_layers=args.layers, seq_len=SEQ,
                draft_shape="stories15M, vocab 32000", graph_mode=True, new_tokens=args.new, n_context=N_CTX)
    m = rama_amd.Q8Model.synth(dev, Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, True), 64, 7)
    dm = None if args.plain_leg else rama_amd.Q8Model.synth(dev, Config(**DRAFT), 32, 8)
    check(dev.lib.rama_set_graph_mode(dev.ctx, 1))
    rng = np.random.default_rng(0)
    contexts = [[1] + [int(t) for t in rng.integers(2, VOCAB, N_CTX - 1)] for _ in range(max(slots))]

    def leg(n_slots, max_rows, **kw):
        """one server, the workload once untimed and --reps times timed -> (median, min, max seconds, steps, tokens, the last stats)"""
        srv = rama_amd.Q8Server(m, n_slots, max_rows, args.new, **kw)
        try:
            ts, toks, steps, st = [], None, 0, None
            for rep in range(args.reps + 1):
                before = srv.stats()["steps"]
                t0 = time.perf_counter()
                hs = [srv.submit(c, args.new) for c in contexts[:n_slots]]
                srv.run()
                check(dev.lib.rama_sync(dev.ctx))
                dt = time.perf_counter() - t0
                st = srv.stats()
                steps, toks = st["steps"] - before, [srv.result(h) for h in hs]
                if rep:
                    ts.append(dt)
            return statistics.median(ts), min(ts), max(ts), steps, toks, st
        finally:
            srv.close()

    try:
        for n_slots in slots:
            for max_rows in rows:
                n_tok = n_slots * args.new
                if args.plain_leg:
                    med, lo, hi, steps, toks, _ = leg(n_slots, max_rows)
                    emit(dict(base, metric=f"q8_serve_model_parent_plain_s{n_slots}_r{max_rows}", n_slots=n_slots, max_rows=max_rows, steps=steps,
                              tok_s=round(n_tok / med, 1), ms_per_step=round(med * 1e3 / steps, 4),
                              spread_ms_per_step=[round(lo * 1e3 / steps, 4), round(hi * 1e3 / steps, 4)], tokens=toks))
                    continue
                ref = parent[(n_slots, max_rows)]
                for K in ks:
                    for kind, draft in (("disagree", dm), ("self", m)):
                        med, lo, hi, steps, toks, st = leg(n_slots, max_rows, draft=draft, n_draft=K)
                        if toks != ref["tokens"]:
                            raise SystemExit(f"{kind} k{K} at {n_slots} x {max_rows}: the chain's tokens are not the parent's plain chain's")
                        sp = st["spec"]
                        dec = max(sum(sp["accepted_hist"]), 1)
                        ms_step = med * 1e3 / steps
                        line = dict(base, metric=f"q8_serve_model_{kind}_k{K}_s{n_slots}_r{max_rows}", n_slots=n_slots, max_rows=max_rows, n_draft=K,
                                    draft=kind, steps=steps, tok_s=round(n_tok / med, 1), ms_per_step=round(ms_step, 4),
                                    spread_ms_per_step=[round(lo * 1e3 / steps, 4), round(hi * 1e3 / steps, 4)],
                                    accepted_per_slot_step=round(sp["drafts_accepted"] / dec, 3), granted_per_slot_step=round(sp["drafts_granted"] / dec, 3),
                                    ms_per_step_parent=ref["ms_per_step"], tok_s_parent=ref["tok_s"], step_cost_vs_parent=round(ms_step / ref["ms_per_step"], 3))
                        if kind == "disagree":
                            need = ms_step / ref["ms_per_step"]           # tokens per slot-step that match the parent's one
                            line.update(break_even_accepted_per_slot_step=round(max(need - 1.0, 0.0), 3),
                                        break_even_acceptance=round(max(need - 1.0, 0.0) / K, 3), reachable=bool(need <= K + 1))
                        emit(line)
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        m.free()
        if dm is not None:
            dm.free()
        dev.close()


if __name__ == "__main__":
    main()
