#!/usr/bin/env python3
"""The parity-mode serving chain with a Q8 draft model (rama_serve_begin_model, Server(draft=)) against the plain fp32
serving chain BUILT FROM THE PARENT COMMIT.  The target is a llama2-7B-shaped rama_model_synth model (fp32, seq_len 256, parity mode),
the draft a stories15M-shaped synthetic Q8 model with vocabulary 32 000 (group size 32); greedy, graph mode on.  The requests are
tools/serve_bench.py's mix (contexts of 16..128 tokens, 16..96 new tokens; --requests of them), submitted at once to a server of
n_slots slots and max_rows rows and run to their end: 8 and 16 slots x 32 and 64 rows, K in 1, 2, 4 and 7, --reps repeats (after one
untimed run), the spread reported.  Three legs:
 (parent) the plain Server of the tree given by --parent-tree, in a fresh child process that imports that tree's rama_amd and loads
          that tree's library -- the baseline; never this build's own plain chain;
 (a)      an unrelated synthetic Q8 model as the draft: next to nothing is accepted, so a step pays K draft passes for one token per
          decoding slot -- the per-step price of K draft passes;
 (b)      Q8Model.from_model(target) as the draft: the acceptance upper bound.  Its drafter streams a quarter of the target's bytes
          per pass: its step times say nothing about a small draft model's.
From (a)'s ms per step and the parent's a line states the BREAK-EVEN: the accepted drafts per decoding slot-step at which the chain
matches the parent (steps shrink as tokens per slot-step grow), and that as a fraction of K.  The acceptance of a trained model pair is
NOT measured: none is at hand.  Every leg's tokens are checked against the parent leg's.
Prints ONE JSON line per leg and configuration and, with --out, appends each to that file as it is measured.

Usage:  python tools/serve_model_bench.py --parent-tree <a checkout of the parent commit, built> --out profiles/serve_model_bench.jsonl
        [--reps 3] [--requests 32] [--layers 32] [--slots 8,16] [--rows 32,64] [--ks 1,2,4,7]
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
sys.path.insert(0, str(REPO / "tools"))

from q8_serve_bench import DIM, HIDDEN, NEW_RANGE, SEQ, VOCAB, workload  # noqa: E402  (serve_bench.py's request mix)

DRAFT = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=VOCAB, seq_len=SEQ, shared_weight=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--layers", type=int, default=32, help="fewer target layers: a rehearsal")
    ap.add_argument("--slots", type=str, default="8,16")
    ap.add_argument("--rows", type=str, default="32,64")
    ap.add_argument("--ks", type=str, default="1,2,4,7")
    ap.add_argument("--parent-tree", type=str, default="", help="a built checkout of the parent commit: its plain chain is the baseline")
    ap.add_argument("--plain-leg", action="store_true", help="(the child process) the plain Server of the tree this runs from, nothing else")
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
        cmd = [sys.executable, str(Path(__file__).resolve()), "--plain-leg", "--reps", str(args.reps), "--requests", str(args.requests), "--layers",
               str(args.layers), "--slots", args.slots, "--rows", args.rows]
        out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True).stdout
        for text in out.splitlines():
            line = json.loads(text)
            parent[(line["n_slots"], line["max_rows"])] = line
            emit({k: v for k, v in line.items() if k != "tokens"})      # (the tokens are for the check below, not for the record)

    import rama_amd
    from bench import library_stamp
    from oracle.oracle import Config
    from rama_amd._lib import check
    from tests.helpers import to_rama_cfg
    dev = rama_amd.Hip(0)
    check(dev.lib.rama_set_tuning(dev.ctx, b"ref_order", 1))
    name, cus, _ = dev.info()
    reqs = workload(args.requests)
    n_tok = sum(new for _, new in reqs)
    base = dict(device=name, compute_units=cus, dtype="f32 target (parity mode), Q8 draft", draft_group_size=32, library=library_stamp(),
                n_layers=args.layers, seq_len=SEQ, draft_shape="stories15M, vocab 32000", graph_mode=True, requests=len(reqs),
                generated_tokens=n_tok, unit="tok/s")
    m = rama_amd.Model.synth(dev, to_rama_cfg(Config(DIM, HIDDEN, args.layers, 32, 32, VOCAB, SEQ, False)), 7)
    drafts = {}
    if not args.plain_leg:
        drafts["disagree"] = rama_amd.Q8Model.synth(dev, to_rama_cfg(Config(**DRAFT)), 32, 8)
        drafts["self"] = rama_amd.Q8Model.from_model(m)
    check(dev.lib.rama_set_graph_mode(dev.ctx, 1))

    def leg(n_slots, max_rows, **kw):
        """one server, the workload once untimed and --reps times timed -> (median, min, max seconds, steps, tokens, the last stats)"""
        srv = rama_amd.Server(m, n_slots, max_rows, NEW_RANGE[1], **kw)
        try:
            ts, toks, steps, st = [], None, 0, None
            for rep in range(args.reps + 1):
                before = srv.stats()["steps"]
                check(dev.lib.rama_sync(dev.ctx))
                t0 = time.perf_counter()
                hs = [srv.submit(c, new) for c, new in reqs]
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
                if args.plain_leg:
                    med, lo, hi, steps, toks, _ = leg(n_slots, max_rows)
                    emit(dict(base, metric=f"serve_model_parent_plain_s{n_slots}_r{max_rows}", n_slots=n_slots, max_rows=max_rows, steps=steps,
                              tok_s=round(n_tok / med, 1), wall_s=round(med, 4), wall_s_spread=[round(lo, 4), round(hi, 4)],
                              ms_per_step=round(med * 1e3 / steps, 4), spread_ms_per_step=[round(lo * 1e3 / steps, 4), round(hi * 1e3 / steps, 4)],
                              tokens=toks))
                    continue
                ref = parent[(n_slots, max_rows)]
                for K in ks:
                    for kind, draft in drafts.items():
                        med, lo, hi, steps, toks, st = leg(n_slots, max_rows, draft=draft, n_draft=K)
                        if toks != ref["tokens"]:
                            raise SystemExit(f"{kind} k{K} at {n_slots} x {max_rows}: the chain's tokens are not the parent's plain chain's")
                        sp = st["spec"]
                        dec = max(sum(sp["accepted_hist"]), 1)      # decoding slot-steps that drafted, over the server's life (every run alike)
                        ms_step = med * 1e3 / steps
                        line = dict(base, metric=f"serve_model_{kind}_k{K}_s{n_slots}_r{max_rows}", n_slots=n_slots, max_rows=max_rows, n_draft=K,
                                    draft=kind, draft_group_size=draft.group_size, steps=steps, tok_s=round(n_tok / med, 1), wall_s=round(med, 4),
                                    wall_s_spread=[round(lo, 4), round(hi, 4)], ms_per_step=round(ms_step, 4),
                                    spread_ms_per_step=[round(lo * 1e3 / steps, 4), round(hi * 1e3 / steps, 4)],
                                    accepted_per_slot_step=round(sp["drafts_accepted"] / dec, 3), granted_per_slot_step=round(sp["drafts_granted"] / dec, 3),
                                    ms_per_step_parent=ref["ms_per_step"], steps_parent=ref["steps"], tok_s_parent=ref["tok_s"],
                                    step_cost_vs_parent=round(ms_step / ref["ms_per_step"], 3), speed_vs_parent=round(ref["wall_s"] / med, 3))
                        if kind == "disagree":
                            need = ms_step / ref["ms_per_step"]           # tokens per decoding slot-step that match the parent's one
                            line.update(break_even_accepted_per_slot_step=round(max(need - 1.0, 0.0), 3),
                                        break_even_acceptance=round(max(need - 1.0, 0.0) / K, 3), reachable=bool(need <= K + 1))
                        emit(line)
    finally:
        dev.lib.rama_set_graph_mode(dev.ctx, 0)
        for d in drafts.values():
            d.free()
        m.free()
        dev.close()


if __name__ == "__main__":
    main()
