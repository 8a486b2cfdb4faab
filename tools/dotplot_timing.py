#!/usr/bin/env python3
"""Dot-plot block counts and bits (prf_dotplot_counts / prf_dotplot_bits) on the chr22-sized stand-in, resident in HBM
(prf_genome_standin, the contig of DESIGN 9.5): one JSON line per (mode, window, min_diagonal_run) with the HIP-event time of
the launches of several calls after a warm-up (median, minimum, maximum) and cells per second.  Counts over windows of 2^16 x
2^16 and 2^20 x 2^20 cells at t = 3 and 12 (block 4096), and 2^16 x 2^16 at t = 64, the costliest threshold; bits over 2^14 x
2^14.  Each measurement (its warm-up and timed calls together) runs in a child process of its own under a time limit, so that
one that takes too long ends alone and nothing is started behind it.  A window that the sequence would clip is refused.
The pair cases (prf_dotpair_counts / prf_dotpair_bits) are the four smaller self cases as calls of two ranges: A = B =
the contig, the same window, on the plus and on the minus strand; a fourth field of a case names the strand.

    python3 tools/dotplot_timing.py [--length 50818468] [--runs 7] [--warmup 2] [--limit 300] [--only counts:16:3,bits:14:3:-,...]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colab-repeat-finder_amd")]

CASES = [("counts", 16, 3), ("counts", 16, 12), ("counts", 16, 64), ("counts", 20, 3), ("counts", 20, 12), ("bits", 14, 3),
         ("bits", 14, 12)]
PAIR_CASES = [(mode, log2, t, strand) for strand in "+-" for mode, log2, t in CASES if (mode, log2, t) in
              (("counts", 16, 3), ("counts", 16, 12), ("bits", 14, 3), ("bits", 14, 12))]
OFFSET = 30_000_000      # the window's first row and column: in the sequence, behind the stand-in's inner gap of N


def one(args):
    import prf_native
    import synth  # noqa: F401
    mode, log2, t, strand = (args.case.split(":") + [None])[:4]
    side, t = 1 << int(log2), int(t)
    if OFFSET + side > args.length:
        raise SystemExit(f"--length {args.length} is too short for a window of {side} positions from {OFFSET}")
    ctx = prf_native.Context(0)
    genome = ctx.standin([args.length], [args.seed], 64)
    window = (OFFSET, OFFSET + side)
    ms, launches, total = [], 0, 0
    for i in range(args.warmup + args.runs):
        if strand and mode == "counts":
            out, stats = genome.dotpair_counts((0, 0, None), (0, 0, None), 4096, strand, t, rows=window, cols=window, with_stats=True)
        elif strand:
            out, stats = genome.dotpair_bits((0, 0, None), (0, 0, None), strand, t, rows=window, cols=window, with_stats=True)
        elif mode == "counts":
            out, stats = genome.dotplot_counts(0, 4096, t, rows=window, cols=window, with_stats=True)
        else:
            out, stats = genome.dotplot_bits(0, t, rows=window, cols=window, with_stats=True)
        if i >= args.warmup:
            ms.append(stats.scan_ms)
        launches = stats.n_launches
    total = int(out.sum(dtype="uint64")) if mode == "counts" else None
    med = statistics.median(ms)
    print(json.dumps({"mode": mode, "strand": strand, "rows": side, "cols": side, "min_diagonal_run": t, "runs": args.runs, "launches": launches,
                      "scan_ms_median": round(med, 4), "scan_ms_min": round(min(ms), 4), "scan_ms_max": round(max(ms), 4),
                      "cells_per_s": round(side * side / med * 1e3, 0), "kept_cells": total}), flush=True)
    genome.free()
    ctx.close()


def main():
    import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=synth.CHR22_LEN)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds per measurement (warm-up and timed calls together)")
    ap.add_argument("--only", help="comma-separated measurements to make, e.g. counts:16:3,bits:14:12 (default: all)")
    ap.add_argument("--case", help="(internal) mode:log2 side:min_diagonal_run[:strand] -- run this one measurement in this process")
    args = ap.parse_args()
    if args.case:
        return one(args)
    for case in [":".join(str(v) for v in c) for c in CASES + PAIR_CASES]:
        mode, log2, t = case.split(":")[:3]
        if args.only and case not in args.only.split(","):
            continue
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", case,
               "--length", str(args.length), "--seed", str(args.seed), "--runs", str(args.runs), "--warmup", str(args.warmup)]
        rc = subprocess.call(cmd)
        if rc:                                    # a time limit or a fault: nothing more is started on the device
            print(json.dumps({"case": case, "mode": mode, "log2_side": log2, "min_diagonal_run": t, "exit_status": rc, "stopped": True}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
