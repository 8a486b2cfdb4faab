#!/usr/bin/env python3
"""Dot-plot block counts and bits (prf_dotplot_counts / prf_dotplot_bits) on the chr22-sized stand-in, resident in HBM
(prf_genome_standin, the contig of DESIGN 9.5): one JSON line per (mode, window, min_diagonal_run) with the HIP-event time of
the launches of several calls after a warm-up (median, minimum, maximum) and cells per second.  Counts over windows of 2^16 x
2^16 and 2^20 x 2^20 cells at t = 3 and 12 (block 4096), and 2^16 x 2^16 at t = 64, the costliest threshold; bits over 2^14 x
2^14.  Each measurement (its warm-up and timed calls together) runs in a child process of its own under a time limit, so that
one that takes too long ends alone and nothing is started behind it.  A window that the sequence would clip is refused.
The pair cases (prf_dotpair_counts / prf_dotpair_bits) are the four smaller self cases as calls of two ranges: A = B =
the contig, the same window, on the plus and on the minus strand; a fourth field of a case names the strand.
The runs cases (prf_dotpair_runs; the third field is min_len) count the runs of both directions that start in the same
2^16 x 2^16 window at min_len 11 and 32 on either strand, and -- runs-self -- all runs of 2^22 positions against themselves at
min_len 64, four calls of 2^20 rows each (a call takes at most 2^42 cells), which sends the trivial diagonal through the long
kernel.  They are counting calls (no destination): the time is the kernels', whatever the number of runs.
The chains cases (prf_dotpair_chains; the third field is min_seed, the fifth max_gap) count the chains that start in the
same 2^16 x 2^16 window at (11, 8) and (16, 64) on either strand, without a min_len, so that every head is a chain; the runs cases
at min_len 11 and 16 are their yardstick.  They report the seeds and the event times of the seed kernels and of the chain kernels.
The links cases (prf_dotpair_links; the sixth field is max_shift) count the junctions into the chains that start in the
same window at (11, 8, 4) and (16, 64, 32) on either strand; the chains cases are their yardstick.  The stand-in has almost no
diverged copies, so the join kernel mostly finds no candidate there: links-synth and chains-synth run the same calls on two
loaded sequences of 2^16 letters, the second a copy of the first with a base changed every 20 to 30 letters and a base inserted
or removed every 60 to 100, so that step B and the emission run.  They report the heads and the event times of the seed kernels
and of the heads and join kernels.

    python3 tools/dotplot_timing.py [--length 50818468] [--runs 7] [--warmup 2] [--limit 300] [--only counts:16:3,bits:14:3:-,chains:16:11:+:8,links:16:11:+:8:4,...]
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
RUNS_CASES = [("runs", 16, 11, "+"), ("runs", 16, 11, "-"), ("runs", 16, 32, "+"), ("runs", 16, 32, "-"), ("runs-self", 22, 64, "+")]
CHAINS_CASES = [case for strand in "+-" for case in (("runs", 16, 16, strand), ("chains", 16, 11, strand, 8), ("chains", 16, 16, strand, 64))]
LINKS_CASES = [case for strand in "+-" for case in (("links", 16, 11, strand, 8, 4), ("links", 16, 16, strand, 64, 32))]
LINKS_CASES += [("chains-synth", 16, 11, "+", 8), ("links-synth", 16, 11, "+", 8, 4), ("chains-synth", 16, 16, "+", 64), ("links-synth", 16, 16, "+", 64, 32)]
OFFSET = 30_000_000      # the window's first row and column: in the sequence, behind the stand-in's inner gap of N


def count_runs(genome, a, b, strand, min_len, rows, cols):
    """(runs, ScanStats) of one counting call of prf_dotpair_runs: both directions, no destination."""
    import ctypes
    import prf_native
    n, stats = ctypes.c_uint64(0), prf_native.ScanStats()
    lib = genome.ctx.lib
    prf_native._check(lib, lib.prf_dotpair_runs(genome.ctx._h, genome._h, a[0], a[1], a[2], b[0], b[1], b[2], prf_native.STRANDS[strand],
                                                rows[0], rows[1], cols[0], cols[1], 3, min_len, None, 0, ctypes.byref(n), ctypes.byref(stats)))
    return n.value, stats


def one_runs(args, genome, mode, side, min_len, strand):
    """The runs cases: the 2^16 window of the whole contig against itself, or a range of `side` positions against itself in
    calls of 2^20 rows."""
    whole = (0, 0, (1 << 64) - 1)
    if mode == "runs":
        a, windows = whole, [((OFFSET, OFFSET + side), (OFFSET, OFFSET + side))]
    else:
        a, windows = (0, OFFSET, OFFSET + side), [((r, r + (1 << 20)), (0, side)) for r in range(0, side, 1 << 20)]
    # a pass over 2^44 cells takes seconds: one warm-up and three timed passes there
    warmup, timed = (args.warmup, args.runs) if mode == "runs" else (min(args.warmup, 1), min(args.runs, 3))
    ms = []
    for i in range(warmup + timed):
        total_ms, launches, runs = 0.0, 0, 0
        for rows, cols in windows:
            n, stats = count_runs(genome, a, a, strand, min_len, rows, cols)
            total_ms, launches, runs = total_ms + stats.scan_ms, launches + stats.n_launches, runs + n
        if i >= warmup:
            ms.append(total_ms)
    med = statistics.median(ms)
    print(json.dumps({"mode": mode, "strand": strand, "rows": side, "cols": side, "min_len": min_len, "runs": timed, "calls": len(windows),
                      "launches": launches, "scan_ms_median": round(med, 4), "scan_ms_min": round(min(ms), 4), "scan_ms_max": round(max(ms), 4),
                      "cells_per_s": round(side * side / med * 1e3, 0), "n_runs": runs}), flush=True)


def one_chains(args, genome, side, min_seed, strand, max_gap):
    """The chains cases: counting calls (both directions, no destination, no min_len) on the 2^16 window of the whole contig
    against itself."""
    import ctypes
    import prf_native
    whole, window, lib = (0, 0, (1 << 64) - 1), (OFFSET, OFFSET + side), genome.ctx.lib
    ms, seeds_ms, chain_ms = [], [], []
    for i in range(args.warmup + args.runs):
        n, stats = ctypes.c_uint64(0), prf_native.ScanStats()
        prf_native._check(lib, lib.prf_dotpair_chains(genome.ctx._h, genome._h, *whole, *whole, prf_native.STRANDS[strand], *window, *window, 3,
                                                      min_seed, max_gap, 0, None, 0, ctypes.byref(n), ctypes.byref(stats)))
        if i >= args.warmup:
            ms.append(stats.scan_ms), seeds_ms.append(stats.phase1_ms), chain_ms.append(stats.phase2_ms)
    med = statistics.median(ms)
    print(json.dumps({"mode": "chains", "strand": strand, "rows": side, "cols": side, "min_seed": min_seed, "max_gap": max_gap, "runs": args.runs,
                      "launches": stats.n_launches, "scan_ms_median": round(med, 4), "scan_ms_min": round(min(ms), 4), "scan_ms_max": round(max(ms), 4),
                      "seed_kernels_ms_median": round(statistics.median(seeds_ms), 4), "chain_kernels_ms_median": round(statistics.median(chain_ms), 4),
                      "chain_kernels_ms_max": round(max(chain_ms), 4), "cells_per_s": round(side * side / med * 1e3, 0),
                      "n_seeds": stats.n_candidates, "n_heads": n.value, "n_chains": n.value}), flush=True)


def diverged_pair(side, seed):
    """Two sequences of `side` random letters (bytes): the second is the first with a base changed every 20 to 30 letters and a
    base inserted or removed every 60 to 100, cut to `side` letters."""
    import random
    rng = random.Random(seed)
    a = bytes(rng.choice(b"ACGT") for _ in range(side))
    b = bytearray(a)
    at = 0
    while at < len(b) - 30:
        at += rng.randrange(20, 31)
        b[at] = b"ACGT"[(b"ACGT".index(b[at]) + 1) % 4]
    out, at = bytearray(), 0
    while at < len(b):
        step = rng.randrange(60, 101)
        out += b[at:at + step]
        at += step
        if rng.random() < 0.5:
            out.append(rng.choice(b"ACGT"))
        else:
            at += 1
    return a, bytes(out[:side])


def one_links(args, genome, a, b, window, mode, min_seed, strand, max_gap, max_shift):
    """The links cases (max_shift set) and their chains yardstick on loaded sequences (max_shift None): counting calls, both
    directions, no destination."""
    import ctypes
    import prf_native
    lib, side = genome.ctx.lib, window[1] - window[0]
    ms, seeds_ms, rest_ms = [], [], []
    for i in range(args.warmup + args.runs):
        n, stats = ctypes.c_uint64(0), prf_native.ScanStats()
        head = (genome.ctx._h, genome._h, *a, *b, prf_native.STRANDS[strand], *window, *window, 3, min_seed, max_gap)
        if max_shift is None:
            prf_native._check(lib, lib.prf_dotpair_chains(*head, 0, None, 0, ctypes.byref(n), ctypes.byref(stats)))
        else:
            prf_native._check(lib, lib.prf_dotpair_links(*head, max_shift, None, 0, ctypes.byref(n), ctypes.byref(stats)))
        if i >= args.warmup:
            ms.append(stats.scan_ms), seeds_ms.append(stats.phase1_ms), rest_ms.append(stats.phase2_ms)
    med = statistics.median(ms)
    what = "chain_kernels" if max_shift is None else "link_kernels"
    print(json.dumps({"mode": mode, "strand": strand, "rows": side, "cols": side, "min_seed": min_seed, "max_gap": max_gap, "max_shift": max_shift,
                      "runs": args.runs, "launches": stats.n_launches, "scan_ms_median": round(med, 4), "scan_ms_min": round(min(ms), 4),
                      "scan_ms_max": round(max(ms), 4), "seed_kernels_ms_median": round(statistics.median(seeds_ms), 4),
                      f"{what}_ms_median": round(statistics.median(rest_ms), 4), f"{what}_ms_max": round(max(rest_ms), 4),
                      "cells_per_s": round(side * side / med * 1e3, 0), "n_seeds_or_heads": stats.n_candidates,
                      "n_chains" if max_shift is None else "n_links": n.value}), flush=True)


def one(args):
    import prf_native
    import synth  # noqa: F401
    mode, log2, t, strand, gap, shift = (args.case.split(":") + [None, None, None])[:6]
    side, t = 1 << int(log2), int(t)
    if mode.endswith("-synth"):
        ctx = prf_native.Context(0)
        genome = ctx.load(list(diverged_pair(side, args.seed)), 64)
        one_links(args, genome, (0, 0, side), (1, 0, side), (0, side), mode, t, strand, int(gap), None if shift is None else int(shift))
        genome.free()
        ctx.close()
        return
    if OFFSET + side > args.length:
        raise SystemExit(f"--length {args.length} is too short for a window of {side} positions from {OFFSET}")
    ctx = prf_native.Context(0)
    genome = ctx.standin([args.length], [args.seed], 64)
    if mode == "links":
        whole = (0, 0, (1 << 64) - 1)
        one_links(args, genome, whole, whole, (OFFSET, OFFSET + side), mode, t, strand, int(gap), int(shift))
        genome.free()
        ctx.close()
        return
    if mode.startswith("runs") or mode == "chains":
        one_runs(args, genome, mode, side, t, strand) if mode != "chains" else one_chains(args, genome, side, t, strand, int(gap))
        genome.free()
        ctx.close()
        return
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
    ap.add_argument("--case", help="(internal) mode:log2 side:min_diagonal_run[:strand[:max_gap[:max_shift]]] -- run this one measurement in this process")
    args = ap.parse_args()
    if args.case:
        return one(args)
    for case in [":".join(str(v) for v in c) for c in CASES + PAIR_CASES + RUNS_CASES + CHAINS_CASES + LINKS_CASES]:
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
