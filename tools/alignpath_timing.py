#!/usr/bin/env python3
"""Alignments with their paths (prf_motif_align_path) beside prf_motif_align on the same rows of the same build, on the
chr22-sized stand-in resident in HBM: one JSON line per case with the HIP-event times of several calls after a warm-up (median,
minimum, maximum).  Protocol of DESIGN 18.5: each case (its warm-up and timed calls together) runs in a child process of its own
under a time limit, so that one that takes too long ends alone and nothing is started behind it.

    repeats:S:G    the diverged repeats of the whole contig (period_chains at k = 1 .. kmax, min_seed S, max_gap G; tandem_rows),
                   named by period_consensus: the forward kernels (phase 1), the walk and the counts (phase 2) and the whole
                   call, beside prf_motif_align; the ratio forward / align is the cost of the trace's stores; and how many rows
                   change their motif under two rounds of refine_motifs
    row:K          one row of 2^19 positions of the perfect repetition of a random motif of K letters

    python3 tools/alignpath_timing.py [--length 50818468] [--kmax 1000] [--runs 7] [--warmup 2] [--limit 500] [--only row:1024]
"""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colab-repeat-finder_amd"), os.path.join(ROOT, "tools")]

CASES = ["repeats:12:8", "row:1024", "row:1"]


def one(args, case):
    import numpy as np
    import prf_native
    from align_timing import shape
    from consensus_timing import summary, tandem_of, timed
    from plot_periodicity_matrix import consensus_batches
    mode, *numbers = case.split(":")
    numbers = [int(x) for x in numbers]
    ctx = prf_native.Context(0)
    out = {"case": case, "runs": args.runs}
    if mode == "row":
        k, n, rng = numbers[0], prf_native.ALIGN_MAX_LEN, random.Random(21)
        unit = "".join(rng.choice("ACGT") for _ in range(k))
        genome = ctx.load([("GATTACA" + unit * (n // k + 1))[:n + 7].encode()], 64)
        rows = np.array([(7, 7 + n, k, 0)], dtype=prf_native.REPEAT_DTYPE)
        motifs = [unit]
    else:
        genome = ctx.standin([args.length], [22], max(args.kmax, 64))
        _, tandem = tandem_of(ctx, genome, args, *numbers[:2])
        motifs = [m for lo, hi in consensus_batches(tandem["k"].tolist(), prf_native.CONSENSUS_MAX_ROWS, prf_native.CONSENSUS_MAX_LETTERS)
                  for m in genome.period_consensus(0, 0, None, tandem[lo:hi])[1]]
        rows = np.zeros(len(tandem), dtype=prf_native.REPEAT_DTYPE)
        rows["start"], rows["end"], rows["k"] = tandem["start"], tandem["end"], tandem["k"]
        fits = (rows["k"] <= prf_native.ALIGN_MAX_K) & (rows["end"] - rows["start"] <= prf_native.ALIGN_MAX_LEN)
        rows, motifs = rows[fits], [m for m, ok in zip(motifs, fits.tolist()) if ok]
        out.update(length=args.length, kmax=args.kmax)
    out.update(**shape(rows))
    ms, parts, _ = timed(args, lambda: [genome.motif_align(0, 0, None, rows, motifs, with_stats=True)[1]])
    out.update(**summary("align_", ms, parts))
    ms, parts, stats = timed(args, lambda: [genome.motif_align_path(0, 0, None, rows, motifs, with_counts=True, with_stats=True)[3]])
    out.update(launches=int(stats[0].n_launches), **summary("", ms, parts))
    out["forward_over_align"] = round(out["phase1_ms_median"] / max(out["align_scan_ms_median"], 1e-9), 4)
    out["path_over_align"] = round(out["scan_ms_median"] / max(out["align_scan_ms_median"], 1e-9), 4)
    if mode == "repeats":
        _, _, changed = prf_native.refine_motifs(genome, 0, 0, None, rows, motifs, rounds=2)
        out["rows_refined"] = int((changed > 0).sum())
    print(json.dumps(out), flush=True)
    genome.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--length", type=int, default=50_818_468)
    ap.add_argument("--kmax", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=500, help="seconds a case may take")
    ap.add_argument("--only", help="comma-separated cases")
    ap.add_argument("--case", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:
        return one(args, args.case)
    for case in (args.only.split(",") if args.only else CASES):
        try:
            code = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--length", str(args.length), "--kmax", str(args.kmax),
                                   "--runs", str(args.runs), "--warmup", str(args.warmup)], timeout=args.limit, check=False).returncode
        except subprocess.TimeoutExpired:
            code = 124
        if code:                                 # a case that failed or ran out of time ends the series: nothing is started behind it
            print(json.dumps({"case": case, "returncode": code}), flush=True)
            return code
    return 0


if __name__ == "__main__":
    sys.exit(main())
