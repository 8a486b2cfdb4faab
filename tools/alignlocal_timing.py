#!/usr/bin/env python3
"""Local alignments of windows around tandem repeats to their motifs (prf_motif_align_local) on the chr22-sized
stand-in, resident in HBM (prf_genome_standin): one JSON line per case with the HIP-event time of the kernels of several calls after
a warm-up (median, minimum, maximum).  Protocol of DESIGN 18.5: each case (its warm-up and timed calls together) runs in a child
process of its own under a time limit, so that one that takes too long ends alone and nothing is started behind it.

    repeats:S:G:F  the diverged repeats of the whole contig (period_chains at k = 1 .. kmax, min_seed S, max_gap G; tandem_rows),
                   named by period_consensus, padded by F positions (flank_repeats) and aligned locally to those motifs in one
                   call at the weights of --weights
    row:K          one window of 2^19 positions, the limit, of an array of period K with a substitution every 50 positions

THE YARDSTICK: beside each, from the same process of the same build, prf_motif_align (unit costs, global) on the same
rows.  Every case reports the ratio of the two, the cells (positions x k), and the split of rows, cells and both times over the
five kernels.

    python3 tools/alignlocal_timing.py [--length 50818468] [--kmax 1000] [--runs 7] [--warmup 2] [--limit 500] [--weights 2,7,7] [--only row:1024]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colab-repeat-finder_amd"), os.path.join(ROOT, "tools")]

CASES = ["repeats:12:8:50", "row:1024"]


def per_kernel(args, genome, rows, motifs, weights):
    """Per kernel: its rows, cells and longest row, and the median kernel time of both products on those rows alone."""
    import numpy as np
    from align_timing import REGIME_K
    from consensus_timing import timed
    k, n = rows["k"].astype(np.int64), (rows["end"] - rows["start"]).astype(np.int64)
    regime = np.searchsorted(REGIME_K, k)
    out = {}
    for r, edge in enumerate(REGIME_K):
        at = np.flatnonzero(regime == r)
        if not len(at):
            continue
        part, text = rows[at], [motifs[i] for i in at.tolist()]
        local, _, _ = timed(args, lambda: [genome.motif_align_local(0, 0, None, part, text, *weights, with_stats=True)[1]])
        plain, _, _ = timed(args, lambda: [genome.motif_align(0, 0, None, part, text, with_stats=True)[1]])
        out[f"k<={edge}"] = {"rows": len(at), "cells": int((k * n)[at].sum()), "longest": int(n[at].max()), "local_ms": round(statistics.median(local), 3),
                             "align_ms": round(statistics.median(plain), 3), "ratio": round(statistics.median(local) / max(statistics.median(plain), 1e-9), 3)}
    return out


def one(args, case):
    import numpy as np
    import prf_native
    from consensus_timing import planted_array, summary, tandem_of, timed
    from plot_periodicity_matrix import consensus_batches
    weights = tuple(int(w) for w in args.weights.split(","))
    mode, *numbers = case.split(":")
    numbers = [int(x) for x in numbers]
    ctx = prf_native.Context(0)
    out = {"case": case, "runs": args.runs, "weights": list(weights)}
    if mode == "row":
        k = numbers[0]
        seq, start, end, unit = planted_array(k)
        genome = ctx.load([seq], 64)
        first = start - 50                                                     # a flank of 50 in front; the array goes on behind
        rows = np.array([(first, first + prf_native.ALIGN_MAX_LEN, k, 0)], dtype=prf_native.REPEAT_DTYPE)
        motifs = [unit]
    else:
        genome = ctx.standin([args.length], [22], max(args.kmax, 64))
        s, gp, flank = numbers
        _chains, tandem = tandem_of(ctx, genome, args, s, gp)
        batches = list(consensus_batches(tandem["k"].tolist(), prf_native.CONSENSUS_MAX_ROWS, prf_native.CONSENSUS_MAX_LETTERS))
        motifs = [m for lo, hi in batches for m in genome.period_consensus(0, 0, None, tandem[lo:hi])[1]]
        rows, sent = prf_native.flank_repeats(tandem, flank, args.length)
        out.update(length=args.length, kmax=args.kmax, flank=flank, above_a_limit=int((~sent).sum()))
        rows, motifs = rows[sent], [m for m, ok in zip(motifs, sent.tolist()) if ok]
    k, n = rows["k"].astype(np.int64), (rows["end"] - rows["start"]).astype(np.int64)
    out.update(n_rows=len(rows), positions=int(n.sum()), cells=int((k * n).sum()))
    ms, parts, stats = timed(args, lambda: [genome.motif_align_local(0, 0, None, rows, motifs, *weights, with_stats=True)[1]])
    out.update(launches=int(stats[0].n_launches), **summary("", ms, parts))
    plain, plain_parts, _ = timed(args, lambda: [genome.motif_align(0, 0, None, rows, motifs, with_stats=True)[1]])
    out.update(**summary("align_", plain, plain_parts))
    out["local_over_align"] = round(out["scan_ms_median"] / max(out["align_scan_ms_median"], 1e-9), 3)
    out["cells_per_second"] = round(out["cells"] / max(out["scan_ms_median"], 1e-9) * 1e3)
    got = genome.motif_align_local(0, 0, None, rows, motifs, *weights)
    out["rows_with_a_score"] = int((got["score"] > 0).sum())
    out["rows_trimmed_or_kept_short"] = int(((got["end"] - got["first"]).astype(np.int64) < n).sum())
    out["score_sum"] = int(got["score"].sum(dtype=np.int64))
    out["per_kernel"] = per_kernel(args, genome, rows, motifs, weights)
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
    ap.add_argument("--weights", default="2,7,7", help="match,mismatch,indel")
    ap.add_argument("--only", help="comma-separated cases")
    ap.add_argument("--case", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.case:
        return one(args, args.case)
    for case in (args.only.split(",") if args.only else CASES):
        try:
            code = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--length", str(args.length), "--kmax", str(args.kmax),
                                   "--runs", str(args.runs), "--warmup", str(args.warmup), "--weights", args.weights], timeout=args.limit,
                                  check=False).returncode
        except subprocess.TimeoutExpired:
            code = 124
        if code:                                 # a case that failed or ran out of time ends the series: nothing is started behind it
            print(json.dumps({"case": case, "returncode": code}), flush=True)
            return code
    return 0


if __name__ == "__main__":
    sys.exit(main())
