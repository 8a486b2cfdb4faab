#!/usr/bin/env python3
"""Alignments of tandem repeats to their motifs (prf_motif_align) on the chr22-sized stand-in, resident in HBM
(prf_genome_standin): one JSON line per case with the HIP-event time of the kernels of several calls after a warm-up (median,
minimum, maximum).  Protocol of DESIGN 18.5: each case (its warm-up and timed calls together) runs in a child process of its own
under a time limit, so that one that takes too long ends alone and nothing is started behind it.

    repeats:S:G    the diverged repeats of the whole contig (period_chains at k = 1 .. kmax, min_seed S, max_gap G; tandem_rows),
                   named by period_consensus and aligned to those motifs in one call; beside it, from the same process, the
                   consensus call on the same rows and the prf_period_chains call that found them (a counting call)
    groups:S:G:D   the gapped repeats (period_links with max_shift D on top; join_period_chains, tandem_groups), named by
                   phased_consensus; the whole [start, end) of each aligned to the motif of its chosen piece
    array:K        an array of 3 Mbp of period K with a substitution every 50 positions, cut into rows of 2^19 positions

Every case reports the cells (positions x k), cells per second, the split of rows, cells and time over the five kernels, and the
share of rows with k <= 16 and with at most 64 positions.

    python3 tools/align_timing.py [--length 50818468] [--kmax 1000] [--runs 7] [--warmup 2] [--limit 500] [--only repeats:12:8]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colab-repeat-finder_amd"), os.path.join(ROOT, "tools")]

CASES = ["repeats:12:8", "groups:12:8:4", "array:171"]
END = (1 << 64) - 1
REGIME_K = (64, 128, 256, 512, 1024)                        # the largest k of each kernel


def shape(rows):
    """What the next pull request needs to know of a row set: its split over the kernels and the share of small rows."""
    import numpy as np
    k, n = rows["k"].astype(np.int64), (rows["end"] - rows["start"]).astype(np.int64)
    regime = np.searchsorted(REGIME_K, k)
    per = {f"k<={edge}": {"rows": int((regime == r).sum()), "cells": int((k * n)[regime == r].sum()), "longest": int(n[regime == r].max(initial=0))}
           for r, edge in enumerate(REGIME_K)}
    return {"n_rows": len(rows), "positions": int(n.sum()), "cells": int((k * n).sum()), "letters": int(k.sum()), "per_kernel": per,
            "share_k<=16": round(float((k <= 16).mean()), 4) if len(rows) else 0.0, "share_n<=64": round(float((n <= 64).mean()), 4) if len(rows) else 0.0,
            "share_both": round(float(((k <= 16) & (n <= 64)).mean()), 4) if len(rows) else 0.0}


def per_kernel_ms(args, genome, rows, motifs):
    """The median kernel time of each kernel's rows alone."""
    import numpy as np
    from consensus_timing import timed
    import statistics
    regime = np.searchsorted(REGIME_K, rows["k"].astype(np.int64))
    out = {}
    for r, edge in enumerate(REGIME_K):
        at = np.flatnonzero(regime == r)
        if len(at):
            part, text = rows[at], [motifs[i] for i in at.tolist()]
            ms, _, _ = timed(args, lambda: [genome.motif_align(0, 0, None, part, text, with_stats=True)[1]])
            out[f"k<={edge}"] = round(statistics.median(ms), 3)
    return out


def one(args, case):
    import numpy as np
    import prf_native
    from consensus_timing import planted_array, summary, tandem_of, timed
    from plot_periodicity_matrix import consensus_batches, group_consensus_of
    mode, *numbers = case.split(":")
    numbers = [int(x) for x in numbers]
    ctx = prf_native.Context(0)
    out = {"case": case, "runs": args.runs}
    if mode == "array":
        k = numbers[0]
        seq, start, end, unit = planted_array(k)
        genome = ctx.load([seq], 64)
        cuts = list(range(start, end, prf_native.ALIGN_MAX_LEN)) + [end]
        rows = np.array([(a, b, k, 0) for a, b in zip(cuts, cuts[1:])], dtype=prf_native.REPEAT_DTYPE)
        motifs = [unit] * len(rows)
    else:
        genome = ctx.standin([args.length], [22], max(args.kmax, 64))
        s, gp = numbers[:2]
        if mode == "repeats":
            chains, tandem = tandem_of(ctx, genome, args, s, gp)
            batches = list(consensus_batches(tandem["k"].tolist(), prf_native.CONSENSUS_MAX_ROWS, prf_native.CONSENSUS_MAX_LETTERS))
            name = lambda: [genome.period_consensus(0, 0, None, tandem[lo:hi], with_stats=True) for lo, hi in batches]   # noqa: E731
            motifs = [m for part in name() for m in part[1]]
            rows = np.zeros(len(tandem), dtype=prf_native.REPEAT_DTYPE)
            rows["start"], rows["end"], rows["k"] = tandem["start"], tandem["end"], tandem["k"]
            ms, parts, _ = timed(args, lambda: [part[2] for part in name()])
            out.update(**summary("consensus_", ms, parts))

            def find():
                n, st = ctypes.c_uint64(0), prf_native.ScanStats()
                prf_native._check(ctx.lib, ctx.lib.prf_period_chains(ctx._h, genome._h, 0, 0, END, 0, END, 1, args.kmax, 0, s, gp, 0, None, 0,
                                                                     ctypes.byref(n), ctypes.byref(st)))
                return [st]
        else:
            d = numbers[2]
            chains = genome.period_chains(0, 0, None, 1, args.kmax, s, gp, 0)
            links = genome.period_links(0, 0, None, 1, args.kmax, s, gp, d)
            joined = prf_native.join_period_chains(chains, links, with_paths=True)
            tandem, kept = prf_native.tandem_groups(joined[0], with_index=True)
            keep = np.zeros(len(joined[0]), dtype=bool)
            keep[kept] = True
            named, names = group_consensus_of(genome, 0, None, joined, keep, chains, links)
            motifs = [names[at] for at in kept.tolist()]
            rows = np.zeros(len(tandem), dtype=prf_native.REPEAT_DTYPE)
            rows["start"], rows["end"], rows["k"] = tandem["start"], tandem["end"], [len(m) for m in motifs]

            def find():
                n, st = ctypes.c_uint64(0), prf_native.ScanStats()
                prf_native._check(ctx.lib, ctx.lib.prf_period_links(ctx._h, genome._h, 0, 0, END, 0, END, 1, args.kmax, 0, s, gp, d, None, 0,
                                                                    ctypes.byref(n), ctypes.byref(st)))
                return [st]
        fits = (rows["k"] >= 1) & (rows["k"] <= prf_native.ALIGN_MAX_K) & (rows["end"] - rows["start"] <= prf_native.ALIGN_MAX_LEN)
        out.update(length=args.length, kmax=args.kmax, above_a_limit=int((~fits).sum()))
        rows, motifs = rows[fits], [m for m, ok in zip(motifs, fits.tolist()) if ok]
        ms, parts, _ = timed(args, find)
        out.update(**summary("finding_", ms, parts))
    out.update(**shape(rows))
    ms, parts, stats = timed(args, lambda: [genome.motif_align(0, 0, None, rows, motifs, with_stats=True)[1]])
    got = prf_native.alignment_rows(rows, genome.motif_align(0, 0, None, rows, motifs))
    out.update(launches=int(stats[0].n_launches), **summary("", ms, parts))
    out["cells_per_second"] = round(out["cells"] / max(out["scan_ms_median"], 1e-9) * 1e3)
    out["rows_with_indels"] = int((got["ins"] + got["del"] > 0).sum())
    out["edits"], out["aligned_identity_mean"] = int(got["edits"].sum()), round(float(got["aligned_identity"].mean()), 4) if len(got) else 0.0
    if "finding_scan_ms_median" in out:
        out["align_over_finding"] = round(out["scan_ms_median"] / max(out["finding_scan_ms_median"], 1e-9), 4)
    out["per_kernel_ms"] = per_kernel_ms(args, genome, rows, motifs)
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
