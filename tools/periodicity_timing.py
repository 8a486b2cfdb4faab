#!/usr/bin/env python3
"""Windowed period counts (prf_period_counts) on the chr22-sized stand-in, resident in HBM (prf_genome_standin, the
contig of DESIGN 9.5): one JSON line per (motif sizes, window) with the HIP-event kernel time of several calls after a warm-up
(median, minimum, maximum), cells per second, and the bytes of planes a launch stages into LDS against the 3 x len / 8
algorithmic bytes (computed from the launch shape: span 512 words, reach of the slice).

    python3 tools/periodicity_timing.py [--length 50818468] [--runs 7] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colab-repeat-finder_amd")]

import synth  # noqa: E402

SPAN_WORDS, KSLICE = 512, 2048     # csrc/periodicity.hip::prf_periodicity_shape for a genome of ACGTN


def staged_bytes(length, kmin, kmax):
    """Bytes of the three planes the workgroups of one launch read (both sides as one region where they touch)."""
    spans = -(-(-(-length // 64)) // SPAN_WORDS)
    total = 0
    for klo in range(kmin, kmax + 1, KSLICE):
        khi = min(kmax, klo + KSLICE - 1)
        a, b, apart = SPAN_WORDS + 1, SPAN_WORDS + 2 + (khi - klo) // 64, klo // 64
        total += spans * ((apart + b) if apart <= a else (a + b))
    return 3 * 8 * total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=synth.CHR22_LEN)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import prf_native
    ctx = prf_native.Context(0)
    genome = ctx.standin([args.length], [args.seed], 1000)
    for kmin, kmax in ((1, 50), (1, 1000)):
        for window in (1024, 65536):
            ms = []
            for i in range(args.warmup + args.runs):
                counts, stats = genome.period_counts(0, kmin, kmax, window, with_stats=True)
                if i >= args.warmup:
                    ms.append(stats.scan_ms)
            cells = args.length * (kmax - kmin + 1)
            med = statistics.median(ms)
            alg = 3 * args.length // 8
            print(json.dumps({"length": args.length, "kmin": kmin, "kmax": kmax, "window": window, "runs": args.runs,
                              "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
                              "cells_per_s": round(cells / med * 1e3, 0), "matches": int(counts.sum(dtype="uint64")),
                              "staged_bytes": staged_bytes(args.length, kmin, kmax), "algorithmic_bytes": alg,
                              "staged_over_algorithmic": round(staged_bytes(args.length, kmin, kmax) / alg, 3)}), flush=True)
    genome.free()
    ctx.close()


if __name__ == "__main__":
    main()
