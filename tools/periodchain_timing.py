#!/usr/bin/env python3
"""Chains on the period lines (prf_period_chains) on the chr22-sized stand-in, resident in HBM (prf_genome_standin):
one JSON line per case with the HIP-event time of the launches of several calls after a warm-up (median, minimum, maximum), the
seeds, the chains and the launches.  Protocol of DESIGN 14.5: each case (its warm-up and timed calls together) runs in a child
process of its own under a time limit, so that one that takes too long ends alone and nothing is started behind it.

    chains:S:G     the whole contig as range and window, k = 1 .. kmax, n_matches 0, min_seed S, max_gap G; a counting call
    counts         the yardstick: prf_period_counts over the same range and k with a window of 65 536 -- the same cells
    chains16:S:G   a range of 2^16 positions (from 30 000 000), k = 1 .. kmax, n_matches 1
    band16:S:G     the same band through prf_dotpair_chains(A, A, +, main): the window of 2^16 x 2^16 cells that holds it, which
                   is what covered it before; it lists the other diagonals of the window too
    links:S:G:D    the junctions between those chains (prf_period_links), max_shift D: the whole contig as range and
                   window, k = 1 .. kmax, n_matches 0, a counting call; phase1 = the find and the long kernel, phase2 = the join
    dense:S:G:D    the same on a sequence the tool makes itself (dense_vntrs): 2^20 positions of tandem repeats with planted
                   substitutions and indels, so that most heads have candidates and many lanes of the join kernel walk
    densechains:S:G   prf_period_chains, counting, on that sequence: what the links' phase1 repeats

    python3 tools/periodchain_timing.py [--length 50818468] [--kmax 1000] [--runs 7] [--warmup 2] [--limit 300] [--only chains:12:8,counts]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colab-repeat-finder_amd")]

CASES = ["chains:12:8", "chains:16:64", "counts", "chains16:12:8", "chains16:16:64", "band16:12:8", "band16:16:64",
         "links:12:8:4", "links:16:64:8", "densechains:12:8", "dense:12:8:4", "densechains:16:64", "dense:16:64:8"]
DENSE = 1 << 20
OFFSET, SIDE = 30_000_000, 1 << 16
END = (1 << 64) - 1


def dense_vntrs(n=DENSE, seed=22):
    """n positions of tandem repeats between short random flanks: units of 12 .. 60 random letters, 6 .. 20 copies, a substitution
    every 50 positions on average and an insertion or a deletion of 1 .. 3 letters every 150."""
    import random
    rng, out = random.Random(seed), bytearray()
    while len(out) < n:
        out += bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(50, 200)))
        unit = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(12, 61)))
        body = bytearray(unit * rng.randrange(6, 21))
        for _ in range(len(body) // 50):
            at = rng.randrange(len(body))
            body[at] = rng.choice(b"ACGT")
        for _ in range(len(body) // 150):
            at, d = rng.randrange(len(body)), rng.randrange(1, 4)
            if rng.random() < 0.5:
                body[at:at] = bytes(rng.choice(b"ACGT") for _ in range(d))
            else:
                del body[at:at + d]
        out += body
    return bytes(out[:n])


def one(args, case):
    import prf_native
    mode, *rest = case.split(":")
    min_seed, max_gap, max_shift = ([int(v) for v in rest] + [0, 0, 0])[:3]
    ctx = prf_native.Context(0)
    dense = mode in ("dense", "densechains")
    genome = ctx.load([dense_vntrs()], 64) if dense else ctx.standin([args.length], [22], max(args.kmax, 64))
    lib, ms, parts = ctx.lib, [], []
    out = {"case": case, "length": DENSE if dense else args.length, "kmax": args.kmax, "runs": args.runs}
    if mode == "counts":
        import numpy as np
        dst = np.zeros(args.kmax * (-(-args.length // 65_536)), dtype=np.uint32)
    for i in range(args.warmup + args.runs):
        n, stats = ctypes.c_uint64(0), prf_native.ScanStats()
        if mode in ("links", "dense"):
            prf_native._check(lib, lib.prf_period_links(ctx._h, genome._h, 0, 0, END, 0, END, 1, args.kmax, 0, min_seed, max_gap, max_shift, None, 0,
                                                        ctypes.byref(n), ctypes.byref(stats)))
            total, launches, found, seeds = stats.scan_ms, stats.n_launches, n.value, stats.n_candidates       # links, chain heads
            part = (stats.phase1_ms, stats.phase2_ms)
        elif mode in ("chains", "densechains"):
            prf_native._check(lib, lib.prf_period_chains(ctx._h, genome._h, 0, 0, END, 0, END, 1, args.kmax, 0, min_seed, max_gap, 0, None, 0,
                                                         ctypes.byref(n), ctypes.byref(stats)))
            total, launches, found, seeds = stats.scan_ms, stats.n_launches, n.value, stats.n_candidates
            part = (stats.phase1_ms, stats.phase2_ms)
        elif mode == "chains16":
            prf_native._check(lib, lib.prf_period_chains(ctx._h, genome._h, 0, OFFSET, OFFSET + SIDE, 0, END, 1, args.kmax, 1, min_seed, max_gap, 0,
                                                         None, 0, ctypes.byref(n), ctypes.byref(stats)))
            total, launches, found, seeds = stats.scan_ms, stats.n_launches, n.value, stats.n_candidates
            part = (stats.phase1_ms, stats.phase2_ms)
        elif mode == "band16":
            span = (0, OFFSET, OFFSET + SIDE)
            prf_native._check(lib, lib.prf_dotpair_chains(ctx._h, genome._h, *span, *span, 0, 0, SIDE, 0, SIDE, 1, min_seed, max_gap, 0, None, 0,
                                                          ctypes.byref(n), ctypes.byref(stats)))
            total, launches, found, seeds = stats.scan_ms, stats.n_launches, n.value, stats.n_candidates
            part = (stats.phase1_ms, stats.phase2_ms)
        else:
            prf_native._check(lib, lib.prf_period_counts(ctx._h, genome._h, 0, 0, END, 1, args.kmax, 65_536, dst.ctypes.data, len(dst), ctypes.byref(n),
                                                         ctypes.byref(stats)))
            total, launches, found, seeds, part = stats.scan_ms, stats.n_launches, 0, 0, (stats.scan_ms, 0.0)
        if i >= args.warmup:
            ms.append(total), parts.append(part)
    med = statistics.median(ms)
    out.update(launches=launches, scan_ms_median=round(med, 3), scan_ms_min=round(min(ms), 3), scan_ms_max=round(max(ms), 3),
               phase1_ms_median=round(statistics.median(p[0] for p in parts), 3), phase2_ms_median=round(statistics.median(p[1] for p in parts), 3),
               n_seeds=seeds, n_chains=found)
    if mode in ("links", "dense"):
        out["n_heads"], out["n_links"] = out.pop("n_seeds"), out.pop("n_chains")
    print(json.dumps(out), flush=True)
    genome.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--length", type=int, default=50_818_468)
    ap.add_argument("--kmax", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take")
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
