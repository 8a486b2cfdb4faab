#!/usr/bin/env python3
"""Consensus motifs of gapped tandem repeats (prf_phased_consensus) on the chr22-sized stand-in, resident in HBM
(prf_genome_standin): one JSON line per case with the HIP-event time of the launches of several calls after a warm-up (median,
minimum, maximum).  Protocol of DESIGN 18.5: each case (its warm-up and timed calls together) runs in a child process of its own
under a time limit, so that one that takes too long ends alone and nothing is started behind it.

    groups:S:G:D   the gapped repeats of the whole contig (period_chains at min_len 0 and period_links at k = 1 .. kmax, min_seed S,
                   max_gap G, max_shift D; join_period_chains, tandem_groups), cut into phased segments by group_segments and named
                   by phased_consensus in batches that respect the limits; beside it, from the same process, the prf_period_links
                   call that found the links (a counting call) and prf_period_consensus on the same groups as plain
                   (start, end, period) rows; and the histogram of the work items' lengths

    python3 tools/phased_timing.py [--length 50818468] [--kmax 1000] [--runs 7] [--warmup 2] [--limit 500] [--only groups:12:8:4]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colab-repeat-finder_amd"), os.path.join(ROOT, "tools")]

CASES = ["groups:12:8:4"]
END = (1 << 64) - 1
EDGES = (1, 16, 32, 64, 128, 256, 1024, 4096)              # item lengths: up to each edge


def one(args, case):
    import numpy as np
    import prf_native
    from consensus_timing import summary, timed
    from plot_periodicity_matrix import consensus_batches, piece_batches
    _, s, gp, d = case.split(":")
    s, gp, d = int(s), int(gp), int(d)
    ctx = prf_native.Context(0)
    genome = ctx.standin([args.length], [22], max(args.kmax, 64))
    wall = time.perf_counter()
    chains = genome.period_chains(0, 0, None, 1, args.kmax, s, gp, 0)
    links = genome.period_links(0, 0, None, 1, args.kmax, s, gp, d)
    lists_ms = (time.perf_counter() - wall) * 1e3
    wall = time.perf_counter()
    joined = prf_native.join_period_chains(chains, links, with_paths=True)
    groups = joined[0]
    tandem, kept = prf_native.tandem_groups(groups, with_index=True)
    join_ms = (time.perf_counter() - wall) * 1e3
    wall = time.perf_counter()
    pieces, segments = prf_native.group_segments(chains, links, joined)
    keep = np.zeros(len(groups), dtype=bool)
    keep[kept] = True
    wanted = keep[pieces["group"].astype(np.int64)]
    new_row = np.cumsum(wanted) - 1
    pieces = pieces[wanted]
    segments = segments[wanted[segments["row"].astype(np.int64)]]
    segments["row"] = new_row[segments["row"].astype(np.int64)]
    segments_ms = (time.perf_counter() - wall) * 1e3
    lengths = (segments["end"] - segments["start"]).astype(np.int64)
    each = prf_native.CONSENSUS_SLICE                          # the items of the default slice: whole slices and what is left
    items = np.concatenate([np.full(int((lengths // each).sum()), each, dtype=np.int64), (lengths % each)[lengths % each > 0]])
    histogram = {f"<={edge}": int(((items <= edge) & (items > lo)).sum()) for lo, edge in zip((0,) + EDGES[:-1], EDGES)}
    out = {"case": case, "runs": args.runs, "length": args.length, "kmax": args.kmax, "n_chains": len(chains), "n_links": len(links),
           "n_groups": len(groups), "n_repeats": len(tandem), "n_pieces": len(pieces), "n_segments": len(segments),
           "positions": int(lengths.sum()), "letters": int(pieces["k"].sum()), "groups_with_several_pieces": int((np.bincount(pieces["group"].astype(np.int64)) > 1).sum()),
           "item_lengths": histogram, "item_length_median": float(np.median(items)) if len(items) else 0.0,
           "lists_wall_ms": round(lists_ms, 1), "join_wall_ms": round(join_ms, 1), "group_segments_wall_ms": round(segments_ms, 1)}
    seg0 = np.concatenate([[0], np.cumsum(pieces["segments"].astype(np.int64))])
    batches = list(piece_batches(pieces["k"].tolist(), pieces["segments"].tolist(), prf_native.CONSENSUS_MAX_ROWS, prf_native.CONSENSUS_MAX_LETTERS,
                                 prf_native.PHASED_MAX_SEGMENTS))
    parts = []
    for a, b in batches:
        part = segments[seg0[a]:seg0[b]].copy()
        part["row"] -= a
        parts.append((pieces["k"][a:b].copy(), part))
    name = lambda: [genome.phased_consensus(0, 0, None, ks, part, with_stats=True)[2] for ks, part in parts]   # noqa: E731
    ms, split, stats = timed(args, name)
    out.update(batches=len(batches), items=sum(int(st.n_candidates) for st in stats), launches=sum(int(st.n_launches) for st in stats), **summary("", ms, split))
    wall = time.perf_counter()
    name()
    out["call_wall_ms"] = round((time.perf_counter() - wall) * 1e3, 3)

    def find():
        n, st = ctypes.c_uint64(0), prf_native.ScanStats()
        prf_native._check(ctx.lib, ctx.lib.prf_period_links(ctx._h, genome._h, 0, 0, END, 0, END, 1, args.kmax, 0, s, gp, d, None, 0, ctypes.byref(n), ctypes.byref(st)))
        return [st]
    ms, split, _ = timed(args, find)
    out.update(**summary("links_", ms, split))
    plain = np.zeros(len(tandem), dtype=prf_native.REPEAT_DTYPE)
    plain["start"], plain["end"], plain["k"] = tandem["start"], tandem["end"], tandem["period"]
    flat = list(consensus_batches(plain["k"].tolist(), prf_native.CONSENSUS_MAX_ROWS, prf_native.CONSENSUS_MAX_LETTERS))
    ms, split, stats = timed(args, lambda: [genome.period_consensus(0, 0, None, plain[lo:hi], with_stats=True)[2] for lo, hi in flat])
    out.update(ungapped_items=sum(int(st.n_candidates) for st in stats), ungapped_positions=int((plain["end"] - plain["start"]).sum()), **summary("ungapped_", ms, split))
    out["names_over_links"] = round(out["scan_ms_median"] / max(out["links_scan_ms_median"], 1e-9), 4)
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
