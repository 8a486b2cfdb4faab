#!/usr/bin/env python3
"""Consensus motifs (prf_period_consensus) on the chr22-sized stand-in, resident in HBM (prf_genome_standin): one JSON
line per case with the HIP-event time of the launches of several calls after a warm-up (median, minimum, maximum), the rows, the
work items and the launches.  Protocol of DESIGN 14.5: each case (its warm-up and timed calls together) runs in a child process
of its own under a time limit, so that one that takes too long ends alone and nothing is started behind it.

    names:S:G      the rows of tandem_rows(period_chains(k = 1 .. kmax, min_seed S, max_gap G)) of the whole contig, named in
                   batches that respect both limits; beside it, from the same process, the prf_period_chains calls that found
                   them (counting calls, as tools/periodchain_timing.py times them): whether naming costs a small fraction of finding
    array:K:P      one planted array of about 3 Mbp of period K (a substitution every 50 positions on average) in a sequence the
                   tool makes itself, one row, slice_positions P (0: the default): whether the guessed slice matters
    model:S:G      the first rows of the same list through the host model of the tests (tests/consensus_model.py), wall clock, for
                   the ratio only

    python3 tools/consensus_timing.py [--length 50818468] [--kmax 1000] [--runs 7] [--warmup 2] [--limit 300] [--only names:12:8]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colab-repeat-finder_amd")]

CASES = ["names:12:8", "array:171:0", "array:171:1024", "array:171:65536", "model:12:8"]
ARRAY = 3_000_000
END = (1 << 64) - 1
MODEL_ROWS = 2_000


def planted_array(k, n=ARRAY, seed=22):
    """(sequence, start, end, unit): random flanks of 10 000 positions around n // k copies of a random unit of k letters, with a
    substitution every 50 positions on average."""
    import random
    rng = random.Random(seed)
    unit = bytes(rng.choice(b"ACGT") for _ in range(k))
    body = bytearray(unit * (n // k))
    for _ in range(len(body) // 50):
        body[rng.randrange(len(body))] = rng.choice(b"ACGT")
    flank = bytes(rng.choice(b"ACGT") for _ in range(10_000))
    return flank + bytes(body) + flank, len(flank), len(flank) + len(body), unit.decode()


def timed(args, call):
    """The stats of args.runs calls behind args.warmup: (scan_ms list, (phase1, phase2) list, the last stats)."""
    ms, parts, stats = [], [], None
    for i in range(args.warmup + args.runs):
        stats = call()
        if i >= args.warmup:
            ms.append(sum(s.scan_ms for s in stats))
            parts.append((sum(s.phase1_ms for s in stats), sum(s.phase2_ms for s in stats)))
    return ms, parts, stats


def summary(prefix, ms, parts):
    return {f"{prefix}scan_ms_median": round(statistics.median(ms), 3), f"{prefix}scan_ms_min": round(min(ms), 3), f"{prefix}scan_ms_max": round(max(ms), 3),
            f"{prefix}phase1_ms_median": round(statistics.median(p[0] for p in parts), 3),
            f"{prefix}phase2_ms_median": round(statistics.median(p[1] for p in parts), 3)}


def tandem_of(ctx, genome, args, min_seed, max_gap):
    import prf_native
    chains = genome.period_chains(0, 0, None, 1, args.kmax, min_seed, max_gap)
    return chains, prf_native.tandem_rows(chains)


def one(args, case):
    import numpy as np
    import prf_native
    from plot_periodicity_matrix import consensus_batches
    mode, a, b = case.split(":")
    a, b = int(a), int(b)
    ctx = prf_native.Context(0)
    out = {"case": case, "runs": args.runs}
    if mode == "array":
        seq, start, end, unit = planted_array(a)
        genome = ctx.load([seq], 64)
        rows = np.array([(start, end, a, 0)], dtype=prf_native.REPEAT_DTYPE)
        ms, parts, stats = timed(args, lambda: [genome.period_consensus(0, 0, None, rows, with_stats=True, slice_positions=b)[2]])
        cons, motifs = genome.period_consensus(0, 0, None, rows, slice_positions=b)
        out.update(length=len(seq), k=a, slice_positions=b or prf_native.CONSENSUS_SLICE, positions=end - start, items=int(stats[0].n_candidates),
                   launches=int(stats[0].n_launches), consensus_identity=round(int(cons["agree"][0]) / (end - start), 4),
                   motif_is_the_unit=motifs[0] == unit, **summary("", ms, parts))
    else:
        genome = ctx.standin([args.length], [22], max(args.kmax, 64))
        chains, tandem = tandem_of(ctx, genome, args, a, b)
        out.update(length=args.length, kmax=args.kmax, n_chains=len(chains), n_rows=len(tandem), positions=int((tandem["end"] - tandem["start"]).sum()),
                   letters=int(tandem["k"].sum()))
        if mode == "names":
            def find():
                n, stats = ctypes.c_uint64(0), prf_native.ScanStats()
                prf_native._check(ctx.lib, ctx.lib.prf_period_chains(ctx._h, genome._h, 0, 0, END, 0, END, 1, args.kmax, 0, a, b, 0, None, 0,
                                                                     ctypes.byref(n), ctypes.byref(stats)))
                return [stats]
            batches = list(consensus_batches(tandem["k"].tolist(), prf_native.CONSENSUS_MAX_ROWS, prf_native.CONSENSUS_MAX_LETTERS))
            name = lambda: [genome.period_consensus(0, 0, None, tandem[lo:hi], with_stats=True)[2] for lo, hi in batches]   # noqa: E731
            ms, parts, stats = timed(args, name)
            out.update(batches=len(batches), items=sum(int(s.n_candidates) for s in stats), launches=sum(int(s.n_launches) for s in stats),
                       **summary("", ms, parts))
            wall = time.perf_counter()
            name()
            out["call_wall_ms"] = round((time.perf_counter() - wall) * 1e3, 3)   # with the item cutting, the copies and the binding
            ms, parts, _ = timed(args, find)
            out.update(**summary("chains_", ms, parts))
            out["names_over_chains"] = round(out["scan_ms_median"] / out["chains_scan_ms_median"], 4)
        else:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import consensus_model
            import synth
            sample = tandem[:MODEL_ROWS]
            stop = int(sample["end"].max()) if len(sample) else 0
            text = synth.standin2(args.length, 22, 0, stop).tobytes().decode("ascii")
            wall = time.perf_counter()
            want = consensus_model.consensus(text, sample)
            host_ms = (time.perf_counter() - wall) * 1e3
            got = genome.period_consensus(0, 0, None, sample, with_stats=True)
            out.update(sample_rows=len(sample), sample_positions=int((sample["end"] - sample["start"]).sum()), host_model_ms=round(host_ms, 3),
                       device_scan_ms=round(got[2].scan_ms, 3), same=bool(consensus_model.same(got[0], want[0]) and got[1] == want[1]))
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
