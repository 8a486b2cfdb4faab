#!/usr/bin/env python3
"""Write tests/golden/interrupted.jsonl.gz: interrupted-repeat cases run through the REFERENCE's RepeatTracker.

The reference has no driver for RepeatTracker (its perfect_repeat_finder.py drives PerfectRepeatTracker only), so this tool
runs the driver the project pins: upper-case, N-trimming of the whole sequence (reference perfect_repeat_finder.py
:35-46), one RepeatTracker(k, min_repeats, min_span, max_interruptions, seq, out) per k = kmin .. kmax in ascending order with
ONE shared dict, `while t.advance(): pass; t.done()`, rows = sorted(out.items()) shifted by the trimmed head.

    python3 tools/gen_interrupted_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--cases 3200] [--seed 9]

Each line: {"tag", "seq", "settings": {min_motif_size, max_motif_size, min_repeats, min_span, max_interruptions},
"rows": [[start, end, motif], ...]} -- the motif with N at the phases that were allowed to vary.
"""
import argparse
import gzip
import json
import os
import random
import sys

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "interrupted.jsonl.gz")


def reference_rows(RepeatTracker, seq, kmin, kmax, min_repeats, min_span, max_interruptions):
    s = seq.upper()
    lo, hi = 0, len(s)
    while lo < hi and s[lo] == "N":
        lo += 1
    while hi > lo and s[hi - 1] == "N":
        hi -= 1
    s = s[lo:hi]
    out = {}
    for k in range(kmin, kmax + 1):
        t = RepeatTracker(motif_size=k, min_repeats=min_repeats, min_span=min_span, max_interruptions=max_interruptions,
                          input_sequence=s, output_intervals=out)
        while t.advance():
            pass
        t.done()
    return [[a + lo, b + lo, m] for (a, b), m in sorted(out.items())]


def planted(rng, unit_len, copies, n_changes, alphabet="ACGT"):
    unit = "".join(rng.choice(alphabet) for _ in range(unit_len))
    rep = list(unit * copies)
    for _ in range(n_changes):
        if rep:
            rep[rng.randrange(len(rep))] = rng.choice(alphabet)
    return "".join(rep)


def random_seq(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


# settings come from a small palette, so that a test can hand all cases of one setting to one call
SMALL_K = [(1, 6), (2, 8)]
LARGE_K = [(16, 64)]
THRESHOLDS = [(2, 5), (3, 9)]


def make_case(rng, i):
    kind = ["random", "planted", "homopolymer", "n_iupac", "lower", "large_k", "absorbing", "n_ends", "dense"][i % 9]
    m = rng.randint(1, 3)
    kmin, kmax = rng.choice(LARGE_K if kind == "large_k" else SMALL_K)
    r, span = rng.choice(THRESHOLDS)
    if kind == "random":                      # back-jumps and the stale phase set on plain random sequence
        seq = random_seq(rng, rng.choice([50, 200, 600]), "ACGT")
    elif kind == "planted":                   # interrupted repeats in random flanks: dict precedence, the previous-output rule
        parts = [random_seq(rng, rng.randint(0, 40), "ACGT")]
        for _ in range(rng.randint(1, 4)):
            parts.append(planted(rng, rng.randint(1, 8), rng.randint(2, 14), rng.randint(0, 4)))
            parts.append(random_seq(rng, rng.randint(0, 30), "ACGT"))
        seq = "".join(parts)
    elif kind == "homopolymer":               # AAAC-like units: motifs that are a homopolymer once the varying phases are N
        base = rng.choice("ACGT")
        unit = [base] * rng.randint(2, 7)
        unit[rng.randrange(len(unit))] = rng.choice("ACGT")
        seq = random_seq(rng, rng.randint(0, 20), "ACGT") + "".join(unit) * rng.randint(2, 10) + random_seq(rng, rng.randint(0, 20), "ACGT")
    elif kind == "n_iupac":                   # N inside runs (N == N is a match here) and other letters as ordinary symbols
        seq = random_seq(rng, rng.choice([40, 150, 400]), rng.choice(["ACGTN", "ACGTRY", "ACNNNGT", "ACGTWSKMN"]))
        if rng.random() < 0.5:
            p = rng.randrange(len(seq) + 1)
            seq = seq[:p] + planted(rng, rng.randint(1, 6), rng.randint(2, 8), rng.randint(0, 2), "ACGTN") + seq[p:]
    elif kind == "lower":                     # lower case (upper-cased by the driver)
        seq = random_seq(rng, rng.randint(0, 30), "ACGTacgtn") + planted(rng, rng.randint(1, 6), rng.randint(2, 10), rng.randint(0, 3), "acgtACGT") \
            + random_seq(rng, rng.randint(0, 30), "acgtACGT")
    elif kind == "large_k":                   # motif sizes up to 64, m = 1-3
        k = rng.randint(16, 64)
        seq = random_seq(rng, rng.randint(0, 30), "ACGT") + planted(rng, k, rng.randint(2, 4), rng.randint(0, 5)) + random_seq(rng, rng.randint(0, 30), "ACGT")
    elif kind == "absorbing":                 # k <= m: every phase may vary, a run never ends
        seq = random_seq(rng, rng.randint(0, 200), rng.choice(["ACGT", "AC", "ACGTN"]))
    elif kind == "n_ends":                    # N (either case) at both ends: the trimmed head shifts the rows
        seq = "N" * rng.randint(0, 12) + "n" * rng.randint(0, 3) + planted(rng, rng.randint(1, 5), rng.randint(2, 10), rng.randint(0, 3)) \
            + random_seq(rng, rng.randint(0, 40), "ACGTN") + "n" * rng.randint(0, 3) + "N" * rng.randint(0, 12)
        if rng.random() < 0.05:
            seq = "N" * rng.randint(0, 20)
    else:                                     # low-complexity sequence: many overlapping candidates per k
        seq = random_seq(rng, rng.choice([100, 300]), rng.choice(["AC", "AAC", "ACG", "AT"]))
    return {"tag": kind, "seq": seq,
            "settings": {"min_motif_size": kmin, "max_motif_size": kmax, "min_repeats": r, "min_span": span, "max_interruptions": m}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (holds utils/repeat_tracker.py)")
    ap.add_argument("--cases", type=int, default=3200)
    ap.add_argument("--seed", type=int, default=9)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.abspath(args.reference))
    from utils.repeat_tracker import RepeatTracker
    rng = random.Random(args.seed)
    with gzip.open(args.out, "wt") as f:
        for i in range(args.cases):
            case = make_case(rng, i)
            st = case["settings"]
            case["rows"] = reference_rows(RepeatTracker, case["seq"], st["min_motif_size"], st["max_motif_size"], st["min_repeats"],
                                          st["min_span"], st["max_interruptions"])
            f.write(json.dumps(case, separators=(",", ":")) + "\n")
    print(f"wrote {args.cases} cases to {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
