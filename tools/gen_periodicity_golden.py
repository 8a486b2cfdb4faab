#!/usr/bin/env python3
"""Write tests/golden/periodicity.jsonl.gz: periodicity matrices computed by the REFERENCE's get_period_matrix
(reference utils/plot_utils.py:12-25), imported from a checkout of the reference at generation time only.

    python3 tools/gen_periodicity_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--seed 41]

The reference fills a set cell with abs(hash(...)) of Python's salted hash, so the values differ from run to run.  What is
recorded is what does not: which cells are set, and which set cells of a row share a value.  Each line:
    {"tag", "seq", "min", "max",            the arguments (seq upper case: the reference compares the text as given)
     "shape": [rows, columns],              of the returned matrix (rows = max after the reference's clamp)
     "cells": [hex, ...],                   per row: the set cells as a bit string, bit i of the number = column i
     "classes": [[id, ...], ...]}           per row: for every set cell, in column order, the number of its value in order of
                                            first appearance in that row
The tool asserts that no set cell hashed to 0 (it would read as not set).

About 300 cases from one seed: the lengths 0-3, 63-65, 127-129, 191-193 and random ones up to 600; the alphabets ACGT and two
letters, runs of N inside and at both ends, nothing but N, IUPAC letters (R, Y, K) next to N; planted tandem repeats with units
of 1-70; min > 1, max above len // 2, max = 1.  Most cases ask for few rows, so that the file stays under 200 kB.
"""
import argparse
import gzip
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "periodicity.jsonl.gz")
MAX_BYTES = 200_000
EDGE_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193]


def random_seq(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def with_n_runs(rng, seq, ends):
    s = list(seq)
    n = len(s)
    if n and ends:
        for i in range(min(n, rng.randrange(1, 9))):
            s[i] = "N"
        for i in range(min(n, rng.randrange(1, 9))):
            s[n - 1 - i] = "N"
    for _ in range(rng.randrange(1, 4)):
        if n:
            at, run = rng.randrange(n), rng.randrange(1, 12)
            for i in range(at, min(n, at + run)):
                s[i] = "N"
    return "".join(s)


def with_planted(rng, seq, unit_len, alphabet="ACGT"):
    unit = random_seq(rng, unit_len, alphabet)
    copies = rng.randrange(2, 6)
    rep = (unit * copies)[:max(0, len(seq))]
    at = rng.randrange(0, max(1, len(seq) - len(rep) + 1))
    return seq[:at] + rep + seq[at + len(rep):]


def cases(seed):
    rng = random.Random(seed)
    out = []

    def add(tag, seq, lo, hi):
        out.append((f"{tag}-{len(out)}", seq, lo, hi))

    for n in EDGE_LENGTHS:
        add("edge-acgt", random_seq(rng, n, "ACGT"), 1, 6)
        add("edge-two", random_seq(rng, n, "AT"), 1, 3)
        add("edge-all-n", "N" * n, 1, 4)
        add("edge-n-ends", with_n_runs(rng, random_seq(rng, n, "ACGT"), True), 1, 5)
        add("edge-max-one", random_seq(rng, n, "ACG"), 1, 1)
        add("edge-min-above-one", random_seq(rng, n, "ACGT"), 3, 7)
    for n in (0, 1, 2, 3, 63, 64, 65):
        add("max-above-half", random_seq(rng, n, "ACGT"), 1, n + 5)
        add("min-above-half", random_seq(rng, n, "AC"), n // 2 + 1, n + 5)
    for _ in range(76):
        n = rng.randrange(4, 601)
        lo = rng.choice([1, 1, 1, 2, 5])
        add("random-acgt", random_seq(rng, n, "ACGT"), lo, lo + rng.randrange(0, 6))
    for _ in range(25):
        n = rng.randrange(4, 400)
        add("random-two", random_seq(rng, n, rng.choice(["AC", "GT", "AN"])), 1, rng.randrange(1, 6))
    for _ in range(30):
        n = rng.randrange(4, 400)
        add("n-runs", with_n_runs(rng, random_seq(rng, n, "ACGT"), rng.random() < 0.5), 1, rng.randrange(1, 8))
    for _ in range(30):
        n = rng.randrange(4, 300)
        add("iupac", with_n_runs(rng, random_seq(rng, n, "ACGTRYKN"), rng.random() < 0.3), 1, rng.randrange(1, 7))
    for unit_len in list(range(1, 13)) + [15, 16, 17, 21, 31, 32, 33, 40, 50, 63, 64, 65, 70]:
        n = rng.randrange(max(8, 3 * unit_len), max(9, 3 * unit_len) + 200)
        seq = with_planted(rng, random_seq(rng, n, "ACGT"), unit_len)
        lo = max(1, unit_len - 1)
        add("planted", seq, lo, unit_len + 1)                 # the rows around the unit
        if unit_len % 3 == 0:
            add("planted-multiple", seq, 2 * unit_len, 2 * unit_len)
    for _ in range(8):                                         # a few tall matrices: max up to len // 2 and above
        n = rng.randrange(20, 90)
        add("tall", with_planted(rng, random_seq(rng, n, "ACGTN"), rng.randrange(1, 9)), 1, rng.choice([n // 2, n, 50]))
    for _ in range(6):
        n = rng.randrange(100, 600)
        add("planted-n", with_planted(rng, random_seq(rng, n, "ACGT"), rng.randrange(2, 30), "ACN"), 1, 4)
    return out


def record(get_period_matrix, tag, seq, lo, hi):
    matrix = get_period_matrix(lo, hi, seq)
    cells, classes = [], []
    for r, row in enumerate(matrix):
        period = r + 1
        bits, ids, seen = 0, [], {}
        for i, v in enumerate(row):
            want_set = i + period < len(seq) and seq[i] == seq[i + period] and lo - 1 <= r
            if want_set:
                assert v != 0, f"{tag}: set cell ({period}, {i}) hashed to 0"
            if v:
                assert want_set
                bits |= 1 << i
                ids.append(seen.setdefault(v, len(seen)))
        cells.append(format(bits, "x"))
        classes.append(ids)
    return {"tag": tag, "seq": seq, "min": lo, "max": hi, "shape": [len(matrix), len(seq)], "cells": cells, "classes": classes}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="a checkout of the reference (its utils/plot_utils.py is imported)")
    ap.add_argument("--seed", type=int, default=41)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import importlib.util
    import matplotlib
    matplotlib.use("Agg")          # the reference's module imports pyplot at the top
    spec = importlib.util.spec_from_file_location("reference_plot_utils", os.path.join(args.reference, "utils", "plot_utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    records = [record(ref.get_period_matrix, *case) for case in cases(args.seed)]
    with open(args.out, "wb") as raw:                   # mtime 0 and no file name: the bytes depend on the cases alone
        with gzip.GzipFile(filename="", fileobj=raw, mode="wb", compresslevel=9, mtime=0) as f:
            for rec in records:
                f.write((json.dumps(rec, separators=(",", ":")) + "\n").encode())
    size = os.path.getsize(args.out)
    n_cells = sum(len(ids) for rec in records for ids in rec["classes"])
    print(f"{len(records)} cases, {n_cells} set cells, {size} bytes -> {args.out}")
    assert size < MAX_BYTES, f"{size} bytes: keep the fixture under {MAX_BYTES}"


if __name__ == "__main__":
    sys.exit(main())
