#!/usr/bin/env python3
"""Write tests/golden/dotplot.jsonl.gz: dot plots computed by the REFERENCE's generate_matrix + filter_out_noise
(reference plot_dot_plot.py), imported from a checkout of the reference at generation time only.

    python3 tools/gen_dotplot_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--seed 43]

Each line: {"tag", "seq", "t", "kept": [hex per row]} -- seq in upper case (the reference compares the text as given), t =
min_diagonal_run, kept = the cells that are 1 after filter_out_noise(matrix, t, set_noise_to=0), bit j of row i's number = cell
(i, j).  For every case the tool also runs the filter with set_noise_to=2 and asserts that the result is
kept + 2 * (raw and not kept): the filtered-out cells are exactly the raw cells that are not kept.

About 150 cases from one seed: the lengths 0-3, 63-65, 127-129, 191-193 and random ones up to 200; the alphabets ACGT, two
letters, one letter; runs of N inside and at both ends, nothing but N; IUPAC letters (R, Y, K) next to N; planted tandem units of
1-12; planted palindromic stretches (u + reversed(u)), which exercise the anti-diagonal; t in 0, 1, 2, 3, 4, 5, 8, 16, 63, 64.
The reference's module imports pyfaidx, which only its command line uses: an empty stand-in module of that name is put into
sys.modules before the import.  The file stays under 200 kB.
"""
import argparse
import gzip
import json
import os
import random
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "dotplot.jsonl.gz")
MAX_BYTES = 200_000
EDGE_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193]
THRESHOLDS = [0, 1, 2, 3, 4, 5, 8, 16, 63, 64]


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


def planted(rng, seq, piece):
    piece = piece[:len(seq)]
    at = rng.randrange(0, max(1, len(seq) - len(piece) + 1))
    return seq[:at] + piece + seq[at + len(piece):]


def cases(seed):
    rng = random.Random(seed)
    out = []

    def add(tag, seq, t):
        out.append((f"{tag}-{len(out)}", seq, t))

    for k, n in enumerate(EDGE_LENGTHS):
        add("edge-acgt", random_seq(rng, n, "ACGT"), 3)
        add("edge-two", random_seq(rng, n, "AT"), THRESHOLDS[k % len(THRESHOLDS)])
        add("edge-n-ends", with_n_runs(rng, random_seq(rng, n, "ACGT"), True), rng.choice([3, 4, 5]))
    for n in (0, 1, 2, 3, 63, 64, 65, 129):
        add("all-n", "N" * n, rng.choice([0, 3, 64]))
        add("one-letter", "A" * n, rng.choice([2, 5, 63, 64]))
    for t in THRESHOLDS:
        add("random-acgt", random_seq(rng, rng.randrange(4, 201), "ACGT"), t)
        add("random-two", random_seq(rng, rng.randrange(4, 161), rng.choice(["AC", "GT", "AN"])), t)
        add("n-runs", with_n_runs(rng, random_seq(rng, rng.randrange(4, 161), "ACGT"), rng.random() < 0.5), t)
        add("iupac", with_n_runs(rng, random_seq(rng, rng.randrange(4, 141), "ACGTRYKN"), rng.random() < 0.3), t)
        add("random-acgtn", random_seq(rng, rng.randrange(4, 201), "ACGTN"), t)
        add("random-one", rng.choice("ACGTN") * rng.randrange(4, 131), t)
    for unit_len in range(1, 13):
        n = rng.randrange(max(8, 3 * unit_len), 3 * unit_len + 120)
        unit = random_seq(rng, unit_len, "ACGT")
        add("tandem", planted(rng, random_seq(rng, n, "ACGT"), unit * rng.randrange(2, 8)), THRESHOLDS[2 + unit_len % 8])
    for _ in range(16):
        n = rng.randrange(20, 181)
        u = random_seq(rng, rng.randrange(3, 40), rng.choice(["ACGT", "ACGT", "ACGTN", "ACGTRY"]))
        add("palindrome", planted(rng, random_seq(rng, n, "ACGT"), u + u[::-1]), rng.choice([3, 4, 5, 8, 16, 63, 64]))
    for _ in range(6):
        n = rng.randrange(100, 201)
        unit = random_seq(rng, rng.randrange(2, 13), "ACN")
        add("tandem-n", planted(rng, random_seq(rng, n, "ACGT"), unit * 6), rng.choice([3, 5, 8]))
    return out


def record(ref, tag, seq, t):
    n = len(seq)
    raw = ref.generate_matrix(seq)
    kept = ref.generate_matrix(seq)
    ref.filter_out_noise(kept, min_diagonal_run=t, set_noise_to=0)
    marked = ref.generate_matrix(seq)
    ref.filter_out_noise(marked, min_diagonal_run=t, set_noise_to=2)
    rows = []
    for i in range(n):
        value = 0
        for j in range(n):
            assert kept[i][j] in (0, 1) and (not kept[i][j] or raw[i][j]), (tag, i, j)
            assert marked[i][j] == kept[i][j] + 2 * (raw[i][j] and not kept[i][j]), (tag, i, j)
            value |= kept[i][j] << j
        rows.append(format(value, "x"))
    return {"tag": tag, "seq": seq, "t": t, "kept": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="a checkout of the reference (its plot_dot_plot.py is imported)")
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import importlib.util
    import matplotlib
    matplotlib.use("Agg")          # the reference's module imports pyplot at the top
    sys.modules.setdefault("pyfaidx", types.ModuleType("pyfaidx"))   # used by its command line only
    spec = importlib.util.spec_from_file_location("reference_plot_dot_plot", os.path.join(args.reference, "plot_dot_plot.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    records = [record(ref, *case) for case in cases(args.seed)]
    with open(args.out, "wb") as raw:                   # mtime 0 and no file name: the bytes depend on the cases alone
        with gzip.GzipFile(filename="", fileobj=raw, mode="wb", compresslevel=9, mtime=0) as f:
            for rec in records:
                f.write((json.dumps(rec, separators=(",", ":")) + "\n").encode())
    size = os.path.getsize(args.out)
    print(f"{len(records)} cases, {size} bytes -> {args.out}")
    assert size < MAX_BYTES, f"{size} bytes: keep the fixture under {MAX_BYTES}"


if __name__ == "__main__":
    sys.exit(main())
