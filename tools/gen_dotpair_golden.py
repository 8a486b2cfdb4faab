#!/usr/bin/env python3
"""Write tests/golden/dotpair.jsonl.gz: dot plots of two sequences, on either strand, filtered by the REFERENCE's filter_out_noise
(reference plot_dot_plot.py), imported from a checkout of the reference at generation time only.

    python3 tools/gen_dotpair_golden.py --reference PATH_TO_REFERENCE_CHECKOUT [--seed 44]

The reference plots one sequence against itself, but its filter_out_noise accepts any square 0/1 matrix.  For each case the tool
  1. builds the raw na x nb matrix in plain Python: raw[i][j] = a[i] == b[j] on strand "+", a[i] == comp(b[j]) on strand "-",
     with comp = A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H and every other letter itself (the project's definition, DESIGN 12,
     not the reference's);
  2. pads it with zeros to max(na, nb) square and runs the reference's filter on it (zeros neither pass the filter nor lengthen
     a run, so the padded square is filtered as the rectangle clipped by its own bounds);
  3. asserts that the padding stayed zero and that the set_noise_to=2 run equals kept + 2 * (raw and not kept);
  4. crops and records {"tag", "a", "b", "strand", "t", "kept": [hex per row]}, bit j of row i's number = cell (i, j).

About 150 cases from one seed: na and nb drawn independently from 0-3, 63-65, 127-129, 191-193 and random values up to 200,
with na < nb, na > nb and one side empty among them; the alphabets of tools/gen_dotplot_golden.py plus R, Y, K, M, S, W, B, V, D,
H; runs of N in both sequences; a shared piece (plus strand, main diagonal), a reverse-complemented piece (minus, anti-diagonal),
a reversed piece (plus, anti-diagonal) and a complemented piece (minus, main diagonal), some of them touching a corner of the
rectangle; t in 0, 1, 2, 3, 4, 5, 8, 16, 63, 64.  The file stays under 200 kB.
"""
import argparse
import gzip
import json
import os
import random
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "dotpair.jsonl.gz")
MAX_BYTES = 200_000
EDGE_LENGTHS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193]
THRESHOLDS = [0, 1, 2, 3, 4, 5, 8, 16, 63, 64]
COMP = {**{x: x for x in "ABCDEFGHIJKLMNOPQRSTUVWXYZ"},
        **{x: y for pair in ("AT", "CG", "RY", "KM", "BV", "DH") for x, y in (pair, pair[::-1])}}
IUPAC = "ACGTRYKMSWBVDHN"


def comp(seq):
    return "".join(COMP[x] for x in seq)


def random_seq(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def with_n_runs(rng, seq):
    s = list(seq)
    for _ in range(rng.randrange(1, 4)):
        if s:
            at, run = rng.randrange(len(s)), rng.randrange(1, 12)
            for i in range(at, min(len(s), at + run)):
                s[i] = "N"
    return "".join(s)


def planted(rng, seq, piece, where):
    """seq with piece written over it: at a random place, or touching its start or its end."""
    piece = piece[:len(seq)]
    at = {"start": 0, "end": len(seq) - len(piece)}.get(where, rng.randrange(0, max(1, len(seq) - len(piece) + 1)))
    return seq[:at] + piece + seq[at + len(piece):]


def cases(seed):
    rng = random.Random(seed)
    out = []

    def add(tag, a, b, strand, t):
        out.append((f"{tag}-{len(out)}", a, b, strand, t))

    for k, na in enumerate(EDGE_LENGTHS):                                  # every edge length on both sides, both strands
        nb = EDGE_LENGTHS[(k * 5 + 3) % len(EDGE_LENGTHS)]
        add("edge-acgt", random_seq(rng, na, "ACGT"), random_seq(rng, nb, "ACGT"), "+-"[k % 2], 3)
        add("edge-two", random_seq(rng, nb, "AT"), random_seq(rng, na, "AT"), "-+"[k % 2], THRESHOLDS[k % len(THRESHOLDS)])
        add("edge-n", with_n_runs(rng, random_seq(rng, na, "ACGT")), with_n_runs(rng, random_seq(rng, rng.randrange(0, 201), "ACGT")),
            rng.choice("+-"), rng.choice([3, 4, 5]))
    for na, nb in ((0, 0), (0, 70), (70, 0), (1, 129), (129, 1), (64, 65), (130, 66)):
        add("all-n", "N" * na, "N" * nb, rng.choice("+-"), rng.choice([0, 3, 64]))
        add("one-letter", "A" * na, "T" * nb, "-", rng.choice([2, 5, 63, 64]))
        add("one-letter", "C" * na, "C" * nb, "+", rng.choice([2, 5, 63, 64]))
    for t in THRESHOLDS:
        for strand in "+-":
            add("random-acgt", random_seq(rng, rng.randrange(4, 201), "ACGT"), random_seq(rng, rng.randrange(4, 201), "ACGT"), strand, t)
            add("random-two", random_seq(rng, rng.randrange(4, 161), rng.choice(["AT", "CG", "AN"])),
                random_seq(rng, rng.randrange(4, 161), rng.choice(["AT", "CG", "TN"])), strand, t)
            add("iupac", with_n_runs(rng, random_seq(rng, rng.randrange(4, 141), IUPAC)),
                with_n_runs(rng, random_seq(rng, rng.randrange(4, 141), IUPAC)), strand, t)
    for k in range(32):                                                    # planted pieces, one kind each
        kind = ("shared", "revcomp", "reversed", "complemented")[k % 4]
        alphabet = ("ACGT", "ACGT", "ACGTN", IUPAC)[(k // 4) % 4]
        u = random_seq(rng, rng.randrange(3, 70), alphabet)
        v = {"shared": u, "revcomp": comp(u)[::-1], "reversed": u[::-1], "complemented": comp(u)}[kind]
        where = ("any", "start", "end")[(k // 8) % 3]
        a = planted(rng, random_seq(rng, rng.randrange(len(u), 181), "ACGT"), u, where)
        b = planted(rng, random_seq(rng, rng.randrange(len(u), 181), "ACGT"), v, ("end", "any", "start")[(k // 8) % 3])
        strand = "-" if kind in ("revcomp", "complemented") else "+"
        add(kind, a, b, strand, rng.choice([3, 4, 5, 8, 16, 63, 64]))
        if k % 5 == 0:
            add(kind + "-other-strand", a, b, "+" if strand == "-" else "-", rng.choice([3, 5, 8]))
    return out


def record(ref, tag, a, b, strand, t):
    na, nb = len(a), len(b)
    size = max(na, nb)
    cb = comp(b) if strand == "-" else b
    raw = [[int(i < na and j < nb and a[i] == cb[j]) for j in range(size)] for i in range(size)]
    kept = [row[:] for row in raw]
    ref.filter_out_noise(kept, min_diagonal_run=t, set_noise_to=0)
    marked = [row[:] for row in raw]
    ref.filter_out_noise(marked, min_diagonal_run=t, set_noise_to=2)
    rows = []
    for i in range(size):
        value = 0
        for j in range(size):
            assert kept[i][j] in (0, 1) and (not kept[i][j] or raw[i][j]), (tag, i, j)     # (so the padding stayed zero)
            assert marked[i][j] == kept[i][j] + 2 * (raw[i][j] and not kept[i][j]), (tag, i, j)
            value |= kept[i][j] << j
        if i < na:
            rows.append(format(value, "x"))
    return {"tag": tag, "a": a, "b": b, "strand": strand, "t": t, "kept": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="a checkout of the reference (its plot_dot_plot.py is imported)")
    ap.add_argument("--seed", type=int, default=44)
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
