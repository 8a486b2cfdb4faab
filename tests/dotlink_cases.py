"""The planted junctions of tests/test_dotlink_gpu.py, built without a GPU: a contig of random ACGT (the rows) and, per strand, a
contig of N with one BAND per case and direction (the columns).  A band is a piece of the rows' contig copied with an insertion, a
deletion, changed bases or a homopolymer run next to the breakpoint -- copied (main) or reversed (anti), complemented for the
minus strand -- with N on both sides, so that no run leaves its band and the links of the whole rectangle are the links of the
bands, each found by the model (tests/dotlink_model.py) on the rows x the band's columns.  What a case is there for is asserted
on the model's list (check_claim), by tests/test_dotlink_cpu.py too, so a chance match that spoils a case fails on the CPU."""
import random

import dotchain_model as C
import dotlink_model as L
import dotpair_model as P
import dotruns_model as R

ROWS = 3_000                                                  # the rows' contig
FRONT = 3_000                                                 # N in front of and behind the bands: a band's line cell t is its row
S, G, D = 16, 5, 4                                            # min_seed, max_gap, max_shift of the planted junctions, unless a case says otherwise
FOLLOW = 2_048                                                # PRF_DOTCHAIN_FOLLOW


def _random(n, seed, alphabet=b"ACGT"):
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


def _other(*avoid):
    """A base that is none of `avoid`."""
    return next(x for x in b"ACGT" if x not in avoid)


CHANGE = bytes.maketrans(b"ACGT", b"CGTA")

# name: (row of the piece's first base, [op], (min_seed, max_gap, max_shift), claim)
#   ("m", n) n bases copied; ("x", n) n bases changed; ("ins", k) k bases only the columns have; ("del", k) k bases only the rows have;
#   ("run", r) the next r bases of the rows are one homopolymer run (written into the rows' contig), copied
#   ("N", n): the next n bases of the rows are N (written into the rows' contig), copied; N == N is a match
# claim: (shift, gap, overlap) of the one link the band must have, or None: the band must have no link
CASES = {
    "an insertion of 1": (100, [("m", 40), ("ins", 1), ("m", 40)], (S, G, D), (1, 0, None)),
    "an insertion of max_shift": (200, [("m", 40), ("ins", D), ("m", 40)], (S, G, D), (D, 0, None)),
    "an insertion of max_shift + 1": (300, [("m", 40), ("ins", D + 1), ("m", 40)], (S, G, D), None),
    "a deletion of 1": (400, [("m", 40), ("del", 1), ("m", 40)], (S, G, D), (-1, 0, None)),
    "a deletion of max_shift": (500, [("m", 40), ("del", D), ("m", 40)], (S, G, D), (-D, 0, None)),
    "a deletion of max_shift + 1": (600, [("m", 40), ("del", D + 1), ("m", 40)], (S, G, D), None),
    "a gap of exactly max_gap": (700, [("m", 40), ("ins", 2), ("x", G), ("m", 40)], (S, G, D), (2, G, 0)),
    "a gap of max_gap + 1": (800, [("m", 40), ("ins", 2), ("x", G + 1), ("m", 40)], (S, G, D), None),
    "a gap of max_gap in the columns": (900, [("m", 40), ("del", 2), ("x", G), ("m", 40)], (S, G, D), (-2, G, 0)),
    "an overlap of ov": (1_000, [("m", 30), ("run", S - 1), ("ins_same", 1), ("m", 40)], (S, G, D), (1, 0, S - 1)),
    "an overlap of ov + 1": (1_100, [("m", 30), ("run", S), ("ins_same", 1), ("m", 40)], (S, G, D), None),
    "an overlap of 16 at min_seed 20": (1_200, [("m", 30), ("run", 16), ("ins_same", 1), ("m", 40)], (20, G, D), (1, 0, 16)),
    "an overlap of 17 at min_seed 20": (1_300, [("m", 30), ("run", 17), ("ins_same", 1), ("m", 40)], (20, G, D), None),
    "a junction across a word of the line": (1_350, [("m", 57), ("ins", 1), ("x", 4), ("m", 30)], (S, G, D), (1, 4, 0)),   # 1 406 | 1 411
    "a junction across a tile row": (1_536 - 40, [("m", 40), ("del", 3), ("m", 30)], (S, G, D), (-3, 0, None)),
    "an N block next to the junction": (1_600, [("m", 20), ("N", 6), ("m", 20), ("ins", 2), ("m", 6), ("N", 3), ("m", 30)], (S, G, D), (2, 0, None)),
    "max_gap = 0": (1_800, [("m", 30), ("ins", 3), ("m", 30)], (S, 0, D), (3, 0, None)),
    "max_gap = 0, a changed base behind the insertion": (1_900, [("m", 30), ("ins", 3), ("x", 1), ("m", 30)], (S, 0, D), None),
    "a shift of 32": (2_000, [("m", 40), ("ins", 32), ("m", 40)], (S, G, 32), (32, 0, None)),
    "a shift of -32": (2_100, [("m", 40), ("del", 32), ("m", 40)], (S, G, 32), (-32, 0, None)),
    "a shift of 33": (2_200, [("m", 40), ("ins", 33), ("m", 40)], (S, G, 32), None),
    "a predecessor of more than F cells": (7, [("m", 300), ("x", 2)] * 7 + [("m", 280), ("del", 2), ("m", 50)], (S, G, D), (-2, 0, None)),
}


def build():
    """(rows, {strand: columns}, {strand: {(name, dir): (first column, last column + 1) of the band}})"""
    rows = bytearray(_random(ROWS, 78))
    pieces = {}
    for name, (i, ops, _params, _claim) in CASES.items():      # first the letters the cases write into the rows' contig
        at = i
        for kind, n in ops:
            if kind == "run":
                base = _other(rows[at - 1], rows[at + n])
                rows[at:at + n] = bytes([base]) * n
            elif kind == "N":
                rows[at:at + n] = b"N" * n
            if kind in ("m", "x", "run", "N", "del"):
                at += n
    rng = random.Random(79)
    for name, (i, ops, _params, _claim) in CASES.items():
        at, out = i, bytearray()
        for kind, n in ops:
            if kind in ("m", "run", "N"):
                out += rows[at:at + n]
            elif kind == "x":
                out += bytes(rows[at:at + n]).translate(CHANGE)
            elif kind == "ins":                                 # neither lengthens the run in front (on its line) nor the one behind
                junk = bytearray(rng.choice(b"ACGT") for _ in range(n))
                junk[0] = _other(rows[at], rows[at - 1] if n == 1 else 0)
                junk[-1] = _other(rows[at - 1], rows[at] if n == 1 else 0)
                out += junk
            elif kind == "ins_same":                            # one base more of the homopolymer run in front
                out += rows[at - 1:at] * n
            if kind in ("m", "x", "run", "N", "del"):
                at += n
        assert at <= ROWS
        pieces[name] = bytes(out)
    rows = bytes(rows)
    columns, where = {}, {}
    for strand in "+-":
        b, bands = bytearray(b"N" * FRONT), {}
        for d in (R.MAIN, R.ANTI):
            for k, (name, piece) in enumerate(pieces.items()):
                if strand == "-":
                    piece = P.comp(piece)
                b += b"N" * (3 + 11 * k + (5 if d == R.ANTI else 0))
                bands[name, d] = (len(b), len(b) + len(piece))
                b += piece if d == R.MAIN else piece[::-1]
        b += b"N" * FRONT
        columns[strand], where[strand] = bytes(b), bands
    return rows, columns, where


def expected(rows, columns, band, strand, params):
    """(chains, links) of the rows x the band's columns and the N on either side, in the columns of the whole contig."""
    lo, hi = band[0] - 3, band[1] + 3
    raw = P.kept_cells(rows, columns, strand, 0, (0, None), (lo, hi))
    every = R.all_runs(raw)
    chains = C.all_chains(raw, params[0], params[1], every[every["len"] >= params[0]])
    links = L.select(L.all_links(chains, raw.shape[1], *params), *raw.shape)
    chains = C.select(chains, *raw.shape)
    for rows_ in (chains, links):
        rows_["col"] += lo
    links["from_col"] += lo
    return chains, links


def check_claim(name, links, d):
    """What the case is there for, on the model's list of its band."""
    i, ops, params, claim = CASES[name]
    if claim is None:
        assert len(links) == 0, (name, links)
        return
    shift, gap, overlap = claim
    assert len(links) == 1 and links["dir"][0] == d and links["shift"][0] == shift and links["gap"][0] == gap, (name, d, links)
    assert overlap is None or links["overlap"][0] == overlap, (name, d, links)
