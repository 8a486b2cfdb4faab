"""The inputs of tests/test_far_positions_gpu.py, built without a GPU: small contigs placed so that global position 2^31 and
global position 2^32 fall INSIDE one of them, and one contig wholly beyond 2^32.  tests/test_far_positions_cpu.py asserts what
the cases are built around (the layout, the floors of every expected result) on the CPU.

Layout.  A contig starts on a multiple of T = 65 536; the next base is roundup(base + len + kmax_hint + 64, T) (csrc/genome.cpp).
Five contigs (FAR_LENS): a filler up to 2^31 - 2 T, a contig of 200 000 whose offset EDGE = 131 072 is global 2^31, a filler up to
2^32 - 2 T, a contig of 200 000 whose offset EDGE is global 2^32, and a contig of 70 001 at 2^32 + 2 T.  The three small contigs
alone are the NEAR genome: near contig i is far contig FAR_OF[i], and every product of a range must be the same bytes on both.

Genome A is generated on the device (stand-in recipe 2 of every contig, three planes); its host bytes come from synth.standin2.
Genome B is loaded: the fillers are nothing but N, the small contigs are crafted (b_contigs) and hold letters outside ACGTN, so B
has eight planes.  What B holds around EDGE:
  contig 1 (near 0): a copy of the piece S1 of contig 4 (near 2), 6 000 positions, S1[CENTRE] at EDGE.  S1 holds, at begins that
      are no multiple of 64 in contig 1, an N block of 300, the piece U (IUPAC letters, period 11), a single R and -- across
      CENTRE, so across EDGE -- a perfect tandem repeat of period 7.
  contig 3 (near 1): the reverse complement of the piece S3 of contig 4, S3[CENTRE] at EDGE - 1.  S3 holds the same furniture and,
      across CENTRE, a tandem repeat of period 33 with a substitution every 40 positions.
  Only one item can hold position EDGE itself (inside the enclosing copy): the tandem repeat.  The N block, U and R lie within
  2 300 positions of EDGE, inside every product range that straddles it.
  contig 4 also holds S1 with a substitution every 101 cells and S1 with three indels of 1 to 3 bases (one of them at CENTRE, so
  the junction lies between rows EDGE - 1 and EDGE of contig 1), and a piece repeated at distance 2 050 (the k-slice boundary
  of the periodicity kernels); contig 1 holds S3, S3 with substitutions and S3 with indels far from EDGE: the columns of the
  plots whose rows are contig 3.  Every contig ends in N up to its last position (test_dotruns_gpu._contig).

A product case (CASES) names a genome, what it pins ("2^31", "2^32" or "beyond": wholly in the last contig), a kind and its ranges
in NEAR contig numbers.  calls() runs every call of the case on a resident genome, models() gives the same list from the CPU
models of the tests and asserts on the way, on the MODEL's output, that the case is not vacuous: a run, chain, link, set cell or count
whose extent crosses EDGE (start < EDGE <= last cell, in the contig's coordinates), or, beyond, any entry at all."""
import collections
import functools

import numpy as np

import dotchain_model as C
import dotlink_cases as LC
import dotlink_model as L
import dotpair_model as P
import dotplot_model as D
import dotruns_model as R
import periodchain_model as M
import periodicity_model as PM
import synth
import test_dotruns_gpu as DR
from pipelined_edges_cases import oracle_rows  # noqa: F401  (re-exported for the tests)

T = 65_536
EDGE = 131_072
SMALL_LENS = (200_000, 200_000, 70_001)
FAR_LENS = [2 ** 31 - 2 * T - 1_000, SMALL_LENS[0], 2 ** 31 - 4 * T - 1_000, SMALL_LENS[1], SMALL_LENS[2]]
FAR_OF = (1, 3, 4)                                        # near contig -> far contig
FAR_BASES = [0, 2 ** 31 - 2 * T, 2 ** 31 + 2 * T, 2 ** 32 - 2 * T, 2 ** 32 + 2 * T]
HINT_A, HINT_B = 50, 64                                   # the kmax_hint of the two genomes
HINTS = (HINT_A, HINT_B)                                  # every hint the GPU module uses
A_SEEDS = [501, 502, 503, 504, 505]                       # stand-in seeds of genome A's five contigs
SCAN = (1, 50, 3, 9)
LITERAL = (1, 8, 1, 5)


def expected_bases(lens, kmax_hint):
    """The first global position of every contig of a genome loaded with this hint."""
    out, cur = [], 0
    for n in lens:
        out.append(cur)
        cur = -(-(cur + n + kmax_hint + 64) // T) * T
    return out


# ---- genome A ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def a_contigs():
    """The host bytes of genome A's three small contigs (near order)."""
    return tuple(synth.standin2(FAR_LENS[c], A_SEEDS[c]).tobytes() for c in FAR_OF)


def a_window(far_contig, off, count):
    return synth.standin2(FAR_LENS[far_contig], A_SEEDS[far_contig], off, count).tobytes()


# ---- genome B ---------------------------------------------------------------------------------------------------------------
PIECE, CENTRE = 6_000, 2_989
C1_COPY = EDGE - CENTRE                                   # S1 in contig 1: S1[x] at C1_COPY + x
C3_COPY = EDGE - (PIECE - CENTRE)                         # revcomp(S3) in contig 3: S3[x] at C3_COPY + PIECE - 1 - x
S1_AT, S1_SUBST_AT, S1_INDEL_AT, S3_AT = 10_000, 17_003, 24_007, 31_011        # in contig 4
S3_COPY_AT, S3_SUBST_AT, S3_INDEL_AT = 70_005, 77_009, 84_013                  # in contig 1, behind its first tile: no letter
# outside ACGTN lies in reach of the filler in front of it, whose tiles all stay in the class that is never scanned
FAR_K, FAR_K_AT, FAR_K_LEN = 2_050, 50_500, 400           # contig 4: FAR_K_LEN positions repeated FAR_K further on
INDELS = ((1_200, "ins", 1), (CENTRE, "ins", 2), (4_000, "del", 3))
R_AT = 2_200                                              # the single R of a piece: with U in front of CENTRE, so that the letters outside
# ACGTN of contig 1 lie in its second tile and those of contig 3 in its third, and each keeps one tile for the fused kernel


def _piece(seed, tandem):
    s = bytearray(DR._random(PIECE, seed))
    s[700:1_000] = b"N" * 300
    s[1_500:1_500 + len(DR.U)] = DR.U
    s[R_AT] = ord("R")
    lo, body, period = tandem
    s[lo:lo + len(body)] = body
    s[lo - 1] = LC._other(body[period - 1])               # the repeat starts where it is written and ends where it ends
    s[lo + len(body)] = LC._other(body[len(body) - period])
    return bytes(s)


def _tandem7():
    return CENTRE - 60, (b"ACGGTCA" * 12)[:84], 7


def _tandem33():
    motif = DR._random(33, 103)
    body = bytearray(motif * 13)
    for at in range(17, len(body), 40):
        body[at] = LC._other(body[at])
    return CENTRE - 200, bytes(body), 33


def substituted(piece):
    """A copy with a substitution every 101 cells (N and the letters outside ACGT stay)."""
    s = bytearray(piece)
    for at in range(50, len(s), 101):
        s[at:at + 1] = bytes(s[at:at + 1]).translate(LC.CHANGE)
    return bytes(s)


def with_indels(piece, seed):
    """A copy with the INDELS: ("ins", k) k bases only the copy has in front of piece[at], ("del", k) piece[at:at + k] left out;
    an insertion lengthens neither the run in front of it nor the one behind (tests/dotlink_cases.py)."""
    import random
    rng, out, done = random.Random(seed), bytearray(), 0
    for at, kind, k in INDELS:
        out += piece[done:at]
        done = at
        if kind == "ins":
            junk = bytearray(rng.choice(b"ACGT") for _ in range(k))
            junk[0] = LC._other(piece[at], piece[at - 1] if k == 1 else 0)
            junk[-1] = LC._other(piece[at - 1], piece[at] if k == 1 else 0)
            out += junk
        else:
            done = at + k
    return bytes(out + piece[done:])


@functools.lru_cache(maxsize=None)
def b_contigs():
    """The three crafted contigs of genome B (near order: contig 1, contig 3, contig 4 of the far genome)."""
    s1, s3 = _piece(101, _tandem7()), _piece(104, _tandem33())
    far_k = DR._random(FAR_K_LEN, 105)
    c4 = DR._contig(SMALL_LENS[2], 50, True, [(S1_AT, s1), (S1_SUBST_AT, substituted(s1)), (S1_INDEL_AT, with_indels(s1, 106)),
                                               (S3_AT, s3), (FAR_K_AT, far_k), (FAR_K_AT + FAR_K, far_k), (69_500, DR.U[:260])])
    assert c4[S1_AT:S1_AT + PIECE] == s1 and c4[S3_AT:S3_AT + PIECE] == s3
    c1 = DR._contig(SMALL_LENS[0], 40, False, [(C1_COPY, s1), (S3_COPY_AT, s3), (S3_SUBST_AT, substituted(s3)),
                                                (S3_INDEL_AT, with_indels(s3, 107))])
    c3 = DR._contig(SMALL_LENS[1], 41, False, [(C3_COPY, P.revcomp(s3))])
    return c1, c3, c4


def near_contigs(genome):
    return a_contigs() if genome == "A" else b_contigs()


# ---- product cases ----------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name genome pins kind a b strand opt")
SPAN = 2_600                                              # positions of a straddling range: EDGE lies 1 307 or 1 280 behind its begin
OFF = {37: 1_307, 0: 1_280}                               # EDGE - begin of a straddling range, by begin % 64


def _straddle(contig, mod, span=SPAN):
    return (contig, EDGE - OFF[mod], EDGE - OFF[mod] + span)


def _cases():
    """Every product at every place with one begin that is a multiple of 64 (the kernels' case without a funnel shift) and one that
    is 37 beyond one (the shift across the word that holds the boundary): of the range that lies at the place -- the straddling
    one, or, beyond, the rows' range."""
    out = []
    for genome in "BA":
        big = genome == "B"
        hint = HINT_B if big else HINT_A                       # period_bits and period_counts take periods up to the genome's kmax_hint
        seeds = ((12, 8), (3, 2)) if big else ((3, 2),)
        for mod in (37, 0):
            for pins, contig in (("2^31", 0), ("2^32", 1)):
                r = _straddle(contig, mod)
                out.append(Case(f"{genome} period {pins} begin%64={mod}", genome, pins, "period", r, None, None, {"k": (1, hint)}))
                out.append(Case(f"{genome} dotplot {pins} begin%64={mod}", genome, pins, "dotplot", r, None, None,
                                {"t_wide": 64, "long_repeat": (pins == "2^31") if big else None}))
                begin = EDGE - 20_000 - 32 + mod               # (EDGE - 20 000 is 32 beyond a multiple of 64)
                out.append(Case(f"{genome} period_chains {pins} begin%64={mod}", genome, pins, "pchains", (contig, begin, begin + 40_000),
                                None, None, {"k": (1, 130), "seeds": seeds}))
            out.append(Case(f"{genome} period beyond begin%64={mod}", genome, "beyond", "period",
                            (2, S1_AT + 48 + mod, S1_AT + 48 + mod + SPAN), None, None, {"k": (1, hint)}))
            # (period_chains takes any period: lines 1 .. 2 100 cross the k slices of 1 024 (eight planes) and 2 048 (three))
            out.append(Case(f"{genome} period_chains beyond, k-slice boundary begin%64={mod}", genome, "beyond", "pchains",
                            (2, 49_920 + mod, 61_920 + mod), None, None,
                            {"k": (1, 2_100), "seeds": ((12, 8),) if big else ((3, 2),), "far_k": big, "k_slices": True}))
            out.append(Case(f"{genome} dotplot beyond begin%64={mod}", genome, "beyond", "dotplot",
                            (2, S1_AT + 1_648 + mod, S1_AT + 1_648 + mod + SPAN), None, None,
                            {"t_wide": 64, "long_repeat": True if big else None}))
            out.append(Case(f"{genome} period_chains beyond begin%64={mod}", genome, "beyond", "pchains", (2, mod, 40_000 + mod), None, None,
                            {"k": (1, 130), "seeds": seeds}))
        out.append(Case(f"{genome} dotplot to the last position", genome, "beyond", "dotplot", (2, 69_312 + 37, None), None, None, {"t_wide": None}))
    # the pair products of B: rows across EDGE against the columns that hold the piece, its copy with substitutions (chains)
    # and its copy with indels (links); both orders, both strands (the planted strand: + for the copy, - for the inverted one);
    # the begin of the straddling range changes with the order, and for the kinds that run on both strands with the strand too
    for pins, contig, other, exact, subst, indel, planted in (
            ("2^31", 0, 2, S1_AT, S1_SUBST_AT, S1_INDEL_AT, "+"), ("2^32", 1, 0, S3_COPY_AT, S3_SUBST_AT, S3_INDEL_AT, "-")):
        for strand in "+-":
            for swap in (False, True):
                mod = 37 if (strand == "+") != swap else 0
                rows = _straddle(contig, mod)
                order = "columns" if swap else "rows"
                tag = f"{pins} in the {order} {strand} begin%64={mod}"
                pair = (lambda x, y: (y, x)) if swap else (lambda x, y: (x, y))
                a, b = pair(rows, (other, exact + 1_100, exact + 5_300))
                out.append(Case(f"B dotpair {tag}", "B", pins, "pair", a, b, strand,
                                {"planted": strand == planted, "t_wide": 64 if strand == planted else None, "across": order}))
                if strand == planted:                          # (at 12 cells a seed is no chance: the other strand has none)
                    a, b = pair(rows, (other, subst + 1_500, subst + 4_500))
                    out.append(Case(f"B dotpair_chains {tag}", "B", pins, "chains", a, b, strand,
                                    {"planted": True, "seeds": (12, 8), "across": order}))
                    a, b = pair(rows, (other, indel + 1_500, indel + 4_500))
                    out.append(Case(f"B dotpair_links {tag}", "B", pins, "links", a, b, strand,
                                    {"planted": True, "seeds": (12, 8), "across": order}))
                # (3, 2): every chance run of three cells is a seed, so the rectangle is small: the junction at EDGE and 96 cells each way
                small = (contig, EDGE - 91 if mod == 37 else EDGE - 128, EDGE + 101)
                mid = indel + (CENTRE if planted == "+" else CENTRE + 2)
                a, b = pair(small, (other, mid - 100 + 3, mid + 100 + 3))
                out.append(Case(f"B dotpair_links (3, 2) {tag}", "B", pins, "links", a, b, strand,
                                {"planted": False, "seeds": (3, 2), "chains_too": True, "across": order}))
    out.append(Case("B dotpair 2^31 against itself", "B", "2^31", "pair", _straddle(0, 37), _straddle(0, 37), "+",
                    {"planted": True, "t_wide": None, "across": "rows", "self": True}))
    out.append(Case("B dotpair 2^32 against 2^31", "B", "2^32", "pair", _straddle(1, 37), _straddle(0, 0), "-",
                    {"planted": False, "t_wide": None, "across": "rows"}))
    for mod in (37, 0):
        for kind, at, seeds in (("pair", S1_AT, None), ("chains", S1_SUBST_AT, (12, 8)), ("links", S1_INDEL_AT, (12, 8))):
            out.append(Case(f"B dotpair {kind} beyond begin%64={mod}", "B", "beyond", kind, (2, S1_AT + 1_648 + mod, S1_AT + 1_648 + mod + SPAN),
                            (2, at + 1_100, at + 5_300), "+", {"planted": True, "t_wide": None, "seeds": seeds, "across": None}))
    out.append(Case("B dotpair beyond, to the last positions", "B", "beyond", "pair", (2, 69_312, None), (0, 199_600 + 37, None), "+",
                    {"planted": False, "t_wide": None, "across": None}))
    # the pair products of A (three planes): chance runs only, so small thresholds; one strand per boundary, a begin per order
    for pins, contig, other, strand in (("2^31", 0, 2, "+"), ("2^32", 1, 0, "-")):
        for swap in (False, True):
            mod = 37 if swap == (strand == "+") else 0
            rows = _straddle(contig, mod)
            order = "columns" if swap else "rows"
            tag = f"{pins} in the {order} {strand} begin%64={mod}"
            pair = (lambda x, y: (y, x)) if swap else (lambda x, y: (x, y))
            a, b = pair(rows, (other, 30_011, 34_211))
            out.append(Case(f"A dotpair {tag}", "A", pins, "pair", a, b, strand, {"planted": False, "t_wide": 64, "across": order}))
            small = (contig, EDGE - 91 if mod == 37 else EDGE - 128, EDGE + 101)
            a, b = pair(small, (other, 30_011, 30_211))
            out.append(Case(f"A dotpair_links (3, 2) {tag}", "A", pins, "links", a, b, strand,
                            {"planted": False, "seeds": (3, 2), "chains_too": True, "across": order}))
    out.append(Case("A dotpair 2^32 against itself", "A", "2^32", "pair", _straddle(1, 0), _straddle(1, 0), "+",
                    {"planted": False, "t_wide": None, "across": "rows", "self": True}))
    for mod, strand in ((37, "-"), (0, "+")):
        out.append(Case(f"A dotpair beyond begin%64={mod}", "A", "beyond", "pair", (2, 20_032 + mod, 20_032 + mod + SPAN), (2, 30_011, 34_211),
                        strand, {"planted": False, "t_wide": 64, "across": None}))
        out.append(Case(f"A dotpair_links (3, 2) beyond begin%64={mod}", "A", "beyond", "links", (2, 20_032 + mod, 20_224 + mod),
                        (2, 30_011, 30_211), strand, {"planted": False, "seeds": (3, 2), "chains_too": True, "across": None}))
    return out


def place_begin(case):
    """The begin of the case's range that lies at the place it pins: the straddling range, or, beyond, the rows' range."""
    return (case.b if case.opt.get("across") == "columns" else case.a)[1]


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)


def far_range(r):
    return None if r is None else (FAR_OF[r[0]],) + tuple(r[1:])


def _length(seqs, r):
    return (len(seqs[r[0]]) if r[2] is None else min(r[2], len(seqs[r[0]]))) - r[1]


def _wide_rows(case, seqs):
    """The window of the rows of the calls at min_diagonal_run 64: 120 rows around EDGE (beyond: around the middle)."""
    n = _length(seqs, case.a)
    mid = EDGE - case.a[1] if case.pins != "beyond" and case.opt.get("across") != "columns" else n // 2
    return (mid - 60, mid + 60)


def calls(g, case, far, seqs):
    """[(label, array)]: every call of the case on genome g.  far: g is the far genome (the ranges' contigs are mapped)."""
    a, b = (far_range(case.a), far_range(case.b)) if far else (case.a, case.b)
    out, opt = [], case.opt
    if case.kind == "period":
        kmin, kmax = opt["k"]
        out.append(("bits", g.period_bits(a[0], kmin, kmax, a[1], a[2])))
        for window in (64, 128):
            out.append((f"counts {window}", g.period_counts(a[0], kmin, kmax, window, a[1], a[2])))
    elif case.kind == "dotplot":
        n = _length(seqs, case.a)
        for t, block in ((2, 128), (3, 64)):
            out.append((f"bits t={t}", g.dotplot_bits(a[0], t, a[1], a[2])))
            out.append((f"counts t={t} block={block}", g.dotplot_counts(a[0], block, t, a[1], a[2])))
        out.append(("bits t=3, a launch per tile of rows", g.dotplot_bits(a[0], 3, a[1], a[2], launch_cells=64 * n)))
        if opt["t_wide"]:
            rows = _wide_rows(case, seqs)
            out.append(("bits t=64", g.dotplot_bits(a[0], opt["t_wide"], a[1], a[2], rows=rows)))
            out.append(("counts t=64 block=64", g.dotplot_counts(a[0], 64, opt["t_wide"], a[1], a[2], rows=rows)))
    elif case.kind == "pchains":
        kmin, kmax = opt["k"]
        for min_seed, max_gap in opt["seeds"]:
            for nm in (False, True):
                out.append((f"chains ({min_seed}, {max_gap}) n_matches={nm}", g.period_chains(a[0], a[1], a[2], kmin, kmax, min_seed, max_gap, n_matches=nm)))
        min_seed, max_gap = opt["seeds"][0]
        out.append(("chains, a launch per span", g.period_chains(a[0], a[1], a[2], kmin, kmax, min_seed, max_gap, launch_cells=64 * 256 * 130)))
    elif case.kind == "pair":
        nb = _length(seqs, case.b)
        for t, block in ((2, 128), (3, 64)):
            out.append((f"bits t={t}", g.dotpair_bits(a, b, case.strand, t)))
            out.append((f"counts t={t} block={block}", g.dotpair_counts(a, b, block, case.strand, t)))
        out.append(("bits t=3, a launch per tile of rows", g.dotpair_bits(a, b, case.strand, 3, launch_cells=64 * nb)))
        if opt["t_wide"]:
            rows = _wide_rows(case, seqs)
            out.append(("bits t=64", g.dotpair_bits(a, b, case.strand, opt["t_wide"], rows=rows)))
            out.append(("counts t=64 block=64", g.dotpair_counts(a, b, 64, case.strand, opt["t_wide"], rows=rows)))
        for min_len in (3, 16, 64):
            out.append((f"runs min_len={min_len}", g.dotpair_runs(a, b, case.strand, "both", min_len)))
        out.append(("runs main", g.dotpair_runs(a, b, case.strand, "main", 5)))
        out.append(("runs anti, a launch per tile of rows", g.dotpair_runs(a, b, case.strand, "anti", 5, launch_cells=64 * nb)))
        if opt.get("self"):
            out.append(("the self plot t=3", g.dotplot_bits(a[0], 3, a[1], a[2])))
    elif case.kind == "chains":
        min_seed, max_gap = opt["seeds"]
        out.append(("chains", g.dotpair_chains(a, b, case.strand, "both", min_seed, max_gap)))
        out.append(("chains min_len=100", g.dotpair_chains(a, b, case.strand, "both", min_seed, max_gap, min_len=100)))
    elif case.kind == "links":
        min_seed, max_gap = opt["seeds"]
        nb = _length(seqs, case.b)
        out.append(("links", g.dotpair_links(a, b, case.strand, "both", min_seed, max_gap, 4)))
        out.append(("links, a launch per tile of rows", g.dotpair_links(a, b, case.strand, "both", min_seed, max_gap, 4, launch_cells=64 * nb)))
        if opt.get("chains_too"):
            out.append(("chains", g.dotpair_chains(a, b, case.strand, "both", min_seed, max_gap)))
    else:
        raise ValueError(case.kind)
    return out


def _crosses(lo, hi, e):
    return bool(np.any((lo < e) & (e <= hi)))


def _list_crosses(rows, case, longer_than=0):
    """A listed run, chain or link of a pair product whose extent crosses EDGE on the side that straddles it."""
    rows = rows[rows["len"] > longer_than] if "len" in rows.dtype.names else rows
    if case.opt["across"] == "rows":
        e = EDGE - case.a[1]
        first = rows["from_row"] if "from_row" in rows.dtype.names else rows["row"]
        last = rows["row"] if "from_row" in rows.dtype.names else rows["row"] + rows["len"] - 1
        return _crosses(first.astype(np.int64), last.astype(np.int64), e)
    e = EDGE - case.b[1]
    col = rows["col"].astype(np.int64)
    if "from_col" in rows.dtype.names:
        other = rows["from_col"].astype(np.int64)
    else:
        other = col + np.where(rows["dir"] == R.ANTI, -1, 1) * (rows["len"].astype(np.int64) - 1)
    return _crosses(np.minimum(col, other), np.maximum(col, other), e)


def _cells_cross(cells, e, axis):
    """A diagonal or anti-diagonal pair of set cells on either side of row (axis 0) or column (axis 1) e of a window's cells."""
    if axis == 1:
        cells = cells.T
    up, down = cells[e - 1], cells[e]
    return bool((up[:-1] & down[1:]).any() or (up[1:] & down[:-1]).any())


@functools.lru_cache(maxsize=None)
def _raw(genome, a, b, strand):
    seqs = near_contigs(genome)
    raw = P.kept_cells(seqs[a[0]], seqs[b[0]], strand, 0, a[1:], b[1:])
    return raw, R.all_runs(raw)


def models(case):
    """[(label, array)] as calls() returns it, from the CPU models; the floors of the case are asserted on the way."""
    seqs = near_contigs(case.genome)
    a, b, opt, out = case.a, case.b, case.opt, []
    beyond = case.pins == "beyond"
    if case.kind == "period":
        kmin, kmax = opt["k"]
        cells = PM.period_cells(seqs[a[0]], kmin, kmax, a[1], a[2])
        out.append(("bits", PM.pack_bits(cells)))
        for window in (64, 128):
            out.append((f"counts {window}", PM.window_sums(cells, window)))
        if beyond:
            assert cells.any()
        else:
            e = EDGE - a[1]
            # a run of set cells on one line across EDGE: four cells either side in B (the tandem repeat), one in A (chance)
            half = 4 if case.genome == "B" else 1
            assert cells[:, e - half:e + half].all(axis=1).any()
            for window in (64, 128):
                w = PM.window_sums(cells, window)
                if e % window:
                    assert w[:, e // window].any()             # the window that holds EDGE - 1 and EDGE
                else:
                    assert w[:, e // window - 1].any() and w[:, e // window].any()
    elif case.kind == "dotplot":
        n = _length(seqs, a)
        kept = {t: D.kept_cells(seqs[a[0]], t, a[1], a[2]) for t in (2, 3)}
        for t, block in ((2, 128), (3, 64)):
            out.append((f"bits t={t}", D.pack_bits(kept[t])))
            out.append((f"counts t={t} block={block}", D.block_sums(kept[t], block)))
        out.append(("bits t=3, a launch per tile of rows", D.pack_bits(kept[3])))
        if opt["t_wide"]:
            rows = _wide_rows(case, seqs)
            wide = D.kept_cells(seqs[a[0]], opt["t_wide"], a[1], a[2], rows=rows)
            out.append(("bits t=64", D.pack_bits(wide)))
            out.append(("counts t=64 block=64", D.block_sums(wide, 64)))
            off = np.ones_like(wide)
            off[np.arange(rows[1] - rows[0]), np.arange(rows[0], rows[1])] = False
            if opt["long_repeat"] is not None:                 # kept cells off the main diagonal: a repeat of 63 cells or more
                assert (wide & off).any() == opt["long_repeat"]
        off = ~np.eye(n, dtype=bool)
        if beyond:
            assert (kept[3] & off).any()
        else:
            assert _cells_cross(kept[3] & off, EDGE - a[1], 0)
    elif case.kind == "pchains":
        kmin, kmax = opt["k"]
        first = None
        for min_seed, max_gap in opt["seeds"]:
            for nm in (False, True):
                want = M.line_chains(seqs[a[0]], nm, kmin, kmax, min_seed, max_gap, a[1], a[2])
                out.append((f"chains ({min_seed}, {max_gap}) n_matches={nm}", want))
                first = want if first is None else first
                assert len(want)
                if opt.get("k_slices"):                        # chains on lines of the last k slice, of three and of eight planes
                    assert bool(np.any(want["k"] > 2_048)) and (min_seed > 3 or bool(np.any(want["k"] <= 1_024)))
                if opt.get("far_k"):                           # the planted copy at distance FAR_K: a chain on a line of the last k slice
                    at = FAR_K_AT - a[1]
                    assert bool(np.any((want["k"] == FAR_K) & (want["start"] <= at) & (want["start"] + want["len"] >= at + FAR_K_LEN)))
                    assert kmax > 2_048 and FAR_K > 2_048
                if not beyond:
                    start, length = want["start"].astype(np.int64), want["len"].astype(np.int64)
                    assert _crosses(start, start + length - 1, EDGE - a[1])
                    if min_seed == 3:                          # starts in each of the three spans of 16 384 positions
                        assert all(bool(np.any(start // 16_384 == span)) for span in (0, 1, 2))
        out.append(("chains, a launch per span", first))
    elif case.kind == "pair":
        raw, every = _raw(case.genome, a, b, case.strand)
        na, nb = raw.shape
        kept3 = P.kept_cells(seqs[a[0]], seqs[b[0]], case.strand, 3, a[1:], b[1:])
        for t, block, cells in ((2, 128, raw), (3, 64, kept3)):
            out.append((f"bits t={t}", P.pack_bits(cells)))
            out.append((f"counts t={t} block={block}", P.block_sums(cells, block)))
        out.append(("bits t=3, a launch per tile of rows", P.pack_bits(kept3)))
        if opt["t_wide"]:
            rows = _wide_rows(case, seqs)
            wide = P.kept_cells(seqs[a[0]], seqs[b[0]], case.strand, opt["t_wide"], a[1:], b[1:], rows=rows)
            out.append(("bits t=64", P.pack_bits(wide)))
            out.append(("counts t=64 block=64", P.block_sums(wide, 64)))
            assert wide.any() or not opt["planted"]            # (chance has no run of 63 cells: there the result is empty, and must be)
        for min_len in (3, 16, 64):
            out.append((f"runs min_len={min_len}", R.select(every, na, nb, min_len=min_len)))
        out.append(("runs main", R.select(every, na, nb, directions="main", min_len=5)))
        out.append(("runs anti, a launch per tile of rows", R.select(every, na, nb, directions="anti", min_len=5)))
        if opt.get("self"):
            out.append(("the self plot t=3", P.pack_bits(kept3)))
        runs3 = R.select(every, na, nb, min_len=3)
        assert len(runs3)
        if a[2] is None and b[2] is None:                      # N up to the last position of both contigs: a run into the corner
            assert bool(np.any((runs3["dir"] == R.MAIN) & (runs3["row"] + runs3["len"] == na) & (runs3["col"] + runs3["len"] == nb)))
        if not beyond:
            assert _list_crosses(runs3, case)
            if opt["planted"]:
                assert _list_crosses(runs3, case, longer_than=1_000)
            e, axis = (EDGE - a[1], 0) if opt["across"] == "rows" else (EDGE - b[1], 1)
            assert _cells_cross(kept3, e, axis)
            counts = P.block_sums(kept3, 64)
            assert counts[e // 64 - 1].any() and counts[e // 64].any() if axis == 0 else counts[:, e // 64 - 1].any() and counts[:, e // 64].any()
    elif case.kind in ("chains", "links"):
        raw, every = _raw(case.genome, a, b, case.strand)
        na, nb = raw.shape
        min_seed, max_gap = opt["seeds"]
        chains = C.all_chains(raw, min_seed, max_gap, every[every["len"] >= min_seed])
        listed = C.select(chains, na, nb)
        if case.kind == "chains":
            out.append(("chains", listed))
            out.append(("chains min_len=100", C.select(chains, na, nb, min_len=100)))
            if opt["planted"]:
                assert len(listed)
            if opt["planted"] and not beyond:                               # the copy with substitutions: chains of several seeds across EDGE
                assert _list_crosses(listed[listed["seeds"] >= 3], case, longer_than=300)
        else:
            links = L.select(L.all_links(chains, nb, min_seed, max_gap, 4), na, nb)
            out.append(("links", links))
            out.append(("links, a launch per tile of rows", links))
            if opt.get("chains_too"):
                out.append(("chains", listed))
                assert len(listed) and (beyond or _list_crosses(listed, case))
            if opt["planted"] or min_seed == 3:
                assert len(links)
                if not beyond:
                    assert _list_crosses(links, case)          # a junction between the cells on either side of EDGE
    else:
        raise ValueError(case.kind)
    return out


def same(got, want):
    """A call's array against the model's: field by field for a list, value by value for a matrix."""
    if want.dtype.names:
        return len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in want.dtype.names)
    return got.shape == want.shape and np.array_equal(got, want)
