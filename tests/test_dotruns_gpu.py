"""GPU (-m gpu): the list of diagonal runs of the dot plot of two ranges (prf_dotpair_runs, csrc/dotruns.hip).  Every
list is compared EXACTLY: with the model (tests/dotruns_model.py, pinned to the reference's filter by tests/test_dotruns_cpu.py)
or with rows known by construction.

Shapes: the fixture's cases (at most 200 x 200); ranges of at most 4 096 x 2 500 either way round, so that both a tile-row
boundary (64 rows) and a span boundary (62 words = 3 968 columns) are crossed; planted runs whose lengths sit around the probe
depth P and the follow limit F (3 F + 17: the long kernel over several wave steps); one 65 536 x 70 001 rectangle, where only
planted copies can reach min_len 200."""
import ctypes
import random

import numpy as np
import pytest

import dotpair_model as P
import dotruns_model as R
from conftest import load_jsonl_gz

pytestmark = pytest.mark.gpu

FIELDS = ("row", "col", "len", "dir")


@pytest.fixture(scope="module")
def ctx():
    import torch  # the same load order as the other GPU tests (torch's HIP runtime first)
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return load_jsonl_gz("dotpair.jsonl.gz")


def _random(n, seed, alphabet=b"ACGT"):
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


def _same(got, want, what=None):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)


def _rows(*runs):
    """A list of (row, col, len, dir) as the calls return it."""
    return np.sort(np.array(list(runs), dtype=R.DTYPE), order=["row", "col", "dir"])


def _raw(seq_a, seq_b, strand, i, j):
    x, y = seq_a[i:i + 1], seq_b[j:j + 1]
    return x == (P.comp(y) if strand == "-" else y)


def _extended(seq_a, seq_b, strand, i, j, n, d):
    """The planted run (i, j, n, d), lengthened at both ends where chance made the neighbouring bases match as well."""
    dj = 1 if d == R.MAIN else -1
    assert all(_raw(seq_a, seq_b, strand, i + s, j + dj * s) for s in (0, n // 2, n - 1))
    while i > 0 and 0 <= j - dj < len(seq_b) and _raw(seq_a, seq_b, strand, i - 1, j - dj):
        i, j, n = i - 1, j - dj, n + 1
    while i + n < len(seq_a) and 0 <= j + dj * n < len(seq_b) and _raw(seq_a, seq_b, strand, i + n, j + dj * n):
        n += 1
    return i, j, n, d


# ---- 1. the fixture ----

def test_every_fixture_case_through_the_one_shot_call(ctx, golden):
    import prf_native
    bad = []
    for c in golden:
        na, nb = len(c["a"]), len(c["b"])
        min_len = max(c["t"] - 1, 1)
        got, st = ctx.dotpair_runs(c["a"], c["b"], c["strand"], "both", min_len, with_stats=True)
        want = R.runs(c["a"], c["b"], c["strand"], min_len=min_len)
        if len(got) != len(want) or any(not np.array_equal(got[f], want[f]) for f in FIELDS) or \
                not np.array_equal(prf_native.run_cells(got, na, nb), P.fixture_cells(c)):
            bad.append(c["tag"])
        assert st.path == 7 and st.positions == na + nb and st.n_hits == len(got)
        assert (st.scan_ms > 0 and st.n_launches >= 1) or not (na and nb)
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


# ---- 2. ranges of three contigs against the model ----

def _contig(n, seed, iupac, pieces):
    """Random ACGT with an N block, the given (position, piece) pairs written over it, N up to its last position (the guard gap
    behind it is N too and must not match) and, with iupac, stretches of letters outside ACGTN."""
    s = bytearray(_random(n, seed))
    s[500:650] = b"N" * 150
    if iupac:
        rng = random.Random(seed + 1)
        for at in (300, 4000, n // 2, n - 100):
            s[at:at + 24] = bytes(rng.choice(b"RYKMSWBVDHN") for _ in range(24))
    for at, piece in pieces:
        s[at:at + len(piece)] = piece
    s[n - 40:] = b"N" * 40
    return bytes(s)


U = _random(300, 7) + b"RYKMBVDHSWN" * 4 + _random(120, 8)                     # 464 letters, IUPAC in the middle
PLANTED = [                                                                   # (row in mid, col in long, len, dir, strand)
    (5_000, 20_000, 20_000, R.MAIN, "+"),                                     # a copy
    (30_000, 49_999, 5_000, R.ANTI, "-"),                                     # reverse-complemented
    (40_000, 60_000, 300, R.MAIN, "-"),                                       # complemented
    (41_000, 61_299, 300, R.ANTI, "+"),                                       # reversed
]


@pytest.fixture(scope="module")
def three_contigs(ctx):
    """100 positions of nothing but N, a contig of 65 536 (ends on a tile boundary of the genome) and one of 70 001 with IUPAC
    letters.  The second holds pieces of the third: copied, reverse-complemented, complemented and reversed (PLANTED), and the
    piece U in all four forms."""
    long_ = _contig(70_001, 50, True, [(3_000, U), (69_500, U[:260])])
    mid = _contig(65_536, 40, False, [(5_000, long_[20_000:40_000]), (30_000, P.revcomp(long_[45_000:50_000])),
                                       (40_000, P.comp(long_[60_000:60_300])), (41_000, long_[61_000:61_300][::-1]),
                                       (50_000, U), (51_000, P.revcomp(U)), (52_000, U[::-1]), (53_000, P.comp(U)),
                                       (65_100, P.revcomp(U[:260]))])
    seqs = [b"N" * 100, mid, long_]
    g = ctx.load(seqs, 64)
    yield g, seqs
    g.free()


# (a, b) of (contig, begin, end): begins off a word on each side independently (a contig starts at a multiple of 65 536 in the
# genome, so a begin's offset within a word of the planes is the begin modulo 64), ends with the contig and inside a copy
SMALL = [((1, 49_990, 50_500), (2, 2_969, 3_500)),          # U against U: 510 x 531, IUPAC letters; 22 and 25 bits off a word
         ((2, 2_944, 3_400), (1, 50_950, 51_500)),          # the other way round against the reverse complement; a begin on a word
         ((2, 69_300, None), (1, 64_900, None)),            # both end with their contigs: N up to the last position
         ((0, 3, 90), (1, 480, 700)),                       # nothing but N against the N block
         ((1, 52_000, 52_464), (2, 3_000, 3_464))]          # the reversed piece: one anti run corner to corner on plus
LARGE = [((1, 4_031, 4_031 + 4_096), (2, 19_001, 19_001 + 2_500)),     # the copy starts inside and leaves through the rectangle's edge
         ((2, 44_000, 44_000 + 2_500), (1, 31_000, 31_000 + 4_096))]   # 2 500 x 4 096: the inverted piece starts at column 3 999, across the span boundary


def _lengths():
    import prf_native
    p = prf_native.DOTRUN_PROBE
    return [1, 2, 3, p - 1, p, p + 1, 64]


@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("which", range(len(SMALL)))
def test_small_ranges_against_the_model(three_contigs, which, strand):
    g, seqs = three_contigs
    a, b = SMALL[which]
    raw = P.kept_cells(seqs[a[0]], seqs[b[0]], strand, 0, a[1:], b[1:])
    every = R.all_runs(raw)
    found = 0
    for min_len in _lengths():
        for directions in ("main", "anti", "both"):
            want = R.select(every, *raw.shape, directions=directions, min_len=min_len)
            _same(g.dotpair_runs(a, b, strand, directions, min_len), want, (a, b, strand, directions, min_len))
            found += len(want)
    assert found > 100                                                        # no vacuous pass


@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("which", range(len(LARGE)))
def test_large_ranges_against_the_model(three_contigs, which, strand):
    import prf_native
    g, seqs = three_contigs
    a, b = LARGE[which]
    raw = P.kept_cells(seqs[a[0]], seqs[b[0]], strand, 0, a[1:], b[1:])
    every = R.all_runs(raw)
    every = every[every["len"] >= 3]
    for min_len in _lengths()[2:]:
        want = R.select(every, *raw.shape, min_len=min_len)
        _same(g.dotpair_runs(a, b, strand, "both", min_len), want, (a, b, strand, min_len))
    for directions in ("main", "anti"):
        _same(g.dotpair_runs(a, b, strand, directions, 5), R.select(every, *raw.shape, directions=directions, min_len=5), directions)
    if which == 0 and strand == "+":                                          # clipped by the rectangle and by nothing else
        assert any(r[3] == R.MAIN and r[1] - r[0] == 30 and r[0] <= 969 and r[1] + r[2] == 2_500 for r in want.tolist())
    if which == 1 and strand == "-":
        assert int(want["len"].max()) >= 1_500 > prf_native.DOTRUN_PROBE and (1_000, 3_999, R.ANTI) in {(r[0] + r[2] - 1_500, r[1] - r[2] + 1_500, r[3]) for r in want.tolist()}


def test_the_all_n_contig_against_itself(three_contigs):
    g, _ = three_contigs
    got = g.dotpair_runs((0, 0, None), (0, 0, None), "+", "both", 1)
    lengths = list(range(1, 101)) + list(range(99, 0, -1))
    main = [(max(0, -k), max(0, k), 100 - abs(k), R.MAIN) for k in range(-99, 100)]
    anti = [(max(0, k - 99), min(k, 99), min(k, 198 - k) + 1, R.ANTI) for k in range(199)]
    assert sorted(r[2] for r in main) == sorted(lengths) and sorted(r[2] for r in anti) == sorted(lengths)
    _same(got, _rows(*main, *anti))
    for strand, directions in (("-", "main"), ("+", "anti")):
        part = g.dotpair_runs((0, 0, None), (0, 0, None), strand, directions, 1)
        assert len(part) == 199 and sorted(part["len"].tolist()) == sorted(lengths)


# ---- 3. where the kernel can go wrong: planted runs ----

def _planted_lengths():
    import prf_native
    p, f = prf_native.DOTRUN_PROBE, prf_native.DOTRUN_FOLLOW
    return [p - 1, p, p + 1, f - 1, f, f + 1, 3 * f + 17]


@pytest.fixture(scope="module")
def bands(ctx):
    """Contig 0: random ACGT (the rows).  Contigs 1 and 2 (the columns, for the plus and for the minus strand): nothing but N --
    which no letter of contig 0 matches -- except one band per planted run, a piece of contig 0 copied (main) or reversed (anti),
    complemented for the minus strand.  Every band has N on both sides, so each planted run is maximal by construction, and the
    bands begin at every offset within a word."""
    lengths = _planted_lengths()
    rows_seq = _random(max(lengths) + 300, 77)
    columns, planted = {}, {}
    for strand in "+-":
        b, runs = bytearray(), []
        for d in (R.MAIN, R.ANTI):
            for k, n in enumerate(lengths):
                b += b"N" * (3 + 11 * k + (5 if d == R.ANTI else 0))
                i = 7 + 37 * k + (64 if d == R.ANTI else 0)
                piece = rows_seq[i:i + n]
                if strand == "-":
                    piece = P.comp(piece)
                runs.append((i, len(b) if d == R.MAIN else len(b) + n - 1, n, d))
                b += piece if d == R.MAIN else piece[::-1]
        b += b"N" * 9
        columns[strand], planted[strand] = bytes(b), runs
    g = ctx.load([rows_seq, columns["+"], columns["-"]], 64)
    yield g, rows_seq, columns, planted
    g.free()


@pytest.mark.parametrize("strand", ["+", "-"])
def test_planted_lengths_around_the_probe_and_the_follow_limit(bands, strand):
    import prf_native
    g, rows_seq, columns, planted = bands
    a, b = (0, 0, None), (1 if strand == "+" else 2, 0, None)
    for i, j, n, d in planted[strand]:
        # the start decides: a window of 3 x 3 cells around it holds this run and, at this length, no other
        rows, cols = (max(0, i - 1), i + 2), (max(0, j - 1), j + 2)
        got, st = g.dotpair_runs(a, b, strand, "both", n, rows, cols, with_stats=True)
        _same(got, _rows((i, j, n, d)), (strand, i, j, n, d))                 # length exactly min_len
        assert st.n_launches == (2 if n >= prf_native.DOTRUN_FOLLOW else 1), n          # the long kernel finishes what F cells did not
        assert len(g.dotpair_runs(a, b, strand, "both", n + 1, rows, cols)) == 0        # length min_len - 1
        other = "anti" if d == R.MAIN else "main"
        assert len(g.dotpair_runs(a, b, strand, other, n, rows, cols)) == 0
    # the whole rectangle at once: chance cannot reach F - 1 cells, so the list is the planted runs of that length
    floor = prf_native.DOTRUN_FOLLOW - 1
    got, st = g.dotpair_runs(a, b, strand, "both", floor, with_stats=True)
    _same(got, _rows(*[r for r in planted[strand] if r[2] >= floor]), strand)
    assert len(got) == 8 and st.n_launches == 2 and st.n_hits == 8
    # ... and on the other strand's columns only chance matches: nothing that long
    assert len(g.dotpair_runs(a, (2 if strand == "+" else 1, 0, None), strand, "both", 40)) == 0
    # the transposed rectangle: the bands are the rows, the long runs start in many tiles
    mirror = [(j if d == R.MAIN else j - n + 1, i if d == R.MAIN else i + n - 1, n, d) for i, j, n, d in planted[strand] if n >= floor]
    _same(g.dotpair_runs(b, a, strand, "both", floor), _rows(*mirror), "transposed")


def _corner_sequences(strand):
    """Two sequences of 333 and 517 letters (the rows, the columns) whose corners hold planted runs of this strand: a[i] is raw
    against tr(a[i]).  Starts at row 0, at column 0 and at column nb - 1, ends exactly at (na, nb) and at column 0, an N block and
    an R... / Y... stretch."""
    tr = P.comp if strand == "-" else bytes
    a, b = bytearray(_random(333, 21)), bytearray(_random(517, 22))
    a[150:170], b[300:330] = b"N" * 20, b"N" * 30         # 20 x 30 cells, all raw on both strands
    a[60:72], b[400:412] = b"R" * 12, b"Y" * 12           # R == comp(Y): raw on the minus strand only
    a[0:16] = a[333 - 16:][::-1]                          # with the tails below: an anti run from (0, nb - 1)
    b[0:30] = tr(a[0:30])                                 # a main run from (0, 0)
    b[100:140] = tr(a[0:40])                              # a main run from row 0
    b[517 - 25:] = tr(a[333 - 25:])                       # a main run that ends at (na, nb): the last position of both
    a[200:235] = tr(b[0:35])                              # a main run from column 0
    a[260:278] = tr(b[0:18])[::-1]                        # an anti run that ends at column 0
    return bytes(a), bytes(b)


@pytest.mark.parametrize("strand", ["+", "-"])
def test_runs_at_the_corners_and_at_the_ends_of_the_planes(ctx, strand):
    """The rows are the LAST contig (a main run that ends at its last position looks ahead behind the planes' last word) and the
    columns are contig 0 from b_begin = 0 (an anti run's backward look reaches in front of the planes); then the other way round."""
    a, b = _corner_sequences(strand)
    g = ctx.load([b, a], 64)
    try:
        for rows_of, cols_of, sa, sb in (((1, 0, None), (0, 0, None), a, b), ((0, 0, None), (1, 0, None), b, a)):
            raw = P.kept_cells(sa, sb, strand, 0)
            every = R.all_runs(raw)
            na, nb = raw.shape
            for min_len in (1, 2, 12, 16, 17):
                want = R.select(every, na, nb, min_len=min_len)
                _same(g.dotpair_runs(rows_of, cols_of, strand, "both", min_len), want, (strand, rows_of[0], min_len))
            # the planted runs are there, seen with a as the rows: the transposed rectangle holds their mirror images
            listed = {tuple(r) for r in R.select(every, na, nb, min_len=12).tolist()}
            if sa is b:
                listed = {(j, i, n, d) if d == R.MAIN else (j - n + 1, i + n - 1, n, d) for i, j, n, d in listed}
            starts = {(r[0], r[1], r[3]) for r in listed}
            ends = {(r[0] + r[2], r[1] + r[2] if r[3] == R.MAIN else r[1] - r[2], r[3]) for r in listed}
            assert {(0, 0, R.MAIN), (0, 100, R.MAIN), (200, 0, R.MAIN), (0, 516, R.ANTI)} <= starts
            assert (333, 517, R.MAIN) in ends and any(e[1] == -1 and e[2] == R.ANTI and 270 <= e[0] <= 285 for e in ends)
            assert any(r[2] == 20 and r[3] == R.MAIN and r[0] == 150 for r in listed)                                 # the N block's diagonals
            assert any(r[3] == R.MAIN and r[1] - r[0] == 340 and r[0] <= 60 and r[0] + r[2] >= 72 for r in listed) == (strand == "-")    # R / Y
    finally:
        g.free()


def test_runs_across_launch_tile_and_span_boundaries(three_contigs):
    g, seqs = three_contigs
    a, b = (2, 44_800, 44_800 + 700), (1, 31_000, 31_000 + 4_096)             # the inverted piece: from (200, 3 999) across eight tile rows and the span boundary
    want = R.runs(seqs[2], seqs[1], "-", a[1:], b[1:], min_len=3)
    one, st1 = g.dotpair_runs(a, b, "-", "both", 3, with_stats=True)
    _same(one, want)
    assert st1.n_launches == 1 and int(want["len"].max()) >= 500
    cut, st = g.dotpair_runs(a, b, "-", "both", 3, with_stats=True, launch_cells=64 * 4_096)      # one tile of rows per launch
    assert st.n_launches == 11 and st.path == 7 and st.positions == 700 + 4_096 and st.n_hits == len(want)
    _same(cut, want)
    cut, st = g.dotpair_runs(a, b, "-", "both", 3, with_stats=True, launch_cells=3 * 64 * 4_096 + 5)
    assert st.n_launches == 4
    _same(cut, want)
    cut, st = g.dotpair_runs(a, b, "-", "both", 3, with_stats=True, launch_cells=1)              # never less than a tile
    assert st.n_launches == 11
    _same(cut, want)


# ---- 4. long ranges ----

@pytest.mark.parametrize("strand", ["+", "-"])
def test_whole_contigs_hold_the_planted_copies_and_nothing_else(three_contigs, strand):
    g, seqs = three_contigs
    want = _rows(*[_extended(seqs[1], seqs[2], strand, i, j, n, d) for i, j, n, d, s in PLANTED if s == strand],
                 *[_extended(seqs[1], seqs[2], strand, i, j, 260, d) for i, j, d, s in
                   ((50_000, 3_000, R.MAIN, "+"), (52_000 + 164, 3_000 + 299, R.ANTI, "+"),     # U and its mirror images: the first 300
                    (53_000, 3_000, R.MAIN, "-"), (51_000 + 164, 3_000 + 299, R.ANTI, "-"),
                    (50_000, 69_500, R.MAIN, "+"), (52_000 + 204, 69_500 + 259, R.ANTI, "+"),    # ... and the 260 at the contig's end
                    (53_000, 69_500, R.MAIN, "-"), (51_000 + 204, 69_500 + 259, R.ANTI, "-"),
                    (65_100, 3_259, R.ANTI, "-"), (65_100, 69_759, R.ANTI, "-")) if s == strand])
    got, st = g.dotpair_runs((1, 0, None), (2, 0, None), strand, "both", 200, with_stats=True)
    _same(got, want, strand)
    assert st.positions == 65_536 + 70_001 and st.n_hits == len(want) and st.scan_ms > 0
    assert int(got["len"].max()) >= (20_000 if strand == "+" else 5_000)


# ---- 5. capacity, windows, identity, determinism, neighbours ----

def _call(g, a, b, strand, directions, min_len, capacity, dst, rows=(0, 1 << 62), cols=(0, 1 << 62)):
    import prf_native
    n, st = ctypes.c_uint64(0), prf_native.ScanStats()
    rc = g.ctx.lib.prf_dotpair_runs(g.ctx._h, g._h, a[0], a[1], a[2], b[0], b[1], b[2], strand, rows[0], rows[1], cols[0], cols[1],
                                    directions, min_len, None if dst is None else dst.ctypes.data, capacity, ctypes.byref(n), ctypes.byref(st))
    assert rc == prf_native.PRF_OK, g.ctx.lib.prf_last_error()
    return n.value, st


def test_capacity_counts_fills_or_leaves_the_destination_alone(three_contigs):
    import prf_native
    g, seqs = three_contigs
    a, b = (1, 49_990, 50_500), (2, 2_969, 3_500)
    want = R.runs(seqs[1], seqs[2], "+", a[1:], b[1:], min_len=4)
    n = len(want)
    assert n > 300
    assert _call(g, a, b, 0, 3, 4, 0, None)[0] == n                            # counting only
    dst = np.full(n + 8, 0xEE, dtype=np.uint8).repeat(32).view(prf_native.DOTRUN_DTYPE)
    sentinel = dst.copy()
    count, st = _call(g, a, b, 0, 3, 4, n - 1, dst)
    assert count == n and st.n_hits == n and np.array_equal(dst.view(np.uint8), sentinel.view(np.uint8))      # untouched
    assert _call(g, a, b, 0, 3, 4, n, dst)[0] == n                             # exactly enough: filled
    _same(dst[:n], want)
    assert (dst["reserved"][:n] == 0).all() and np.array_equal(dst[n:].view(np.uint8), sentinel[n:].view(np.uint8))
    # the binding's second call: more runs than its first call has room for
    many = g.dotpair_runs((1, 10_000, 10_700), (2, 10_000, 10_600), "+", "both", 1)
    assert len(many) > prf_native.DOTRUN_DEFAULT_CAPACITY
    _same(many, R.runs(seqs[1], seqs[2], "+", (10_000, 10_700), (10_000, 10_600)))
    rc = g.ctx.lib.prf_dotpair_runs(g.ctx._h, g._h, 1, 0, 10, 3, 0, 10, 0, 0, 10, 0, 10, 3, 2, None, 0, ctypes.byref(ctypes.c_uint64(0)), None)
    assert rc == prf_native.PRF_EINVAL and "contig 3" in g.ctx.lib.prf_last_error().decode()


def test_windows_add_up_to_the_whole_list(three_contigs):
    g, seqs = three_contigs
    a, b = (2, 2_944, 3_400), (1, 50_950, 51_500)                             # 456 x 550, U against its reverse complement
    whole = g.dotpair_runs(a, b, "-", "both", 3)
    _same(whole, R.runs(seqs[2], seqs[1], "-", a[1:], b[1:], min_len=3))
    for row_cuts, col_cuts in (((0, 131, 9_999), (0, 257, None)), ((0, 64, 300, 456), (0, None))):             # 2 x 2 and 3 x 1
        parts = [g.dotpair_runs(a, b, "-", "both", 3, rows=(r0, r1), cols=(c0, c1))
                 for r0, r1 in zip(row_cuts, row_cuts[1:]) for c0, c1 in zip(col_cuts, col_cuts[1:])]
        assert all(len(p) for p in parts)
        _same(np.sort(np.concatenate(parts), order=["row", "col", "dir"]), whole, row_cuts)                  # each once, unclipped
    long_run = whole[np.argmax(whole["len"])]
    assert long_run["len"] >= 400 and long_run["dir"] == R.ANTI
    i, j = int(long_run["row"]) + 150, int(long_run["col"]) - 150            # a window that holds only the middle of it
    assert len(g.dotpair_runs(a, b, "-", "both", 100, rows=(i, i + 60), cols=(j - 60, j))) == 0
    _same(g.dotpair_runs(a, b, "-", "both", 100, rows=(int(long_run["row"]), i), cols=(j, None)), whole[whole["len"] >= 100])


@pytest.mark.parametrize("strand", ["+", "-"])
def test_run_cells_equal_the_bits_kernel(three_contigs, strand):
    import prf_native
    g, _ = three_contigs
    a, b = LARGE[0] if strand == "+" else LARGE[1]
    na, nb = a[2] - a[1], b[2] - b[1]
    for t in (3, 5, 19, 64):
        runs = g.dotpair_runs(a, b, strand, "both", t - 1)
        kept = prf_native.unpack_bits(g.dotpair_bits(a, b, strand, t), nb).astype(bool)
        assert kept.any() and np.array_equal(prf_native.run_cells(runs, na, nb), kept), t


def test_two_calls_give_equal_arrays(three_contigs):
    g, _ = three_contigs
    a, b = LARGE[1]
    first = g.dotpair_runs(a, b, "-", "both", 2)
    assert len(first) > 100_000 and np.array_equal(first, g.dotpair_runs(a, b, "-", "both", 2))


def test_scans_period_counts_and_bits_are_not_disturbed(ctx):
    import torch
    import prf_native
    tile = prf_native.tile_positions()
    seq = bytearray(_random(3 * tile + 500, 13))
    for at in range(1000, len(seq) - 200, 9_973):
        seq[at:at + 60] = b"CAG" * 20
    seq = bytes(seq)
    seqs = [seq, _random(900, 14)]
    g = ctx.load(seqs, 50)
    cap = 100_000
    buf = torch.empty((cap + 1, 3), dtype=torch.int64, device="cuda")
    try:
        g.select([(0, tile, 3 * tile)])
        ctx.set_row_sink(buf.data_ptr(), cap)
        before, _ = g.scan(1, 50, 3, 9)
        sink_before = buf.cpu().numpy().copy()
        period_before = g.period_counts(0, 1, 50, 1024)
        bits_before = g.dotpair_bits((0, 900, 1_300), (1, 0, None), "-", 3)
        runs = g.dotpair_runs((0, 900, 1_300), (1, 0, None), "-", "both", 3)                     # whatever is selected
        _same(runs, R.runs(seq, seqs[1], "-", (900, 1_300), (0, None), min_len=3))
        tandem = g.dotpair_runs((0, 1_000, 1_100), (0, 1_000 + 9_973, 1_100 + 9_973), "+", "main", 50)
        assert any(r[0] == 0 and r[1] == 0 and r[2] >= 60 for r in tandem.tolist())
        assert np.array_equal(buf.cpu().numpy(), sink_before)                 # nothing was written to the sink
        assert np.array_equal(g.period_counts(0, 1, 50, 1024), period_before)
        assert np.array_equal(g.dotpair_bits((0, 900, 1_300), (1, 0, None), "-", 3), bits_before)
        after, _ = g.scan(1, 50, 3, 9)
        assert len(before) > 10 and np.array_equal(before, after)
        assert before["start"].min() >= tile and before["start"].max() < 3 * tile
        assert np.array_equal(buf.cpu().numpy(), sink_before)
    finally:
        ctx.set_row_sink(None, 0)
        g.select([])
        g.free()


def test_cli_writes_the_runs_of_two_intervals(ctx, tmp_path):
    import plot_dot_plot as cli
    u = _random(150, 41)
    chrom = (_random(3_000, 14) + u + b"N" * 200 + _random(5_000, 15)).decode()
    other = (_random(400, 16) + P.revcomp(u) + _random(250, 17)).decode()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\n" + other + "\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    tsv = tmp_path / "runs.tsv"
    cli.main(["-R", str(fa), "chrT:100-8000", "--versus", "other:300-700", "--strand", "both", "--runs-tsv", str(tsv), "--min-run", "100",
              "-d", str(tmp_path)], context=ctx)                               # 7 900 positions: no --block needed without an image
    i, j, n, _ = _extended(chrom[100:8000].encode(), other[300:700].encode(), "-", 2_900, 100 + 149, 150, R.ANTI)
    assert tsv.read_text() == f"chrT\t{100 + i}\t{100 + i + n}\tother\t{300 + j - n + 1}\t{300 + j + 1}\t-\tanti\t{n}\n"
    assert not list(tmp_path.glob("*.png"))
    cli.main([chrom[2_950:3_100] + "ACGTTGCA" + chrom[3_000:3_150], "--runs-tsv", str(tsv), "--min-run", "60", "-d", str(tmp_path)], context=ctx)
    lines = tsv.read_text().splitlines()
    seq = (chrom[2_950:3_100] + "ACGTTGCA" + chrom[3_000:3_150]).encode()
    i, j, n, _ = _extended(seq, seq, "+", 50, 158, 100, R.MAIN)
    assert lines == [f"sequence\t{i}\t{i + n}\tsequence\t{j}\t{j + n}\t+\tmain\t{n}"]
