"""GPU (-m gpu): the list of chained diagonal runs of the dot plot of two ranges (prf_dotpair_chains, csrc/dotchain.hip, DESIGN
14).  Every list is compared EXACTLY: with the model (tests/dotchain_model.py, pinned to a brute force by
tests/test_dotchain_cpu.py) or with rows known by construction.

Shapes: the fixture's cases (at most 200 x 200); the ranges of the three-contig genome of tests/test_dotruns_gpu.py (at most
4 096 x 2 500 either way round: a tile-row boundary and the span boundary are crossed; IUPAC letters: the 8-plane kernels);
planted chains in a genome of ACGT and N (the 3-plane kernels), each a copied piece with single bases changed, as main and anti
lines on both strands, looked at through windows of 3 x 3 cells around their starts."""
import ctypes
import random
import re

import numpy as np
import pytest

import dotchain_model as C
import dotpair_model as P
import dotruns_model as R
from conftest import load_jsonl_gz
from test_dotruns_gpu import LARGE, SMALL, U, _contig, _random

pytestmark = pytest.mark.gpu

PAIRS = [(1, 0), (2, 1), (3, 2), (4, 8), (8, 16)]             # (min_seed, max_gap): the fixture
RANGE_PAIRS = [(11, 5), (16, 64), (17, 4096)]                 # the ranges of the three contigs


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
    cases = load_jsonl_gz("dotpair.jsonl.gz")
    for c in cases:                                            # the raw cells and their runs once, for the five pairs
        c["raw"] = P.kept_cells(c["a"], c["b"], c["strand"], 0)
        c["every"] = R.all_runs(c["raw"])
    return cases


def _same(got, want, what=None):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in C.FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)


def _rows(*chains):
    """A list of (row, col, len, matches, dir, seeds) as the calls return it."""
    return np.sort(np.array(list(chains), dtype=C.DTYPE), order=["row", "col", "dir"])


# ---- 1. the fixture ----

@pytest.mark.parametrize("min_seed,max_gap", PAIRS)
def test_every_fixture_case_through_the_one_shot_call(ctx, golden, min_seed, max_gap):
    bad, joined = [], 0
    assert len(golden) == 159
    for c in golden:
        na, nb = c["raw"].shape
        got, st = ctx.dotpair_chains(c["a"], c["b"], c["strand"], "both", min_seed, max_gap, with_stats=True)
        want = C.select(C.all_chains(c["raw"], min_seed, max_gap, c["every"]), na, nb)
        if not C.same(got, want):
            bad.append(c["tag"])
        joined += int((want["seeds"] >= 2).sum())
        assert st.path == 8 and st.positions == na + nb and st.n_hits == len(got)
        assert st.n_candidates == int((c["every"]["len"] >= min_seed).sum())
        assert (st.scan_ms > 0 and st.n_launches >= 1) or not (na and nb)
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"
    assert joined >= (1000 if max_gap in (1, 2, 8) else 8 if max_gap else 0)


# ---- 2. ranges of three contigs against the model ----

@pytest.fixture(scope="module")
def three_contigs(ctx):
    """The genome of tests/test_dotruns_gpu.py: 100 positions of nothing but N, a contig of 65 536 and one of 70 001 with IUPAC
    letters; the second holds pieces of the third copied, reverse-complemented, complemented and reversed."""
    long_ = _contig(70_001, 50, True, [(3_000, U), (69_500, U[:260])])
    mid = _contig(65_536, 40, False, [(5_000, long_[20_000:40_000]), (30_000, P.revcomp(long_[45_000:50_000])),
                                       (40_000, P.comp(long_[60_000:60_300])), (41_000, long_[61_000:61_300][::-1]),
                                       (50_000, U), (51_000, P.revcomp(U)), (52_000, U[::-1]), (53_000, P.comp(U)),
                                       (65_100, P.revcomp(U[:260]))])
    seqs = [b"N" * 100, mid, long_]
    g = ctx.load(seqs, 64)
    yield g, seqs
    g.free()


@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("which", range(len(SMALL)))
def test_small_ranges_against_the_model(three_contigs, which, strand):
    g, seqs = three_contigs
    a, b = SMALL[which]
    raw = P.kept_cells(seqs[a[0]], seqs[b[0]], strand, 0, a[1:], b[1:])
    every = R.all_runs(raw)
    found = joined = 0
    for min_seed, max_gap in RANGE_PAIRS + [(3, 2), (5, 40)]:                 # the last two: many chains of several seeds
        chains = C.all_chains(raw, min_seed, max_gap, every)
        for directions in ("main", "anti", "both"):
            want = C.select(chains, *raw.shape, directions=directions)
            _same(g.dotpair_chains(a, b, strand, directions, min_seed, max_gap), want, (a, b, strand, directions, min_seed, max_gap))
        found, joined = found + len(want), joined + int((want["seeds"] >= 2).sum())
        floor = 3 * min_seed                                                  # min_len filters on the span
        _same(g.dotpair_chains(a, b, strand, "both", min_seed, max_gap, floor), want[want["len"] >= floor], ("min_len", min_seed, max_gap))
    assert found > 100 and (joined > 20 or which == 3)                        # no vacuous pass (N against N: every line is one run)
    # max_gap = 0: the list of runs, row for row
    for min_seed, min_len in ((1, 0), (4, 0), (4, 9), (9, 4), (16, 0), (17, 17)):
        runs = g.dotpair_runs(a, b, strand, "both", max(min_seed, min_len))
        got = g.dotpair_chains(a, b, strand, "both", min_seed, 0, min_len)
        assert R.same(got, runs) and np.array_equal(got["matches"], got["len"]) and (got["seeds"] == 1).all(), (min_seed, min_len)


@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("which", range(len(LARGE)))
def test_large_ranges_against_the_model(three_contigs, which, strand):
    g, seqs = three_contigs
    a, b = LARGE[which]
    raw = P.kept_cells(seqs[a[0]], seqs[b[0]], strand, 0, a[1:], b[1:])
    every = R.all_runs(raw)
    every = every[every["len"] >= 5]
    for min_seed, max_gap in RANGE_PAIRS + [(5, 3)]:
        chains = C.all_chains(raw, min_seed, max_gap, every)
        for directions in ("both",) if min_seed != 11 else ("main", "anti", "both"):
            want = C.select(chains, *raw.shape, directions=directions)
            _same(g.dotpair_chains(a, b, strand, directions, min_seed, max_gap), want, (a, b, strand, directions, min_seed, max_gap))
    assert len(want) > 1_000 and int((want["seeds"] >= 2).sum()) > 20          # at (5, 3)
    if which == 0 and strand == "+":                                          # the copy leaves through the rectangle's edge
        assert any(r[4] == R.MAIN and r[1] - r[0] == 30 and r[0] <= 969 and r[1] + r[2] == 2_500 for r in want.tolist())


def test_the_all_n_contig_against_itself(three_contigs):
    g, _ = three_contigs
    main = [(max(0, -k), max(0, k), 100 - abs(k), 100 - abs(k), R.MAIN, 1) for k in range(-99, 100)]
    anti = [(max(0, k - 99), min(k, 99), min(k, 198 - k) + 1, min(k, 198 - k) + 1, R.ANTI, 1) for k in range(199)]
    for strand in "+-":                                                       # N == N on both strands: every line is one exact run
        _same(g.dotpair_chains((0, 0, None), (0, 0, None), strand, "both", 1, 7), _rows(*main, *anti), strand)
        _same(g.dotpair_chains((0, 0, None), (0, 0, None), strand, "both", 60, 4096), _rows(*[r for r in main + anti if r[2] >= 60]))
    assert len(g.dotpair_chains((0, 0, None), (0, 0, None), "+", "anti", 3, 1, 98)) == 5


# ---- 3. where the kernels can go wrong: planted chains ----

S, G = 16, 5                                                  # min_seed, max_gap of the planted chains, unless a case says otherwise
FRONT = 9_300                                                 # N in front of and behind the bands: a band's line cell t is its row


def _pattern_cells(pattern):
    return "".join(("1" if kind == "m" else "0") * n for kind, n in pattern)


def _chains_of(text, min_seed, max_gap):
    """[(first cell, cells, matches, seeds, cells of the first seed)] of one line given as a string of 0 and 1."""
    out = []
    for m in re.finditer("1+", text):
        if m.end() - m.start() < min_seed:
            continue
        if out and m.start() - out[-1][1] - 1 <= max_gap:
            out[-1][1], out[-1][2] = m.end() - 1, out[-1][2] + 1
        else:
            out.append([m.start(), m.end() - 1, 1, m.end() - m.start()])
    return [(s, e - s + 1, text[s:e + 1].count("1"), seeds, first) for s, e, seeds, first in out]


def _of_length(cells, long_run_at=None):
    """A pattern of exactly `cells` cells: seeds of 40 and 37 cells one to three mismatches apart; long_run_at: an exact run of
    2 500 cells from about that cell on."""
    pattern, used = [("m", 40), ("x", 3)], 43
    while cells - used > 90:
        if long_run_at is not None and used >= long_run_at and cells - used > 2_600:
            pattern += [("m", 2_500), ("x", 1)]
            used, long_run_at = used + 2_501, None
        else:
            pattern += [("m", 37), ("x", 1 + used % 3)]
            used += 38 + used % 3
    return pattern + [("m", cells - used)]


def _cases():
    import prf_native
    f = prf_native.DOTCHAIN_FOLLOW
    return {                                                   # name: (row of the first cell, pattern, min_seed, max_gap)
        "gap of exactly max_gap": (300, [("m", S), ("x", G), ("m", S)], S, G),
        "gap of max_gap + 1": (410, [("m", S), ("x", G + 1), ("m", S)], S, G),
        "a short run inside the gap": (500, [("m", S), ("x", 2), ("m", S - 1), ("x", 2), ("m", S)], S, S + 3),
        "a short run behind the last seed": (600, [("m", S), ("x", 2), ("m", S), ("x", 2), ("m", S - 1)], S, G),
        "a gap across a word of the line": (40, [("m", 22), ("x", 4), ("m", 20)], S, G),
        "a gap across a tile row": (100, [("m", 26), ("x", 4), ("m", 20), ("x", 5), ("m", 60)], S, G),
        "a first seed of F + 5 cells": (900, [("m", f + 5), ("x", 2), ("m", 20), ("x", 6), ("m", 16)], S, G),
        "a gap of 4 096": (800, [("m", 20), ("x", 4_096), ("m", 17), ("x", 4_097), ("m", 30)], 17, 4_096),
        "F - 1 cells": (7, _of_length(f - 1), S, G),
        "F cells": (33, _of_length(f), S, G),
        "F + 1 cells": (64, _of_length(f + 1), S, G),
        "F + 38 cells: the walk ends a cell short of the hand-over": (1_003, _of_length(f + 38), S, G),
        "F + 39 cells: handed over at the last cell": (1_101, _of_length(f + 39), S, G),
        "F + 41 cells": (1_250, _of_length(f + 41), S, G),
        "3 F + 17 cells": (131, _of_length(3 * f + 17), S, G),
        "3 F + 17 cells, handed over inside a run": (1, _of_length(3 * f + 17, 1_500), S, G),
    }


@pytest.fixture(scope="module")
def bands(ctx):
    """Contig 0: random ACGT (the rows).  Contigs 1 and 2 (the columns, for the plus and for the minus strand): nothing but N --
    which no letter of contig 0 matches -- except one band per case and direction: a piece of contig 0 with the bases at the
    pattern's x cells changed, copied (main) or reversed (anti), complemented for the minus strand.  Every band has N on both sides,
    so no run leaves its band.  planted[strand][name, dir] = (row, col of the band's first cell of the line)."""
    cases = _cases()
    rows_seq = _random(FRONT, 78)
    change = bytes.maketrans(b"ACGT", b"CGTA")
    columns, planted = {}, {}
    for strand in "+-":
        b, where = bytearray(b"N" * FRONT), {}
        for d in (R.MAIN, R.ANTI):
            for k, (name, (i, pattern, _s, _g)) in enumerate(cases.items()):
                cells = _pattern_cells(pattern)
                assert i + len(cells) <= len(rows_seq)
                piece = bytes(x if c == "1" else x.to_bytes(1, "big").translate(change)[0] for x, c in zip(rows_seq[i:i + len(cells)], cells))
                if strand == "-":
                    piece = P.comp(piece)
                b += b"N" * (3 + 11 * k + (5 if d == R.ANTI else 0))
                where[name, d] = (i, len(b) if d == R.MAIN else len(b) + len(cells) - 1)
                b += piece if d == R.MAIN else piece[::-1]
        b += b"N" * FRONT
        columns[strand], planted[strand] = bytes(b), where
    g = ctx.load([rows_seq, columns["+"], columns["-"]], 64)
    yield g, planted
    g.free()


def _expected(i, j, d, pattern, min_seed, max_gap):
    dj = 1 if d == R.MAIN else -1
    return [(i + s, j + dj * s, n, m, d, seeds) for s, n, m, seeds, _first in _chains_of(_pattern_cells(pattern), min_seed, max_gap)]


def _handed_over(t0, cells, first_seed, max_gap):
    """The link kernel's thread stops where its cursor is F cells behind the first seed (cell t0 + first_seed + F) or further
    and the chain is not complete.  The cursor passes the cell behind the last seed's mismatch, e + 2, and then, over the
    mismatches behind a band, every multiple of 64 up to e + max_gap + 1, where the look for another seed ends."""
    import prf_native
    e, stop = t0 + cells - 1, t0 + first_seed + prf_native.DOTCHAIN_FOLLOW
    return e + 2 >= stop or (e + max_gap + 1) // 64 * 64 >= stop


@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("d", [R.MAIN, R.ANTI])
def test_planted_chains_through_windows_around_their_starts(bands, strand, d):
    import prf_native
    g, planted = bands
    a, b = (0, 0, None), (1 if strand == "+" else 2, 0, None)
    for name, (i, pattern, min_seed, max_gap) in _cases().items():
        i, j = planted[strand][name, d]
        want = _expected(i, j, d, pattern, min_seed, max_gap)
        assert want and want[0][:2] == (i, j), name
        first_seeds = [c[4] for c in _chains_of(_pattern_cells(pattern), min_seed, max_gap)]
        for k, chain in enumerate(want):
            # the start decides: a window of 3 x 3 cells around it holds this chain and no other, whatever lies outside it
            rows, cols = (max(0, chain[0] - 1), chain[0] + 2), (chain[1] - 1, chain[1] + 2)
            got, st = g.dotpair_chains(a, b, strand, "both", min_seed, max_gap, rows=rows, cols=cols, with_stats=True)
            _same(got, _rows(chain), (strand, d, name, k))
            # launches: the seed kernel, the seeds' long kernel for a first seed of F cells, the link kernel, and the chains' long
            # kernel where the walk is handed over
            long_seed = first_seeds[k] >= prf_native.DOTRUN_FOLLOW
            handed_over = _handed_over(chain[0], chain[2], first_seeds[k], max_gap)
            assert st.n_candidates == 1 and st.n_launches == 2 + long_seed + handed_over, (name, k, st.n_launches)
            assert len(g.dotpair_chains(a, b, strand, "both", min_seed, max_gap, chain[2] + 1, rows=rows, cols=cols)) == 0   # min_len
            _same(g.dotpair_chains(a, b, strand, "both", min_seed, max_gap, chain[2], rows=rows, cols=cols), _rows(chain))
            other = "anti" if d == R.MAIN else "main"
            assert len(g.dotpair_chains(a, b, strand, other, min_seed, max_gap, rows=rows, cols=cols)) == 0
        # a seed in the window whose predecessor lies outside it is not a start: windows around the later seeds of the chains
        dj = 1 if d == R.MAIN else -1
        starts = {c[0] for c in want}
        at = 0
        for kind, n in pattern[:40]:
            if kind == "m" and n >= min_seed and i + at not in starts:
                rows, cols = (i + at - 1, i + at + 2), (j + dj * at - 1, j + dj * at + 2)
                got, st = g.dotpair_chains(a, b, strand, "both", min_seed, max_gap, rows=rows, cols=cols, with_stats=True)
                assert len(got) == 0 and st.n_candidates == 1, (name, at)
            at += n
    assert planted[strand]["gap of max_gap + 1", d] and len(_expected(0, 9_000, d, _cases()["gap of max_gap + 1"][1], S, G)) == 2
    for name, matches, cells in (("a short run inside the gap", 3 * S - 1, 3 * S + 3), ("a short run behind the last seed", 2 * S, 2 * S + 2)):
        i, pattern, min_seed, max_gap = _cases()[name]
        only, = _expected(0, 9_000, d, pattern, min_seed, max_gap)
        assert only[2:4] == (cells, matches) and only[5] == 2


@pytest.mark.parametrize("strand", ["+", "-"])
def test_chains_across_launch_and_tile_boundaries(bands, strand):
    g, planted = bands
    a, b = (0, 0, None), (1 if strand == "+" else 2, 0, None)
    for d in (R.MAIN, R.ANTI):
        for name in ("a gap across a tile row", "3 F + 17 cells"):
            i, pattern, min_seed, max_gap = _cases()[name]
            i, j = planted[strand][name, d]
            want = _rows(*_expected(i, j, d, pattern, min_seed, max_gap))
            n_cells = len(_pattern_cells(pattern))
            assert len(want) == 1
            rows, cols = (max(0, i - 1), i + n_cells), (j - 1, j + 2)          # a strip of 3 columns over the chain's tile rows
            whole, st1 = g.dotpair_chains(a, b, strand, "both", min_seed, max_gap, rows=rows, cols=cols, with_stats=True)
            _same(whole, want, (name, d))
            cut, st = g.dotpair_chains(a, b, strand, "both", min_seed, max_gap, rows=rows, cols=cols, with_stats=True,
                                       launch_cells=64 * (cols[1] - cols[0]))                     # one tile of rows per launch
            _same(cut, want, (name, d, "cut"))
            assert st.n_launches - st1.n_launches == -(-(rows[1] - rows[0]) // 64) - 1 and st.n_candidates == st1.n_candidates


def _diverged(piece, every, tr=bytes):
    """tr(piece) with every `every`-th base changed to one that does not match (letters outside ACGT stay)."""
    out = bytearray(piece)
    for at in range(every - 1, len(out), every):
        if out[at] in b"ACGT":
            out[at] = b"ACGT"[(b"ACGT".index(out[at]) + 1) % 4]
    return tr(bytes(out))


def _corner_sequences(strand):
    """Two sequences of 333 and 517 letters (the rows, the columns) with diverged copies in the corners of their rectangle:
    chains from (0, 0), from row 0, from column 0, up to (na, nb), an anti chain from (0, nb - 1) and one down to column 0; an N
    block and an R / Y stretch inside a chain."""
    tr = P.comp if strand == "-" else bytes
    a, b = bytearray(_random(333, 23)), bytearray(_random(517, 24))
    a[95:101], a[110:116] = b"NNNNNN", b"RRYYRY"                # inside a[80:130]
    a[0:24] = a[333 - 24:][::-1]                                # with b's tail below: an anti chain from (0, nb - 1)
    b[0:40] = _diverged(a[0:40], 7, tr)                         # a main chain from (0, 0)
    b[100:140] = _diverged(a[0:40], 9, tr)                      # from row 0
    b[150:200] = _diverged(a[80:130], 13, tr)                   # through the N block and the R / Y stretch: changed at 92, 105, 118
    b[517 - 33:] = _diverged(a[333 - 33:], 7, tr)               # up to (na, nb): the last position of both
    a[200:245] = _diverged(tr(bytes(b[0:45])), 11)              # from column 0 (tr is its own inverse)
    a[260:284] = _diverged(tr(bytes(b[0:24]))[::-1], 9)         # an anti chain that ends at column 0
    return bytes(a), bytes(b)


@pytest.mark.parametrize("strand", ["+", "-"])
def test_chains_at_the_corners_and_at_the_ends_of_the_planes(ctx, strand):
    """The rows are the LAST contig (a look ahead behind the planes' last word) and the columns contig 0 from b_begin = 0 (an anti
    line's look backwards reaches in front of the planes); then the other way round.  IUPAC letters: the 8-plane kernels."""
    a, b = _corner_sequences(strand)
    g = ctx.load([b, a], 64)
    try:
        for rows_of, cols_of, sa, sb in (((1, 0, None), (0, 0, None), a, b), ((0, 0, None), (1, 0, None), b, a)):
            raw = P.kept_cells(sa, sb, strand, 0)
            every = R.all_runs(raw)
            na, nb = raw.shape
            for min_seed, max_gap in ((1, 1), (2, 1), (3, 2), (4, 3), (5, 64), (6, 4096)):
                want = C.select(C.all_chains(raw, min_seed, max_gap, every), na, nb)
                _same(g.dotpair_chains(rows_of, cols_of, strand, "both", min_seed, max_gap), want, (strand, rows_of[0], min_seed, max_gap))
            listed = C.select(C.all_chains(raw, 4, 3, every), na, nb, min_len=22).tolist()
            if sa is b:                                                       # seen with a as the rows
                listed = [(j, i, n, m, d, s) if d == R.MAIN else (j - n + 1, i + n - 1, n, m, d, s) for i, j, n, m, d, s in listed]
            joined = [r for r in listed if r[5] >= 2 and r[3] < r[2]]
            starts = {(r[0], r[1], r[4]) for r in joined}
            ends = {(r[0] + r[2], r[1] + r[2] if r[4] == R.MAIN else r[1] - r[2], r[4]) for r in joined}
            assert {(0, 0, R.MAIN), (0, 100, R.MAIN), (200, 0, R.MAIN), (0, 516, R.ANTI)} <= starts, starts
            assert (333, 517, R.MAIN) in ends and any(e[1] == -1 and e[2] == R.ANTI and 270 <= e[0] <= 290 for e in ends)
            assert any(r[4] == R.MAIN and r[1] - r[0] == 70 and r[0] <= 92 and r[0] + r[2] >= 119 and r[5] >= 4 for r in joined)    # N block, R / Y
    finally:
        g.free()


# ---- 4. capacity, windows, determinism, neighbours ----

def _call(g, a, b, strand, directions, min_seed, max_gap, min_len, capacity, dst, rows=(0, 1 << 62), cols=(0, 1 << 62)):
    import prf_native
    n, st = ctypes.c_uint64(0), prf_native.ScanStats()
    rc = g.ctx.lib.prf_dotpair_chains(g.ctx._h, g._h, a[0], a[1], a[2], b[0], b[1], b[2], strand, rows[0], rows[1], cols[0], cols[1],
                                      directions, min_seed, max_gap, min_len, None if dst is None else dst.ctypes.data, capacity,
                                      ctypes.byref(n), ctypes.byref(st))
    assert rc == prf_native.PRF_OK, g.ctx.lib.prf_last_error()
    return n.value, st


def test_capacity_counts_fills_or_leaves_the_destination_alone(three_contigs):
    import prf_native
    g, seqs = three_contigs
    a, b = (1, 49_990, 50_500), (2, 2_969, 3_500)
    want = C.chains(seqs[1], seqs[2], "+", 4, 3, 0, a[1:], b[1:])
    n = len(want)
    assert n > 300 and int((want["seeds"] >= 2).sum()) > 10
    assert _call(g, a, b, 0, 3, 4, 3, 0, 0, None)[0] == n                      # counting only
    dst = np.full(n + 8, 0xEE, dtype=np.uint8).repeat(40).view(prf_native.DOTCHAIN_DTYPE)
    sentinel = dst.copy()
    count, st = _call(g, a, b, 0, 3, 4, 3, 0, n - 1, dst)
    assert count == n and st.n_hits == n and np.array_equal(dst.view(np.uint8), sentinel.view(np.uint8))      # untouched
    assert _call(g, a, b, 0, 3, 4, 3, 0, n, dst)[0] == n                       # exactly enough: filled
    _same(dst[:n], want)
    assert np.array_equal(dst[n:].view(np.uint8), sentinel[n:].view(np.uint8))
    # the binding's second call: more chains than its first call has room for
    many = g.dotpair_chains((1, 10_000, 10_700), (2, 10_000, 10_600), "+", "both", 1, 1)
    assert len(many) > prf_native.DOTCHAIN_DEFAULT_CAPACITY
    _same(many, C.chains(seqs[1], seqs[2], "+", 1, 1, 0, (10_000, 10_700), (10_000, 10_600)))
    rc = g.ctx.lib.prf_dotpair_chains(g.ctx._h, g._h, 1, 0, 10, 3, 0, 10, 0, 0, 10, 0, 10, 3, 2, 1, 0, None, 0, ctypes.byref(ctypes.c_uint64(0)), None)
    assert rc == prf_native.PRF_EINVAL and "contig 3" in g.ctx.lib.prf_last_error().decode()


def test_more_seeds_than_the_first_pass_has_room_for(ctx):
    """The seeds are written into 2^20 rows of room at first and once more into the exact number (grow_once, csrc/list_host.h).
    At min_seed = 1 every run start of the window is a seed, 3/16 per cell and direction of random ACGT: 1 800 x 1 900 cells hold
    1.28 million, a fifth above 2^20.  Without gaps a chain is its seed, and min_len keeps the list short."""
    seqs = [_random(1_800, 61), _random(1_900, 62)]
    g = ctx.load(seqs, 64)
    try:
        got, st = g.dotpair_chains((0, 0, None), (1, 0, None), "+", "both", 1, 0, 6, with_stats=True)
    finally:
        g.free()
    assert st.n_candidates > 1 << 20
    want = C.chains(seqs[0], seqs[1], "+", 1, 0, 6)
    assert len(want) > 1_000 and st.n_hits == len(want)
    _same(got, want)


def test_windows_add_up_to_the_whole_list(three_contigs):
    g, seqs = three_contigs
    a, b = (2, 2_944, 3_400), (1, 50_950, 51_500)                             # 456 x 550, U against its reverse complement
    whole = g.dotpair_chains(a, b, "-", "both", 3, 2)
    _same(whole, C.chains(seqs[2], seqs[1], "-", 3, 2, 0, a[1:], b[1:]))
    assert int((whole["seeds"] >= 2).sum()) > 100
    for row_cuts, col_cuts in (((0, 131, 9_999), (0, 257, None)), ((0, 64, 300, 456), (0, None))):             # 2 x 2 and 3 x 1
        parts = [g.dotpair_chains(a, b, "-", "both", 3, 2, rows=(r0, r1), cols=(c0, c1))
                 for r0, r1 in zip(row_cuts, row_cuts[1:]) for c0, c1 in zip(col_cuts, col_cuts[1:])]
        assert all(len(p) for p in parts)
        _same(np.sort(np.concatenate(parts), order=["row", "col", "dir"]), whole, row_cuts)                  # each once, unclipped


def test_two_calls_give_equal_arrays(three_contigs):
    g, _ = three_contigs
    a, b = LARGE[1]
    first = g.dotpair_chains(a, b, "-", "both", 2, 1)
    assert len(first) > 100_000 and np.array_equal(first, g.dotpair_chains(a, b, "-", "both", 2, 1))


def test_scans_runs_and_bits_are_not_disturbed(ctx):
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
        runs_before = g.dotpair_runs((0, 900, 1_300), (1, 0, None), "-", "both", 3)
        bits_before = g.dotpair_bits((0, 900, 1_300), (1, 0, None), "-", 3)
        chains = g.dotpair_chains((0, 900, 1_300), (1, 0, None), "-", "both", 3, 2)            # whatever is selected
        _same(chains, C.chains(seq, seqs[1], "-", 3, 2, 0, (900, 1_300), (0, None)))
        tandem = g.dotpair_chains((0, 1_000, 1_100), (0, 1_000 + 9_973, 1_100 + 9_973), "+", "main", 20, 4, 50)
        assert any(r[0] == 0 and r[1] == 0 and r[2] >= 60 for r in tandem.tolist())
        assert np.array_equal(buf.cpu().numpy(), sink_before)                 # nothing was written to the sink
        assert np.array_equal(g.dotpair_runs((0, 900, 1_300), (1, 0, None), "-", "both", 3), runs_before)
        assert np.array_equal(g.dotpair_bits((0, 900, 1_300), (1, 0, None), "-", 3), bits_before)
        after, _ = g.scan(1, 50, 3, 9)
        assert len(before) > 10 and np.array_equal(before, after)
        assert before["start"].min() >= tile and before["start"].max() < 3 * tile
        assert np.array_equal(buf.cpu().numpy(), sink_before)
    finally:
        ctx.set_row_sink(None, 0)
        g.select([])
        g.free()


def test_cli_writes_the_chains_of_two_intervals(ctx, tmp_path):
    import plot_dot_plot as cli
    u = _random(150, 41)
    v = _diverged(u, 30)                                                      # bases 29, 59, 89, 119, 149 changed: runs of 29 cells
    chrom = (_random(3_000, 14) + u + b"N" * 200 + _random(5_000, 15)).decode()
    other = (_random(400, 16) + P.revcomp(v) + _random(250, 17)).decode()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\n" + other + "\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    tsv = tmp_path / "chains.tsv"
    cli.main(["-R", str(fa), "chrT:100-8000", "--versus", "other:300-700", "--strand", "both", "--chains-tsv", str(tsv), "--min-seed", "20",
              "--max-gap", "2", "--min-chain", "100", "-d", str(tmp_path)], context=ctx)         # 7 900 positions: no --block needed without an image
    want = C.chains(chrom[100:8000], other[300:700], "-", 20, 2, 100)
    assert len(want) == 1 and want["seeds"][0] == 5 and want["dir"][0] == R.ANTI
    i, j, n, m = (int(want[f][0]) for f in ("row", "col", "len", "matches"))
    assert 145 <= m == n - 4 and 2_900 - 5 <= i <= 2_900
    assert tsv.read_text() == f"chrT\t{100 + i}\t{100 + i + n}\tother\t{300 + j - n + 1}\t{300 + j + 1}\t-\tanti\t{n}\t{m}\t5\t{m / n:.4f}\n"
    assert not list(tmp_path.glob("*.png"))
    cli.main(["-R", str(fa), "chrT:100-8000", "--versus", "other:300-700", "--strand", "-", "--chains-tsv", str(tsv), "--min-seed", "20",
              "--max-gap", "2", "--min-chain", "100", "--min-identity", "0.99", "-d", str(tmp_path)], context=ctx)
    assert tsv.read_text() == ""
    seq = u.decode() + "ACGTTGCA" + v.decode()                                # without --versus: each repeat once
    cli.main([seq, "--chains-tsv", str(tsv), "--min-seed", "20", "--max-gap", "2", "--min-chain", "90", "-d", str(tmp_path)], context=ctx)
    only = C.chains(seq, seq, "+", 20, 2, 90)
    only = only[only["col"] > only["row"]]
    assert len(only) == 1 and only["seeds"][0] == 5
    i, j, n, m = (int(only[f][0]) for f in ("row", "col", "len", "matches"))
    assert tsv.read_text().splitlines() == [f"sequence\t{i}\t{i + n}\tsequence\t{j}\t{j + n}\t+\tmain\t{n}\t{m}\t5\t{m / n:.4f}"]
