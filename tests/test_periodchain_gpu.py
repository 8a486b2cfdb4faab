"""GPU (-m gpu): the list of chains on the period lines of one range (prf_period_chains, csrc/periodchain.hip).  Every
list is compared EXACTLY: with the model (tests/periodchain_model.py, pinned to a brute force and to the reference's rows by
tests/test_periodchain_cpu.py), with prf_dotpair_chains of the same range against itself, with rows known by construction, or
with the rows of the pinned perfect scan.

Shapes: the fixture's 276 sequences (at most 195 positions); ranges of up to 8 192 positions of the three-contig genome of
tests/test_dotruns_gpu.py (IUPAC letters: the 8-plane kernels); planted lines in a genome of ACGT and N (the 3-plane kernels:
40 000 positions so that the span boundary at 32 768 is crossed, 12 000 positions x 2 100 lines so that the k-slice boundary at
2 048 is) and in one with R / Y stretches (20 000 positions: the 8-plane span boundary at 16 384); the 1 Mbp synthetic contig."""
import ctypes
import random
import re

import numpy as np
import pytest

import periodchain_model as M
from conftest import load_json, load_jsonl_gz
from test_dotruns_gpu import U, _contig, _random

pytestmark = pytest.mark.gpu

PAIRS = [(1, 0), (2, 1), (3, 2), (4, 8), (8, 16)]             # (min_seed, max_gap): the fixture
RANGE_PAIRS = [(11, 5), (16, 64), (17, 4096)]                 # the ranges of the three contigs
F = 2048                                                      # PRF_DOTCHAIN_FOLLOW


@pytest.fixture(scope="module")
def ctx():
    import torch  # the same load order as the other GPU tests (torch's HIP runtime first)
    assert torch.cuda.is_available()
    import prf_native
    assert prf_native.DOTCHAIN_FOLLOW == F
    c = prf_native.Context(0)
    yield c
    c.close()


def _same(got, want, what=None):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in M.FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)


# ---- 1. the fixture ----

@pytest.fixture(scope="module")
def modelled():
    """[(sequence, {(n_matches, min_seed, max_gap): every chain of lines 1 .. 64, sorted})], computed once."""
    seen = {}
    for c in load_jsonl_gz("dotpair.jsonl.gz"):
        for s in (c["a"], c["b"]):
            seen.setdefault(s, None)
    out = []
    for s in seen:
        want = {}
        for nm in (0, 1):
            raw = M.band_cells(s, nm, 1, 64)
            every = M.runs_of(raw)
            for pair in PAIRS:
                want[(nm, *pair)] = M.all_chains(raw, *pair, every)
        out.append((s, want))
    return out


@pytest.mark.parametrize("n_matches", [0, 1])
@pytest.mark.parametrize("min_seed,max_gap", PAIRS)
def test_every_fixture_sequence_through_the_one_shot_call(ctx, modelled, min_seed, max_gap, n_matches):
    bad, joined, total = [], 0, 0
    assert len(modelled) == 276
    for at, (s, wants) in enumerate(modelled):
        want = wants[n_matches, min_seed, max_gap]
        got, st = ctx.period_chains(s, 1, 64, min_seed, max_gap, n_matches=bool(n_matches), with_stats=True)
        if not M.same(got, want):
            bad.append(at)
        total, joined = total + len(want), joined + int((want["seeds"] >= 2).sum())
        assert st.path == 10 and st.positions == len(s) and st.n_hits == len(got) == len(want)
        assert st.n_candidates == int(want["seeds"].sum())                    # every seed of a line belongs to one chain
        assert (st.scan_ms > 0 and st.n_launches >= 1 and st.scan_ms == pytest.approx(st.phase1_ms + st.phase2_ms)) or len(s) < 2
    assert not bad, f"{len(bad)} sequences differ: {bad[:5]}"
    floors = {1: {(1, 0): (206_096, 0), (2, 1): (57_502, 7_606), (3, 2): (22_729, 2_494), (4, 8): (9_618, 1_503), (8, 16): (1_754, 12)},
              0: {(1, 0): (197_550, 0), (2, 1): (51_732, 6_093), (3, 2): (18_475, 1_878), (4, 8): (7_171, 1_080), (8, 16): (1_150, 6)}}
    assert total >= floors[n_matches][min_seed, max_gap][0] and joined >= floors[n_matches][min_seed, max_gap][1]


# ---- 2. the same lists as prf_dotpair_chains of the range against itself ----

@pytest.fixture(scope="module")
def three_contigs(ctx):
    """The genome of tests/test_dotruns_gpu.py: 100 positions of nothing but N, a contig of 65 536 and one of 70 001 with IUPAC
    letters (U holds RYKMBVDHSWN four times: lines 11, 22 and 33)."""
    import dotpair_model as P
    long_ = _contig(70_001, 50, True, [(3_000, U), (69_500, U[:260])])
    mid = _contig(65_536, 40, False, [(5_000, long_[20_000:40_000]), (30_000, P.revcomp(long_[45_000:50_000])),
                                       (40_000, P.comp(long_[60_000:60_300])), (41_000, long_[61_000:61_300][::-1]),
                                       (50_000, U), (51_000, P.revcomp(U)), (52_000, U[::-1]), (53_000, P.comp(U)),
                                       (65_100, P.revcomp(U[:260]))])
    seqs = [b"N" * 100, mid, long_]
    g = ctx.load(seqs, 64)
    yield g, seqs
    g.free()


BAND_RANGES = [(1, 0, 8_192),                   # from position 0 of a contig; the N block at 500 .. 650: lines 1 .. 149
               (2, 37, 8_192),                  # begin % 64 = 37; IUPAC stretches, U with its period of 11 in IUPAC letters
               (2, 70_001 - 8_000, None),       # ends the last contig: IUPAC, then N up to the last position
               (1, 49_990, 55_000),             # U and its three other forms
               (0, 0, None), (0, 3, 90)]        # nothing but N: every line is one run


@pytest.mark.parametrize("which", range(len(BAND_RANGES)))
def test_the_band_of_the_dot_plot_of_a_range_with_itself(three_contigs, which):
    g, seqs = three_contigs
    contig, begin, end = BAND_RANGES[which]
    n = len(seqs[contig][begin:end])
    found = 0
    for min_seed, max_gap in RANGE_PAIRS:
        square = g.dotpair_chains((contig, begin, end), (contig, begin, end), "+", "main", min_seed, max_gap)
        for kmin, kmax in ((1, n + 5), (1, 200), (7, 2_500)):
            line = square["col"].astype(np.int64) - square["row"].astype(np.int64)
            band = square[(line >= kmin) & (line <= kmax)]
            want = np.zeros(len(band), dtype=M.DTYPE)
            want["start"], want["len"], want["matches"], want["seeds"] = band["row"], band["len"], band["matches"], band["seeds"]
            want["k"] = band["col"] - band["row"]
            want = np.sort(want, order=["start", "k"])
            got = g.period_chains(contig, begin, end, kmin, kmax, min_seed, max_gap, n_matches=True)
            _same(got, want, (which, min_seed, max_gap, kmin, kmax))
            found += len(want)
    # no vacuous pass: N == N gives a run of 150 - k cells on every line k of the N block, n - k cells in the all-N contig
    assert found >= (3 * 3 * 100 if which == 0 else 3 * 2 * (n - 20) if which >= 4 else 15), found
    if which >= 4:                                              # and N never matches under the scans' rule
        assert len(g.period_chains(contig, begin, end, 1, n + 5, 1, 0, n_matches=False)) == 0
        every = g.period_chains(contig, begin, end, 1, n + 5, 1, 0, n_matches=True)
        assert every.tolist() == [(0, n - k, n - k, k, 1) for k in range(1, n)]


# ---- 3. planted lines ----

def _draw(seq, at, k, pattern):
    """Cells at .. at + len(pattern) - 1 of line k of the contig become `pattern`: position at + k + t repeats position at + t or not."""
    for t, c in enumerate(pattern):
        here = seq[at + t]
        seq[at + k + t] = here if c == "1" else b"ACGT"[(b"ACGT".index(here) + 1 + t % 3) % 4]


def _pattern_chains(pattern, min_seed, max_gap):
    """(first cell, len, matches, seeds) of the chains of a line that reads `pattern`, by the definition."""
    out, chain = [], None
    for m in list(re.finditer("1+", pattern)) + [None]:
        if m is not None and m.end() - m.start() < min_seed:
            continue
        if m is not None and chain is not None and m.start() - chain[1] - 1 <= max_gap:
            chain[1], chain[2] = m.end() - 1, chain[2] + 1
            continue
        if chain is not None:
            out.append((chain[0], chain[1] - chain[0] + 1, pattern[chain[0]:chain[1] + 1].count("1"), chain[2]))
        chain = None if m is None else [m.start(), m.end() - 1, 1]
    return out


def _long_pattern(cells):
    """A chain of exactly `cells` cells at (12, 8): runs of 100 cells, one mismatch between two of them, a seed at the end."""
    p = ["1"] * cells
    for at in range(100, cells - 12, 101):
        p[at] = "0"
    return "".join(p)


S, G = 12, 8
EDGE = "0" * (G + 1)
# seeds of exactly min_seed and min_seed - 1 cells, gaps of exactly max_gap and max_gap + 1: two chains, of 2 seeds and of 1
P1 = EDGE + "1" * S + "0" * G + "1" * S + "0" * (G + 1) + "1" * (S - 1) + "0" * G + "1" * S + EDGE
assert _pattern_chains(P1, S, G) == [(9, 32, 24, 2), (69, 12, 12, 1)]
PLANTED0 = [(5, 64 * 5 - 30, P1),                # (k, first cell, pattern) in contig 0: across a 64-cell word
            (9, 32_768 - 40, P1),               # across the span boundary of a range that begins at 0
            (63, 1_000, P1), (64, 1_200, P1), (65, 1_400, P1), (127, 1_600, P1), (128, 1_900, P1),
            (70, 2_300, EDGE + _long_pattern(F - 1) + EDGE), (71, 4_600, EDGE + _long_pattern(F) + EDGE),
            (72, 6_900, EDGE + _long_pattern(F + 1) + EDGE), (73, 9_200, EDGE + _long_pattern(3 * F + 17) + EDGE),
            (74, 15_600, EDGE + "1" * (F + 500) + "000" + "1" * 40 + EDGE),      # a first seed longer than F
            (75, 18_500, EDGE + "1" * (5 * F) + EDGE),                         # one run of 5 F cells
            (3, 0, "1" * 20 + EDGE)]                                           # a seed at t = 0
LEN0, LEN2 = 40_000, 12_000


@pytest.fixture(scope="module")
def planted(ctx):
    """A genome of ACGT and N: contig 0 with PLANTED0 and a chain that ends on the last cell of line 6; contig 1 nothing but N;
    contig 2, the last, with patterns on lines 2 048 and 2 049 and a repeat of period 7 with 5 000 N in the middle."""
    c0 = bytearray(_random(LEN0, 71))
    for k, at, pattern in PLANTED0:
        _draw(c0, at, k, pattern)
    last0 = EDGE + "1" * 15                                                    # ... ending on cell n - k - 1 of line 6
    _draw(c0, LEN0 - 6 - len(last0), 6, last0)
    c2 = bytearray(_random(LEN2, 72))
    unit = b"ACGGTCA"
    for at in list(range(600, 1_200)) + list(range(6_200, 6_800)):
        c2[at] = unit[(at - 600) % 7]
    c2[1_200:6_200] = b"N" * 5_000
    for k, at in ((2_048, 7_000), (2_049, 7_200)):
        _draw(c2, at, k, P1)
    seqs = [bytes(c0), b"N" * 300, bytes(c2)]
    g = ctx.load(seqs, 64)
    yield g, seqs
    g.free()


def _expected(planted_lines, begin, min_seed, max_gap):
    return {(at - begin + a, n, m, k, s) for k, at, pattern in planted_lines for a, n, m, s in _pattern_chains(pattern, min_seed, max_gap)}


@pytest.mark.parametrize("begin,end", [(0, None), (37, None), (64, 33_000)])
def test_planted_lines_in_the_first_contig(planted, begin, end):
    g, seqs = planted
    s = seqs[0]
    for nm in (False, True):
        got, st = g.period_chains(0, begin, end, 1, 130, S, G, n_matches=nm, with_stats=True)
        _same(got, M.line_chains(s, nm, 1, 130, S, G, begin, end), (begin, end, nm))
        rows = set(got.tolist())
        lines = [p for p in PLANTED0 if p[1] >= begin and (end is None or p[1] + len(p[2]) + p[0] <= end)]
        assert len(lines) >= 12 and _expected(lines, begin, S, G) <= rows
        assert st.n_launches >= 2                                              # the long kernel ran: chains and a run beyond F cells
    if end is None:
        n = LEN0 - begin
        assert (n - 6 - 15, 15, 15, 6, 1) in rows                              # ends on the line's last cell
    if begin == 0:
        assert (0, 20, 20, 3, 1) in rows                                       # starts with the line
        assert {(2_309, F - 1, F - 1 - 20, 70, 21), (4_609, F, F - 20, 71, 21), (6_909, F + 1, F + 1 - 20, 72, 21),
                (9_209, 3 * F + 17, 3 * F + 17 - 60, 73, 61), (15_609, F + 543, F + 540, 74, 2), (18_509, 5 * F, 5 * F, 75, 1)} <= rows


@pytest.mark.parametrize("min_seed,max_gap", [(12, 8), (13, 8), (12, 7), (11, 9), (1, 0)])
def test_thresholds_around_the_planted_seeds_and_gaps(planted, min_seed, max_gap):
    g, seqs = planted
    begin, end = 200, 2_200                                                    # the P1 lines of k = 5, 63, 64, 65, 127, 128
    got = g.period_chains(0, begin, end, 1, 130, min_seed, max_gap)
    _same(got, M.line_chains(seqs[0], 0, 1, 130, min_seed, max_gap, begin, end), (min_seed, max_gap))
    lines = [p for p in PLANTED0 if p[2] is P1 and begin <= p[1] and p[1] + len(p[2]) + p[0] <= end]
    assert len(lines) == 6 and _expected(lines, begin, min_seed, max_gap) <= set(got.tolist())
    if (min_seed, max_gap) == (11, 9):                                          # the short run is a seed now and every gap links
        assert _pattern_chains(P1, 11, 9) == [(9, 72, 47, 4)]


def test_lines_at_and_beyond_the_ends_of_a_short_range(planted):
    g, seqs = planted
    for contig, begin, end in ((0, 1_000, 1_300), (0, 0, 200), (2, LEN2 - 211, None), (0, 77, 78), (0, 5, 5)):
        n = len(seqs[contig][begin:end])
        for kmin, kmax in ((1, n + 5), (n - 1, n - 1), (n, n), (n + 5, n + 5), (max(1, n - 3), n + 5)):
            if kmin < 1:
                continue
            for nm in (False, True):
                got = g.period_chains(contig, begin, end, kmin, kmax, 1, 0, n_matches=nm)
                _same(got, M.line_chains(seqs[contig], nm, kmin, kmax, 1, 0, begin, end), (contig, begin, end, kmin, kmax, nm))
                assert kmin < n or len(got) == 0


def test_the_last_contig_k_slices_and_an_n_block_inside_a_repeat(planted):
    g, seqs = planted
    s = seqs[2]
    for nm in (False, True):
        got = g.period_chains(2, 0, None, 1, 2_100, S, G, n_matches=nm)
        _same(got, M.line_chains(s, nm, 1, 2_100, S, G), nm)
        rows = set(got.tolist())
        assert _expected([(2_048, 7_000, P1), (2_049, 7_200, P1)], 0, S, G) <= rows   # the last line of a k slice and the first of the next
        seven = [r for r in got.tolist() if r[3] == 7 and 500 < r[0] < 6_800 and r[1] > 100]
        if nm:                                                                 # 593 cells, 7 of base against N, 4 993 of N == N, 7, 593: one chain
            assert len(seven) == 1 and seven[0][1] >= 6_193 and seven[0][4] == 3 and seven[0][1] - seven[0][2] == 14
        else:                                                                  # 5 007 cells without a match: two chains
            assert len(seven) == 2 and all(r[1] >= 593 and r[4] == 1 for r in seven)
    # a slice of its own, and a window that begins behind every start
    _same(g.period_chains(2, 0, None, 2_049, 2_100, S, G), got_k := M.select(M.line_chains(s, 0, 1, 2_100, S, G), LEN2, kmin=2_049))
    assert len(got_k) >= 2
    assert len(g.period_chains(2, 0, None, 1, 2_100, S, G, positions=(LEN2 - 1, None))) == 0
    # the contig of nothing but N
    assert len(g.period_chains(1, 0, None, 1, 400, 1, 0)) == 0
    assert g.period_chains(1, 0, None, 1, 400, S, G, n_matches=True).tolist() == [(0, 300 - k, 300 - k, k, 1) for k in range(1, 300 - S + 1)]


def test_stretches_of_r_and_y_through_the_eight_plane_kernels(ctx):
    rng = random.Random(5)
    s = bytearray(_random(20_000, 73))
    s[300:420] = b"N" * 120
    unit = b"RYRRY"
    for at in range(16_384 - 150, 16_384 + 150):                               # across the span boundary of the 8-plane kernels
        s[at] = unit[at % 5]
    s[16_384 + 20] = ord("R") if s[16_384 + 20] != ord("R") else ord("Y")
    for at in (5_000, 5_100, 9_000):                                           # R / Y noise: chance matches among IUPAC letters and with N
        s[at:at + 60] = bytes(rng.choice(b"RYN") for _ in range(60))
    _draw(s, 12_000, 33, P1)
    s = bytes(s)
    g = ctx.load([s], 64)
    try:
        for begin, end in ((0, None), (29, 19_000)):
            for nm in (False, True):
                for min_seed, max_gap in ((S, G), (4, 3)):
                    got = g.period_chains(0, begin, end, 1, 70, min_seed, max_gap, n_matches=nm)
                    _same(got, M.line_chains(s, nm, 1, 70, min_seed, max_gap, begin, end), (begin, end, nm, min_seed, max_gap))
                rows = set(g.period_chains(0, begin, end, 1, 70, S, G, n_matches=nm).tolist())
                assert _expected([(33, 12_000, P1)], begin, S, G) <= rows
                five = [r for r in rows if r[3] == 5 and r[1] > 200]
                assert len(five) == 1 and five[0][4] == 2 and five[0][1] - five[0][2] <= 2      # the R / Y repeat, joined across the change
                assert any(r[3] == 1 and r[1] == 119 for r in rows) == nm       # the N block matches itself only if asked to
    finally:
        g.free()


# ---- 4. partitions, launches, capacity, determinism ----

def test_windows_and_periods_add_up_and_launches_do_not_matter(planted):
    g, seqs = planted
    begin = 37
    whole, st = g.period_chains(0, begin, None, 1, 130, 4, 8, with_stats=True)
    _same(whole, M.line_chains(seqs[0], 0, 1, 130, 4, 8, begin), "whole")
    assert len(whole) > 10_000 and int((whole["seeds"] >= 2).sum()) > 100
    inside = 9_209 - begin + 3_000                                             # a cell inside the chain of 3 F + 17 cells
    for cuts, k_cuts in (((0, inside, None), (1, 73, 131)),                    # 2 x 2: cut inside a chain, and between lines 72 and 73
                         ((0, 64, inside, 32_768 - begin, None), (1, 131)),
                         ((0, None), (1, 2, 64, 65, 70, 71, 129, 131))):         # 1 x 7
        parts = [g.period_chains(0, begin, None, ka, kb - 1, 4, 8, positions=(p0, p1))
                 for p0, p1 in zip(cuts, cuts[1:]) for ka, kb in zip(k_cuts, k_cuts[1:])]
        assert all(len(p) for p in parts)
        _same(np.sort(np.concatenate(parts), order=["start", "k"]), whole, cuts)                             # each once, unclipped
    assert st.n_launches <= 2
    for cells in (1, 64 * 512 * 130, 64 * 512 * 130 + 1):                      # one span of 512 words x 130 lines per launch
        cut, st_cut = g.period_chains(0, begin, None, 1, 130, 4, 8, with_stats=True, launch_cells=cells)
        assert np.array_equal(cut, whole) and st_cut.n_launches == st.n_launches + 1 and st_cut.n_candidates == st.n_candidates
    assert np.array_equal(g.period_chains(0, begin, None, 1, 130, 4, 8), whole)                               # two calls, equal bytes
    assert whole.tobytes() == g.period_chains(0, begin, None, 1, 130, 4, 8).tobytes()
    floor = 40
    _same(g.period_chains(0, begin, None, 1, 130, 4, 8, min_len=floor), whole[whole["len"] >= floor], "min_len")


def test_capacity_and_counting(ctx, planted):
    import prf_native as pn
    g, _ = planted
    want = g.period_chains(0, 0, 5_000, 1, 130, S, G)
    n = len(want)
    assert n > 5
    for capacity, written in ((n - 1, False), (0, False), (n, True), (n + 3, True)):
        buf = np.full(max(1, capacity + 1), 0xAB, dtype=np.uint8).repeat(32)
        found, stats = ctypes.c_uint64(0), pn.ScanStats()
        rc = ctx.lib.prf_period_chains(ctx._h, g._h, 0, 0, 5_000, 0, 5_000, 1, 130, 0, S, G, 0, buf.ctypes.data if capacity else None, capacity,
                                       ctypes.byref(found), ctypes.byref(stats))
        assert rc == pn.PRF_OK and found.value == n == stats.n_hits
        if written:
            assert buf[:32 * n].tobytes() == want.tobytes() and (buf[32 * n:] == 0xAB).all()
        else:
            assert (buf == 0xAB).all()


# ---- 5. the pinned perfect scan ----

def test_the_rows_of_the_perfect_scan_are_in_the_list(ctx):
    golden = load_json("synth_n1000000_seed22_k1-50.json")
    g = ctx.synth([1_000_000], [22], 50)
    try:
        rows, _ = g.scan(1, 50, 3, 9)
        assert [(int(a), int(b), int(k)) for a, b, k in zip(rows["start"], rows["end"], rows["k"])] == [(a, b, len(m)) for a, b, m in golden["rows"]]
        got = g.period_chains(0, 0, None, 1, 50, 8, 0, n_matches=False)
        listed = set(got.tolist())
        long_rows = [(int(a), int(b - a - k), int(b - a - k), int(k), 1) for a, b, k in zip(rows["start"], rows["end"], rows["k"]) if b - a - k >= 8]
        assert len(long_rows) == 47 and set(long_rows) <= listed
        assert (got["matches"] == got["len"]).all() and (got["seeds"] == 1).all() and (got["len"] >= 8).all() and len(got) > 300
    finally:
        g.free()


# ---- 6. the neighbours are not disturbed; the command line ----

def test_scans_and_the_other_products_are_not_disturbed(ctx):
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
        bits_before = g.period_bits(0, 1, 20, 900, 1_300)
        chains_before = g.dotpair_chains((0, 900, 1_300), (1, 0, None), "-", "both", 3, 2)
        links_before = g.dotpair_links((0, 900, 1_300), (1, 0, None), "-", "both", 3, 2, 2)
        got = g.period_chains(0, 0, 3_000, 1, 50, 20, 4, min_len=50)              # whatever is selected
        _same(got, M.select(M.line_chains(seq, 0, 1, 50, 20, 4, 0, 3_000), 3_000, min_len=50))
        assert any(r[0] <= 1_000 and r[3] == 3 and r[1] >= 57 for r in got.tolist())
        assert len(ctx.period_chains(seq[:2_000], 1, 50, 20, 4)) >= 1               # and the one-shot form, a genome of its own
        assert np.array_equal(buf.cpu().numpy(), sink_before)                 # nothing was written to the sink
        assert np.array_equal(g.period_bits(0, 1, 20, 900, 1_300), bits_before)
        assert np.array_equal(g.dotpair_chains((0, 900, 1_300), (1, 0, None), "-", "both", 3, 2), chains_before)
        assert np.array_equal(g.dotpair_links((0, 900, 1_300), (1, 0, None), "-", "both", 3, 2, 2), links_before)
        after, _ = g.scan(1, 50, 3, 9)
        assert len(before) > 10 and np.array_equal(before, after)
        assert before["start"].min() >= tile and before["start"].max() < 3 * tile
        assert np.array_equal(buf.cpu().numpy(), sink_before)
    finally:
        ctx.set_row_sink(None, 0)
        g.select([])
        g.free()


def test_cli_writes_the_repeats_of_an_interval(ctx, tmp_path):
    import plot_periodicity_matrix as cli
    import prf_native as pn
    unit = b"ACGGTCA"
    body = bytearray(unit * 40)
    for at in (33, 90, 151, 200, 260):
        body[at] = ord("T") if body[at] != ord("T") else ord("G")
    chrom = (_random(3_000, 14) + bytes(body) + b"N" * 200 + _random(5_000, 15)).decode().lower()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\nACGT\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    tsv = tmp_path / "repeats.tsv"
    base = [str(fa), "-i", "chrT:100-8000", "--max-motif-size", "40", "--chains-tsv", str(tsv), "--min-seed", "10", "--max-gap", "8"]

    def lines(chains, drop=True, identity=0.0):
        rows = pn.tandem_rows(chains, drop_multiples=drop)
        return [f"chrT\t{100 + a}\t{100 + b}\t{k}\t{c:.3f}\t{i:.4f}\t{m}\t{s}\t{chrom[100 + a:100 + a + k].upper()}"
                for a, b, k, c, i, m, s in rows.tolist() if i >= identity]

    def model(min_len=0, nm=0):
        found = M.select(M.line_chains(chrom, nm, 1, 40, 10, 8, 100, 8_000), 7_900, min_len=min_len)
        out = np.zeros(len(found), dtype=pn.PCHAIN_DTYPE)
        for f in M.FIELDS:
            out[f] = found[f]
        return out

    cli.main(base + ["--min-chain", "100", "--chain-window", "1000"], context=ctx)       # 7 900 positions in 8 windows, no image
    want = lines(model(100))
    assert tsv.read_text().splitlines() == want
    seven = [line.split("\t") for line in want if line.split("\t")[3] == "7"]          # the repeat: one line of period 7
    assert len(seven) == 1 and int(seven[0][1]) <= 3_000 and int(seven[0][2]) == 3_280 and len(seven[0][8]) == 7 and int(seven[0][7]) >= 5
    assert not any(line.split("\t")[3] in ("14", "21", "28") for line in want)          # its images inside it are gone
    assert not list(tmp_path.glob("*.png"))
    cli.main(base + ["--min-chain", "100", "--keep-multiples"], context=ctx)
    kept = lines(model(100), drop=False)
    assert tsv.read_text().splitlines() == kept and len(kept) > len(want)
    cli.main(base + ["--min-chain", "100", "--min-identity", "0.995"], context=ctx)
    assert tsv.read_text() == ""
    cli.main(base + ["--n-matches", "--min-chain", "150"], context=ctx)
    with_n = lines(model(150, 1))
    assert tsv.read_text().splitlines() == with_n and any(line.split("\t")[3] == "1" and line.endswith("\tN") for line in with_n)
