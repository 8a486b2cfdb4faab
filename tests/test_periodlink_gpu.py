"""GPU (-m gpu): the list of junctions between the chains of the period lines of one range (prf_period_links, csrc/periodlink.hip,
DESIGN 17).  Every list is compared EXACTLY: with the model (tests/periodlink_model.py, pinned to a brute force and to
dotlink_model by tests/test_periodlink_cpu.py), with prf_dotpair_links of the same range against itself, or with links known by
construction (tests/periodlink_cases.py).

Shapes: the fixture's 276 sequences (at most 195 positions); the planted cases, 120 to 260 positions each, one contig per case;
a contig of 33 000 positions so that the find kernel's span boundary at 32 768 is crossed, one of 7 219 with a period of 2 048 so
that the k-slice boundary is; ranges of up to 8 192 positions of the three-contig genome of tests/test_dotruns_gpu.py."""
import ctypes
import random

import numpy as np
import pytest

import periodchain_model as M
import periodlink_cases as K
import periodlink_model as L
from conftest import load_jsonl_gz
from test_dotruns_gpu import _random
from test_periodchain_gpu import BAND_RANGES, three_contigs  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

TRIPLES = [(3, 2, 1), (3, 2, 4), (4, 8, 8), (5, 3, 32), (8, 16, 32)]             # (min_seed, max_gap, max_shift), DESIGN 15.4's
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
    for f in L.FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)


# ---- 1. the fixture, one-shot ----

@pytest.fixture(scope="module")
def modelled():
    """[(sequence, {(n_matches, triple): (every link, the chains of the band)})], computed once."""
    seen = {}
    for c in load_jsonl_gz("dotpair.jsonl.gz"):
        for s in (c["a"], c["b"]):
            seen.setdefault(s, None)
    out = []
    for s in seen:
        want = {}
        for nm in (0, 1):
            chains = {}
            for triple in TRIPLES:
                if triple[:2] not in chains:
                    chains[triple[:2]] = L.band_chains(s, nm, *triple[:2])
                want[nm, triple] = L.all_links(chains[triple[:2]], *triple), len(chains[triple[:2]])
        out.append((s, want))
    return out


@pytest.mark.parametrize("n_matches", [0, 1])
@pytest.mark.parametrize("triple", TRIPLES)
def test_every_fixture_sequence_through_the_one_shot_call(ctx, modelled, triple, n_matches):
    bad, total = [], 0
    assert len(modelled) == 276
    for at, (s, wants) in enumerate(modelled):
        want, heads = wants[n_matches, triple]
        got, st = ctx.period_links(s, 1, max(len(s), 1), *triple, n_matches=bool(n_matches), with_stats=True)
        if not L.same(got, want):
            bad.append(at)
        total += len(want)
        assert st.path == 11 and st.positions == len(s) and st.n_hits == len(got) and st.n_candidates == heads
        assert (st.scan_ms > 0 and st.n_launches >= 1 and st.scan_ms == pytest.approx(st.phase1_ms + st.phase2_ms)) or len(s) < 2
    assert not bad, f"{len(bad)} sequences differ: {bad[:5]}"
    floors = {((3, 2, 1), 0): 5804, ((3, 2, 1), 1): 7613, ((3, 2, 4), 0): 10318, ((3, 2, 4), 1): 12840, ((4, 8, 8), 0): 3940,
              ((4, 8, 8), 1): 5108, ((5, 3, 32), 0): 2095, ((5, 3, 32), 1): 2812, ((8, 16, 32), 0): 203, ((8, 16, 32), 1): 299}
    assert total >= floors[triple, n_matches]                   # the brute force's counts (tests/test_periodlink_cpu.py)


def test_letters_outside_acgtn_use_the_eight_plane_kernels(ctx):
    rng = random.Random(31)
    unit = bytes(rng.choice(b"ACGTRYKMSWN") for _ in range(23))
    first = _random(40, 32) + (unit * 5)[:60] + b"RY" + (unit * 5)[60:] + _random(40, 33)       # two letters inserted into a repeat of IUPAC letters
    second = bytes(rng.choice(b"ACRYN") for _ in range(300))                                   # dense: five letters, N among them
    total = 0
    for s, triple in ((first, (10, 3, 4)), (first, (4, 8, 8)), (second, (3, 2, 4)), (second, (3, 2, 32))):
        for nm in (False, True):
            got = ctx.period_links(s, 1, len(s), *triple, n_matches=nm)
            _same(got, L.links(s, 1, len(s), *triple, n_matches=nm), (triple, nm))
            total += len(got)
    assert total >= 100
    got = ctx.period_links(first, 1, 40, 10, 3, 4, n_matches=True)
    assert [(int(r["k"]), int(r["shift"])) for r in got if r["k"] in (23, 25)] == [(25, 2), (23, -2)]


# ---- 2. the planted junctions ----

WORD = K.tandem(20, 70, [("ins", 35, 1)], 41, flank=49)                        # X ends at cell 63, the detour starts at cell 64
SPAN_AT = 32_728                                                              # ... at cell 32 767 | 32 768 of a contig of N
SPAN = b"N" * SPAN_AT + K.tandem(20, 70, [("ins", 35, 1)], 42) + b"N" * (33_000 - SPAN_AT - 121)
SLICE = K.tandem(2_048, 7_168, [("ins", 3_584, 1)], 43)                       # k_X = 2 048, k_Y = 2 049: two k slices
LONG = K.tandem(20, 2_600, [("ins", 2_400, 1)], 44)                           # a predecessor of 2 380 cells > F
FIRST = K.tandem(20, 70, [("ins", 35, 1)], 45, flank=0)                       # a chain at position 0 of contig 0, one up to the last position


@pytest.fixture(scope="module")
def planted(ctx):
    """One genome of ACGT and N (the 3-plane kernels): FIRST, the cases, the placed ones, FIRST again as the last contig."""
    names = list(K.CASES)
    seqs = [FIRST] + [K.CASES[name][0] for name in names] + [WORD, SPAN, SLICE, LONG, FIRST]
    assert all(set(s) <= set(b"ACGTN") for s in seqs)
    g = ctx.load(seqs, 64)
    yield g, seqs, {name: 1 + at for at, name in enumerate(names)}
    g.free()


@pytest.mark.parametrize("name", list(K.CASES))
def test_planted_cases(planted, name):
    g, seqs, where = planted
    seq, params, _claims = K.CASES[name]
    for nm in (0, 1):
        want = K.expected(name, nm)
        K.check_claim(name, want, nm)
        got = g.period_links(where[name], 0, None, 1, len(seq), *params, n_matches=bool(nm))
        _same(got, want, (name, nm))
        _same(g.period_links(where[name], 7, None, 1, len(seq), *params, n_matches=bool(nm)),
              L.links(seq, 1, len(seq), *params, n_matches=nm, begin=7), (name, nm, "begin 7"))


def test_dense_bands_up_to_the_last_line(ctx):
    for seq, params in K.DENSE:
        for nm in (False, True):
            _same(ctx.period_links(seq, 1, len(seq), *params, n_matches=nm), L.links(seq, 1, len(seq), *params, n_matches=nm), (seq, nm))
            _same(ctx.period_links(seq, len(seq) - 9, 1 << 31, *params, n_matches=nm),
                  L.links(seq, len(seq) - 9, None, *params, n_matches=nm), (seq, nm, "the last lines"))


def test_junctions_across_a_word_a_span_and_a_k_slice(planted):
    g, seqs, where = planted
    base = 1 + len(where)
    params = (K.S, K.G, K.D)
    # a word of the line: cells 63 | 64
    want = L.links(WORD, 1, len(WORD), *params)
    assert (int(want["from_end"][0]), int(want["start"][0]), int(want["k"][0])) == (63, 64, 21)
    _same(g.period_links(base, 0, None, 1, len(WORD), *params), want, "word")
    # the span boundary of the find kernel: Y starts in the second span, X ended in the first
    want = L.links(SPAN, 1, 4_000, *params, sparse=True)
    assert (int(want["from_end"][0]), int(want["start"][0])) == (32_767, 32_768) and len(want) == 2
    got, st = g.period_links(base + 1, 0, None, 1, 4_000, *params, with_stats=True)
    _same(got, want, "span")
    assert st.n_candidates == len(M.select(L.band_chains(SPAN, 0, K.S, K.G, sparse=True), len(SPAN), None, 1, 4_000))
    _same(g.period_links(base + 1, 0, None, 1, 4_000, *params, positions=(32_768, 32_769)), want[:1], "the first cell of the second span alone")
    _same(g.period_links(base + 1, 0, None, 1, 4_000, *params, positions=(0, 32_768)), want[:0], "the first span alone")
    # begin % 64 != 0, and a window that starts inside
    _same(g.period_links(base + 1, 32_700 + 37, 32_900, 1, 150, *params), L.links(SPAN, 1, 150, *params, begin=32_737, end=32_900), "begin % 64 = 33")
    # two k slices: k_X = 2 048 in the first, k_Y = 2 049 in the second
    want = L.links(SLICE, 1, len(SLICE), *params, sparse=True)
    assert [(int(r["k"]), int(r["shift"])) for r in want if r["k"] in (2_048, 2_049)] == [(2_049, 1), (2_048, -1)]
    _same(g.period_links(base + 2, 0, None, 1, len(SLICE), *params), want, "k slices")
    _same(g.period_links(base + 2, 0, None, 2_049, 2_049, *params), want[want["k"] == 2_049], "the second slice alone")


def test_first_position_last_position_and_a_long_predecessor(planted):
    g, seqs, where = planted
    params = (K.S, K.G, K.D)
    want = L.links(FIRST, 1, len(FIRST), *params)
    assert [(int(r["k"]), int(r["shift"])) for r in want] == [(21, 1), (20, -1)]
    chains = L.band_chains(FIRST, 0, K.S, K.G)
    assert int(chains["start"].min()) == 0 and int((chains["start"] + chains["len"] + chains["k"]).max()) == len(FIRST)
    _same(g.period_links(0, 0, None, 1, len(FIRST), *params), want, "contig 0")
    _same(g.period_links(len(seqs) - 1, 0, None, 1, len(FIRST), *params), want, "the last contig")
    # X has more than F cells and starts in front of the window
    want = L.links(LONG, 1, 100, *params, sparse=True)
    long_one = want[want["k"] == 21]
    assert len(long_one) == 1 and int(long_one["from_end"][0]) >= F + 300
    at = int(long_one["start"][0])
    _same(g.period_links(len(seqs) - 2, 0, None, 1, 100, *params), want, "long")
    _same(g.period_links(len(seqs) - 2, 0, None, 1, 100, *params, positions=(at - 50, None)), want[want["start"] >= at - 50], "window behind X's start")


# ---- 3. the same lists as prf_dotpair_links of the range against itself ----

def _against_the_rectangle(g, contig, begin, end, n, triple, what):
    """period_links of the lines above 2 max_shift against dotpair_links of the range with itself, main direction, restricted to
    delta_Y >= 1 and the same lines (tests/test_periodlink_cpu.py has the reason); the number of links."""
    min_seed, max_gap, max_shift = triple
    square = g.dotpair_links((contig, begin, end), (contig, begin, end), "+", "main", min_seed, max_gap, max_shift)
    delta = square["col"].astype(np.int64) - square["row"].astype(np.int64)
    square = square[(delta >= 1) & (delta > 2 * max_shift)]
    want = np.zeros(len(square), dtype=L.DTYPE)
    want["start"], want["from_end"], want["k"] = square["row"], square["from_row"], square["col"] - square["row"]
    for f in ("shift", "gap", "overlap"):
        want[f] = square[f]
    want = np.sort(want, order=["start", "k"])
    got = g.period_links(contig, begin, end, 2 * max_shift + 1, max(n, 2 * max_shift + 1), min_seed, max_gap, max_shift, n_matches=True)
    _same(got, want, what)
    return got


@pytest.mark.parametrize("which", range(len(BAND_RANGES)))
def test_links_above_twice_max_shift_are_those_of_the_rectangle(three_contigs, which):  # noqa: F811
    """The ranges of tests/test_periodchain_gpu.py.  That genome holds copies, IUPAC stretches and N blocks but no repeat with an
    indel: at these two triples both lists are EMPTY on every one of its ranges (the model says so for every window of 8 192
    positions of its contigs), so this pins only that neither product invents a link there.  The ranges with links follow."""
    g, seqs = three_contigs
    contig, begin, end = BAND_RANGES[which]
    n = len(seqs[contig][begin:end])
    for triple in ((11, 5, 4), (16, 64, 32)):
        _against_the_rectangle(g, contig, begin, end, n, triple, (which, triple))


RECT = _random(1_500, 51) + K.tandem(80, 640, [("ins", 170, 1), ("del", 330, 2), ("ins", 490, 3)], 52, flank=100) + K.vntr()[0] + _random(500, 53)


def test_links_of_repeats_with_indels_are_those_of_the_rectangle(ctx):
    """The same comparison where there are links: a repeat of period 80 and one of period 24, three indels each, in one contig."""
    g = ctx.load([b"N" * 70, RECT], 64)
    try:
        for begin, end in ((0, None), (37, 3_300)):
            n = len(RECT[begin:end])
            for triple, least in (((11, 5, 4), 12), ((16, 64, 32), 6)):
                got = _against_the_rectangle(g, 1, begin, end, n, triple, (begin, triple))
                _same(got, L.links(RECT, 2 * triple[2] + 1, n, *triple, n_matches=True, begin=begin, end=end, sparse=True), (begin, triple, "model"))
                assert len(got) >= least, (begin, triple, len(got))
    finally:
        g.free()


# ---- 4. partitions, launches, capacity, determinism ----

def test_windows_and_periods_add_up_and_launches_do_not_matter(three_contigs):  # noqa: F811
    g, seqs = three_contigs
    contig, begin, end = 2, 37, 4_133
    triple = (4, 8, 8)
    whole, st = g.period_links(contig, begin, end, 1, 130, *triple, with_stats=True)
    _same(whole, L.links(seqs[contig], 1, 130, *triple, begin=begin, end=end), "whole")
    assert len(whole) > 400 and int((whole["shift"] < 0).sum()) > 100 and int((whole["overlap"] > 0).sum()) > 100
    k_x = whole["k"].astype(np.int64) - whole["shift"]
    for cuts, k_cuts in (((0, 2_000, None), (1, 73, 131)),                     # 2 x 2: between lines 72 and 73, X on either side
                         ((0, 64, 2_001, None), (1, 131)),
                         ((0, None), (1, 2, 64, 65, 70, 71, 129, 131))):         # 1 x 7: k ranges of one line, X outside them
        parts = [g.period_links(contig, begin, end, ka, kb - 1, *triple, positions=(p0, p1))
                 for p0, p1 in zip(cuts, cuts[1:]) for ka, kb in zip(k_cuts, k_cuts[1:])]
        assert all(len(p) for p in parts)
        _same(np.sort(np.concatenate(parts), order=["start", "k"]), whole, cuts)                             # each once, unclipped
    one_line = g.period_links(contig, begin, end, 70, 70, *triple)
    assert len(one_line) and (one_line["shift"] != 0).all()                    # every X lies on a line outside [70, 70]
    assert int((k_x > 130).sum()) >= 1                                         # and X above kmax
    # 39 963 positions: three spans of 256 words (8 planes), a launch each when a launch may hold one span x 130 lines
    big, st_big = g.period_links(contig, begin, 40_000, 1, 130, *triple, with_stats=True)
    assert len(big) > len(whole)
    for cells in (1, 64 * 256 * 130, 64 * 256 * 130 + 1):
        cut, st_cut = g.period_links(contig, begin, 40_000, 1, 130, *triple, with_stats=True, launch_cells=cells)
        assert np.array_equal(cut, big) and st_cut.n_launches == st_big.n_launches + 2 and st_cut.n_candidates == st_big.n_candidates
    assert whole.tobytes() == g.period_links(contig, begin, end, 1, 130, *triple).tobytes()                  # two calls, equal bytes
    assert st.n_candidates == len(g.period_chains(contig, begin, end, 1, 130, *triple[:2])) and st.n_hits == len(whole)


def test_capacity_and_counting(ctx, three_contigs):  # noqa: F811
    import prf_native as pn
    g, _ = three_contigs
    want = g.period_links(2, 0, 3_000, 1, 130, 4, 8, 8)
    n = len(want)
    assert n > 5
    for capacity, written in ((n - 1, False), (0, False), (n, True), (n + 3, True)):
        buf = np.full(max(1, capacity + 1), 0xAB, dtype=np.uint8).repeat(32)
        found, stats = ctypes.c_uint64(0), pn.ScanStats()
        rc = ctx.lib.prf_period_links(ctx._h, g._h, 2, 0, 3_000, 0, 3_000, 1, 130, 0, 4, 8, 8, buf.ctypes.data if capacity else None, capacity,
                                      ctypes.byref(found), ctypes.byref(stats))
        assert rc == pn.PRF_OK and found.value == n == stats.n_hits
        if written:
            assert buf[:32 * n].tobytes() == want.tobytes() and (buf[32 * n:] == 0xAB).all()
        else:
            assert (buf == 0xAB).all()


def test_more_heads_than_the_first_pass_has_room_for(ctx):
    """The heads are written into 2^20 rows of room at first and once more into the exact number (grow_once, csrc/list_host.h).
    At min_seed = 1 and max_gap = 0 every run start of the window is a head, 3/16 per cell of random ACGT: 6 200 positions x
    1 000 lines hold 1.16 million, a tenth above 2^20.  So many chains do not fit the model's pairwise matrices: its join form,
    which tests/test_periodlink_cpu.py pins to them."""
    seq = _random(7_000, 63)
    g = ctx.load([seq], 64)
    try:
        got, st = g.period_links(0, 0, None, 1, 1_000, 1, 0, 1, positions=(0, 6_200), with_stats=True)
    finally:
        g.free()
    assert st.n_candidates > 1 << 20
    want = L.links(seq, 1, 1_000, 1, 0, 1, positions=(0, 6_200), pairwise=False)
    assert len(want) > 100_000 and st.n_hits == len(want)
    _same(got, want)


# ---- 5. the neighbours are not disturbed ----

def test_scans_and_the_other_products_are_not_disturbed(ctx):
    import torch
    import prf_native
    tile = prf_native.tile_positions()
    seq = bytearray(_random(3 * tile + 500, 13))
    for at in range(1000, len(seq) - 200, 9_973):
        seq[at:at + 60] = b"CAG" * 20
    seq[2_000:2_000 + len(K.vntr()[0])] = K.vntr()[0]
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
        chains_before = g.period_chains(0, 0, 3_000, 1, 50, 10, 3)
        links_before = g.dotpair_links((0, 900, 1_300), (1, 0, None), "-", "both", 3, 2, 2)
        got = g.period_links(0, 0, 3_000, 1, 50, 10, 3, 4)                        # whatever is selected
        _same(got, L.links(seq, 1, 50, 10, 3, 4, end=3_000, sparse=True))
        assert len(got) >= 6
        assert len(ctx.period_links(seq[2_000:2_400], 1, 50, 10, 3, 4)) >= 6     # and the one-shot form, a genome of its own
        assert np.array_equal(buf.cpu().numpy(), sink_before)                 # nothing was written to the sink
        assert np.array_equal(g.period_bits(0, 1, 20, 900, 1_300), bits_before)
        assert np.array_equal(g.period_chains(0, 0, 3_000, 1, 50, 10, 3), chains_before)
        assert np.array_equal(g.dotpair_links((0, 900, 1_300), (1, 0, None), "-", "both", 3, 2, 2), links_before)
        after, _ = g.scan(1, 50, 3, 9)
        assert len(before) > 10 and np.array_equal(before, after)
        assert before["start"].min() >= tile and before["start"].max() < 3 * tile
        assert np.array_equal(buf.cpu().numpy(), sink_before)
    finally:
        ctx.set_row_sink(None, 0)
        g.select([])
        g.free()


# ---- 6. end to end ----

def test_join_of_the_devices_own_lists(ctx):
    import prf_native as pn
    seq, start, end, indel = K.vntr()
    chains = ctx.period_chains(seq, 1, len(seq), K.S, K.G)
    links = ctx.period_links(seq, 1, len(seq), K.S, K.G, K.D)
    groups = pn.join_period_chains(chains, links)
    assert int(groups["chains"].sum()) == len(chains)
    rows = pn.tandem_groups(groups)
    assert len(rows) == 1 and abs(int(rows["start"][0]) - start) <= 1 and abs(int(rows["end"][0]) - end) <= 1
    assert (int(rows["period"][0]), int(rows["indel"][0]), int(rows["chains"][0])) == (24, indel, 7)
    # a range of k without the detours' lines: the links into line 24 come from outside, the groups are open
    inside = pn.join_period_chains(ctx.period_chains(seq, 24, 24, K.S, K.G), ctx.period_links(seq, 24, 24, K.S, K.G, K.D))
    assert len(inside) == 4 and inside["open"].tolist() == [False, True, True, True]


def test_cli_writes_the_groups_of_an_interval(ctx, tmp_path):
    import plot_periodicity_matrix as cli
    import prf_native as pn
    seq, start, end, indel = K.vntr()
    chrom = (_random(3_000, 14) + seq + b"N" * 200 + _random(2_000, 15)).decode().lower()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\nACGT\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    tsv = tmp_path / "groups.tsv"
    base = [str(fa), "-i", "chrT:100-5000", "--max-motif-size", "80", "--groups-tsv", str(tsv), "--min-seed", str(K.S), "--max-gap", str(K.G),
            "--max-shift", str(K.D)]

    def model(drop=True, floor=0):
        found = M.select(L.band_chains(chrom, 0, K.S, K.G, 100, 5_000, sparse=True), 4_900, None, 1, 80)
        chains = np.zeros(len(found), dtype=pn.PCHAIN_DTYPE)
        for f in M.FIELDS:
            chains[f] = found[f]
        found = L.links(chrom, 1, 80, K.S, K.G, K.D, begin=100, end=5_000, sparse=True)
        links = np.zeros(len(found), dtype=pn.PLINK_DTYPE)
        for f in L.FIELDS:
            links[f] = found[f]
        rows = pn.tandem_groups(pn.join_period_chains(chains, links), drop_covered=drop)
        return [line.rstrip("\n") for line in cli.group_lines("chrT", 100, chrom, rows[rows["end"] - rows["start"] >= floor])]

    cli.main(base + ["--min-group", "100", "--chain-window", "1000"], context=ctx)          # 4 900 positions in 5 windows, no image
    want = model(floor=100)
    assert tsv.read_text().splitlines() == want and len(want) == 1
    line = want[0].split("\t")
    assert line[3] == "24" and line[6] == str(indel) and abs(int(line[1]) - 3_000 - start) <= 1 and abs(int(line[2]) - 3_000 - end) <= 1
    assert not list(tmp_path.glob("*.png"))
    cli.main(base + ["--min-group", "100", "--keep-covered"], context=ctx)
    kept = model(drop=False, floor=100)
    assert tsv.read_text().splitlines() == kept and len(kept) > 1
    cli.main(base, context=ctx)
    assert tsv.read_text().splitlines() == model()
