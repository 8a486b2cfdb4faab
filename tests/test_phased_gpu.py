"""GPU (-m gpu): the consensus over phased segments (prf_phased_consensus, csrc/phased.hip).  Every result -- rows,
letters and counts -- is compared EXACTLY with the model (tests/phased_model.py, pinned to a brute force and to the ungapped model
by tests/test_phased_cpu.py).

Shapes: the genome of tests/test_consensus_gpu.py (two contigs of 30 011 and 20 003 positions of ACGT, N blocks and lower case)
and one of 12 000 positions with R / Y stretches (eight planes); segments of 1 to 3 011 positions at every k around the regime
boundaries (64 | 65, 1 024 | 1 025) at the phases 0, 1 and k - 1; the planted gapped repeats of tests/phased_cases.py (a few
hundred to 1 300 positions) from the chains to their names."""
import itertools
import random

import numpy as np
import pytest

import consensus_model as C
import phased_cases as K
import phased_model as M
from test_consensus_gpu import _first_contig
from test_dotruns_gpu import _random

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 63, 64, 65, 1_023, 1_024, 1_025, 2_500]
STARTS = [0, 1, 63]                                           # start % 64
LONG = 3_011


def _lengths(k):
    return sorted({1, max(1, k - 1), k, k + 1, 64, 65, LONG})


def _phases(k):
    return sorted({0, 1 % k, k - 1})


@pytest.fixture(scope="module")
def ctx():
    import torch  # the same load order as the other GPU tests (torch's HIP runtime first)
    assert torch.cuda.is_available()
    import prf_native
    assert np.dtype(prf_native.SEGMENT_DTYPE).itemsize == 24
    c = prf_native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def two_contigs(ctx):
    seqs = [_first_contig(), _random(20_003, 184)]
    g = ctx.load(seqs, 64)
    yield g, seqs
    g.free()


def _check(got, want, what=None):
    rows, motifs, counts = got[:3]
    assert rows.dtype == np.dtype(M.DTYPE) and M.same(rows, want[0]), what
    assert motifs == want[1], what
    assert counts.dtype == np.uint32 and counts.shape == want[2].shape and np.array_equal(counts, want[2]), what


@pytest.mark.parametrize("begin", [29, 192])
def test_periods_lengths_phases_and_alignments_against_the_model(two_contigs, begin):
    """Every k x every length x every phase x every start % 64, one row of one segment each, in one call per range; begin % 64 is
    29 (every word is funnel-shifted) or 0."""
    g, seqs = two_contigs
    segs, ks = [], []
    for at, (k, start) in enumerate(itertools.product(KS, STARTS)):
        for n, phase in itertools.product(_lengths(k), _phases(k)):
            segs.append((start + 64 * (at % 5), start + 64 * (at % 5) + n, len(ks), phase))
            ks.append(k)
    assert len(ks) > 500 and {a % 64 for a, _, _, _ in segs} == set(STARTS)
    table = M.segments(*segs)
    want = M.consensus(seqs[0], ks, table, begin, 9_000)
    got = g.phased_consensus(0, begin, 9_000, ks, table, counts=True, with_stats=True)
    _check(got, want, begin)
    st = got[3]
    assert st.path == 13 and st.n_hits == len(ks) and st.positions == sum(b - a for a, b, _, _ in segs)
    assert st.n_candidates == len(segs)                                        # no segment is longer than a slice
    assert st.n_launches == 4 and st.scan_ms > 0 and st.scan_ms == pytest.approx(st.phase1_ms + st.phase2_ms)   # three regimes, one finish
    assert sum("N" in m for m in want[1]) > 100 and int((want[0]["agree"] < want[0]["acgt"]).sum()) > 100       # empty columns; real votes


def _rows_of_segments(n, rng):
    """Rows of 1, 2 and 7 segments with gaps and overlaps between them and one without, at k of every regime; the segments
    shuffled, so that they come unsorted and the rows interleave."""
    ks, segs = [], []
    for k in (1, 3, 7, 64, 65, 171, 1_024, 1_025, 2_500):
        for count in (1, 2, 7, 0):
            at = rng.randrange(n - 8_000)
            for j in range(count):
                length = rng.choice((1, 5, 64, 65, 300, 900))
                segs.append((at, at + length, len(ks), rng.choice(_phases(k) + [rng.randrange(k)])))
                at += rng.choice((-length // 2, 0, 1, 70, length + 13))        # overlap, repeat the start, touch, gap
                at = max(at, 0)
            ks.append(k)
    rng.shuffle(segs)
    return ks, segs


def test_rows_of_several_segments_unsorted_and_interleaved(two_contigs):
    g, seqs = two_contigs
    ks, segs = _rows_of_segments(len(seqs[0]), random.Random(191))
    counts = np.bincount([row for _, _, row, _ in segs], minlength=len(ks))
    assert sorted(set(counts.tolist())) == [0, 1, 2, 7] and [row for _, _, row, _ in segs] != sorted(row for _, _, row, _ in segs)
    table = M.segments(*segs)
    want = M.consensus(seqs[0], ks, table)
    got = g.phased_consensus(0, 0, None, ks, table, counts=True)
    _check(got, want)
    bare = np.flatnonzero(counts == 0)
    assert all(got[1][r] == "N" * ks[r] for r in bare) and not got[0]["acgt"][bare].any() and not got[0]["agree"][bare].any()
    # no segments at all: every row is all N, nothing is counted, only the finish kernel runs
    rows, motifs, table0, st = g.phased_consensus(0, 0, None, ks, M.segments(), counts=True, with_stats=True)
    assert motifs == ["N" * k for k in ks] and not table0.any() and not rows["agree"].any() and rows["k"].tolist() == ks
    assert st.n_launches == 1 and st.n_candidates == 0 and st.positions == 0 and st.n_hits == len(ks)
    _check((rows, motifs, table0), M.consensus(seqs[0], ks, M.segments()))
    # no rows: nothing at all
    rows, motifs, table0, st = g.phased_consensus(0, 0, None, [], M.segments(), counts=True, with_stats=True)
    assert len(rows) == 0 and motifs == [] and table0.shape == (0, 4) and st.n_launches == 0


def test_the_first_position_and_the_last_of_the_genome(two_contigs):
    g, seqs = two_contigs
    for contig, seq in enumerate(seqs):
        n = len(seq)
        ks = [1, 7, 64, 65, 171, 1_024, 1_025, 5_000, n + 5]
        segs = [(0, n // 2, row, k - 1) for row, k in enumerate(ks)] + [(n // 2 + 3, n, row, 1 % k) for row, k in enumerate(ks)]
        segs += [(0, 1, 0, 0), (n - 1, n, 0, 0), (n - 70, n, 1, 3), (n - 1_100, n, 6, 1_024), (0, 70, 5, 1_023)]
        table = M.segments(*segs)
        _check(g.phased_consensus(contig, 0, None, ks, table, counts=True), M.consensus(seq, ks, table), contig)


def test_n_blocks_lower_case_and_ties(two_contigs):
    g, seqs = two_contigs
    ks = [5, 3, 100, 1_500, 4, 70, 1, 1, 4, 66]
    segs = [(400, 600, 0, 2), (560, 800, 0, 4), (4_000, 4_300, 1, 1), (4_300, 4_700, 1, 0), (4_000, 4_700, 2, 99), (4_000, 4_700, 3, 7),
            (900, 1_500, 4, 3), (1_000, 1_400, 5, 69), (2_000, 2_032, 6, 0), (2_032, 2_064, 6, 0), (2_100, 2_164, 7, 0),
            (2_000, 2_030, 8, 2), (2_034, 2_064, 8, 0), (2_100, 2_164, 9, 65), (3_990, 4_010, 0, 0)]
    table = M.segments(*segs)
    got = g.phased_consensus(0, 0, None, ks, table, counts=True)
    _check(got, M.consensus(seqs[0], ks, table))
    rows, motifs, counts = got
    assert motifs[1] == "NNN" and motifs[2] == "N" * 100 and rows["acgt"][1:4].tolist() == [0, 0, 0]
    assert motifs[6] == "A" and rows[6].tolist()[1:3] == (32, 64) and motifs[7] == "G"     # 32 A against 32 C, 32 G against 32 T
    assert motifs[8] == "ACAC" and rows[8].tolist()[1:3] == (60, 60)          # [2 000, 2 030) from column 2, [2 034, 2 064) from column 0
    assert counts[rows["offset"][6]].tolist() == [32, 32, 0, 0]


def test_stretches_of_r_and_y_through_the_same_kernels(ctx):
    """A genome of eight planes: R and Y (and every letter outside ACGT) count for nothing, as N does; and the one-shot form."""
    rng = random.Random(192)
    s = bytearray(_random(12_000, 186))
    for at in (300, 5_000, 9_000):
        s[at:at + 90] = bytes(rng.choice(b"RYN") for _ in range(90))
    s[7_000:7_400] = (b"RYRRY" * 80)
    s = bytes(s)
    ks = [1, 5, 64, 65, 400, 1_025]
    segs = [(a, b, row, (a * 7 + row) % k) for row, k in enumerate(ks) for a, b in ((0, 6_000), (5_990, 12_000), (250, 450), (7_000, 7_400), (7_100, 7_101))]
    table = M.segments(*segs)
    g = ctx.load([s], 64)
    try:
        for begin, end in ((0, None), (0, 12_000)):
            _check(g.phased_consensus(0, begin, end, ks, table, counts=True), M.consensus(s, ks, table), (begin, end))
        inner = M.segments((0, 200, 0, 3), (210, 400, 0, 1), (10, 411, 1, 63), (5, 6, 2, 0))            # position 7 000: an R
        got = g.phased_consensus(0, 7_000 - 5, 7_000 + 406, [5, 64, 1], inner, counts=True)
        _check(got, M.consensus(s, [5, 64, 1], inner, 7_000 - 5, 7_000 + 406))
        assert got[1][2] == "N" and got[0]["acgt"][0] == 5                      # five letters in front of the stretch
    finally:
        g.free()
    _check(ctx.phased_consensus(s, ks, table, counts=True), M.consensus(s, ks, table), "one shot")
    _check(ctx.phased_consensus(s.decode(), [5, 64, 1], inner, begin=6_995, end=7_406, counts=True), M.consensus(s, [5, 64, 1], inner, 6_995, 7_406),
           "one shot, a range")
    rows, motifs = ctx.phased_consensus("acgACGtACGACG", [3], M.segments((0, 6, 0, 0), (7, 13, 0, 0)))
    assert motifs == ["ACG"] and rows["agree"][0] == 12


@pytest.mark.parametrize("k", [1, 3, 64, 65, 171, 1_024, 1_025, 2_500])
def test_slices_do_not_change_the_result(two_contigs, k):
    g, seqs = two_contigs
    segs = [(6_000 + 37, 6_000 + 37 + LONG, 0, k - 1), (1, 2 * k, 0, 1 % k), (63, 64 + k, 1, 0), (100, 101, 1, k // 2), (9_000, 9_000 + LONG, 1, 1 % k)]
    table = M.segments(*segs)
    want = M.consensus(seqs[0], [k, k], table, 29, None)
    whole = g.phased_consensus(0, 29, None, [k, k], table, counts=True)
    _check(whole, want)
    for slice_positions in (64, 100, k - 1, 4_096, 1 << 40):
        got = g.phased_consensus(0, 29, None, [k, k], table, counts=True, with_stats=True, slice_positions=slice_positions)
        _check(got, want, slice_positions)
        assert got[0].tobytes() == whole[0].tobytes() and got[2].tobytes() == whole[2].tobytes()
        each = slice_positions or 4_096
        assert got[3].n_candidates == sum(-(-(b - a) // each) for a, b, _, _ in segs)


def test_five_thousand_segments_over_seven_hundred_rows(two_contigs):
    g, seqs = two_contigs
    rng = random.Random(193)
    n = len(seqs[1])
    ks = [rng.choice((1, 2, 3, 4, 6, 17, 64, 65, 171, 1_025)) for _ in range(700)]
    segs = []
    for _ in range(5_000):
        start, row = rng.randrange(n), rng.randrange(690)                      # the last ten rows have no segment
        segs.append((start, min(n, start + rng.choice((1, 2, 10, 64, 65, 300, 2_000))), row, rng.randrange(ks[row])))
    segs[100:200] = segs[:100]                                                 # duplicates count once each
    table = M.segments(*segs)
    want = M.consensus(seqs[1], ks, table)
    got = g.phased_consensus(1, 0, None, ks, table, counts=True)
    _check(got, want)
    again = g.phased_consensus(1, 0, None, ks, table, counts=True)             # equal bytes twice
    assert again[0].tobytes() == got[0].tobytes() and again[1] == got[1] and again[2].tobytes() == got[2].tobytes()
    assert got[0]["k"].tolist() == ks and got[1][-10:] == ["N" * k for k in ks[-10:]]
    rows_only = g.phased_consensus(1, 0, None, ks, table)                      # without the counts
    assert len(rows_only) == 2 and rows_only[0].tobytes() == got[0].tobytes() and rows_only[1] == got[1]


def test_one_segment_of_phase_0_per_row_is_period_consensus(two_contigs):
    g, seqs = two_contigs
    rows = [(start + 64 * (at % 5), start + 64 * (at % 5) + n, k) for at, (k, start) in enumerate(itertools.product(KS, STARTS)) for n in _lengths(k)]
    rows += [(0, 29_900, k) for k in (1, 171, 1_025)]                          # several work items each
    plain = C.repeats(*rows)
    table = M.segments(*[(a, b, at, 0) for at, (a, b, _) in enumerate(rows)])
    old = g.period_consensus(0, 29, None, plain, counts=True)
    new = g.phased_consensus(0, 29, None, [k for _, _, k in rows], table, counts=True)
    assert new[0].tobytes() == old[0].tobytes() and new[1] == old[1] and new[2].tobytes() == old[2].tobytes()


def test_refusals_on_a_resident_genome(ctx, two_contigs):
    import prf_native as pn
    g, _ = two_contigs
    ks, seg = np.array([3], dtype=np.uint32), M.segments((0, 30_012, 0, 0))
    out, letters = np.zeros(1, dtype=pn.CONSENSUS_DTYPE), np.zeros(8, dtype=np.uint8)
    args = (0, 1 << 63, ks.ctypes.data, 1, seg.ctypes.data, 1, out.ctypes.data, letters.ctypes.data, 8, None, None)
    rc = ctx.lib.prf_phased_consensus(ctx._h, g._h, 0, *args)
    assert rc == pn.PRF_EINVAL and "segment 0: end 30012 is behind the range's 30011 positions" in ctx.lib.prf_last_error().decode()
    rc = ctx.lib.prf_phased_consensus(ctx._h, g._h, 2, *args)
    assert rc == pn.PRF_EINVAL and not out["agree"][0]
    rc = ctx.lib.prf_phased_consensus_ex(ctx._h, g._h, 0, 0, 1 << 63, ks.ctypes.data, 0, None, 0, None, None, 0, None, None, 0)
    assert rc == pn.PRF_OK
    with pytest.raises(pn.PrfError, match="unsupported symbol at position 4"):
        ctx.phased_consensus("ACGT-ACGT", [3], M.segments((0, 9, 0, 0)))


@pytest.mark.parametrize("kind", ["ins", "del", "both"])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("period", [7, 17, 40])
def test_a_planted_gapped_repeat_from_the_chains_to_its_name(ctx, period, d, kind):
    """period_chains -> period_links -> join_period_chains -> group_segments -> phased_consensus -> group_consensus_rows on the
    planted inputs of tests/test_phased_cpu.py: one piece, the planted motif rotated to its anchor, and a consensus identity
    above what the ungapped columns give."""
    import prf_native as pn
    motif, seq = K.planted(period, d, kind)
    g = ctx.load([seq.encode()], 64)
    try:
        chains = g.period_chains(0, 0, None, 1, period + 8, K.MIN_SEED[period], K.MAX_GAP, 0)
        links = g.period_links(0, 0, None, 1, period + 8, K.MIN_SEED[period], K.MAX_GAP, K.MAX_SHIFT)
        groups = pn.join_period_chains(chains, links)
        pieces, segments = pn.group_segments(chains, links)
        cons, motifs, counts = g.phased_consensus(0, 0, None, pieces["k"], segments, counts=True)
        at = K.body_group(groups, period, len(seq))
        flat, _ = g.period_consensus(0, 0, None, C.repeats((int(groups["start"][at]), int(groups["end"][at]), period)))
    finally:
        g.free()
    _check((cons, motifs, counts), M.consensus(seq, pieces["k"].tolist(), segments))
    assert (M.group_segments(chains, links, groups["period"].tolist())) == ([tuple(p) for p in pieces.tolist()], [tuple(s) for s in segments.tolist()])
    rows, names = pn.group_consensus_rows(groups, pieces, cons, motifs)
    turn = (int(groups["start"][at]) - K.FLANK) % period
    assert rows["pieces"][at] == 1 and names[at] == motif[turn:] + motif[:turn] and rows["primitive"][at] == period
    assert pn.canonical_motif(names[at]) == pn.canonical_motif(motif)
    span = int(groups["end"][at]) - int(groups["start"][at])
    assert rows["consensus_identity"][at] > flat["agree"][0] / span and rows["consensus_identity"][at] >= 0.97 and rows["covered"][at] > 0.9


def test_scans_and_the_other_products_are_not_disturbed(ctx):
    import torch
    import prf_native
    tile = prf_native.tile_positions()
    seq = bytearray(_random(3 * tile + 500, 13))
    for at in range(1000, len(seq) - 200, 9_973):
        seq[at:at + 60] = b"CAG" * 20
    seq = bytes(seq)
    g = ctx.load([seq, _random(900, 14)], 50)
    cap = 100_000
    buf = torch.empty((cap + 1, 3), dtype=torch.int64, device="cuda")
    try:
        g.select([(0, tile, 3 * tile)])
        ctx.set_row_sink(buf.data_ptr(), cap)
        before, _ = g.scan(1, 50, 3, 9)
        sink_before = buf.cpu().numpy().copy()
        bits_before = g.period_bits(0, 1, 20, 900, 1_300)
        plain = C.repeats((1_000, 1_060, 3), (0, 3_000, 50))
        named_before = g.period_consensus(0, 0, None, plain, counts=True)
        ks = [3, 50, 171, 1_025]
        table = M.segments((1_000, 1_030, 0, 0), (1_030, 1_060, 0, 0), (0, 3_000, 1, 49), (10, 2_000, 2, 5), (0, 3 * tile, 3, 1_024))   # whatever is selected
        got = g.phased_consensus(0, 0, None, ks, table, counts=True)
        _check(got, M.consensus(seq, ks, table))
        assert got[1][0] == "CAG" and got[0]["agree"][0] == 60
        assert ctx.phased_consensus(seq[:2_000], ks[:1], table[:2])[1] == ["CAG"]   # and the one-shot form, a genome of its own
        assert np.array_equal(buf.cpu().numpy(), sink_before)                 # nothing was written to the sink
        assert np.array_equal(g.period_bits(0, 1, 20, 900, 1_300), bits_before)
        named_after = g.period_consensus(0, 0, None, plain, counts=True)
        assert named_after[0].tobytes() == named_before[0].tobytes() and named_after[2].tobytes() == named_before[2].tobytes()
        after, _ = g.scan(1, 50, 3, 9)
        assert len(before) > 10 and np.array_equal(before, after)
        assert before["start"].min() >= tile and before["start"].max() < 3 * tile
        assert np.array_equal(buf.cpu().numpy(), sink_before)
    finally:
        ctx.set_row_sink(None, 0)
        g.select([])
        g.free()


def test_cli_names_the_gapped_repeats_of_an_interval(ctx, tmp_path):
    import plot_periodicity_matrix as cli
    import prf_native as pn
    motif, body = K.planted(17, 2, "both")
    chrom = (_random(3_000, 14).decode() + body + "N" * 200 + K.planted(17, 1, "ins")[1] + _random(2_000, 15).decode()).lower()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\nACGT\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    plain, named = tmp_path / "plain.tsv", tmp_path / "named.tsv"
    base = [str(fa), "-i", f"chrT:100-{len(chrom) - 50}", "--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--max-shift", "4",
            "--min-group", "60", "--chain-window", "1000"]
    cli.main(base + ["--groups-tsv", str(plain)], context=ctx)
    cli.main(base + ["--groups-tsv", str(named), "--group-consensus"], context=ctx)
    old, new = plain.read_text().splitlines(), named.read_text().splitlines()
    assert len(old) == len(new) >= 2
    # the model's answer for the same interval: the chains and links of the device (pinned elsewhere), the segments and the counts here
    g = ctx.load([chrom.encode()], 64)
    try:
        n, windows = len(chrom) - 150, range(0, len(chrom) - 150, 1_000)
        chains = np.concatenate([g.period_chains(0, 100, len(chrom) - 50, 1, 25, 12, 8, 0, False, (at, min(at + 1_000, n))) for at in windows])
        links = np.concatenate([g.period_links(0, 100, len(chrom) - 50, 1, 25, 12, 8, 4, False, (at, min(at + 1_000, n))) for at in windows])
    finally:
        g.free()
    groups = pn.join_period_chains(chains, links)
    pieces, segs = M.group_segments(chains, links, groups["period"].tolist())
    pieces, segs = np.array(pieces, dtype=pn.PIECE_DTYPE), np.array(segs, dtype=pn.SEGMENT_DTYPE)
    cons, motifs, _ = M.consensus(chrom, pieces["k"].tolist(), segs, 100, len(chrom) - 50)
    rows, names = pn.group_consensus_rows(groups, pieces, cons.astype(pn.CONSENSUS_DTYPE), motifs)
    by_place = {(int(r["start"]) + 100, int(r["end"]) + 100, int(r["period"])): (r, name) for r, name in zip(rows, names)}
    assert len(by_place) == len(rows)
    seventeen = 0
    for before, line in zip(old, new):
        assert line.startswith(before + "\t")
        r, name = by_place[tuple(int(x) for x in before.split("\t")[1:4])]
        assert line[len(before) + 1:].split("\t") == [name, f"{r['consensus_identity']:.4f}", str(r["primitive"]), pn.canonical_motif(name),
                                                     str(r["pieces"]), f"{r['covered']:.4f}"]
        if before.split("\t")[3] == "17" and int(before.split("\t")[2]) - int(before.split("\t")[1]) > 400:
            seventeen += 1
            assert r["pieces"] == 1 and r["consensus_identity"] > 0.97
    assert seventeen == 2
    first = [name for (a, b, period), (_, name) in by_place.items() if period == 17 and 3_000 <= a < 3_100 and b - a > 400]
    assert [pn.canonical_motif(name) for name in first] == [pn.canonical_motif(motif)]
    cli.main(base + ["--groups-tsv", str(named), "--group-consensus", "--min-group-consensus-identity", "0.97"], context=ctx)
    assert named.read_text().splitlines() == [line for line in new if float(line.split("\t")[11]) >= 0.97]
