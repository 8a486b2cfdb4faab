"""GPU (-m gpu): the consensus motifs of tandem repeats (prf_period_consensus, csrc/consensus.hip).  Every result --
rows, letters and counts -- is compared EXACTLY with the model (tests/consensus_model.py, pinned to a brute force and to the
reference's rows by tests/test_consensus_cpu.py).

Shapes: a genome of two contigs of 30 011 and 20 003 positions of ACGT, N blocks and lower case (three planes) and one of 12 000
positions with R / Y stretches (eight planes); rows of 1 to 3 000 positions at every k around the regime boundaries (64 | 65,
1 024 | 1 025); the reference's fixture sequences (at most a few hundred positions) through the one-shot call."""
import itertools
import random

import numpy as np
import pytest

import consensus_model as M
from test_consensus_cpu import reference_rows
from test_dotruns_gpu import _random

pytestmark = pytest.mark.gpu

# the issue's periods, the last k of each regime (64, 1 024) and one more (65, 1 025), and one deep in the last regime
KS = [1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1_023, 1_024, 1_025, 2_500]
STARTS = [0, 1, 37, 63]                                       # start % 64; the range begins 29 bits into a word
LONG = 3_011


def _lengths(k):
    return sorted({1, max(1, k - 1), k, k + 1, 2 * k - 1, 64, 65, LONG})


@pytest.fixture(scope="module")
def ctx():
    import torch  # the same load order as the other GPU tests (torch's HIP runtime first)
    assert torch.cuda.is_available()
    import prf_native
    assert (prf_native.CONSENSUS_SLICE, np.dtype(prf_native.CONSENSUS_DTYPE).itemsize) == (4096, 32)
    c = prf_native.Context(0)
    yield c
    c.close()


def _first_contig():
    s = bytearray(_random(30_011, 181))
    s[500:650] = b"N" * 150                                                    # an N block inside long rows
    s[1_000:1_400] = bytes(s[1_000:1_400]).lower()                             # lower case
    s[2_000:2_064] = b"AC" * 32                                                # ties: A against C, G against T
    s[2_100:2_164] = b"GT" * 32
    s[4_000:4_700] = b"N" * 700                                                # rows of nothing but N
    unit = _random(171, 182)
    for at in range(6_000, 6_000 + 171 * 30):                                  # a diverged array of period 171
        s[at] = unit[(at - 6_000) % 171]
    rng = random.Random(183)
    for at in rng.sample(range(6_000, 6_000 + 171 * 30), 400):
        s[at] = rng.choice(b"ACGTN")
    return bytes(s)


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
def test_periods_lengths_and_alignments_against_the_model(two_contigs, begin):
    """Every k x every length x every start % 64, in one call per range; begin % 64 is 29 (every word is funnel-shifted) or 0."""
    g, seqs = two_contigs
    rows = [(start + 64 * (at % 5), start + 64 * (at % 5) + n, k)
            for at, (k, start) in enumerate(itertools.product(KS, STARTS)) for n in _lengths(k)]
    assert len(rows) > 400 and {a % 64 for a, _, _ in rows} == set(STARTS)
    table = M.repeats(*rows)
    want = M.consensus(seqs[0], table, begin, 9_000)
    got = g.period_consensus(0, begin, 9_000, table, counts=True, with_stats=True)
    _check(got, want, begin)
    st = got[3]
    assert st.path == 12 and st.n_hits == len(rows) and st.positions == sum(b - a for a, b, _ in rows)
    assert st.n_candidates == sum(-(-(b - a) // 4096) for a, b, _ in rows) == len(rows) + len(STARTS)   # 2 x 2 500 - 1 positions: two items
    assert st.n_launches == 4 and st.scan_ms > 0 and st.scan_ms == pytest.approx(st.phase1_ms + st.phase2_ms)   # three regimes, one finish
    assert sum("N" in m for m in want[1]) > 100 and int((want[0]["agree"] < want[0]["acgt"]).sum()) > 150       # empty columns; real votes


def test_the_first_position_and_the_last_of_the_genome(two_contigs):
    g, seqs = two_contigs
    for contig, seq in enumerate(seqs):
        n = len(seq)
        rows = [(0, n, k) for k in (1, 7, 64, 65, 171, 1_024, 1_025, 5_000)] + [(0, 1, 1), (n - 1, n, 1), (n - 70, n, 3), (n - 1_100, n, 1_025), (0, n, n + 5)]
        table = M.repeats(*rows)
        _check(g.period_consensus(contig, 0, None, table, counts=True), M.consensus(seq, table), contig)
    # the array of period 171 of the first contig: its consensus is the unit, though 400 of its 5 130 letters were changed
    rows, motifs = g.period_consensus(0, 0, None, M.repeats((6_000, 6_000 + 171 * 30, 171)))
    assert motifs == [_random(171, 182).decode()] and 171 * 30 - 400 <= rows["agree"][0] < 171 * 30


def test_n_blocks_all_n_rows_lower_case_and_ties(two_contigs):
    g, seqs = two_contigs
    table = M.repeats((400, 800, 5), (4_000, 4_700, 3), (4_100, 4_101, 1), (4_000, 4_700, 100), (4_000, 4_700, 1_500), (900, 1_500, 4), (1_000, 1_400, 70),
                      (2_000, 2_064, 1), (2_001, 2_064, 1), (2_100, 2_164, 1), (2_000, 2_064, 4), (2_100, 2_164, 66), (3_990, 4_010, 7))
    got = g.period_consensus(0, 0, None, table, counts=True)
    _check(got, M.consensus(seqs[0], table))
    rows, motifs, counts = got
    assert motifs[1] == "NNN" and motifs[2] == "N" and motifs[3] == "N" * 100 and rows["acgt"][1:5].tolist() == [0, 0, 0, 0]
    assert motifs[7] == "A" and rows[7].tolist()[1:3] == (32, 64)              # 32 A against 32 C: the first in A, C, G, T
    assert motifs[8] == "C" and motifs[9] == "G" and motifs[10] == "ACAC"      # 31 A against 32 C; 32 G against 32 T
    assert counts[rows["offset"][7]].tolist() == [32, 32, 0, 0] and counts[rows["offset"][9]].tolist() == [0, 0, 32, 32]


def test_stretches_of_r_and_y_through_the_same_kernels(ctx):
    """A genome of eight planes: R and Y (and every letter outside ACGT) count for nothing, as N does."""
    rng = random.Random(185)
    s = bytearray(_random(12_000, 186))
    for at in (300, 5_000, 9_000):
        s[at:at + 90] = bytes(rng.choice(b"RYN") for _ in range(90))
    s[7_000:7_400] = (b"RYRRY" * 80)
    s = bytes(s)
    rows = [(a, b, k) for k in (1, 5, 64, 65, 400, 1_025) for a, b in ((0, 12_000), (250, 450), (7_000, 7_400), (6_990, 7_411), (7_100, 7_101))]
    table = M.repeats(*rows)
    g = ctx.load([s], 64)
    try:
        for begin, end in ((0, None), (0, 12_000)):
            _check(g.period_consensus(0, begin, end, table, counts=True), M.consensus(s, table), (begin, end))
        inner = M.repeats((0, 400, 5), (10, 411, 64), (5, 6, 1))               # position 7 000: an R
        got = g.period_consensus(0, 7_000 - 5, 7_000 + 406, inner, counts=True)
        _check(got, M.consensus(s, inner, 7_000 - 5, 7_000 + 406))
        assert got[1][2] == "N" and got[0]["acgt"][0] == 5
    finally:
        g.free()
    _check(ctx.period_consensus(s, table, counts=True), M.consensus(s, table), "one shot")
    _check(ctx.period_consensus(s.decode(), inner, begin=6_995, end=7_406, counts=True), M.consensus(s, inner, 6_995, 7_406), "one shot, a range")


@pytest.mark.parametrize("k", [1, 3, 64, 65, 171, 1_024, 1_025, 2_500])
def test_slices_do_not_change_the_result(two_contigs, k):
    g, seqs = two_contigs
    table = M.repeats((6_000 + 37, 6_000 + 37 + LONG, k), (1, 2 * k, k), (63, 64 + k, k), (100, 101, k))
    want = M.consensus(seqs[0], table, 29, None)
    whole = g.period_consensus(0, 29, None, table, counts=True)
    _check(whole, want)
    for slice_positions in (64, 100, k - 1, 4_096, 1 << 40):
        got = g.period_consensus(0, 29, None, table, counts=True, with_stats=True, slice_positions=slice_positions)
        _check(got, want, slice_positions)
        assert got[0].tobytes() == whole[0].tobytes() and got[2].tobytes() == whole[2].tobytes()
        each = slice_positions or 4_096
        assert got[3].n_candidates == sum(-(-(b - a) // each) for a, b in zip(table["start"].tolist(), table["end"].tolist()))


def test_five_thousand_overlapping_rows_keep_their_order(two_contigs):
    g, seqs = two_contigs
    rng = random.Random(187)
    n = len(seqs[1])
    rows = []
    for _ in range(2_400):
        start = rng.randrange(n)
        rows.append((start, min(n, start + rng.choice((1, 2, 10, 64, 65, 300, 2_000))), rng.choice((1, 2, 3, 4, 6, 17, 64, 65, 171, 1_025))))
    rows += rows[:100]                                                         # duplicates
    rows += [rng.choice(rows[:50]) for _ in range(2_500)]                      # ... many of a few
    assert len(rows) == 5_000 and len(set(rows)) < 2_500
    table = M.repeats(*rows)
    want = M.consensus(seqs[1], table)
    got = g.period_consensus(1, 0, None, table, counts=True)
    _check(got, want)
    again = g.period_consensus(1, 0, None, table, counts=True)                 # equal bytes twice
    assert again[0].tobytes() == got[0].tobytes() and again[1] == got[1] and again[2].tobytes() == got[2].tobytes()
    assert got[0]["k"].tolist() == [k for _, _, k in rows]                     # nothing is sorted
    rows_only = g.period_consensus(1, 0, None, table)                          # without the counts
    assert len(rows_only) == 2 and rows_only[0].tobytes() == got[0].tobytes() and rows_only[1] == got[1]


def test_no_rows_and_refusals_on_a_resident_genome(ctx, two_contigs):
    import prf_native as pn
    g, _ = two_contigs
    rows, motifs, counts, st = g.period_consensus(0, 0, None, M.repeats(), counts=True, with_stats=True)
    assert len(rows) == 0 and motifs == [] and counts.shape == (0, 4) and st.n_launches == 0
    table = M.repeats((0, 30_012, 3))
    out, letters = np.zeros(1, dtype=pn.CONSENSUS_DTYPE), np.zeros(8, dtype=np.uint8)
    rc = ctx.lib.prf_period_consensus(ctx._h, g._h, 0, 0, 1 << 63, table.ctypes.data, 1, out.ctypes.data, letters.ctypes.data, 8, None, None)
    assert rc == pn.PRF_EINVAL and "row 0: end 30012 is behind the range's 30011 positions" in ctx.lib.prf_last_error().decode()
    rc = ctx.lib.prf_period_consensus(ctx._h, g._h, 2, 0, 1 << 63, table.ctypes.data, 1, out.ctypes.data, letters.ctypes.data, 8, None, None)
    assert rc == pn.PRF_EINVAL and not out["agree"][0]
    with pytest.raises(pn.PrfError, match="unsupported symbol at position 4"):
        ctx.period_consensus("ACGT-ACGT", M.repeats((0, 9, 3)))


def test_every_reference_row_through_the_one_shot_call(ctx):
    """The fact of tests/test_consensus_cpu.py on the device: every reference row whose motif is all ACGT is its own consensus."""
    cases, _ = reference_rows()
    rows = 0
    for seq, plain in cases:
        table = M.repeats(*[(a, b, len(m)) for a, b, m in plain])
        got, motifs = ctx.period_consensus(seq, table)
        assert motifs == [m.upper() for _, _, m in plain], seq
        assert got["agree"].tolist() == got["acgt"].tolist() == [b - a for a, b, _ in plain]
        rows += len(plain)
    assert rows >= 8_718


def test_a_planted_repeat_from_the_chains_to_its_name(ctx):
    """period_chains -> tandem_rows -> period_consensus -> consensus_rows: 40 copies of a motif of 17 with a substitution every 45
    positions (45 = 11 mod 17: they spread over the columns, at most two of 40 in any column), so every column's majority is the
    planted letter and the consensus is the planted motif, rotated to where the row starts."""
    import prf_native as pn
    motif = b"ACGGTCATTGCAGACCT"
    assert len(motif) == 17 and pn.primitive_period(motif.decode()) == 17
    at, body = 5_003, bytearray(motif * 40)
    changed = list(range(20, len(body), 45))
    for p in changed:
        body[p] = ord("A") if body[p] != ord("A") else ord("C")
    assert max(np.bincount([p % 17 for p in changed])) <= 2
    seq = _random(at, 188) + bytes(body) + _random(4_000, 189)
    g = ctx.load([seq], 64)
    try:
        chains = g.period_chains(0, 100, None, 1, 40, 12, 8)
        tandem = pn.tandem_rows(chains)
        cons, motifs = g.period_consensus(0, 100, None, tandem)
    finally:
        g.free()
    named = pn.consensus_rows(tandem, cons, motifs)
    mine = [i for i in range(len(named)) if named["k"][i] == 17 and named["end"][i] - named["start"][i] > 600]
    assert len(mine) == 1
    row, text = named[mine[0]], motifs[mine[0]]
    shift = (int(row["start"]) + 100 - at) % 17
    assert text == (motif[shift:] + motif[:shift]).decode() and row["primitive"] == 17
    assert pn.canonical_motif(text) == pn.canonical_motif(motif.decode())
    span = int(row["end"] - row["start"])
    assert 1 - (len(changed) + 4) / span <= row["consensus_identity"] <= 1 - (len(changed) - 2) / span    # the flanks may add a few positions
    assert row["consensus_identity"] > row["identity"]                        # a substitution costs one position here, two cells there
    assert M.same(cons, M.consensus(seq, tandem, 100)[0]) and motifs == M.consensus(seq, tandem, 100)[1]


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
        chains_before = g.period_chains(0, 0, 3_000, 1, 50, 20, 4)
        table = M.repeats((1_000, 1_060, 3), (0, 3_000, 50), (10, 2_000, 171), (0, 3 * tile, 1_025))   # whatever is selected
        got = g.period_consensus(0, 0, None, table, counts=True)
        _check(got, M.consensus(seq, table))
        assert got[1][0] == "CAG" and got[0]["agree"][0] == 60
        assert ctx.period_consensus(seq[:2_000], table[:1])[1] == ["CAG"]        # and the one-shot form, a genome of its own
        assert np.array_equal(buf.cpu().numpy(), sink_before)                 # nothing was written to the sink
        assert np.array_equal(g.period_bits(0, 1, 20, 900, 1_300), bits_before)
        assert np.array_equal(g.period_chains(0, 0, 3_000, 1, 50, 20, 4), chains_before) and len(chains_before) >= 1
        after, _ = g.scan(1, 50, 3, 9)
        assert len(before) > 10 and np.array_equal(before, after)
        assert before["start"].min() >= tile and before["start"].max() < 3 * tile
        assert np.array_equal(buf.cpu().numpy(), sink_before)
    finally:
        ctx.set_row_sink(None, 0)
        g.select([])
        g.free()


def test_cli_names_the_repeats_of_an_interval(ctx, tmp_path):
    import plot_periodicity_matrix as cli
    import prf_native as pn
    unit = b"ACGGTCA"
    body = bytearray(unit * 40)
    for at in (33, 90, 151, 200, 260):
        body[at] = ord("T") if body[at] != ord("T") else ord("G")
    chrom = (_random(3_000, 14) + bytes(body) + b"N" * 200 + _random(5_000, 15)).decode().lower()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\nACGT\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    plain, named = tmp_path / "plain.tsv", tmp_path / "named.tsv"
    base = [str(fa), "-i", "chrT:100-8000", "--max-motif-size", "40", "--min-seed", "10", "--max-gap", "8", "--min-chain", "30", "--chain-window", "1000"]
    cli.main(base + ["--chains-tsv", str(plain)], context=ctx)
    cli.main(base + ["--chains-tsv", str(named), "--consensus"], context=ctx)
    old, new = plain.read_text().splitlines(), named.read_text().splitlines()
    assert len(old) == len(new) >= 1
    for before, line in zip(old, new):
        assert line.startswith(before + "\t")
        _, a, b, k = before.split("\t")[:4]
        a, b, k = int(a), int(b), int(k)
        rows, motifs, _ = M.consensus(chrom, M.repeats((a - 100, b - 100, k)), 100, 8_000)
        assert line[len(before) + 1:].split("\t") == [motifs[0], f"{rows['agree'][0] / (b - a):.4f}", str(pn.primitive_period(motifs[0])),
                                                     pn.canonical_motif(motifs[0])]
    seven = [line.split("\t") for line in new if line.split("\t")[3] == "7"]
    assert len(seven) == 1 and seven[0][11] == "7" and seven[0][12] == pn.canonical_motif(unit.decode()) and float(seven[0][10]) > 0.97
    shift = (int(seven[0][1]) - 3_000) % 7
    assert seven[0][9] == (unit[shift:] + unit[:shift]).decode()              # the planted unit, where the first k bases carry a substitution or not
    for floor, seven_stays in (("0.97", True), ("1.0", False)):                # five substitutions in 280 positions
        cli.main(base + ["--chains-tsv", str(named), "--consensus", "--min-consensus-identity", floor], context=ctx)
        kept = named.read_text().splitlines()
        assert kept == [line for line in new if float(line.split("\t")[10]) >= float(floor)]
        assert ("\t".join(seven[0]) in kept) == seven_stays
