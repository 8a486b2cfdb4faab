"""GPU (-m gpu): the exact dot plot of two ranges on either strand (prf_dotpair_bits / prf_dotpair_counts, csrc/dotplot_pair.hip,
DESIGN 12) against the fixture filtered by the reference (tests/golden/dotpair.jsonl.gz) and the numpy model
(tests/dotpair_model.py): ranges on different contigs and overlapping ranges of one, begins off a word on each side
independently, ends at a contig's end and inside it, windows at the corners and across the tile, span and launch boundaries of
the launch shape, both plane sets, and the four identities of DESIGN 12.4: pair(A, A, +) is the self plot, the transpose swaps
the ranges, the minus strand is the plus strand of the reverse complement with mirrored columns, counts are block sums.

The windows are 130-200 rows x 200-260 columns at large coordinates, as small as the kernel can still go wrong in; one window
per threshold is as wide as a workgroup's span (62 or 30 words of 64 columns) plus 200 columns."""
import random

import numpy as np
import pytest

import dotpair_model as P
from conftest import load_jsonl_gz

pytestmark = pytest.mark.gpu

THRESHOLDS = [0, 2, 3, 5, 19, 64]


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


def _contig(n, seed, iupac, pieces):
    """Random ACGT with an N block, the given (position, piece) pairs written over it, N up to its last position (the guard gap
    behind it is N too and must not match) and, with iupac, stretches of letters outside ACGTN."""
    s = bytearray(_random(n, seed))
    s[500:700] = b"N" * 200
    for at, piece in pieces:
        s[at:at + len(piece)] = piece
    s[n - 40:] = b"N" * 40
    if iupac:
        rng = random.Random(seed + 1)
        for at in (300, 4000, n // 2, n - 100):
            s[at:at + 24] = bytes(rng.choice(b"RYKMSWBVDHN") for _ in range(24))
    return bytes(s)


@pytest.fixture(scope="module")
def three_contigs(ctx):
    """100 positions of nothing but N, a contig of 65 536 (ends on a tile boundary of the genome) and one of 70 001 with IUPAC
    letters; the second holds pieces of the third: copied, reverse-complemented, reversed and complemented."""
    u = _random(300, 7) + b"RYKMBVDHSWN" * 4 + _random(120, 8)
    long_ = _contig(70_001, 50, True, [(20_000, u), (69_500, u[:260]), (1_000, _random(9, 3) * 40)])
    mid = _contig(65_536, 40, False, [(30_000, u), (31_000, P.revcomp(u)), (32_000, u[::-1]), (33_000, P.comp(u)),
                                       (65_100, P.revcomp(u[:260])), (2_000, _random(9, 3) * 40)])
    seqs = [b"N" * 100, mid, long_]
    g = ctx.load(seqs, 64)
    yield g, seqs
    g.free()


def _check(g, seqs, a, b, strand, t, rows, cols, **kw):
    want = P.kept_bits(seqs[a[0]], seqs[b[0]], strand, t, a[1:], b[1:], rows, cols)
    got = g.dotpair_bits(a, b, strand, t, rows, cols, **kw)
    assert got.dtype == np.uint64 and got.shape == want.shape, (a, b, strand, t, rows, cols, got.shape, want.shape)
    assert np.array_equal(got, want), (a, b, strand, t, rows, cols)
    return got


# ---- 1. the fixture ----

def test_every_fixture_case_through_the_one_shot_bits_call(ctx, golden):
    bad = []
    for c in golden:
        bits, st = ctx.dotpair_bits(c["a"], c["b"], c["strand"], c["t"], with_stats=True)
        want = P.pack_bits(P.fixture_cells(c))
        if bits.shape != want.shape or not np.array_equal(bits, want):
            bad.append(c["tag"])
        assert st.path == 6 and st.positions == len(c["a"]) + len(c["b"]) and st.n_hits == 0
        assert st.scan_ms > 0 or not (c["a"] and c["b"])
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


@pytest.mark.parametrize("set_noise_to", [0, 2])
def test_every_fixture_case_through_dot_plot_matrix(ctx, golden, set_noise_to):
    import plot_dot_plot as cli
    bad = []
    for i, c in enumerate(golden):
        kept = P.fixture_cells(c)
        want = kept + set_noise_to * (P.kept_cells(c["a"], c["b"], c["strand"], 0) & ~kept)
        matrix = cli.dot_plot_matrix(c["a"].lower() if i % 2 else c["a"], c["t"], set_noise_to, context=ctx, versus=c["b"],
                                     strand=c["strand"])
        if matrix.shape != want.shape or not np.array_equal(matrix, want):
            bad.append(c["tag"])
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


def test_dot_plot_matrix_marks_the_cells_of_the_minus_strand_only(ctx):
    import plot_dot_plot as cli
    a, b = "ACGGTCAANNTTGACCGA", "TCGGTCAANNTTGACCGT"
    plus, minus = P.kept_cells(a, b, "+", 3), P.kept_cells(a, b, "-", 3)
    raw = P.kept_cells(a, b, "+", 0) | P.kept_cells(a, b, "-", 0)
    want = np.where(plus, 1, np.where(minus, cli.MINUS_ONLY, 0))
    assert (want == cli.MINUS_ONLY).any() and (plus & minus).any()                 # N == N is kept on both strands
    assert np.array_equal(cli.dot_plot_matrix(a, 3, 0, context=ctx, versus=b, strand="both"), want)
    assert np.array_equal(cli.dot_plot_matrix(a, 3, 2, context=ctx, versus=b, strand="both"), want + 2 * (raw & ~plus & ~minus))
    assert np.array_equal(cli.dot_plot_matrix(a, 3, 0, context=ctx, strand="-"), P.kept_cells(a, a, "-", 3))


# ---- 2. ranges and windows on a resident genome ----

def _ranges(seqs):
    """(a, b) pairs of (contig, begin, end): different contigs with na != nb both ways, overlapping ranges of one contig, begins
    off a word on each side independently, a range ending with its contig (end None) and an inner end, each followed by letters
    that would match if read (the planted copies end exactly at an end, and go on behind it).  A contig starts at a multiple
    of 65 536 in the genome, so a begin's offset within a word of the planes is the begin modulo 64."""
    n1, n2 = len(seqs[1]), len(seqs[2])
    return [((1, 28_992, 34_000), (2, 19_937, 20_600)),          # na > nb; a begin on a word (453 * 64) against one 33 bits off
            ((2, 19_999, 20_500), (1, 29_952, 33_700)),          # na < nb; the other way round: 31 bits off against 468 * 64
            ((1, 1_987, 2_400), (1, 2_001, 2_900)),              # overlapping ranges of one contig, through the tandem stretch
            ((2, 69_300, None), (1, 64_900, None)),              # both end with their contigs: N up to the last position
            ((2, 20_063, 20_300), (1, 30_001, 30_200)),          # inner ends inside the copy: the letters behind them would match
            ((1, 31_000 + 131, 31_000 + 400), (2, 20_000 + 1, 20_000 + 300)),   # the same on the reverse-complemented piece
            ((0, 3, 90), (1, 480, 720)),                         # nothing but N against the N block
            ((2, 0, n2), (1, 0, n1))]                            # whole contigs: windows at large coordinates only


def _windows(na, nb, t):
    import prf_native
    tile_rows, span_words, _halo = prf_native.dotplot_shape(t)
    span = 64 * span_words
    out = [((0, 130), (0, 230)), ((0, 130), (nb - 230, nb + 9)), ((na - 130, na), (0, 260)), ((na - 140, na + 50), (nb - 215, nb + 50)),   # corners
           ((tile_rows - 7, tile_rows - 7 + 150), (37, 37 + 250)),         # tile-row boundaries, col0 off a word
           ((5, 5 + tile_rows + 6), (130, 130 + span + 200)),              # across a column-span boundary
           ((na // 2, na // 2), (0, 200)), ((10, 90), (nb, nb + 5)), ((na + 5, na + 9), (0, 100))]   # empty windows
    return [w for w in out if min(w[0][0], w[1][0]) >= 0]


@pytest.mark.parametrize("strand", ["+", "-"])
@pytest.mark.parametrize("t", THRESHOLDS)
def test_windows_of_ranges_of_three_contigs(three_contigs, t, strand):
    g, seqs = three_contigs
    kept = 0
    for a, b in _ranges(seqs):
        na = (len(seqs[a[0]]) if a[2] is None else a[2]) - a[1]
        nb = (len(seqs[b[0]]) if b[2] is None else b[2]) - b[1]
        for rows, cols in _windows(na, nb, t):
            kept += int(_check(g, seqs, a, b, strand, t, rows, cols).any())
    assert kept >= 3                                                          # (the N ranges at the least: no vacuous pass)
    # the planted pieces, where the whole contigs meet: copy and reversed piece on plus, the other two on minus
    for at in (30_000, 31_000, 32_000, 33_000):                               # (rows: the first 130 of the piece's 464 letters)
        c0 = at if at in (30_000, 33_000) else at + 300
        got = _check(g, seqs, (2, 0, None), (1, 0, None), strand, t, (20_000, 20_000 + 130), (c0, c0 + 200))
        if t == 64:
            assert got.any() == ((at in (30_000, 32_000)) == (strand == "+")), at


@pytest.mark.parametrize("t", THRESHOLDS)
def test_a_window_cut_into_several_launches(three_contigs, t):
    g, seqs = three_contigs
    a, b = (2, 19_900, 20_700), (1, 30_950, 31_500)
    # 260 rows: five tiles of rows.  The reverse-complemented piece (rows 100 .., columns .. 513 of these ranges) crosses the
    # window as an anti-diagonal of 230 cells through all four cuts: at t = 64 the halo of a tile reaches 62 rows into its neighbours
    rows, cols = (70, 70 + 260), (250, 250 + 233)
    for strand in "+-":
        one, st1 = g.dotpair_bits(a, b, strand, t, rows, cols, with_stats=True)
        assert one.any() or (strand == "+" and t >= 19)                       # (plus: chance runs only, none that long)
        cut, st = g.dotpair_bits(a, b, strand, t, rows, cols, with_stats=True, launch_cells=64 * 233)     # one tile per launch
        assert st1.n_launches == 1 and st.n_launches == 5 and st.path == 6 and st.positions == 800 + 550
        assert np.array_equal(cut, one) and np.array_equal(one, P.kept_bits(seqs[2], seqs[1], strand, t, a[1:], b[1:], rows, cols))
        cut, st = g.dotpair_bits(a, b, strand, t, rows, cols, with_stats=True, launch_cells=2 * 64 * 233 + 5)
        assert st.n_launches == 3 and np.array_equal(cut, one)
        counts = g.dotpair_counts(a, b, 128, strand, t, rows, cols)
        cut, st = g.dotpair_counts(a, b, 128, strand, t, rows, cols, with_stats=True, launch_cells=1)    # never less than a tile
        assert st.n_launches == 5 and np.array_equal(cut, counts)
        assert np.array_equal(counts, P.block_sums(P.kept_cells(seqs[2], seqs[1], strand, t, a[1:], b[1:], rows, cols), 128))


# ---- 3. the identities ----

@pytest.mark.parametrize("t", [3, 64])
def test_a_range_against_itself_on_plus_is_the_self_plot(three_contigs, t):
    g, seqs = three_contigs
    n = len(seqs[2])
    for begin, end, rows, cols in ((0, None, (n - 200, n), (n - 260, n)), (19_937, 20_700, (0, 300), (37, 600)),
                                   (65, None, (900, 1_100), (930, 930 + 64 * 62 + 200))):
        a = (2, begin, end)
        pair = g.dotpair_bits(a, a, "+", t, rows, cols)
        self_plot = g.dotplot_bits(2, t, begin, end, rows, cols)
        assert self_plot.any() and np.array_equal(pair, self_plot), (begin, end, rows, cols)


@pytest.mark.parametrize("strand", ["+", "-"])
def test_the_transpose_swaps_the_ranges(three_contigs, strand):
    import prf_native
    g, seqs = three_contigs
    a, b = (2, 19_800, 21_000), (1, 29_900, 34_000)
    rows, cols = (100, 100 + 1_024), (1_000 if strand == "-" else 0, (1_000 if strand == "-" else 0) + 640)
    for t in (3, 8):
        ab = prf_native.unpack_bits(g.dotpair_bits(a, b, strand, t, rows, cols), 640)
        ba = prf_native.unpack_bits(g.dotpair_bits(b, a, strand, t, cols, rows), 1_024)
        assert ab.shape == (1_024, 640) and ab.any() and np.array_equal(ab, ba.T)
        assert np.array_equal(ab[:100, :300], P.kept_cells(seqs[2], seqs[1], strand, t, a[1:], b[1:], (100, 200), (cols[0], cols[0] + 300)))


def test_minus_is_plus_of_the_reverse_complement_with_mirrored_columns(ctx):
    import prf_native
    u = _random(200, 31)
    a = _random(150, 32) + u + _random(77, 33, b"ACGTRYKMSWBVDHN")
    b = _random(61, 34, b"ACGTN") + P.revcomp(u) + _random(300, 35, b"ACGTRYKMSWBVDHN")
    for t in (0, 3, 5, 64):
        minus = prf_native.unpack_bits(ctx.dotpair_bits(a, b, "-", t), len(b))
        plus = prf_native.unpack_bits(ctx.dotpair_bits(a, P.revcomp(b), "+", t), len(b))
        assert minus.shape == (len(a), len(b)) and np.array_equal(minus, plus[:, ::-1]), t
        # the planted inverted repeat: an anti-diagonal run of 200 cells of the minus matrix
        assert all(minus[150 + k, 61 + 199 - k] for k in range(200))
    assert np.array_equal(minus, P.kept_cells(a, b, "-", 64))
    window = ctx.dotpair_bits(a, b, "-", 64, a=(100, 400), b=(30, 300), rows=(10, 200), cols=(5, 270))
    assert np.array_equal(window, P.kept_bits(a, b, "-", 64, (100, 400), (30, 300), (10, 200), (5, 270)))


@pytest.mark.parametrize("block", [64, 128, 4096])
def test_counts_equal_the_block_sums_of_the_bits(three_contigs, block):
    import prf_native
    g, seqs = three_contigs
    for a, b, strand, t, rows, cols in (((2, 19_937, 20_700), (1, 29_000, 34_000), "+", 3, (10, 10 + 333), (300, 300 + 4_500)),
                                        ((2, 19_937, 20_700), (1, 29_000, 34_000), "-", 5, (0, 763), (1_900, 2_500)),
                                        ((1, 0, None), (2, 0, None), "-", 0, (64_000, 64_130), (64, 64 + 8_500)),
                                        ((2, 69_300, None), (1, 64_900, None), "-", 64, (0, 701), (0, 636))):
        bits = g.dotpair_bits(a, b, strand, t, rows, cols)
        cells = prf_native.unpack_bits(bits, cols[1] - cols[0])
        counts, st = g.dotpair_counts(a, b, block, strand, t, rows, cols, with_stats=True)
        assert counts.dtype == np.uint32 and st.path == 6 and st.scan_ms > 0 and cells.any()
        assert np.array_equal(counts, P.block_sums(cells, block)), (a, b, strand, t, block)
        again = g.dotpair_counts(a, b, block, strand, t, rows, cols)
        assert np.array_equal(again, counts)                                  # the output is zeroed per call
    assert g.dotpair_counts((2, 0, None), (1, 0, None), block, "-", 3, (5, 5), (0, 100)).shape == (0, -(-100 // block))


def test_a_contig_the_genome_does_not_hold_is_refused(three_contigs):
    import prf_native
    g, _ = three_contigs
    buf = np.zeros(64, dtype=np.uint64)
    n0, st = prf_native.ctypes.c_uint64(0), prf_native.ScanStats()
    rc = g.ctx.lib.prf_dotpair_bits(g.ctx._h, g._h, 1, 0, 10, 3, 0, 10, 0, 0, 10, 0, 10, 3, buf.ctypes.data, 64,
                                    prf_native.ctypes.byref(n0), prf_native.ctypes.byref(st))
    assert rc == prf_native.PRF_EINVAL and "contig 3" in g.ctx.lib.prf_last_error().decode()


# ---- 4. neighbours ----

def test_scans_and_period_counts_are_not_disturbed(ctx):
    import torch
    import prf_native
    tile = prf_native.tile_positions()
    seq = bytearray(_random(3 * tile + 500, 13))
    for at in range(1000, len(seq) - 200, 9_973):
        seq[at:at + 60] = b"CAG" * 20
    seq = bytes(seq)
    g = ctx.load([seq, _random(900, 14)], 50)
    seqs = [seq, _random(900, 14)]
    cap = 100_000
    buf = torch.empty((cap + 1, 3), dtype=torch.int64, device="cuda")
    try:
        g.select([(0, tile, 3 * tile)])
        ctx.set_row_sink(buf.data_ptr(), cap)
        before, _ = g.scan(1, 50, 3, 9)
        sink_before = buf.cpu().numpy().copy()
        period_before = g.period_counts(0, 1, 50, 1024)
        _check(g, seqs, (0, 900, 1_300), (1, 0, None), "-", 3, (0, 200), (650, 900))      # whatever is selected
        counts = g.dotpair_counts((0, 100, 5_000), (0, 1_000, 1_400), 64, "+", 3, (0, 300), (0, 300))
        assert np.array_equal(counts, P.block_sums(P.kept_cells(seq, seq, "+", 3, (100, 5_000), (1_000, 1_400), (0, 300), (0, 300)), 64))
        assert np.array_equal(buf.cpu().numpy(), sink_before)                 # nothing was written to the sink
        assert np.array_equal(g.period_counts(0, 1, 50, 1024), period_before)
        after, _ = g.scan(1, 50, 3, 9)
        assert len(before) > 10 and np.array_equal(before, after)
        assert before["start"].min() >= tile and before["start"].max() < 3 * tile
        assert np.array_equal(buf.cpu().numpy(), sink_before)
    finally:
        ctx.set_row_sink(None, 0)
        g.select([])
        g.free()


def test_cli_writes_rectangular_plots_and_counts(ctx, tmp_path):
    import plot_dot_plot as cli
    from PIL import Image
    u = _random(150, 41)
    chrom = (_random(3_000, 14) + u + b"N" * 200 + _random(2_000, 15)).decode()
    other = (_random(400, 16) + P.revcomp(u) + _random(250, 17)).decode()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\n" + other + "\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    cli.main(["-R", str(fa), "chrT:2900-3300", "--versus", "other:300-600", "--strand", "both", "-d", str(tmp_path), "-w", "4",
              "--show-filtered-pixels"], context=ctx)
    with Image.open(tmp_path / "dot_plot_001_of_1.chrT_2900-3300.400bp_sequence.png") as image:
        width, height = image.size
        assert image.format == "PNG" and abs(width / height - 300 / 400) < 0.03
        colours = {c[:3] for _, c in image.convert("RGB").getcolors(1 << 20)}
    assert {(255, 255, 255), (0, 0, 0), (255, 0, 0), (65, 105, 225)} <= colours          # royalblue: the inverted repeat
    tsv, out = tmp_path / "density.tsv", tmp_path / "density.png"
    cli.main(["-R", str(fa), "chrT:2500-4900", "--versus", "other:0-800", "--strand=-", "--block", "128", "--tsv", str(tsv), "-o", str(out),
              "-d", str(tmp_path)], context=ctx)
    counts = P.block_sums(P.kept_cells(chrom, other, "-", 3, (2500, 4900), (0, 800)), 128)
    assert counts.shape == (19, 7) and counts.any()
    assert tsv.read_text() == "".join(cli.density_lines("chrT", 2500, 2400, 128, counts, 0, 800))
    with Image.open(tmp_path / "dot_plot_001_of_1.chrT_2500-4900.2400bp_sequence.png") as image:
        assert image.format == "PNG" and image.size[0] < image.size[1]
