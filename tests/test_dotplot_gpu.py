"""GPU (-m gpu): the exact dot plot (prf_dotplot_bits / prf_dotplot_counts, csrc/dotplot.hip) against the reference's
generate_matrix + filter_out_noise fixture (tests/golden/dotplot.jsonl.gz) and the numpy model (tests/dotplot_model.py): windows
at the corners, across both diagonals, across the tile, span and launch boundaries of the launch shape, ranges that begin
anywhere and end inside or with a contig, both plane sets, counts against the block sums of the bits, the symmetry of the
matrix, and that a dot-plot call leaves the scans and the periodicity calls alone.

The windows are 200 rows x 200-260 columns, as small as the kernel can still go wrong in; one window per threshold is as wide
as a workgroup's span (62 or 30 words of 64 columns) plus 200 columns, because a span boundary lies that far from col0."""
import random

import numpy as np
import pytest

import dotplot_model as D
from conftest import load_jsonl_gz

pytestmark = pytest.mark.gpu

THRESHOLDS = [0, 2, 3, 5, 64]
BEGINS = [0, 1, 63, 64, 65, 1000]


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
    return load_jsonl_gz("dotplot.jsonl.gz")


def _random(n, seed, alphabet=b"ACGT"):
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


def _planted(n, seed, iupac):
    """A contig with N blocks, planted tandem units of 1-40, palindromes, (IUPAC letters,) and N up to its last position."""
    rng = random.Random(seed)
    s = bytearray(_random(n, seed + 1))
    s[500:700] = b"N" * 200
    at = 1100
    for unit in range(1, 41):
        piece = _random(unit, seed + 100 + unit) * (3 + 120 // unit)
        s[at:at + len(piece)] = piece
        at += len(piece) + rng.randrange(5, 90)
    for k in range(12):
        u = _random(rng.randrange(4, 70), seed + 300 + k, b"ACGTN" if k % 3 == 0 else b"ACGT")
        where = rng.randrange(at, n - 400)
        s[where:where + 2 * len(u)] = u + u[::-1]
    s[n - 330:n - 130] = _random(7, seed + 2) * 28 + b"CAGT"         # a tandem stretch near the end
    s[n - 40:] = b"N" * 40                                             # N up to the last position: the guard gap must not match
    if iupac:
        for where in (300, 4000, n // 2, n - 100):
            s[where:where + 24] = bytes(rng.choice(b"RYKMSWN") for _ in range(24))
        s[n - 420:n - 360] = b"RYK" * 20
    return bytes(s)


@pytest.fixture(scope="module")
def three_contigs(ctx):
    """100 positions of nothing but N in front, a contig that ends on a tile boundary of the genome, one that crosses one."""
    seqs = [b"N" * 100, _planted(65_536, 40, False), _planted(70_001, 50, True)]
    g = ctx.load(seqs, 64)
    yield g, seqs
    g.free()


def _windows(n, t):
    """(rows, cols) pairs for a matrix of n x n: what the issue lists, with the boundaries taken from the launch shape."""
    import prf_native
    tile_rows, span_words, _halo = prf_native.dotplot_shape(t)
    span = 64 * span_words
    mid = (n // 2) | 1
    out = [((0, 200), (0, 230)), ((0, 200), (n - 230, n)), ((n - 200, n), (0, 260)), ((n - 200, n + 50), (n - 215, n + 50)),   # corners
           ((mid, mid + 200), (mid - 30, mid + 200)),                         # across the main diagonal
           ((mid, mid + 200), (n - 1 - mid - 230, n - 1 - mid + 30)),         # across the anti-diagonal i + j = n - 1
           ((tile_rows - 7, tile_rows - 7 + 200), (37, 37 + 250)),            # tile-row boundaries (3 of them), col0 not a multiple of 64
           ((n - 300, n - 100), (n - 301, n - 101)),                          # the tandem stretch near the end, col0 odd
           ((5, 5 + tile_rows + 6), (130, 130 + span + 200)),                 # across a column-span boundary
           ((900, 900), (0, 200)), ((10, 210), (n, n + 5)), ((n + 5, n + 9), (0, 100))]   # empty windows
    return [w for w in out if min(w[0][0], w[1][0]) >= 0]


def _check(g, contig, seq, t, begin, end, rows, cols, **kw):
    want = D.kept_bits(seq, t, begin, end, rows, cols)
    got = g.dotplot_bits(contig, t, begin, end, rows, cols, **kw)
    assert got.dtype == np.uint64 and got.shape == want.shape, (contig, t, begin, end, rows, cols, got.shape, want.shape)
    assert np.array_equal(got, want), (contig, t, begin, end, rows, cols)
    return got


# ---- 1. the fixture ----

def test_every_fixture_case_through_the_one_shot_bits_call(ctx, golden):
    bad = []
    for c in golden:
        bits, st = ctx.dotplot_bits(c["seq"], c["t"], with_stats=True)
        want = D.pack_bits(D.fixture_cells(c))
        if bits.shape != want.shape or not np.array_equal(bits, want):
            bad.append(c["tag"])
        assert st.path == 5 and st.positions == len(c["seq"]) and st.n_hits == 0 and (st.scan_ms > 0 or not c["seq"])
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


@pytest.mark.parametrize("set_noise_to", [0, 2])
def test_every_fixture_case_through_dot_plot_matrix(ctx, golden, set_noise_to):
    import plot_dot_plot as cli
    bad = []
    for i, c in enumerate(golden):
        kept = D.fixture_cells(c)
        want = kept + set_noise_to * (D.kept_cells(c["seq"], 0) & ~kept)
        matrix = cli.dot_plot_matrix(c["seq"].lower() if i % 2 else c["seq"], c["t"], set_noise_to, context=ctx)     # any case
        if matrix.shape != want.shape or not np.array_equal(matrix, want):
            bad.append(c["tag"])
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"
    raw = cli.generate_matrix("ACGNnRA", context=ctx)
    assert raw == [[int(a == b) for a in "ACGNNRA"] for b in "ACGNNRA"]


# ---- 2. tile, span, word and launch boundaries ----

@pytest.mark.parametrize("t", THRESHOLDS)
def test_windows_of_three_contigs(three_contigs, t):
    g, seqs = three_contigs
    done = 0
    for k, begin in enumerate(BEGINS):
        contig = 2 if k % 3 else 1
        seq = seqs[contig]
        for end in (None, len(seq) - 37 - k):                # the contig's end (clipped: END_OF_CONTIG), an inner end
            n = (len(seq) if end is None else end) - begin
            for rows, cols in _windows(n, t):
                _check(g, contig, seq, t, begin, end, rows, cols)
                done += 1
    assert done == 6 * 2 * 12
    _check(g, 0, seqs[0], t, 0, None, None, None)            # the contig of nothing but N, whole: all cells, or none
    _check(g, 0, seqs[0], t, 3, 70, (0, 67), (1, 66))


@pytest.mark.parametrize("t", [2, 3, 64])
def test_a_window_cut_into_several_launches(three_contigs, t):
    g, seqs = three_contigs
    seq, n = seqs[1], len(seqs[1])
    rows, cols = (n - 330, n - 70), (n - 333, n - 100)                     # 260 rows: five tiles of rows
    one, st1 = g.dotplot_bits(1, t, 0, None, rows, cols, with_stats=True)
    cut, st = g.dotplot_bits(1, t, 0, None, rows, cols, with_stats=True, launch_cells=64 * 233)     # one tile per launch
    assert st1.n_launches == 1 and st.n_launches == 5
    assert np.array_equal(cut, one) and np.array_equal(one, D.kept_bits(seq, t, 0, None, rows, cols))
    cut, st = g.dotplot_bits(1, t, 0, None, rows, cols, with_stats=True, launch_cells=1)            # never less than a tile
    assert st.n_launches == 5 and np.array_equal(cut, one)
    cut, st = g.dotplot_bits(1, t, 0, None, rows, cols, with_stats=True, launch_cells=2 * 64 * 233 + 5)
    assert st.n_launches == 3 and np.array_equal(cut, one)
    counts = g.dotplot_counts(1, 128, t, 0, None, rows, cols)
    cut, st = g.dotplot_counts(1, 128, t, 0, None, rows, cols, with_stats=True, launch_cells=64 * 233)
    assert st.n_launches == 5 and np.array_equal(cut, counts)
    assert np.array_equal(counts, D.block_sums(D.kept_cells(seq, t, 0, None, rows, cols), 128))


# ---- 3. both plane sets, and the guard gap ----

@pytest.mark.parametrize("iupac", [False, True])
def test_the_guard_gap_does_not_match(ctx, iupac):
    """The gap behind a contig is packed as N and N == N matches: the halo of the last rows and columns reaches into it, and
    an inner `end` puts real N behind the range."""
    n = 3000
    s = bytearray(_random(n, 60 + iupac))
    s[n - 90:] = b"N" * 90
    s[n - 300:n - 200] = b"N" * 100
    if iupac:
        s[1000:1030] = b"RYKRYKRRYYKKNNRYKMSWRYKRYKRYKN"
        s[n - 95:n - 90] = b"RRRRR"
    seq = bytes(s)
    g = ctx.load([seq, b"N" * 500], 64)
    try:
        for t in (0, 3, 5, 64):
            for end in (None, n - 30, n - 250):
                m = n if end is None else end
                got = _check(g, 0, seq, t, 7, end, (m - 7 - 150, m), (m - 7 - 140, m + 64))
                if t == 5:
                    assert got[-1, -1]                                    # the diagonal is kept up to the corner
        _check(g, 1, b"N" * 500, 64, 0, None, (400, 500), (0, 500))
    finally:
        g.free()


# ---- 4. counts ----

@pytest.mark.parametrize("block", [64, 128, 4096])
def test_counts_equal_the_block_sums_of_the_bits(three_contigs, block):
    import prf_native
    g, seqs = three_contigs
    for contig, t, begin, rows, cols in ((2, 3, 65, (10, 10 + 333), (4000, 4000 + 4500)),      # wider than a span, 6 tiles of rows
                                         (1, 5, 0, (65_000, 65_536), (64_900, 65_536)),
                                         (1, 0, 1000, (0, 130), (64, 64 + 8500)),             # spans of block 4096, not whole
                                         (2, 64, 0, (69_700, 70_001), (69_650, 70_001))):
        bits = g.dotplot_bits(contig, t, begin, None, rows, cols)
        cells = prf_native.unpack_bits(bits, cols[1] - cols[0])
        counts, st = g.dotplot_counts(contig, block, t, begin, None, rows, cols, with_stats=True)
        assert counts.dtype == np.uint32 and st.path == 5 and st.scan_ms > 0
        assert np.array_equal(counts, D.block_sums(cells, block)), (contig, t, block)
        again = g.dotplot_counts(contig, block, t, begin, None, rows, cols)
        assert np.array_equal(again, counts)                                  # the output is zeroed per call
    assert g.dotplot_counts(2, block, 3, 0, None, (5, 5), (0, 100)).shape == (0, -(-100 // block))


# ---- 5. symmetry ----

def test_the_matrix_is_symmetric(three_contigs):
    import prf_native
    g, seqs = three_contigs
    a, b = (1500, 2524), (1100, 2124)                                         # across the diagonal, through the planted units
    for t in (3, 8):
        ab = prf_native.unpack_bits(g.dotplot_bits(2, t, 0, None, a, b), 1024)
        ba = prf_native.unpack_bits(g.dotplot_bits(2, t, 0, None, b, a), 1024)
        assert ab.any() and np.array_equal(ab, ba.T)
        assert np.array_equal(ab[:100, :300], D.kept_cells(seqs[2], t, 0, None, (1500, 1600), (1100, 1400)))


# ---- 6. neighbours ----

def test_scans_and_period_counts_are_not_disturbed(ctx):
    import torch
    import prf_native
    tile = prf_native.tile_positions()
    seq = bytearray(_random(3 * tile + 500, 13))
    for at in range(1000, len(seq) - 200, 9_973):
        seq[at:at + 60] = b"CAG" * 20
    seq = bytes(seq)
    g = ctx.load([seq], 50)
    cap = 100_000
    buf = torch.empty((cap + 1, 3), dtype=torch.int64, device="cuda")
    try:
        g.select([(0, tile, 3 * tile)])
        ctx.set_row_sink(buf.data_ptr(), cap)
        before, _ = g.scan(1, 50, 3, 9)
        sink_before = buf.cpu().numpy().copy()
        period_before = g.period_counts(0, 1, 50, 1024)
        _check(g, 0, seq, 3, 0, None, (900, 1100), (850, 1100))              # whatever is selected
        counts = g.dotplot_counts(0, 64, 3, 100, 5000, (0, 300), (0, 300))
        assert np.array_equal(counts, D.block_sums(D.kept_cells(seq, 3, 100, 5000, (0, 300), (0, 300)), 64))
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


def test_matrix_calls_wait_for_pipelined_scans_and_fill_their_stats(ctx):
    """What the two matrix products share on the host: all four calls are refused, under their own names, while a pipelined
    scan holds a slot (until scan_wait, whether or not its kernel has finished), leave that scan alone, serve afterwards, and
    fill the stats of a lane that waits for its own kernels."""
    import prf_native
    import periodicity_model as P
    seq = _random(4096, 21)
    g = ctx.load([seq], 64)                                                   # one launched tile
    win = dict(rows=(0, 64), cols=(0, 64))
    calls = [("prf_period_bits", lambda: g.period_bits(0, 1, 4)),
             ("prf_period_counts", lambda: g.period_counts(0, 1, 4, 64)),
             ("prf_dotplot_bits", lambda: g.dotplot_bits(0, **win)),
             ("prf_dotplot_counts", lambda: g.dotplot_counts(0, 64, **win))]
    try:
        _, sync = g.scan(1, 6, 3, 9)                                          # sizes the buffers
        pending = g.scan_async(1, 6, 3, 9)
        try:
            for name, call in calls:
                with pytest.raises(prf_native.PrfError) as info:
                    call()
                assert info.value.code == prf_native.PRF_EINVAL, name
                assert "pipelined scans are in flight" in info.value.message and f"{name}:" in info.value.message
        finally:
            waited = ctx.scan_wait(pending)
        assert waited.n_hits == sync.n_hits
        got = [call() for _, call in calls]
        cells = D.kept_cells(seq, 3, 0, None, (0, 64), (0, 64))
        want = [P.period_bits(seq, 1, 4), P.period_counts(seq, 1, 4, 64), D.pack_bits(cells), D.block_sums(cells, 64)]
        for (name, _), a, b in zip(calls, got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
        _, st = g.period_bits(0, 1, 4, with_stats=True)
        assert (st.path, st.n_launches, st.n_hits, st.positions, st.packed_bytes) == (4, 1, 0, 4096, 1024)
        empty, st = g.period_bits(0, 1, 4, begin=100, end=100, with_stats=True)
        assert empty.shape == (4, 0) and st.n_launches == 0 and st.scan_ms == 0 and st.path == 4
        _, st = g.dotplot_bits(0, with_stats=True, **win)
        assert (st.path, st.n_launches, st.packed_bytes) == (5, 1, 1024)
    finally:
        g.free()


def test_cli_writes_plots_density_and_counts(ctx, tmp_path, capsys):
    import plot_dot_plot as cli
    from PIL import Image
    chrom = (_random(3_000, 14) + b"ACGGT" * 300 + b"N" * 200 + _random(2_000, 15)).decode()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\nACGT\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    cli.main(["-R", str(fa), "chrT:2900-3100", "-d", str(tmp_path), "--show-filtered-pixels", "-w", "3"], context=ctx)
    png = tmp_path / "dot_plot_001_of_1.chrT_2900-3100.200bp_sequence.png"
    with Image.open(png) as image:
        assert image.format == "PNG" and image.size[0] == image.size[1]
        assert (255, 0, 0) in {c[:3] for _, c in image.convert("RGB").getcolors(1 << 20)}
    tsv, out = tmp_path / "density.tsv", tmp_path / "density.png"
    cli.main(["-R", str(fa), "chrT:2500-4900", "--block", "128", "--tsv", str(tsv), "-o", str(out), "-d", str(tmp_path)], context=ctx)
    counts = D.block_sums(D.kept_cells(chrom, 3, 2500, 4900), 128)
    assert tsv.read_text() == "".join(cli.density_lines("chrT", 2500, 2400, 128, counts)) and counts.shape == (19, 19)
    assert (tmp_path / "dot_plot_001_of_1.chrT_2500-4900.2400bp_sequence.png").read_bytes()[:4] == b"\x89PNG"
    capsys.readouterr()
    cli.main(["CAGCAGCAGCAGTTTCTGCTGCTG", "-o", "lit.png", "-d", str(tmp_path)], context=ctx)
    assert (tmp_path / "lit.png").read_bytes()[:4] == b"\x89PNG" and "Loaded" not in capsys.readouterr().out
