"""GPU (-m gpu): the periodicity matrix and the windowed period counts (prf_period_bits / prf_period_counts, csrc/periodicity.hip,
DESIGN 10) against the reference's get_period_matrix fixture (tests/golden/periodicity.jsonl.gz) and the numpy model
(tests/periodicity_model.py): ranges that begin anywhere, contigs that end on and cross a tile boundary, every path of the
kernel (one LDS region and two, one slice of motif sizes and several, with and without letters outside ACGTN), and that a
periodicity call leaves the scans alone."""
import os
import random

import numpy as np
import pytest

import periodicity_model as P
from conftest import load_jsonl_gz
from test_periodicity_cpu import clamped, fixture_cells, partition

pytestmark = pytest.mark.gpu


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
    return load_jsonl_gz("periodicity.jsonl.gz")


def _random(n, seed, alphabet=b"ACGT"):
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


def _use_ctx(monkeypatch, ctx):
    """The command-line tools take the process-wide context: hand them this module's."""
    import prf_native
    device = int(os.environ.get("PRF_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    monkeypatch.setitem(prf_native._default_ctx, device, ctx)


def _check_range(genome, contig, seq, kmin, kmax, begin, end, windows):
    """bits and counts of one range against the model; counts also against the popcount of the bits."""
    cells = P.period_cells(seq, kmin, kmax, begin, end)
    bits, st = genome.period_bits(contig, kmin, kmax, begin, end, with_stats=True)
    assert bits.dtype == np.uint64 and np.array_equal(bits, P.pack_bits(cells)), (contig, begin, end)
    assert st.path == 4 and st.positions == cells.shape[1] and (st.scan_ms > 0 or cells.shape[1] == 0)
    for window in windows:
        counts = genome.period_counts(contig, kmin, kmax, window, begin, end)
        assert counts.dtype == np.uint32 and np.array_equal(counts, P.window_sums(cells, window)), (contig, begin, end, window)
        assert np.array_equal(counts, P.popcount_per_window(bits, window))


def test_every_fixture_case_through_the_one_shot_bits_call(ctx, golden):
    bad = []
    for c in golden:
        lo, hi = clamped(c)
        if hi < lo:
            continue
        bits = ctx.period_bits(c["seq"], lo, hi)
        want = P.pack_bits(fixture_cells(c)[lo - 1:])
        if bits.shape != want.shape or not np.array_equal(bits, want):
            bad.append(c["tag"])
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


def test_every_fixture_case_through_get_period_matrix(ctx, golden):
    from utils.plot_utils import get_period_matrix
    bad = []
    for i, c in enumerate(golden):
        matrix = get_period_matrix(c["min"], c["max"], c["seq"].lower() if i % 2 else c["seq"], context=ctx)   # any case
        assert len(matrix) == c["shape"][0] and all(len(row) == c["shape"][1] for row in matrix)
        if [[bool(v) for v in row] for row in matrix] != fixture_cells(c).tolist():
            bad.append(c["tag"])
        elif [partition(row) for row in matrix] != c["classes"]:
            bad.append(c["tag"])
    assert not bad, f"{len(bad)} cases differ: {bad[:5]}"


@pytest.fixture(scope="module")
def three_contigs(ctx):
    """100 positions, a contig that ends on a tile boundary, one that crosses one."""
    seqs = []
    for i, n in enumerate((100, 65_536, 70_001)):
        s = bytearray(_random(n, 100 + i))
        if n > 1000:
            s[500:700] = b"N" * 200
            s[n - 900:n - 300] = b"CAGT" * 150
            s[n - 40:] = b"N" * 40                       # N up to the last position: the row must still end with the contig
        seqs.append(bytes(s))
    g = ctx.load(seqs, 200)
    yield g, seqs
    g.free()


@pytest.mark.parametrize("contig", [0, 1, 2])
def test_ranges_of_three_contigs(three_contigs, contig):
    g, seqs = three_contigs
    n = len(seqs[contig])
    done = 0
    for begin in (0, 1, 63, 64, 65_535, 65_537):
        for end in (None, n - 37, n + 1000):             # the whole contig, an inner end, an end the library clips
            if begin > (n if end is None else end):
                continue
            _check_range(g, contig, seqs[contig], 1, 200, begin, end, (64, 128, 4096))
            done += 1
    assert done >= (12 if contig else 10)


def test_long_sequence_with_n_blocks_iupac_and_planted_units(ctx):
    rng = random.Random(5)
    s = bytearray(_random(300_000, 6))
    s[10_000:14_000] = b"N" * 4000
    s[200_000:200_300] = b"n" * 300
    for at in (50_000, 120_001, 250_063):
        s[at:at + 20] = bytes(rng.choice(b"RYKMSWN") for _ in range(20))
    s[60_000:60_000 + 171 * 12] = _random(171, 7) * 12
    s[150_037:150_037 + 1000 * 5] = _random(1000, 8, b"ACGTR") * 5
    seq = bytes(s)
    g = ctx.load([seq], 1024)
    try:
        for k in (1, 63, 64, 65, 127, 128, 171, 1000, 1001):
            _check_range(g, 0, seq, k, k, 0, None, (1024,))
        _check_range(g, 0, seq, 1000, 1001, 149_999, 156_000, (64, 192))
        counts = g.period_counts(0, 171, 171, 4096)
        assert counts[0, 60_000 // 4096] > 1400            # the planted unit of 171 fills the rest of its window
        import prf_native
        with pytest.raises(prf_native.PrfError) as info:
            g.period_bits(0, 1, 1025)                      # above the genome's kmax_hint
        assert info.value.code == prf_native.PRF_EUNSUPPORTED
    finally:
        g.free()


def test_motif_sizes_at_the_limit_and_in_several_slices(ctx):
    seq = _random(200_000, 9)
    g = ctx.load([seq], 60_000)
    try:
        _check_range(g, 0, seq, 59_990, 60_000, 0, None, (64, 65_536))     # the two sides of a row lie 937 words apart
        _check_range(g, 0, seq, 59_999, 60_000, 70_001, 140_000, (128,))    # rows of nothing: k >= the length of the range is all zero
        assert not g.period_bits(0, 59_999, 60_000, 70_001, 130_000).any()
    finally:
        g.free()
    seq = _random(6_000, 10) + b"NNNN" + b"ACGTTG" * 400
    g = ctx.load([seq], 2_100)
    try:
        _check_range(g, 0, seq, 1, 2_100, 3, None, (64, 1024))             # two slices of motif sizes
    finally:
        g.free()
    seq = _random(3_000, 11, b"ACGTRYN") + b"RY" * 300
    g = ctx.load([seq], 1_100)
    try:
        _check_range(g, 0, seq, 1, 1_100, 65, None, (64, 320))             # the same with letters outside ACGTN
    finally:
        g.free()


def test_a_row_ends_with_the_contig_not_in_the_gap(ctx):
    """The guard gap behind a contig is packed as N, and N == N matches here: the kernel clips the row itself."""
    all_n = b"N" * 1000
    other = b"N" * 50 + _random(500, 12)
    g = ctx.load([all_n, other], 64)
    try:
        for k in (1, 7, 64):
            bits = g.period_bits(0, k, k)
            assert int(np.unpackbits(bits.view(np.uint8)).sum()) == 1000 - k
            counts = g.period_counts(0, k, k, 64)
            assert counts.sum() == 1000 - k and counts[0, -1] == max(0, 1000 - 960 - k)
        _check_range(g, 0, all_n, 1, 64, 0, None, (64, 128))
        _check_range(g, 0, all_n, 1, 64, 937, 990, (64,))
        _check_range(g, 1, other, 1, 64, 0, None, (64,))
    finally:
        g.free()


def test_scans_are_not_disturbed(ctx):
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
        _check_range(g, 0, seq, 1, 50, 0, None, (1024,))         # the whole contig, whatever is selected
        _check_range(g, 0, seq, 3, 3, 100, 5000, (64,))
        assert np.array_equal(buf.cpu().numpy(), sink_before)     # nothing was written to the sink
        after, _ = g.scan(1, 50, 3, 9)
        assert len(before) > 10 and np.array_equal(before, after)
        assert before["start"].min() >= tile and before["start"].max() < 3 * tile
        assert np.array_equal(buf.cpu().numpy(), sink_before)
    finally:
        ctx.set_row_sink(None, 0)
        g.select([])
        g.free()


def test_cli_writes_the_profile_of_a_fasta_interval(ctx, tmp_path, monkeypatch, capsys):
    import plot_periodicity_matrix as cli
    _use_ctx(monkeypatch, ctx)
    chrom = (_random(20_000, 14) + b"ACGGT" * 600 + b"N" * 700 + _random(9_000, 15)).decode()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\nACGT\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    tsv, png = tmp_path / "profile.tsv", tmp_path / "profile.png"
    cli.main([str(fa), "-i", "chrT:1500-40000", "--min-motif-size", "2", "--max-motif-size", "12", "--window", "1024",
              "--tsv", str(tsv), "-o", str(png)])
    counts = P.period_counts(chrom, 2, 12, 1024, 1500, 40_000)
    want = list(cli.profile_lines("chrT", 1500, len(chrom), 1024, 2, counts))
    assert tsv.read_text() == "".join(want) and len(want) > 300
    assert png.read_bytes()[:4] == b"\x89PNG"
    png2 = tmp_path / "matrix.png"
    cli.main(["ACGT" * 5 + "TTTTTTTTNNNN", "--max-motif-size", "8", "-o", str(png2)])
    assert png2.read_bytes()[:4] == b"\x89PNG"


def test_repeat_finder_plot_flag_writes_a_png_and_the_same_tsv(ctx, tmp_path, monkeypatch, capsys):
    import perfect_repeat_finder as prf
    _use_ctx(monkeypatch, ctx)
    seq = (_random(100, 16) + b"CAG" * 30 + _random(80, 17) + b"AT" * 15).decode()
    assert len(seq) == 300
    prf.main([seq, "-o", str(tmp_path / "plain")])
    prf.main([seq, "-o", str(tmp_path / "plotted"), "-p", str(tmp_path / "out.png")])
    assert (tmp_path / "out.png").read_bytes()[:4] == b"\x89PNG"
    rows = (tmp_path / "plain.tsv").read_text()
    assert rows == (tmp_path / "plotted.tsv").read_text() and rows.count("\n") > 2
    capsys.readouterr()
    prf.main(["ACGT" * 1300, "-o", str(tmp_path / "long"), "-p", str(tmp_path / "long.png")])
    assert "too long (5,200 bp). Skipping plot" in capsys.readouterr().out and not (tmp_path / "long.png").exists()
