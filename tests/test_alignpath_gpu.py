"""GPU (-m gpu): the alignment of tandem repeats to their motifs with its path (prf_motif_align_path, csrc/alignpath.hip).
Every result -- the rows, the path, the counts -- is compared EXACTLY with the model (tests/alignpath_model.py, pinned to a
full-matrix traceback by tests/test_alignpath_cpu.py), and the rows with prf_motif_align on the same call.

Shapes: the genome of tests/test_align_gpu.py; rows at every k around the boundaries between the five forward kernels and of 1, 2,
3, 4, 5, 8, 9, 16, 17 positions (every number of positions per trace word: 16, 8, 4, 2, 1), k - 1, k, k + 1, 64, 65 and 300; every
k = 1 .. 1 024 at 24 positions; planted repeats with a substitution, an insertion, a deletion and a run of deletions across the
wrap in every kernel; batches of the trace; rows of 2^19 positions, the limit, by their closed form."""
import itertools
import random

import numpy as np
import pytest

import align_model as A
import alignpath_model as P
import phased_cases as K
from test_align_gpu import KS, REGIME_KS, STARTS, _motif_near, _planted_genome
from test_consensus_gpu import _first_contig
from test_dotruns_gpu import _random

pytestmark = pytest.mark.gpu


def _lengths(k):
    return sorted({1, 2, 3, 4, 5, 8, 9, 16, 17, max(1, k - 1), k, k + 1, 64, 65, 300})


@pytest.fixture(scope="module")
def ctx():
    import torch  # the same load order as the other GPU tests (torch's HIP runtime first)
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def two_contigs(ctx):
    seqs = [_first_contig(), _random(20_003, 184)]
    g = ctx.load(seqs, 64)
    yield g, seqs
    g.free()


def _same(got, want, what=None):
    """got: what motif_align_path returned with_counts; want: the model's (rows, concatenated path, counts)."""
    rows, paths, counts = got[:3]
    assert rows.dtype == np.dtype(A.DTYPE) and len(rows) == len(want[0]), what
    if not A.same(rows, want[0]):
        bad = [at for at in range(len(rows)) if rows[at] != want[0][at]]
        raise AssertionError((what, "rows", len(bad), bad[:5], rows[bad[:5]], want[0][bad[:5]]))
    path = np.concatenate(paths) if paths else np.zeros(0, dtype=np.uint16)
    assert path.dtype == np.uint16 and len(path) == len(want[1]), what
    if not np.array_equal(path, want[1]):
        bad = np.flatnonzero(path != want[1])
        raise AssertionError((what, "path", len(bad), bad[:5], path[bad[:5]], want[1][bad[:5]]))
    assert counts.dtype == np.uint32 and counts.shape == want[2].shape, what
    if not np.array_equal(counts, want[2]):
        bad = np.flatnonzero((counts != want[2]).any(axis=1))
        raise AssertionError((what, "counts", len(bad), bad[:5], counts[bad[:5]], want[2][bad[:5]]))


def _compare(g, seq, contig, begin, end, table, motifs, what=None, **more):
    want = P.align_path(seq, table, motifs, begin, end)
    got = g.motif_align_path(contig, begin, end, table, motifs, with_counts=True, **more)
    _same(got, want, what)
    assert g.motif_align(contig, begin, end, table, motifs).tobytes() == got[0].tobytes(), what     # bit for bit
    return got, want


@pytest.mark.parametrize("begin", [29, 192])
def test_periods_lengths_and_word_alignments_against_the_model(two_contigs, begin):
    """Every k x every length x every start % 64, in one call per range; begin % 64 is 29 (every word is funnel-shifted) or 0."""
    g, seqs = two_contigs
    rng = random.Random(301)
    rows, motifs = [], []
    for at, (k, start) in enumerate(itertools.product(KS, STARTS)):
        for n in _lengths(k):
            a = start + 64 * (at % 5) + (4_992 if at % 2 else 0)                # random letters, and the N block and lower case
            rows.append((a, a + n, k))
            motifs.append(_motif_near(seqs[0], begin + a + (at % 3), k, rng))
    assert len(rows) > 700 and {a % 64 for a, _, _ in rows} == set(STARTS)
    table = A.repeats(*rows)
    want = P.align_path(seqs[0], table, motifs, begin, 9_000)
    got = g.motif_align_path(0, begin, 9_000, table, motifs, with_counts=True, with_stats=True)
    _same(got, want, begin)
    st = got[3]
    assert st.path == 15 and st.n_hits == len(rows) and st.positions == sum(b - a for a, b, _ in rows) == len(want[1])
    assert st.n_candidates == sum((b - a) * k for a, b, k in rows) and st.n_launches == 5 + 1 + 1       # one batch
    assert st.phase1_ms > 0 and st.phase2_ms > 0 and abs(st.scan_ms - (st.phase1_ms + st.phase2_ms)) < 1e-3
    assert g.motif_align(0, begin, 9_000, table, motifs).tobytes() == got[0].tobytes()
    flags = want[1]
    assert int((flags & P.INS != 0).sum()) > 50 and int((flags & P.SUB != 0).sum()) > 500 and int(want[2][:, 4].sum()) > 50   # the inputs
    _same(g.motif_align_path(0, begin, 9_000, table, "".join(motifs), with_counts=True), want, "the letters in one buffer")


def test_every_k_in_one_call(two_contigs):
    g, seqs = two_contigs
    rng = random.Random(302)
    rows = [(100 + 7 * k, 124 + 7 * k, k) for k in range(1, 1_025)]
    motifs = [_motif_near(seqs[1], 100 + 7 * k - (k % 5), k, rng) for k in range(1, 1_025)]
    _compare(g, seqs[1], 1, 0, None, A.repeats(*rows), motifs)


def _wrap_rows():
    """Per kernel: copies of a motif from phase 0 with the last letter of the second copy and the first of the third taken out: a
    run of deletions across the wrap, columns k - 1 and 0.  (sequence, rows, motifs)"""
    rng = random.Random(303)
    seq, rows, motifs = bytearray(_random(23, 304)), [], []
    for k in REGIME_KS:
        motif = ""
        # the letters around the cut differ, so that the run cannot slide to other columns at the same cost
        while not motif or not K.primitive(motif) or len({motif[-2], motif[-1], motif[0]}) < 3 or len({motif[-1], motif[0], motif[1]}) < 3:
            motif = "".join(rng.choice("ACGT") for _ in range(k))
        body = list(motif * (9 if k == 5 else 4))
        del body[2 * k - 1:2 * k + 1]
        rows.append((len(seq), len(seq) + len(body), k))
        motifs.append(motif)
        seq += "".join(body).encode() + _random(rng.randrange(1, 70), rng.randrange(1 << 30))
    return bytes(seq), rows, motifs


def test_planted_repeats_in_every_kernel(ctx):
    seq, rows, motifs, expect = _planted_genome()
    wseq, wrows, wmotifs = _wrap_rows()
    rows = rows + [(a + len(seq), b + len(seq), k) for a, b, k in wrows]
    motifs, seq = motifs + wmotifs, seq + wseq
    table = A.repeats(*rows)
    g = ctx.load([seq], 64)
    try:
        got, want = _compare(g, seq, 0, 0, None, table, motifs)
    finally:
        g.free()
    assert [tuple(r)[:5] for r in want[0].tolist()][:len(expect)] == expect        # the model finds what was planted
    offsets = np.concatenate([[0], np.cumsum(table["k"])]).astype(np.int64)
    for at, (row, path) in enumerate(zip(got[0], got[1])):
        k, n = int(table["k"][at]), len(path)
        ins, sub = int((path & P.INS != 0).sum()), int((path & P.SUB != 0).sum())
        dels = int(got[2][offsets[at]:offsets[at + 1], 4].sum())
        assert ins + dels == row["indels"] and sub + ins + dels == row["edits"] and n - ins + dels == row["consumed"]
        assert not path[0] & P.INS and path[0] & P.COLUMN == row["start_column"]
        if at < len(expect) and not expect[at][0]:                              # perfect from a phase: the closed form
            assert np.array_equal(path, P.perfect(motifs[at], expect[at][3], n))
    for at in range(len(expect), len(rows)):                                    # the runs across the wrap
        k = int(table["k"][at])
        assert got[0][at].tolist()[:5] == (2, 2, len(got[1][at]) + 2, 0, k - 1)
        assert np.flatnonzero(got[2][offsets[at]:offsets[at + 1], 4]).tolist() == [0, k - 1]
        assert P.deletions_behind(got[1][at], k).tolist() == [2 if i == 2 * k - 2 else 0 for i in range(len(got[1][at]) - 1)]


def test_n_blocks_lower_case_and_a_motif_with_n(two_contigs):
    g, seqs = two_contigs
    s = seqs[0]
    rows = [(400, 700, 5), (480, 660, 70), (500, 650, 3), (1_000, 1_400, 7), (990, 1_410, 300), (2_000, 2_064, 2), (2_000, 2_164, 2), (4_000, 4_100, 1),
            (3_990, 4_010, 4), (6_000, 6_000 + 171 * 30, 171), (6_010, 6_000 + 171 * 12, 171)]
    unit = s[6_000 + 171 * 3:6_000 + 171 * 4].decode()
    motifs = ["ACGTA", s[700:770].decode(), "NNN", s[1_000:1_007].decode(), s[1_000:1_300].decode().upper(), "AC", "ca", "N", "ANGT", unit,
              unit[:50] + "n" * 5 + unit[55:]]
    motifs = ["".join(c if c in "ACGTNacgtn" else "N" for c in m) for m in motifs]
    got, _ = _compare(g, s, 0, 0, None, A.repeats(*rows), motifs)
    assert got[0][2].tolist()[:5] == (150, 0, 150, 1, 0) and (got[1][7] == P.SUB).all()       # N matches nothing: all SUB, no indel
    assert np.array_equal(got[1][2], P.perfect("NNN", 1, 150) | P.SUB)
    assert np.array_equal(got[1][5], P.perfect("AC", 0, 64))


def test_stretches_of_r_and_y_and_the_one_shot_form(ctx):
    """A genome of eight planes: R and Y (and every letter outside ACGT) match nothing and count nowhere; and the one-shot form."""
    rng = random.Random(305)
    s = bytearray(_random(12_000, 186))
    for at in (300, 5_000, 9_000):
        s[at:at + 90] = bytes(rng.choice(b"RYN") for _ in range(90))
    s[7_000:7_400] = (b"RYRRY" * 80)
    s = bytes(s)
    ks = [1, 5, 64, 65, 400, 1_000]
    rows = [(a, b, k) for k in ks for a, b in ((250, 450), (6_990, 7_300), (7_100, 7_101), (8_950, 9_200))]
    motifs = [_motif_near(s, a + 100, k, rng) for a, _, k in rows]
    table = A.repeats(*rows)
    g = ctx.load([s], 64)
    try:
        _, want = _compare(g, s, 0, 0, None, table, motifs)
        inner = A.repeats((0, 200, 5), (10, 411, 64), (5, 6, 1))                  # position 7 000: an R
        _compare(g, s, 0, 6_995, 7_406, inner, ["ACAAC", motifs[8], "A"])
    finally:
        g.free()
    _same(ctx.motif_align_path(s, table, motifs, with_counts=True), want, "one shot")
    _same(ctx.motif_align_path(s.decode(), inner, ["ACAAC", motifs[8], "A"], begin=6_995, end=7_406, with_counts=True),
          P.align_path(s, inner, ["ACAAC", motifs[8], "A"], 6_995, 7_406), "one shot, a range")
    rows_, paths = ctx.motif_align_path("acgACGtACGACG", A.repeats((0, 13, 3)), ["ACG"])
    assert rows_[0].tolist()[:5] == (1, 1, 12, 0, 2) and int((paths[0] & P.INS != 0).sum()) == 1


def _trace_bytes(rows):
    regime = lambda k: 0 if k <= 64 else 1 if k <= 128 else 2 if k <= 256 else 3 if k <= 512 else 4
    return sum(-(-(b - a) // (16 >> regime(k))) * 256 for a, b, k in rows)


def test_five_thousand_rows_in_batches_follow_their_rows(two_contigs):
    g, seqs = two_contigs
    rng = random.Random(306)
    n = len(seqs[1])
    rows, motifs = [], []
    for _ in range(5_000):
        k = rng.choice((1, 2, 3, 4, 6, 17, 33, 64)) if rng.random() < 0.9 else rng.choice((65, 128, 171, 257, 700, 1_024))
        start = rng.randrange(n - 200)
        rows.append((start, start + rng.choice((1, 2, 10, 24, 64, 65, 130)), k))
        motifs.append(_motif_near(seqs[1], start + rng.randrange(3), k, rng))
    table = A.repeats(*rows)
    want = P.align_path(seqs[1], table, motifs)
    whole = g.motif_align_path(1, 0, None, table, motifs, with_counts=True, with_stats=True)
    _same(whole, want, "one batch")
    assert whole[3].n_launches == 5 + 1 + 1
    budget = _trace_bytes(rows) // 4
    dealt = g.motif_align_path(1, 0, None, table, motifs, with_counts=True, with_stats=True, trace_bytes=budget)
    _same(dealt, want, "batches")
    assert dealt[3].n_launches >= 5 + 4 + 1                                      # four walks or more: four batches or more
    _same(g.motif_align_path(1, 0, None, table, motifs, with_counts=True, trace_bytes=256), want, "every row a batch of its own")
    back = g.motif_align_path(1, 0, None, table[::-1].copy(), motifs[::-1], with_counts=True, trace_bytes=budget)   # the results follow the rows
    assert back[0][::-1].tobytes() == whole[0].tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(back[1][::-1], whole[1]))
    plain = g.motif_align_path(1, 0, None, table, motifs)                       # without the counts: the same rows and paths
    assert len(plain) == 2 and plain[0].tobytes() == whole[0].tobytes() and all(np.array_equal(a, b) for a, b in zip(plain[1], whole[1]))


def test_a_row_larger_than_the_trace(two_contigs):
    g, seqs = two_contigs
    rng = random.Random(307)
    rows = [(50, 350, 1_000), (10, 20, 3), (400, 1_400, 5), (30, 31, 600)]
    motifs = [_motif_near(seqs[1], a + 1, k, rng) for a, _, k in rows]
    assert _trace_bytes(rows[:1]) == 300 * 256
    for budget in (1, 4_096, 300 * 256, 300 * 256 + 256):
        _compare(g, seqs[1], 1, 0, None, A.repeats(*rows), motifs, budget, trace_bytes=budget)


@pytest.mark.parametrize("k", [1_024, 1])
def test_a_row_at_the_limit_of_positions(ctx, k):
    """2^19 positions of the perfect repetition of a random primitive motif from a phase: the closed form (the model would take
    minutes): path[i] = (phase + i) mod k without flags, the counts are the sizes of the columns."""
    import prf_native as pn
    n, rng = A.MAX_LEN, random.Random(308)
    motif = ""
    while not motif or not K.primitive(motif):
        motif = "".join(rng.choice("ACGT") for _ in range(k))
    phase = 389 % k
    copies = motif * (n // k + 2)
    head = "GATTACA" * 3
    seq = head + copies[phase:phase + n] + "TTGCA"
    g = ctx.load([seq.encode()], 64)
    try:
        table = A.repeats((len(head), len(head) + n, k), (len(head) + 5, len(head) + 5 + 3 * k + 1, k))
        rows, paths, counts = g.motif_align_path(0, 0, None, table, [motif, motif], with_counts=True)
        assert rows.tobytes() == g.motif_align(0, 0, None, table, [motif, motif]).tobytes()
    finally:
        g.free()
    assert rows[0].tolist() == (0, 0, n, phase, (phase + n - 1) % k, 0)
    assert np.array_equal(paths[0], P.perfect(motif, phase, n)) and np.array_equal(paths[1], P.perfect(motif, (phase + 5) % k, 3 * k + 1))
    sizes = np.bincount((phase + np.arange(n)) % k, minlength=k)
    want = np.zeros((k, 6), dtype=np.uint32)
    want[np.arange(k), ["ACGT".index(c) for c in motif]] = sizes
    assert np.array_equal(counts[:k], want)
    assert pn.path_cigar(paths[0], k) == f"{n}=" and pn.aligned_consensus(counts[:k], motif) == motif


def test_refusals_on_a_resident_genome(ctx, two_contigs):
    import prf_native as pn
    g, _ = two_contigs
    out = np.zeros(1, dtype=pn.ALIGNMENT_DTYPE)
    path = np.full(200, 0xABCD, dtype=np.uint16)
    counts = np.full((8, 6), 7, dtype=np.uint32)

    def call(row, motif, contig=0, capacity=200, with_path=True):
        table = A.repeats(row)
        return ctx.lib.prf_motif_align_path_ex(ctx._h, g._h, contig, 0, 1 << 63, table.ctypes.data, 1, motif, len(motif), out.ctypes.data,
                                               path.ctypes.data if with_path else None, capacity, counts.ctypes.data, None, 0)

    assert call((0, 100, 1_025), b"A" * 1_025) == pn.PRF_EUNSUPPORTED and "PRF_ALIGN_MAX_K" in ctx.lib.prf_last_error().decode()
    assert call((0, 100, 3), b"ACG", capacity=99) == pn.PRF_EINVAL and "the path holds 99 entries" in ctx.lib.prf_last_error().decode()
    assert call((0, 100, 3), b"ACG", with_path=False) == pn.PRF_EINVAL and "NULL path" in ctx.lib.prf_last_error().decode()
    assert call((0, 30_012, 3), b"ACG", capacity=1 << 20) == pn.PRF_EINVAL and "row 0: end 30012" in ctx.lib.prf_last_error().decode()
    assert call((0, 30, 3), b"ACG", contig=2) == pn.PRF_EINVAL
    assert (path == 0xABCD).all() and (counts == 7).all() and not out["consumed"][0]         # a refused call writes nothing
    assert call((0, 30, 3), b"ACG") == pn.PRF_OK and out["consumed"][0] > 0
    assert (path[:30] != 0xABCD).all() and (path[30:] == 0xABCD).all() and (counts[3:] == 7).all() and counts[:3, :4].sum() > 0
    assert ctx.lib.prf_motif_align_path(ctx._h, g._h, 0, 0, 1 << 63, None, 0, None, 0, None, None, 0, None, None) == pn.PRF_OK
    with pytest.raises(ValueError, match="more than an alignment takes"):
        g.motif_align_path(0, 0, None, A.repeats((0, 100, 1_025)), ["A" * 1_025])
    with pytest.raises(pn.PrfError, match="row 1: column 2 of the motif"):
        g.motif_align_path(0, 0, None, A.repeats((0, 100, 3), (0, 100, 4)), ["ACG", "ACRT"])
    with pytest.raises(pn.PrfError, match="unsupported symbol at position 4"):
        ctx.motif_align_path("ACGT-ACGT", A.repeats((0, 9, 3)), ["ACG"])


def _planted_bodies():
    """The 30 planted inputs of tests/phased_cases.py in one sequence: (sequence, the bodies as repeats, the planted motifs)."""
    seq, rows, motifs = "", [], []
    for key in list(K.SEEDS) + [7, 17, 40]:
        motif, text = K.planted(*key) if isinstance(key, tuple) else K.close_pair(key)
        rows.append((len(seq) + K.FLANK, len(seq) + len(text) - K.FLANK, len(motif)))
        motifs.append(motif)
        seq += text
    return seq, A.repeats(*rows), motifs


def test_refine_motifs_restores_the_planted_motifs(ctx):
    import prf_native as pn
    seq, table, motifs = _planted_bodies()
    wrong = [m[:len(m) // 3] + next(c for c in "ACGT" if c != m[len(m) // 3]) + m[len(m) // 3 + 1:] for m in motifs]
    g = ctx.load([seq.encode()], 64)
    try:
        rows, paths, counts = g.motif_align_path(0, 0, None, table, motifs, with_counts=True)
        assert pn.aligned_consensus(counts, motifs) == motifs                  # the aligned majority is the planted motif, 30 of 30
        refined, align, changed = pn.refine_motifs(g, 0, 0, None, table, wrong, rounds=1)
        assert refined == motifs and changed.tolist() == [1] * 30              # one round restores it
        assert align.tobytes() == rows.tobytes()                               # ... and the alignment is that of the returned motifs
        again, align2, changed2 = pn.refine_motifs(g, 0, 0, None, table, wrong, rounds=5)
        assert again == motifs and changed2.tolist() == [1] * 30 and align2.tobytes() == rows.tobytes()     # stops when nothing changes
        same, _, unchanged = pn.refine_motifs(g, 0, 0, None, table, "".join(motifs), rounds=3)
        assert same == motifs and not unchanged.any()
    finally:
        g.free()
    shot, _, once = pn.refine_motifs(ctx, seq, 0, None, table, wrong, rounds=2)
    assert shot == motifs and once.tolist() == [1] * 30
    want = P.align_path(seq, table, motifs)
    _same((rows, paths, counts), want)
    for at, key in enumerate(list(K.SEEDS)):                                    # the number of INS entries, not their places
        d, kind = key[1], key[2]
        assert int((paths[at] & P.INS != 0).sum()) == (d if kind != "del" else 0), key


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
        rows = A.repeats((1_000, 1_060, 3), (0, 3_000, 50), (990, 1_070, 3), (3 * tile, 3 * tile + 400, 700))   # whatever is selected
        motifs = ["CAG", seq[:50].decode(), "AGC", "ACGT" * 175]
        aligned_before = g.motif_align(0, 0, None, rows, motifs)
        got, _ = _compare(g, seq, 0, 0, None, rows, motifs)
        assert got[0][0].tolist()[:5] == (0, 0, 60, 0, 2) and np.array_equal(got[1][0], P.perfect("CAG", 0, 60))
        assert ctx.motif_align_path(seq[:2_000], rows[:1], motifs[:1])[0][0].tolist()[:3] == (0, 0, 60)   # the one-shot form, a genome of its own
        assert np.array_equal(buf.cpu().numpy(), sink_before)                 # nothing was written to the sink
        assert g.motif_align(0, 0, None, rows, motifs).tobytes() == aligned_before.tobytes()
        after, _ = g.scan(1, 50, 3, 9)
        assert len(before) > 10 and np.array_equal(before, after)
        assert before["start"].min() >= tile and before["start"].max() < 3 * tile
        assert np.array_equal(buf.cpu().numpy(), sink_before)
    finally:
        ctx.set_row_sink(None, 0)
        g.select([])
        g.free()


def test_cli_writes_the_paths_of_an_interval(ctx, tmp_path):
    """--align-path, --refine and --copies-tsv over a FASTA interval: the new columns against the model and the host helpers;
    without the new flags the file is what --align alone writes."""
    import prf_native as pn
    import plot_periodicity_matrix as cli
    motif, body = K.planted(17, 2, "both")
    chrom = (_random(3_000, 14).decode() + body + "N" * 200 + K.planted(17, 1, "ins")[1] + _random(2_000, 15).decode()).lower()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\nACGT\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    base = [str(fa), "-i", f"chrT:100-{len(chrom) - 50}", "--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--chain-window", "1000"]
    for flag, more, name_at in (("--groups-tsv", ["--max-shift", "4", "--min-group", "60", "--group-consensus"], 10), ("--chains-tsv", ["--consensus"], 9)):
        plain, paths, refined, copies = (tmp_path / f"{flag[2:]}.{name}.tsv" for name in ("plain", "paths", "refined", "copies"))
        cli.main(base + [flag, str(plain)] + more + ["--align"], context=ctx)
        cli.main(base + [flag, str(paths)] + more + ["--align", "--align-path", "--copies-tsv", str(copies)], context=ctx)
        old, new = plain.read_text().splitlines(), paths.read_text().splitlines()
        assert len(old) == len(new) >= 2
        listed = [line.split("\t") for line in copies.read_text().splitlines()]
        gapped = 0
        for before, line in zip(old, new):
            f = before.split("\t")
            start, end, k = int(f[1]), int(f[2]), int(f[3])
            path = P.path_one(chrom[start:end], f[name_at])[1]
            assert line == before + "\t" + pn.path_cigar(path, k), before
            mine = [c[4:] for c in listed if c[:4] == f[:4]]
            assert mine == [[str(v) for v in (c, start + a, start + b, s, i, d)] for c, a, b, s, i, d in pn.path_copies(path, 0, k).tolist()]
            gapped += "I" in line.split("\t")[-1] or "D" in line.split("\t")[-1]
        assert gapped >= (2 if flag == "--groups-tsv" else 0)
        cli.main(base + [flag, str(refined)] + more + ["--align", "--refine", "2"], context=ctx)
        for before, line in zip(old, refined.read_text().splitlines()):
            f, r = before.split("\t"), line.split("\t")
            start, end, k = int(f[1]), int(f[2]), int(f[3])
            name, rounds = f[name_at], 0                                        # the model's loop: align, aligned majority, twice at most
            for _ in range(2):
                better = pn.aligned_consensus(P.path_one(chrom[start:end], name)[2], name)
                if better == name:
                    break
                name, rounds = better, rounds + 1
            al = A.align_one(chrom[start:end], name)
            subs, ins, dele, _, identity, n_copies = A.derived(end - start, k, *al[:3])
            assert r[name_at] == name and r[name_at + 3] == pn.canonical_motif(name) and r[-1] == str(rounds)
            assert r[-7:-1] == [str(al[0]), str(subs), str(ins), str(dele), f"{identity:.4f}", f"{n_copies:.2f}"]
            assert r[:name_at] == f[:name_at] and r[name_at + 1:name_at + 3] == f[name_at + 1:name_at + 3]
