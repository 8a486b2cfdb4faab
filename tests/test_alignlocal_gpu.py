"""GPU (-m gpu): the local alignment of windows to motifs (prf_motif_align_local, csrc/alignlocal.hip).  Every result is
compared EXACTLY, every field, with the model (tests/alignlocal_model.py, pinned to the brute force by tests/test_alignlocal_cpu.py).

Shapes: the genome of tests/test_consensus_gpu.py (two contigs of 30 011 and 20 003 positions of ACGT, N blocks and lower case);
windows of 1 to 1 025 positions at every k around the boundaries between the five kernels (64 | 65, 128 | 129, 256 | 257, 512 | 513,
1 024) and every k = 1 .. 1 024 at 24 positions; planted repeats between random flanks in every kernel; two-letter windows, where
the tie rules decide; the eight weight triples of the model; one row of 2^19 positions with match = 16, the score field's maximum."""
import itertools
import random

import numpy as np
import pytest

import align_model as A
import alignlocal_model as L
import phased_cases as K
from test_consensus_gpu import _first_contig
from test_dotruns_gpu import _random

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1_023, 1_024]
STARTS = [0, 1, 63]                                           # start % 64
REGIME_KS = [5, 100, 200, 400, 900]                           # one k per kernel
TRF = (2, 7, 7)


def _lengths(k):
    return sorted({1, 2, max(1, k - 1), k, k + 1, 64, 65, 300})


@pytest.fixture(scope="module")
def ctx():
    import torch  # the same load order as the other GPU tests (torch's HIP runtime first)
    assert torch.cuda.is_available()
    import prf_native
    assert np.dtype(prf_native.LOCAL_ALIGNMENT_DTYPE).itemsize == 24
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
    assert got.dtype == np.dtype(L.DTYPE) and len(got) == len(want), what
    if not L.same(got, want):
        bad = [at for at in range(len(want)) if got[at] != want[at]]
        raise AssertionError((what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]]))


def _motif_near(seq, at, k, rng):
    """k letters of the sequence from `at` on (upper case, N kept), every ninth changed: the windows align with many ties."""
    text = bytearray(seq[at:at + k].upper())
    text += bytes(rng.choice(b"ACGT") for _ in range(k - len(text)))
    for j in range(0, k, 9):
        text[j] = rng.choice(b"ACGT")
    return bytes(b if b in b"ACGTN" else ord("N") for b in text).decode()


@pytest.mark.parametrize("begin", [29, 192])
def test_periods_lengths_and_word_alignments_against_the_model(two_contigs, begin):
    """Every k x every length x every start % 64, in one call per range; begin % 64 is 29 (every word is funnel-shifted) or 0."""
    g, seqs = two_contigs
    rng = random.Random(231)
    rows, motifs = [], []
    for at, (k, start) in enumerate(itertools.product(KS, STARTS)):
        for n in _lengths(k):
            a = start + 64 * (at % 5) + (4_992 if at % 2 else 0)                # random letters, and the N block and lower case
            rows.append((a, a + n, k))
            motifs.append(_motif_near(seqs[0], begin + a + (at % 3), k, rng))
    assert len(rows) > 350 and {a % 64 for a, _, _ in rows} == set(STARTS)
    table = A.repeats(*rows)
    want = L.local(seqs[0], table, motifs, TRF, begin, 9_000)
    got, st = g.motif_align_local(0, begin, 9_000, table, motifs, with_stats=True)
    _check(got, want, begin)
    assert st.path == 16 and st.n_hits == len(rows) and st.positions == sum(b - a for a, b, _ in rows)
    assert st.n_candidates == sum((b - a) * k for a, b, k in rows) and st.n_launches == 5 and st.scan_ms > 0 and st.scan_ms == st.phase1_ms
    lengths = np.array([b - a for a, b, _ in rows])
    assert int((want["end"] - want["first"] < lengths).sum()) > 50 and int((want["score"] == 2 * lengths).sum()) > 10    # trimmed windows, perfect ones
    _check(g.motif_align_local(0, begin, 9_000, table, "".join(motifs)), want, "the letters in one buffer")


def test_every_k_in_one_call(two_contigs):
    g, seqs = two_contigs
    rng = random.Random(232)
    rows = [(100 + 7 * k, 124 + 7 * k, k) for k in range(1, 1_025)]
    motifs = [_motif_near(seqs[1], 100 + 7 * k - (k % 5), k, rng) for k in range(1, 1_025)]
    table = A.repeats(*rows)
    _check(g.motif_align_local(1, 0, None, table, motifs, 2, 3, 5), L.local(seqs[1], table, motifs, (2, 3, 5)))


BODIES = ((0, ""), (1, ""), (-1, ""), (2, "S"), (0, "I"), (3, "D"), (1, "W"), (2, "E"))


def W_RUN(k):
    return 5 if k > 5 else 3


def _planted_genome():
    """For every kernel's k: a motif, and windows flank + body + flank with random flanks whose body is copies of the motif --
    perfect from three phases, with one substitution, one insertion, one deletion, a run of deletions across the wrap (W: the last
    letters of a copy in the middle of the body and the first two of the next, five in all, three at k = 5), an edit two positions
    from the body's end, which is trimmed (E).  Returns
    (sequence, windows, motifs, where each body lies in its window)."""
    rng = random.Random(233)
    seq, rows, motifs, bodies = bytearray(_random(37, 234)), [], [], []
    for k in REGIME_KS:
        motif = ""
        while not motif or not K.primitive(motif):
            motif = "".join(rng.choice("ACGT") for _ in range(k))
        copies = 11 if k == 5 else 3
        for phase, edit in BODIES:
            phase %= k
            body = [motif[(phase + t) % k] for t in range(copies * k + 2)]
            place = rng.randrange(k // 2 + 2, len(body) - k // 2 - 2)
            if edit == "S":
                body[place] = next(c for c in "ACGT" if c != body[place])
            elif edit == "I":
                body.insert(place, next(c for c in "acgt" if c.upper() not in (body[place - 1], body[place])))
            elif edit == "D":
                del body[place]
            elif edit == "W":
                wrap = next(t for t in range(len(body) // 2, len(body)) if (phase + t) % k == 0)     # the first letter of a copy
                del body[wrap - (W_RUN(k) - 2):wrap + 2]
            elif edit == "E":
                body[-3] = next(c for c in "ACGT" if c != body[-3])
            left, right = rng.randrange(1, 60), rng.randrange(1, 60)
            start = len(seq)
            seq += _random(left, rng.randrange(1 << 30)) + "".join(body).encode() + _random(right, rng.randrange(1 << 30))
            rows.append((start, len(seq), k))
            motifs.append(motif)
            bodies.append((left, left + len(body), edit))
        seq += _random(rng.randrange(1, 90), rng.randrange(1 << 30))
    return bytes(seq), rows, motifs, bodies


def test_planted_repeats_in_every_kernel_and_their_composition(ctx):
    seq, rows, motifs, bodies = _planted_genome()
    table = A.repeats(*rows)
    want = L.local(seq, table, motifs, TRF)
    for row, (left, right, edit) in zip(want.tolist(), bodies):                  # the model finds what was planted, give or take a chance match
        assert row[1] <= left + 3 and (row[2] >= right - 3 if edit == "E" else row[2] >= right), (row, left, right, edit)
        assert row[2] <= right - 3 or edit != "E" or row[2] >= right
    assert any(row[2] == right - 3 for row, (_, right, edit) in zip(want.tolist(), bodies) if edit == "E")     # a trimmed edit
    g = ctx.load([seq], 64)
    try:
        got = g.motif_align_local(0, 0, None, table, motifs)
        _check(got, want)
        # the composition: motif_align on the refined intervals, with the same motifs
        refined = A.repeats(*((a + int(r["first"]), a + int(r["end"]), k) for (a, _, k), r in zip(rows, got)))
        aligned = g.motif_align(0, 0, None, refined, motifs)
        assert A.same(aligned, A.align(seq, refined, motifs))
        # the planted indels are in it (three deleted letters of five are two inserted ones); a chance match in a flank, reached
        # across an indel, may add one
        planted = [{"": 0, "S": 0, "I": 1, "D": 1, "E": 0, "W": min(W_RUN(k), k - W_RUN(k))}[edit] for (_, _, k), (_, _, edit) in zip(rows, bodies)]
        assert (aligned["indels"] >= planted).all() and int((aligned["indels"] == planted).sum()) > len(rows) * 3 // 4
        # the motif rotated: the same scores and ends
        turned = [m[3 % len(m):] + m[:3 % len(m)] for m in motifs]
        again = g.motif_align_local(0, 0, None, table, turned)
        assert np.array_equal(again["score"], got["score"]) and np.array_equal(again["end"], got["end"])
    finally:
        g.free()


def test_closed_forms_between_flanks_of_t(ctx):
    """A primitive motif over A, C, G between flanks of T, which match nothing: a perfect repeat of L positions at phase f behind
    a flank gives (match L, flank, flank + L, f, (f + L - 1) mod k); one substitution at offset d from the left edge is kept iff
    match d > mismatch."""
    rng = random.Random(235)
    seq, rows, motifs, expect = bytearray(b"T" * 70), [], [], []
    for k in (1, 3, 7, 64, 65, 130, 300, 600, 1_024):
        motif = ""
        while not motif or not K.primitive(motif):
            motif = "".join(rng.choice("ACG") for _ in range(k))
        for phase, length, flank in ((0, k, 0), (k - 1, k + 1, 1), (rng.randrange(k), 2 * k + 5, 63), (1 % k, 3 * k, 64)):
            start = len(seq) - flank
            seq += "".join(motif[(phase + t) % k] for t in range(length)).encode() + b"T" * 70
            rows.append((start, len(seq) - 3, k))
            motifs.append(motif)
            expect.append((2 * length, flank, flank + length, phase, (phase + length - 1) % k, 0))
    motif = "ACGGCAG"
    for d in range(1, 9):
        body = bytearray((motif * 9).encode()[:60])
        body[d] = ord("T")
        start = len(seq) - 5
        seq += bytes(body) + b"T" * 70
        rows.append((start, len(seq) - 60, 7))
        motifs.append(motif)
        expect.append((2 * 59 - 7, 5, 65, 0, 59 % 7, 0) if 2 * d > 7 else (2 * (59 - d), 5 + d + 1, 65, (d + 1) % 7, 59 % 7, 0))
    table = A.repeats(*rows)
    want = L.local(bytes(seq), table, motifs, TRF)
    assert [tuple(r) for r in want.tolist()] == expect
    _check(ctx.motif_align_local(bytes(seq), table, motifs), want)


def test_two_letter_windows_where_the_ties_are(ctx):
    rng = random.Random(236)
    seq = bytes(rng.choice(b"AC") for _ in range(5_000))
    rows, motifs = [], []
    for _ in range(2_000):
        k = rng.randint(1, 4)
        start = rng.randrange(len(seq) - 40)
        rows.append((start, start + rng.randint(1, 30), k))
        motifs.append("".join(rng.choice("AC") for _ in range(k)))
    table = A.repeats(*rows)
    g = ctx.load([seq], 64)
    try:
        for weights in ((1, 1, 1), (2, 5, 1)):
            _check(g.motif_align_local(0, 0, None, table, motifs, *weights), L.local(seq, table, motifs, weights), weights)
    finally:
        g.free()


def _mixed_rows(seq, rng, count):
    rows, motifs = [], []
    for _ in range(count):
        k = rng.choice((1, 2, 3, 4, 6, 17, 33, 64)) if rng.random() < 0.8 else rng.choice((65, 128, 171, 257, 700, 1_024))
        start = rng.randrange(len(seq) - 200)
        rows.append((start, start + rng.choice((1, 2, 10, 24, 64, 65, 130)), k))
        motifs.append(_motif_near(seq, start + rng.randrange(3), k, rng))
    return rows, motifs


@pytest.mark.parametrize("weights", L.WEIGHTS, ids=[",".join(str(w) for w in t) for t in L.WEIGHTS])
def test_each_weight_triple_on_one_mixed_call(two_contigs, weights):
    g, seqs = two_contigs
    rows, motifs = _mixed_rows(seqs[1], random.Random(237), 160)
    table = A.repeats(*rows)
    _check(g.motif_align_local(1, 0, None, table, motifs, *weights), L.local(seqs[1], table, motifs, weights), weights)


def test_n_blocks_lower_case_and_a_motif_with_n(two_contigs):
    g, seqs = two_contigs
    s = seqs[0]
    rows = [(400, 700, 5), (480, 660, 70), (500, 650, 3), (1_000, 1_400, 7), (990, 1_410, 300), (2_000, 2_064, 2), (2_000, 2_164, 2), (4_000, 4_100, 1),
            (3_990, 4_010, 4), (6_000, 6_000 + 171 * 12, 171), (6_010, 6_000 + 171 * 12, 171)]
    unit = s[6_000 + 171 * 3:6_000 + 171 * 4].decode()
    motifs = ["ACGTA", s[700:770].decode(), "NNN", s[1_000:1_007].decode(), s[1_000:1_300].decode().upper(), "AC", "ca", "N", "ANGT", unit,
              unit[:50] + "n" * 5 + unit[55:]]
    motifs = ["".join(c if c in "ACGTNacgtn" else "N" for c in m) for m in motifs]
    table = A.repeats(*rows)
    want = L.local(s, table, motifs, TRF)
    got = g.motif_align_local(0, 0, None, table, motifs)
    _check(got, want)
    assert got[2].tolist() == (0, 0, 0, 0, 0, 0) and got[7].tolist() == (0, 0, 0, 0, 0, 0)    # a motif of N matches nothing, not even N
    assert L.same(got[3:5], L.local(s.upper(), table[3:5], motifs[3:5], TRF)) and got[3]["score"] > 0       # lower case matches upper case
    n_block = next(at for at in range(len(s) - 40) if s[at:at + 40] == b"N" * 40)                          # an all-N window: the zero row
    zero = g.motif_align_local(0, 0, None, A.repeats((n_block, n_block + 40, 3), (n_block + 1, n_block + 2, 1)), ["ACG", "A"])
    assert zero.tolist() == [(0, 0, 0, 0, 0, 0)] * 2


def test_stretches_of_r_and_y_and_the_one_shot_form(ctx):
    """A genome of eight planes: R and Y (and every letter outside ACGT) match nothing, as N does; and the one-shot form."""
    rng = random.Random(238)
    s = bytearray(_random(12_000, 186))
    for at in (300, 5_000, 9_000):
        s[at:at + 90] = bytes(rng.choice(b"RYN") for _ in range(90))
    s[7_000:7_400] = (b"RYRRY" * 80)
    s = bytes(s)
    ks = [1, 5, 64, 65, 400, 1_000]
    rows = [(a, b, k) for k in ks for a, b in ((250, 450), (6_990, 7_300), (7_100, 7_101), (8_950, 9_200))]
    motifs = [_motif_near(s, a + 100, k, rng) for a, _, k in rows]
    table = A.repeats(*rows)
    want = L.local(s, table, motifs, TRF)
    inner = A.repeats((0, 200, 5), (10, 411, 64), (5, 6, 1))                      # position 7 000: an R
    g = ctx.load([s], 64)
    try:
        for begin, end in ((0, None), (0, 12_000)):
            _check(g.motif_align_local(0, begin, end, table, motifs), want, (begin, end))
        got = g.motif_align_local(0, 6_995, 7_406, inner, ["ACAAC", motifs[8], "A"])
        _check(got, L.local(s, inner, ["ACAAC", motifs[8], "A"], TRF, 6_995, 7_406))
        assert got[2].tolist() == (0, 0, 0, 0, 0, 0)
    finally:
        g.free()
    _check(ctx.motif_align_local(s, table, motifs), want, "one shot")
    _check(ctx.motif_align_local(s.decode(), inner, ["ACAAC", motifs[8], "A"], begin=6_995, end=7_406, match=3, mismatch=1, indel=2),
           L.local(s, inner, ["ACAAC", motifs[8], "A"], (3, 1, 2), 6_995, 7_406), "one shot, a range, other weights")
    got = ctx.motif_align_local("ttacgACGtACGACGtt", A.repeats((0, 17, 3)), ["ACG"], indel=3)
    assert got[0].tolist() == (2 * 12 - 3, 2, 15, 0, 2, 0)


def test_the_first_position_and_the_last_of_the_genome(two_contigs):
    g, seqs = two_contigs
    rng = random.Random(239)
    for contig, seq in enumerate(seqs):
        n = len(seq)
        rows = [(0, 1, 1), (0, 70, 7), (0, 130, 65), (0, 40, 1_024), (n - 1, n, 1), (n - 70, n, 3), (n - 200, n, 171), (n - 33, n, 1_000), (0, 300, 300)]
        motifs = [_motif_near(seq, a, k, rng) for a, _, k in rows]
        motifs[0], motifs[4] = seq[:1].decode().upper(), seq[n - 1:].decode().upper()
        table = A.repeats(*rows)
        want = L.local(seq, table, motifs, TRF)
        _check(g.motif_align_local(contig, 0, None, table, motifs), want, contig)
        assert want[0].tolist() == (2, 0, 1, 0, 0, 0) and want[4].tolist() == (2, 0, 1, 0, 0, 0)
        tail = A.repeats((0, 300, 9), (299, 300, 1))
        _check(g.motif_align_local(contig, n - 300, None, tail, ["ACGTACGTA", motifs[4]]), L.local(seq, tail, ["ACGTACGTA", motifs[4]], TRF, n - 300),
               (contig, "a range at the end"))


def test_five_thousand_rows_of_mixed_k_follow_their_rows(two_contigs):
    g, seqs = two_contigs
    rows, motifs = _mixed_rows(seqs[1], random.Random(240), 5_000)
    table = A.repeats(*rows)
    got = g.motif_align_local(1, 0, None, table, motifs)
    assert g.motif_align_local(1, 0, None, table, motifs).tobytes() == got.tobytes()    # equal bytes twice
    back = g.motif_align_local(1, 0, None, table[::-1].copy(), motifs[::-1])            # the results follow the rows
    assert back[::-1].tobytes() == got.tobytes()
    some = np.arange(0, 5_000, 7)                                                       # ... and are the model's
    _check(got[some], L.local(seqs[1], table[some], [motifs[at] for at in some.tolist()], TRF))
    assert int((got["score"] > 0).sum()) > 4_000


def test_a_row_at_the_limit_of_positions(ctx):
    """2^19 positions of one letter with match = 16: against the same letter, at k = 1 and k = 1 024 -- the score field's maximum,
    2^23 -- and against another: the zero row.  The closed form is the model's at 2 048 positions."""
    n = A.MAX_LEN
    assert L.one("A" * 2_048, "A" * 1_024, (16, 1, 1)) == (16 * 2_048, 0, 2_048, 1, 0) and L.one("A" * 2_048, "A", (16, 1, 1)) == (16 * 2_048, 0, 2_048, 0, 0)
    assert L.one("T" + "A" * 2_047, "A" * 1_024, (16, 16, 16)) == (16 * 2_047, 1, 2_048, 2, 0)
    seq = b"ACGT" * 10 + b"A" * n + b"C" * 50
    g = ctx.load([seq], 64)
    try:
        rows = A.repeats((40, 40 + n, 1), (40, 40 + n, 1_024), (40, 40 + n, 1), (40, 40 + n, 3), (39, 39 + n, 1_024))
        motifs = ["A", "A" * 1_024, "C", "GGG", "A" * 1_024]
        got = g.motif_align_local(0, 0, None, rows, motifs, 16, 16, 16)
        assert got[0].tolist() == (1 << 23, 0, n, 0, 0, 0)
        assert got[1].tolist() == (1 << 23, 0, n, 1, 0, 0)
        assert got[2].tolist() == (0, 0, 0, 0, 0, 0) and got[3].tolist() == (0, 0, 0, 0, 0, 0)
        assert got[4].tolist() == ((1 << 23) - 16, 1, n, 2, 0, 0)                   # the T in front is left out
        assert g.motif_align_local(0, 0, None, rows[:2], motifs[:2], 16, 1, 1)["score"].tolist() == [1 << 23] * 2
    finally:
        g.free()


def test_refusals_on_a_resident_genome(ctx, two_contigs):
    import prf_native as pn
    g, _ = two_contigs
    out = np.zeros(1, dtype=pn.LOCAL_ALIGNMENT_DTYPE)

    def call(row, motif, contig=0, end=1 << 63, weights=TRF):
        table = A.repeats(row)
        return ctx.lib.prf_motif_align_local(ctx._h, g._h, contig, 0, end, table.ctypes.data, 1, motif, len(motif), *weights, out.ctypes.data, None)

    assert call((0, 100, 1_025), b"A" * 1_025) == pn.PRF_EUNSUPPORTED and "PRF_ALIGN_MAX_K" in ctx.lib.prf_last_error().decode()
    assert call((0, A.MAX_LEN + 1, 3), b"ACG") == pn.PRF_EUNSUPPORTED and "PRF_ALIGN_MAX_LEN" in ctx.lib.prf_last_error().decode()
    assert call((0, 30, 3), b"ACG", weights=(2, 0, 7)) == pn.PRF_EINVAL and "mismatch is 0" in ctx.lib.prf_last_error().decode()
    assert call((0, 30, 3), b"ACG", weights=(2, 7, 17)) == pn.PRF_EUNSUPPORTED and "PRF_ALIGNLOCAL_MAX_WEIGHT" in ctx.lib.prf_last_error().decode()
    assert call((0, 30_012, 3), b"ACG") == pn.PRF_EINVAL and "row 0: end 30012 is behind the range's 30011 positions" in ctx.lib.prf_last_error().decode()
    assert call((0, 30, 3), b"ACG", contig=2) == pn.PRF_EINVAL and not out["end"][0]
    assert call((0, 30, 3), b"ACG") == pn.PRF_OK and out["end"][0] > 0
    assert ctx.lib.prf_motif_align_local(ctx._h, g._h, 0, 0, 1 << 63, None, 0, None, 0, 2, 7, 7, None, None) == pn.PRF_OK
    with pytest.raises(ValueError, match="more than an alignment takes"):
        g.motif_align_local(0, 0, None, A.repeats((0, 100, 1_025)), ["A" * 1_025])
    with pytest.raises(pn.PrfError, match="row 1: column 2 of the motif"):
        g.motif_align_local(0, 0, None, A.repeats((0, 100, 3), (0, 100, 4)), ["ACG", "ACRT"])
    with pytest.raises(pn.PrfError, match="unsupported symbol at position 4"):
        ctx.motif_align_local("ACGT-ACGT", A.repeats((0, 9, 3)), ["ACG"])


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
        rows = A.repeats((950, 1_110, 3), (0, 3_000, 50), (990, 1_070, 3), (3 * tile, 3 * tile + 400, 700))   # whatever is selected
        motifs = ["CAG", _motif_near(seq, 40, 50, random.Random(241)), "AGC", "ACGT" * 175]
        aligned_before = g.motif_align(0, 0, None, rows, motifs)
        got = g.motif_align_local(0, 0, None, rows, motifs)
        _check(got, L.local(seq, rows, motifs, TRF))
        assert got[0]["score"] >= 120 and got[0]["first"] <= 50 and got[0]["end"] >= 110
        assert ctx.motif_align_local(seq[:2_000], rows[:1], motifs[:1]).tobytes() == got[:1].tobytes()   # the one-shot form, a genome of its own
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


def _extension(chrom, begin, end, fields, motif, flank, weights=TRF):
    start, stop = int(fields[1]), int(fields[2])
    a, b = max(begin, start - flank), min(end, stop + flank)
    score, first, last = L.one(chrom[a:b], motif, weights)[:3]
    return [str(a + first), str(a + last), str(score)] if score else [str(start), str(stop), "0"]


def test_cli_extends_the_repeats_of_an_interval(ctx, tmp_path):
    import plot_periodicity_matrix as cli
    motif, body = K.planted(17, 2, "both")
    chrom = (_random(3_000, 14).decode() + body + "N" * 200 + K.planted(17, 1, "ins")[1] + _random(2_000, 15).decode()).lower()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\nACGT\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    begin, end = 100, len(chrom) - 50
    base = [str(fa), "-i", f"chrT:{begin}-{end}", "--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--chain-window", "1000"]
    for flag, more, name_at in (("--groups-tsv", ["--max-shift", "4", "--min-group", "60", "--group-consensus"], 10), ("--chains-tsv", ["--consensus"], 9)):
        plain, extended, kept = (tmp_path / f"{flag[2:]}.{name}.tsv" for name in ("plain", "extended", "kept"))
        cli.main(base + [flag, str(plain)] + more, context=ctx)
        cli.main(base + [flag, str(extended)] + more + ["--extend", "50", "--weights", "2,7,7"], context=ctx)
        old, new = plain.read_text().splitlines(), extended.read_text().splitlines()
        assert len(old) == len(new) >= 2
        for before, line in zip(old, new):
            fields = before.split("\t")
            assert line.startswith(before + "\t") and line[len(before) + 1:].split("\t") == _extension(chrom, begin, end, fields, fields[name_at], 50), before
        scores = sorted(int(line.split("\t")[-1]) for line in new)
        cli.main(base + [flag, str(kept)] + more + ["--extend", "50", "--min-score", str(scores[-1])], context=ctx)
        assert kept.read_text().splitlines() == [line for line in new if int(line.split("\t")[-1]) >= scores[-1]]
