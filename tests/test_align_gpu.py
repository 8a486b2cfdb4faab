"""GPU (-m gpu): the alignment of tandem repeats to their motifs (prf_motif_align, csrc/align.hip).  Every result is
compared EXACTLY, byte for byte, with the model (tests/align_model.py, pinned to a brute force by tests/test_align_cpu.py).

Shapes: the genome of tests/test_consensus_gpu.py (two contigs of 30 011 and 20 003 positions of ACGT, N blocks and lower case);
rows of 1 to 1 025 positions at every k around the boundaries between the five kernels (64 | 65, 128 | 129, 256 | 257, 512 | 513,
1 024) and every k = 1 .. 1 024 at 24 positions; planted repeats of three to eleven copies with a substitution, an insertion, a
deletion in every kernel; one row of 2^19 positions, the limit, where the packed counts are largest."""
import itertools
import random

import numpy as np
import pytest

import align_model as A
import consensus_model as C
import phased_cases as K
from test_consensus_gpu import _first_contig
from test_dotruns_gpu import _random

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1_023, 1_024]
STARTS = [0, 1, 63]                                           # start % 64
REGIME_KS = [5, 100, 200, 400, 900]                           # one k per kernel


def _lengths(k):
    return sorted({1, max(1, k - 1), k, k + 1, 64, 65, 300})


@pytest.fixture(scope="module")
def ctx():
    import torch  # the same load order as the other GPU tests (torch's HIP runtime first)
    assert torch.cuda.is_available()
    import prf_native
    assert np.dtype(prf_native.ALIGNMENT_DTYPE).itemsize == 24
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
    assert got.dtype == np.dtype(A.DTYPE) and len(got) == len(want), what
    if not A.same(got, want):
        bad = [at for at in range(len(want)) if got[at] != want[at]]
        raise AssertionError((what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]]))


def _motif_near(seq, at, k, rng):
    """k letters of the sequence from `at` on (upper case, N kept), every ninth changed: the rows align with many ties."""
    text = bytearray(seq[at:at + k].upper())
    text += bytes(rng.choice(b"ACGT") for _ in range(k - len(text)))
    for j in range(0, k, 9):
        text[j] = rng.choice(b"ACGT")
    return bytes(b if b in b"ACGTN" else ord("N") for b in text).decode()


@pytest.mark.parametrize("begin", [29, 192])
def test_periods_lengths_and_word_alignments_against_the_model(two_contigs, begin):
    """Every k x every length x every start % 64, in one call per range; begin % 64 is 29 (every word is funnel-shifted) or 0."""
    g, seqs = two_contigs
    rng = random.Random(201)
    rows, motifs = [], []
    for at, (k, start) in enumerate(itertools.product(KS, STARTS)):
        for n in _lengths(k):
            a = start + 64 * (at % 5) + (4_992 if at % 2 else 0)                # random letters, and the N block and lower case
            rows.append((a, a + n, k))
            motifs.append(_motif_near(seqs[0], begin + a + (at % 3), k, rng))
    assert len(rows) > 350 and {a % 64 for a, _, _ in rows} == set(STARTS)
    table = A.repeats(*rows)
    want = A.align(seqs[0], table, motifs, begin, 9_000)
    got, st = g.motif_align(0, begin, 9_000, table, motifs, with_stats=True)
    _check(got, want, begin)
    assert st.path == 14 and st.n_hits == len(rows) and st.positions == sum(b - a for a, b, _ in rows)
    assert st.n_candidates == sum((b - a) * k for a, b, k in rows) and st.n_launches == 5 and st.scan_ms > 0 and st.scan_ms == st.phase1_ms
    assert int((want["indels"] > 0).sum()) > 50 and int((want["edits"] == 0).sum()) > 10    # the inputs: gapped alignments, perfect ones
    _check(g.motif_align(0, begin, 9_000, table, "".join(motifs)), want, "the letters in one buffer")


def test_every_k_in_one_call(two_contigs):
    g, seqs = two_contigs
    rng = random.Random(202)
    rows = [(100 + 7 * k, 124 + 7 * k, k) for k in range(1, 1_025)]
    motifs = [_motif_near(seqs[1], 100 + 7 * k - (k % 5), k, rng) for k in range(1, 1_025)]
    table = A.repeats(*rows)
    _check(g.motif_align(1, 0, None, table, motifs), A.align(seqs[1], table, motifs))


def _planted_genome():
    """For every kernel's k: a motif, and rows that are copies of it -- perfect from three phases, with one substitution, one
    insertion, one deletion, one of each -- between random flanks.  Returns (sequence, rows, motifs, what each row must give)."""
    rng = random.Random(203)
    seq, rows, motifs, expect = bytearray(_random(37, 204)), [], [], []
    for k in REGIME_KS:
        motif = ""
        while not motif or not K.primitive(motif):
            motif = "".join(rng.choice("ACGT") for _ in range(k))
        copies = 11 if k == 5 else 3
        for phase, edits in ((0, ""), (1, ""), (k - 1, ""), (2, "S"), (0, "I"), (3, "D"), (1, "SID")):
            body = [motif[(phase + t) % k] for t in range(copies * k + 2)]
            places = sorted(rng.sample(range(k // 2 + 2, len(body) - k // 2 - 2, max(1, k // 3)), len(edits)), reverse=True)
            for place, kind in zip(places, edits):
                if kind == "S":
                    body[place] = next(c for c in "ACGT" if c != body[place])
                elif kind == "I":
                    body.insert(place, next(c for c in "acgt" if c.upper() not in (body[place - 1], body[place])))
                else:
                    del body[place]
            rows.append((len(seq), len(seq) + len(body), k))
            motifs.append(motif)
            n_ins, n_del = edits.count("I"), edits.count("D")
            consumed = len(body) - n_ins + n_del
            expect.append((len(edits), n_ins + n_del, consumed, phase, (phase + consumed - 1) % k))
            seq += "".join(body).encode() + _random(rng.randrange(1, 90), rng.randrange(1 << 30))
    return bytes(seq), rows, motifs, expect


def test_planted_repeats_in_every_kernel(ctx):
    seq, rows, motifs, expect = _planted_genome()
    table = A.repeats(*rows)
    want = A.align(seq, table, motifs)
    assert [tuple(r)[:5] for r in want.tolist()] == expect                       # the model finds what was planted
    g = ctx.load([seq], 64)
    try:
        _check(g.motif_align(0, 0, None, table, motifs), want)
        # the motif rotated: the same counts, the columns turned
        turned = [m[3 % len(m):] + m[:3 % len(m)] for m in motifs]
        got = g.motif_align(0, 0, None, table, turned)
        _check(got, A.align(seq, table, turned))
        assert all(np.array_equal(got[f], want[f]) for f in ("edits", "indels", "consumed"))
    finally:
        g.free()


def test_n_blocks_lower_case_and_a_motif_with_n(two_contigs):
    g, seqs = two_contigs
    s = seqs[0]
    rows = [(400, 700, 5), (480, 660, 70), (500, 650, 3), (1_000, 1_400, 7), (990, 1_410, 300), (2_000, 2_064, 2), (2_000, 2_164, 2), (4_000, 4_100, 1),
            (3_990, 4_010, 4), (6_000, 6_000 + 171 * 30, 171), (6_010, 6_000 + 171 * 12, 171)]
    unit = s[6_000 + 171 * 3:6_000 + 171 * 4].decode()
    motifs = ["ACGTA", s[700:770].decode(), "NNN", s[1_000:1_007].decode(), s[1_000:1_300].decode().upper(), "AC", "ca", "N", "ANGT", unit,
              unit[:50] + "n" * 5 + unit[55:]]
    motifs = ["".join(c if c in "ACGTNacgtn" else "N" for c in m) for m in motifs]
    table = A.repeats(*rows)
    want = A.align(s, table, motifs)
    got = g.motif_align(0, 0, None, table, motifs)
    _check(got, want)
    assert got[2].tolist()[:3] == (150, 0, 150) and got[7].tolist()[:3] == (100, 0, 100)    # N matches nothing, not even N
    assert got[5].tolist()[:5] == (0, 0, 64, 0, 1)                                        # AC x 32
    assert A.same(got[3:5], A.align(s.upper(), table[3:5], motifs[3:5])) and got[3]["edits"] < 300     # lower case matches upper case
    assert 0 < got[9]["edits"] < 171 * 30 // 4 and got[10]["edits"] >= 5 * 11               # a diverged array; a motif N costs every copy


def test_stretches_of_r_and_y_and_the_one_shot_form(ctx):
    """A genome of eight planes: R and Y (and every letter outside ACGT) match nothing, as N does; and the one-shot form."""
    rng = random.Random(205)
    s = bytearray(_random(12_000, 186))
    for at in (300, 5_000, 9_000):
        s[at:at + 90] = bytes(rng.choice(b"RYN") for _ in range(90))
    s[7_000:7_400] = (b"RYRRY" * 80)
    s = bytes(s)
    ks = [1, 5, 64, 65, 400, 1_000]
    rows = [(a, b, k) for k in ks for a, b in ((250, 450), (6_990, 7_300), (7_100, 7_101), (8_950, 9_200))]
    motifs = [_motif_near(s, a + 100, k, rng) for a, _, k in rows]
    table = A.repeats(*rows)
    want = A.align(s, table, motifs)
    g = ctx.load([s], 64)
    try:
        for begin, end in ((0, None), (0, 12_000)):
            _check(g.motif_align(0, begin, end, table, motifs), want, (begin, end))
        inner = A.repeats((0, 200, 5), (10, 411, 64), (5, 6, 1))                  # position 7 000: an R
        got = g.motif_align(0, 6_995, 7_406, inner, ["RYRRY".replace("R", "A").replace("Y", "C"), motifs[8], "A"])
        _check(got, A.align(s, inner, ["ACAAC", motifs[8], "A"], 6_995, 7_406))
        assert got[2].tolist()[:3] == (1, 0, 1)
    finally:
        g.free()
    _check(ctx.motif_align(s, table, motifs), want, "one shot")
    _check(ctx.motif_align(s.decode(), inner, ["ACAAC", motifs[8], "A"], begin=6_995, end=7_406), A.align(s, inner, ["ACAAC", motifs[8], "A"], 6_995, 7_406),
           "one shot, a range")
    got = ctx.motif_align("acgACGtACGACG", A.repeats((0, 13, 3)), ["ACG"])
    assert got[0].tolist()[:5] == (1, 1, 12, 0, 2)


def test_the_first_position_and_the_last_of_the_genome(two_contigs):
    g, seqs = two_contigs
    rng = random.Random(206)
    for contig, seq in enumerate(seqs):
        n = len(seq)
        rows = [(0, 1, 1), (0, 70, 7), (0, 130, 65), (0, 40, 1_024), (n - 1, n, 1), (n - 70, n, 3), (n - 200, n, 171), (n - 33, n, 1_000), (0, 300, 300)]
        motifs = [_motif_near(seq, a, k, rng) for a, _, k in rows]
        table = A.repeats(*rows)
        _check(g.motif_align(contig, 0, None, table, motifs), A.align(seq, table, motifs), contig)
        _check(g.motif_align(contig, n - 300, None, A.repeats((0, 300, 9), (299, 300, 2)), ["ACGTACGTA", "GT"]),
               A.align(seq, A.repeats((0, 300, 9), (299, 300, 2)), ["ACGTACGTA", "GT"], n - 300), (contig, "a range at the end"))


def test_five_thousand_rows_of_mixed_k_follow_their_rows(two_contigs):
    g, seqs = two_contigs
    rng = random.Random(207)
    n = len(seqs[1])
    rows, motifs = [], []
    for _ in range(5_000):
        k = rng.choice((1, 2, 3, 4, 6, 17, 33, 64)) if rng.random() < 0.9 else rng.choice((65, 128, 171, 257, 700, 1_024))
        start = rng.randrange(n - 200)
        rows.append((start, start + rng.choice((1, 2, 10, 24, 64, 65, 130)), k))
        motifs.append(_motif_near(seqs[1], start + rng.randrange(3), k, rng))
    table = A.repeats(*rows)
    want = A.align(seqs[1], table, motifs)
    got = g.motif_align(1, 0, None, table, motifs)
    _check(got, want)
    assert g.motif_align(1, 0, None, table, motifs).tobytes() == got.tobytes()    # equal bytes twice
    back = g.motif_align(1, 0, None, table[::-1].copy(), motifs[::-1])            # the results follow the rows
    assert back[::-1].tobytes() == got.tobytes()


def test_a_row_at_the_limit_of_positions(ctx):
    """2^19 positions of one letter: against the same letter, at k = 1 and k = 1 024, and against another (closed forms): the
    packed counts at their largest."""
    n = A.MAX_LEN
    seq = b"ACGT" * 10 + b"A" * n + b"C" * 50
    g = ctx.load([seq], 64)
    try:
        rows = A.repeats((40, 40 + n, 1), (40, 40 + n, 1_024), (40, 40 + n, 1), (40, 40 + n, 3), (39, 39 + n, 1))
        got = g.motif_align(0, 0, None, rows, ["A", "A" * 1_024, "C", "CCC", "A"])
        assert got[0].tolist() == (0, 0, n, 0, 0, 0)
        assert got[1].tolist() == (0, 0, n, (1 - n) % 1_024, 0, 0)
        assert got[2].tolist() == (n, 0, n, 0, 0, 0)
        assert got[3].tolist() == (n, 0, n, (1 - n) % 3, 0, 0)
        assert got[4].tolist() == (1, 0, n, 0, 0, 0)                               # the T in front: a substitution, not an insertion
    finally:
        g.free()


def test_refusals_on_a_resident_genome(ctx, two_contigs):
    import prf_native as pn
    g, _ = two_contigs
    out = np.zeros(1, dtype=pn.ALIGNMENT_DTYPE)

    def call(row, motif, contig=0, end=1 << 63):
        table = A.repeats(row)
        return ctx.lib.prf_motif_align(ctx._h, g._h, contig, 0, end, table.ctypes.data, 1, motif, len(motif), out.ctypes.data, None)

    assert call((0, 100, 1_025), b"A" * 1_025) == pn.PRF_EUNSUPPORTED and "PRF_ALIGN_MAX_K" in ctx.lib.prf_last_error().decode()
    assert call((0, A.MAX_LEN + 1, 3), b"ACG") == pn.PRF_EUNSUPPORTED and "PRF_ALIGN_MAX_LEN" in ctx.lib.prf_last_error().decode()
    assert call((0, 30_012, 3), b"ACG") == pn.PRF_EINVAL and "row 0: end 30012 is behind the range's 30011 positions" in ctx.lib.prf_last_error().decode()
    assert call((0, 30, 3), b"ACG", contig=2) == pn.PRF_EINVAL and not out["consumed"][0]
    assert call((0, 30, 3), b"ACG") == pn.PRF_OK and out["consumed"][0] > 0
    assert ctx.lib.prf_motif_align(ctx._h, g._h, 0, 0, 1 << 63, None, 0, None, 0, None, None) == pn.PRF_OK
    with pytest.raises(ValueError, match="more than an alignment takes"):
        g.motif_align(0, 0, None, A.repeats((0, 100, 1_025)), ["A" * 1_025])
    with pytest.raises(pn.PrfError, match="row 1: column 2 of the motif"):
        g.motif_align(0, 0, None, A.repeats((0, 100, 3), (0, 100, 4)), ["ACG", "ACRT"])
    with pytest.raises(pn.PrfError, match="unsupported symbol at position 4"):
        ctx.motif_align("ACGT-ACGT", A.repeats((0, 9, 3)), ["ACG"])


@pytest.mark.parametrize("kind", ["ins", "del", "both"])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("period", [7, 17, 40])
def test_a_planted_repeat_from_the_chains_to_its_alignment(ctx, period, d, kind):
    """period_chains -> tandem_rows -> period_consensus -> motif_align, and ... -> group_segments -> phased_consensus -> motif_align
    over the whole of each group against the motif of its chosen piece, on the planted inputs of tests/phased_cases.py."""
    import prf_native as pn
    motif, seq = K.planted(period, d, kind)
    g = ctx.load([seq.encode()], 64)
    try:
        chains = g.period_chains(0, 0, None, 1, period + 8, K.MIN_SEED[period], K.MAX_GAP, 0)
        links = g.period_links(0, 0, None, 1, period + 8, K.MIN_SEED[period], K.MAX_GAP, K.MAX_SHIFT)
        tandem = pn.tandem_rows(chains)
        cons, names = g.period_consensus(0, 0, None, tandem)
        aligned = g.motif_align(0, 0, None, tandem, names)
        groups = pn.join_period_chains(chains, links)
        pieces, segments = pn.group_segments(chains, links)
        pcons, pnames = g.phased_consensus(0, 0, None, pieces["k"], segments)
        rows, chosen = pn.group_consensus_rows(groups, pieces, pcons, pnames)
        whole = np.zeros(len(groups), dtype=pn.REPEAT_DTYPE)
        whole["start"], whole["end"], whole["k"] = groups["start"], groups["end"], [len(m) for m in chosen]
        galigned = g.motif_align(0, 0, None, whole, "".join(chosen))
    finally:
        g.free()
    _check(aligned, A.align(seq, tandem, names), "the repeats")
    _check(galigned, A.align(seq, whole, chosen), "the groups")
    assert (aligned["edits"].astype(np.int64) <= (tandem["end"] - tandem["start"]).astype(np.int64) - cons["agree"].astype(np.int64)).all()
    at = K.body_group(groups, period, len(seq))
    full = pn.alignment_rows(rows, galigned)[at]
    assert full["ins"] + full["del"] == galigned["indels"][at] == d * (2 if kind == "both" else 1)


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
        plain = C.repeats((1_000, 1_060, 3), (0, 3_000, 50))
        named_before = g.period_consensus(0, 0, None, plain, counts=True)
        rows = A.repeats((1_000, 1_060, 3), (0, 3_000, 50), (990, 1_070, 3), (3 * tile, 3 * tile + 400, 700))   # whatever is selected
        motifs = ["CAG", named_before[1][1], "AGC", "ACGT" * 175]
        got = g.motif_align(0, 0, None, rows, motifs)
        _check(got, A.align(seq, rows, motifs))
        assert got[0].tolist()[:5] == (0, 0, 60, 0, 2)
        assert ctx.motif_align(seq[:2_000], rows[:1], motifs[:1])[0].tolist()[:3] == (0, 0, 60)   # the one-shot form, a genome of its own
        assert np.array_equal(buf.cpu().numpy(), sink_before)                 # nothing was written to the sink
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


def _aligned_columns(chrom, fields, motif):
    start, end, k = (int(x) for x in fields[1:4])
    al = A.align_one(chrom[start:end], motif)
    subs, ins, dele, _, identity, copies = A.derived(end - start, k, *al[:3])
    return [str(al[0]), str(subs), str(ins), str(dele), f"{identity:.4f}", f"{copies:.2f}"]


def test_cli_aligns_the_repeats_of_an_interval(ctx, tmp_path):
    import plot_periodicity_matrix as cli
    motif, body = K.planted(17, 2, "both")
    chrom = (_random(3_000, 14).decode() + body + "N" * 200 + K.planted(17, 1, "ins")[1] + _random(2_000, 15).decode()).lower()
    fa = tmp_path / "g.fa"
    fa.write_text(">other\nACGT\n>chrT\n" + "\n".join(chrom[i:i + 70] for i in range(0, len(chrom), 70)) + "\n")
    base = [str(fa), "-i", f"chrT:100-{len(chrom) - 50}", "--max-motif-size", "25", "--min-seed", "12", "--max-gap", "8", "--chain-window", "1000"]
    for flag, more, name_at in (("--groups-tsv", ["--max-shift", "4", "--min-group", "60", "--group-consensus"], 10), ("--chains-tsv", ["--consensus"], 9)):
        plain, aligned, kept = (tmp_path / f"{flag[2:]}.{name}.tsv" for name in ("plain", "aligned", "kept"))
        cli.main(base + [flag, str(plain)] + more, context=ctx)
        cli.main(base + [flag, str(aligned)] + more + ["--align"], context=ctx)
        old, new = plain.read_text().splitlines(), aligned.read_text().splitlines()
        assert len(old) == len(new) >= 2
        gapped = 0
        for before, line in zip(old, new):
            fields = before.split("\t")
            assert line.startswith(before + "\t") and line[len(before) + 1:].split("\t") == _aligned_columns(chrom, fields, fields[name_at]), before
            if flag == "--groups-tsv" and fields[3] == "17" and int(fields[2]) - int(fields[1]) > 400:
                gapped += 1
                assert int(line.split("\t")[-4]) + int(line.split("\t")[-3]) in (1, 4)      # one insertion; two inserted and two deleted bases
        assert gapped == (2 if flag == "--groups-tsv" else 0)
        cli.main(base + [flag, str(kept)] + more + ["--align", "--min-aligned-identity", "0.97"], context=ctx)
        assert kept.read_text().splitlines() == [line for line in new if float(line.split("\t")[-2]) >= 0.97]
