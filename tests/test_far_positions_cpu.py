"""CPU: what tests/test_far_positions_gpu.py is built around (tests/far_cases.py), proven without a GPU and without the 2 GB
fillers, which are lengths only here -- the layout that puts global 2^31 and 2^32 inside a small contig, the crafted contigs of
the loaded genome, every product case of that genome through its CPU model with the floors that keep it from passing vacuously
(a run, chain, link, set cell or count across the boundary; an entry wholly beyond 2^32), and the host codec of the 8-byte wire
rows at those positions, which refuses what the 23-bit tile field cannot hold."""
import numpy as np
import pytest

import far_cases as F
import multi_gpu

T, EDGE = F.T, F.EDGE


# ---- 1. the layout ----

@pytest.mark.parametrize("hint", sorted(set(F.HINTS) | {1, 900}))     # the hints in use, and the ends of what the fillers' margin allows
def test_the_layout_puts_both_boundaries_inside_a_small_contig(hint):
    bases = F.expected_bases(F.FAR_LENS, hint)
    assert bases == F.FAR_BASES == [0, 2 ** 31 - 2 * T, 2 ** 31 + 2 * T, 2 ** 32 - 2 * T, 2 ** 32 + 2 * T]
    assert bases[1] + EDGE == 2 ** 31 and bases[3] + EDGE == 2 ** 32 and bases[4] > 2 ** 32
    assert all(b % T == 0 for b in bases) and EDGE % T == 0 and EDGE % 64 == 0
    for c in (1, 3):
        assert bases[c] < bases[c] + EDGE < bases[c] + F.FAR_LENS[c]       # the boundary lies inside the contig
    assert [F.FAR_LENS[c] for c in F.FAR_OF] == list(F.SMALL_LENS)
    assert F.expected_bases(F.SMALL_LENS, hint) == [0, 4 * T, 8 * T]
    # the whole coordinate space, with the sentinel tile, stays below 2^35: byte offsets of the planes stay below 2^32
    assert bases[4] + 2 * T + T < 2 ** 35


def test_the_rule_is_the_librarys():
    """expected_bases against hand-computed cases of roundup(base + len + kmax_hint + 64, T)."""
    assert F.expected_bases([1, 1], 1) == [0, T]
    assert F.expected_bases([T - 65, 5], 1) == [0, T]              # T - 65 + 1 + 64 = T: exactly full
    assert F.expected_bases([T - 64, 5], 1) == [0, 2 * T]          # one more position: the next tile
    assert F.expected_bases([0, 0, 7], 50) == [0, T, 2 * T]        # an empty contig still takes its guard gap


# ---- 2. the crafted contigs ----

def test_the_crafted_contigs_hold_what_the_cases_need():
    import dotpair_model as P
    import test_dotruns_gpu as DR
    c1, c3, c4 = F.b_contigs()
    assert [len(c) for c in (c1, c3, c4)] == list(F.SMALL_LENS)
    s1, s3 = c4[F.S1_AT:F.S1_AT + F.PIECE], c4[F.S3_AT:F.S3_AT + F.PIECE]
    # the copy across 2^31 and the inverted copy across 2^32, at begins that are no multiple of 64
    assert c1[F.C1_COPY:F.C1_COPY + F.PIECE] == s1 and F.C1_COPY < EDGE < F.C1_COPY + F.PIECE and F.C1_COPY % 64
    assert c3[F.C3_COPY:F.C3_COPY + F.PIECE] == P.revcomp(s3) and F.C3_COPY < EDGE < F.C3_COPY + F.PIECE and F.C3_COPY % 64
    assert c1[EDGE] == s1[F.CENTRE] and c3[EDGE - 1] == P.comp(s3[F.CENTRE:F.CENTRE + 1])[0]
    # the perfect tandem repeat of period 7 across EDGE of contig 1, bounded on both sides
    lo, hi = EDGE - 60, EDGE + 24
    assert all(c1[i] == c1[i + 7] for i in range(lo, hi - 7)) and c1[lo - 1] != c1[lo + 6] and c1[hi] != c1[hi - 7] and lo % 64
    # the tandem repeat of period 33 across EDGE of contig 3: mismatches on its line, none of them within 4 cells of EDGE
    lo, hi = F.C3_COPY + F.PIECE - 1 - (F.CENTRE - 200 + 429 - 1), F.C3_COPY + F.PIECE - (F.CENTRE - 200)
    assert lo < EDGE - 100 and hi > EDGE + 100 and lo % 64
    line = [c3[i] == c3[i + 33] for i in range(lo, hi - 33)]
    assert 10 <= line.count(False) <= 22 and all(line[EDGE - 4 - lo:EDGE + 4 - lo])
    # the N block, U and the single R near EDGE in both contigs, off the word boundaries
    for contig, at_n, at_u, at_r in ((c1, F.C1_COPY + 700, F.C1_COPY + 1_500, F.C1_COPY + F.R_AT),
                                     (c3, F.C3_COPY + F.PIECE - 1_000, F.C3_COPY + F.PIECE - 1_500 - len(DR.U), F.C3_COPY + F.PIECE - 1 - F.R_AT)):
        assert contig[at_n:at_n + 300] == b"N" * 300 and contig[at_n - 1] != ord("N") and contig[at_n + 300] != ord("N")
        assert contig[at_u:at_u + len(DR.U)] in (DR.U, P.revcomp(DR.U)) and contig[at_r] in b"RY"
        assert all(at % 64 and abs(at - EDGE) < 2_300 for at in (at_n, at_u, at_r))
    # the copies with substitutions and with indels
    sub = c4[F.S1_SUBST_AT:F.S1_SUBST_AT + F.PIECE]
    differ = [i for i in range(F.PIECE) if sub[i] != s1[i]]
    assert 50 <= len(differ) <= 60 and all(i % 101 == 50 for i in differ)
    ind = c4[F.S1_INDEL_AT:F.S1_INDEL_AT + F.PIECE]
    assert ind[:1_200] == s1[:1_200] and ind[1_201:F.CENTRE + 1] == s1[1_200:F.CENTRE]
    assert ind[F.CENTRE + 3:4_003] == s1[F.CENTRE:4_000] and ind[4_003:F.PIECE] == s1[4_003:]
    assert c1[F.S3_COPY_AT:F.S3_COPY_AT + F.PIECE] == s3 and c1[F.S3_SUBST_AT:F.S3_SUBST_AT + F.PIECE] == F.substituted(s3)
    assert c1[F.S3_INDEL_AT:F.S3_INDEL_AT + F.PIECE] == F.with_indels(s3, 107)
    assert c4[F.FAR_K_AT:F.FAR_K_AT + F.FAR_K_LEN] == c4[F.FAR_K_AT + F.FAR_K:F.FAR_K_AT + F.FAR_K + F.FAR_K_LEN]
    # N up to the last position; letters outside ACGTN: the genome takes the eight-plane kernels and the scan has exotic tiles
    assert all(c[-40:] == b"N" * 40 and c[-41] != ord("N") for c in (c1, c3, c4))
    assert all(set(c) - set(b"ACGTN") for c in (c1, c3, c4))
    # ... which lie in one tile of contig 1 and one of contig 3: a tile two away from them is left to the fused kernel
    for contig, tile in ((c1, 1), (c3, 2)):
        assert {i // T for i, x in enumerate(contig) if x not in b"ACGTN"} == {tile}


def test_the_generated_contigs_are_the_recipes():
    import synth
    seqs = F.a_contigs()
    assert [len(s) for s in seqs] == list(F.SMALL_LENS) and all(set(s) <= set(b"ACGTN") for s in seqs)
    c, off = F.FAR_OF[0], EDGE - 100
    assert F.a_window(c, off, 300) == seqs[0][off:off + 300]
    n = F.FAR_LENS[0]
    tail = F.a_window(0, n - 400_000, 400_000)
    assert len(tail) == 400_000 and tail[-synth.standin2_layout(n)[1]:] == b"N" * 10_000 and tail[:1_000].count(b"N") == 0


# ---- 3. every product case of the loaded genome, and the cheap ones of the generated genome ----

ON_CPU = [c for c in F.CASES if c.genome == "B" or c.kind != "pair"]


@pytest.mark.parametrize("case", ON_CPU, ids=[c.name for c in ON_CPU])
def test_the_case_is_not_vacuous(case):
    """models() asserts the floors of the case on the model's output; here also that every array holds something."""
    out = F.models(case)
    labels = [label for label, _ in out]
    assert len(set(labels)) == len(labels) and len(out) >= 2
    assert case.pins in ("2^31", "2^32", "beyond")
    if case.pins != "beyond":                                    # a range of the contig that straddles EDGE
        side = case.b if case.opt and case.opt.get("across") == "columns" else case.a
        assert side[0] == ("2^31", "2^32").index(case.pins) and side[1] < EDGE < side[2]
    else:
        assert case.a[0] == 2 and (case.b is None or case.b[0] == 2 or case.b[2] is None)
    assert any(np.asarray(a).size and (len(a) if a.dtype.names else a.any()) for _, a in out)


def test_the_cases_cover_every_product_at_every_place():
    kinds = {(c.genome, c.kind, c.pins) for c in F.CASES}
    for genome, wanted in (("B", ("period", "dotplot", "pchains", "pair", "chains", "links")), ("A", ("period", "dotplot", "pchains", "pair", "links"))):
        for kind in wanted:
            for pins in ("2^31", "2^32", "beyond"):
                assert (genome, kind, pins) in kinds, (genome, kind, pins)
    # every kind at every place on either genome: a begin on a word of the planes and one 37 bits into a word
    begins = {}
    for c in F.CASES:
        begins.setdefault((c.genome, c.kind, c.pins), set()).add(F.place_begin(c) % 64)
    assert all(found >= {0, 37} for found in begins.values()), {k: v for k, v in begins.items() if not v >= {0, 37}}
    strands = {(c.pins, c.opt["across"], c.strand) for c in F.CASES if c.genome == "B" and c.kind == "pair" and not c.opt.get("self")}
    assert strands >= {(p, o, s) for p in ("2^31", "2^32") for o in ("rows", "columns") for s in "+-"}


# ---- 4. the host codec of the wire rows ----

def _rows(*rows):
    return np.array(list(rows), dtype=multi_gpu.ROW_DTYPE)


def test_wire_rows_round_trip_at_the_far_bases():
    bases = F.expected_bases(F.FAR_LENS, F.HINT_A)
    rows = _rows((EDGE - 1, EDGE + 11, 3, 1),                  # global start 2^31 - 1
                 (EDGE, EDGE + 40, 7, 1),                      # 2^31
                 (EDGE - 30, EDGE - 30 + 70_000, 2, 3),        # a long row across 2^32: through the side list, contig index 3
                 (EDGE - 1, EDGE + 20, 5, 3),                  # 2^32 - 1
                 (EDGE, EDGE + 65_534, 1, 3),                  # 2^32, the longest span the word holds
                 (0, 9, 1, 4), (T - 1, T + 30, 50, 4), (70_001 - 12, 70_001, 4, 4))
    assert [int(bases[r["contig"]]) + int(r["start"]) for r in rows[[0, 1, 3, 4]]] == [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32]
    cap, side = len(rows) + 2, 2
    words = multi_gpu.pack_rows(rows, cap, side, bases, T)
    assert int(words[cap]) == len(rows) | (1 << 40)
    assert words[cap + 1:cap + 4].tolist() == [EDGE - 30, EDGE - 30 + 70_000, 2 | (3 << 32)] and not words[cap + 4:].any()
    tiles = (words[:len(rows)] >> np.uint64(41)).tolist()
    assert tiles[:2] == [2 ** 15 - 1, 2 ** 15] and tiles[3:5] == [2 ** 16 - 1, 2 ** 16] and min(tiles[5:]) >= 2 ** 16 + 2
    assert ((words[:len(rows)] >> np.uint64(25)) & np.uint64(0xFFFF)).tolist()[:5] == [T - 1, 0, T - 30, T - 1, 0]
    back = multi_gpu.unpack_rows(words, cap, side, bases, T)
    assert back.dtype == rows.dtype and np.array_equal(back, rows)


def test_the_wire_row_addresses_2_to_the_39_positions():
    """The tile field has 23 bits: the last position the wire row holds is 2^39 - 1, and pack_rows refuses the next one, where
    it used to wrap to position 0 (a genome may hold 2^40 positions)."""
    bases = [0, 2 ** 39 - T, 2 ** 39]
    last = _rows((7, 19, 3, 0), (T - 1, T + 11, 3, 1))          # global start 2^39 - 1
    words = multi_gpu.pack_rows(last, 2, 0, bases, T)
    assert int(words[1]) >> 41 == 2 ** 23 - 1 and (int(words[1]) >> 25) & 0xFFFF == T - 1
    assert np.array_equal(multi_gpu.unpack_rows(words, 2, 0, bases, T), last)
    for beyond in (_rows((T, T + 12, 3, 1)), _rows((0, 12, 3, 2)), _rows((7, 19, 3, 0), (5, 17, 3, 2)),
                   _rows((2 ** 39, 2 ** 39 + 12, 3, 0))):
        with pytest.raises(ValueError, match="2\\^39"):
            multi_gpu.pack_rows(beyond, 4, 1, bases, T)
    assert multi_gpu.WIRE_POSITIONS == 2 ** 39 == (2 ** 23) * T
