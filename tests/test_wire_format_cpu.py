"""CPU: the 8-byte wire format of the multi-GPU gather on the host (multi_gpu.pack_rows / unpack_rows) at its field boundaries,
and what the cases of tests/test_pipelined_edges_gpu.py are built around, asserted with the oracle."""
import numpy as np
import pytest

import multi_gpu
import pipelined_edges_cases as cases

TILE = cases.TILE
SPANS = (9, 10, 300, 65_533, 65_534, 65_535, 65_536, 65_537, 70_000, 200_000)


def random_rows(rng):
    """-> (rows, bases): 1 to 5 contigs whose bases are tile multiples; starts at tile offsets 0 and 65 535 among others, spans on
    either side of the span field's limit, motif sizes 1 .. 511.  Unique in (contig, start, k), as the rows of a scan are."""
    n_contigs = int(rng.integers(1, 6))
    tiles = rng.integers(5, 40, size=n_contigs)
    bases = np.concatenate(([0], np.cumsum(tiles)[:-1])).astype(np.uint64) * np.uint64(TILE)
    lens = tiles * TILE - rng.integers(0, TILE, size=n_contigs)
    seen, out = set(), []
    for _ in range(int(rng.integers(0, 40))):
        c = int(rng.integers(0, n_contigs))
        span = int(rng.choice(SPANS)) if rng.random() < 0.7 else int(rng.integers(1, 3 * TILE))
        k = int(rng.choice([1, 2, 255, 256, 510, 511])) if rng.random() < 0.5 else int(rng.integers(1, 512))
        room = int(lens[c]) - span
        offset = int(rng.choice([0, 1, TILE - 1, TILE - 2])) if rng.random() < 0.6 else int(rng.integers(0, TILE))
        start = int(rng.integers(0, room // TILE)) * TILE + offset
        if start > room or (c, start, k) in seen:
            continue
        seen.add((c, start, k))
        out.append((start, start + span, k, c))
    rows = np.array(out, dtype=multi_gpu.ROW_DTYPE) if out else np.zeros(0, dtype=multi_gpu.ROW_DTYPE)
    return rows[np.lexsort((rows["end"], rows["start"], rows["contig"]))], bases


def test_pack_and_unpack_round_trip_on_random_row_sets():
    rng = np.random.default_rng(2024)
    seen_spans, seen_offsets, seen_k = set(), set(), set()
    for _ in range(200):
        rows, bases = random_rows(rng)
        n_long = int(np.count_nonzero(rows["end"] - rows["start"] >= 65_535))
        cap, side = len(rows) + int(rng.integers(0, 4)), n_long + int(rng.integers(0, 3))
        words = multi_gpu.pack_rows(rows, cap, side, bases, TILE)
        assert words.dtype == np.uint64 and len(words) == cap + 1 + 3 * side
        assert int(words[cap]) == len(rows) | (n_long << 40)
        assert np.array_equal(multi_gpu.unpack_rows(words, cap, side, bases, TILE), rows)
        assert np.array_equal(multi_gpu.unpack_rows(words.view(np.int64), cap, side, bases, TILE), rows)   # as a torch tensor holds them
        seen_spans.update((rows["end"] - rows["start"]).tolist())
        seen_offsets.update(((bases[rows["contig"]] + rows["start"]) % np.uint64(TILE)).tolist())
        seen_k.update(rows["k"].tolist())
    assert {65_534, 65_535, 65_536} <= seen_spans and {0, 65_535} <= seen_offsets and {1, 511} <= seen_k


def test_a_span_of_65534_is_the_last_that_stays_in_the_word():
    bases = np.array([0, 3 * TILE], dtype=np.uint64)
    rows = np.array([(65_535, 65_535 + 65_534, 511, 1), (65_536, 65_536 + 65_535, 1, 1)], dtype=multi_gpu.ROW_DTYPE)
    words = multi_gpu.pack_rows(rows, 2, 1, bases, TILE)
    assert int(words[0]) == (3 << 41) | (65_535 << 25) | (65_534 << 9) | 511
    assert int(words[1]) == (4 << 41) | (0 << 25) | (65_535 << 9) | 1
    assert words[2:].tolist() == [2 | (1 << 40), 65_536, 65_536 + 65_535, 1 | (1 << 32)]


def test_refusals_of_the_host_encoder_and_the_poisoned_count_word():
    bases = np.array([0], dtype=np.uint64)
    rows = np.array([(0, 12, 2, 0), (100, 100 + 65_535, 1, 0), (70_000, 170_000, 3, 0)], dtype=multi_gpu.ROW_DTYPE)
    assert np.array_equal(multi_gpu.unpack_rows(multi_gpu.pack_rows(rows, 3, 2, bases, TILE), 3, 2, bases, TILE), rows)
    with pytest.raises(ValueError):
        multi_gpu.pack_rows(rows, 2, 2, bases, TILE)            # too many rows
    with pytest.raises(ValueError):
        multi_gpu.pack_rows(rows, 3, 1, bases, TILE)            # too many long rows
    wide = rows.copy()
    wide["k"][0] = 512
    with pytest.raises(ValueError):
        multi_gpu.pack_rows(wide, 3, 2, bases, TILE)            # the motif size has 9 bits
    wide["k"][0] = 511
    assert int(multi_gpu.unpack_rows(multi_gpu.pack_rows(wide, 3, 2, bases, TILE), 3, 2, bases, TILE)["k"][0]) == 511
    words = multi_gpu.pack_rows(rows, 3, 2, bases, TILE)
    words[3] = np.uint64(0xFFFFFFFFFFFFFFFF)
    with pytest.raises(ValueError):
        multi_gpu.unpack_rows(words, 3, 2, bases, TILE)
    with pytest.raises(ValueError):
        multi_gpu.unpack_rows(words.view(np.int64), 3, 2, bases, TILE)


def as_tuples(rows):
    return [(int(r["contig"]), int(r["start"]), int(r["end"]), int(r["k"])) for r in rows]


def test_cases_hold_what_they_are_built_around():
    """What tests/test_pipelined_edges_gpu.py relies on, from the oracle alone."""
    # A: a row starts in front of every cut and ends behind it; the three largest sizes do so somewhere; one row is longer than the
    # span field holds; the N block cuts the rows at its cut
    seqs, rows = cases.share_genome()
    assert [len(s) for s in seqs] == cases.SHARE_LENS
    crossing_k, starting_k = set(), set()
    for c, s in enumerate(seqs):
        for cut in range(TILE, len(s), TILE):
            over = rows[(rows["contig"] == c) & (rows["start"] < cut) & (rows["start"] >= cut - 140) & (rows["end"] > cut)]
            if (c, cut - 10) == cases.N_BLOCK_AT:
                assert len(over) == 0 and s[cut - 10:cut + 10] == b"N" * 20
                continue
            if c == cases.LONG_AT[0] and cases.LONG_AT[1] < cut < cases.LONG_AT[1] + 80_000:
                continue                                             # (the long run lies over this cut: asserted below)
            assert len(over) >= 1, (c, cut)
            crossing_k.update(over["k"].tolist())
            starting_k.update(rows[(rows["contig"] == c) & (rows["start"] < cut) & (rows["start"] >= cut - 140)]["k"].tolist())
    assert {12, 20, 50} <= crossing_k and set(cases.SHARE_KS) <= starting_k, (crossing_k, starting_k)
    long_rows = rows[rows["end"] - rows["start"] >= 65_535]
    assert as_tuples(long_rows) == [(cases.LONG_AT[0], cases.LONG_AT[1], cases.LONG_AT[1] + 80_000, 2)]
    assert len(rows) > 500
    # B: exactly one row per contig, of span L
    seqs, rows = cases.span_genome()
    assert as_tuples(rows) == [(c, 3, 3 + L, 1) for c, L in enumerate(cases.SPAN_LS)]
    # C: the planted runs are rows where they were planted; the widest motif the wire holds is a row
    seqs, rows = cases.field_genome()
    assert set((c, at, at + 24, 3) for c, at in cases.FIELD_PLANTS) <= set(as_tuples(rows))
    assert [at + 24 for c, at in cases.FIELD_PLANTS if at + 24 == len(seqs[c])] == [140_001, 131_072]
    assert 511 in cases.oracle_rows([cases.wide_motif(511)], (505, 511, 2, 9))["k"].tolist()
    assert 512 in cases.oracle_rows([cases.wide_motif(512)], (505, 512, 2, 9))["k"].tolist()
    # E, slabs: 6 000 rows, 2 048 in the densest tile -- above the default slab of 1 024 rows, far below the row array; the sizing
    # contig stays below both
    sizing, dense, rows = cases.slab_case()
    assert len(dense) == 192_000 and len(rows) == 6_000 and cases.max_rows_per_tile(rows) == 2_048
    sized = cases.oracle_rows([sizing], cases.OVF_SETTINGS)
    assert len(sizing) == 262_144 and cases.max_rows_per_tile(sized) < 1_024 and len(rows) < 262_144 // 32 + 65_536


def test_the_row_array_case_overflows_the_row_array_alone():
    """E, row array: 436 906 rows against a row array of positions / 32 + 65 536, in slabs that hold the densest tile."""
    slabs, sizing, dense, rows = cases.row_array_case()
    assert len(dense) == len(sizing) == 10_485_744
    assert len(rows) == 436_906 and cases.max_rows_per_tile(rows) == 2_731
    assert 436_906 > 10_485_744 // 32 + 65_536 == 393_215
    sized = cases.oracle_rows([slabs], cases.OVF_SETTINGS)
    assert len(slabs) == 196_608 and cases.max_rows_per_tile(sized) == 2_731       # the slabs grow to the dense contig's demand
    assert len(sized) <= 196_608 // 32 + 65_536
    # the contig that sizes the row array does not make the library grow it beyond positions / 32 + 65 536
    assert len(cases.oracle_rows([sizing], cases.OVF_SETTINGS)) < 393_215
