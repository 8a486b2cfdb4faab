"""The inputs of tests/test_pipelined_edges_gpu.py and their expected rows, built on the CPU: every expected row set comes from the
oracle (oracle.prf_oracle.detect_rows), none from the library.  tests/test_wire_format_cpu.py asserts what the cases are built
around (row counts, rows per tile, the rows at the wire format's field boundaries) without a GPU."""
import collections
import functools

import numpy as np

import multi_gpu
import synth
from oracle import prf_oracle

TILE = 65_536


def oracle_rows(seqs, settings):
    """The oracle's rows of every contig, as the library's row array (sorted by contig, start, end)."""
    per_contig = []
    for c, seq in enumerate(seqs):
        found = prf_oracle.detect_rows(bytes(seq), *settings)
        a = np.zeros(len(found), dtype=multi_gpu.ROW_DTYPE)
        if found:
            t = np.array(found, dtype=np.uint64)
            a["start"], a["end"], a["k"] = t[:, 0], t[:, 1], t[:, 3].astype(np.uint32)
        a["contig"] = c
        per_contig.append(a)
    rows = np.concatenate(per_contig) if per_contig else np.zeros(0, dtype=multi_gpu.ROW_DTYPE)
    return rows[np.lexsort((rows["k"], rows["end"], rows["start"], rows["contig"]))]


def rows_of_parts(rows, parts):
    """The rows that start inside `parts` ((contig, begin, end) ranges): a row belongs to the part that holds its first position."""
    keep = np.zeros(len(rows), dtype=bool)
    for c, b, e in parts:
        keep |= (rows["contig"] == c) & (rows["start"] >= b) & (rows["start"] < e)
    return rows[keep]


def max_rows_per_tile(rows):
    return max(collections.Counter((rows["start"] // np.uint64(TILE)).tolist()).values())


# ---- A: shares of one genome --------------------------------------------------------------------------------------------------
SHARE_LENS = [200_000, 65_536, 70_001, 131_072]
SHARE_HINT = 50
SHARE_SETTINGS = (1, 50, 3, 9)
SHARE_KS = (1, 3, 7, 12, 20, 50)
SHARE_WHOLE = (7, 50, 20, 12, 3)   # cut by cut in genome order (the first cut carries the N block, the last one the long run)
LONG_AT = (3, 20_000)          # contig, start of "GT" * 40_000: across the cut at 65 536 of the last contig
N_BLOCK_AT = (0, TILE - 10)    # contig, start of N * 20: on the first cut of the first contig


@functools.lru_cache(maxsize=None)
def share_genome():
    """-> (contigs, oracle rows).  Runs of every size in SHARE_KS start 1 to 140 positions before every tile cut (at one cut they
    overlap: the last one written is left whole, the others keep what lies in front of the next one's start -- enough for a row of
    the sizes 1, 3 and 7 -- and SHARE_WHOLE names the size written last at each cut in turn, so that the three largest are whole
    at the three free cuts); one run longer
    than a wire row's span field crosses a cut, and a block of N lies on another."""
    seqs = [bytearray(synth.standin2(n, 70 + i).tobytes()) for i, n in enumerate(SHARE_LENS)]
    rng = np.random.default_rng(37)
    turn = 0
    for s in seqs:
        for cut in range(TILE, len(s), TILE):
            last = SHARE_WHOLE[turn % len(SHARE_WHOLE)]
            turn += 1
            big = tuple(k for k in SHARE_KS if k > 7 and k != last)
            order = tuple(k for k in (1, 3, 7) if k != last) + big + (last,)
            backs = [int(rng.integers(1, 41))]                                      # of the last one, then towards the front
            for _ in big:
                backs.append(backs[0] + int(rng.integers(1, 31)))
            front = max(backs)
            for k in reversed(order[:len(order) - len(big) - 1]):
                front += max(3 * k, 9) + int(rng.integers(0, 5))                    # room for a row of this size in front of the next
                backs.append(front)
            assert front <= 140
            backs = backs[::-1]
            for k, back in zip(order, backs):
                motif = bytes(rng.choice(list(b"ACGT"), size=k).astype(np.uint8))
                body = motif * (300 // k + 4)
                at = cut - back
                body = body[:len(s) - at]
                s[at:at + len(body)] = body
                s[at - 1] = b"ACGT"[(b"ACGT".index(motif[-1]) + 1) % 4]     # the run starts where it is planted, not earlier
    c, at = LONG_AT
    seqs[c][at - 1:at + 80_001] = b"C" + b"GT" * 40_000 + b"C"
    c, at = N_BLOCK_AT
    seqs[c][at:at + 20] = b"N" * 20
    seqs = tuple(bytes(s) for s in seqs)
    return seqs, oracle_rows(seqs, SHARE_SETTINGS)


# ---- B: the span field's boundary -----------------------------------------------------------------------------------------------
SPAN_LS = (65_533, 65_534, 65_535, 65_536)
SPAN_SETTINGS = (1, 3, 3, 9)


@functools.lru_cache(maxsize=None)
def span_genome():
    seqs = tuple(b"CGT" + b"A" * L + b"CGT" for L in SPAN_LS)
    return seqs, oracle_rows(seqs, SPAN_SETTINGS)


# ---- C: the position field and the motif-size field -----------------------------------------------------------------------------
FIELD_LENS = [70_000, 140_001, 131_072]
FIELD_SETTINGS = (1, 50, 3, 9)
FIELD_PLANTS = [(1, 65_535), (1, 140_001 - 24), (2, 65_536), (2, 131_072 - 24)]     # contig, start of "ACG" * 8


@functools.lru_cache(maxsize=None)
def field_genome():
    seqs = [bytearray(synth.synth_bases(n, 90 + i).tobytes()) for i, n in enumerate(FIELD_LENS)]
    for c, at in FIELD_PLANTS:
        seqs[c][at - 1:at + 24] = b"T" + b"ACG" * 8        # (the T in front, and the one behind, end the run where it is planted)
        if at + 24 < len(seqs[c]):
            seqs[c][at + 24] = ord("T")
    seqs = tuple(bytes(s) for s in seqs)
    return seqs, oracle_rows(seqs, FIELD_SETTINGS)


def wide_motif(k, seed=77):
    return synth.synth_bases(k, seed).tobytes() * 3 + b"TTGACCA"


# ---- E: overflow behind the sizing scan -------------------------------------------------------------------------------------
OVF_SETTINGS = (1, 6, 3, 9)
SLAB_SIZING = (262_144, 5)         # synth.synth_bases(length, seed)
SLAB_DENSE_UNIT, SLAB_DENSE_N = b"ACACACACACAC" + b"GTTGCAGATCCGTAGCTAGG", 6000
ROWS_UNIT = b"ACACACACACAC" + b"GTTGCAGATCCG"
ROWS_SLAB_N, ROWS_DENSE_N = 8192, 436_906
ROWS_SIZING = (10_485_744, 6)


@functools.lru_cache(maxsize=None)
def slab_case():
    """-> (sizing contig, dense contig, the dense contig's oracle rows)"""
    dense = SLAB_DENSE_UNIT * SLAB_DENSE_N
    return synth.synth_bases(*SLAB_SIZING).tobytes(), dense, oracle_rows([dense], OVF_SETTINGS)


@functools.lru_cache(maxsize=None)
def row_array_case():
    """-> (contig that sizes the slabs, contig that sizes the row array, dense contig, the dense contig's oracle rows)"""
    dense = ROWS_UNIT * ROWS_DENSE_N
    return ROWS_UNIT * ROWS_SLAB_N, synth.synth_bases(*ROWS_SIZING).tobytes(), dense, oracle_rows([dense], OVF_SETTINGS)
