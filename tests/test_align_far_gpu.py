"""GPU (-m gpu): prf_motif_align on the contigs that hold the global positions 2^31 and 2^32 and on the one beyond (the genomes and
builders of tests/far_cases.py, unchanged; the fixtures of tests/test_far_positions_gpu.py).  Every result equals the model
(tests/align_model.py) and the same call on the genome of the three small contigs alone, byte for byte.

Shapes: a range of 2 600 positions whose position 1 307 (begin % 64 = 37) or 1 280 (begin % 64 = 0) is the boundary, with rows that
straddle it in every kernel (k = 7 and 33, the periods of the tandem repeats planted across it; 64 | 65; 171; 300; 600; 1 024),
rows that end at it, begin at it and lie wholly behind it; the whole contig as one range with a row of 12 000 positions around
the boundary; beyond, 3 000 and 6 100 positions of the last contig.  The motifs are the letters the sequence holds at the row's
start, every ninth changed, and for k = 7 the planted unit itself."""
import random

import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import align_model as A
import far_cases as F
from test_far_positions_gpu import ctx, far_a, far_b, near_a, near_b  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EDGE = F.EDGE
KS = (1, 7, 33, 64, 65, 171, 300, 600, 1_024)


def _straddling(at):
    """Rows of a range whose position `at` is the boundary: per k one across it, one up to it, one from it on, and a few more."""
    rows = []
    for row, k in enumerate(KS):
        rows += [(at - 100, at + 100, k), (max(0, at - 300 - row), at, k), (at, at + 300 + row, k)]
    rows += [(at - 1, at + 1, 1), (at - 1, at + 1, 2), (at - 1, at + 1, 65), (0, F.SPAN, 7), (at, F.SPAN, 1_024), (at + 1, at + 65, 64),
             (at + 200, F.SPAN, 171), (at, at + 1, 1), (at - 70, at, 33)]
    return rows


# (name, near contig, begin, end, rows relative to begin)
RANGES = [(f"{pin} begin%64={mod}", contig, EDGE - F.OFF[mod], EDGE - F.OFF[mod] + F.SPAN, _straddling(F.OFF[mod]))
          for pin, contig in (("2^31", 0), ("2^32", 1)) for mod in (37, 0)]
RANGES += [(f"{pin} the whole contig", contig, 0, None, [(EDGE - 6_000, EDGE + 6_000, 7), (EDGE, EDGE + 500, 33), (EDGE - 500, EDGE, 171), (EDGE - 20, EDGE + 20, 600)])
           for pin, contig in (("2^31", 0), ("2^32", 1))]
RANGES += [("beyond begin%64=37", 2, 20_032 + 37, 23_032 + 37, [(0, 1_400, k) for k in KS] + [(1_450, 3_000, k) for k in KS] + [(5, 70, 64), (2_999, 3_000, 1)]),
           ("beyond begin%64=0", 2, 9_984, 9_984 + 6_100, [(0, 6_100, k) for k in KS] + [(F.S1_AT - 9_984 + F.CENTRE - 60, F.S1_AT - 9_984 + F.CENTRE + 24, 7)])]


def _motifs(seq, begin, rows):
    rng = random.Random(221)
    out = []
    for start, _, k in rows:
        text = bytearray(seq[begin + start:begin + start + k].upper())
        text += bytes(rng.choice(b"ACGT") for _ in range(k - len(text)))
        for j in range(0, k, 9):
            text[j] = rng.choice(b"ACGT")
        out.append("ACGGTCA" if k == 7 else bytes(b if b in b"ACGT" else ord("N") for b in text).decode())
    return out


def _check(far, near, seqs, case):
    name, contig, begin, end, rows = case
    table = A.repeats(*rows)
    motifs = _motifs(seqs[contig], begin, rows)
    want = A.align(seqs[contig], table, motifs, begin, end)
    got_far = far.motif_align(F.FAR_OF[contig], begin, end, table, motifs)
    got_near = near.motif_align(contig, begin, end, table, motifs)
    assert got_far.dtype == np.dtype(A.DTYPE)
    assert A.same(got_far, want), (name, "far genome against the model", np.flatnonzero(got_far != want)[:5])
    assert A.same(got_near, want), (name, "near genome against the model")
    assert got_far.tobytes() == got_near.tobytes(), (name, "far genome against the near one")
    lengths = np.array([b - a for a, b, _ in rows])
    assert int((want["edits"] < lengths).sum()) > len(rows) // 2, name      # not a range of nothing but N


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_motif_align_on_the_generated_genome(far_a, near_a, case):  # noqa: F811
    _check(far_a, near_a, F.near_contigs("A"), case)


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_motif_align_on_the_loaded_genome(far_b, near_b, case):  # noqa: F811
    _check(far_b, near_b, F.near_contigs("B"), case)
    name, contig, begin, end, rows = case
    if name.startswith("2^31 begin"):         # the perfect repeat of period 7 planted across the boundary: 84 positions, no edit
        at = F.OFF[int(name[-2:].lstrip("="))]
        got = far_b.motif_align(F.FAR_OF[contig], begin, end, A.repeats((at - 60, at + 24, 7)), ["ACGGTCA"])
        assert got[0].tolist() == (0, 0, 84, 0, 6, 0)
