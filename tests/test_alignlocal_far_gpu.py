"""GPU (-m gpu): prf_motif_align_local on the contigs that hold the global positions 2^31 and 2^32 and on the one beyond (the genomes
and builders of tests/far_cases.py, unchanged; the fixtures of tests/test_far_positions_gpu.py).  Every result equals the model
(tests/alignlocal_model.py) and the same call on the genome of the three small contigs alone, byte for byte.

Shapes: a range of 2 600 positions whose position 1 307 (begin % 64 = 37) or 1 280 (begin % 64 = 0) is the boundary, with windows
that straddle it in every kernel (k = 7 and 33, the periods of the tandem repeats planted across it; 64 | 65; 171; 300; 600;
1 024), windows that end at it, begin at it and lie wholly behind it; the whole contig as one range with a window of 4 000
positions around the boundary; beyond, 3 000 positions of the last contig.  The motifs are the letters the sequence holds at the
window's start, every ninth changed, and for k = 7 the planted unit itself."""
import random

import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import align_model as A
import alignlocal_model as L
import far_cases as F
from test_far_positions_gpu import ctx, far_a, far_b, near_a, near_b  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EDGE = F.EDGE
KS = (1, 7, 33, 64, 65, 171, 300, 600, 1_024)


def _straddling(at):
    """Windows of a range whose position `at` is the boundary: per k one across it, one up to it, one from it on, and a few more."""
    rows = []
    for row, k in enumerate(KS):
        rows += [(at - 100, at + 100, k), (max(0, at - 150 - row), at, k), (at, at + 150 + row, k)]
    rows += [(at - 1, at + 1, 1), (at - 1, at + 1, 2), (at - 1, at + 1, 65), (0, F.SPAN, 7), (at, at + 700, 1_024), (at + 1, at + 65, 64),
             (at + 200, at + 900, 171), (at, at + 1, 1), (at - 70, at, 33)]
    return rows


# (name, near contig, begin, end, windows relative to begin, weights)
RANGES = [(f"{pin} begin%64={mod}", contig, EDGE - F.OFF[mod], EDGE - F.OFF[mod] + F.SPAN, _straddling(F.OFF[mod]), weights)
          for (pin, contig), weights in zip((("2^31", 0), ("2^32", 1)), ((2, 7, 7), (2, 3, 5))) for mod in (37, 0)]
RANGES += [(f"{pin} the whole contig", contig, 0, None, [(EDGE - 2_000, EDGE + 2_000, 7), (EDGE, EDGE + 500, 33), (EDGE - 500, EDGE, 171), (EDGE - 20, EDGE + 20, 600)],
            (2, 7, 7)) for pin, contig in (("2^31", 0), ("2^32", 1))]
RANGES += [("beyond begin%64=37", 2, 20_032 + 37, 23_032 + 37, [(0, 400, k) for k in KS] + [(2_450, 3_000, k) for k in KS] + [(5, 70, 64), (2_999, 3_000, 1)], (3, 1, 2)),
           ("beyond begin%64=0", 2, 9_984, 9_984 + 6_100, [(3_000 + 64 * at, 3_300 + 65 * at, k) for at, k in enumerate(KS)] +
            [(F.S1_AT - 9_984 + F.CENTRE - 110, F.S1_AT - 9_984 + F.CENTRE + 74, 7), (6_099, 6_100, 1)], (2, 7, 7))]


def _motifs(seq, begin, rows):
    rng = random.Random(251)
    out = []
    for start, _, k in rows:
        text = bytearray(seq[begin + start:begin + start + k].upper())
        text += bytes(rng.choice(b"ACGT") for _ in range(k - len(text)))
        for j in range(0, k, 9):
            text[j] = rng.choice(b"ACGT")
        out.append("ACGGTCA" if k == 7 else bytes(b if b in b"ACGT" else ord("N") for b in text).decode())
    return out


def _check(far, near, seqs, case):
    name, contig, begin, end, rows, weights = case
    table = A.repeats(*rows)
    motifs = _motifs(seqs[contig], begin, rows)
    want = L.local(seqs[contig], table, motifs, weights, begin, end)
    got_far = far.motif_align_local(F.FAR_OF[contig], begin, end, table, motifs, *weights)
    got_near = near.motif_align_local(contig, begin, end, table, motifs, *weights)
    assert got_far.dtype == np.dtype(L.DTYPE)
    assert L.same(got_far, want), (name, "far genome against the model", np.flatnonzero(got_far != want)[:5])
    assert L.same(got_near, want), (name, "near genome against the model")
    assert got_far.tobytes() == got_near.tobytes(), (name, "far genome against the near one")
    assert int((want["score"] > 0).sum()) > len(rows) // 2, name            # not a range of nothing but N


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_motif_align_local_on_the_generated_genome(far_a, near_a, case):  # noqa: F811
    _check(far_a, near_a, F.near_contigs("A"), case)


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_motif_align_local_on_the_loaded_genome(far_b, near_b, case):  # noqa: F811
    _check(far_b, near_b, F.near_contigs("B"), case)
    name, contig, begin, end, rows, weights = case
    if name.startswith("2^31 begin"):         # the perfect repeat of period 7 planted across the boundary: 84 positions, found in a wider window
        at = F.OFF[int(name[-2:].lstrip("="))]
        got = far_b.motif_align_local(F.FAR_OF[contig], begin, end, A.repeats((at - 110, at + 74, 7)), ["ACGGTCA"])
        assert got[0]["score"] >= 2 * 84 and got[0]["first"] <= 50 and got[0]["end"] >= 134
