"""GPU (-m gpu): prf_phased_consensus on the contigs that hold the global positions 2^31 and 2^32 and on the one beyond (the genomes
and builders of tests/far_cases.py, unchanged; the fixtures of tests/test_far_positions_gpu.py).  Every result -- rows, letters,
counts -- equals the model (tests/phased_model.py) and the same call on the genome of the three small contigs alone.

Shapes: a range of 2 600 positions whose position 1 307 (begin % 64 = 37) or 1 280 (begin % 64 = 0) is the boundary, with segments
that straddle it in every regime (k = 7 and 33, the periods of the tandem repeats planted across it; 64 | 65; 171; 1 024 | 1 025),
segments that end at it, begin at it and lie wholly behind it, two and three to a row at the phases 0, 1 and k - 1; the whole
contig as one range with a segment of 12 000 positions around the boundary, cut into three work items; beyond, 3 000 and 6 100
positions of the last contig.  Every call is repeated at slice_positions = 100, so that the boundary falls inside an item and
between two."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import far_cases as F
import phased_model as M
from test_far_positions_gpu import ctx, far_a, far_b, near_a, near_b  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EDGE = F.EDGE
KS = (1, 7, 33, 64, 65, 171, 1_024, 1_025)


def _straddling(at):
    """(ks, segments) of a range whose position `at` is the boundary: row r < 8 has KS[r] columns and three segments -- across the
    boundary, up to it, from it on -- and the rows behind them one segment each."""
    ks, segs = list(KS), []
    for row, k in enumerate(KS):
        segs += [(at - 100, at + 100, row, k - 1), (max(0, at - 300 - row), at, row, 1 % k), (at, at + 300 + row, row, 0)]
    for k, (a, b, phase) in ((1, (at - 1, at + 1, 0)), (2, (at - 1, at + 1, 1)), (65, (at - 1, at + 1, 64)), (7, (0, F.SPAN, 3)), (1_025, (at, F.SPAN, 1_024)),
                             (64, (at + 1, at + 65, 63)), (171, (at + 200, F.SPAN, 1)), (1, (at, at + 1, 0)), (33, (at - 70, at, 32))):
        segs.append((a, b, len(ks), phase))
        ks.append(k)
    return ks, segs


def _around(k):
    return [(EDGE - 6_000, EDGE + 6_000, 0, k - 1), (EDGE, EDGE + 500, 1, 1), (EDGE - 500, EDGE, 1, 32), (EDGE - 20, EDGE + 20, 1, 0)]


# (name, near contig, begin, end, ks, segments relative to begin)
RANGES = [(f"{pin} begin%64={mod}", contig, EDGE - F.OFF[mod], EDGE - F.OFF[mod] + F.SPAN, *_straddling(F.OFF[mod]))
          for pin, contig in (("2^31", 0), ("2^32", 1)) for mod in (37, 0)]
RANGES += [(f"{pin} the whole contig k={k}", contig, 0, None, [k, 33], _around(k)) for pin, contig in (("2^31", 0), ("2^32", 1)) for k in (7, 171, 1_025)]
RANGES += [("beyond begin%64=37", 2, 20_032 + 37, 23_032 + 37, list(KS), [(0, 1_400, row, k - 1) for row, k in enumerate(KS)] +
            [(1_450, 3_000, row, 1 % k) for row, k in enumerate(KS)] + [(5, 70, 3, 0), (2_999, 3_000, 0, 0)]),
           ("beyond begin%64=0", 2, 9_984, 9_984 + 6_100, list(KS), [(0, 6_100, row, k // 2) for row, k in enumerate(KS)] +
            [(F.S1_AT - 9_984 + F.CENTRE - 60, F.S1_AT - 9_984 + F.CENTRE + 24, 1, 0)])]


def _check(far, near, seqs, case):
    name, contig, begin, end, ks, segs = case
    table = M.segments(*segs)
    want = M.consensus(seqs[contig], ks, table, begin, end)
    got_far = far.phased_consensus(F.FAR_OF[contig], begin, end, ks, table, counts=True)
    got_near = near.phased_consensus(contig, begin, end, ks, table, counts=True)
    for got, what in ((got_far, "far genome against the model"), (got_near, "near genome against the model")):
        assert M.same(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2]), (name, what)
    assert got_far[0].tobytes() == got_near[0].tobytes() and got_far[2].tobytes() == got_near[2].tobytes(), (name, "far genome against the near one")
    assert int(want[0]["acgt"].sum()) > 1_000, name                           # not a range of nothing but N
    sliced = far.phased_consensus(F.FAR_OF[contig], begin, end, ks, table, counts=True, slice_positions=100)
    assert sliced[0].tobytes() == got_far[0].tobytes() and sliced[1] == got_far[1] and sliced[2].tobytes() == got_far[2].tobytes(), (name, "slices")


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_phased_consensus_on_the_generated_genome(far_a, near_a, case):  # noqa: F811
    _check(far_a, near_a, F.near_contigs("A"), case)


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_phased_consensus_on_the_loaded_genome(far_b, near_b, case):  # noqa: F811
    _check(far_b, near_b, F.near_contigs("B"), case)
    name, contig, begin, end, ks, segs = case
    if name.startswith("2^31 begin"):         # the perfect repeat of period 7 planted across the boundary names itself, in two segments
        at = F.OFF[int(name[-2:].lstrip("="))]
        got, motifs = far_b.phased_consensus(F.FAR_OF[contig], begin, end, [7], M.segments((at, at + 24, 0, 60 % 7), (at - 60, at, 0, 0)))
        assert motifs == ["ACGGTCA"] and got["agree"][0] == 84
