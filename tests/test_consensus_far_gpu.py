"""GPU (-m gpu): prf_period_consensus on the contigs that hold the global positions 2^31 and 2^32 and on the one beyond (the genomes
and builders of tests/far_cases.py, unchanged; the fixtures of tests/test_far_positions_gpu.py).  Every result -- rows, letters,
counts -- equals the model (tests/consensus_model.py) and the same call on the genome of the three small contigs alone.

Shapes: a range of 2 600 positions whose position 1 307 (begin % 64 = 37) or 1 280 (begin % 64 = 0) is the boundary, with rows
that straddle it in every regime (k = 7 and 33, the periods of the tandem repeats planted across it; 64 | 65; 171; 1 024 | 1 025),
rows that end at it, begin at it and lie wholly behind it; the whole contig as one range with a row of 12 000 positions around the
boundary, cut into three work items; beyond, 3 000 and 6 100 positions of the last contig (the second around its perfect repeat
of period 7).  Every call is repeated at slice_positions = 100, so that the boundary falls inside an item and between two."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import consensus_model as M
import far_cases as F
from test_far_positions_gpu import ctx, far_a, far_b, near_a, near_b  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EDGE = F.EDGE
KS = (1, 7, 33, 64, 65, 171, 1_024, 1_025)


def _straddling(at):
    """Rows of a range whose position `at` is the boundary: across it, up to it, from it on, behind it."""
    rows = [(0, F.SPAN, k) for k in KS] + [(at - 100, at + 100, k) for k in KS] + [(at - 1, at + 1, k) for k in (1, 2, 65)]
    rows += [(at - 300, at, 7), (at - 70, at, 65), (at, at + 300, 7), (at, at + 1, 1), (at, F.SPAN, 1_025), (at + 1, at + 65, 64), (at + 200, F.SPAN, 171)]
    return rows


# (name, near contig, begin, end, rows relative to begin)
RANGES = [(f"{pin} begin%64={mod}", contig, EDGE - F.OFF[mod], EDGE - F.OFF[mod] + F.SPAN, _straddling(F.OFF[mod]))
          for pin, contig in (("2^31", 0), ("2^32", 1)) for mod in (37, 0)]
RANGES += [(f"{pin} the whole contig", contig, 0, None, [(EDGE - 6_000, EDGE + 6_000, k) for k in (7, 171, 1_025)] + [(EDGE, EDGE + 500, 33), (EDGE - 500, EDGE, 33)])
           for pin, contig in (("2^31", 0), ("2^32", 1))]
RANGES += [("beyond begin%64=37", 2, 20_032 + 37, 23_032 + 37, [(0, 3_000, k) for k in KS] + [(5, 70, 64), (2_999, 3_000, 1)]),
           ("beyond begin%64=0", 2, 9_984, 9_984 + 6_100, [(0, 6_100, k) for k in KS] + [(F.S1_AT - 9_984 + F.CENTRE - 60, F.S1_AT - 9_984 + F.CENTRE + 24, 7)])]


def _check(far, near, seqs, case):
    name, contig, begin, end, rows = case
    table = M.repeats(*rows)
    want = M.consensus(seqs[contig], table, begin, end)
    got_far = far.period_consensus(F.FAR_OF[contig], begin, end, table, counts=True)
    got_near = near.period_consensus(contig, begin, end, table, counts=True)
    for got, what in ((got_far, "far genome against the model"), (got_near, "near genome against the model")):
        assert M.same(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2]), (name, what)
    assert got_far[0].tobytes() == got_near[0].tobytes() and got_far[2].tobytes() == got_near[2].tobytes(), (name, "far genome against the near one")
    assert int(want[0]["acgt"].sum()) > 1_000, name                           # not a range of nothing but N
    sliced = far.period_consensus(F.FAR_OF[contig], begin, end, table, counts=True, slice_positions=100)
    assert sliced[0].tobytes() == got_far[0].tobytes() and sliced[1] == got_far[1] and sliced[2].tobytes() == got_far[2].tobytes(), (name, "slices")


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_consensus_on_the_generated_genome(far_a, near_a, case):  # noqa: F811
    _check(far_a, near_a, F.near_contigs("A"), case)


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_consensus_on_the_loaded_genome(far_b, near_b, case):  # noqa: F811
    _check(far_b, near_b, F.near_contigs("B"), case)
    name, contig, begin, end, rows = case
    if name.startswith("2^31 begin"):                             # the perfect repeat of period 7 planted across the boundary names itself
        at = F.OFF[int(name[-2:].lstrip("="))]
        got, motifs = far_b.period_consensus(F.FAR_OF[contig], begin, end, M.repeats((at - 60, at + 24, 7)))
        assert motifs == ["ACGGTCA"] and got["agree"][0] == 84
