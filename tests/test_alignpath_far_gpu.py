"""GPU (-m gpu): prf_motif_align_path on the contigs that hold the global positions 2^31 and 2^32 and on the one beyond (the genomes
and builders of tests/far_cases.py, unchanged; the fixtures of tests/test_far_positions_gpu.py; the ranges, rows and motifs of
tests/test_align_far_gpu.py).  Rows, paths and counts equal the model (tests/alignpath_model.py) and the same call on the genome of
the three small contigs alone: far == near == model."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import align_model as A
import alignpath_model as P
import far_cases as F
from test_align_far_gpu import RANGES, _motifs
from test_far_positions_gpu import ctx, far_a, far_b, near_a, near_b  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _equal(got, want):
    return (A.same(got[0], want[0]) and np.array_equal(np.concatenate(got[1]), np.concatenate(want[1]) if isinstance(want[1], list) else want[1])
            and np.array_equal(got[2], want[2]))


def _check(far, near, seqs, case):
    name, contig, begin, end, rows = case
    table = A.repeats(*rows)
    motifs = _motifs(seqs[contig], begin, rows)
    want = P.align_path(seqs[contig], table, motifs, begin, end)
    got_far = far.motif_align_path(F.FAR_OF[contig], begin, end, table, motifs, with_counts=True)
    got_near = near.motif_align_path(contig, begin, end, table, motifs, with_counts=True)
    assert got_far[0].dtype == np.dtype(A.DTYPE) and got_far[1][0].dtype == np.uint16 and got_far[2].dtype == np.uint32
    assert _equal(got_far, want), (name, "far genome against the model")
    assert _equal(got_near, want), (name, "near genome against the model")
    assert _equal(got_far, got_near), (name, "far genome against the near one")
    assert got_far[0].tobytes() == far.motif_align(F.FAR_OF[contig], begin, end, table, motifs).tobytes(), name
    assert int((want[1] & P.SUB == 0).sum()) > len(want[1]) // 2, name        # not a range of nothing but N
    # the trace dealt into batches, on the far genome: the same
    assert _equal(far.motif_align_path(F.FAR_OF[contig], begin, end, table, motifs, with_counts=True, trace_bytes=1 << 16), want), (name, "batches")


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_motif_align_path_on_the_generated_genome(far_a, near_a, case):  # noqa: F811
    _check(far_a, near_a, F.near_contigs("A"), case)


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_motif_align_path_on_the_loaded_genome(far_b, near_b, case):  # noqa: F811
    _check(far_b, near_b, F.near_contigs("B"), case)
    name, contig, begin, end, rows = case
    if name.startswith("2^31 begin"):         # the perfect repeat of period 7 planted across the boundary: 84 positions, no edit
        at = F.OFF[int(name[-2:].lstrip("="))]
        rows_, paths = far_b.motif_align_path(F.FAR_OF[contig], begin, end, A.repeats((at - 60, at + 24, 7)), ["ACGGTCA"])
        assert rows_[0].tolist() == (0, 0, 84, 0, 6, 0) and np.array_equal(paths[0], P.perfect("ACGGTCA", 0, 84))
