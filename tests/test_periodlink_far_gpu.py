"""GPU (-m gpu): prf_period_links on the contigs that hold the global positions 2^31 and 2^32 and on the one beyond (the genomes
and builders of tests/far_cases.py, unchanged; the fixtures of tests/test_far_positions_gpu.py).  Every list equals the model
(tests/periodlink_model.py) and the same call on the genome of the three small contigs alone.

Shapes: ranges of 192 to 230 positions across the boundary at (3, 2, 4), where every chance run of three cells is a seed, with a
begin on a word of the planes and one 37 bits into a word; beyond, 3 000 positions around the tandem repeat of period 7 with its
inserted pair of bases at (12, 8, 4): the images at 14 and 21 make their detours on lines 16 and 23."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import far_cases as F
import periodlink_model as L
from test_far_positions_gpu import ctx, far_a, far_b, near_a, near_b  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EDGE = F.EDGE
# (name, near contig, begin, end, (kmin, kmax), (min_seed, max_gap, max_shift), the least links)
RANGES = [("2^31 begin%64=37", 0, EDGE - 91, EDGE + 101, (1, 192), (3, 2, 4), 5),
          ("2^31 begin%64=0", 0, EDGE - 128, EDGE + 101, (1, 60), (3, 2, 4), 5),
          ("2^32 begin%64=37", 1, EDGE - 91, EDGE + 101, (1, 192), (3, 2, 4), 5),
          ("2^32 begin%64=0", 1, EDGE - 128, EDGE + 101, (5, 229), (3, 2, 4), 5),
          ("beyond begin%64=37", 2, 20_032 + 37, 20_224 + 37, (1, 192), (3, 2, 4), 5),
          ("beyond begin%64=0", 2, 20_032, 20_224, (1, 192), (3, 2, 32), 5)]
INDEL_AT = F.S1_INDEL_AT + F.CENTRE                           # genome B, beyond: the repeat of period 7 with two bases inserted
B_RANGES = RANGES + [("beyond, the repeat with an insertion begin%64=37", 2, INDEL_AT - 1_500 + 37 - (INDEL_AT - 1_500) % 64, INDEL_AT + 1_500,
                      (1, 40), (12, 8, 4), 2)]


def _check(far, near, seqs, case):
    name, contig, begin, end, (kmin, kmax), triple, least = case
    for nm in (False, True):
        want = L.links(seqs[contig], kmin, kmax, *triple, n_matches=nm, begin=begin, end=end, sparse=triple[0] >= 10)
        got_far = far.period_links(F.FAR_OF[contig], begin, end, kmin, kmax, *triple, n_matches=nm)
        got_near = near.period_links(contig, begin, end, kmin, kmax, *triple, n_matches=nm)
        assert L.same(got_far, want), (name, nm, "far genome against the model")
        assert L.same(got_far, got_near) and got_far.dtype == got_near.dtype, (name, nm, "far genome against the near one")
        assert len(want) >= least, (name, nm, len(want))
        half = (end - begin) // 2                               # two windows add up on the far genome too
        parts = [far.period_links(F.FAR_OF[contig], begin, end, kmin, kmax, *triple, n_matches=nm, positions=w) for w in ((0, half), (half, None))]
        assert L.same(np.sort(np.concatenate(parts), order=["start", "k"]), want), (name, nm, "windows")


@pytest.mark.parametrize("case", RANGES, ids=[c[0] for c in RANGES])
def test_links_on_the_generated_genome(far_a, near_a, case):  # noqa: F811
    _check(far_a, near_a, F.near_contigs("A"), case)


@pytest.mark.parametrize("case", B_RANGES, ids=[c[0] for c in B_RANGES])
def test_links_on_the_loaded_genome(far_b, near_b, case):  # noqa: F811
    _check(far_b, near_b, F.near_contigs("B"), case)
    if case[5] == (12, 8, 4):                                   # out to the detours of the images at 14 and 21; behind the insertion
        # the repeat has 24 bases left: 10 cells of line 14, no seed, so no link leads back
        name, contig, begin, end, (kmin, kmax), triple, _least = case
        got = far_b.period_links(F.FAR_OF[contig], begin, end, kmin, kmax, *triple)
        assert {(16, 2), (23, 2)} <= {(int(r["k"]), int(r["shift"])) for r in got}
