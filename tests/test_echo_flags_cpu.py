"""CPU: the sampled primitive-motif test of the exact tasks (tests/echo_flags_model.py) against the test at the run's start.

The kernel decides "echo of a shorter motif" once per segment of S start rows, at the segment's last row, instead of at every
start.  That is exact if the sampled row lies inside the start's run and a segment holds at most one start; here the two
verdicts are compared for every start of low-entropy sequences -- short periodic pieces over 2-4 letters, where echoes, primitive
runs and their neighbourhoods are as dense as they get -- for every (K <= 4, M <= 8) that the settings of
tests/test_echo_flags_gpu.py reach, and for the larger K of the general statement."""
import numpy as np
import pytest

import echo_flags_model as model

SETTINGS = ((3, 9), (2, 9), (2, 4), (4, 12), (5, 9))      # (min_repeats, min_span); the first three are the GPU file's
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def low_entropy(seed, length=100_000):
    """Periodic pieces: a motif of 1-6 letters over an alphabet of 2-4, repeated for 2-40 positions, one after the other."""
    rng = np.random.RandomState(seed)
    letters = BASES[rng.permutation(4)[:2 + seed % 3]]
    out, n = [], 0
    while n < length:
        motif = letters[rng.randint(0, len(letters), rng.randint(1, 7))]
        ln = rng.randint(2, 41)
        out.append(np.tile(motif, ln // len(motif) + 1)[:ln])
        n += ln
    return np.concatenate(out)[:length]


@pytest.fixture(scope="module")
def sequences():
    return [low_entropy(seed) for seed in range(6)]


def test_segment_lengths():
    assert [model.segment(M) for M in range(2, 10)] == [2, 4, 4, 4, 4, 8, 8, 8]
    assert (model.segment(7), model.segment(6), model.segment(8)) == (8, 4, 8)      # the default (K, M) = (2,7), (3,6), (4,8)
    assert all(model.segment(M) <= M + 1 and T_is_multiple(model.segment(M)) for M in range(1, 15))
    assert [model.cofactors(k) for k in (1, 2, 3, 4, 6, 8)] == [[], [1], [1], [2], [3, 2], [4]]


def T_is_multiple(s):
    return model.T % s == 0


@pytest.mark.parametrize("r,span", SETTINGS)
def test_sampled_verdict_is_the_verdict_at_the_start(sequences, r, span):
    n_starts = n_echo = 0
    for a in sequences:
        for k in range(2, 9):
            M = model.min_matches(k, r, span)
            if M >= model.SMALL_M:
                continue
            t, at_start, sampled = model.verdicts(a, k, M)
            # the premises: the sample lies inside the run's rows t .. t+M, and two starts are more than a segment apart
            S = model.segment(M)
            assert S <= M + 1 and (len(t) < 2 or int(np.diff(t).min()) >= M + 1 >= S)
            bad = np.flatnonzero(at_start != sampled)
            assert len(bad) == 0, (k, M, t[bad][:5])
            n_starts += len(t)
            n_echo += int(at_start.sum())
    print("settings", (r, span), "starts", n_starts, "of them echoes", n_echo)
    assert n_starts > 10_000 and n_echo > 1_000 and n_starts - n_echo > 1_000


def test_echo_is_what_the_oracle_drops(sequences):
    """The verdict at the start is the reference's own: the runs it reports at size k are the primitive starts that are long enough."""
    from oracle import prf_oracle
    a = sequences[0][:20_000]
    rows = prf_oracle.detect_rows(a.tobytes(), 2, 4, 3, 9)
    for k in (2, 3, 4):
        M = model.min_matches(k, 3, 9)
        t, at_start, _ = model.verdicts(a, k, M)
        assert sorted(s for s, _e, _ml, kk in rows if kk == k) == [int(x) for x in t[~at_start]]


def test_stream_counts_tell_echoes_from_primitive_runs():
    rng = np.random.RandomState(5)
    a = BASES[rng.randint(0, 4, 2 * model.TILE)].copy()
    for i in range(50):
        p = 1_000 + 1_200 * i
        a[p:p + 12] = a[p]
        a[p - 1] = a[p + 12] = BASES[(int(np.where(BASES == a[p])[0][0]) + 1) % 4]
    seen, prim, flagged = model.count_flags(a, 0, (2, 4, 3, 9))
    print("streams with a start", seen, "with a primitive start", prim, "flagged by the sampled rule", flagged)
    assert seen >= prim + 150 and prim <= flagged <= prim + 3
