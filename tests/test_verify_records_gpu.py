"""GPU (-m gpu): the record pass of the fused kernel's verification (csrc/vscan_verify.h: stage A lists the flagged streams of the
group-task records, stage B takes one stream per thread, finds its leaders and verifies each with its looks fetched in one batch).

Every case is a sequence of 3 tiles (196 608 bp) plus a guard of 64 bp, scanned with motif 1-50, min_repeats 3, min_span 9 and
compared row for row with the generic path and with the CPU oracle.  The oracle's row counts per motif size are pinned (taken from
the oracle on the CPU, where every case was first checked to hold the candidates it is meant to hold), so that a case which stops
exercising its path fails; the rows a case is built around are asserted by position as well."""
import collections

import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

pytestmark = pytest.mark.gpu

TILE = 65_536
N_SEQ = 3 * TILE + 64
SETTINGS = (1, 50, 3, 9)
LEAD_CAP = 192           # csrc/vscan_verify.h: flagged streams of one record wave's list
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def background(seed):
    return BASES[np.random.RandomState(seed).randint(0, 4, N_SEQ)].copy()


def primitive_motif(rng, k):
    while True:
        m = BASES[rng.randint(0, 4, k)]
        if all(k % d or not np.array_equal(m, np.tile(m[:d], k // d)) for d in range(1, k)):
            return m


def other_base(b):
    return BASES[(int(np.where(BASES == b)[0][0]) + 1) % 4]


def plant(seq, pos, motif, length):
    """seq[pos : pos+length] = copies of the motif, cut at `length`; the bases on either side break the period.
    Returns the row (start, end, k) this gives when it is long enough."""
    k = len(motif)
    seq[pos:pos + length] = np.tile(motif, length // k + 1)[:length]
    seq[pos - 1] = other_base(seq[pos - 1 + k])
    seq[pos + length] = other_base(seq[pos + length - k])
    return (pos, pos + length, k)


def case_echoes():
    """(a) runs of motif sizes 1-7, 40-400 bp: every multiple k >= 8 of the motif size gives a record that the primitive-motif test
    must reject -- k = 30 and 42 with three distinct primes, k = 46, 47, 49 with a period test longer than 32 positions (motif 1 at
    k = 47: 46 positions) -- beside primitive motifs of 30, 42 and 47 bp that it must keep (no k <= 50 has four primes)."""
    rng = np.random.RandomState(101)
    seq, want, pos = background(1), [], TILE + 1_000
    for m in range(1, 8):
        for length in (40, 97, 160, 400):
            want.append(plant(seq, pos, primitive_motif(rng, m), length))
            pos += 1_511
    for k, length in ((30, 125), (42, 150), (47, 141)):
        want.append(plant(seq, pos, primitive_motif(rng, k), length))
        pos += 1_511
    assert pos < 2 * TILE
    return [seq], want


def case_word_bits():
    """(b) the same motif 2 048 positions apart: one lane, several stream bits of one record word -- k = 9 (a group task of 4
    sizes, 8-11) and k = 24 (one of 8 sizes, 20-27)."""
    rng = np.random.RandomState(102)
    seq, want = background(2), []
    m9, m24 = primitive_motif(rng, 9), primitive_motif(rng, 24)
    for i in range(6):
        want.append(plant(seq, TILE + 4_100 + 2_048 * i, m9, 40))
        want.append(plant(seq, TILE + 21_300 + 2_048 * i, m24, 100))
    return [seq], want


def case_two_leaders():
    """(c) k = 8 (every group examined): 16 matches, one substituted base, 16 matches more -- the first run's leader is group g of
    its stream, the second run's three groups on (g = 0: both in one stream); and two phases of the motif that abut, whose leaders
    are two groups apart ((0, 2) and (1, 3))."""
    rng = np.random.RandomState(103)
    seq, want = background(3), []
    for g in range(4):
        s = TILE + 3_200 * (g + 1) + 8 * g          # (s - 8 g) is the first position of a stream
        w = primitive_motif(rng, 8)
        plant(seq, s - 7, w, 49)                    # matches at k = 8: s - 7 .. s + 33
        seq[s + 17] = other_base(seq[s + 17])       # mismatches at s + 9 and s + 17
        want += [(s - 7, s + 17, 8), (s + 18, s + 42, 8)]
    for g in range(2):
        s = TILE + 20_000 + 3_200 * g + 8 * g
        w = primitive_motif(rng, 8)
        plant(seq, s - 7, w, 23)                    # matches s - 7 .. s + 7 at least: a leader in group g
        w2 = primitive_motif(rng, 8)
        w2[7] = other_base(seq[s + 15])             # s + 15 differs from s + 23: the second run starts at s + 16, its leader is
        w2[0] = other_base(w2[7])                   # group g + 2 with nothing in front of it
        seq[s + 16:s + 40] = np.tile(w2, 3)
        seq[s + 40] = other_base(seq[s + 32])
        want.append((s + 16, s + 40, 8))
    return [seq], want


def case_run_ends():
    """(d) run ends at every depth: inside stage A's look, inside the look behind it, found by the walk, and past the window (3 kb:
    deferred, also by the next tile, whose first stream it covers); a homopolymer across a tile boundary gives the next tile
    a deferred candidate for every motif size >= 8: more than the list of 16 holds -> the tile is verified by the general routine."""
    rng = np.random.RandomState(104)
    seq, want, pos = background(4), [], 9_000
    for k in (10, 25):
        for length in (3 * k + 2, 3 * k + 40, 3 * k + 75, 300, 777):
            want.append(plant(seq, pos, primitive_motif(rng, k), length))
            pos += 2_111
    want.append(plant(seq, TILE - 500, primitive_motif(rng, 10), 3_000))
    want.append(plant(seq, 2 * TILE - 100, primitive_motif(rng, 1), 3_000))
    return [seq], want


def case_starts():
    """(e) starts in the last 31 positions of a tile for every stride (k = 9: each group, 14: every 2nd, 22: every 4th) -- the
    boundary items -- and in the first stream of a clean tile (the first tile of a contig and a later one).  Two contigs."""
    rng = np.random.RandomState(105)
    seqs = [background(5), background(6)]
    want = [(0,) + plant(seqs[0], TILE - 3, primitive_motif(rng, 9), 36),
            (0,) + plant(seqs[0], 2 * TILE - 15, primitive_motif(rng, 14), 56),
            (0,) + plant(seqs[0], 7, primitive_motif(rng, 12), 50),
            (1,) + plant(seqs[1], TILE - 31, primitive_motif(rng, 22), 88),
            (1,) + plant(seqs[1], 2 * TILE + 5, primitive_motif(rng, 12), 50)]
    return seqs, want


def case_mixed():
    """(f) N blocks inside and beside runs: the not-ACGT plane feeds stage A's and stage B's looks."""
    rng = np.random.RandomState(106)
    seq, want, pos = background(7), [], TILE + 2_000
    n = np.frombuffer(b"N", dtype=np.uint8)[0]
    for k in (3, 10, 16, 30, 47):
        for length in (4 * k + 5, 300):
            a, b, _ = plant(seq, pos, primitive_motif(rng, k), length)
            seq[a - 4:a - 1] = n                    # beside the run, in front
            want.append((a, b, k))
            a, b, _ = plant(seq, pos + 700, primitive_motif(rng, k), length)
            seq[b + 1:b + 9] = n                    # behind it
            want.append((a, b, k))
            a, b, _ = plant(seq, pos + 1_400, primitive_motif(rng, k), 2 * length + 20)
            seq[a + length:a + length + 20] = n     # inside: two runs
            want += [(a, a + length, k), (a + length + 20, b, k)]
            pos += 2_203
    seq[2 * TILE + 100:2 * TILE + 5_000] = n
    return [seq], want


def case_overflow():
    """(g) more flagged streams with a leader in a tile than the record waves' lists hold (2 x LEAD_CAP): 48 bp runs of 3 bp motifs,
    32 stream bits in each of 9 lanes; each is a leader at k = 9, 12, 15, 18 that the primitive-motif test rejects, so the tile
    keeps 288 rows."""
    rng = np.random.RandomState(107)
    seq, want = background(8), []
    for lane in range(9):
        for bit in range(32):
            want.append(plant(seq, TILE + bit * 2_048 + lane * 192 + 70, primitive_motif(rng, 3), 48))
    return [seq], want


# name -> (builder, the oracle's rows per motif size, all contigs together)
CASES = {
    "echoes": (case_echoes, {1: 6, 2: 10, 3: 42, 4: 6, 5: 4, 6: 4, 7: 4, 30: 1, 42: 1, 47: 1}),
    "word_bits": (case_word_bits, {1: 3, 2: 6, 3: 36, 4: 2, 9: 6, 24: 6}),
    "two_leaders": (case_two_leaders, {2: 6, 3: 19, 4: 4, 8: 11}),
    "run_ends": (case_run_ends, {1: 6, 2: 3, 3: 28, 10: 6, 25: 5}),
    "starts": (case_starts, {2: 13, 3: 49, 4: 4, 5: 1, 9: 1, 12: 2, 14: 1, 22: 1}),
    "mixed": (case_mixed, {1: 5, 2: 6, 3: 47, 4: 1, 10: 8, 16: 8, 30: 8, 47: 8}),
    "overflow": (case_overflow, {1: 2, 2: 7, 3: 319, 4: 2}),
}
# n_launches of the overflow case with the kernel as it was before the record pass had two stages (one scan kernel, one gather)
OVERFLOW_N_LAUNCHES = 2


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


_built = {}


def built(name):
    """(contigs as bytes, rows the case is built around as (contig, start, end, k), the oracle's rows): once per session."""
    if name not in _built:
        from oracle import prf_oracle
        seqs, want = CASES[name][0]()
        seqs = [s.tobytes() for s in seqs]
        want = [w if len(w) == 4 else (0,) + w for w in want]
        rows = [(ci, s, e, k) for ci, seq in enumerate(seqs) for s, e, _ml, k in prf_oracle.detect_rows(seq, *SETTINGS)]
        _built[name] = (seqs, want, rows)
    return _built[name]


def per_k(rows):
    return dict(sorted(collections.Counter(k for _c, _s, _e, k in rows).items()))


@pytest.mark.parametrize("name", list(CASES))
def test_record_pass_case(ctx, name):
    import prf_native
    seqs, want, oracle = built(name)
    assert all(len(s) == N_SEQ for s in seqs) and len(seqs) == (2 if name == "starts" else 1)
    have = set(oracle)
    assert all(w in have for w in want), [w for w in want if w not in have]
    print(name, "oracle rows per motif size:", per_k(oracle))
    assert per_k(oracle) == CASES[name][1]
    g = ctx.load(seqs, 50)
    try:
        rows, st = g.scan(*SETTINGS)
        print(name, "n_launches", st.n_launches, "rows", len(rows))
        assert st.path == 1 and st.sorted_on_device == 1
        got = [(int(r["contig"]), int(r["start"]), int(r["end"]), int(r["k"])) for r in rows]
        assert got == oracle
        gen, stg = g.scan(*SETTINGS, flags=prf_native.SCAN_FORCE_GENERIC)
        assert stg.path == 0 and np.array_equal(rows, gen)
        if name == "overflow":
            assert st.n_launches == OVERFLOW_N_LAUNCHES
    finally:
        g.free()


def count_leaders(seq, tile):
    """The leaders of one tile (each in a flagged stream of its own, or two to a stream), counted on the CPU: per motif size k >= 8 the examined aligned groups of 8 positions (every
    one for k < 12, every 2nd for k < 20, else every 4th) that match throughout at distance k, follow fewer than 8 S matches and
    belong to a run that starts in the tile."""
    a = np.frombuffer(seq, dtype=np.uint8).astype(np.int16)
    n = 0
    for k in range(8, 51):
        S = 1 if k < 12 else (2 if k < 20 else 4)
        lo = tile * TILE
        m = a[lo - 64:lo + TILE] == a[lo - 64 + k:lo + TILE + k]           # m[64 + i]: match at tile position i
        for gpos in range(0, TILE, 8 * S):
            if not m[64 + gpos:64 + gpos + 8].all():
                continue
            nb = 0
            while nb < 8 * S and m[64 + gpos - 1 - nb]:
                nb += 1
            n += nb < 8 * S and gpos - nb >= 0
    return n


def test_overflow_case_overflows():
    """The overflow case has more than twice as many leaders in its middle tile as both lists together hold streams -- a stream
    of 32 positions has at most two, with a group that does not match between them -- however the records fall to the two
    waves (counted on the CPU: nothing here runs on the device)."""
    seqs, _want, _oracle = built("overflow")
    n = count_leaders(seqs[0], 1)
    print("leaders in the middle tile:", n)
    assert n > 2 * 2 * LEAD_CAP
