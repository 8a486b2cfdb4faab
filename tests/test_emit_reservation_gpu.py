"""GPU (-m gpu): how the scan phase of the fused kernel hands its candidates to the tile's lists (csrc/vscan_tasks.h,
Emit::push_words and Emit::push_flags): every lane reserves its own slots -- one returning LDS add per lane and task -- and
writes its records / flags behind the base it got; what the lists cannot take is verified on the spot.

Every case is a contig of 3 tiles (196 608 bp) plus a guard of 64 bp, built from a seeded background and planted runs, and is
compared row for row with the generic path and with the CPU oracle.  The cases that rely on a full list count the tile's
records / flags on the CPU first, with a numpy model of the flag rules (nothing of that runs on the device)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

pytestmark = pytest.mark.gpu

TILE = 65_536
T = 32                   # positions per stream; stream s of a tile = lane s % 64, bit s // 64
N_SEQ = 3 * TILE + 64
REC_CAP = 192            # csrc/prf_plan.h: group-task records of a tile
FLAG_CAP = 960           # ... and (stream, exact task) flags
SMALL_M = 15             # M(k) below this: exact / coarse task, else group task
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
N = np.frombuffer(b"N", dtype=np.uint8)[0]
DEFAULT = (1, 50, 3, 9)
ONE_LANE_ROWS = (8, 11, 13, 12, 16, 19, 44, 47, 50)   # primitive motifs planted in the one-lane case


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
    """seq[pos : pos+length] = copies of the motif, cut at `length`; the bases on either side break the period."""
    k = len(motif)
    seq[pos:pos + length] = np.tile(motif, length // k + 1)[:length]
    seq[pos - 1] = other_base(seq[pos - 1 + k])
    seq[pos + length] = other_base(seq[pos + length - k])
    return (pos, pos + length, k)


def stream_pos(tile, lane, bit):
    return tile * TILE + (bit * 64 + lane) * T


# ---- the flag rules on the CPU (clean tiles) ----
def min_matches(k, min_repeats, min_span):
    return max((min_repeats - 1) * k, min_span - k)


def matches(seq, tile, k, before, after):
    """m[before + i]: position tile * TILE + i equals the one k further on."""
    a = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, bytes) else seq
    lo = tile * TILE
    return a[lo - before:lo + TILE + after] == a[lo - before + k:lo + TILE + after + k]


def count_records(seq, tile, settings):
    """Group-task records of a clean tile: (lane, k) pairs, M(k) >= 15, with a flagged stream -- an examined aligned group of 8
    positions (every one for M < 23, every 2nd for M < 39, else every 4th) that matches throughout at distance k and, where
    every group is examined, does not follow an all-match group of its own stream."""
    kmin, kmax, r, span = settings
    n = 0
    for k in range(kmin, kmax + 1):
        M = min_matches(k, r, span)
        if M < SMALL_M:
            continue
        ok = matches(seq, tile, k, 0, 0).reshape(TILE // T, 4, 8).all(axis=2)          # [stream][group]
        if M >= 39:
            hot = ok[:, 0]
        elif M >= 23:
            hot = ok[:, 0] | ok[:, 2]
        else:
            hot = ok[:, 0] | (ok[:, 1:] & ~ok[:, :-1]).any(axis=1)
        n += int(hot.reshape(T, 64).any(axis=0).sum())                                 # [bit][lane] -> lanes with a word
    return n


def count_flags(seq, tile, settings):
    """(stream, exact task) flags of a clean tile, M(k) < 15: streams that hold the first position of a run of >= M matches.  The
    coarse tasks (M >= 9) flag these streams and some more: a lower bound."""
    kmin, kmax, r, span = settings
    n = 0
    for k in range(kmin, kmax + 1):
        M = min_matches(k, r, span)
        if M >= SMALL_M:
            continue
        m = matches(seq, tile, k, 1, M)
        win = np.ones(TILE + 1, dtype=bool)                  # win[j]: the M positions from tile position j - 1 on match
        for i in range(M):
            win &= m[i:i + TILE + 1]
        start = win[1:] & ~m[:TILE]
        n += int(start.reshape(TILE // T, T).any(axis=1).sum())
    return n


# ---- cases: name -> (builder -> contig, the settings it is scanned with) ----
def case_one_lane_many_sizes():
    """A 400 bp homopolymer and a 300 bp dinucleotide run: records at every motif size of every group task, all in a few lanes
    (echoes, which the verification rejects) -- beside runs of primitive motifs of those sizes, which must come out as rows."""
    rng = np.random.RandomState(201)
    seq = background(11)
    plant(seq, stream_pos(1, 5, 3) + 3, primitive_motif(rng, 1), 400)
    plant(seq, stream_pos(1, 40, 17) + 9, primitive_motif(rng, 2), 300)
    for i, k in enumerate(ONE_LANE_ROWS):
        plant(seq, stream_pos(1, 6 + i, 20 + i % 3) + 5, primitive_motif(rng, k), 3 * k + 10)   # (lanes the homopolymer covers as well)
    return seq


def case_many_lanes_one_size():
    """64 runs of a 24 bp motif, 80 bp each, one starting in every lane (stream bits spread): every lane reserves in the same
    instruction of the task that holds k = 24."""
    rng = np.random.RandomState(202)
    seq = background(12)
    for lane in range(64):
        plant(seq, stream_pos(1, lane, (lane * 5) % 32) + (lane % 7), primitive_motif(rng, 24), 80)
    return seq


def case_record_overflow():
    """40 homopolymers of 200 bp in distinct lanes of the middle tile: each is a record for every motif size k with 3 k <= 200 (and
    an echo of every larger one), in every lane it covers -- far more than the list's 192."""
    rng = np.random.RandomState(203)
    seq = background(13)
    for i in range(40):
        plant(seq, stream_pos(1, (i * 8) % 64 + i // 8, i % 32) + 2, primitive_motif(rng, 1), 200)
    return seq


def case_flag_overflow():
    """1 200 runs of 3 bp motifs, 12 bp each, one per stream: more (stream, exact task) flags than the list's 960."""
    rng = np.random.RandomState(204)
    seq = background(14)
    for s in range(1200):
        plant(seq, TILE + s * T + 8 + s % 9, primitive_motif(rng, 3), 12)
    return seq


def case_lane_several_flags():
    """Several flags of one exact task in one lane: runs of a 2 bp motif in three streams of lane 9 and two of lane 50 (bits apart),
    and two and three run starts of k = 1 inside one 32-position stream."""
    rng = np.random.RandomState(205)
    seq = background(15)
    for lane, bits in ((9, (1, 2, 30)), (50, (0, 31))):
        for bit in bits:
            plant(seq, stream_pos(1, lane, bit) + 4, primitive_motif(rng, 2), 14)
    for lane, offs in ((21, (1, 17)), (33, (0, 11, 22))):
        for off in offs:
            plant(seq, stream_pos(1, lane, 12) + off, primitive_motif(rng, 1), 9)
    return seq


def case_mixed_tile():
    """An N block inside the middle tile (the relaxed flag rule, every group task without the predecessor test): runs directly behind
    the block, in front of it, and further on."""
    rng = np.random.RandomState(206)
    seq = background(16)
    lo = TILE + 20_000
    seq[lo:lo + 3_000] = N
    for i, k in enumerate((1, 3, 7, 9, 14, 24, 47)):
        plant(seq, lo + 3_000 + 400 * i, primitive_motif(rng, k), 3 * k + 20)                       # i = 0: directly behind the block
        plant(seq, lo - 400 * i - (3 * k + 20), primitive_motif(rng, k), 3 * k + 20)                # i = 0: ends where it begins
        plant(seq, lo + 30_000 + 500 * i, primitive_motif(rng, k), 4 * k + 9)
    seq[lo:lo + 3_000] = N
    return seq


def case_kmax():
    """Runs of every motif size up to 23 and a homopolymer: with kmax = 15 or 23 the last group task's second half lies beyond the
    largest size, and the plan has exact, coarse and group tasks."""
    rng = np.random.RandomState(207)
    seq = background(17)
    pos = TILE + 500
    for k in range(1, 24):
        plant(seq, pos, primitive_motif(rng, k), 3 * k + 11)
        pos += 1_777
    plant(seq, pos, primitive_motif(rng, 1), 120)
    return seq


CASES = {
    "one_lane_many_sizes": (case_one_lane_many_sizes, DEFAULT),
    "one_lane_sizes_8_13": (case_one_lane_many_sizes, (8, 13, 3, 9)),      # a task of 4 sizes and one of 2
    "one_lane_sizes_12_19": (case_one_lane_many_sizes, (12, 19, 3, 9)),    # one task of 8 sizes
    "one_lane_sizes_44_50": (case_one_lane_many_sizes, (44, 50, 3, 9)),    # 7 valid sizes
    "many_lanes_one_size": (case_many_lanes_one_size, DEFAULT),
    "record_overflow": (case_record_overflow, DEFAULT),
    "flag_overflow": (case_flag_overflow, DEFAULT),
    "lane_several_flags": (case_lane_several_flags, DEFAULT),
    "mixed_tile": (case_mixed_tile, DEFAULT),
    "kmax_15": (case_kmax, (1, 15, 3, 9)),
    "kmax_23": (case_kmax, (1, 23, 3, 9)),
}
# launches per scan as they were before the lanes reserved for themselves (2: scan kernel + row gather)
# (not flag_overflow: 1 208 rows in one tile make the slabs grow and the scan repeat, which is not what this file is about)
N_LAUNCHES = {name: 2 for name in CASES if name != "flag_overflow"}


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


_built = {}


def built(name):
    """(the contig as bytes, the oracle's rows): once per session."""
    if name not in _built:
        from oracle import prf_oracle
        builder, settings = CASES[name]
        seq = builder().tobytes()
        assert len(seq) == N_SEQ
        _built[name] = (seq, [(s, e, k) for s, e, _ml, k in prf_oracle.detect_rows(seq, *settings)])
    return _built[name]


@pytest.mark.parametrize("name", list(CASES))
def test_emit_case(ctx, name):
    import prf_native
    seq, oracle = built(name)
    settings = CASES[name][1]
    if name == "record_overflow":
        n = count_records(seq, 1, settings)
        print(name, "records in the middle tile (CPU model):", n)
        assert n > REC_CAP
    if name == "flag_overflow":
        n = count_flags(seq, 1, settings)
        print(name, "flags in the middle tile (CPU model, lower bound):", n)
        assert n > FLAG_CAP
    g = ctx.load([seq], 50)
    try:
        rows, st = g.scan(*settings)
        print(name, "n_launches", st.n_launches, "rows", len(rows), "oracle", len(oracle))
        assert st.path == 1
        got = [(int(r["start"]), int(r["end"]), int(r["k"])) for r in rows]
        assert got == oracle
        gen, stg = g.scan(*settings, flags=prf_native.SCAN_FORCE_GENERIC)
        assert stg.path == 0 and np.array_equal(rows, gen)
        assert name not in N_LAUNCHES or st.n_launches == N_LAUNCHES[name]
    finally:
        g.free()


def test_cases_hold_what_they_are_built_around():
    """On the CPU: the planted runs are rows of the oracle, and the one-lane cases have records at every motif size of their range."""
    seq, oracle = built("one_lane_many_sizes")
    a = np.frombuffer(seq, dtype=np.uint8)
    assert any(k == 1 and e - s == 400 for s, e, k in oracle) and any(k == 2 and e - s == 300 for s, e, k in oracle)
    assert all(any(k == kk and e - s == 3 * kk + 10 for s, e, k in oracle) for kk in ONE_LANE_ROWS)
    for name in ("one_lane_sizes_8_13", "one_lane_sizes_12_19", "one_lane_sizes_44_50"):
        assert len(built(name)[1]) >= 3, name
    for lo, hi in ((8, 13), (12, 19), (44, 50), (8, 50)):
        for k in range(lo, hi + 1):
            assert count_records(a, 1, (k, k, 3, 9)) >= 2, k      # the homopolymer's lanes and the dinucleotide's (even k)
    # (13 lanes under the homopolymer, 10 under the dinucleotide run: the three narrow ranges fit the list, motif 1-50 does not)
    assert all(count_records(a, 1, (lo, hi, 3, 9)) <= REC_CAP for lo, hi in ((8, 13), (12, 19), (44, 50)))
    assert count_records(a, 1, DEFAULT) > REC_CAP
    seq, oracle = built("many_lanes_one_size")
    assert sum(k == 24 for _s, _e, k in oracle) == 64
    assert count_records(np.frombuffer(seq, dtype=np.uint8), 1, (24, 24, 3, 9)) == 64
    seq, oracle = built("lane_several_flags")
    assert sum(k == 2 and e - s == 14 for s, e, k in oracle) == 5 and sum(k == 1 and e - s == 9 for s, e, k in oracle) == 5


def test_overflow_is_deterministic(ctx):
    """The full record list 20 times: which records find room depends on the order the waves arrive in, the rows do not."""
    seq, oracle = built("record_overflow")
    settings = CASES["record_overflow"][1]
    g = ctx.load([seq], 50)
    try:
        first, _ = g.scan(*settings)
        assert [(int(r["start"]), int(r["end"]), int(r["k"])) for r in first] == oracle
        for _ in range(19):
            rows, _st = g.scan(*settings)
            assert np.array_equal(rows, first)
    finally:
        g.free()
