"""GPU (-m gpu): the exact tasks of motif sizes 2, 3 and 4 do not flag the echoes of a shorter motif (csrc/vscan_tasks.h,
exact_stream): the primitive-motif test is made once per segment of start rows, at the segment's last row.

Every case is a contig of 3 tiles (196 608 bp) with planted runs in the middle tile, scanned with three settings --
(1, 50, 3, 9): (K, M) = (2, 7), (3, 6), (4, 8), segments of 8, 4, 8 rows; (1, 8, 2, 9): (2, 7), (3, 6), (4, 5); (1, 12, 2, 4):
M = K, segments of 2, 4, 4 -- and compared row for row with the generic path and with the CPU oracle: a suppressed primitive
run would be a missing row.  That echoes ARE suppressed is the last test's subject: with only exact tasks in the plan the
device's candidate count is the number of flags, which the numpy model (tests/echo_flags_model.py) counts beforehand."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import echo_flags_model as model

pytestmark = pytest.mark.gpu

TILE = model.TILE
T = model.T
N_SEQ = 3 * TILE
FLAG_CAP = 960           # csrc/prf_plan.h: (stream, exact task) flags of a tile
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
N = np.frombuffer(b"N", dtype=np.uint8)[0]
SETTINGS = {"r3_span9": (1, 50, 3, 9), "r2_span9": (1, 8, 2, 9), "r2_span4": (1, 12, 2, 4)}
_backgrounds = {}
# (planted constructs lie three streams apart: gcd(3, 64) = 1, so they visit every lane)


def background(seed, settings, n=N_SEQ):
    """Seeded random sequence.  For min_span 4 (runs of 4 positions count) no position equals the one 2 or 3 before it: no
    runs of the sizes 1-3 but the planted ones, so that the tiles' flag lists are not full to begin with."""
    quiet = settings[3] < 9
    if (seed, quiet) not in _backgrounds:
        rng = np.random.RandomState(seed)
        idx = rng.randint(0, 4, n).tolist()
        if quiet:
            pick = rng.randint(0, 2, n).tolist()
            for i in range(3, n):
                free = [b for b in (0, 1, 2, 3) if b != idx[i - 2] and b != idx[i - 3]]
                idx[i] = free[pick[i] % len(free)]
        _backgrounds[(seed, quiet)] = BASES[np.array(idx)]
    return _backgrounds[(seed, quiet)].copy()


def primitive_motif(rng, k):
    while True:
        m = BASES[rng.randint(0, 4, k)]
        if all(k % d or not np.array_equal(m, np.tile(m[:d], k // d)) for d in range(1, k)):
            return m


def other_base(*bs):
    return next(b for b in BASES if b not in bs)


def plant(seq, pos, motif, length):
    """seq[pos : pos+length] = copies of the motif, cut at `length`; the bases on either side break the period."""
    k = len(motif)
    seq[pos:pos + length] = np.tile(motif, length // k + 1)[:length]
    if pos > 0:
        seq[pos - 1] = other_base(seq[pos - 1 + k])
    seq[pos + length] = other_base(seq[pos + length - k])


def M_of(k, settings):
    return model.min_matches(k, settings[2], settings[3])


def plant_pair(seq, pos, rng, K, echo_len, echo_first, settings, dinucleotide=False):
    """An echo run (homopolymer, or dinucleotide run for K = 4) and a primitive run of size K over the same letters, one directly
    behind the other, between two bases of a third letter.  Returns the construct's length."""
    e, x, g = BASES[rng.permutation(4)[:3]]
    if dinucleotide:
        echo = np.tile(np.array([e, x], dtype=np.uint8), echo_len)[:echo_len]
        motif = np.array([e, x, x, x], dtype=np.uint8)
    else:
        echo = np.full(echo_len, e, dtype=np.uint8)
        motif = np.array([x] + [e] * (K - 1), dtype=np.uint8)
    lp = M_of(K, settings) + K + 3
    prim = np.tile(motif, lp // K + 1)[:lp]
    both = np.concatenate([echo, prim] if echo_first else [prim, echo])
    seq[pos:pos + len(both)] = both
    if pos > 0:
        seq[pos - 1] = g
    seq[pos + len(both)] = g
    return len(both)


# ---- cases: builder(settings) -> list of contigs ----
def case_primitive_every_offset(settings):
    """Primitive runs of the sizes 2, 3, 4 at every row offset of a stream, of the minimal length M + K (the sampled row lies on
    the run's last letters) and of 40 positions; offsets 25-31 are sampled at row 32, the next stream's row 0.  Extra: minimal
    runs in streams of lane 0 and lane 63 at the offsets 0, 25 and 31."""
    rng = np.random.RandomState(301)
    seq = background(21, settings)
    s = 1
    for K in (2, 3, 4):
        for length in (M_of(K, settings) + K, 40):
            for off in range(T):
                plant(seq, TILE + s * T + off, primitive_motif(rng, K), length)
                s += 3
    assert s < 10 * 64
    bit = 10   # (lane 0 in the bits 10-18, lane 63 in 20-28: a run of lane 63 reaches into lane 0 of the next bit)
    for K in (2, 3, 4):
        for off in (0, 25, 31):
            for lane in (0, 63):
                plant(seq, TILE + ((bit + (10 if lane else 0)) * 64 + lane) * T + off, primitive_motif(rng, K), M_of(K, settings) + K)
            bit += 1
    return [seq]


def case_echo_every_offset(settings):
    """Homopolymers of 9 .. 40 bases and dinucleotide runs of 12 .. 40 at every row offset: no row at k = 2, 3, 4 from the
    former or at k = 4 from the latter, and none lost at k = 1, 2."""
    rng = np.random.RandomState(302)
    seq = background(22, settings)
    s = 1
    for rep in range(2):
        for off in range(T):
            plant(seq, TILE + s * T + off, primitive_motif(rng, 1), 9 + (off * 7 + 13 * rep) % 32)
            s += 3
            plant(seq, TILE + s * T + off, primitive_motif(rng, 2), 12 + (off * 5 + 11 * rep) % 29)
            s += 3
    return [seq]


def case_echo_next_to_primitive(settings):
    """An echo run directly followed by (and directly following) a primitive run of the same size that shares its letters, e.g.
    A..AACACAC..: at the low offsets both starts fall in one stream."""
    rng = np.random.RandomState(303)
    seq = background(23, settings)
    s = 1
    for first in (True, False):
        for off in range(T):
            for K in (2, 3, 4):
                plant_pair(seq, TILE + s * T + off, rng, K, 12, first, settings)
                s += 3
            plant_pair(seq, TILE + s * T + off, rng, 4, 16, first, settings, dinucleotide=True)
            s += 3
    assert s < TILE // T
    return [seq]


def case_tile_edges(settings):
    """One contig per construct and position: primitive runs, echo runs and echo-primitive pairs that start at the middle tile's
    first position (its conservative first stream) or five positions in front of it (the run crosses the edge: the tile's first
    row lies in the middle of it); each contig has the same construct at its own first position as well."""
    rng = np.random.RandomState(304)
    contigs = []
    kinds = [("run", k) for k in (2, 3, 4)] + [("long", 1), ("long", 2)] + [("pair", k) for k in (2, 3, 4)]
    for kind, k in kinds:
        for delta in (0, 5):
            seq = background(24, settings)
            for pos in (0, TILE - delta):
                if kind == "run":
                    plant(seq, pos, primitive_motif(rng, k), max(M_of(k, settings) + k, 12))
                elif kind == "long":
                    plant(seq, pos, primitive_motif(rng, k), 40)
                else:
                    plant_pair(seq, pos, rng, k, 12, True, settings)
            contigs.append(seq)
    return contigs


def case_mixed_tile(settings):
    """An N block inside the middle tile: this tile and the one before it take the relaxed rule and suppress nothing.  Echo runs
    and primitive runs of the sizes 2-4 directly behind the block, directly in front of it, and further on."""
    rng = np.random.RandomState(305)
    seq = background(25, settings)
    lo = TILE + 20_000
    seq[lo:lo + 3_000] = N
    for i, k in enumerate((1, 2, 3, 4, 1, 2, 3, 4)):
        length = 12 if i < 4 else 33
        plant(seq, lo + 3_000 + 300 * i, primitive_motif(rng, k), length)                 # i = 0: directly behind the block
        plant(seq, lo - 300 * i - length, primitive_motif(rng, k), length)                # i = 0: ends where it begins
        plant(seq, lo + 30_000 + 300 * i + i, primitive_motif(rng, k), length)
        plant_pair(seq, lo + 3_000 + 300 * i + 100, rng, 2 + i % 3, 12, i % 2 == 0, settings)
        plant_pair(seq, lo - 300 * i - 200, rng, 2 + i % 3, 12, i % 2 == 0, settings)
    plant(seq, TILE // 2 + 7, primitive_motif(rng, 1), 20)                                # the tile in front: mixed as well
    plant(seq, TILE // 2 + 307, primitive_motif(rng, 3), 14)
    seq[lo:lo + 3_000] = N
    return [seq]


def case_flag_overflow(settings):
    """1 300 primitive runs of the sizes 2 and 3, 12 bp each, one per stream, and a homopolymer in every tenth of the streams left:
    more flags than the list's 960 after suppression (counted by the model before the device is asked)."""
    rng = np.random.RandomState(306)
    seq = background(26, settings)
    for s in range(1, 1301):
        plant(seq, TILE + s * T + 6 + s % 11, primitive_motif(rng, 2 + s % 2), 12)
    for s in range(1310, 2040, 10):
        plant(seq, TILE + s * T + s % 17, primitive_motif(rng, 1), 12)
    return [seq]


CASES = {
    "primitive_every_offset": case_primitive_every_offset,
    "echo_every_offset": case_echo_every_offset,
    "echo_next_to_primitive": case_echo_next_to_primitive,
    "tile_edges": case_tile_edges,
    "mixed_tile": case_mixed_tile,
    "flag_overflow": case_flag_overflow,
}


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


_built = {}


def built(name, sname):
    """[(the contig as bytes, the oracle's rows)]: once per session."""
    if (name, sname) not in _built:
        from oracle import prf_oracle
        settings = SETTINGS[sname]
        out = []
        for seq in CASES[name](settings):
            assert len(seq) == N_SEQ
            b = seq.tobytes()
            out.append((b, [(s, e, k) for s, e, _ml, k in prf_oracle.detect_rows(b, *settings)]))
        _built[(name, sname)] = out
    return _built[(name, sname)]


@pytest.mark.parametrize("sname", list(SETTINGS))
@pytest.mark.parametrize("name", list(CASES))
def test_echo_case(ctx, name, sname):
    import prf_native
    settings = SETTINGS[sname]
    for seq, oracle in built(name, sname):
        if name == "flag_overflow":
            seen, prim, flagged = model.count_flags(seq, 1, settings)
            print(name, sname, "middle tile (CPU model): streams with a start", seen, "with a primitive start", prim, "flagged", flagged)
            assert flagged > FLAG_CAP
        g = ctx.load([seq], 50)
        try:
            rows, st = g.scan(*settings)
            assert st.path == 1
            got = [(int(r["start"]), int(r["end"]), int(r["k"])) for r in rows]
            assert got == oracle
            gen, stg = g.scan(*settings, flags=prf_native.SCAN_FORCE_GENERIC)
            assert stg.path == 0 and np.array_equal(rows, gen)
        finally:
            g.free()
    print(name, sname, "contigs", len(built(name, sname)), "rows", sum(len(o) for _s, o in built(name, sname)))


def test_cases_hold_what_they_are_built_around():
    """On the CPU: the planted primitive runs are rows of the oracle at their own size, the echo runs are rows at the echoed size
    and at no other of 2, 3, 4, and the model sees both kinds of start in the middle tile."""
    for sname, settings in SETTINGS.items():
        (_seq, oracle), = built("primitive_every_offset", sname)
        for K in (2, 3, 4):
            lens = [e - s for s, e, k in oracle if k == K and TILE <= s < 2 * TILE]
            assert lens.count(40) >= T and lens.count(M_of(K, settings) + K) >= T + 6, (sname, K)
        (seq, oracle), = built("echo_every_offset", sname)
        assert sum(k == 1 and 9 <= e - s <= 40 for s, e, k in oracle) >= 2 * T
        assert sum(k == 2 and 12 <= e - s <= 40 for s, e, k in oracle) >= 2 * T
        seen, prim, flagged = model.count_flags(seq, 1, (2, 4) + settings[2:])
        print(sname, "echo_every_offset, sizes 2-4, middle tile: streams with a start", seen, "primitive", prim, "flagged", flagged)
        assert seen - prim >= 3 * T and prim <= flagged <= prim + 3        # (2 T dinucleotide runs stay, at k = 2)
        (seq, oracle), = built("echo_next_to_primitive", sname)
        for K in (2, 3, 4):
            assert sum(k == K and e - s >= M_of(K, settings) + K + 3 for s, e, k in oracle) >= 2 * T, (sname, K)


def test_echoes_are_not_flagged(ctx):
    """Motif sizes 2-4 only: every task is an exact task, so stats.n_candidates is the number of flags.  Two tiles of random
    background with 200 homopolymers of 12 bases (an echo at each of the three sizes), and a last tile -- mixed, because the contig
    ends behind it: no suppression there -- of AACCGGTT.., in which no position equals the one 2, 3 or 4 further on."""
    settings = (2, 4, 3, 9)
    rng = np.random.RandomState(307)
    seq = background(27, settings)
    seq[2 * TILE:] = np.tile(np.frombuffer(b"AACCGGTT", dtype=np.uint8), TILE // 8)
    for i in range(200):
        plant(seq, 300 + 650 * i + rng.randint(0, 32), primitive_motif(rng, 1), 12)
    counts = [model.count_flags(seq, tile, settings) for tile in range(3)]
    assert counts[2] == (0, 0, 0)
    unsuppressed = sum(c[0] for c in counts)
    m = sum(c[1] for c in counts)
    print("streams x sizes with a start", unsuppressed, "with a primitive start", m, "flagged by the model's sampled rule", sum(c[2] for c in counts))
    assert unsuppressed >= 2 * m
    g = ctx.load([seq.tobytes()], 50)
    try:
        rows, st = g.scan(*settings)
        print("n_candidates", st.n_candidates, "rows", len(rows))
        assert st.path == 1
        assert m <= st.n_candidates <= m + 3 * 3
    finally:
        g.free()
