"""GPU (-m gpu): the rows phase of the fused kernel (csrc/scan_vertical.hip, step 4).  A tile keeps four row lists, one per
quarter of its start positions (key >> 30, 16 384 positions each, QCAP = 112 rows); wave w ranks list w, and a row's place in the
slab is the number of rows in the lower quarters plus its rank among its own.  A tile with a quarter of more than 112 rows is
"dense": all its rows are collected in R1, grouped by quarter, and ranked there (up to 2 304 rows), or sorted on the host.

Every case is a set of contigs of 3 tiles (196 608 bp) plus a guard of 64 bp with the planted runs in the middle tile, and must
hold fused = generic = oracle row for row with st.path == 1.  The background is random sequence whose chance rows were broken
on the CPU, so a tile holds the planted rows and nothing else; where a case relies on a count of rows per quarter, the count is
taken from the oracle's rows and asserted before the device is asked.  Nothing here depends on how the rows are ranked: the file
passes on a library with one list per tile as well."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

from test_emit_reservation_gpu import BASES, N, N_SEQ, TILE, T, FLAG_CAP, count_flags, other_base, plant, primitive_motif

pytestmark = pytest.mark.gpu

QUARTER = TILE // 4
QCAP = 112               # csrc/prf_plan.h: rows of a quarter in its LDS sublist
R1_ROWS = 2_304          # rows a dense tile sorts on the device (motif sizes up to 50: the 72-lane image)
DEFAULT = (1, 50, 3, 9)
SHORT = (1, 6, 3, 9)
WIDE = (1, 100, 3, 9)    # the kernel's 80-lane instantiation
EDGE_OFFSETS = (0, 16_383, 16_384, 16_385, 32_767, 32_768, 49_151, 49_152, 65_535)
EDGE_SIZES = (3, 6, 24)  # an exact, a coarse and a group task at the default thresholds
ONE_QUARTER_N = (1, 2, 16, 17, 32, 33, 64, 65, 111, 112, 113, 200)   # (16 | 17 and 32 | 33: the lanes per row change)
SMALL = ((3, 12), (2, 11), (4, 14))   # (motif size, length) of the short planted runs, in turn


def oracle_rows(seq, settings):
    from oracle import prf_oracle
    return [(s, e, k) for s, e, _ml, k in prf_oracle.detect_rows(seq, *settings)]


_background = {}


def background(seed=31):
    """Random sequence without a single row at motif sizes 1-100: every chance row is broken in its middle (on the CPU)."""
    if seed not in _background:
        rng = np.random.RandomState(seed)
        seq = BASES[rng.randint(0, 4, N_SEQ)].copy()
        for _ in range(20):
            rows = oracle_rows(seq.tobytes(), WIDE)
            if not rows:
                break
            for s, e, _k in rows:
                seq[(s + e) // 2] = other_base(seq[(s + e) // 2])
        assert not oracle_rows(seq.tobytes(), WIDE)
        _background[seed] = seq
    return _background[seed].copy()


def settle(seq, planted):
    """Break what the planting made by chance: rows of the oracle (motif sizes 1-100) that are not planted runs.  Returns the
    sequence as bytes."""
    want = set(planted)
    free = np.ones(len(seq), dtype=bool)              # positions outside the planted runs
    for a, b, _k in planted:
        free[a:b] = False
    for _ in range(20):
        extra = [r for r in oracle_rows(seq.tobytes(), WIDE) if r not in want]
        if not extra:
            return seq.tobytes()
        for s, e, _k in extra:                            # a letter outside the planted runs, as near the row's middle as there is one
            at = s + np.flatnonzero(free[s:e])
            assert len(at), (s, e)
            p = int(at[np.argmin(np.abs(at - (s + e) // 2))])
            seq[p] = other_base(seq[p])
    raise AssertionError("the planted tile does not settle")


def plant_small(seq, rng, positions):
    return [plant(seq, p, primitive_motif(rng, SMALL[i % 3][0]), SMALL[i % 3][1]) for i, p in enumerate(positions)]


def spread(q, n, step=None):
    """n start positions in quarter q of the middle tile, evenly apart."""
    step = step or min(80, (QUARTER - 40) // n)
    assert step >= 24 and 20 + n * step <= QUARTER
    return [TILE + q * QUARTER + 20 + i * step for i in range(n)]


# ---- cases: builders return (contigs as bytes, expected rows per quarter of contig 0's middle tile or None) ----
def case_quarter_edges():
    """Runs of an exact, a coarse and a group motif size that start at the first and last position of every quarter and one behind
    the first: nine contigs, one per (offset class, motif size), because runs one position apart would overlap.  The runs at
    offset 65 535 and 65 529 start in quarter 3 and end in the next tile."""
    rng = np.random.RandomState(301)
    contigs = []
    for delta in (-1, 0, 1):
        for k in EDGE_SIZES:
            seq = background()
            offs = [o for o in EDGE_OFFSETS if o % QUARTER == delta % QUARTER]
            if delta == 1:
                offs.append(TILE - 7)
            planted = [plant(seq, TILE + o, primitive_motif(rng, k), 3 * k + 5) for o in offs]
            contigs.append(settle(seq, planted))
    return contigs, None


def case_two_rows_one_start():
    """Two rows with one start, different ends and motif sizes (a word of 12 whose first 11 letters have period 3, three times):
    inside quarter 1 and at the first position of quarter 2."""
    seq = background()
    word = np.frombuffer(b"ACGACGACGACT", dtype=np.uint8)
    planted = []
    for pos in (TILE + QUARTER + 5_000, TILE + 2 * QUARTER):
        planted.append(plant(seq, pos, word, 36))
        planted += [(pos + 12 * i, pos + 12 * i + 11, 3) for i in range(3)]   # (the period-3 stretch of every copy; the first shares the start)
    return [settle(seq, planted)], None


def one_quarter(q, n):
    def build():
        seq = background()
        planted = plant_small(seq, np.random.RandomState(400 + 4 * n + q), spread(q, n))
        return [settle(seq, planted)], tuple(n if i == q else 0 for i in range(4))
    return build


def quarters(counts, step=None):
    def build():
        seq = background()
        rng = np.random.RandomState(500 + sum(counts))
        planted = []
        for q, n in enumerate(counts):
            planted += plant_small(seq, rng, spread(q, n, step))
        return [settle(seq, planted)], tuple(counts)
    return build


def case_scan_time_rows():
    """Two runs in each of 500 streams of quarter 1: more (stream, exact task) flags than the tile's list holds, so some rows are
    made while the tile is still scanned; all 1 000 rows in one quarter."""
    rng = np.random.RandomState(302)
    seq = background()
    planted = []
    for s in range(500):
        p = TILE + QUARTER + s * T
        planted.append(plant(seq, p + 1, primitive_motif(rng, 3), 12))
        planted.append(plant(seq, p + 16, primitive_motif(rng, 2), 11))
    return [settle(seq, planted)], (0, 1000, 0, 0)


def case_long_row():
    """A run of 65 600 positions (span clipped to 16 bits in the key) that starts in quarter 2, short rows in front of it in the
    quarters 0 - 2 and behind it in the next tile."""
    rng = np.random.RandomState(303)
    seq = background()
    start = TILE + 2 * QUARTER + 3_000
    long_run = plant(seq, start, primitive_motif(rng, 5), 65_600)
    planted = [long_run] + plant_small(seq, rng, spread(0, 20) + spread(1, 9) + spread(2, 30)[:25] + [start + 65_600 + 50 + 70 * i for i in range(10)])
    return [settle(seq, planted)], (20, 9, 26, 0)


def case_mixed_tile():
    """An N block across the edge of the quarters 1 and 2, rows in all four quarters."""
    rng = np.random.RandomState(304)
    seq = background()
    lo, hi = TILE + QUARTER + 14_000, TILE + 2 * QUARTER + 2_000
    seq[lo:hi] = N
    pos = spread(0, 30) + spread(1, 40) + [hi + 30 + 80 * i for i in range(35)] + spread(3, 25)
    planted = plant_small(seq, rng, pos)
    seq[lo:hi] = N
    return [settle(seq, planted)], (30, 40, 35, 25)


EDGE_CASES = {"quarter_edges": case_quarter_edges}
EDGE_CASES.update({f"quarter{q}_rows{n}": one_quarter(q, n) for q in (0, 3) for n in ONE_QUARTER_N})
CASES = dict(EDGE_CASES)
CASES.update({
    "two_rows_one_start": case_two_rows_one_start,
    "full_112_each": quarters((112, 112, 112, 112)),
    "full_112_112_112_113": quarters((112, 112, 112, 113)),
    "dense_every_quarter": quarters((150, 130, 170, 140)),
    "dense_more_than_r1": quarters((600, 590, 610, 600), step=24),
    "scan_time_rows": case_scan_time_rows,
    "long_row": case_long_row,
    "mixed_tile": case_mixed_tile,
})
PARAMS = [(name, st) for st in (DEFAULT, SHORT) for name in CASES] + [(name, WIDE) for name in EDGE_CASES]


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


_built = {}


def built(name, settings):
    """(contigs, rows per quarter, the oracle's rows per contig): contigs once per session, rows once per (case, settings)."""
    if name not in _built:
        _built[name] = CASES[name]() + ({},)
    contigs, counts, rows = _built[name]
    if settings not in rows:
        rows[settings] = [oracle_rows(c, settings) for c in contigs]
    return contigs, counts, rows[settings]


def per_quarter(rows):
    """Rows of the middle tile per quarter of their start."""
    return tuple(sum(1 for s, _e, _k in rows if s // TILE == 1 and (s % TILE) // QUARTER == q) for q in range(4))


def cpu_checks(name, settings):
    """What a case is built around, from the oracle's rows alone.  Returns (contigs, oracle rows per contig, rows in the fullest tile)."""
    contigs, counts, oracle = built(name, settings)
    assert all(len(c) == N_SEQ for c in contigs)
    if counts is not None:      # (the planted runs have motif sizes 2 - 5: the same rows at every setting)
        assert per_quarter(oracle[0]) == counts
    if name == "quarter_edges":
        for ci, rows in enumerate(oracle):
            delta, k = (-1, 0, 1)[ci // 3], EDGE_SIZES[ci % 3]
            want = {TILE + o for o in EDGE_OFFSETS if o % QUARTER == delta % QUARTER} | ({2 * TILE - 7} if delta == 1 else set())
            assert {s for s, _e, kk in rows if kk == k} == (want if settings[0] <= k <= settings[1] else set())
        assert any(s < 2 * TILE < e for rows in oracle for s, e, _k in rows)
    if name == "two_rows_one_start":
        starts = [s for s, _e, _k in oracle[0]]
        assert len(starts) - len(set(starts)) == (2 if settings[1] >= 12 else 0)
        assert settings[1] < 12 or TILE + 2 * QUARTER in starts
    if name == "scan_time_rows":
        n = count_flags(contigs[0], 1, settings)
        print(name, "flags in the middle tile (CPU model, lower bound):", n)
        assert n > FLAG_CAP
    if name == "long_row":
        assert any(e - s >= 65_535 and s // TILE == 1 and (s % TILE) // QUARTER == 2 for s, e, _k in oracle[0])
    if name == "mixed_tile":
        assert N in np.frombuffer(contigs[0], dtype=np.uint8)[TILE:2 * TILE]
    return contigs, oracle, max(sum(per_quarter(r)) for r in oracle)


@pytest.mark.parametrize("name,settings", PARAMS, ids=[f"{n}-{s[1]}" for n, s in PARAMS])
def test_rank_case(ctx, name, settings):
    import prf_native
    contigs, oracle, n_tile = cpu_checks(name, settings)
    g = ctx.load(contigs, settings[1])
    try:
        rows, st = g.scan(*settings)
        print(name, settings, "rows per quarter", _built[name][1], "rows in the tile", n_tile, "n_launches", st.n_launches, "sorted_on_device", st.sorted_on_device)
        assert st.path == 1
        got = [(int(r["contig"]), int(r["start"]), int(r["end"]), int(r["k"])) for r in rows]
        assert got == [(c, s, e, k) for c, rr in enumerate(oracle) for s, e, k in rr]
        assert st.sorted_on_device == (1 if n_tile <= R1_ROWS else 0)     # (quarter*_rows113 / 200: dense below 448 rows per tile)
        gen, stg = g.scan(*settings, flags=prf_native.SCAN_FORCE_GENERIC)
        assert stg.path == 0 and np.array_equal(rows, gen)
    finally:
        g.free()
