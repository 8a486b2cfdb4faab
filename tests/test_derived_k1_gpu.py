"""GPU (-m gpu): homopolymer rows of the fused kernel.  Where the plan derives them (csrc/prf_plan.h, prf_plan_derives_k1) a
clean tile does not run the k = 1 task: the k = 2 task's echo starts leave as the k = 1 task's flags (csrc/vscan_tasks.h,
exact_stream<2, M> and run_tasks).  A mixed tile -- not-ACGT letters in reach, or the contig's last tile -- runs the k = 1 task.

Every case is a list of contigs of 3 tiles (196 608 bp) with planted homopolymers, scanned at the five settings that derive and
the four that do not (tests/test_derived_k1_cpu.py), and compared row for row with the generic path and with the CPU oracle: a
homopolymer start that the k = 2 task does not hand over is a missing row.  The tiles 0 and 1 of a contig without N are clean,
tile 2 is mixed.  Nothing here depends on where the k = 1 flags come from: the file passes on a library that runs the k = 1 task
on every tile as well."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

from test_echo_flags_gpu import BASES, N, N_SEQ, TILE, T, background, other_base

pytestmark = pytest.mark.gpu

DERIVED = ((1, 50, 3, 9), (1, 2, 3, 9), (1, 6, 2, 4), (1, 6, 4, 8), (1, 6, 2, 10))
NOT_DERIVED = ((1, 1, 3, 9), (2, 6, 3, 9), (1, 6, 3, 5), (1, 6, 2, 11))
SETTINGS = DERIVED + NOT_DERIVED
LENGTHS = (8, 9, 10, 11, 40, 100, 5_000)          # 8 letters are no row at min_span 9
ROWS = (0, 1, 7, 8, 9, 23, 24, 30, 31)            # start rows of a stream: segment edges, and runs that cross into the next lane


def homopolymer(seq, pos, base, length, left="x"):
    """seq[pos : pos + length] = base, another letter behind it; in front "x" (two other letters) or "Ax" (base, other letter)."""
    seq[pos:pos + length] = base
    if pos + length < len(seq):
        seq[pos + length] = other_base(base)
    if pos >= 1:
        seq[pos - 1] = other_base(base)
    if pos >= 2:
        seq[pos - 2] = base if left == "Ax" else other_base(base, seq[pos - 1])


def stream_pos(tile, s):
    return tile * TILE + s * T


# ---- cases: builder(settings) -> list of contigs ----
def case_lengths_and_rows(settings):
    """Homopolymers of each base and length with both kinds of left neighbour; starts at the rows of ROWS with 9, 12 and 40 letters
    in the lanes 0 - 63; a start in lane 63 whose run goes on in lane 0 of the next bit; two starts in one stream; a dinucleotide
    row against a homopolymer, both ways round."""
    seq = background(41, settings)
    pos = 3_000                                     # tile 0: the long ones
    for base in BASES:
        for left in ("x", "Ax"):
            homopolymer(seq, pos + 13, base, 5_000 if left == "x" else 100, left)
            pos += 6_000
    s = 3                                           # tile 1, three streams apart: every lane is visited
    for li, length in enumerate(LENGTHS[:-1]):
        for bi, base in enumerate(BASES):
            for left in ("x", "Ax"):
                homopolymer(seq, stream_pos(1, s) + (5 * li + 3 * bi) % T, base, length, left)
                s += 3 + (length + T - 1) // T
    for row in ROWS:
        for li, length in enumerate((9, 12, 40)):
            homopolymer(seq, stream_pos(1, s) + row, BASES[(row + li) % 4], length, "Ax" if (row + li) % 2 else "x")
            s += 5
    assert s < 1_200
    for i, (row, length) in enumerate(((28, 20), (31, 9), (24, 9), (0, 40))):      # lane 63 of the bits 20 ..: on into lane 0, one bit up
        homopolymer(seq, stream_pos(1, (20 + 2 * i) * 64 + 63) + row, BASES[i], length)
    for i in range(4):                              # two starts in one stream, in different segments; the first has 8 letters
        p = stream_pos(1, 30 * 64 + 7 + 3 * i)
        homopolymer(seq, p + 2, BASES[i], 8)
        homopolymer(seq, p + 14 + i, BASES[i], 12)
    word = np.frombuffer(b"AAAAAAAAAACACACACACACAC", dtype=np.uint8)
    for i, w in enumerate((word, word[::-1])):
        for row in (0, 3, 9, 27):
            p = stream_pos(1, 31 * 64 + 5 + 12 * i + 3 * (row % 4)) + row
            seq[p:p + len(w)] = w
            seq[p - 1] = seq[p + len(w)] = ord("G")
    return [seq]


def case_edges(settings):
    """Contig 0: a start on the first position of tile 1 with another letter in front, a run across the end of tile 1 (which tile 1
    owns), a start at position 0 of the contig and a run in the contig's last 9 letters.  Contig 1: a run across the end of tile 0
    and one that ends on tile 1's last position, a run of exactly 9 letters at position 0, the last 9 letters again.  Contig 2: a
    run that begins on the last position of tile 0."""
    a = background(42, settings)
    homopolymer(a, 0, BASES[0], 30)
    homopolymer(a, TILE, BASES[1], 12)
    homopolymer(a, 2 * TILE - 5, BASES[2], 20)
    homopolymer(a, N_SEQ - 9, BASES[3], 9)
    b = background(43, settings)
    homopolymer(b, 0, BASES[2], 9)
    homopolymer(b, TILE - 5, BASES[3], 20, "Ax")
    homopolymer(b, 2 * TILE - 11, BASES[0], 11)
    homopolymer(b, N_SEQ - 9, BASES[1], 9, "Ax")
    c = background(44, settings)
    homopolymer(c, TILE - 1, BASES[0], 10)
    homopolymer(c, 2 * TILE - 1, BASES[1], 9)
    return [a, b, c]


def case_all_a(settings):
    """One letter from end to end: one row at k = 1, a candidate in no stream but the contig's first."""
    return [np.full(N_SEQ, BASES[0], dtype=np.uint8)]


def case_n_blocks(settings):
    """Mixed tiles, which run the k = 1 task themselves: homopolymers directly behind and directly in front of an N block, inside a
    tile that holds an N elsewhere, and in the clean tile in front of the one with the block."""
    seq = background(45, settings)
    lo, hi = TILE + 20_000, TILE + 23_000
    seq[lo:hi] = N
    homopolymer(seq, hi, BASES[0], 12)              # the letter in front is N
    homopolymer(seq, lo - 12, BASES[1], 12)         # ends where the block begins
    seq[lo:hi] = N
    for i, length in enumerate(LENGTHS[:-1]):
        homopolymer(seq, hi + 5_000 + 700 * i + i, BASES[i % 4], length, "Ax" if i % 2 else "x")
        homopolymer(seq, TILE + 3_000 + 700 * i + 3 * i, BASES[(i + 1) % 4], length, "x" if i % 2 else "Ax")
        homopolymer(seq, 10_000 + 700 * i + 5 * i, BASES[(i + 2) % 4], length)     # tile 0: the block is out of its reach
    other = background(46, settings)
    other[TILE + 40_000] = N                        # a single N in tile 1
    for i, length in enumerate(LENGTHS[:-1]):
        homopolymer(other, TILE + 1_000 + 900 * i + 7 * i, BASES[i % 4], length)
    homopolymer(other, TILE + 40_001, BASES[2], 15)
    homopolymer(other, TILE + 39_000, BASES[3], 1_000)   # ends on the N
    other[TILE + 40_000] = N
    return [seq, other]


CASES = {"lengths_and_rows": case_lengths_and_rows, "edges": case_edges, "all_a": case_all_a, "n_blocks": case_n_blocks}


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


_contigs, _built = {}, {}


def built(name, settings):
    """[(the contig as bytes, the oracle's rows)]: the contigs of a case once per kind of background, the rows once per settings."""
    from oracle import prf_oracle
    key = (name, settings[3] < 9)
    if key not in _contigs:
        contigs = [c.tobytes() for c in CASES[name](settings)]
        assert all(len(c) == N_SEQ for c in contigs)
        _contigs[key] = contigs
    if (name, settings) not in _built:
        _built[(name, settings)] = [(c, [(s, e, k) for s, e, _ml, k in prf_oracle.detect_rows(c, *settings)]) for c in _contigs[key]]
    return _built[(name, settings)]


def test_cases_hold_what_they_are_built_around():
    """On the CPU: the planted homopolymers are rows of the oracle at k = 1 at the default thresholds (those of 8 letters are not),
    where the cases say they are."""
    settings = DERIVED[0]
    (_seq, rows), = built("lengths_and_rows", settings)
    k1 = [(s, e) for s, e, k in rows if k == 1]
    for length in LENGTHS[1:]:
        assert sum(e - s == length for s, e in k1) >= (8 if length < 5_000 else 4), length
    assert not any(e - s == 8 for s, e in k1)
    for row in ROWS:
        assert sum(s // TILE == 1 and s % T == row for s, _e in k1) >= 3, row
    assert any(s // TILE == 1 and (s % TILE) // T % 64 == 63 and (e - 1) // T > s // T for s, e in k1)     # lane 63 into the next bit
    assert sum(k == 2 and e - s >= 14 for s, e, k in rows) >= 8                                               # the dinucleotide rows
    edges = built("edges", settings)
    starts = [{s: e for s, e, k in rows if k == 1} for _seq, rows in edges]
    assert starts[0][0] == 30 and starts[0][TILE] == TILE + 12 and starts[0][2 * TILE - 5] == 2 * TILE + 15 and starts[0][N_SEQ - 9] == N_SEQ
    assert starts[1][0] == 9 and starts[1][TILE - 5] == TILE + 15 and starts[1][2 * TILE - 11] == 2 * TILE and starts[1][N_SEQ - 9] == N_SEQ
    assert starts[2][TILE - 1] == TILE + 9 and starts[2][2 * TILE - 1] == 2 * TILE + 8
    (_seq, rows), = built("all_a", settings)
    assert rows == [(0, N_SEQ, 1)]
    (seq, rows), (other, rows2) = built("n_blocks", settings)
    k1 = {s: e for s, e, k in rows if k == 1}
    assert k1[TILE + 23_000] == TILE + 23_012 and k1[TILE + 20_000 - 12] == TILE + 20_000
    assert seq.count(b"N") == 3_000 and other.count(b"N") == 1
    k1 = {s: e for s, e, k in rows2 if k == 1}
    assert k1[TILE + 40_001] == TILE + 40_016 and k1[TILE + 39_000] == TILE + 40_000


@pytest.mark.parametrize("settings", SETTINGS, ids=["-".join(map(str, s)) for s in SETTINGS])
@pytest.mark.parametrize("name", list(CASES))
def test_homopolymer_case(ctx, name, settings):
    import prf_native
    derive = {t["k0"]: t.get("derive") for t in prf_native.plan_describe(*settings)["tasks"] if t["kind"]}
    n_rows = 0
    for seq, oracle in built(name, settings):
        g = ctx.load([seq], 50)
        try:
            rows, st = g.scan(*settings)
            assert st.path == 1
            got = [(int(r["start"]), int(r["end"]), int(r["k"])) for r in rows]
            assert got == oracle
            gen, stg = g.scan(*settings, flags=prf_native.SCAN_FORCE_GENERIC)
            assert stg.path == 0 and np.array_equal(rows, gen)
            n_rows += len(got)
        finally:
            g.free()
    print(name, settings, "rows", n_rows, "of them k = 1:", sum(k == 1 for _s, o in built(name, settings) for _a, _b, k in o),
          "derive", (derive.get(1), derive.get(2)))
