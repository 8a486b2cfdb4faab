"""The inputs of tests/test_task_variants_gpu.py, built on the CPU with numpy: runs of the minimal length for every exact-task
variant (K, M) and every group-task form of the fused scan kernel (csrc/vscan_tasks.h), and the rows they must and must not give.
tests/test_task_variants_cpu.py asserts what the cases are built around -- the plans, the oracle's rows at the constructs, the
caps per tile -- without a GPU.  Nothing here touches the device.

A construct is a primitive motif of size k repeated over exactly `length` positions, with the base on either side chosen to break
the period: `length` = M + k gives exactly M matches at distance k (threshold: a row), M + k - 1 gives M - 1 (one below: no row).
Layout (csrc/pack.hip, csrc/vscan_tasks.h): a tile has 65 536 positions; stream s of a tile covers the positions [32 s, 32 s + 32),
lane = s % 64, bit = s // 64.  Constructs lie three streams apart (gcd(3, 64) = 1: they visit every lane), dealt over the four
quarters of a tile in turn so that no quarter's row list fills up."""
import functools

import numpy as np

import prf_native

TILE = 65_536
T = 32                   # positions per stream
STREAMS = TILE // T      # 2 048 streams of a tile, 512 per quarter
SMALL_M = 15             # csrc/prf_plan.h: M(k) below this -> exact task
FLAG_CAP = 960           # (stream, exact task) flags of a tile
QCAP = 112               # rows of a quarter tile in its LDS sublist
REC_CAP = 192            # group-task records of a tile
MAX_FLAGS = 720          # what a case may hold per tile: 3/4 of FLAG_CAP run starts,
MAX_QROWS = 100          # rows per quarter tile,
MAX_GROUP = 120          # group-task constructs
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
A = BASES[0]
N = np.frombuffer(b"N", dtype=np.uint8)[0]
VARIANTS = [(K, M) for K in range(1, SMALL_M) for M in range(K, SMALL_M)]     # the 105 device functions per image width


def min_matches(k, min_repeats, min_span):
    """The planner's rule (prf_plan_min_matches)."""
    return max((min_repeats - 1) * k, min_span - k)


def single_setting(K, M):
    """(kmin, kmax, min_repeats, min_span) whose plan is the one exact task (K, M)."""
    return (K, K, 2, K + M) if M > K else (K, K, 2, 1)


def exact_variants_of(settings):
    """The (K, M) of the exact tasks in the plan of these settings, read from the library's planner."""
    plan = prf_native.plan_describe(*settings)
    assert plan["path"] == "fused", settings
    return sorted((t["k0"], t["kind"]) for t in plan["tasks"] if t["kind"])


def group_tasks_of(settings):
    """[(k0, valid, stride, half, [(k, M)])] of the group tasks in the plan of these settings."""
    plan = prf_native.plan_describe(*settings)
    assert plan["path"] == "fused", settings
    out = []
    for t in plan["tasks"]:
        if t["kind"] == 0:
            sizes = [(t["k0"] + i, min_matches(t["k0"] + i, settings[2], settings[3])) for i in range(8) if t["valid"] >> i & 1]
            out.append((t["k0"], t["valid"], t["stride"], (t["valid"] & 0xF0) == 0, sizes))
    return sorted(out)


# ---- letters ------------------------------------------------------------------------------------------------------------------
def random_bases(seed, n):
    return BASES[np.random.RandomState(seed).randint(0, 4, n)].copy()


def quiet_bases(seed, n, ks):
    """Seeded bases in which no position equals the one k before it, for every k in ks (at most three sizes)."""
    assert 1 <= len(ks) <= 3
    rng = np.random.RandomState(seed)
    if len(ks) == 1:                                   # k interleaved walks with non-zero steps
        k = ks[0]
        rows = (n + k - 1) // k + 1
        walk = (rng.randint(0, 4, k)[None, :] + np.cumsum(rng.randint(1, 4, (rows, k)), axis=0)) % 4
        return BASES[walk.reshape(-1)[:n]].copy()
    idx = rng.randint(0, 4, n).tolist()
    pick = rng.randint(0, 4, n).tolist()
    for i in range(n):
        free = [b for b in (0, 1, 2, 3) if all(i < k or b != idx[i - k] for k in ks)]
        idx[i] = free[pick[i] % len(free)]
    return BASES[np.array(idx)]


def is_primitive(m):
    k = len(m)
    return all(k % d or not np.array_equal(m, np.tile(m[:d], k // d)) for d in range(1, k))


def primitive_motif(rng, k):
    while True:
        m = BASES[rng.randint(0, 4, k)]
        if is_primitive(m):
            return m


def a_rich_motif(k, a_at):
    """A motif of A with one C, and an A at index a_at (k = 1: A)."""
    m = np.full(k, A, dtype=np.uint8)
    if k > 1:
        m[(a_at + 1) % k] = BASES[1]
    return m


def other_base(*bs):
    return next(b for b in BASES if b not in bs)


def plant(seq, pos, motif, length):
    """seq[pos : pos+length] = copies of the motif, cut at `length`.  The base in front differs from the ones k behind and k in
    front of it, the base behind likewise: the period breaks on either side and no new match at distance k arises."""
    k = len(motif)
    seq[pos:pos + length] = np.tile(motif, length // k + 1)[:length]
    if pos > 0:
        seq[pos - 1] = other_base(seq[pos - 1 + k], seq[pos - 1 - k] if pos - 1 - k >= 0 else seq[pos - 1 + k])
    end = pos + length
    seq[end] = other_base(seq[end - k], seq[end + k])


def run_starts(a, k, M):
    """start[t]: a run of >= M matches at distance k begins at position t (numpy; N never matches)."""
    n = len(a)
    m = np.zeros(n + M + 1, dtype=bool)
    m[:n - k] = (a[:n - k] == a[k:]) & (a[:n - k] != N)
    win = np.ones(n, dtype=bool)
    for q in range(M):
        win &= m[q:q + n]
    st = win.copy()
    st[1:] &= ~m[:n - 1]
    return st


def per_tile(flags, n_tiles):
    """Count of set positions per tile."""
    out = np.zeros(n_tiles, dtype=np.int64)
    pos = np.flatnonzero(flags)
    np.add.at(out, pos // TILE, 1)
    return out


class Placer:
    """Hands out the first positions of streams inside one tile: three streams apart (more for a long construct), the four
    quarters of the tile in turn, from the stream `first` of each quarter on."""

    def __init__(self, tile, first=(1, 1, 1, 1), per_quarter=STREAMS // 4):
        self.base = tile * TILE
        self.cursor = list(first)
        self.turn = 0
        self.count = 0
        self.limit = per_quarter

    def next(self, off, length):
        need = max(3, (off + length + 2 + T - 1) // T + 1)
        need += 1 - need % 2                                   # odd: every lane is visited
        q = self.turn % 4
        self.turn += 1
        s = self.cursor[q]
        self.cursor[q] += need
        assert self.cursor[q] <= self.limit, "quarter full"
        self.count += 1
        return self.base + (512 * q + s) * T + off


class Case:
    """One contig and what it is built around: `want` rows (start, end, k) and `never` (start, k): no row of size k starts there."""

    def __init__(self, seq, settings):
        self.arr = seq
        self.settings = settings
        self.want = []
        self.never = []
        self.n_group = {}            # tile -> group-task constructs

    def put(self, pos, motif, length, row):
        plant(self.arr, pos, motif, length)
        (self.want.append((pos, pos + length, len(motif))) if row else self.never.append((pos, len(motif))))

    @property
    def seq(self):
        return self.arr.tobytes()

    @property
    def n_tiles(self):
        return (len(self.arr) + TILE - 1) // TILE

    def threshold_streams(self):
        return len({s // T for s, _e, _k in self.want})


# ---- exact tasks: one contig per (K, M) ------------------------------------------------------------------------------------------
def exact_len(mixed):
    """The clean contig has a third clean tile, so that a run can cross from one clean tile into another."""
    return (3 if mixed else 4) * TILE + 64


# stream bits of tile 1 (64 streams each).  The every-offset runs take the bits 0, 8-9, 17-18 and 26-27.
LANE0_BITS = (3, 4, 5, 6, 7, 11)       # threshold / one below at the offsets 0, 25, 31 in the streams of lane 0 of these bits
LANE63_BITS = (12, 13, 14, 15, 19, 20)  # ... and of lane 63: a run of the offsets 25 and 31 reaches into lane 0 of the next bit
PAIR_BIT, POWER_BIT, N_BIT, LONE_N_BIT = 21, 22, 23, 30
EDGE_OFFSETS = (0, 25, 31)


def exact_background(K, M, seed, n):
    """Random bases; where their own run starts (>= M matches at distance K) would take more than half of a tile's flag list
    (M <= 3), bases in which no position equals the one K before it."""
    seq = random_bases(seed, n)
    if per_tile(run_starts(seq, K, M), n // TILE + 1)[:n // TILE].max() > FLAG_CAP // 2:
        seq = quiet_bases(seed, n, (K,))
    return seq


@functools.lru_cache(maxsize=32)
def exact_case(K, M, mixed):
    """One contig of 4 tiles + 64 positions for the exact-task variant (K, M), scanned with single_setting(K, M): the tiles 0, 1
    and 2 are clean, tile 3 (the next one holds the contig's end) is mixed.  In tile 1:
    * threshold and one-below runs at every row offset 0 .. 31;
    * the same at the offsets 0, 25, 31 in streams of lane 0 with bit > 0 (row -1 is row 31 of lane 63 one bit down) and of lane
      63; the threshold run at offset 31 of lane 63 begins in the stream before a lane-0 stream, which must not find it again;
    * a threshold run at the tile's first position (lane 0, bit 0: the conservative row -1);
    * a threshold run from the tile's last stream into tile 2, from a clean tile into a clean one: tile 1 reads it in the rows of
      virtual lane 64, tile 2 sees it in progress at its conservative first row and must not report it; and one from tile 2's
      last stream into the mixed tile 3;
    * two threshold runs in one stream whose starts lie M + 1 rows apart, the second at row 31;
    * for every proper divisor d of K a run of M + K positions of a word of size d: no row at size K.
    mixed: a contig of 3 tiles + 64 positions with the same constructs, but at the edges a run from tile 0's last stream into tile 1
    and one from tile 1's into tile 2, and a lone N in tile 1 (class 1 for every tile), at least 2 kb from every construct, and runs of a
    motif of A's and one C -- a not-ACGT position reads as A in the image, so the image sees these runs one match longer than
    they are -- with an N directly in front (threshold / one below, offsets 0, 5, 31), directly behind (the same), and one run of
    2 (M + K) + 1 positions with an N in its middle: two rows."""
    rng = np.random.RandomState(1000 + 20 * K + M)
    case = Case(exact_background(K, M, 5000 + 20 * K + M, exact_len(mixed)), single_setting(K, M))
    case.K, case.M = K, M
    seq = case.arr
    L = M + K
    stream = lambda bit, lane: TILE + (bit * 64 + lane) * T
    # every offset, threshold and one below, dealt over the quarters, 16 to each: the lanes 1, 4, .. 46 in the first, 49 .. 94 in
    # the second, and so on -- every lane once
    pl = Placer(1, first=(1, 49, 97, 145), per_quarter=3 * 64 + 2)
    for off in range(T):
        for length, row in ((L, True), (L - 1, False)):
            case.put(pl.next(off, length), primitive_motif(rng, K), length, row)
    # lane 0 (bit > 0) and lane 63
    for lane, bits in ((0, LANE0_BITS), (63, LANE63_BITS)):
        for i, off in enumerate(EDGE_OFFSETS):
            case.put(stream(bits[2 * i], lane) + off, primitive_motif(rng, K), L, True)
            case.put(stream(bits[2 * i + 1], lane) + off, primitive_motif(rng, K), L - 1, False)
    # the tile's edges
    if mixed:
        case.put(TILE - min(5, L - 1), primitive_motif(rng, K), L, True)       # from tile 0's last stream into tile 1
    else:
        case.put(TILE, primitive_motif(rng, K), L, True)                       # tile 1's first position
        case.put(3 * TILE - min(6, L - 1), primitive_motif(rng, K), L, True)   # from tile 2's last stream into tile 3
    case.put(2 * TILE - min(7, L - 1), primitive_motif(rng, K), L, True)       # from tile 1's last stream into tile 2
    # two starts in one stream, M + 1 rows apart: rows 30 - M and 31
    t0 = stream(PAIR_BIT, 5) + 30 - M
    for _try in range(200):
        w = primitive_motif(rng, K)
        plant(seq, t0, w, L)
        x = t0 + L                                      # the letter that ends the first run; the second run's motif holds it
        for c in BASES:
            if c == seq[x - K]:
                continue
            seq[x] = c
            for i in range(t0 + M + 1, t0 + 2 * M + 1):
                seq[i + K] = seq[i]
            if is_primitive(seq[t0 + M + 1:t0 + M + 1 + K]):
                break
        else:
            continue
        break
    else:
        raise AssertionError("no pair of runs")
    e2 = t0 + 2 * M + 1 + K
    seq[e2] = other_base(seq[e2 - K], seq[e2 + K])
    case.want += [(t0, t0 + L, K), (t0 + M + 1, e2, K)]
    # powers of a shorter word
    for i, d in enumerate(d for d in range(1, K) if K % d == 0):
        pos = stream(POWER_BIT, 2 + 3 * i) + (7 * i + 3) % T
        plant(seq, pos, primitive_motif(rng, d), L)
        case.never.append((pos, K))
    if mixed:
        s = 1
        for off in (0, 5, 31):
            for length, row in ((L, True), (L - 1, False)):
                pos = stream(N_BIT, s) + off                       # N in front: the letter K behind it is the motif's last
                case.put(pos, a_rich_motif(K, K - 1), length, row)
                seq[pos - 1] = N
                pos = stream(N_BIT, s + 3) + off                   # N behind: the letter K in front of it is an A
                case.put(pos, a_rich_motif(K, (length - K) % K), length, row)
                seq[pos + length] = N
                s += 6
        pos = stream(N_BIT, s) + 9                                 # N in the middle
        w = primitive_motif(rng, K)
        plant(seq, pos, w, 2 * L + 1)
        seq[pos + L] = N
        case.want += [(pos, pos + L, K), (pos + L + 1, pos + 2 * L + 1, K)]
        case.lone_n = stream(LONE_N_BIT, 32) + 11
        seq[case.lone_n] = N
        assert all(abs(case.lone_n - p) >= 2048 + 64 for p, _e, _k in case.want) and all(abs(case.lone_n - p) >= 2048 + 64 for p, _k in case.never)
    case.want.sort()
    return case


def flag_bound(seqs, K, M):
    """An upper bound of the streams the one task (K, M) flags on these contigs, from the tasks' rules (csrc/vscan_tasks.h) applied
    to the image, in which a not-ACGT position -- the gap behind a contig as well -- reads as A.  W = M rows (exact form), or the
    G C rows of a window of the coarse form.  A stream is flagged
    * by a window that follows a row (coarse: a group) with a mismatch: then a run of >= W matches starts in the stream -- or,
      coarse form only, in the last G - 1 rows of the stream before it or in row 0 of the next one (window j = T / G), so that a
      start flags at most two streams;
    * on a mixed tile also when its first W rows match: a run of >= W matches starts at its row 0 (counted above) or covers it;
    * the first stream of a tile, whose row -1 counts as a mismatch: one per tile.
    Echo suppression only takes flags away.  The kernel comes within 3 % of this bound at some variants: the bound pins the
    flagging rule.  A change that flags more on purpose -- another conservative row, a coarser window -- has to change this
    function with it, and say why."""
    coarse = M >= 9
    G = (4 if M >= 11 else 2) if coarse else 1
    W = G * ((M + 1) // G - 1) if coarse else M
    total = 0
    for seq in seqs:
        a = np.frombuffer(seq, dtype=np.uint8)
        n = len(a)
        img = np.concatenate([np.where(np.isin(a, BASES), a, A), np.full(256, A, dtype=np.uint8)])
        m = img[:n + W] == img[K:K + n + W]
        win = np.ones(n, dtype=bool)
        for q in range(W):
            win &= m[q:q + n]
        starts = win.copy()
        starts[1:] &= ~m[:n - 1]
        covered = win[T::T] & m[T - 1:n - 1:T]          # the stream's first W rows match and so does the row before it
        total += (2 if coarse else 1) * int(starts.sum()) + int(covered.sum()) + (n + TILE - 1) // TILE
    return total


# ---- span sweeps: every exact task of a plan beside its group tasks -----------------------------------------------------------------
SWEEP_SPANS = tuple(range(8, 29))
SWEEP72 = (1, 22)        # (kmin, kmax), min_repeats 2: image of 72 virtual lanes
SWEEP80 = (1, 264)       # ... of 80: the group task of the sizes 256 .. 263 reads row 24 + 256 + 15 of its lane's stream
SWEEP_QUIET = (4,)       # no position of the background equals the one 4 before it: no runs of the sizes 1, 2 and 4 but the planted
                         # ones (at span 8 random bases give 330 rows per tile, two thirds of them at size 4)


def sweep_settings(krange, span):
    return (krange[0], krange[1], 2, span)


def sweep_lengths(k):
    """The lengths a run of size k is planted with: for every span of the sweep the threshold max(2 k, span) and one below."""
    lo = max(2 * k, SWEEP_SPANS[0])
    return list(range(lo - 1, max(lo, SWEEP_SPANS[-1]) + 1))


class SweepCase:
    def __init__(self, seq, runs, kmax):
        self.seq, self.runs, self.kmax = seq, runs, kmax       # runs: (pos, length, k)
        self.n_tiles = (len(seq) + TILE - 1) // TILE

    def expect(self, span):
        """(want, never) at this span: the runs of exactly the threshold length, and of one below."""
        want, never = [], []
        for pos, length, k in self.runs:
            thr = max(2 * k, span)
            if length == thr:
                want.append((pos, pos + length, k))
            elif length == thr - 1:
                never.append((pos, k))
        return want, never


@functools.lru_cache(maxsize=None)
def sweep_case(n_tiles, offsets, reps, kmax, seed, extra=(), n_mixed=1):
    """A contig of n_tiles + 64 positions with `reps` primitive runs of every size 1 .. min(kmax, 22) and every length of
    sweep_lengths: the first of them in a mixed tile, the others in the clean tiles in turn, each at a row offset drawn from
    `offsets`; `extra`: larger sizes k, with 2 k - 1 and with 2 k positions, in the same way.  The last whole tile is mixed; with
    n_mixed = 2 an N near its end makes the tile before it mixed as well, and the two take the runs in turn."""
    n = n_tiles * TILE + 64
    arr = quiet_bases(seed, n, SWEEP_QUIET)
    rng = np.random.RandomState(seed + 1)
    placers = [Placer(t) for t in range(n_tiles)]
    runs = []
    i = 0
    for k in list(range(1, min(kmax, 22) + 1)) + list(extra):
        for length in (sweep_lengths(k) if k <= 22 else (2 * k - 1, 2 * k)):
            for r in range(reps):
                off = offsets[rng.randint(len(offsets))]
                tile = n_tiles - 1 - i % n_mixed if r == 0 else i % (n_tiles - n_mixed)
                i += r == reps - 1
                pos = placers[tile].next(off, length)
                plant(arr, pos, primitive_motif(rng, k), length)
                runs.append((pos, length, k))
    if n_mixed == 2:
        lone_n = n_tiles * TILE - 40 * T
        assert all(pos + length + 300 < lone_n for pos, length, _k in runs)
        arr[lone_n] = N
    return SweepCase(arr.tobytes(), runs, kmax)


def sweep72_case():
    return sweep_case(5, (0, 13, 25, 31, 7), 3, SWEEP72[1], 72)


SWEEP80_EXTRA = (100, 255, 256, 263, 264)   # 256 .. 263: the group task that reads furthest, into the image's last virtual lanes
SWEEP80_SPLIT = 28                          # the oracle's rows of the wide sweep: the sizes up to here per span, the rest once


def sweep80_case():
    return sweep_case(4, (0, 31, 17, 25, 8), 2, SWEEP80[1], 80, SWEEP80_EXTRA, n_mixed=2)


@functools.lru_cache(maxsize=None)
def sweep80_large_rows():
    from oracle import prf_oracle
    return prf_oracle.detect_rows(sweep80_case().seq, SWEEP80_SPLIT + 1, SWEEP80[1], 2, SWEEP_SPANS[-1])


def sweep80_oracle(span):
    """The oracle's rows (start, end, motif length, k) of the wide sweep's contig at (1, 264, 2, span), from two calls: the sizes
    1 .. 28 at this span, and the sizes 29 .. 264 once for all spans.  The oracle tests every motif for N at every mismatch, so its
    time goes with the sum of the sizes: 3 s for one call over 1 .. 264 on this contig, 0.1 s for 1 .. 28.  For k >= 29 both of its
    length filters are decided by min_repeats k = 2 k >= 58 > span, so those rows are the same at every span of the sweep; and no
    row of one call can meet a row of the other in the oracle's table of (start, end), where the shorter motif wins: a stretch
    of >= 2 k' positions with the periods k < k' has the period gcd(k, k'), so the longer motif is no primitive one and gives no
    row.  tests/test_task_variants_cpu.py compares the two calls with the single one at the sweep's first span."""
    from oracle import prf_oracle
    small = prf_oracle.detect_rows(sweep80_case().seq, SWEEP80[0], SWEEP80_SPLIT, 2, span)
    return sorted(small + sweep80_large_rows(), key=lambda r: (r[0], r[1]))


# ---- group tasks -------------------------------------------------------------------------------------------------------------------
# (kmin, kmax, min_repeats, min_span) -> the blocks of row offsets of its constructs, a contig each.  What the planner makes of the
# settings is asserted on the CPU (tests/test_task_variants_cpu.py): the six forms {stride 1, 2, 4} x {half, full}, a smallest M of
# exactly 8 S + 7 per stride, valid masks with holes at either end.
EVERY_OFFSET = (tuple(range(T)),)
GROUP_SETTINGS = {
    (8, 15, 2, 30): EVERY_OFFSET,     # full, stride 1, M = 22 .. 15
    (8, 15, 2, 38): EVERY_OFFSET,     # full, stride 2, M = 30 .. 23
    (8, 15, 2, 54): EVERY_OFFSET,     # full, stride 4, M = 46 .. 39
    (15, 22, 2, 1): EVERY_OFFSET,     # M = k: 15 is the lowest size of a full task (hole at the low end); 20-22 a half task, stride 1
    (23, 26, 2, 1): EVERY_OFFSET,     # stride 2, tight at k = 23, holes at both ends
    (39, 42, 2, 1): EVERY_OFFSET,     # stride 4, tight at k = 39, holes at both ends
    (8, 26, 2, 1): EVERY_OFFSET,      # exact tasks 8-14 beside: full stride 1, half stride 1, half stride 2 with valid = 7
    (48, 50, 2, 1): EVERY_OFFSET,     # half, stride 4
    # seven group tasks and no exact one: the sizes 1-7 in a task of k0 = 0, a full stride-1 task with valid = 255, a half stride-4
    # task last.  A run of a short motif echoes at every multiple of its size -- a record each -- so the constructs of this one
    # take some 50 tiles: four contigs of eight offsets each.
    (1, 50, 2, 40): tuple(tuple(range(b, b + 8)) for b in range(0, T, 8)),
}
GROUP_N_VARIANT = (8, 26, 2, 1)    # this one a second time with an N inside a middle tile
MAX_WEIGHT = 150                   # per tile: the records the constructs are expected to give (REC_CAP = 192)


@functools.lru_cache(maxsize=None)
def group_case(settings, with_n=False, block=0):
    """For every motif size of every group task of the plan: threshold and one-below runs at the row offsets of block `block` of
    GROUP_SETTINGS (every offset, but for one setting), in clean tiles; the contig's last whole tile, which is mixed, holds a
    threshold and a one-below run of every size as well.  A clean tile takes constructs
    until it has MAX_GROUP of them or their weights reach MAX_WEIGHT -- a construct's weight is the number of sizes in group tasks
    at which it has 8 matches: the records it can give -- so that the records travel through the tile's list of REC_CAP."""
    offsets = GROUP_SETTINGS[settings][block]
    sizes = [km for _k0, _v, _s, _h, ks in group_tasks_of(settings) for km in ks]
    weight = lambda k, length: sum(1 for k2, _m in sizes if k2 % k == 0 and length - k2 >= 8)
    todo = [(k, off, length, row) for k, M in sizes for off in offsets for length, row in ((M + k, True), (M + k - 1, False))]
    tiles, n, w = [], 0, 0                              # tile index (before the N tile is put in) per construct
    for k, _off, length, _row in todo:
        if n == MAX_GROUP or w + weight(k, length) > MAX_WEIGHT:
            n, w = 0, 0
            tiles.append(tiles[-1] + 1)
        else:
            tiles.append(tiles[-1] if tiles else 0)
        n, w = n + 1, w + weight(k, length)
    n_clean = tiles[-1] + 1
    skip = n_clean // 2 if with_n else -1           # (with_n) a tile without constructs but one N: it and the one before are mixed
    n_tiles = n_clean + 1 + (1 if with_n else 0)
    seed = 9000 + settings[0] * 7 + settings[1] * 3 + settings[3] + 1000 * block
    case = Case(random_bases(seed, n_tiles * TILE + 64), settings)
    rng = np.random.RandomState(seed + 1)
    placers = {t: Placer(t) for t in range(n_tiles)}
    for (k, off, length, row), t in zip(todo, tiles):
        t += 1 if with_n and t >= skip else 0
        case.put(placers[t].next(off, length), primitive_motif(rng, k), length, row)
    last = n_tiles - 1
    for j, (k, M) in enumerate(sizes):
        for length, row in ((M + k, True), (M + k - 1, False)):
            case.put(placers[last].next((5 * j + 3 + 8 * block) % T, length), primitive_motif(rng, k), length, row)
    case.n_group = {t: p.count for t, p in placers.items()}
    if with_n:
        case.lone_n = skip * TILE + 30_000
        case.arr[case.lone_n] = N
    case.want.sort()
    return case


# name -> (settings, with an N in a middle tile, block of offsets)
GROUP_CASES = {"_".join(map(str, s)) + ("_o%d" % blocks[b][0] if len(blocks) > 1 else ""): (s, False, b)
               for s, blocks in GROUP_SETTINGS.items() for b in range(len(blocks))}
GROUP_CASES["_".join(map(str, GROUP_N_VARIANT)) + "_N"] = (GROUP_N_VARIANT, True, 0)


def group_cases():
    """name -> Case"""
    return {name: group_case(*args) for name, args in GROUP_CASES.items()}


def group_records_bound(seq, settings, n_tiles):
    """Per tile, an upper bound of the records its group tasks list (one per lane and motif size with a flagged stream): the
    streams that hold an examined aligned group of 8 rows matching throughout, by the rule of a mixed tile (a clean tile's
    stride-1 task counts fewer)."""
    a = np.frombuffer(seq, dtype=np.uint8)
    n = n_tiles * TILE
    out = np.zeros(n_tiles, dtype=np.int64)
    for _k0, _valid, stride, _half, sizes in group_tasks_of(settings):
        for k, _M in sizes:
            m = np.zeros(n, dtype=bool)
            top = min(n, len(a) - k)
            m[:top] = (a[:top] == a[k:k + top])        # (N reads as A in the image: N = N counts, an over-estimate here)
            grp = m.reshape(-1, 8).all(axis=1).reshape(-1, 4)[:, ::stride].any(axis=1)       # per stream
            lanes = grp.reshape(n_tiles, 32, 64).any(axis=1)
            out += lanes.sum(axis=1)
    return out
