"""numpy model of the exact tasks' flag rule with echo suppression (csrc/vscan_tasks.h, exact_stream).

An exact task of motif size k flags a stream when a run of >= M matches at distance k starts in it.  For k = 2, 3, 4 on a clean
tile it leaves out the starts whose run is the echo of a shorter motif: the k letters have a period k / p for a prime p | k.
The kernel does not make that test at the start t but once per segment of S start rows, at the first multiple j of S at or
after t (S = the largest power of two <= min(M + 1, 8)).  Both rules are here, position by position, so that they can be compared
start for start (tests/test_echo_flags_cpu.py) and counted per stream before the device is asked (tests/test_echo_flags_gpu.py).
Nothing of this runs on the device."""
import numpy as np

TILE = 65_536
T = 32                   # positions per stream; stream s of a tile = lane s % 64, bit s // 64
SMALL_M = 15             # M(k) below this: exact / coarse task, else group task
COARSE_M = 9             # ... and from here on the coarse form, which is not suppressed
ECHO_K = (2, 3, 4)       # the motif sizes whose exact task suppresses echoes


def min_matches(k, min_repeats, min_span):
    return max((min_repeats - 1) * k, min_span - k)


def segment(M):
    """Start rows per sample: the largest power of two <= min(M + 1, 8)."""
    s = 1
    while 2 * s <= min(M + 1, 8):
        s *= 2
    return s


def cofactors(k):
    return [k // p for p in range(2, k + 1) if k % p == 0 and all(p % q for q in range(2, p))]


def as_array(seq):
    return np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)


def matches(a, d, n):
    """m[i], i < n: position i equals position i + d (False where i + d lies behind the sequence)."""
    m = np.zeros(n, dtype=bool)
    top = min(n, len(a) - d)
    if top > 0:
        m[:top] = a[:top] == a[d:d + top]
    return m


def all_of(m, width, n):
    """w[i], i < n: m[i .. i+width-1] all hold (m is long enough)."""
    w = np.ones(n, dtype=bool)
    for q in range(width):
        w &= m[q:q + n]
    return w


def starts(a, k, M):
    """start[t]: a run of >= M matches at distance k begins at position t (position 0: its M positions match)."""
    n = len(a)
    m = matches(a, k, n + M)
    win = all_of(m, M, n)
    st = win.copy()
    st[1:] &= ~m[:n - 1]
    return st


def echo(a, k):
    """e[j], j <= len(a): the k letters from position j on are a power of a shorter word.  Only read inside runs."""
    n = len(a) + 1
    e = np.zeros(n, dtype=bool)
    for d in cofactors(k):
        e |= all_of(matches(a, d, n + k), k - d, n)
    return e


def sample_row(t, S):
    """The first multiple of S at or after t."""
    return (t + S - 1) // S * S


def verdicts(a, k, M):
    """For every start t (ascending): (t, echo at t, echo at the sampled row)."""
    a = as_array(a)
    t = np.flatnonzero(starts(a, k, M))
    e = echo(a, k)
    return t, e[t], e[sample_row(t, segment(M))]


def stream_counts(seq, tile, k, M):
    """Streams of a clean tile, as three counts: those that hold a start; those that hold a start with a primitive motif; those
    the kernel's sampled rule flags (for k in ECHO_K; else every stream with a start).  The tile's first position counts as a
    start when its M positions match (the conservative first stream): it is in the first and the third count only if so, and in
    the second only if it is a true start."""
    a = as_array(seq)
    lo = tile * TILE
    hi = min(len(a), lo + TILE)
    st = starts(a, k, M)
    e = echo(a, k)
    m = matches(a, k, len(a) + M)
    first_win = bool(all_of(m[lo:], M, 1)[0])
    pos = np.arange(lo, hi)
    true_start = np.zeros(TILE, dtype=bool)
    true_start[:hi - lo] = st[lo:hi]
    seen = true_start.copy()                      # what the kernel sees: the row before the tile reads as a mismatch
    seen[0] |= first_win
    prim = np.zeros(TILE, dtype=bool)
    prim[:hi - lo] = ~e[pos]
    if k in ECHO_K and M < COARSE_M:
        smp = np.zeros(TILE, dtype=bool)
        smp[:hi - lo] = ~e[np.minimum(sample_row(pos - lo, segment(M)) + lo, len(a))]
    else:
        smp = np.ones(TILE, dtype=bool)
    per_stream = lambda x: int(x.reshape(TILE // T, T).any(axis=1).sum())
    return per_stream(seen), per_stream(true_start & prim), per_stream(seen & smp)


def count_flags(seq, tile, settings):
    """(stream, exact task) pairs of a clean tile over the exact-form tasks (M < 9) of the settings:
    (with a start, with a primitive start, flagged by the sampled rule)."""
    kmin, kmax, r, span = settings
    tot = np.zeros(3, dtype=np.int64)
    for k in range(kmin, kmax + 1):
        M = min_matches(k, r, span)
        if M < COARSE_M:
            tot += stream_counts(seq, tile, k, M)
    return tuple(int(x) for x in tot)
