"""The CPU model of the local alignment product (include/prf_alignlocal.h): the best local alignment of a window
against the endless repetition of a motif under (match, mismatch, indel) weights.  Three forms of the same thing:
  brute        the definition: every tuple (p, q, a, C), one plain matrix per (p, a);
  one_triples  the wraparound recurrence on explicit triples (score, p, a);
  one          the same recurrence on cells packed into one uint64, in numpy, one step per position: what the GPU tests use.
tests/test_alignlocal_cpu.py checks the three against each other; the library is compared with `local` exactly."""
import numpy as np

import align_model as A

FIELDS = ("score", "first", "end", "start_column", "end_column", "reserved")
DTYPE = [(name, "<u4") for name in FIELDS]
MAX_K, MAX_LEN, MAX_WEIGHT = A.MAX_K, A.MAX_LEN, 16
WEIGHTS = [(2, 7, 7), (1, 1, 1), (2, 3, 5), (16, 16, 16), (16, 1, 1), (1, 16, 16), (3, 1, 2), (2, 5, 1)]

S_SHIFT, P_SHIFT = 29, 10                                   # a cell: score (25 bits) | p (19 bits) | a (10 bits)


def _codes(seq, motif):
    s = A._SEQ[np.frombuffer(seq.encode("ascii") if isinstance(seq, str) else bytes(seq), dtype=np.uint8)]
    return s, A.motif_codes(motif)


def _weights(weights):
    match, mismatch, indel = (int(w) for w in weights)
    assert all(1 <= w <= MAX_WEIGHT for w in (match, mismatch, indel)), weights
    return match, mismatch, indel


# ---- the definition

def brute(seq, motif, weights):
    """(score, first, end, start_column, end_column): over every first position p, start column a, last position q >= p and
    number of letters C >= 1 the global alignment of positions p .. q with M[(a + t) mod k], t < C; the greatest score, then the
    least q, the least end column, the greatest p, the greatest a.  C runs up to (n + 1) k + 2 n."""
    match, mismatch, indel = _weights(weights)
    s, m = _codes(seq, motif)
    n, k = len(s), len(m)
    width = (n + 1) * k + 2 * n
    c = np.arange(width + 1, dtype=np.int64)
    letters = m[(np.arange(k)[:, None] + np.arange(width)[None, :]) % k]        # [a][t]
    best = None
    for p in range(n):
        prev = np.broadcast_to(-c * indel, (k, width + 1)).copy()              # no position against c letters
        for q in range(p, n):
            step = np.where(letters == s[q], match, -mismatch)
            t = np.empty_like(prev)
            t[:, 0] = prev[:, 0] - indel
            t[:, 1:] = np.maximum(prev[:, :-1] + step, prev[:, 1:] - indel)
            prev = np.maximum.accumulate(t + c * indel, axis=1) - c * indel    # letters against nothing, along the row
            top = int(prev[:, 1:].max())
            if top <= 0 or (best is not None and top < best[0]):
                continue
            for a, cc in np.argwhere(prev[:, 1:] == top).tolist():
                key = (-top, q, (a + cc) % k, -p, -a)                          # cc = C - 1
                if best is None or key < best[1]:
                    best = (top, key)
    if best is None:
        return 0, 0, 0, 0, 0
    score, (_, q, end_column, p, a) = best
    return score, -p, q + 1, -a, end_column


# ---- the recurrence on explicit triples

ZERO = (0, 0, 0)


def _sub(v, w):
    return (v[0] - w, v[1], v[2]) if v[0] > w else ZERO


def one_triples(seq, motif, weights):
    match, mismatch, indel = _weights(weights)
    s, m = _codes(seq, motif)
    k = len(m)
    D = [ZERO] * k
    best, where = ZERO, (0, 0)
    for i, b in enumerate(s.tolist()):
        T = []
        for j in range(k):
            din = D[(j - 1) % k]
            if din[0] == 0:
                din = (0, i, j)                                                # a fresh start takes its label here
            diag = (din[0] + match, din[1], din[2]) if m[j] == b else _sub(din, mismatch)
            T.append(max(diag, _sub(D[j], indel)))
        P = [max(_sub(T[jj], (j - jj) * indel) for jj in range(j + 1)) for j in range(k)]
        D = [max(P[j], _sub(P[k - 1], (j + 1) * indel)) for j in range(k)]
        for j in range(k):
            if D[j][0] > best[0]:
                best, where = D[j], (i + 1, j)
    if best[0] == 0:
        return 0, 0, 0, 0, 0
    return best[0], best[1], where[0], best[2], where[1]


# ---- the recurrence on packed cells

def one(seq, motif, weights):
    match, mismatch, indel = _weights(weights)
    s, m = _codes(seq, motif)
    k = len(m)
    assert 1 <= k <= MAX_K and 1 <= len(s) <= MAX_LEN
    unit = np.uint64(1 << S_SHIFT)
    j = np.arange(k, dtype=np.uint64)
    bias = j * np.uint64(indel) * unit
    wrap = (j + np.uint64(1)) * np.uint64(indel) * unit
    m_unit, x_unit, g_unit = np.uint64(match) * unit, np.uint64(mismatch) * unit, np.uint64(indel) * unit
    zero = np.uint64(0)
    D = np.zeros(k, dtype=np.uint64)
    best_score, best_cell, best_end, best_col = 0, 0, 0, 0
    for i, b in enumerate(s.tolist()):
        din = np.roll(D, 1)
        din = np.where(din < unit, (np.uint64(i) << np.uint64(P_SHIFT)) | j, din)
        diag = np.where(m == b, din + m_unit, np.where(din >= x_unit + unit, din - x_unit, zero))
        T = np.maximum(diag, np.where(D >= g_unit + unit, D - g_unit, zero))
        P = np.maximum.accumulate(T + bias) - bias
        last = P[k - 1]
        D = np.maximum(P, np.where(last >= wrap + unit, last - wrap, zero))
        scores = D >> np.uint64(S_SHIFT)
        col = int(np.argmax(scores))                                           # the first of equal maxima
        if int(scores[col]) > best_score:
            best_score, best_cell, best_end, best_col = int(scores[col]), int(D[col]), i + 1, col
    if best_score == 0:
        return 0, 0, 0, 0, 0
    return best_score, (best_cell >> P_SHIFT) & 0x7FFFF, best_end, best_cell & 0x3FF, best_col


def local(seq, rows, motifs, weights=(2, 7, 7), begin=0, end=None):
    """Rows of DTYPE for the windows `rows` (fields start, end, k, relative to begin) of seq[begin:end], in their order."""
    if isinstance(seq, (bytes, bytearray)):
        seq = bytes(seq).decode("ascii")
    s = seq[begin:len(seq) if end is None else min(end, len(seq))]
    out = np.zeros(len(rows), dtype=DTYPE)
    for at, (start, stop, motif) in enumerate(zip(rows["start"].tolist(), rows["end"].tolist(), A.split_motifs(rows, motifs))):
        assert 0 <= start < stop <= len(s), (start, stop, len(s))
        out[at] = one(s[start:stop], motif, weights) + (0,)
    return out


def bound(weights, subs, ins, dele, matches):
    """The score of an alignment with these counts."""
    match, mismatch, indel = weights
    return match * matches - mismatch * subs - indel * (ins + dele)


same = A.same
