"""numpy model of the periodicity matrix (reference utils/plot_utils.py:12-25), for the tests.

The sequence is upper-cased; cell (k, i) of the range [begin, end) is set iff begin <= i, i + k < end and seq[i] == seq[i + k]
as symbols -- N == N is a match, a letter matches only itself; `end` beyond the sequence is clipped to its length.  The
layouts are those of prf_period_bits / prf_period_counts (include/prf.h)."""
import numpy as np


def _symbols(seq):
    if isinstance(seq, str):
        seq = seq.encode("ascii")
    a = np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.where((a >= ord("a")) & (a <= ord("z")), a - 32, a).astype(np.uint8)


def period_cells(seq, kmin, kmax, begin=0, end=None):
    """bool[nk, length]: the cells of the range, column j = position begin + j."""
    a = _symbols(seq)
    end = len(a) if end is None else min(end, len(a))
    s = a[begin:end] if begin < end else a[:0]
    n = len(s)
    cells = np.zeros((kmax - kmin + 1, n), dtype=bool)
    for r, k in enumerate(range(kmin, kmax + 1)):
        if k < n:
            cells[r, :n - k] = s[:n - k] == s[k:]
    return cells


def pack_bits(cells):
    """uint64[nk, ceil(length / 64)]: bit j of word w = column 64 w + j; tail bits zero."""
    nk, n = cells.shape
    words = -(-n // 64)
    padded = np.zeros((nk, words * 64), dtype=np.uint8)
    padded[:, :n] = cells
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(nk, words)


def period_bits(seq, kmin, kmax, begin=0, end=None):
    return pack_bits(period_cells(seq, kmin, kmax, begin, end))


def window_sums(cells, window):
    """uint32[nk, ceil(length / window)]: set cells per window of `window` columns."""
    nk, n = cells.shape
    nw = -(-n // window)
    padded = np.zeros((nk, nw * window), dtype=np.uint32)
    padded[:, :n] = cells
    return padded.reshape(nk, nw, window).sum(axis=2, dtype=np.uint32)


def period_counts(seq, kmin, kmax, window, begin=0, end=None):
    return window_sums(period_cells(seq, kmin, kmax, begin, end), window)


def popcount_per_window(bits, window):
    """The same sums from packed bits (window a multiple of 64): what prf_period_counts must equal."""
    nk, words = bits.shape
    per_word = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1).reshape(nk, words, 64).sum(axis=2, dtype=np.uint32)
    wpw = window // 64
    nw = -(-words // wpw)
    padded = np.zeros((nk, nw * wpw), dtype=np.uint32)
    padded[:, :words] = per_word
    return padded.reshape(nk, nw, wpw).sum(axis=2, dtype=np.uint32)
