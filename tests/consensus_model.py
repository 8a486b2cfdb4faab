"""The CPU model of the consensus product (include/prf_consensus.h): plain Python over the string.  The tests compare
the library with it exactly; tests/test_consensus_cpu.py checks it against an independent brute force first."""
import numpy as np

FIELDS = ("offset", "agree", "acgt", "k", "reserved")
DTYPE = [("offset", "<u8"), ("agree", "<u8"), ("acgt", "<u8"), ("k", "<u4"), ("reserved", "<u4")]
REPEAT_DTYPE = [("start", "<u8"), ("end", "<u8"), ("k", "<u4"), ("reserved", "<u4")]
BASES = "ACGT"


def column_counts(seq, start, end, k):
    """count[p][b] of the repeat [start, end) of period k of seq: a (k, 4) array."""
    s = seq.upper()
    counts = np.zeros((k, 4), dtype=np.uint32)
    for p in range(min(k, end - start)):
        column = s[start + p:end:k]
        for b, letter in enumerate(BASES):
            counts[p, b] = column.count(letter)
    return counts


def letters_of(counts):
    """The consensus letters of a (k, 4) array of counts: the largest count, ties to the first of A, C, G, T; N for an empty column."""
    best = counts.argmax(axis=1)                       # the first of equal maxima
    return "".join(BASES[b] if row[b] else "N" for row, b in zip(counts.tolist(), best.tolist()))


def repeats(*rows):
    """Rows (start, end, k) as the array the calls take."""
    out = np.zeros(len(rows), dtype=REPEAT_DTYPE)
    for at, (start, end, k) in enumerate(rows):
        out[at] = (start, end, k, 0)
    return out


def consensus(seq, rows, begin=0, end=None):
    """(rows of DTYPE, motifs as a list of str, counts of (sum of k, 4)) of the repeats `rows` (fields start, end, k, relative to
    begin) of seq[begin:end] (str or bytes), in their order."""
    if isinstance(seq, (bytes, bytearray)):
        seq = bytes(seq).decode("ascii")
    s = seq[begin:len(seq) if end is None else min(end, len(seq))]
    out = np.zeros(len(rows), dtype=DTYPE)
    motifs, tables, offset = [], [np.zeros((0, 4), dtype=np.uint32)], 0
    for at, (start, stop, k) in enumerate(zip(rows["start"].tolist(), rows["end"].tolist(), rows["k"].tolist())):
        assert 0 <= start < stop <= len(s) and k >= 1, (start, stop, k, len(s))
        counts = column_counts(s, start, stop, k)
        out[at] = (offset, int(counts.max(axis=1).sum(dtype=np.uint64)), int(counts.sum(dtype=np.uint64)), k, 0)
        motifs.append(letters_of(counts))
        tables.append(counts)
        offset += k
    return out, motifs, np.concatenate(tables)


def same(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and a.tobytes() == b.tobytes()
