"""The CPU model of the alignment-path product (include/prf_alignpath.h): align_model's forward recurrence in numpy, one
step per position, keeping the two bits of every cell (from_ins, from_del), then the walk back in plain Python.  The tests compare
the library with it exactly; tests/test_alignpath_cpu.py pins it to an independent full-matrix traceback on explicit triples
first."""
import numpy as np

import align_model as A

INS, SUB, COLUMN = 0x8000, 0x4000, 0x03FF
MAX_POSITIONS = 1 << 30
_U = np.uint64


def _bytes(text):
    return np.frombuffer(text.encode("ascii") if isinstance(text, str) else bytes(text), dtype=np.uint8)


def forward(s, m):
    """(cells after the last position, from_ins, from_del) for base codes s and motif codes m; the bits as (n, k) arrays."""
    k = len(m)
    j = np.arange(k, dtype=_U)
    bias = (_U(k - 1) - j) * _U(A.DEL)
    wrap = (j + _U(1)) * _U(A.DEL)
    cells = np.zeros(k, dtype=_U)
    from_ins, from_del = np.zeros((len(s), k), dtype=bool), np.zeros((len(s), k), dtype=bool)
    for i, b in enumerate(s.tolist()):
        across = np.roll(cells, 1) + np.where(m == b, A.MATCH, A.SUB)
        down = cells + A.INS
        t = np.minimum(across, down)
        p = np.minimum.accumulate(t + bias) - bias
        cells = np.minimum(p, p[k - 1] + wrap)
        from_ins[i], from_del[i] = down < across, cells < t
    return cells, from_ins, from_del


def path_one(seq, motif):
    """(alignment, path, counts, deleted) of the whole of seq against the endless motif: the five numbers of align_model.align_one,
    one uint16 per position, a (k, 6) uint32 array, and the deleted columns as a list of (position in front, column) in the order
    of the walk (descending)."""
    m = A.motif_codes(motif)
    k = len(m)
    s = A._SEQ[_bytes(seq)]
    n = len(s)
    assert k >= 1 and n >= 1
    cells, from_ins, from_del = forward(s, m)
    col = int(np.argmin(cells))
    v = int(cells[col])
    consumed = v & 0x1FFFFF
    alignment = (v >> A.E_SHIFT, (v >> A.I_SHIFT) & 0xFFFFF, consumed, (col + 1 - consumed) % k, col)
    path = np.zeros(n, dtype=np.uint16)
    counts = np.zeros((k, 6), dtype=np.uint32)
    deleted = []
    i, j = n - 1, col
    while i >= 0:
        if from_del[i, j]:
            deleted.append((i, j))
            counts[j, 4] += 1
            j = (j - 1) % k
        elif from_ins[i, j]:
            path[i] = j | INS
            counts[j, 5] += 1
            i -= 1
        else:
            b = int(s[i])
            path[i] = j | (0 if b == int(m[j]) else SUB)
            if b < 4:
                counts[j, b] += 1
            j = (j - 1) % k
            i -= 1
    return alignment, path, counts, deleted


def align_path(seq, rows, motifs, begin=0, end=None):
    """(rows of align_model.DTYPE, the concatenated path, the (letters, 6) counts) for the repeats `rows` of seq[begin:end]."""
    if isinstance(seq, (bytes, bytearray)):
        seq = bytes(seq).decode("ascii")
    s = seq[begin:len(seq) if end is None else min(end, len(seq))]
    out = np.zeros(len(rows), dtype=A.DTYPE)
    paths, counts = [], []
    for at, (start, stop, motif) in enumerate(zip(rows["start"].tolist(), rows["end"].tolist(), A.split_motifs(rows, motifs))):
        assert 0 <= start < stop <= len(s), (start, stop, len(s))
        al, path, cnt, _ = path_one(s[start:stop], motif)
        out[at] = al + (0,)
        paths.append(path)
        counts.append(cnt)
    return (out, np.concatenate(paths) if paths else np.zeros(0, dtype=np.uint16),
            np.concatenate(counts) if counts else np.zeros((0, 6), dtype=np.uint32))


def deletions_behind(path, k):
    """Per position i < n - 1 the number of deletions between i and i + 1, from the path alone."""
    p = path.astype(np.int64)
    state, col, ins = p[:-1] & COLUMN, p[1:] & COLUMN, (p[1:] & INS) != 0
    return np.where(ins, col - state, col - 1 - state) % k


def perfect(motif, phase, n):
    """The path of n positions of the motif's repetition from `phase`: no flags."""
    return ((phase + np.arange(n)) % len(motif)).astype(np.uint16)
