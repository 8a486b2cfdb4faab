"""The CPU model of the alignment product (include/prf_align.h): the wraparound recurrence in numpy, one step per
position, the three counts of a cell packed into one uint64 so that the lexicographic minimum is the integer minimum.  The tests
compare the library with it exactly; tests/test_align_cpu.py checks it against an independent brute force first."""
import numpy as np

FIELDS = ("edits", "indels", "consumed", "start_column", "end_column", "reserved")
DTYPE = [(name, "<u4") for name in FIELDS]
REPEAT_DTYPE = [("start", "<u8"), ("end", "<u8"), ("k", "<u4"), ("reserved", "<u4")]
MAX_K, MAX_LEN = 1024, 1 << 19

E_SHIFT, I_SHIFT = 41, 21
MATCH = np.uint64(1)                                        # (0, 0, 1)
SUB = np.uint64((1 << E_SHIFT) | 1)                         # (1, 0, 1)
INS = np.uint64((1 << E_SHIFT) | (1 << I_SHIFT))            # (1, 1, 0)
DEL = (1 << E_SHIFT) | (1 << I_SHIFT) | 1                   # (1, 1, 1)

_SEQ = np.full(256, 4, dtype=np.uint8)                      # everything that is not A, C, G, T: no match
_MOTIF = np.full(256, 0xFF, dtype=np.uint8)
for _code, _letter in enumerate("ACGT"):
    _SEQ[ord(_letter)] = _SEQ[ord(_letter.lower())] = _code
    _MOTIF[ord(_letter)] = _MOTIF[ord(_letter.lower())] = _code
_MOTIF[ord("N")] = _MOTIF[ord("n")] = 5


def motif_codes(motif):
    """0 .. 3 for A, C, G, T, 5 for N, in either case; anything else is a ValueError naming the column."""
    codes = _MOTIF[np.frombuffer(motif.encode("ascii") if isinstance(motif, str) else bytes(motif), dtype=np.uint8)]
    if (codes == 0xFF).any():
        raise ValueError(f"column {int(np.argmax(codes == 0xFF))} of the motif is not one of A C G T N")
    return codes


def align_one(seq, motif):
    """(edits, indels, consumed, start_column, end_column) of the whole of seq (str or bytes) against the endless motif."""
    m = motif_codes(motif)
    k = len(m)
    s = _SEQ[np.frombuffer(seq.encode("ascii") if isinstance(seq, str) else bytes(seq), dtype=np.uint8)]
    assert k >= 1 and len(s) >= 1
    j = np.arange(k, dtype=np.uint64)
    bias = (np.uint64(k - 1) - j) * np.uint64(DEL)
    wrap = (j + np.uint64(1)) * np.uint64(DEL)
    cells = np.zeros(k, dtype=np.uint64)
    for b in s.tolist():
        t = np.minimum(np.roll(cells, 1) + np.where(m == b, MATCH, SUB), cells + INS)
        p = np.minimum.accumulate(t + bias) - bias
        cells = np.minimum(p, p[k - 1] + wrap)
    col = int(np.argmin(cells))                             # the first of equal minima
    v = int(cells[col])
    consumed = v & 0x1FFFFF
    return v >> E_SHIFT, (v >> I_SHIFT) & 0xFFFFF, consumed, (col + 1 - consumed) % k, col


def repeats(*rows):
    """Rows (start, end, k) as the array the calls take."""
    out = np.zeros(len(rows), dtype=REPEAT_DTYPE)
    for at, (start, end, k) in enumerate(rows):
        out[at] = (start, end, k, 0)
    return out


def split_motifs(rows, motifs):
    """One motif per row from a list of str, or from the letters (str or bytes) that a consensus call returned."""
    ks = rows["k"].tolist()
    if isinstance(motifs, (str, bytes, bytearray)):
        text = motifs if isinstance(motifs, str) else bytes(motifs).decode("ascii")
        assert len(text) == sum(ks)
        offsets = np.concatenate([[0], np.cumsum(ks)]).tolist()
        return [text[offsets[at]:offsets[at + 1]] for at in range(len(ks))]
    assert [len(m) for m in motifs] == ks
    return list(motifs)


def align(seq, rows, motifs, begin=0, end=None):
    """Rows of DTYPE for the repeats `rows` (fields start, end, k, relative to begin) of seq[begin:end], in their order."""
    if isinstance(seq, (bytes, bytearray)):
        seq = bytes(seq).decode("ascii")
    s = seq[begin:len(seq) if end is None else min(end, len(seq))]
    out = np.zeros(len(rows), dtype=DTYPE)
    for at, (start, stop, motif) in enumerate(zip(rows["start"].tolist(), rows["end"].tolist(), split_motifs(rows, motifs))):
        assert 0 <= start < stop <= len(s), (start, stop, len(s))
        out[at] = align_one(s[start:stop], motif) + (0,)
    return out


def derived(n, k, edits, indels, consumed):
    """(subs, ins, del, matches, aligned identity, aligned copies) of a row of n positions."""
    subs, ins, dele = edits - indels, (indels + n - consumed) // 2, (indels - n + consumed) // 2
    matches = n - subs - ins
    return subs, ins, dele, matches, matches / (n + dele), consumed / k


def same(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and a.tobytes() == b.tobytes()
