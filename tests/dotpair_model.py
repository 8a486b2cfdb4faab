"""numpy model of the exact dot plot of two ranges, for the tests: dotplot_model.kept_cells with two sequences, two
bounds and the complement.

A = positions [a_begin, a_end) of seq_a (the rows), B = positions [b_begin, b_end) of seq_b (the columns), both upper-cased, each
end clipped to its sequence.  raw(i, j) = A[i] == B[j] on strand "+", A[i] == comp(B[j]) on strand "-"; comp swaps A/T, C/G, R/Y,
K/M, B/V, D/H and leaves every other letter alone.  kept(i, j) is the closed form of dotplot_model on the na x nb rectangle; for a
window the model walks at most t cells each way from each cell.  The layouts are those of prf_dotpair_bits / prf_dotpair_counts
(include/prf_dotpair.h), which are those of the self plot."""
import numpy as np

from dotplot_model import _range, block_sums, pack_bits  # noqa: F401  (re-exported for the tests)

COMPLEMENT = np.arange(256, dtype=np.uint8)
for _x, _y in ("AT", "CG", "RY", "KM", "BV", "DH"):
    COMPLEMENT[ord(_x)], COMPLEMENT[ord(_y)] = ord(_y), ord(_x)


def comp(seq):
    """The complement of an upper-case sequence (bytes), position by position, not reversed."""
    return COMPLEMENT[np.frombuffer(bytes(seq), dtype=np.uint8)].tobytes()


def revcomp(seq):
    return comp(seq)[::-1]


def clip_window(na, nb, rows, cols):
    out = []
    for pair, n in ((rows, na), (cols, nb)):
        lo, hi = (0, n) if pair is None else pair
        hi = n if hi is None else min(hi, n)
        out += [min(lo, hi), hi]
    return out


def kept_cells(seq_a, seq_b, strand, t, a=(0, None), b=(0, None), rows=None, cols=None):
    """bool[rows, columns] of the window rows = (row0, row1) x cols = (col0, col1) of the na x nb rectangle (None: all)."""
    sa, sb = _range(seq_a, *a), _range(seq_b, *b)
    if strand == "-":
        sb = COMPLEMENT[sb]
    else:
        assert strand == "+", strand
    na, nb = len(sa), len(sb)
    r0, r1, c0, c1 = clip_window(na, nb, rows, cols)
    i = np.arange(r0, r1, dtype=np.int64)[:, None]
    j = np.arange(c0, c1, dtype=np.int64)[None, :]
    if na == 0 or nb == 0 or r1 == r0 or c1 == c0:
        return np.zeros((r1 - r0, c1 - c0), dtype=bool)

    def raw(di, dj):
        p, q = i + di, j + dj
        inside = (p >= 0) & (p < na) & (q >= 0) & (q < nb)
        return inside & (sa[np.clip(p, 0, na - 1)] == sb[np.clip(q, 0, nb - 1)])

    centre = raw(0, 0)
    if t <= 2:
        return centre
    kept = np.zeros_like(centre)
    for dj in (1, -1):
        run = centre.astype(np.int32)                     # the cell itself, then the cells reached each way, capped at t
        for sign in (1, -1):
            alive = centre.copy()
            for v in range(1, t):
                alive &= raw(sign * v, sign * v * dj)
                if not alive.any():
                    break
                run += alive
        kept |= centre & (run + 1 >= t)
    return kept


def kept_bits(seq_a, seq_b, strand, t, a=(0, None), b=(0, None), rows=None, cols=None):
    return pack_bits(kept_cells(seq_a, seq_b, strand, t, a, b, rows, cols))


def fixture_cells(case):
    """bool[na, nb] from the hex rows of a fixture case."""
    na, nb = len(case["a"]), len(case["b"])
    out = np.zeros((na, nb), dtype=bool)
    for r, text in enumerate(case["kept"]):
        value = int(text, 16)
        out[r] = [(value >> k) & 1 for k in range(nb)]
    return out
