"""numpy model of the exact dot plot (reference plot_dot_plot.py: generate_matrix + filter_out_noise), for the tests.

The sequence is upper-cased; s = positions [begin, end) (end clipped to the sequence), n = len(s).  raw(i, j) = s[i] == s[j] as
symbols -- N == N is a match, a letter matches only itself.  With t = min_diagonal_run the closed form of the reference's
in-place filter is
    kept(i, j)  <=>  raw(i, j) and (Lmain + 1 >= t or Lanti + 1 >= t),
Lmain / Lanti = the length of the maximal run of raw cells through (i, j) along (+1, +1) / (+1, -1) in the unfiltered n x n
matrix.  For a window the model walks at most t cells each way from each cell, so a small window at a large coordinate is cheap.
The layouts are those of prf_dotplot_bits / prf_dotplot_counts (include/prf_dotplot.h)."""
import numpy as np

from periodicity_model import _symbols, pack_bits  # noqa: F401  (pack_bits: the same word layout)


def _range(seq, begin, end):
    a = _symbols(seq)
    end = len(a) if end is None else min(end, len(a))
    return a[begin:end] if begin < end else a[:0]


def clip_window(n, rows, cols):
    out = []
    for pair in (rows, cols):
        lo, hi = (0, n) if pair is None else pair
        hi = n if hi is None else min(hi, n)
        out += [min(lo, hi), hi]
    return out


def kept_cells(seq, t, begin=0, end=None, rows=None, cols=None):
    """bool[rows, columns] of the window rows = (row0, row1) x cols = (col0, col1) of the range's matrix (None: all)."""
    s = _range(seq, begin, end)
    n = len(s)
    r0, r1, c0, c1 = clip_window(n, rows, cols)
    i = np.arange(r0, r1, dtype=np.int64)[:, None]
    j = np.arange(c0, c1, dtype=np.int64)[None, :]
    if n == 0 or r1 == r0 or c1 == c0:
        return np.zeros((r1 - r0, c1 - c0), dtype=bool)

    def raw(di, dj):
        a, b = i + di, j + dj
        inside = (a >= 0) & (a < n) & (b >= 0) & (b < n)
        return inside & (s[np.clip(a, 0, n - 1)] == s[np.clip(b, 0, n - 1)])

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


def kept_bits(seq, t, begin=0, end=None, rows=None, cols=None):
    return pack_bits(kept_cells(seq, t, begin, end, rows, cols))


def block_sums(cells, block):
    """uint32[ceil(rows / block), ceil(columns / block)]: set cells per block of block x block cells."""
    n_rows, n_cols = cells.shape
    br, bc = -(-n_rows // block), -(-n_cols // block)
    padded = np.zeros((br * block, bc * block), dtype=np.uint32)
    padded[:n_rows, :n_cols] = cells
    return padded.reshape(br, block, bc, block).sum(axis=(1, 3), dtype=np.uint32)


def filter_matrix(matrix, t):
    """The closed form on ANY 0/1 matrix (not only a dot plot of a sequence), cell by cell: bool matrix of the kept cells."""
    cells = np.asarray(matrix) > 0
    n_rows, n_cols = cells.shape if cells.ndim == 2 else (0, 0)
    kept = np.zeros((n_rows, n_cols), dtype=bool)

    def reach(i, j, di, dj):
        steps = 0
        while 0 <= i < n_rows and 0 <= j < n_cols and cells[i, j]:
            i, j, steps = i + di, j + dj, steps + 1
        return steps

    for i in range(n_rows):
        for j in range(n_cols):
            if cells[i, j]:
                kept[i, j] = any(reach(i, j, 1, dj) + reach(i, j, -1, -dj) - 1 + 1 >= t for dj in (1, -1))
    return kept


def fixture_cells(case):
    """bool[n, n] from the hex rows of a fixture case."""
    n = len(case["seq"])
    out = np.zeros((n, n), dtype=bool)
    for r, text in enumerate(case["kept"]):
        value = int(text, 16)
        out[r] = [(value >> b) & 1 for b in range(n)]
    return out
