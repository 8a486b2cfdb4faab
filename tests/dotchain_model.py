"""numpy model of the list of chained diagonal runs of the dot plot of two ranges (include/prf_dotchain.h), for the
tests: the runs of dotruns_model.all_runs(raw) with at least min_seed cells are the seeds; they are grouped by line (diagonal or
anti-diagonal of the whole rectangle), ordered along it and linked where at most max_gap cells lie between two neighbours; a
chain is a maximal sequence of linked seeds; its matches are counted on raw, by prefix sums along the lines.  Then the filters of
the call (start cell in the window, directions, min_len) and the sort by (row, col, dir)."""
import numpy as np

import dotpair_model as P
import dotruns_model as R

MAIN, ANTI = R.MAIN, R.ANTI
DTYPE = [("row", "<u8"), ("col", "<u8"), ("len", "<u8"), ("matches", "<u8"), ("dir", "<u4"), ("seeds", "<u4")]
FIELDS = tuple(name for name, _ in DTYPE)


def _diagonal_sums(raw):
    """c[i, j] = the raw cells among (i, j), (i - 1, j - 1), ... up to the rectangle's edge."""
    c = raw.astype(np.int64)
    for i in range(1, c.shape[0]):
        c[i, 1:] += c[i - 1, :-1]
    return c


def all_chains(raw, min_seed, max_gap, every=None):
    """Every chain of both directions of a bool matrix, unsorted.  every: all_runs(raw), if the caller has it."""
    na, nb = raw.shape
    runs = R.all_runs(raw) if every is None else every
    seeds = runs[runs["len"] >= min_seed]
    row, col, length = (seeds[f].astype(np.int64) for f in ("row", "col", "len"))
    main = seeds["dir"] == MAIN
    line = np.where(main, col - row, row + col)
    t = np.where(main, np.minimum(row, col), np.minimum(row, nb - 1 - col))
    order = np.lexsort((t, line, seeds["dir"]))
    row, col, length, line, t, main = row[order], col[order], length[order], line[order], t[order], main[order]
    n = len(order)
    out = np.zeros(0, dtype=DTYPE)
    if not n:
        return out
    same_line = (line[1:] == line[:-1]) & (main[1:] == main[:-1])
    gap = t[1:] - t[:-1] - length[:-1]                         # the cells strictly between two neighbours
    assert (gap[same_line] >= 1).all()
    linked = np.concatenate(([False], same_line & (gap <= max_gap)))
    first = np.flatnonzero(~linked)
    last = np.concatenate((first[1:], [n])) - 1
    out = np.zeros(len(first), dtype=DTYPE)
    out["row"], out["col"], out["dir"] = row[first], col[first], np.where(main[first], MAIN, ANTI)
    span = t[last] + length[last] - t[first]
    out["len"], out["seeds"] = span, last - first + 1
    # matches: the prefix sum at the chain's last cell minus the one in front of its first cell (which is a mismatch or outside)
    sums = {MAIN: _diagonal_sums(raw), ANTI: _diagonal_sums(raw[:, ::-1])}
    matches = np.zeros(len(first), dtype=np.int64)
    for d in (MAIN, ANTI):
        pick = out["dir"] == d
        i0, n_cells = row[first][pick], span[pick]
        j0 = col[first][pick] if d == MAIN else nb - 1 - col[first][pick]        # in the flipped matrix an anti line is a main line
        c = sums[d]
        matches[pick] = c[i0 + n_cells - 1, j0 + n_cells - 1] - c[i0, j0] + 1
    out["matches"] = matches
    return out


def select(chains, na, nb, rows=None, cols=None, directions="both", min_len=0):
    """The filters of a call on a list of chains, and its order."""
    r0, r1, c0, c1 = P.clip_window(na, nb, rows, cols)
    keep = (chains["row"] >= r0) & (chains["row"] < r1) & (chains["col"] >= c0) & (chains["col"] < c1) & (chains["len"] >= min_len)
    keep &= np.isin(chains["dir"], R.DIRECTIONS[directions])
    return np.sort(chains[keep], order=["row", "col", "dir"])


def chains(seq_a, seq_b, strand, min_seed, max_gap, min_len=0, a=(0, None), b=(0, None), rows=None, cols=None, directions="both"):
    raw = P.kept_cells(seq_a, seq_b, strand, 0, a, b)
    return select(all_chains(raw, min_seed, max_gap), raw.shape[0], raw.shape[1], rows, cols, directions, min_len)


def same(got, want):
    """Two lists are equal row by row in the six fields."""
    return len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in FIELDS)
