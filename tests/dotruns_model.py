"""numpy / Python model of the list of diagonal runs of the dot plot of two ranges (include/prf_dotruns.h), for the
tests: raw = dotpair_model.kept_cells(..., t=0) of the whole na x nb rectangle, every diagonal and anti-diagonal walked for its
maximal runs of raw cells, then the filters of the call (start cell in the window, min_len, directions) and the sort by (row,
col, dir).  A main run is (row + s, col + s), an anti run (row + s, col - s): the start is the cell with the smallest row."""
import numpy as np

import dotpair_model as P

MAIN, ANTI = 1, 2
DIRECTIONS = {"main": (MAIN,), "anti": (ANTI,), "both": (MAIN, ANTI)}
DTYPE = [("row", "<u8"), ("col", "<u8"), ("len", "<u8"), ("dir", "<u4")]


def _main_runs(raw):
    """(rows, cols, lens) of the maximal runs along (+1, +1) of a bool matrix, diagonal by diagonal."""
    na, nb = raw.shape
    rows, cols, lens = [], [], []
    for k in range(-(na - 1), nb):
        d = np.diagonal(raw, k)
        if not d.any():
            continue
        edge = np.diff(np.concatenate(([0], d.astype(np.int8), [0])))
        starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
        rows.append(max(0, -k) + starts)
        cols.append(max(0, k) + starts)
        lens.append(ends - starts)
    if not rows:
        return (np.zeros(0, dtype=np.int64),) * 3
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(lens)


def all_runs(raw):
    """Every run of both directions of a bool matrix, unsorted, as a structured array."""
    nb = raw.shape[1]
    mi, mj, mn = _main_runs(raw)
    ai, aj, an = _main_runs(raw[:, ::-1])
    out = np.zeros(len(mi) + len(ai), dtype=DTYPE)
    out["row"], out["col"], out["len"] = np.concatenate((mi, ai)), np.concatenate((mj, nb - 1 - aj)), np.concatenate((mn, an))
    out["dir"][:len(mi)], out["dir"][len(mi):] = MAIN, ANTI
    return out


def select(runs, na, nb, rows=None, cols=None, directions="both", min_len=1):
    """The filters of a call on a list of runs, and its order."""
    r0, r1, c0, c1 = P.clip_window(na, nb, rows, cols)
    keep = (runs["row"] >= r0) & (runs["row"] < r1) & (runs["col"] >= c0) & (runs["col"] < c1) & (runs["len"] >= min_len)
    keep &= np.isin(runs["dir"], DIRECTIONS[directions])
    return np.sort(runs[keep], order=["row", "col", "dir"])


def runs(seq_a, seq_b, strand, a=(0, None), b=(0, None), rows=None, cols=None, directions="both", min_len=1):
    raw = P.kept_cells(seq_a, seq_b, strand, 0, a, b)
    return select(all_runs(raw), raw.shape[0], raw.shape[1], rows, cols, directions, min_len)


def cells(runs_, na, nb):
    """bool[na, nb] of a list's cells, cell by cell (the plain counterpart of prf_native.run_cells)."""
    out = np.zeros((na, nb), dtype=bool)
    for i, j, n, d in zip(runs_["row"].tolist(), runs_["col"].tolist(), runs_["len"].tolist(), runs_["dir"].tolist()):
        for s in range(n):
            out[i + s, j + s if d == MAIN else j - s] = True
    return out


def same(got, want):
    """Two lists are equal row by row in the four fields."""
    return len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in ("row", "col", "len", "dir"))
