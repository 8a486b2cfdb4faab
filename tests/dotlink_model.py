"""numpy model of the list of junctions between the chains of the dot plot of two ranges (include/prf_dotlink.h), for
the tests: the definition, word for word, on dotchain_model.all_chains -- per direction the chains in the coordinates (i, c), the
pairwise matrices of shift, gap and key, pred and succ as the argmin of a column and of a row, a link where they are mutual.  Then
the filters of the call (Y's first cell in the window, directions) and the sort by (row, col, dir)."""
import numpy as np

import dotchain_model as C
import dotpair_model as P
import dotruns_model as R

MAIN, ANTI = R.MAIN, R.ANTI
OVERLAP, MAX_SHIFT = 16, 32                                   # PRF_DOTLINK_OVERLAP, PRF_DOTLINK_MAX_SHIFT
DTYPE = [("row", "<u8"), ("col", "<u8"), ("from_row", "<u8"), ("from_col", "<u8"), ("dir", "<u4"), ("shift", "<i4"), ("gap", "<u4"),
         ("overlap", "<u4")]
FIELDS = tuple(name for name, _ in DTYPE)
NONE = np.int64(1) << 62                                      # the key of a pair that is no candidate


def key_matrix(chains, nb, d, min_seed, max_gap, max_shift):
    """For the chains of direction d, in the list's order: (index into chains, key[x, y], shift[x, y], g[x, y]); key is
    ((m + |s|) * 64 + |s|) * 32 + o) * 2 + (s < 0), NONE where (x, y) is no candidate."""
    at = np.flatnonzero(chains["dir"] == d)
    i_s = chains["row"][at].astype(np.int64)
    col = chains["col"][at].astype(np.int64)
    c_s = col if d == MAIN else nb - 1 - col
    i_e = i_s + chains["len"][at].astype(np.int64) - 1
    delta = c_s - i_s
    ov = min(min_seed - 1, OVERLAP)
    s = delta[None, :] - delta[:, None]                        # [x, y]
    gi = i_s[None, :] - i_e[:, None] - 1
    g = np.minimum(gi, gi + s)
    candidate = (np.abs(s) >= 1) & (np.abs(s) <= max_shift) & (g >= -ov) & (g <= max_gap)
    m, o = np.maximum(g, 0), np.maximum(-g, 0)
    key = (((m + np.abs(s)) * 64 + np.abs(s)) * 32 + o) * 2 + (s < 0)
    return at, np.where(candidate, key, NONE), s, g


def all_links(chains, nb, min_seed, max_gap, max_shift, unique=None):
    """Every link between the chains of a whole rectangle (dotchain_model.all_chains), unsorted.  unique: a list that receives,
    per direction, whether every chain's smallest key is held by one candidate only."""
    out = []
    for d in (MAIN, ANTI):
        at, key, s, g = key_matrix(chains, nb, d, min_seed, max_gap, max_shift)
        if not len(at):
            continue
        pred, succ = key.argmin(axis=0), key.argmin(axis=1)    # pred[y] = x, succ[x] = y
        has_pred = key.min(axis=0) < NONE
        if unique is not None:
            unique.append(bool(((key == key.min(axis=0)[None, :]).sum(axis=0)[has_pred] == 1).all()
                               and ((key == key.min(axis=1)[:, None]).sum(axis=1)[key.min(axis=1) < NONE] == 1).all()))
        y = np.flatnonzero(has_pred & (succ[pred] == np.arange(len(at))))
        x = pred[y]
        rows = np.zeros(len(y), dtype=DTYPE)
        cx, cy = chains[at[x]], chains[at[y]]
        rows["row"], rows["col"], rows["dir"] = cy["row"], cy["col"], d
        n = cx["len"].astype(np.int64) - 1
        rows["from_row"] = cx["row"].astype(np.int64) + n
        rows["from_col"] = cx["col"].astype(np.int64) + (n if d == MAIN else -n)
        rows["shift"], rows["gap"], rows["overlap"] = s[x, y], np.maximum(g[x, y], 0), np.maximum(-g[x, y], 0)
        out.append(rows)
    return np.concatenate(out) if out else np.zeros(0, dtype=DTYPE)


def select(links, na, nb, rows=None, cols=None, directions="both"):
    """The filters of a call on a list of links, and its order."""
    r0, r1, c0, c1 = P.clip_window(na, nb, rows, cols)
    keep = (links["row"] >= r0) & (links["row"] < r1) & (links["col"] >= c0) & (links["col"] < c1)
    keep &= np.isin(links["dir"], R.DIRECTIONS[directions])
    return np.sort(links[keep], order=["row", "col", "dir"])


def links(seq_a, seq_b, strand, min_seed, max_gap, max_shift, a=(0, None), b=(0, None), rows=None, cols=None, directions="both"):
    raw = P.kept_cells(seq_a, seq_b, strand, 0, a, b)
    every = all_links(C.all_chains(raw, min_seed, max_gap), raw.shape[1], min_seed, max_gap, max_shift)
    return select(every, raw.shape[0], raw.shape[1], rows, cols, directions)


def same(got, want):
    """Two lists are equal row by row in the eight fields."""
    return len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in FIELDS)
