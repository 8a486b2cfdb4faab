"""numpy model of the list of junctions between the chains of the period lines of one range (include/prf_periodlink.h),
for the tests: dotlink_model's pairwise construction -- the matrices of shift, gap and key, pred and succ as the argmin of a column
and of a row, a link where they are mutual -- on periodchain_model's chains of the WHOLE band k = 1 .. n - 1.  A cell of line k is
(i, c) = (t, t + k), so delta = k.  The candidates are restricted to the lines >= 1 BEFORE pred and succ are chosen: the band
holds nothing else.  Then the filters of the call (Y's start in the window, kmin <= k_Y <= kmax) and the sort by (start, k)."""
import numpy as np

import periodchain_model as M

OVERLAP, MAX_SHIFT = 16, 32                                   # PRF_DOTLINK_OVERLAP, PRF_DOTLINK_MAX_SHIFT
DTYPE = [("start", "<u8"), ("from_end", "<u8"), ("k", "<u4"), ("shift", "<i4"), ("gap", "<u4"), ("overlap", "<u4")]
FIELDS = tuple(name for name, _ in DTYPE)
NONE = np.int64(1) << 62                                      # the key of a pair that is no candidate


def seed_lines(seq, n_matches, min_seed, begin=0, end=None, top=None):
    """The lines k >= 1 of the range that can hold a seed: two equal words of min_seed letters lie k apart.  Every other line has
    no chain, so line_chains need not look at it (ranges of tens of thousands of positions)."""
    s = M._bytes(seq).upper()[begin:end]
    at = {}
    for t in range(len(s) - min_seed + 1):
        word = s[t:t + min_seed]
        if not n_matches and b"N" in word:
            continue
        at.setdefault(word, []).append(t)
    lines = set()
    for where in at.values():
        if len(where) > 1:
            a = np.array(where, dtype=np.int64)
            lines.update(np.unique(a[None, :] - a[:, None]).tolist())
    return sorted(k for k in lines if k >= 1 and (top is None or k <= top))


def band_chains(seq, n_matches, min_seed, max_gap, begin=0, end=None, sparse=False, top=None):
    """Every chain of the lines 1 .. n - 1 of the range (periodchain_model.DTYPE, sorted by (start, k)).  sparse: only the lines
    of seed_lines are looked at.  top: only the lines up to it."""
    n = len(M._bytes(seq)[begin:end])
    top = max(n - 1, 1) if top is None else max(min(top, n - 1), 1)
    if not sparse:
        return M.line_chains(seq, n_matches, 1, top, min_seed, max_gap, begin, end)
    parts = [M.line_chains(seq, n_matches, k, k, min_seed, max_gap, begin, end) for k in seed_lines(seq, n_matches, min_seed, begin, end, top)]
    found = np.concatenate(parts) if parts else np.zeros(0, dtype=M.DTYPE)
    return np.sort(found, order=["start", "k"])


def key_matrix(chains, min_seed, max_gap, max_shift):
    """(key[x, y], shift[x, y], g[x, y]) of the chains in the list's order; key is ((m + |s|) * 64 + |s|) * 32 + o) * 2 + (s < 0),
    NONE where (x, y) is no candidate.  Only chains of the lines >= 1 are looked at: the caller's list holds no others."""
    assert not len(chains) or int(chains["k"].min()) >= 1
    t_s = chains["start"].astype(np.int64)
    t_e = t_s + chains["len"].astype(np.int64) - 1
    delta = chains["k"].astype(np.int64)
    ov = min(min_seed - 1, OVERLAP)
    s = delta[None, :] - delta[:, None]                        # [x, y]
    gi = t_s[None, :] - t_e[:, None] - 1
    g = np.minimum(gi, gi + s)
    candidate = (np.abs(s) >= 1) & (np.abs(s) <= max_shift) & (g >= -ov) & (g <= max_gap)
    m, o = np.maximum(g, 0), np.maximum(-g, 0)
    key = (((m + np.abs(s)) * 64 + np.abs(s)) * 32 + o) * 2 + (s < 0)
    return np.where(candidate, key, NONE), s, g


def all_links(chains, min_seed, max_gap, max_shift, unique=None):
    """Every link between the chains of a whole band, sorted by (start, k).  unique: a list that receives whether every chain's
    smallest key is held by one candidate only."""
    if not len(chains):
        return np.zeros(0, dtype=DTYPE)
    key, s, g = key_matrix(chains, min_seed, max_gap, max_shift)
    pred, succ = key.argmin(axis=0), key.argmin(axis=1)        # pred[y] = x, succ[x] = y
    has_pred = key.min(axis=0) < NONE
    if unique is not None:
        unique.append(bool(((key == key.min(axis=0)[None, :]).sum(axis=0)[has_pred] == 1).all()
                           and ((key == key.min(axis=1)[:, None]).sum(axis=1)[key.min(axis=1) < NONE] == 1).all()))
    y = np.flatnonzero(has_pred & (succ[pred] == np.arange(len(chains))))
    x = pred[y]
    rows = np.zeros(len(y), dtype=DTYPE)
    rows["start"], rows["k"] = chains["start"][y], chains["k"][y]
    rows["from_end"] = chains["start"][x] + chains["len"][x] - 1
    rows["shift"], rows["gap"], rows["overlap"] = s[x, y], np.maximum(g[x, y], 0), np.maximum(-g[x, y], 0)
    return np.sort(rows, order=["start", "k"])


def all_links_by_join(chains, min_seed, max_gap, max_shift):
    """all_links for lists whose pairwise matrices would not fit (a million chains): the same candidates, keys and choices, but
    the candidates are listed instead of tabulated.  X is a candidate for Y at shift s = k_Y - k_X and distance gi = t_s(Y) -
    t_e(X) - 1, so for each (s, gi) that the rule admits X is the one chain of line k_Y - s that ends at t_s(Y) - 1 - gi: an exact
    join (chains of one line end at different cells).  pred and succ are the smallest key of a column and of a row, at equal keys
    the first chain in the list's order, as argmin chooses.  tests/test_periodlink_cpu.py pins it to all_links."""
    if not len(chains):
        return np.zeros(0, dtype=DTYPE)
    assert int(chains["k"].min()) >= 1
    t_s = chains["start"].astype(np.int64)
    t_e = t_s + chains["len"].astype(np.int64) - 1
    delta = chains["k"].astype(np.int64)
    ov = min(min_seed - 1, OVERLAP)
    width = int(t_e.max()) + OVERLAP + max_gap + max_shift + 2    # (line, end cell) as one number: above every cell asked for
    ends = delta * width + t_e
    by_end = np.argsort(ends, kind="stable")
    sorted_ends = ends[by_end]
    xs, ys, keys = [], [], []
    for s in [d for d in range(-max_shift, max_shift + 1) if d]:
        for g in range(-ov, max_gap + 1):
            gi = g if s > 0 else g - s                              # g = min(gi, gi + s)
            line, cell = delta - s, t_s - 1 - gi
            ok = (line >= 1) & (cell >= 0)
            wanted = line * width + cell
            at = np.minimum(np.searchsorted(sorted_ends, wanted), len(chains) - 1)
            ok &= sorted_ends[at] == wanted
            m, o = max(g, 0), max(-g, 0)
            xs.append(by_end[at][ok])
            ys.append(np.flatnonzero(ok))
            keys.append(np.full(int(ok.sum()), (((m + abs(s)) * 64 + abs(s)) * 32 + o) * 2 + (s < 0), dtype=np.int64))
    x, y, key = np.concatenate(xs), np.concatenate(ys), np.concatenate(keys)
    pred = np.full(len(chains), -1, dtype=np.int64)
    succ = np.full(len(chains), -1, dtype=np.int64)
    order = np.lexsort((x, key, y))                               # per Y: the smallest key, then the first chain
    first = np.concatenate(([True], y[order][1:] != y[order][:-1])) if len(order) else np.zeros(0, dtype=bool)
    pred[y[order][first]] = x[order][first]
    order = np.lexsort((y, key, x))
    first = np.concatenate(([True], x[order][1:] != x[order][:-1])) if len(order) else np.zeros(0, dtype=bool)
    succ[x[order][first]] = y[order][first]
    y = np.flatnonzero(pred >= 0)
    y = y[succ[pred[y]] == y]
    x = pred[y]
    g = np.minimum(t_s[y] - t_e[x] - 1, t_s[y] - t_e[x] - 1 + delta[y] - delta[x])
    rows = np.zeros(len(y), dtype=DTYPE)
    rows["start"], rows["k"] = chains["start"][y], chains["k"][y]
    rows["from_end"] = t_e[x]
    rows["shift"], rows["gap"], rows["overlap"] = delta[y] - delta[x], np.maximum(g, 0), np.maximum(-g, 0)
    return np.sort(rows, order=["start", "k"])


def select(links, n, positions=None, kmin=1, kmax=None):
    """The filters of a call on a list of links, and its order."""
    lo, hi = (0, n) if positions is None else positions
    hi = n if hi is None else min(hi, n)
    lo = min(lo, hi)
    keep = (links["start"] >= lo) & (links["start"] < hi) & (links["k"] >= kmin)
    if kmax is not None:
        keep &= links["k"] <= kmax
    return np.sort(links[keep], order=["start", "k"])


def links(seq, kmin, kmax, min_seed, max_gap, max_shift, n_matches=False, begin=0, end=None, positions=None, sparse=False,
          pairwise=True):
    """The list of a call; pairwise False: by all_links_by_join, for a million chains.  pred(Y) is chosen among the lines k_Y +- max_shift and succ(X) among k_X +- max_shift, so the links
    with k_Y <= kmax are decided by the lines up to kmax + 2 max_shift: the lines above are not looked at (ranges of thousands of
    positions with short seeds, where the pairwise matrices of the whole band would not fit)."""
    n = len(M._bytes(seq)[begin:end])
    top = None if kmax is None else kmax + 2 * max_shift
    every = (all_links if pairwise else all_links_by_join)(band_chains(seq, n_matches, min_seed, max_gap, begin, end, sparse, top),
                                                           min_seed, max_gap, max_shift)
    return select(every, n, positions, kmin, kmax)


def same(got, want):
    """Two lists are equal row by row in the six fields."""
    return len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in FIELDS)
