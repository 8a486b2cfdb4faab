"""numpy model of the list of chains on the period lines of one range (include/prf_periodchain.h), for the tests: line k
of the range s is the diagonal col - row = k of the dot plot of s with itself on the plus strand, so the model IS
dotchain_model.all_chains on dotpair_model.kept_cells(s, s, "+", 0) -- with the rows and columns of N cleared for n_matches = 0 --
filtered to the main direction and kmin <= col - row <= kmax.  Then the filters of the call (start in the window, min_len) and the
sort by (start, k)."""
import numpy as np

import dotchain_model as C
import dotpair_model as P
import dotruns_model as R

DTYPE = [("start", "<u8"), ("len", "<u8"), ("matches", "<u8"), ("k", "<u4"), ("seeds", "<u4")]
FIELDS = tuple(name for name, _ in DTYPE)


def _bytes(seq):
    return seq.encode("ascii") if isinstance(seq, str) else bytes(seq)


def band_cells(seq, n_matches, kmin, kmax, begin=0, end=None):
    """bool[n, n]: the raw cells of the range with itself on the lines kmin .. kmax, nothing else."""
    s = _bytes(seq).upper()[begin:end]
    raw = P.kept_cells(s, s, "+", 0)
    if not n_matches and len(s):
        is_n = np.frombuffer(s, dtype=np.uint8) == ord("N")
        raw[is_n, :] = False
        raw[:, is_n] = False
    n = len(s)
    line = np.arange(n, dtype=np.int64)[None, :] - np.arange(n, dtype=np.int64)[:, None]
    raw &= (line >= kmin) & (line <= kmax)
    return raw


def runs_of(raw):
    """The runs of the band, for all_chains(..., every): computed once for several (min_seed, max_gap)."""
    return R.all_runs(raw)


def all_chains(raw, min_seed, max_gap, every=None):
    """Every chain of the band as rows of DTYPE, sorted by (start, k)."""
    found = C.all_chains(raw, min_seed, max_gap, every)
    found = found[found["dir"] == C.MAIN]
    out = np.zeros(len(found), dtype=DTYPE)
    out["start"], out["len"], out["matches"], out["seeds"] = found["row"], found["len"], found["matches"], found["seeds"]
    out["k"] = found["col"] - found["row"]
    return np.sort(out, order=["start", "k"])


def select(chains, n, positions=None, kmin=1, kmax=None, min_len=0):
    """The filters of a call on a list of chains, and its order."""
    lo, hi = (0, n) if positions is None else positions
    hi = n if hi is None else min(hi, n)
    lo = min(lo, hi)
    keep = (chains["start"] >= lo) & (chains["start"] < hi) & (chains["len"] >= min_len) & (chains["k"] >= kmin)
    if kmax is not None:
        keep &= chains["k"] <= kmax
    return np.sort(chains[keep], order=["start", "k"])


def chains(seq, kmin, kmax, min_seed, max_gap, n_matches=False, min_len=0, begin=0, end=None, positions=None):
    raw = band_cells(seq, n_matches, kmin, kmax, begin, end)
    return select(all_chains(raw, min_seed, max_gap), raw.shape[0], positions, min_len=min_len)


def line_chains(seq, n_matches, kmin, kmax, min_seed, max_gap, begin=0, end=None):
    """The same list without the n x n matrix, for ranges too long for it: every line as a vector of cells, its runs by the
    changes of that vector, the chains by the gaps between the seeds, the matches by prefix sums.  Pinned to all_chains by
    tests/test_periodchain_cpu.py."""
    s = np.frombuffer(_bytes(seq).upper()[begin:end], dtype=np.uint8)
    n, parts = len(s), []
    for k in range(kmin, min(kmax, n - 1) + 1):
        cells = s[:n - k] == s[k:]
        if not n_matches:
            cells &= s[:n - k] != ord("N")
        edge = np.diff(np.concatenate(([0], cells.view(np.int8), [0])))
        first, behind = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)          # runs [first, behind)
        seed = behind - first >= min_seed
        first, behind = first[seed], behind[seed]
        if not len(first):
            continue
        head = np.concatenate(([True], first[1:] - behind[:-1] > max_gap))            # cells strictly between: first - behind
        at = np.flatnonzero(head)
        last = np.concatenate((at[1:], [len(first)])) - 1
        sums = np.concatenate(([0], np.cumsum(cells)))
        out = np.zeros(len(at), dtype=DTYPE)
        out["start"], out["len"], out["k"], out["seeds"] = first[at], behind[last] - first[at], k, last - at + 1
        out["matches"] = sums[behind[last]] - sums[first[at]]
        parts.append(out)
    found = np.concatenate(parts) if parts else np.zeros(0, dtype=DTYPE)
    return np.sort(found, order=["start", "k"])


def same(got, want):
    """Two lists are equal row by row in the five fields."""
    return len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in FIELDS)
