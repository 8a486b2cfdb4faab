"""The CPU model of the consensus over phased segments (include/prf_phased.h) and of the host step that turns the
chains and links of a gapped repeat into such segments (prf_native.group_segments): plain Python over the string and over lists.
The tests compare the library and the binding with it exactly; tests/test_phased_cpu.py checks it against an independent brute
force first."""
import numpy as np

import consensus_model as C

DTYPE = C.DTYPE
SEGMENT_DTYPE = [("start", "<u8"), ("end", "<u8"), ("row", "<u4"), ("phase", "<u4")]
PIECE_DTYPE = [("group", "<u8"), ("anchor", "<u8"), ("end", "<u8"), ("k", "<u4"), ("segments", "<u4"), ("positions", "<u8")]
BASES = C.BASES


def segments(*rows):
    """Segments (start, end, row, phase) as the array the calls take."""
    out = np.zeros(len(rows), dtype=SEGMENT_DTYPE)
    for at, row in enumerate(rows):
        out[at] = tuple(row)
    return out


def consensus(seq, ks, segs, begin=0, end=None):
    """(rows of DTYPE, motifs as a list of str, counts of (sum of k, 4)) of the rows of ks[r] columns over the segments `segs`
    (fields start, end, row, phase, relative to begin) of seq[begin:end] (str or bytes), in row order.  A segment's slice
    s[start + j:end:k], j = 0 .. k - 1, is what falls into column (phase + j) mod k."""
    if isinstance(seq, (bytes, bytearray)):
        seq = bytes(seq).decode("ascii")
    s = seq[begin:len(seq) if end is None else min(end, len(seq))].upper()
    ks = [int(k) for k in ks]
    tables = [np.zeros((k, 4), dtype=np.uint32) for k in ks]
    for start, stop, row, phase in zip(*(segs[f].tolist() for f in ("start", "end", "row", "phase"))):
        k = ks[row]
        assert 0 <= start < stop <= len(s) and 0 <= phase < k, (start, stop, row, phase, k, len(s))
        for j in range(min(k, stop - start)):
            column = s[start + j:stop:k]
            for b, letter in enumerate(BASES):
                tables[row][(phase + j) % k, b] += column.count(letter)
    out = np.zeros(len(ks), dtype=DTYPE)
    motifs, offset = [], 0
    for at, (k, counts) in enumerate(zip(ks, tables)):
        out[at] = (offset, int(counts.max(axis=1).sum(dtype=np.uint64)), int(counts.sum(dtype=np.uint64)), k, 0)
        motifs.append(C.letters_of(counts))
        offset += k
    return out, motifs, np.concatenate([np.zeros((0, 4), dtype=np.uint32)] + tables)


def paths_of(chains, links):
    """The paths of join_period_chains, as lists of chain indices in the order of their first chains: every link names its
    successor by (start, k) and its predecessor by (last cell, k - shift)."""
    n = len(chains)
    rows = list(zip(chains["start"].tolist(), chains["len"].tolist(), chains["k"].tolist()))
    succ, has_pred = {}, set()
    for t_s, t_e, k, shift in zip(*(links[f].tolist() for f in ("start", "from_end", "k", "shift"))):
        y = [at for at, (s, _, line) in enumerate(rows) if (s, line) == (t_s, k)]
        x = [at for at, (s, length, line) in enumerate(rows) if (s + length - 1, line) == (t_e, k - shift)]
        assert len(y) == 1 and len(x) <= 1
        if x:
            succ[x[0]] = y[0]
            has_pred.add(y[0])
    out = []
    for head in range(n):
        if head in has_pred:
            continue
        path = [head]
        while path[-1] in succ:
            path.append(succ[path[-1]])
        out.append(path)
    return out


def group_segments(chains, links, periods):
    """(pieces as tuples of PIECE_DTYPE, segments as tuples of SEGMENT_DTYPE) by the rule of DESIGN 19.2, path by path; periods:
    the period of every path (join_period_chains' `period`)."""
    rows = list(zip(chains["start"].tolist(), chains["len"].tolist(), chains["k"].tolist()))
    pieces, segs = [], []
    for group, (path, period) in enumerate(zip(paths_of(chains, links), periods)):
        state = None                                            # anchor, drift, end of the last segment, index of the piece
        detour = None                                           # the chains since the last on-period chain
        for c in path:
            start, length, line = rows[c]
            if line != period:
                if detour is not None:
                    detour.append(c)
                continue
            isolated = detour is not None and len(detour) == 1 and rows[detour[0]][1] <= rows[detour[0]][2]
            if state is not None and isolated:
                state[1] += rows[detour[0]][2] - period
            else:
                state = [start, 0, start, len(pieces)]
                pieces.append([group, start, start, period, 0, 0])
            detour = []
            lo, hi = max(start, state[2]), start + length + period
            if lo < hi:
                segs.append((lo, hi, state[3], (lo - state[0] - state[1]) % period))
                state[2] = hi
                piece = pieces[state[3]]
                piece[2], piece[4], piece[5] = hi, piece[4] + 1, piece[5] + hi - lo
    return [tuple(p) for p in pieces], segs


def same(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and a.tobytes() == b.tobytes()
