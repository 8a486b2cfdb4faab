"""The chunked walk of the interrupted-repeat driver in plain Python: the CPU model of prf_scan_interrupted_chunked.

Write match(q) for seq[q] == seq[q + k].  The boundaries of motif size k are the positions q + 1 with 1 <= q < n - k,
match(q - 1) and not match(q).  With min_repeats >= 2 every jump back of interrupted_model.walk() lands in the clean state on
the next boundary, none skipped, until an episode reaches the end of the sequence.  So the episodes that start at [0] + boundaries
do not depend on each other, and the walk can be cut by landing position: the piece for [lo, hi) starts clean on the first
boundary >= lo (position 0 for lo == 0), stops without walking it at the first landing >= hi, and says whether it reached the
end.  The pieces in order, up to the first one that reached the end, list the candidates of the whole walk.
"""
import interrupted_model as M


def boundaries(seq, k):
    """Ascending positions q + 1 with 1 <= q < n - k, match(q - 1) and not match(q)."""
    n = len(seq)
    return [q + 1 for q in range(1, n - k) if seq[q - 1] == seq[q - 1 + k] and seq[q] != seq[q + k]]


def first_boundary(seq, k, lo, hi):
    """The first boundary in [lo, hi) (lo >= 2), found the way a lane does: scanning forward from q = lo - 1.  None: no work."""
    n = len(seq)
    for q in range(lo - 1, min(n - k, hi - 1)):
        if seq[q - 1] == seq[q - 1 + k] and seq[q] != seq[q + k]:
            return q + 1
    return None


class Piece(M.Walk):
    """Candidates of the episodes of one (sequence, k) that land in [lo, hi)."""

    def __init__(self):
        super().__init__()
        self.at_end = False      # the walk ended in one of these episodes
        self.has_work = True     # False: no boundary in [lo, hi)
        self.episodes = 0


def walk_range(seq, k, min_repeats, min_span, max_interruptions, lo, hi, stride=0, slots=0, episodes=None):
    """interrupted_model.walk() restricted to the landings in [lo, hi): the same moves, the same memo (a table of its own),
    three differences: the start, the stop at a landing >= hi (normal reset and memo hit alike), and at_end."""
    n = len(seq)
    w = Piece()
    pos = 0
    if lo > 0:
        pos = first_boundary(seq, k, lo, hi)
        if pos is None:
            w.has_work = False
            return w
    run = mask = n_int = 0
    first = -1
    memo = [None] * slots if stride and slots else None
    outcome = []
    r_span = min_repeats * k

    def close(result):
        if memo is not None and outcome and outcome[-1] is M.PENDING:
            outcome[-1] = result

    def open_episode():
        w.episodes += 1
        if memo is not None and (episodes is None or len(outcome) < episodes):
            outcome.append(M.PENDING)

    open_episode()
    while True:
        if memo is not None and pos % stride == 0:
            s = M._slot(pos, run, mask, slots)
            rec = memo[s]
            if first >= 0:
                w.lookups += 1
            if (first >= 0 and rec is not None and rec[0] == pos and rec[1] == run and rec[2] == mask
                    and outcome[rec[3]] is not M.PENDING):
                w.hits += 1
                cand, at_end = outcome[rec[3]]
                if cand is not None:
                    w.cands.append(cand)
                close(outcome[rec[3]])
                if at_end:
                    w.at_end = True
                    return w
                if first + 1 >= hi:
                    return w
                pos = first + 1
                w.landings.append(pos)
                first, run, mask, n_int = -1, 0, 0, 0
                open_episode()
                continue
            if outcome and outcome[-1] is M.PENDING:
                memo[s] = (pos, run, mask, len(outcome) - 1)

        at_end = pos >= n - k
        if not at_end:
            w.steps += 1
            if seq[pos] == seq[pos + k]:
                run += 1
                pos += 1
                continue
            if run > 0:
                if first < 0:
                    first = pos
                ph = run % k
                if n_int < max_interruptions and not (mask >> ph) & 1:
                    mask |= 1 << ph
                    n_int += 1
                if (mask >> ph) & 1:
                    run += 1
                    pos += 1
                    continue

        if run + k < min_span or run + k < r_span:
            if at_end:
                close((None, True))
                w.at_end = True
                return w
            run = 0
            pos += 1
            continue
        cand = None
        start = pos - run
        if b"N" not in seq[start:start + k]:
            while pos < n and (seq[pos] == seq[pos - k] or (mask >> (run % k)) & 1):
                run += 1
                pos += 1
                w.steps += 1
            if run >= min_span and run >= r_span:
                cand = (start, pos, mask, M._homopolymer(seq, start, k, mask))
                w.cands.append(cand)
        close((cand, at_end))
        if at_end:
            w.at_end = True
            return w
        assert first >= 0        # with min_repeats >= 2 a passing check not at the end follows a mismatch behind a run
        if first + 1 >= hi:
            return w
        pos = first + 1
        w.landings.append(pos)
        first, run, mask, n_int = -1, 0, 0, 0
        open_episode()


def n_chunks(n, chunk):
    """Lanes per (sequence, k) for a trimmed length n: chunk == 0 is one lane."""
    return max(1, -(-n // chunk)) if chunk else 1


def walk_chunked(seq, k, min_repeats, min_span, max_interruptions, chunk, stride=0, slots=0, episodes=None, counters=None):
    """The candidate list of (sequence, k) from independent pieces of `chunk` landing positions each."""
    if chunk == 0:
        return M.walk(seq, k, min_repeats, min_span, max_interruptions, stride, slots, episodes).cands
    nc = n_chunks(len(seq), chunk)
    pieces = [walk_range(seq, k, min_repeats, min_span, max_interruptions, c * chunk, (c + 1) * chunk, stride, slots, episodes)
              for c in range(nc)]
    ended = [c for c, p in enumerate(pieces) if p.at_end]
    assert ended, "no piece reached the end of the sequence"
    if counters is not None:
        counters["lanes"] = counters.get("lanes", 0) + nc
        counters["dropped_lanes"] = counters.get("dropped_lanes", 0) + nc - 1 - ended[0]
        counters["idle_lanes"] = counters.get("idle_lanes", 0) + sum(not p.has_work for p in pieces)
        counters["dropped_candidates"] = counters.get("dropped_candidates", 0) + sum(len(p.cands) for p in pieces[ended[0] + 1:])
        counters["steps"] = counters.get("steps", 0) + sum(p.steps for p in pieces)
    return [c for p in pieces[:ended[0] + 1] for c in p.cands]


def detect_chunked(seq, kmin, kmax, min_repeats, min_span, max_interruptions, chunk, stride=0, slots=0, episodes=None,
                   counters=None):
    """interrupted_model.detect() with every walk cut into chunks: the same rows for every chunk size."""
    s, head = M.trim(seq)
    if counters is not None and chunk == 0:
        counters["lanes"] = counters.get("lanes", 0) + (kmax - kmin + 1)
        counters.setdefault("dropped_lanes", 0)
    per_k = [(k, walk_chunked(s, k, min_repeats, min_span, max_interruptions, chunk, stride, slots, episodes, counters))
             for k in range(kmin, kmax + 1)]
    out = M.emit(per_k)
    return [(a + head, b + head, k, mask, M.motif_text(s, a, k, mask)) for (a, b), (k, mask) in sorted(out.items())]


def lane_count(seqs, kmin, kmax, chunk):
    """The lanes prf_scan_interrupted_chunked launches for these sequences."""
    return sum(n_chunks(len(M.trim(s)[0]), chunk) for s in seqs) * (kmax - kmin + 1)
