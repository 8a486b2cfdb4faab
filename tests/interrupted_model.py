"""A restatement of the interrupted-repeat driver in plain Python: the CPU model the GPU lane is checked against.

The driver the project pins for the reference's RepeatTracker with max_interruptions > 0: upper-case, trim the N at both ends,
then one tracker per motif size k = kmin .. kmax in ascending order over the trimmed sequence, all writing one shared
(start, end) -> motif dictionary; rows are the dictionary sorted, shifted by the trimmed head.

walk() computes the candidate list of one (sequence, k) in two ways that must agree:
  plain -- the tracker's moves one by one (it jumps back to its first interruption after every decision);
  memo  -- the same walk with a table of recorded states every `stride` positions: an episode that meets a state recorded
           by an earlier episode takes that episode's outcome and jumps at once.
emit() turns the candidate lists of one sequence into rows (the dictionary, the previous-output rule, the homopolymer rule).
"""

PENDING = None


class Walk:
    """Candidates of one (sequence, k) in path order, with counters."""

    def __init__(self):
        self.cands = []          # (start, end, phase mask, homopolymer)
        self.steps = 0           # advance() calls + extension steps
        self.landings = []       # positions a jump back resumes from
        self.lookups = 0
        self.hits = 0


def _homopolymer(seq, start, k, mask):
    bases = {seq[start + i] for i in range(k) if not (mask >> i) & 1}
    return k > 1 and len(bases) == 1


def _slot(pos, run, mask, slots):
    h = (pos * 0x9E3779B97F4A7C15 + run * 0xC2B2AE3D27D4EB4F + mask * 0x165667B19E3779F9) & 0xFFFFFFFFFFFFFFFF
    h ^= h >> 29
    h = (h * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    return (h >> 32) % slots


def walk(seq, k, min_repeats, min_span, max_interruptions, stride=0, slots=0, episodes=None):
    """seq: upper-cased, N-trimmed bytes.  stride == 0 or slots == 0: the plain walk.  Otherwise the memo walk: at every
    position that is a multiple of `stride` the state (position, run, phase set) is looked up in a table of `slots` records
    (hashed on the whole state, a new record replaces whatever held its slot) that remembers which episode passed through it;
    `episodes` (default: unbounded) caps the episodes whose outcome is remembered."""
    n = len(seq)
    w = Walk()
    pos = run = 0
    mask = n_int = 0
    first = -1                   # position of the first interruption, -1: none
    memo = [None] * slots if stride and slots else None
    outcome = []                 # per episode: PENDING, or (candidate or None, the walk ended there)
    r_span = min_repeats * k

    def close(result):
        if memo is not None and outcome and outcome[-1] is PENDING:
            outcome[-1] = result

    def open_episode():
        if memo is not None and (episodes is None or len(outcome) < episodes):
            outcome.append(PENDING)

    open_episode()
    while True:
        if memo is not None and pos % stride == 0:
            s = _slot(pos, run, mask, slots)
            rec = memo[s]
            if first >= 0:
                w.lookups += 1
            if (first >= 0 and rec is not None and rec[0] == pos and rec[1] == run and rec[2] == mask
                    and outcome[rec[3]] is not PENDING):
                w.hits += 1
                cand, at_end = outcome[rec[3]]
                if cand is not None:
                    w.cands.append(cand)
                close(outcome[rec[3]])
                if at_end:
                    return w
                pos = first + 1
                w.landings.append(pos)
                first, run, mask, n_int = -1, 0, 0, 0
                open_episode()
                continue
            if outcome and outcome[-1] is PENDING:
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

        # the output check (reference :145-222)
        if run + k < min_span or run + k < r_span:
            if at_end:
                close((None, True))
                return w
            run = 0                           # no reset: the first interruption and the phase set stay
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
                cand = (start, pos, mask, _homopolymer(seq, start, k, mask))
                w.cands.append(cand)
        close((cand, at_end))
        if at_end:
            return w
        if first >= 0:
            pos = first
            w.landings.append(pos + 1)
        first, run, mask, n_int = -1, 0, 0, 0
        pos += 1
        open_episode()


def emit(cands_by_k):
    """cands_by_k: [(k, candidates in path order)] in ascending k.  Returns {(start, end): (k, mask)}."""
    out = {}
    for k, cands in cands_by_k:
        prev_end = None
        last = None
        for c in cands:
            if c == last:
                continue
            last = c
            start, end, mask, homo = c
            if (start, end) in out or (prev_end is not None and end - prev_end < k) or homo:
                continue
            out[(start, end)] = (k, mask)
            prev_end = end
    return out


def trim(seq):
    """(upper-cased bytes without the N at both ends, number of bases trimmed off the front)."""
    s = seq.upper() if isinstance(seq, bytes) else seq.upper().encode()
    lo = len(s) - len(s.lstrip(b"N"))
    return s[lo:len(s.rstrip(b"N"))] if lo < len(s) else b"", lo


def motif_text(seq, start, k, mask):
    m = bytearray(seq[start:start + k])
    for i in range(k):
        if (mask >> i) & 1:
            m[i] = ord("N")
    return m.decode()


def detect(seq, kmin, kmax, min_repeats, min_span, max_interruptions, stride=0, slots=0, episodes=None, counters=None):
    """Rows [(start, end, k, mask, motif)] sorted by (start, end), as the pinned driver reports them."""
    s, head = trim(seq)
    per_k = []
    for k in range(kmin, kmax + 1):
        w = walk(s, k, min_repeats, min_span, max_interruptions, stride, slots, episodes)
        per_k.append((k, w.cands))
        if counters is not None:
            counters["steps"] = counters.get("steps", 0) + w.steps
            counters["lookups"] = counters.get("lookups", 0) + w.lookups
            counters["hits"] = counters.get("hits", 0) + w.hits
            counters.setdefault("landings", []).append(w.landings)
    out = emit(per_k)
    return [(a + head, b + head, k, mask, motif_text(s, a, k, mask)) for (a, b), (k, mask) in sorted(out.items())]
