"""The interrupted-repeat driver with a budget of varying phases per motif size in plain Python: the CPU model of
prf_scan_interrupted_by_k.

The driver of interrupted_model.py with one change: the tracker of motif size k walks with its own max_interruptions m_k.  The
walk of a (sequence, k) depends on k's own budget alone and the emission is the same, so this module only hands each k its budget:
interrupted_model.walk / interrupted_chunks_model.walk_chunked per k, then interrupted_model.emit over all of them.
"""
import interrupted_chunks_model as C
import interrupted_model as M


def budgets(kmin, kmax, by_k, max_interruptions=0):
    """{k: budget} for k = kmin .. kmax.  by_k: None (max_interruptions for every k), a dict {k: m} (a k it omits takes
    max_interruptions; other keys are ignored), or a sequence with one entry per k."""
    if by_k is None:
        return {k: max_interruptions for k in range(kmin, kmax + 1)}
    if isinstance(by_k, dict):
        return {k: by_k.get(k, max_interruptions) for k in range(kmin, kmax + 1)}
    assert len(by_k) == kmax - kmin + 1
    return {kmin + j: m for j, m in enumerate(by_k)}


def _rows(s, head, per_k):
    out = M.emit(per_k)
    return [(a + head, b + head, k, mask, M.motif_text(s, a, k, mask)) for (a, b), (k, mask) in sorted(out.items())]


def detect(seq, kmin, kmax, min_repeats, min_span, by_k, max_interruptions=0, stride=0, slots=0, episodes=None, counters=None):
    """interrupted_model.detect() with the budget of budgets() for each k: rows [(start, end, k, mask, motif)] sorted by (start, end)."""
    s, head = M.trim(seq)
    m_of = budgets(kmin, kmax, by_k, max_interruptions)
    per_k = []
    for k in range(kmin, kmax + 1):
        w = M.walk(s, k, min_repeats, min_span, m_of[k], stride, slots, episodes)
        per_k.append((k, w.cands))
        if counters is not None:
            counters["steps"] = counters.get("steps", 0) + w.steps
            counters["lookups"] = counters.get("lookups", 0) + w.lookups
            counters["hits"] = counters.get("hits", 0) + w.hits
    return _rows(s, head, per_k)


def detect_chunked(seq, kmin, kmax, min_repeats, min_span, by_k, chunk, max_interruptions=0, stride=0, slots=0, episodes=None,
                   counters=None):
    """interrupted_chunks_model.detect_chunked() with the budget of budgets() for each k: the same rows for every chunk size."""
    s, head = M.trim(seq)
    m_of = budgets(kmin, kmax, by_k, max_interruptions)
    if counters is not None and chunk == 0:
        counters["lanes"] = counters.get("lanes", 0) + (kmax - kmin + 1)
        counters.setdefault("dropped_lanes", 0)
    return _rows(s, head, [(k, C.walk_chunked(s, k, min_repeats, min_span, m_of[k], chunk, stride, slots, episodes, counters))
                           for k in range(kmin, kmax + 1)])
