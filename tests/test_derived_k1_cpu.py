"""CPU: why the fused kernel may read the k = 1 task's flags off the k = 2 task (csrc/vscan_tasks.h, exact_stream<2, M>), and
when the planner says so (csrc/prf_plan.h, prf_plan_derives_k1).

The model.  M(k) = max((r - 1) k, span - k) matches make a reportable run.  A start of the size-k task is a position t whose M(k)
rows t .. t+M-1 match at distance k while row t-1 does not.  The k = 2 task tests whether a start's two letters are equal (an
echo of the motif of one letter) and throws such a start away; the derivation hands those starts to k = 1 instead.  Over every
string of 15 letters from {A, C} between two sentinel letters:
  * M(2) + 1 == M(1): the k = 1 starts ARE the k = 2 starts with equal letters;
  * min_span >= 2 min_repeats: every k = 1 start is among them (the planner's condition; it implies the line above);
  * otherwise some string has a k = 1 start that is not: the condition cannot be weakened."""
import itertools

import numpy as np
import pytest

import prf_native

LEN = 15
REPEATS = (2, 3, 4)
SPANS = tuple(range(2, 12))


def M(k, r, span):
    return max((r - 1) * k, span - k)


_strings = None


def strings():
    """Every string over two letters of length LEN, a sentinel letter of its own in front and behind: one row each."""
    global _strings
    if _strings is None:
        n = np.arange(1 << LEN, dtype=np.uint32)
        s = np.empty((1 << LEN, LEN + 2), dtype=np.uint8)
        s[:, 0] = 2
        s[:, -1] = 3
        for i in range(LEN):
            s[:, 1 + i] = (n >> i) & 1
        _strings = s
    return _strings


_matches = {}


def matches(k):
    """[string, t]: the letters t and t + k are equal (False where t + k lies behind the string)."""
    if k not in _matches:
        s = strings()
        m = np.zeros(s.shape, dtype=bool)
        m[:, :-k] = s[:, :-k] == s[:, k:]
        _matches[k] = m
    return _matches[k]


_starts = {}


def starts(k, m_min):
    """[string, t]: rows t .. t + m_min - 1 match at distance k and row t - 1 does not (or there is none)."""
    if (k, m_min) not in _starts:
        m = matches(k)
        width = m.shape[1]
        run = np.ones(m.shape, dtype=bool)
        for i in range(m_min):
            shifted = np.zeros(m.shape, dtype=bool)
            shifted[:, :width - i] = m[:, i:]
            run &= shifted
        before = np.zeros(m.shape, dtype=bool)
        before[:, 1:] = m[:, :-1]
        _starts[(k, m_min)] = run & ~before
    return _starts[(k, m_min)]


def start_sets(r, span):
    """(the k = 1 task's starts, the k = 2 task's starts whose two letters are equal)"""
    return starts(1, M(1, r, span)), starts(2, M(2, r, span)) & matches(1)


@pytest.mark.parametrize("r,span", list(itertools.product(REPEATS, SPANS)))
def test_k1_starts_against_k2_echo_starts(r, span):
    k1, echo2 = start_sets(r, span)
    assert k1.any() or M(1, r, span) + 1 > LEN        # (the model is not vacuous)
    missed = int((k1 & ~echo2).any(axis=1).sum())      # strings with a k = 1 start that is no k = 2 echo start
    extra = int((echo2 & ~k1).any(axis=1).sum())
    print(f"min_repeats {r} min_span {span}: M(1) {M(1, r, span)} M(2) {M(2, r, span)}: strings with a missed start {missed}, "
          f"with an extra one {extra}")
    if M(2, r, span) + 1 == M(1, r, span):
        assert missed == 0 and extra == 0
    if span >= 2 * r:
        assert missed == 0
        assert M(2, r, span) + 1 == M(1, r, span)      # (so the derived flags are the task's flags, not a superset)
    else:
        assert missed > 0


def tasks_of(settings):
    plan = prf_native.plan_describe(*settings)
    assert plan["path"] == "fused"
    return plan["tasks"]


DERIVED = ((1, 50, 3, 9), (1, 2, 3, 9), (1, 6, 2, 4), (1, 6, 4, 8), (1, 6, 2, 10))
NOT_DERIVED = ((1, 1, 3, 9),     # no k = 2 task
               (2, 6, 3, 9),     # k = 1 is not asked for
               (1, 6, 3, 5),     # min_span < 2 min_repeats
               (1, 6, 2, 11))    # M(2) = 9: the coarse form, which has no echo test


@pytest.mark.parametrize("settings", DERIVED)
def test_plan_derives_k1(settings):
    _kmin, _kmax, r, span = settings
    tasks = tasks_of(settings)
    by_k = {t["k0"]: t for t in tasks if t["kind"]}
    assert by_k[1]["derive"] == 1 and by_k[1]["kind"] == M(1, r, span)      # the task stays in the plan: mixed tiles run it
    assert by_k[2]["derive"] == 2 and by_k[2]["kind"] == M(2, r, span) <= 8
    assert all(t["derive"] == 0 for t in tasks if t is not by_k[1] and t is not by_k[2])


def test_plan_derives_k1_in_the_coarse_form():
    assert M(1, 2, 10) == 9                                                 # k = 1 itself would take the coarse form
    assert {t["k0"]: t["derive"] for t in tasks_of((1, 6, 2, 10)) if t["kind"]}[1] == 1


@pytest.mark.parametrize("settings", NOT_DERIVED)
def test_plan_does_not_derive_k1(settings):
    assert all(t["derive"] == 0 for t in tasks_of(settings))


def test_planner_condition_over_a_sweep():
    """derive is set exactly where kmin = 1 < kmax, M(2) <= 8 and min_span >= 2 min_repeats."""
    for kmin, kmax, r, span in itertools.product((1, 2), (1, 2, 7, 50), (2, 3, 4, 5, 7), range(1, 16)):
        if kmax < kmin:
            continue
        want = kmin == 1 and kmax >= 2 and M(2, r, span) <= 8 and span >= 2 * r
        got = {t["k0"]: t["derive"] for t in tasks_of((kmin, kmax, r, span)) if t["kind"]}
        assert (got.get(1, 0), got.get(2, 0)) == ((1, 2) if want else (0, 0)), (kmin, kmax, r, span)
        assert all(t["derive"] == 0 for t in tasks_of((kmin, kmax, r, span)) if not t["kind"] or t["k0"] > 2)
