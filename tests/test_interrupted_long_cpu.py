"""CPU: the interrupted-repeat models (tests/interrupted_model.py, tests/interrupted_chunks_model.py) against the reference's
RepeatTracker at 3-40 kb (tests/golden/interrupted_long.jsonl.gz, written by tools/gen_interrupted_golden.py --long), and the
conditions the fixture has to keep so that it cannot quietly shrink."""
import pytest

import interrupted_chunks_model as C
import interrupted_model as M
from conftest import load_jsonl_gz

PLAIN_WALK_CAP = 20_000       # the plain walk is quadratic: it leaves out the cases longer than this, and no others


@pytest.fixture(scope="module")
def golden_long():
    return load_jsonl_gz("interrupted_long.jsonl.gz")


def _settings(case):
    st = case["settings"]
    return st["min_motif_size"], st["max_motif_size"], st["min_repeats"], st["min_span"], st["max_interruptions"]


def _differing(cases, rows_of):
    return [(i, c["tag"], len(c["seq"])) for i, c in enumerate(cases)
            if [[a, b, motif] for a, b, _k, _mask, motif in rows_of(c)] != c["rows"]]


@pytest.fixture(scope="module")
def plain_walks(golden_long):
    """Per case of at most PLAIN_WALK_CAP positions: (rows, {k: tracker moves}) of the plain walk."""
    out = {}
    for i, c in enumerate(golden_long):
        if len(c["seq"]) > PLAIN_WALK_CAP:
            continue
        kmin, kmax, r, span, m = _settings(c)
        s, head = M.trim(c["seq"])
        walks = [(k, M.walk(s, k, r, span, m)) for k in range(kmin, kmax + 1)]
        rows = [[a + head, b + head, M.motif_text(s, a, k, mask)]
                for (a, b), (k, mask) in sorted(M.emit([(k, w.cands) for k, w in walks]).items())]
        out[i] = (rows, {k: w.steps for k, w in walks})
    return out


@pytest.mark.parametrize("memo", [(8, 1 << 16, None), (1, 7, 5)], ids=["stride8", "stride1_7slots_5episodes"])
def test_memo_walk_matches_every_long_case(golden_long, memo):
    bad = _differing(golden_long, lambda c: M.detect(c["seq"], *_settings(c), *memo))
    assert not bad, f"{len(bad)} of {len(golden_long)} cases differ: {bad[:5]}"


def test_plain_walk_matches_every_long_case_up_to_the_cap(golden_long, plain_walks):
    left_out = [i for i, c in enumerate(golden_long) if len(c["seq"]) > PLAIN_WALK_CAP]
    print(f"plain walk: {len(plain_walks)} cases, {len(left_out)} left out (longer than {PLAIN_WALK_CAP} positions)")
    assert len(left_out) == 1 and len(plain_walks) == len(golden_long) - 1
    bad = [(i, golden_long[i]["tag"]) for i, (rows, _steps) in plain_walks.items() if rows != golden_long[i]["rows"]]
    assert not bad, f"{len(bad)} of {len(plain_walks)} cases differ: {bad[:5]}"


@pytest.mark.parametrize("chunk", [7, 1000, 4096, 1 << 16])
def test_chunked_model_matches_every_long_case(golden_long, chunk):
    assert chunk < 1 << 16 or all(len(c["seq"]) < chunk for c in golden_long)
    bad = _differing(golden_long, lambda c: C.detect_chunked(c["seq"], *_settings(c), chunk, 8, 1 << 12))
    assert not bad, f"chunk {chunk}: {len(bad)} of {len(golden_long)} cases differ: {bad[:5]}"


def test_long_fixture_keeps_its_reach(golden_long):
    assert 30 <= len(golden_long) <= 60
    assert sum(len(c["seq"]) >= 10_000 for c in golden_long) >= 8
    assert any(len(c["seq"]) >= 40_000 for c in golden_long)
    assert max(c["settings"]["max_interruptions"] for c in golden_long) >= 64
    assert any(c["settings"]["max_motif_size"] == 64 for c in golden_long)
    assert {(c["settings"]["min_motif_size"], c["settings"]["max_motif_size"]) for c in golden_long} >= {(1, 6), (2, 8), (16, 64), (60, 64)}
    assert {c["settings"]["min_repeats"] for c in golden_long} >= {2, 3, 5}
    assert {c["settings"]["min_span"] for c in golden_long} >= {1, 5, 9, 100}
    assert {c["settings"]["max_interruptions"] for c in golden_long} >= {1, 2, 3, 4, 6, 8, 64}
    # m >= k for every k of the range
    assert any(c["settings"]["max_interruptions"] >= c["settings"]["max_motif_size"] and c["settings"]["min_motif_size"] == 1 for c in golden_long)
    assert {"random", "random_planted", "low_complexity", "large_k", "large_k_unit64", "many_interruptions", "thresholds", "n_block",
            "lower_n_block", "iupac", "n_ends_lower_iupac"} <= {c["tag"] for c in golden_long}
    assert len({_settings(c) for c in golden_long}) <= 24       # a palette: the GPU tests make one call per setting
    # a unit of exactly 64 reported with phase 63 varying: the top bit of the phase mask
    assert any(len(motif) == 64 and motif[63] == "N" for c in golden_long for _a, _b, motif in c["rows"])
    assert all(c["rows"] for c in golden_long)


def test_low_complexity_cases_overflow_the_one_lane_room(golden_long):
    """The one-lane engine gives a lane len / 4 + 16 candidate slots and len / 4 + 64 recorded episodes (csrc/interrupted.cpp,
    size_walk_room): some (sequence, k) of the fixture has to exceed each, or the count-only second walk never runs."""
    most_cands = most_eps = 0
    for c in golden_long:
        if c["tag"] != "low_complexity":
            continue
        kmin, kmax, r, span, m = _settings(c)
        s, _head = M.trim(c["seq"])
        assert len(s) == len(c["seq"])
        for k in range(kmin, kmax + 1):
            w = M.walk(s, k, r, span, m, stride=8, slots=1 << 16)
            most_cands = max(most_cands, len(w.cands) - (len(s) // 4 + 16))
            most_eps = max(most_eps, len(w.landings) + 1 - (len(s) // 4 + 64))
    assert most_cands > 0 and most_eps > 0, (most_cands, most_eps)


def test_random_long_cases_reach_the_stale_phase_set_regime(golden_long, plain_walks):
    """40-260 tracker moves per position on random sequence at 10-40 kb (r 3, span 9).  Every random case of that
    length and those thresholds walked here has to show at least the lower figure for some k.  The random cases with r 2 and
    span 5 are not held to it: the figure is for r 3 and span 9, and with the lower thresholds the first span test passes sooner,
    so episodes close before their phase set goes stale.  The 40 kb case is not walked plainly (PLAIN_WALK_CAP)."""
    seen = 0
    for i, (_rows, steps) in plain_walks.items():
        c = golden_long[i]
        if not c["tag"].startswith("random") or len(c["seq"]) < 10_000 or _settings(c)[2:4] != (3, 9):
            continue
        per_position = {k: round(n / len(c["seq"]), 1) for k, n in steps.items()}
        print(c["tag"], len(c["seq"]), _settings(c), per_position)
        assert max(per_position.values()) >= 40, per_position
        seen += 1
    assert seen >= 3
