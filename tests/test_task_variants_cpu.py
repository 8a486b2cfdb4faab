"""CPU (-m "not gpu"): what tests/test_task_variants_gpu.py is built around (tests/task_variants_cases.py), asserted without a
device -- the planner's plans (prf_native.plan_describe needs no GPU), the oracle's rows at the planted runs, and the caps per
tile that keep a case on the task's own path (flag list, row sublists, record list) and off the overflow paths."""
import collections

import numpy as np
import pytest

import prf_native
import task_variants_cases as tv
from oracle import prf_oracle

# the oracle's row counts, (clean contig, mixed contig) for M = K .. 14: 43 planted rows in the clean contig (32 offsets, 3 + 3 in
# the lanes 0 and 63, 3 at the tiles' edges, 2 in one stream), 50 in the mixed one (2 at the edges, 8 beside N), and the background's own
EXACT_ROWS = {
    1: [(43, 50), (43, 50), (43, 50), (824, 638), (233, 193), (89, 85), (54, 56), (44, 51), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50)],
    2: [(43, 50), (43, 50), (628, 484), (214, 175), (95, 95), (52, 57), (45, 50), (45, 51), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50)],
    3: [(43, 50), (736, 557), (233, 193), (84, 77), (52, 59), (47, 54), (44, 51), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50)],
    4: [(803, 607), (222, 194), (81, 75), (49, 56), (43, 50), (44, 51), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50)],
    5: [(232, 199), (93, 86), (55, 57), (44, 51), (44, 50), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50)],
    6: [(83, 79), (60, 61), (46, 53), (44, 51), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50)],
    7: [(59, 63), (47, 53), (45, 51), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50)],
    8: [(48, 54), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50)],
    9: [(43, 50), (43, 50), (43, 50), (43, 50), (43, 50), (43, 50)],
    10: [(43, 50), (43, 50), (43, 50), (43, 50), (43, 50)],
    11: [(43, 50), (43, 50), (43, 50), (43, 50)],
    12: [(43, 50), (43, 50), (43, 50)],
    13: [(43, 50), (43, 50)],
    14: [(43, 50)],
}
SWEEP72_ROWS = [1244, 1067, 997, 770, 686, 604, 561, 508, 479, 431, 401, 370, 343, 313, 283, 249, 216, 180, 144, 105, 66]
SWEEP80_ROWS = [926, 764, 702, 538, 467, 408, 383, 351, 328, 301, 281, 258, 240, 219, 199, 177, 154, 130, 106, 80, 54]
GROUP_ROWS = {"8_15_2_30": 264, "8_15_2_38": 264, "8_15_2_54": 264, "15_22_2_1": 264, "23_26_2_1": 132, "39_42_2_1": 132,
              "8_26_2_1": 401, "48_50_2_1": 99, "1_50_2_40_o0": 450, "1_50_2_40_o8": 450, "1_50_2_40_o16": 450,
              "1_50_2_40_o24": 450, "8_26_2_1_N": 401}
# the variants a sweep over the spans 8 .. 28 cannot reach: M(k) = max(k, span - k) >= span - k, so K + M >= 8
BELOW_SWEEP = [(K, M) for K, M in tv.VARIANTS if K + M <= 7]


def check_rows(rows, want, never):
    """Every threshold run is a row at its position; no row of a one-below run's size starts where that run starts."""
    have = {(s, e, k) for s, e, _ml, k in rows}
    starts = {(s, k) for s, _e, _ml, k in rows}
    assert [w for w in want if w not in have] == []
    assert [n for n in never if n in starts] == []


def check_caps(seq, settings, rows, n_tiles):
    """Run starts of all exact tasks (planted and the background's own) per tile, and rows per quarter tile."""
    a = np.frombuffer(seq, dtype=np.uint8)
    flags = np.zeros(n_tiles, dtype=np.int64)
    for K, M in tv.exact_variants_of(settings):
        flags += tv.per_tile(tv.run_starts(a, K, M), n_tiles)
    assert flags.max() <= tv.MAX_FLAGS, flags
    per_quarter = collections.Counter(s // (tv.TILE // 4) for s, _e, _ml, _k in rows)
    assert max(per_quarter.values()) <= tv.MAX_QROWS, per_quarter.most_common(3)
    return int(flags.max()), max(per_quarter.values())


def test_single_variant_settings_give_one_task():
    """All 105 (K, M): the plan of single_setting(K, M) is the one exact task {kind: M, k0: K}, in the image of 72 lanes."""
    assert len(tv.VARIANTS) == 105
    for K, M in tv.VARIANTS:
        plan = prf_native.plan_describe(*tv.single_setting(K, M))
        assert plan["path"] == "fused" and plan["nc"] == 72
        assert [(t["kind"], t["k0"]) for t in plan["tasks"]] == [(M, K)], (K, M)


@pytest.mark.parametrize("krange,nc", [(tv.SWEEP72, 72), (tv.SWEEP80, 80)])
def test_span_sweeps_reach_93_variants(krange, nc):
    """(1, 22, 2, s) and (1, 264, 2, s), s = 8 .. 28: every plan has exact tasks beside group tasks at its image width, and together
    the plans hold all variants but the 12 with K + M <= 7."""
    seen = set()
    for span in tv.SWEEP_SPANS:
        settings = tv.sweep_settings(krange, span)
        plan = prf_native.plan_describe(*settings)
        assert plan["path"] == "fused" and plan["nc"] == nc
        exact = tv.exact_variants_of(settings)
        assert exact and tv.group_tasks_of(settings)
        ks = [K for K, _M in exact]
        assert ks == list(range(ks[0], ks[0] + len(ks)))
        seen |= set(exact)
    assert len(BELOW_SWEEP) == 12
    assert sorted(seen) == sorted(set(tv.VARIANTS) - set(BELOW_SWEEP))


def test_group_settings_reach_the_forms():
    """The six forms {stride 1, 2, 4} x {half, full}; per stride S a task whose smallest M is exactly 8 S + 7, the least run that
    must hold an examined group; valid masks with a hole at the low end, at the high end and at both; a plan whose first group
    task starts at k0 = 0."""
    forms, tight, masks, k0s = set(), set(), set(), set()
    for settings in tv.GROUP_SETTINGS:
        for k0, valid, stride, half, sizes in tv.group_tasks_of(settings):
            forms.add((stride, half))
            if min(M for _k, M in sizes) == 8 * stride + 7:
                tight.add(stride)
            masks.add(valid)
            k0s.add(k0)
            assert half == (valid & 0xF0 == 0) and all(M >= tv.SMALL_M for _k, M in sizes)
    assert forms == {(s, h) for s in (1, 2, 4) for h in (False, True)}
    assert tight == {1, 2, 4}
    assert {0xFF, 0xF8, 0x78, 0x07, 0x0F, 0xFE} <= masks, sorted(masks)
    assert 0 in k0s
    # the settings named for a form give it
    assert (2, True, 7) in {(s, h, v) for _k0, v, s, h, _z in tv.group_tasks_of((8, 26, 2, 1))}
    assert (1, False, 255) in {(s, h, v) for _k0, v, s, h, _z in tv.group_tasks_of((1, 50, 2, 40))}
    assert (4, True, 7) in {(s, h, v) for _k0, v, s, h, _z in tv.group_tasks_of((48, 50, 2, 1))}
    assert tv.exact_variants_of((8, 26, 2, 1)) == [(k, k) for k in range(8, 15)]


@pytest.mark.parametrize("K", range(1, tv.SMALL_M))
def test_exact_cases(K):
    worst = (0, 0)
    for M in range(K, tv.SMALL_M):
        for mixed in (False, True):
            case = tv.exact_case(K, M, mixed)
            assert len(case.arr) == tv.exact_len(mixed) and case.settings == tv.single_setting(K, M)
            rows = prf_oracle.detect_rows(case.seq, *case.settings)
            check_rows(rows, case.want, case.never)
            assert len(case.want) == (50 if mixed else 43) and len(case.never) >= (44 if mixed else 38)
            assert len(rows) == EXACT_ROWS[K][M - K][mixed], (K, M, mixed, len(rows))
            worst = max(worst, check_caps(case.seq, case.settings, rows, case.n_tiles))
            # every row offset and every lane holds a threshold run
            in_tile = [s - tv.TILE for s, _e, _k in case.want if tv.TILE <= s < 2 * tv.TILE]
            assert {s % tv.T for s in in_tile} == set(range(tv.T))
            assert {s // tv.T % 64 for s, _k in case.never} | {s // tv.T % 64 for s in in_tile} == set(range(64))
            assert (np.frombuffer(case.seq, dtype=np.uint8) == tv.N).sum() == (14 if mixed else 0)
            # a run across the edge between two clean tiles (clean contig), between two mixed ones (mixed contig)
            assert any(s < 2 * tv.TILE < e for s, e, _k in case.want)
            assert any(s < tv.TILE < e for s, e, _k in case.want) == mixed and ((tv.TILE, tv.TILE + M + K, K) in case.want) != mixed
        # the bound of the device's candidate count leaves room for the threshold runs' own streams
        pair = [tv.exact_case(K, M, False), tv.exact_case(K, M, True)]
        assert tv.flag_bound([c.seq for c in pair], K, M) >= sum(c.threshold_streams() for c in pair) + 8
    print("K", K, "most run starts per tile, most rows per quarter:", worst)


def test_sweep72_case():
    case = tv.sweep72_case()
    assert np.all(np.frombuffer(case.seq, dtype=np.uint8) != tv.N)
    for span, n_rows in zip(tv.SWEEP_SPANS, SWEEP72_ROWS):
        settings = tv.sweep_settings(tv.SWEEP72, span)
        rows = prf_oracle.detect_rows(case.seq, *settings)
        want, never = case.expect(span)
        assert len(want) == 3 * 22 and len(never) == 3 * 22          # three runs of every size at the threshold and one below
        mixed_tile = case.n_tiles - 2                                # every size on the mixed tile and on clean ones
        assert {k for s, _e, k in want if s // tv.TILE == mixed_tile} == {k for s, _e, k in want if s // tv.TILE < mixed_tile} == set(range(1, 23))
        assert {k for s, k in never if s // tv.TILE == mixed_tile} == {k for s, k in never if s // tv.TILE < mixed_tile} == set(range(1, 23))
        check_rows(rows, want, never)
        assert len(rows) == n_rows, (span, len(rows))
        check_caps(case.seq, settings, rows, case.n_tiles)


def test_sweep80_case():
    """The wide sweep's rows come from two oracle calls (task_variants_cases.sweep80_oracle): the same as one call at span 8."""
    case = tv.sweep80_case()
    large = tv.sweep80_large_rows()
    assert sorted((k, e - s) for s, e, _ml, k in large) == sorted(2 * [(255, 510), (256, 512), (263, 526), (100, 200), (264, 528)])
    assert (np.frombuffer(case.seq, dtype=np.uint8) == tv.N).sum() == 1      # it makes the third tile mixed as well
    first = tv.SWEEP_SPANS[0]
    assert tv.sweep80_oracle(first) == prf_oracle.detect_rows(case.seq, *tv.sweep_settings(tv.SWEEP80, first))
    for span, n_rows in zip(tv.SWEEP_SPANS, SWEEP80_ROWS):
        rows = tv.sweep80_oracle(span)
        want, never = case.expect(span)
        assert len(want) == 2 * (22 + len(tv.SWEEP80_EXTRA)) and len(never) == len(want)
        for part in (want, never):       # every size on a mixed tile (the tiles 2, 3) and on a clean one
            assert {r[-1] for r in part if r[0] // tv.TILE >= 2} == {r[-1] for r in part if r[0] // tv.TILE < 2} == set(range(1, 23)) | set(tv.SWEEP80_EXTRA)
        check_rows(rows, want, never)
        assert len(rows) == n_rows, (span, len(rows))
        check_caps(case.seq, tv.sweep_settings(tv.SWEEP80, span), rows, case.n_tiles)


@pytest.mark.parametrize("name", list(GROUP_ROWS))
def test_group_cases(name):
    case = tv.group_case(*tv.GROUP_CASES[name])
    rows = prf_oracle.detect_rows(case.seq, *case.settings)
    check_rows(rows, case.want, case.never)
    assert len(rows) == GROUP_ROWS[name], len(rows)
    check_caps(case.seq, case.settings, rows, case.n_tiles)
    assert max(case.n_group.values()) <= tv.MAX_GROUP
    bound = tv.group_records_bound(case.seq, case.settings, case.n_tiles - 1)
    print(name, "tiles", case.n_tiles, "constructs per tile", list(case.n_group.values()), "records per tile at most", bound.tolist())
    assert bound.max() <= tv.REC_CAP
    # every size of every group task at every offset of the case's block, threshold and one below, on clean tiles; both kinds of
    # every size in the mixed last tile too
    sizes = [k for _k0, _v, _s, _h, ks in tv.group_tasks_of(case.settings) for k, _M in ks]
    offsets = set(tv.GROUP_SETTINGS[case.settings][tv.GROUP_CASES[name][2]])
    last = (case.n_tiles - 2) * tv.TILE
    for k in sizes:
        assert offsets <= {s % tv.T for s, _e, kk in case.want if kk == k and s < last}
        assert offsets <= {s % tv.T for s, kk in case.never if kk == k and s < last}
        assert any(kk == k and s >= last for s, _e, kk in case.want) and any(kk == k and s >= last for s, kk in case.never)
    n_count = int((np.frombuffer(case.seq, dtype=np.uint8) == tv.N).sum())
    assert n_count == (1 if name.endswith("_N") else 0)


def test_group_settings_have_every_offset():
    """The blocks of offsets of a setting's cases make up 0 .. 31."""
    for settings, blocks in tv.GROUP_SETTINGS.items():
        assert sorted(off for block in blocks for off in block) == list(range(tv.T)), settings
        assert sum(args[0] == settings and not args[1] for args in tv.GROUP_CASES.values()) == len(blocks)
