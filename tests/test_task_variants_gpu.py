"""GPU (-m gpu): every exact-task variant (K, M) and every group-task form of the fused scan kernel (csrc/vscan_tasks.h:
exact_stream for M <= 8, coarse_stream for M = 9 .. 14, group_task<NC, S1, HALF>) on runs of exactly the minimal length.

The inputs come from tests/task_variants_cases.py; tests/test_task_variants_cpu.py asserts on the CPU that they hold what they
are built around and stay below the caps of a tile's lists.  Every scan is compared row for row with the CPU oracle and, bit for
bit, with the generic path; the rows of the threshold runs are asserted by position, and so is that no one-below run gives a row."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import task_variants_cases as tv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    import prf_native
    c = prf_native.Context(0)
    yield c
    c.close()


def oracle_rows(seqs, settings):
    from oracle import prf_oracle
    return [(ci, s, e, k) for ci, seq in enumerate(seqs) for s, e, _ml, k in prf_oracle.detect_rows(seq, *settings)]


def scan_and_compare(g, settings, oracle, want, never):
    """One fused scan against the oracle's rows (contig, start, end, k), the generic path and the constructs; returns its stats."""
    import prf_native
    rows, st = g.scan(*settings)
    assert st.path == 1, settings
    got = [(int(r["contig"]), int(r["start"]), int(r["end"]), int(r["k"])) for r in rows]
    if got != oracle:
        lost, extra = sorted(set(oracle) - set(got)), sorted(set(got) - set(oracle))
        raise AssertionError(f"{settings}: {len(got)} rows, the oracle has {len(oracle)}; missing {lost[:5]}, not in the oracle {extra[:5]}")
    have = set(got)
    starts = {(c, s, k) for c, s, _e, k in got}
    assert [w for w in want if w not in have] == [], settings
    assert [n for n in never if n in starts] == [], settings
    gen, stg = g.scan(*settings, flags=prf_native.SCAN_FORCE_GENERIC)
    assert stg.path == 0 and np.array_equal(rows, gen), settings
    return st


@pytest.mark.parametrize("K", range(1, tv.SMALL_M))
def test_single_variant(ctx, K):
    """The plan is the one exact task (K, M), M = K .. 14, on a clean and a mixed contig (task_variants_cases.exact_case): threshold
    and one-below runs at every row offset, in the lanes 0 and 63, at the tile's edges, two in one stream, beside N.  The
    candidates the device counts are this task's flags: at least one per stream in which a threshold run starts, and no more
    than the task's rule allows on this input (task_variants_cases.flag_bound): a window that tests too little shows here, not
    in the rows, which the verification derives again."""
    for M in range(K, tv.SMALL_M):
        clean, mixed = tv.exact_case(K, M, False), tv.exact_case(K, M, True)
        settings = tv.single_setting(K, M)
        seqs = [clean.seq, mixed.seq]
        g = ctx.load(seqs, 50)
        try:
            assert g.tile_classes(0).tolist() == [0, 0, 0, 1, 1]    # (the last tile holds the contig's last 64 positions)
            assert g.tile_classes(1).tolist() == [1, 1, 1, 1]
            want = [(ci,) + w for ci, c in enumerate((clean, mixed)) for w in c.want]
            never = [(ci,) + n for ci, c in enumerate((clean, mixed)) for n in c.never]
            st = scan_and_compare(g, settings, oracle_rows(seqs, settings), want, never)
            bound = tv.flag_bound(seqs, K, M)
            print("K", K, "M", M, "rows", st.n_hits, "candidates", st.n_candidates, "threshold streams", clean.threshold_streams() + mixed.threshold_streams(),
                  "bound", bound)
            assert clean.threshold_streams() + mixed.threshold_streams() <= st.n_candidates <= bound, (K, M)
        finally:
            g.free()


def test_span_sweep_nc72(ctx):
    """(1, 22, 2, s), s = 8 .. 28: all exact tasks of a plan at once, beside group tasks (item0, the dispatch, the flags' task tags),
    on one contig with three runs of every size at every span's threshold length and one below it, one of the three on the mixed
    tile.  At the spans 8 - 10 the plan derives the k = 1 flags of a clean tile from the k = 2 task (prf_plan_derives_k1): there
    the variants (1, 7), (1, 8) and (1, 9) themselves run on the mixed tile only, and the clean tiles exercise the derived path."""
    case = tv.sweep72_case()
    g = ctx.load([case.seq], 50)
    try:
        assert g.tile_classes(0).tolist() == [0] * (case.n_tiles - 2) + [1, 1]
        for span in tv.SWEEP_SPANS:
            settings = tv.sweep_settings(tv.SWEEP72, span)
            want, never = case.expect(span)
            st = scan_and_compare(g, settings, oracle_rows([case.seq], settings), [(0,) + w for w in want], [(0,) + n for n in never])
            print("span", span, "rows", st.n_hits, "candidates", st.n_candidates)
    finally:
        g.free()


def test_span_sweep_nc80(ctx):
    """(1, 264, 2, s), s = 8 .. 28, on a contig of two clean and two mixed tiles, every run on either kind: the image of 80 virtual
    lanes.  (As in the narrow sweep, (1, 7), (1, 8) and (1, 9) run on the mixed tiles only.)  This runs 93 of the 105 variants at
    the wide image; the 12 with K + M <= 7 are not run there (no span from 8 on gives them; below 8 a background gives thousands
    of rows per tile).  Runs of the sizes 100 and 255 - 264 sit beside the small ones: the task of the sizes 256 - 263 is the one that
    reads the image's last lanes.  The oracle's rows come from two calls (task_variants_cases.sweep80_oracle)."""
    import prf_native
    case = tv.sweep80_case()
    g = ctx.load([case.seq], tv.SWEEP80[1])
    try:
        assert g.tile_classes(0).tolist() == [0, 0, 1, 1, 1]
        for span in tv.SWEEP_SPANS:
            settings = tv.sweep_settings(tv.SWEEP80, span)
            assert prf_native.plan_describe(*settings)["nc"] == 80
            want, never = case.expect(span)
            oracle = [(0, s, e, k) for s, e, _ml, k in tv.sweep80_oracle(span)]
            st = scan_and_compare(g, settings, oracle, [(0,) + w for w in want], [(0,) + n for n in never])
            print("span", span, "rows", st.n_hits, "candidates", st.n_candidates)
    finally:
        g.free()


@pytest.mark.parametrize("name", list(tv.GROUP_CASES))
def test_group_forms(ctx, name):
    """The six forms of the group task and the tight thresholds M = 8 S + 7 (task_variants_cases.GROUP_SETTINGS): threshold and
    one-below runs of every size of every group task at every row offset, in clean tiles (stride 1: the S1 code) and in the mixed
    last tile (the other code for the same sizes); (1, 50, 2, 40), whose short motifs echo at up to 50 sizes, as four contigs of
    eight offsets each; one setting a second time with an N in a middle tile."""
    case = tv.group_case(*tv.GROUP_CASES[name])
    g = ctx.load([case.seq], 50)
    try:
        classes = g.tile_classes(0).tolist()
        if tv.GROUP_CASES[name][1]:
            mixed = {case.lone_n // tv.TILE - 1, case.lone_n // tv.TILE, case.n_tiles - 2, case.n_tiles - 1}
            assert classes == [1 if t in mixed else 0 for t in range(case.n_tiles)]
        else:
            assert classes == [0] * (case.n_tiles - 2) + [1, 1]
        st = scan_and_compare(g, case.settings, oracle_rows([case.seq], case.settings), [(0,) + w for w in case.want],
                              [(0,) + n for n in case.never])
        print(name, "tiles", case.n_tiles, "rows", st.n_hits, "candidates", st.n_candidates)
    finally:
        g.free()
