"""GPU (-m gpu): the hand-over from the scan phase of the fused kernel to its verify phase (csrc/scan_vertical.hip): the waves
arrive from their tasks in an order the plan's deal decides, the first two load the window of the linear planes and store it
behind the barrier, and the arrival counter (`cnt` parity, CNT_ROWS0) is reused from tile to tile and from scan to scan.

One genome of four contigs, built around what crosses that hand-over:
  A  2 tiles + 4 000 bp: a k = 20 run that starts 6 positions in front of tile 1 (its first examined group lies in the next tile:
     the boundary pass reports it), a k = 3 run across the edge between tile 1 and the tail;
  B  3 tiles + 37 bp: an N block inside tile 1 (mixed) beside the clean tile 0, homopolymers on both sides of the block, a k = 3
     run across the edge of the clean and the mixed tile, a k = 45 run that starts 10 positions in front of tile 2;
  C  2 tiles + 64 bp: a k = 7 run from 2 000 positions in front of tile 1 to 1 500 behind its start (it ends in the last 1 536
     positions of tile 0's window);
  D  2 tiles + 100 bp: a k = 3 run from 9 000 positions in front of tile 1 to 3 000 behind its start: it leaves tile 0's window.
Settings: one wave with tasks and three without (3 - 3), two waves with tasks (2 - 3), the default 1 - 50, 1 - 100, a plan of the
wide image (1 - 280: nc 80) and one that does not derive the k = 1 flags (min_span < 2 min_repeats).  Fused = generic = oracle row
for row; every setting is scanned twice on one context and three times pipelined, two scans in flight.  Nothing here depends on
the deal or on the priorities: the file passes on a library whose plan is dealt differently."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libprf: see test_gpu_parity.py)

import pipelined_edges_cases as cases
from test_echo_flags_gpu import BASES, N, TILE, plant, primitive_motif

pytestmark = pytest.mark.gpu

SETTINGS = {"one_wave_3-3": (3, 3, 3, 9), "two_waves_2-3": (2, 3, 3, 9), "default_1-50": (1, 50, 3, 9), "1-100": (1, 100, 3, 9),
            "nc80_1-280": (1, 280, 3, 9), "not_derived_1-50_r5": (1, 50, 5, 9)}
KMAX_HINT = 280
WINDOW_POST = 1536                  # positions of the linear window behind the tile (csrc/prf_plan.h: 64 LIN_POST)


def genome():
    rng = np.random.RandomState(20261020)
    a = BASES[rng.randint(0, 4, 2 * TILE + 4_000)]
    plant(a, TILE - 6, primitive_motif(rng, 20), 400)
    plant(a, 2 * TILE - 40, primitive_motif(rng, 3), 120)
    plant(a, 30_000, primitive_motif(rng, 2), 40)
    b = BASES[rng.randint(0, 4, 3 * TILE + 37)]
    lo, hi = TILE + 20_000, TILE + 23_000
    plant(b, hi, BASES[:1], 14)                   # directly behind the block
    plant(b, lo - 13, BASES[1:2], 12)             # ends one position in front of it
    b[lo:hi] = N
    plant(b, TILE - 40, primitive_motif(rng, 3), 120)
    plant(b, 2 * TILE - 10, primitive_motif(rng, 45), 300)
    plant(b, 10_000, BASES[2:3], 30)              # the clean tile: a homopolymer, a k = 3 and a k = 12 run
    plant(b, 12_000, primitive_motif(rng, 3), 50)
    plant(b, 14_000, primitive_motif(rng, 12), 90)
    plant(b, TILE + 40_000, primitive_motif(rng, 3), 60)   # the mixed tile
    c = BASES[rng.randint(0, 4, 2 * TILE + 64)]
    plant(c, TILE - 2_000, primitive_motif(rng, 7), 3_500)
    d = BASES[rng.randint(0, 4, 2 * TILE + 100)]
    plant(d, TILE - 9_000, primitive_motif(rng, 3), 12_000)
    return [a.tobytes(), b.tobytes(), c.tobytes(), d.tobytes()]


_state = {}


def seqs():
    if "seqs" not in _state:
        _state["seqs"] = genome()
    return _state["seqs"]


def oracle(name):
    """The oracle's rows of a setting, computed once and handed out read-only."""
    if name not in _state:
        rows = cases.oracle_rows(seqs(), SETTINGS[name])
        rows.setflags(write=False)
        _state[name] = rows
    return _state[name]


@pytest.fixture(scope="module")
def loaded():
    assert torch.cuda.is_available()
    import prf_native
    assert prf_native.tile_positions() == TILE
    c = prf_native.Context(0)
    g = c.load(seqs(), KMAX_HINT)
    yield c, g
    g.free()
    c.close()


def by_position(rows):
    import multi_gpu
    rows = np.asarray(rows, dtype=multi_gpu.ROW_DTYPE)
    return rows[np.lexsort((rows["k"], rows["end"], rows["start"], rows["contig"]))]


def test_the_genome_holds_what_it_is_built_around():
    want = oracle("default_1-50")
    rows = {(int(r["contig"]), int(r["start"])): (int(r["end"]), int(r["k"])) for r in want}
    assert rows[(0, TILE - 6)] == (TILE + 394, 20)                        # first examined group in the next tile
    assert rows[(0, 2 * TILE - 40)] == (2 * TILE + 80, 3)                 # across the edge into the tail
    assert rows[(1, TILE - 40)] == (TILE + 80, 3)                         # clean tile -> mixed tile
    assert rows[(1, 2 * TILE - 10)] == (2 * TILE + 290, 45)
    assert rows[(1, TILE + 23_000)] == (TILE + 23_014, 1) and rows[(1, TILE + 20_000 - 13)] == (TILE + 20_000 - 1, 1)
    assert seqs()[1].count(b"N") == 3_000
    end, k = rows[(2, TILE - 2_000)]
    assert k == 7 and 0 < end - TILE <= WINDOW_POST and end == TILE + 1_500             # ends in the window's last 1 536 positions
    assert rows[(3, TILE - 9_000)] == (TILE + 3_000, 3)                  # leaves the window
    only3 = oracle("one_wave_3-3")
    assert len(only3) >= 5 and set(only3["k"].tolist()) == {3}


def test_the_settings_deal_the_waves_as_named():
    import prf_native
    plans = {name: prf_native.plan_describe(*s) for name, s in SETTINGS.items()}
    assert all(p["path"] == "fused" for p in plans.values())
    assert [plans[n]["waves"] for n in ("one_wave_3-3", "two_waves_2-3", "default_1-50")] == [1, 2, 4]
    assert plans["nc80_1-280"]["nc"] == 80 and plans["default_1-50"]["nc"] == 72
    derives = {n: any(t.get("derive") for t in p["tasks"]) for n, p in plans.items()}
    assert derives == {"one_wave_3-3": False, "two_waves_2-3": False, "default_1-50": True, "1-100": True, "nc80_1-280": True,
                       "not_derived_1-50_r5": False}


@pytest.mark.parametrize("name", list(SETTINGS))
def test_fused_generic_oracle(loaded, name):
    import prf_native
    ctx, g = loaded
    settings, want = SETTINGS[name], oracle(name)
    rows, st = g.scan(*settings)
    assert st.path == 1 and int(st.n_hits) == len(want)
    assert np.array_equal(by_position(rows), want)
    again, st2 = g.scan(*settings)                     # the counters' parity and the arrival counter carry over
    assert int(st2.n_hits) == len(want) and np.array_equal(rows, again)
    gen, stg = g.scan(*settings, flags=prf_native.SCAN_FORCE_GENERIC)
    assert stg.path == 0 and np.array_equal(by_position(gen), want)
    print(name, settings, "rows", len(want))


@pytest.mark.parametrize("name", list(SETTINGS))
def test_pipelined_three_times(loaded, name):
    ctx, g = loaded
    settings, want = SETTINGS[name], oracle(name)
    rows, st = g.scan(*settings)                       # sizes the buffers
    assert int(st.n_hits) == len(want)
    pending, counts = [], []
    try:
        pending.append(g.scan_async(*settings))
        pending.append(g.scan_async(*settings))
        counts.append(int(ctx.scan_wait(pending.pop(0)).n_hits))
        pending.append(g.scan_async(*settings))
        counts.append(int(ctx.scan_wait(pending.pop(0)).n_hits))
        counts.append(int(ctx.scan_wait(pending.pop(0)).n_hits))
    finally:
        for s in pending:
            ctx.scan_wait(s)
    assert counts == [len(want)] * 3
    cap = len(want) + 3
    buf = torch.full((cap + 1, 3), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert ctx.last_hits_to_device(buf.data_ptr(), cap, count_row=True) == len(want)
    host = buf.cpu().numpy()
    got = np.ascontiguousarray(host[:len(want)]).view(want.dtype).reshape(-1)
    assert np.array_equal(by_position(got), want)
