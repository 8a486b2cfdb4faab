"""CPU: the deal of the fused kernel's work plan (csrc/plan.cpp) under its table of measured task prices, through
prf_native.plan_describe -- which reports, per task, the price the deal charged and, per plan, the W' of its objective
max(a4, a2 + W') and what a wave with tasks is charged on top -- over the parameter sweep of tests/test_plan.py.

What the kernel relies on, whatever the prices: every motif size is scanned once; the derived k = 1 task stands directly behind the
k = 2 task in the same wave (it pushes the word that task left in LDS); a deriving plan orders a wave's tasks stride-1/2 group tasks,
exact tasks, stride-4 group tasks (the record list's slots go to the small strides: chr22-real's densest tile); the task count and
the image width are within the kernel's limits.  What the new table is for: on the default parameters the busiest wave is no busier
than under the deal it replaces, priced by the same table."""
import itertools

import prf_native

MAX_TASKS, MAX_WAVES, MAX_K = 80, 4, 480          # csrc/prf_plan.h
SWEEP = list(itertools.product((1, 2, 3, 5, 9, 16, 33), (0, 1, 5, 17, 50, 130), (2, 3, 4, 7), (1, 5, 9, 14, 15, 16, 30, 200)))
EXTRA = [(1, 480, 3, 9), (1, 100, 3, 9), (1, 280, 3, 9), (3, 3, 3, 9), (2, 3, 3, 9), (1, 50, 5, 9), (1, 2, 3, 9), (1, 6, 2, 4)]

# The deal of the default parameters (1, 50, 3, 9) before this table: wave -> (kind, k0) in the wave's order
PARENT_DEAL = {0: [(0, 12), (12, 6), (0, 28)],
               1: [(0, 8), (7, 2), (8, 1), (14, 7)],
               2: [(6, 3), (10, 5), (0, 44)],
               3: [(8, 4), (0, 20), (0, 36)]}

_plans = {}


def plan_of(params):
    if params not in _plans:
        _plans[params] = prf_native.plan_describe(*params)
    return _plans[params]


def all_params():
    return [(kmin, kmin + width, r, span) for kmin, width, r, span in SWEEP] + EXTRA


def waves_of(plan):
    waves = [[] for _ in range(plan["waves"])]
    for t in plan["tasks"]:                        # (listed wave by wave, in each wave's order)
        waves[t["wave"]].append(t)
    return waves


def loads_of(plan):
    return [sum(t["price"] for t in w) + plan["first_task"] for w in waves_of(plan)]


def test_every_motif_size_is_scanned_once():
    for params in all_params():
        kmin, kmax, _r, _span = params
        plan = plan_of(params)
        assert plan["path"] == "fused", params
        sizes = []
        for t in plan["tasks"]:
            sizes += [t["k0"]] if t["kind"] else [t["k0"] + i for i in range(8) if (t["valid"] >> i) & 1]
        assert sorted(sizes) == list(range(kmin, kmax + 1)), params


def test_limits_of_the_kernel():
    for params in all_params():
        plan = plan_of(params)
        assert 1 <= len(plan["tasks"]) <= MAX_TASKS and 1 <= plan["waves"] <= MAX_WAVES, params
        assert plan["nc"] in (72, 80), params
        assert all(0 <= t["wave"] < plan["waves"] for t in plan["tasks"]), params
        assert all(w for w in waves_of(plan)), params             # a wave that counts has a task
        assert [t["wave"] for t in plan["tasks"]] == sorted(t["wave"] for t in plan["tasks"]), params
        assert all(t["price"] > 0 for t in plan["tasks"]), params
    assert prf_native.plan_describe(300, MAX_K + 1, 2, 5)["path"] == "generic"


def test_the_derived_task_stands_behind_the_task_that_raises_it():
    n_deriving = 0
    for params in all_params():
        kmin, kmax, r, span = params
        plan = plan_of(params)
        derives = kmin == 1 and kmax >= 2 and span >= 2 * r and max((r - 1) * 2, span - 2) <= 8
        marks = [t["derive"] for t in plan["tasks"]]
        assert sorted(m for m in marks if m) == ([1, 2] if derives else []), params
        if not derives:
            continue
        n_deriving += 1
        for w in waves_of(plan):
            for i, t in enumerate(w):
                if t["derive"] == 2:
                    assert t["kind"] and t["k0"] == 2 and i + 1 < len(w), params
                    assert w[i + 1]["derive"] == 1 and w[i + 1]["kind"] and w[i + 1]["k0"] == 1, params
                assert t["derive"] != 1 or (i > 0 and w[i - 1]["derive"] == 2), params
    assert n_deriving >= 20


def test_a_deriving_plan_orders_a_wave_by_stride():
    def rank(t):
        return 1 if t["kind"] else (0 if t["stride"] < 4 else 2)
    for params in all_params():
        plan = plan_of(params)
        if not any(t["derive"] for t in plan["tasks"]):
            continue
        for w in waves_of(plan):
            ranks = [rank(t) for t in w]
            assert ranks == sorted(ranks), (params, w)


def test_the_default_deal_is_no_busier_than_the_one_it_replaces():
    plan = plan_of((1, 50, 3, 9))
    price = {(t["kind"], t["k0"]): t["price"] for t in plan["tasks"]}
    assert sorted(price) == sorted(kk for w in PARENT_DEAL.values() for kk in w)       # the same thirteen tasks
    parent = sorted(sum(price[kk] for kk in w) + plan["first_task"] for w in PARENT_DEAL.values())
    new = sorted(loads_of(plan))
    print("parent's deal under the new table:", parent, " new deal:", new, " window:", plan["window"])
    assert len(new) == 4 and sum(new) == sum(parent)
    assert new[-1] <= parent[-1]
    # and what the deal minimises is no larger either
    assert max(new[-1], new[1] + plan["window"]) <= max(parent[-1], parent[1] + plan["window"])
